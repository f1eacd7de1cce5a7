#!/usr/bin/env python3
"""Times a Swin model on the gfx950 kernels (default: Swin-T, batch 256 at 224 x 224; --arch swin_base_patch4_window12_384 --hw 384
--batch 64 for the window-12 model):

  * the whole training step through engine.train_one_epoch on synthetic data with bench.py's recipe (AdamW, label smoothing 0.1,
    1000 classes, --steps after --warmup);
  * the window attention kernels (csrc/window_attention.hip, csrc/window_attention_w12.hip) alone at the model's stage shapes
    (Swin-T: 56 / 28 / 14 / 7 tokens per side, 3 / 6 / 12 / 24 heads; odd blocks' shift 3, none at 7), forward and backward, and patch
    merging + LayerNorm at its shapes,
    beside two yardsticks taken in the same session:
      - a byte roof: algorithmic bytes (every operand read once, every result written once) divided by the streaming bandwidth
        tools/bench_bn.py reports for icamd_bn_apply (read y, write a) -- it is run first, as a child process;
      - torch's own route on the same tensors: roll, window-partition copies, scaled_dot_product_attention with bias + mask as
        attn_mask, the reverse copies and the roll back (backward: autograd of exactly that).

Method: device events around `reps` back-to-back launches after `warmup` launches, `rounds` rounds, the median round reported.

    python tools/bench_swin.py [--steps 20] [--warmup 5] [--batch 256] > profiles/swin.txt
    python tools/bench_swin.py --arch swin_base_patch4_window12_384 --hw 384 --batch 64 > profiles/swin_w12.txt
"""
import argparse
import contextlib
import io
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclassification_amd import hip  # noqa: E402
from imageclassification_amd.swin import config, relative_position_index, stage_plan, window_geometry  # noqa: E402

D = 32


def stages_of(arch, hw):
    """[(tokens per side, heads, channels, window, shift of the odd blocks)] per stage; Swin-T at 224: (56, 3, 96, 7, 3) ..."""
    embed, _, heads, _ = config(arch)
    return [(res, heads[i], embed << i, ws, shift) for i, (res, ws, shift) in enumerate(stage_plan(arch, hw))]


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us


def median_of(fn, args):
    return statistics.median(timed(fn, args.kwarmup, args.reps) for _ in range(args.rounds))


def stream_roof():
    """TB/s of icamd_bn_apply (read y, write a) from tools/bench_bn.py, run now."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bn.py")], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError("tools/bench_bn.py failed:\n" + out.stdout + out.stderr)
    print("# tools/bench_bn.py:")
    for line in out.stdout.splitlines():
        print("#   " + line)
    m = re.search(r"bn_apply \(read y, write a\): [\d.]+ us, ([\d.]+) TB/s", out.stdout)
    return float(m.group(1))


def window_partition(x, ws):
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws * ws, C)


def window_reverse(w, ws, H, W):
    C = w.shape[-1]
    return w.view(-1, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, H, W, C)


def torch_route(qkv, attn_mask, B, res, H, ws, shift):
    """timm's data movement around torch's fused attention; qkv [B, res, res, 3*H*D] bf16, attn_mask [nW or 1, H, T, T] bf16"""
    sh = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift else qkv
    xw = window_partition(sh, ws)
    B_, T, _ = xw.shape
    q, k, v = xw.reshape(B_, T, 3, H, D).permute(2, 0, 3, 1, 4)
    nW = attn_mask.shape[0]
    o = torch.nn.functional.scaled_dot_product_attention(q.reshape(B_ // nW, nW, H, T, D), k.reshape(B_ // nW, nW, H, T, D),
                                                         v.reshape(B_ // nW, nW, H, T, D), attn_mask=attn_mask.unsqueeze(0))
    o = o.reshape(B_, H, T, D).transpose(1, 2).reshape(B_, T, H * D)
    o = window_reverse(o, ws, res, res)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift else o


def step_time(args):
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.swin import SwinTransformer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount, cosine_scheduler
    dev = torch.device("cuda")
    C, B = 1000, args.batch
    net = SwinTransformer(args.arch, C, img_size=args.hw, seed=88)          # drop_path_rate: the class default (0.1)
    opt = create_optimizer("adamw", 1e-3, 5e-4, net)
    crit = LabelSmoothingCrossEntropy(0.1)
    total = args.warmup + args.steps
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        lr = cosine_scheduler(1e-3, 1e-6, 1, total, warmup_epochs=0)
        wd = cosine_scheduler(5e-4, 5e-6, 1, total)
    g = torch.Generator(device=dev).manual_seed(88)
    pool = [(torch.randn(B, 3, args.hw, args.hw, generator=g, device=dev), torch.randint(0, C, (B,), generator=g, device=dev)) for _ in range(2)]

    def run(n, start):
        loader = [pool[i % 2] for i in range(n)]
        with contextlib.redirect_stdout(sink):
            return train_one_epoch(net, crit, loader, opt, dev, 0, NativeScalerWithGradNormCount(), None, None, None, start_steps=start,
                                   lr_schedule_values=lr, wd_schedule_values=wd, num_training_steps_per_epoch=n, update_freq=1,
                                   use_amp=True, num_classes=C)

    run(args.warmup, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = run(args.steps, args.warmup)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{args.arch} training step, batch {B}, drop_path 0.1: {1e3 * dt / args.steps:.2f} ms/step, "
          f"{B * args.steps / dt:.0f} img/s over {args.steps} steps after {args.warmup} (loss {stats['loss']:.4f})")
    del net, opt, pool
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--arch", default="swin_tiny_patch4_window7_224")
    ap.add_argument("--hw", type=int, default=224, help="input height = width")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kwarmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="kernel table only")
    args = ap.parse_args()
    hip.require_gpu()
    roof = stream_roof()
    lib = hip.load()
    dev = "cuda"
    s = hip.stream_ptr()
    B = args.batch
    stages = stages_of(args.arch, args.hw)
    print(f"# {args.arch} at {args.hw} x {args.hw}, batch {B}; {torch.cuda.get_device_name(0)}")
    if not args.no_step:
        step_time(args)
    print(f"# kernels: {args.reps} launches per measurement after {args.kwarmup}, median of {args.rounds} rounds; byte roof = "
          f"algorithmic bytes / {roof:.2f} TB/s")

    def chk(rc):
        if rc != 0:
            raise hip.IcamdError(f"rc {rc}")

    print("# window attention              op          us  alg_GB/s   roof_us  roof%   torch_us torch/ours")
    slower = []
    for res, H, _, ws, odd_shift in stages:
        T = ws * ws
        for shift in ((0, odd_shift) if odd_shift else (0,)):
            g = torch.Generator(device=dev).manual_seed(1)
            qkv = torch.randn(B, res, res, 3 * H * D, generator=g, device=dev).to(torch.bfloat16)
            dout = torch.randn(B, res, res, H * D, generator=g, device=dev).to(torch.bfloat16)
            table = torch.randn((2 * ws - 1) ** 2, H, generator=g, device=dev) * 0.5
            bias = torch.empty(H, T, T, device=dev)
            chk(lib.icamd_relpos_bias_gather(table.data_ptr(), bias.data_ptr(), H, ws, s))
            nwin = B * (res // ws) ** 2
            out = torch.empty(B, res, res, H * D, dtype=torch.bfloat16, device=dev)
            lse = torch.empty(nwin * H * T, device=dev)
            dqkv = torch.empty_like(qkv)
            dbias = torch.empty(H, T, T, device=dev)
            wsb = lib.icamd_window_attention_bwd_workspace_bytes(B, res, res, H, ws)
            wsp = torch.empty(wsb, dtype=torch.uint8, device=dev)

            def fwd():
                chk(lib.icamd_window_attention_fwd(qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), lse.data_ptr(), B, res, res, H, D,
                                                   ws, shift, D ** -0.5, s))

            def bwd():
                chk(lib.icamd_window_attention_bwd(qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                                   dqkv.data_ptr(), dbias.data_ptr(), 0, wsp.data_ptr(), wsb, B, res, res, H, D, ws,
                                                   shift, D ** -0.5, s))

            # torch's route: bias + region mask as one additive attn_mask [nW, H, T, T]
            win, slot, region = window_geometry(res, res, ws, shift)
            nW = (res // ws) ** 2
            rw = torch.zeros(nW, T, dtype=torch.int64)
            rw[win, slot] = region
            mask = (rw.unsqueeze(1) != rw.unsqueeze(2)).float() * -100.0
            idx = relative_position_index(ws).to(dev)
            tbias = table[idx.view(-1)].view(T, T, H).permute(2, 0, 1)
            am = (tbias.unsqueeze(0) + mask.to(dev).unsqueeze(1)).to(torch.bfloat16).contiguous()
            if shift == 0:
                am = am[:1].contiguous()
            qkv_t = qkv.clone().requires_grad_(True)

            def t_fwd():
                with torch.no_grad():
                    torch_route(qkv, am, B, res, H, ws, shift)

            def t_fwd_bwd():
                qkv_t.grad = None
                torch_route(qkv_t, am, B, res, H, ws, shift).backward(dout)

            tokens = float(B) * res * res
            uf, ub = median_of(fwd, args), median_of(bwd, args)
            tf = median_of(t_fwd, args)
            tb = median_of(t_fwd_bwd, args) - tf
            name = f"[{B},{res},{res}] {H} heads shift {shift}"
            for op, us, nbytes, other in (("fwd", uf, 8.0 * tokens * H * D + 4.0 * nwin * H * T, tf),
                                          ("bwd", ub, 16.0 * tokens * H * D + 4.0 * nwin * H * T, tb)):
                roof_us = nbytes / (roof * 1e6)
                print(f"{name:31s} {op:4s} {us:10.1f} {nbytes / us / 1e3:9.0f} {roof_us:9.1f} {100.0 * roof_us / us:6.1f} {other:10.1f} "
                      f"{other / us:8.2f}")
                if other < us:
                    slower.append(f"{name} {op}")
            del qkv, dout, out, lse, dqkv, wsp, qkv_t, am
            torch.cuda.empty_cache()
    if slower:
        print("# SLOWER than torch's route at: " + "; ".join(slower))
    else:
        print("# faster than torch's route at every shape above (torch's backward = its forward + backward minus its forward)")

    print("# patch merging + LayerNorm     op          us  alg_GB/s   roof_us  roof%")
    for res, _, C, _, _ in stages[:-1]:
        g = torch.Generator(device=dev).manual_seed(2)
        x = torch.randn(B, res, res, C, generator=g, device=dev).to(torch.bfloat16)
        rows = B * (res // 2) ** 2
        gamma, beta = torch.rand(4 * C, generator=g, device=dev) + 0.5, torch.randn(4 * C, generator=g, device=dev)
        y = torch.empty(rows, 4 * C, dtype=torch.bfloat16, device=dev)
        dy = torch.randn(rows, 4 * C, generator=g, device=dev).to(torch.bfloat16)
        mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        dx = torch.empty_like(x)
        dg, db = torch.empty(4 * C, device=dev), torch.empty(4 * C, device=dev)
        wsb = lib.icamd_patch_merge_ln_bwd_workspace_bytes(B, res, res, C)
        wsp = torch.empty(wsb, dtype=torch.uint8, device=dev)
        uf = median_of(lambda: chk(lib.icamd_patch_merge_ln_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                                                mean.data_ptr(), rstd.data_ptr(), B, res, res, C, 1e-5, s)), args)
        ub = median_of(lambda: chk(lib.icamd_patch_merge_ln_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                                gamma.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), B, res,
                                                                res, C, 0, wsp.data_ptr(), wsb, s)), args)
        full = 2.0 * B * res * res * C
        for op, us, nbytes in (("fwd", uf, 2 * full), ("bwd", ub, 3 * full)):
            roof_us = nbytes / (roof * 1e6)
            print(f"{f'[{B},{res},{res},{C}] -> 4C = {4 * C}':31s} {op:4s} {us:10.1f} {nbytes / us / 1e3:9.0f} {roof_us:9.1f} "
                  f"{100.0 * roof_us / us:6.1f}")
        del x, y, dy, dx, wsp
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
