#!/usr/bin/env python3
"""Times the EfficientNet kernels (csrc/dwconv5x5.hip) and the training step on one GPU, batch 256.

Depthwise 5x5: the nine 5x5 layers of efficientnet_b0 at 224 x 224 are six shapes -- (C, H, stride) = (144, 56, 2), (240, 28, 1),
(480, 14, 1), (672, 14, 1) twice, (672, 14, 2), (1152, 7, 1) three times.  Per shape, alternated in the same process on the same tensors:

    stream     icamd_bn_apply over the input tensor (read one tensor, write one): the streaming rate of this session, the byte roof
    fwd        icamd_dwconv5_fwd with statistics, as the model calls it;  dgrad, wgrad: icamd_dwconv5_dgrad / _wgrad
    torch      F.conv2d(groups=C, padding=2) on the channels-last bf16 tensor; backward: autograd.grad for input and filter (forward +
               backward minus forward), to be set against dgrad + wgrad

Squeeze-and-excitation: the sixteen sites of efficientnet_b0 are eleven (C, H, rd) shapes.  fwd = icamd_bn_silu_squeeze +
icamd_se_excite_silu_fwd + the gated icamd_bn_apply_silu; bwd = icamd_se_silu_bwd_reduce + icamd_se_excite_silu_bwd + icamd_bn_bwd_silu.
torch: F.batch_norm (batch statistics) + F.silu + mean + two 1x1 convolutions + sigmoid + multiply, and autograd.grad of it for y and
the six parameters (forward + backward minus forward).

Algorithmic bytes: depthwise forward / data gradient 2 B per element of input and output (statistics rows besides); weight gradient
input + dy read; SE forward two reads of y2 and one write, SE backward three reads of (dout, y2) and one write of dy2.  roof% = the
time those bytes take at `stream`'s rate over the measured median.  Medians of `rounds` alternated rounds with min / max: a ratio
inside the spread of its own rows is not a measured difference.

Step: efficientnet_b0 and efficientnet_b1 alternated twice with resnet50 through engine.train_one_epoch (AdamW, label smoothing,
synthetic data resident on the device), ms/step and img/s.

    python tools/bench_efficientnet.py [--reps 20] [--rounds 5] [--steps 12] > profiles/efficientnet.txt
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclassification_amd import hip  # noqa: E402
from imageclassification_amd.efficientnet import block_plan  # noqa: E402

N = 256


def sites():
    """({(C, H, stride): count} of the 5x5 layers, {(C, H_out, rd): count} of the SE sites) of efficientnet_b0 at 224 x 224"""
    dw, se, h = {}, {}, 112
    for _, kind, k, cin, mid, cout, stride, rd in block_plan("efficientnet_b0")[1]:
        if k == 5:
            dw[(mid, h, stride)] = dw.get((mid, h, stride), 0) + 1
        h = (h - 1) // stride + 1
        se[(mid, h, rd)] = se.get((mid, h, rd), 0) + 1
    return dw, se


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


def chk(rc, what):
    if rc != 0:
        raise hip.IcamdError(f"{what}: rc {rc}")


class DwCase:
    """the tensors of one (C, H, stride) and the launches on them"""

    def __init__(self, lib, C, hw, stride):
        dev, self.lib, self.C, self.hw, self.stride, self.s = "cuda", lib, C, hw, stride, hip.stream_ptr()
        oh = (hw - 1) // stride + 1
        g = torch.Generator(device=dev).manual_seed(1)
        self.x = torch.randn(N, hw, hw, C, generator=g, device=dev).to(torch.bfloat16)
        self.a = torch.empty_like(self.x)
        self.dy = (torch.randn(N, oh, oh, C, generator=g, device=dev) * 0.1).to(torch.bfloat16)
        self.w = (torch.randn(5, 5, C, generator=g, device=dev) * 0.2).to(torch.bfloat16)
        self.y = torch.empty(N, oh, oh, C, dtype=torch.bfloat16, device=dev)
        self.dx = torch.empty_like(self.x)
        self.dw = torch.empty(5, 5, C, device=dev)
        self.rows = lib.icamd_dwconv5_stats_rows(N, hw, hw, C, stride)
        self.stats = torch.empty(self.rows, 2, C, device=dev)
        self.wsb = lib.icamd_dwconv5_wgrad_workspace_bytes(N, hw, hw, C, stride)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.ones, self.zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        self.in_el, self.out_el = float(self.x.numel()), float(self.y.numel())
        self.xt = self.x.permute(0, 3, 1, 2).requires_grad_(True)      # NCHW views of the same channels-last memory
        self.dyt = self.dy.permute(0, 3, 1, 2)
        self.wt = self.w.permute(2, 0, 1).reshape(C, 1, 5, 5).contiguous().requires_grad_(True)

    def stream(self):
        chk(self.lib.icamd_bn_apply(self.x.data_ptr(), self.ones.data_ptr(), self.zeros.data_ptr(), None, self.a.data_ptr(), None,
                                    self.x.numel(), self.C, 0, self.s), "stream")

    def fwd(self):
        chk(self.lib.icamd_dwconv5_fwd(self.x.data_ptr(), self.w.data_ptr(), self.y.data_ptr(), self.stats.data_ptr(), N, self.hw, self.hw,
                                       self.C, self.stride, self.s), "fwd")

    def dgrad(self):
        chk(self.lib.icamd_dwconv5_dgrad(self.dy.data_ptr(), self.w.data_ptr(), self.dx.data_ptr(), N, self.hw, self.hw, self.C,
                                         self.stride, self.s), "dgrad")

    def wgrad(self):
        chk(self.lib.icamd_dwconv5_wgrad(self.x.data_ptr(), self.dy.data_ptr(), self.dw.data_ptr(), 0, self.ws.data_ptr(), self.wsb, N,
                                         self.hw, self.hw, self.C, self.stride, self.s), "wgrad")

    def torch_fwd(self):
        with torch.no_grad():
            F.conv2d(self.xt, self.wt, None, self.stride, 2, 1, self.C)

    def torch_fwd_bwd(self):      # autograd needs its own forward; torch_fwd is subtracted by the caller
        torch.autograd.grad(F.conv2d(self.xt, self.wt, None, self.stride, 2, 1, self.C), (self.xt, self.wt), self.dyt)


class SeCase:
    """the tensors of one SE site (C, H, rd) and the launches on them"""

    def __init__(self, lib, C, hw, rd):
        dev, self.lib, self.C, self.HW, self.rd, self.s = "cuda", lib, C, hw * hw, rd, hip.stream_ptr()
        g = torch.Generator(device=dev).manual_seed(2)
        f = lambda *shape, scale=1.0: torch.randn(*shape, generator=g, device=dev) * scale      # noqa: E731
        self.y = f(N, hw, hw, C).to(torch.bfloat16)
        self.dout = f(N, hw, hw, C, scale=0.1).to(torch.bfloat16)
        self.out, self.dy = torch.empty_like(self.y), torch.empty_like(self.y)
        self.scale, self.shift = 1.0 + 0.1 * f(C), 0.1 * f(C)
        self.mean, self.invstd = 0.1 * f(C), 1.0 + 0.1 * f(C).abs()
        self.w1, self.b1, self.w2, self.b2 = f(rd, C, scale=(2.0 / rd) ** 0.5), 0.1 * f(rd), f(C, rd, scale=(2.0 / C) ** 0.5), 0.1 * f(C)
        self.asum, self.sv, self.e, self.de, self.dsn = (torch.empty(N, C, device=dev) for _ in range(5))
        self.h = torch.empty(N, rd, device=dev)
        self.grads = [torch.empty_like(t) for t in (self.w1, self.b1, self.w2, self.b2, self.scale, self.shift)]
        self.sqb = lib.icamd_bn_silu_squeeze_workspace_bytes(N, self.HW, C)
        self.sq = torch.empty(self.sqb, dtype=torch.uint8, device=dev)
        self.bwb = lib.icamd_bn_bwd_silu_workspace_bytes(N, self.HW, C)
        self.bw = torch.zeros(self.bwb, dtype=torch.uint8, device=dev)
        self.ones, self.zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        self.el = float(self.y.numel())
        self.yt = self.y.permute(0, 3, 1, 2).requires_grad_(True)
        self.dt = self.dout.permute(0, 3, 1, 2)
        self.params = [t.to(torch.bfloat16).requires_grad_(True) for t in (self.scale, self.shift, self.w1.reshape(rd, C, 1, 1), self.b1,
                                                                          self.w2.reshape(C, rd, 1, 1), self.b2)]

    def stream(self):
        chk(self.lib.icamd_bn_apply(self.y.data_ptr(), self.ones.data_ptr(), self.zeros.data_ptr(), None, self.out.data_ptr(), None,
                                    self.y.numel(), self.C, 0, self.s), "stream")

    def fwd(self):
        lib, p, C, HW, rd, s = self.lib, hip.ptr, self.C, self.HW, self.rd, self.s
        chk(lib.icamd_bn_silu_squeeze(p(self.y), p(self.scale), p(self.shift), p(self.asum), N, HW, C, p(self.sq), self.sqb, s), "squeeze")
        chk(lib.icamd_se_excite_silu_fwd(p(self.asum), 1.0 / HW, p(self.w1), p(self.b1), p(self.w2), p(self.b2), p(self.sv), p(self.h),
                                         p(self.e), N, C, rd, s), "excite")
        chk(lib.icamd_bn_apply_silu(p(self.y), p(self.scale), p(self.shift), p(self.e), p(self.out), N, HW, C, s), "apply")

    def bwd(self):
        lib, p, C, HW, rd, s = self.lib, hip.ptr, self.C, self.HW, self.rd, self.s
        chk(lib.icamd_se_silu_bwd_reduce(p(self.dout), p(self.y), p(self.scale), p(self.shift), p(self.de), N, HW, C, p(self.sq), self.sqb,
                                         s), "gate gradient")
        g = self.grads
        chk(lib.icamd_se_excite_silu_bwd(p(self.de), p(self.sv), p(self.h), p(self.e), p(self.w1), p(self.w2), p(g[0]), p(g[1]), p(g[2]),
                                         p(g[3]), p(self.dsn), N, C, rd, 1.0 / HW, 0, s), "excite bwd")
        chk(lib.icamd_bn_bwd_silu(p(self.dout), p(self.y), p(self.mean), p(self.invstd), p(self.scale), p(self.shift), p(self.e),
                                  p(self.dsn), p(g[4]), p(g[5]), p(self.dy), N, HW, C, 0, p(self.bw), self.bwb, s), "bn bwd")

    def excite_bwd(self):      # the [N, C]-sized part of bwd on its own
        lib, p, g = self.lib, hip.ptr, self.grads
        chk(lib.icamd_se_excite_silu_bwd(p(self.de), p(self.sv), p(self.h), p(self.e), p(self.w1), p(self.w2), p(g[0]), p(g[1]), p(g[2]),
                                         p(g[3]), p(self.dsn), N, self.C, self.rd, 1.0 / self.HW, 0, self.s), "excite bwd")

    def _torch(self):
        gamma, beta, w1, b1, w2, b2 = self.params
        a = F.silu(F.batch_norm(self.yt, None, None, gamma, beta, True, 0.0, 1e-5))
        return a * torch.sigmoid(F.conv2d(F.silu(F.conv2d(a.mean((2, 3), keepdim=True), w1, b1)), w2, b2))

    def torch_fwd(self):
        with torch.no_grad():
            self._torch()

    def torch_fwd_bwd(self):
        torch.autograd.grad(self._torch(), [self.yt] + self.params, self.dt)


def rounds_of(case, names, args):
    ts = {k: [] for k in names}
    for _ in range(args.rounds):
        for k in names:
            reps = args.reps if not k.startswith("torch") else max(args.reps // 4, 3)
            ts[k].append(timed(getattr(case, k), args.warmup, reps))
    return ts


def row(label, op, t, tbs, nbytes, t_torch):
    lo, med, hi = min(t), statistics.median(t), max(t)
    line = f"{label}  {op:10s} {lo:7.1f} {med:7.1f} {hi:7.1f} {tbs:12.2f} "
    if nbytes is not None:
        roof_us = nbytes / (tbs * 1e6)
        line += f"{roof_us:8.1f} {100.0 * roof_us / med:6.1f} "
    else:
        line += f"{'-':>8s} {'-':>6s} "
    line += f"{t_torch:9.1f} {t_torch / med:11.2f}" if t_torch is not None else f"{'-':>9s} {'-':>11s}"
    print(line, flush=True)
    return t_torch is not None and t_torch < med


def kernels(lib, args):
    dw, se = sites()
    slower = []
    print(f"# kernels: {args.reps} launches per measurement after {args.warmup}, {args.rounds} alternated rounds (min / median / max in "
          "us); torch: a quarter of the launches")
    print("# depthwise 5x5; the `bwd` row = dgrad + wgrad against autograd.grad for input + filter (forward + backward minus forward)")
    print("#    C    H  s  n  op            min_us  med_us  max_us  stream_TB/s  roof_us  roof%  torch_us  torch/ours")
    for (C, hw, stride), count in dw.items():
        case = DwCase(lib, C, hw, stride)
        ts = rounds_of(case, ["stream", "fwd", "dgrad", "wgrad", "torch_fwd", "torch_fwd_bwd"], args)
        tbs = 4.0 * case.in_el / statistics.median(ts["stream"]) / 1e6
        io_b = 2 * case.in_el + 2 * case.out_el
        ts["bwd"] = [a + b for a, b in zip(ts["dgrad"], ts["wgrad"])]
        t_bwd = statistics.median([a - b for a, b in zip(ts["torch_fwd_bwd"], ts["torch_fwd"])])
        label = f"{C:6d} {hw:4d} {stride:2d} {count:2d}"
        for op, nb, tt in (("fwd", io_b + 8.0 * case.rows * C, statistics.median(ts["torch_fwd"])), ("dgrad", io_b, None),
                           ("wgrad", io_b, None), ("bwd", None, t_bwd)):
            if row(label, op, ts[op], tbs, nb, tt):
                slower.append(f"dwconv5 {op} ({C}, {hw}, {stride})")
        del case
        torch.cuda.empty_cache()
    print("# squeeze-and-excitation behind BatchNorm + SiLU; `excite_bwd` is the [N, C]-sized part of bwd")
    print("#    C    H  rd n  op            min_us  med_us  max_us  stream_TB/s  roof_us  roof%  torch_us  torch/ours")
    for (C, hw, rd), count in se.items():
        case = SeCase(lib, C, hw, rd)
        ts = rounds_of(case, ["stream", "fwd", "bwd", "excite_bwd", "torch_fwd", "torch_fwd_bwd"], args)
        tbs = 4.0 * case.el / statistics.median(ts["stream"]) / 1e6
        t_bwd = statistics.median([a - b for a, b in zip(ts["torch_fwd_bwd"], ts["torch_fwd"])])
        label = f"{C:6d} {hw:4d} {rd:2d} {count:2d}"
        for op, nb, tt in (("fwd", 6 * case.el, statistics.median(ts["torch_fwd"])), ("bwd", 14 * case.el, t_bwd), ("excite_bwd", None, None)):
            if row(label, op, ts[op], tbs, nb, tt):
                slower.append(f"SE {op} ({C}, {hw}, {rd})")
        del case
        torch.cuda.empty_cache()
    print("# slower than torch's route (median against median): " + ("; ".join(slower) if slower else "none"))


def step_times(args):
    from imageclassification_amd.efficientnet import EfficientNet
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.nets import ResNet
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount, cosine_scheduler
    dev = torch.device("cuda")
    C, B = 1000, N
    g = torch.Generator(device=dev).manual_seed(88)
    pool = [(torch.randn(B, 3, 224, 224, generator=g, device=dev), torch.randint(0, C, (B,), generator=g, device=dev)) for _ in range(2)]
    crit = LabelSmoothingCrossEntropy(0.1)
    total = args.step_warmup + args.steps
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        lr = cosine_scheduler(1e-3, 1e-6, 1, total, warmup_epochs=0)
        wd = cosine_scheduler(5e-4, 5e-6, 1, total)
    print(f"# training step, batch {B} at 224 x 224, 1000 classes: {args.steps} steps after {args.step_warmup}, AdamW, label smoothing 0.1")
    for rnd in range(2):
        for arch in ("efficientnet_b0", "resnet50", "efficientnet_b1", "resnet50"):
            net = EfficientNet(arch, C, seed=88) if arch.startswith("efficientnet") else ResNet(arch, C, seed=88)
            opt = create_optimizer("adamw", 1e-3, 5e-4, net)

            def run(n, start):
                loader = [pool[i % 2] for i in range(n)]
                with contextlib.redirect_stdout(sink):
                    return train_one_epoch(net, crit, loader, opt, dev, 0, NativeScalerWithGradNormCount(), None, None, None,
                                           start_steps=start, lr_schedule_values=lr, wd_schedule_values=wd,
                                           num_training_steps_per_epoch=n, update_freq=1, use_amp=True, num_classes=C)

            run(args.step_warmup, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = run(args.steps, args.step_warmup)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"round {rnd}  {arch:16s} {1e3 * dt / args.steps:8.2f} ms/step {B * args.steps / dt:8.0f} img/s  (loss {stats['loss']:.4f})",
                  flush=True)
            del net, opt
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--step-warmup", type=int, default=4)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    args = ap.parse_args()
    hip.require_gpu()
    lib = hip.load()
    print(f"# EfficientNet (csrc/dwconv5x5.hip, imageclassification_amd/efficientnet.py), batch {N}; {torch.cuda.get_device_name(0)}")
    kernels(lib, args)
    if not args.no_step:
        step_times(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
