#!/usr/bin/env python3
"""Times icamd_grn_fwd and icamd_grn_bwd (csrc/grn.hip) on the four stage shapes of convnextv2_tiny at batch 256 and 224 x 224
((HW, C') = (3136, 384), (784, 768), (196, 1536), (49, 3072)) and, alternated with them in the same process on the same tensors,

    icamd_bn_apply (read one tensor, write one)   -> the streaming rate of this session, in TB/s: the byte roof
    torch's own expression of GRN                  (forward: the timm formula on the bf16 tensor; backward: autograd of it, followed by
                                                    the GELU backward the fused entry includes)

Algorithmic bytes (every operand of a pass read once, every result written once, the two passes counted as two): forward 6 B per
element (a twice, g once), backward with z1 12 B per element (dg and a twice, z1 once, d z1 once).  roof% = the time those bytes take
at icamd_bn_apply's rate of the same shape, over the measured time.

Method: device events around `reps` back-to-back launches after `warmup` launches, the candidates alternated over `rounds` rounds;
min / median / max over the rounds.  A ratio inside the max / min spread of its own rows is not a measured difference.

    python tools/bench_grn.py [--reps 20] [--rounds 5] > profiles/grn.txt
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclassification_amd import hip  # noqa: E402

N = 256
SHAPES = [("stage0", 3136, 384), ("stage1", 784, 768), ("stage2", 196, 1536), ("stage3", 49, 3072)]
EPS = 1e-6


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


def mmm(ts):
    return min(ts), statistics.median(ts), max(ts)


def grn_torch(a, w, b):
    gx = a.norm(p=2, dim=1, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + EPS)
    return a + torch.addcmul(b, w, a * nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    hip.require_gpu()
    lib = hip.load()
    dev = "cuda"
    s = hip.stream_ptr()
    print(f"# GRN (csrc/grn.hip) on the stage shapes of convnextv2_tiny, batch {N}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.reps} launches per measurement after {args.warmup}, {args.rounds} alternated rounds (min / median / max in us)")
    print("# stage     HW    C'  op     min_us  med_us  max_us  alg_GB/s  stream_TB/s  roof_us  roof%   torch_med  torch/ours")
    for name, HW, C in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        z = torch.randn(N, HW, C, generator=g, device=dev).to(torch.bfloat16)
        a = torch.nn.functional.gelu(z.float()).to(torch.bfloat16)
        dg = (torch.randn(N, HW, C, generator=g, device=dev) * 0.1).to(torch.bfloat16)
        out, dx = torch.empty_like(a), torch.empty_like(a)
        gamma = 0.5 * torch.randn(C, generator=g, device=dev)
        beta = 0.1 * torch.randn(C, generator=g, device=dev)
        gx = torch.empty(N, C, device=dev)
        dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        nbytes = lib.icamd_grn_workspace_bytes(N, HW, C)
        wsp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        # torch's route: bf16 parameters, as autocast would hand them to the module
        wt, bt = gamma.to(torch.bfloat16).requires_grad_(True), beta.to(torch.bfloat16).requires_grad_(True)
        zt = z.clone().requires_grad_(True)

        def chk(rc):
            if rc != 0:
                raise hip.IcamdError(f"{name}: rc {rc}")

        def stream():
            chk(lib.icamd_bn_apply(a.data_ptr(), ones.data_ptr(), zeros.data_ptr(), None, out.data_ptr(), None, a.numel(), C, 0, s))

        def fwd():
            chk(lib.icamd_grn_fwd(a.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), gx.data_ptr(), N, HW, C, EPS,
                                  wsp.data_ptr(), nbytes, s))

        def bwd():
            chk(lib.icamd_grn_bwd(dg.data_ptr(), a.data_ptr(), gx.data_ptr(), gamma.data_ptr(), z.data_ptr(), dx.data_ptr(),
                                  dgam.data_ptr(), dbet.data_ptr(), 0, N, HW, C, EPS, wsp.data_ptr(), nbytes, s))

        def torch_fwd():
            with torch.no_grad():
                grn_torch(a, wt, bt)

        def torch_bwd():      # autograd needs its own forward (gelu -> GRN); torch_fwd_for_bwd is subtracted below
            for t in (zt, wt, bt):
                t.grad = None
            grn_torch(torch.nn.functional.gelu(zt), wt, bt).backward(dg)

        def torch_fwd_for_bwd():
            with torch.no_grad():
                grn_torch(torch.nn.functional.gelu(zt), wt, bt)

        fwd()
        numel = float(N) * HW * C
        ts = {k: [] for k in ("stream", "fwd", "bwd", "torch_fwd", "torch_bwd", "torch_fwd_for_bwd")}
        fns = {"stream": stream, "fwd": fwd, "bwd": bwd, "torch_fwd": torch_fwd, "torch_bwd": torch_bwd,
               "torch_fwd_for_bwd": torch_fwd_for_bwd}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                ts[k].append(timed(fn, args.warmup, args.reps if not k.startswith("torch") else max(args.reps // 4, 3)))
        stream_med = statistics.median(ts["stream"])
        tbs = 4.0 * numel / stream_med / 1e6
        # torch's backward alone: its forward + backward minus the same forward, median of the per-round differences
        t_bwd = [x - y for x, y in zip(ts["torch_bwd"], ts["torch_fwd_for_bwd"])]
        for op, key, per_elem, other in (("fwd", "fwd", 6.0, ts["torch_fwd"]), ("bwd", "bwd", 12.0, t_bwd)):
            lo, med, hi = mmm(ts[key])
            roof_us = per_elem * numel / (tbs * 1e6)
            omed = statistics.median(other)
            print(f"{name:8s} {HW:5d} {C:5d}  {op:4s} {lo:8.1f} {med:7.1f} {hi:7.1f} {per_elem * numel / med / 1e3:9.0f} {tbs:12.2f} "
                  f"{roof_us:8.1f} {100.0 * roof_us / med:6.1f} {omed:11.1f} {omed / med:11.2f}", flush=True)
        del z, a, dg, out, dx, zt, wsp
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
