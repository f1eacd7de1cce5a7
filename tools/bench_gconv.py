#!/usr/bin/env python3
"""Times the grouped 3x3 convolution entries (icamd_gconv3x3_fwd / _dgrad / _wgrad) on the seven conv2 shapes of ResNeXt-50 32x4d
at batch 256 and 224 x 224, and -- in the same process, alternated with them -- the dense emulation of the same operation:
icamd_conv2d_fwd / _dgrad / _wgrad on the same tensors with the filter expanded to a block-diagonal [C][3][3][C].

Method: device events around `reps` back-to-back launches after `warmup` launches, grouped and dense alternated over `rounds`
rounds, the median round reported.  Per shape and operation: microseconds, algorithmic GB/s (x + y + filter bytes) and its
share of 8 TB/s, executed MFMA TFLOP/s (the k-steps the kernel really issues), the dense time and the ratio dense / grouped.

    python tools/bench_gconv.py [--reps 50] [--rounds 3] > profiles/gconv.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclassification_amd import hip  # noqa: E402

N, GROUPS = 256, 32
SHAPES = [("layer1.*", 128, 56, 1), ("layer2.0", 256, 56, 2), ("layer2.1-3", 256, 28, 1), ("layer3.0", 512, 28, 2),
          ("layer3.1-5", 512, 14, 1), ("layer4.0", 1024, 14, 2), ("layer4.1-2", 1024, 7, 1)]
HBM_GBS = 8000.0


def executed_over_algorithmic(cg, op):
    """MFMA work the kernels issue per algorithmic 2 M C 9 Cg (csrc/conv_grouped.hip, header comment)."""
    if cg == 32:
        return 1.0
    block = 16.0 / cg
    return block if op == "wgrad" else block * 10.0 / 9.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    hip.require_gpu()
    lib = hip.load()
    dev = "cuda"
    s = hip.stream_ptr()
    print(f"# grouped 3x3 convolution vs its dense emulation, batch {N}, {GROUPS} groups; {torch.cuda.get_device_name(0)}")
    print(f"# {args.reps} launches per measurement after {args.warmup}, median of {args.rounds} alternated rounds; byte roof {HBM_GBS / 1e3:.0f} TB/s")
    print("# layer        C  Cg grid st op      grouped_us  alg_GB/s  roof%  exec_TFLOP/s   dense_us  dense/grouped")
    worst = None
    for name, C, h, st in SHAPES:
        cg = C // GROUPS
        d = hip.conv_desc(N, h, h, C, C, 3, 3, st, 1)
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(N, h, h, C, generator=g, device=dev).clamp_min(0).to(torch.bfloat16)
        dy = torch.randn(N, d.OH, d.OW, C, generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn(C, 3, 3, cg, generator=g, device=dev) * (2.0 / (9 * cg)) ** 0.5).to(torch.bfloat16)
        wfull = torch.zeros(C, 3, 3, C, dtype=torch.bfloat16, device=dev)
        for k in range(GROUPS):
            wfull[k * cg:(k + 1) * cg, :, :, k * cg:(k + 1) * cg] = w[k * cg:(k + 1) * cg]
        wfull_t = wfull.permute(3, 1, 2, 0).contiguous()
        y = torch.empty(N, d.OH, d.OW, C, dtype=torch.bfloat16, device=dev)
        dx = torch.empty(N, h, h, C, dtype=torch.bfloat16, device=dev)
        rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
        stats = torch.empty(rows, 2, C, device=dev)
        dw = torch.empty(C, 3, 3, cg, device=dev)
        dwfull = torch.empty(C, 3, 3, C, device=dev)
        gneed = lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), GROUPS)
        dneed = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
        gws = torch.empty(gneed, dtype=torch.uint8, device=dev)
        dws = torch.empty(dneed, dtype=torch.uint8, device=dev)
        dref = ctypes.byref(d)

        def chk(rc):
            if rc != 0:
                raise hip.IcamdError(f"{name}: rc {rc}")

        ops = {
            "fwd": (lambda: chk(lib.icamd_gconv3x3_fwd(dref, GROUPS, x.data_ptr(), w.data_ptr(), y.data_ptr(), stats.data_ptr(), s)),
                    lambda: chk(lib.icamd_conv2d_fwd(dref, x.data_ptr(), wfull.data_ptr(), y.data_ptr(), None, None, stats.data_ptr(), s))),
            "dgrad": (lambda: chk(lib.icamd_gconv3x3_dgrad(dref, GROUPS, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), s)),
                      lambda: chk(lib.icamd_conv2d_dgrad(dref, dy.data_ptr(), wfull_t.data_ptr(), dx.data_ptr(), None, None, s))),
            "wgrad": (lambda: chk(lib.icamd_gconv3x3_wgrad(dref, GROUPS, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, gws.data_ptr(),
                                                           gneed, s)),
                      lambda: chk(lib.icamd_conv2d_wgrad(dref, x.data_ptr(), dy.data_ptr(), dwfull.data_ptr(), 0, dws.data_ptr(),
                                                         dneed, s))),
        }
        M = N * d.OH * d.OW
        act_bytes = 2.0 * (N * h * h * C + M * C)
        flops = 2.0 * M * C * 9 * cg
        for op, (grouped, dense) in ops.items():
            tg, td = [], []
            for _ in range(args.rounds):
                tg.append(timed(grouped, args.warmup, args.reps))
                td.append(timed(dense, args.warmup, args.reps))
            ug, ud = statistics.median(tg), statistics.median(td)
            nbytes = act_bytes + (4.0 if op == "wgrad" else 2.0) * C * 9 * cg
            gbs = nbytes / ug / 1e3
            tfl = flops * executed_over_algorithmic(cg, op) / ug / 1e6
            ratio = ud / ug
            if worst is None or ratio < worst[0]:
                worst = (ratio, name, op)
            print(f"{name:11s} {C:4d} {cg:3d} {h:3d}  {st}  {op:6s} {ug:10.1f} {gbs:9.0f} {100.0 * gbs / HBM_GBS:6.1f} {tfl:13.1f} {ud:10.1f} "
                  f"{ratio:10.2f}")
        del x, dy, w, wfull, wfull_t, y, dx, dw, dwfull, gws, dws
        torch.cuda.empty_cache()
    print(f"# smallest dense / grouped ratio: {worst[0]:.2f} ({worst[1]} {worst[2]}); the gate is >= 1.00 on every line")
    return 0 if worst[0] >= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
