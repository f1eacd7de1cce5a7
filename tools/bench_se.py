#!/usr/bin/env python3
"""Times the squeeze-and-excitation tail (csrc/se_ops.hip) at the four tail shapes of SE-ResNet-50 at batch 256 and 224 x 224
(C / HW = 256 / 3136, 512 / 784, 1024 / 196, 2048 / 49) and, alternated with it in the same process on the same tensors, the
plain BatchNorm tail it stands beside:

    icamd_se_squeeze                         (no counterpart: the one pass SE adds; algorithmic bytes and share of the byte roof)
    icamd_se_excite_fwd                      ([N, C]-sized; time only)
    icamd_se_bn_apply     vs  icamd_bn_apply     (residual + ReLU + mask bits; + 4 N C bytes of gate)
    icamd_se_bn_bwd       vs  icamd_bn_bwd       (mask bits, relu = 1; + the [N, C] tables and the excitation backward)

Method: device events around `reps` back-to-back launches after `warmup` launches, SE and plain alternated over `rounds` rounds;
min / median / max over the rounds.  The ratio SE / plain is the ratio of the medians and is printed next to the plain kernel's own
max / min spread: a ratio inside that spread is not a measured difference.

    python tools/bench_se.py [--reps 20] [--rounds 7] > profiles/se_tail.txt
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
SHAPES = [("layer1", 256, 3136), ("layer2", 512, 784), ("layer3", 1024, 196), ("layer4", 2048, 49)]
HBM_GBS = 8000.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    hip.require_gpu()
    lib = hip.load()
    dev = "cuda"
    s = hip.stream_ptr()
    print(f"# SE tail vs the plain BatchNorm tail, batch {N}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.reps} launches per measurement after {args.warmup}, {args.rounds} alternated rounds (min / median / max in us); "
          f"byte roof {HBM_GBS / 1e3:.0f} TB/s")
    print("# layer     C    HW  op        se_min  se_med  se_max  alg_GB/s  roof%   plain_min plain_med plain_max  se/plain  plain max/min")
    for name, C, HW in SHAPES:
        rd = C // 16
        g = torch.Generator(device=dev).manual_seed(1)
        y = torch.randn(N, HW, C, generator=g, device=dev).to(torch.bfloat16)
        res = torch.randn(N, HW, C, generator=g, device=dev).to(torch.bfloat16)
        dout = (torch.randn(N, HW, C, generator=g, device=dev) * 0.1).to(torch.bfloat16)
        out, dy = torch.empty_like(y), torch.empty_like(y)
        bits = torch.zeros(y.numel() // 8, dtype=torch.uint8, device=dev)
        yf = y.float()
        mean = yf.mean((0, 1))
        invstd = 1.0 / torch.sqrt(yf.var((0, 1), unbiased=False) + 1e-5)
        del yf
        gamma = torch.rand(C, generator=g, device=dev) + 0.5
        beta = torch.randn(C, generator=g, device=dev) * 0.3
        scale = gamma * invstd
        shift = beta - mean * scale
        w1 = torch.randn(rd, C, generator=g, device=dev) * (1.5 / C ** 0.5)
        b1 = torch.randn(rd, generator=g, device=dev) * 0.3 + 0.3
        w2 = torch.randn(C, rd, generator=g, device=dev) * (1.0 / rd ** 0.5)
        b2 = torch.randn(C, generator=g, device=dev)
        ysum, sv, ev = (torch.empty(N, C, device=dev) for _ in range(3))
        hv = torch.empty(N, rd, device=dev)
        grads = [torch.zeros(n, device=dev) for n in (C, C, rd * C, rd, C * rd, C)]
        dg2, db2 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        sq_b = lib.icamd_se_squeeze_workspace_bytes(N, HW, C)
        se_b = lib.icamd_se_bn_bwd_workspace_bytes(N, HW, C)
        bn_b = lib.icamd_bn_bwd_workspace_bytes(N * HW, C)
        sq_ws = torch.empty(sq_b, dtype=torch.uint8, device=dev)
        se_ws = torch.empty(se_b, dtype=torch.uint8, device=dev)
        bn_ws = torch.zeros(bn_b, dtype=torch.uint8, device=dev)

        def chk(rc):
            if rc != 0:
                raise hip.IcamdError(f"{name}: rc {rc}")

        def squeeze():
            chk(lib.icamd_se_squeeze(y.data_ptr(), ysum.data_ptr(), N, HW, C, sq_ws.data_ptr(), sq_b, s))

        def excite():
            chk(lib.icamd_se_excite_fwd(ysum.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1.0 / HW, w1.data_ptr(), b1.data_ptr(),
                                        w2.data_ptr(), b2.data_ptr(), sv.data_ptr(), hv.data_ptr(), ev.data_ptr(), N, C, rd, s))

        def se_apply():
            chk(lib.icamd_se_bn_apply(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), ev.data_ptr(), res.data_ptr(), None, None,
                                      out.data_ptr(), bits.data_ptr(), N, HW, C, 1, s))

        def bn_apply():
            chk(lib.icamd_bn_apply(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), out.data_ptr(), bits.data_ptr(),
                                   y.numel(), C, 1, s))

        def se_bwd():
            chk(lib.icamd_se_bn_bwd(dout.data_ptr(), bits.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                    gamma.data_ptr(), beta.data_ptr(), ysum.data_ptr(), sv.data_ptr(), hv.data_ptr(), ev.data_ptr(),
                                    w1.data_ptr(), w2.data_ptr(), *(t.data_ptr() for t in grads), dy.data_ptr(), N, HW, C, rd, 0,
                                    se_ws.data_ptr(), se_b, s))

        def bn_bwd():
            chk(lib.icamd_bn_bwd(dout.data_ptr(), None, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(),
                                 shift.data_ptr(), dg2.data_ptr(), db2.data_ptr(), dy.data_ptr(), None, bits.data_ptr(), N * HW, C, 1, 0,
                                 bn_ws.data_ptr(), bn_b, s))

        squeeze(); excite(); se_apply()       # the gate and the mask bits the timed calls read
        numel = float(N) * HW * C
        rows = [("squeeze", squeeze, None, 2.0 * numel + 4.0 * N * C),
                ("excite", excite, None, None),
                ("apply", se_apply, bn_apply, numel * 6 + numel / 8 + 4.0 * N * C),
                ("bwd", se_bwd, bn_bwd, numel * 10 + numel / 4 + 4.0 * N * C * 8)]
        for op, se_fn, plain_fn, nbytes in rows:
            ts, tp = [], []
            for _ in range(args.rounds):
                ts.append(timed(se_fn, args.warmup, args.reps))
                if plain_fn is not None:
                    tp.append(timed(plain_fn, args.warmup, args.reps))
            lo, med, hi = mmm(ts)
            gbs = f"{nbytes / med / 1e3:9.0f} {100.0 * nbytes / med / 1e3 / HBM_GBS:6.1f}" if nbytes else f"{'-':>9s} {'-':>6s}"
            line = f"{name:8s} {C:5d} {HW:5d}  {op:8s} {lo:7.1f} {med:7.1f} {hi:7.1f} {gbs}"
            if tp:
                plo, pmed, phi = mmm(tp)
                line += f"   {plo:9.1f} {pmed:9.1f} {phi:9.1f} {med / pmed:9.2f} {phi / plo:10.2f}"
            print(line, flush=True)
        del y, res, dout, out, dy, bits, se_ws, bn_ws, sq_ws
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
