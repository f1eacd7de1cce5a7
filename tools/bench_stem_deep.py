#!/usr/bin/env python3
"""Times the ResNet-D kernels (csrc/conv_stem_deep.hip) at the flagship shapes, batch 256 at 224 x 224:

  * the thin 3x3 convolutions [256,112,112] 32 -> 32 and 32 -> 64: forward (with statistics), data gradient, weight gradient, each
    beside the general route (icamd_conv2d_fwd / _dgrad / _wgrad) on the same tensors, alternated in the same process;
  * conv1.0 (3 -> 32, stride 2, on the 8-channel packed image) on the general route: forward and weight gradient;
  * the 2x2 average pool forward / backward (with addend) at the three pooled shortcuts of ResNet-50d.

Byte roof: algorithmic bytes (every operand read once, every result written once) divided by the streaming bandwidth that
tools/bench_bn.py reports for icamd_bn_apply (read y, write a) in the same session -- it is run first, as a child process.

Method: device events around `reps` back-to-back launches after `warmup` launches, `rounds` rounds, the median round reported.

    python tools/bench_stem_deep.py [--reps 30] [--rounds 5] > profiles/resnet_d.txt
"""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclassification_amd import hip  # noqa: E402

N = 256


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
    return statistics.median(timed(fn, args.warmup, args.reps) for _ in range(args.rounds))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    hip.require_gpu()
    roof = stream_roof()
    lib = hip.load()
    dev = "cuda"
    s = hip.stream_ptr()
    print(f"# ResNet-D kernels, batch {N}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.reps} launches per measurement after {args.warmup}, median of {args.rounds} rounds; byte roof = algorithmic "
          f"bytes / {roof:.2f} TB/s")

    def chk(rc):
        if rc != 0:
            raise hip.IcamdError(f"rc {rc}")

    def line(name, op, us, nbytes, other=None):
        roof_us = nbytes / (roof * 1e6)
        tail = "" if other is None else f" {other:10.1f} {other / us:8.2f}"
        print(f"{name:26s} {op:6s} {us:10.1f} {nbytes / us / 1e3:9.0f} {roof_us:9.1f} {100.0 * roof_us / us:6.1f}{tail}")

    print("# layer                      op        thin_us  alg_GB/s   roof_us  roof%  general_us general/thin")
    stem_us = {}
    for name, cout in (("conv1.3 [256,112,112] 32->32", 32), ("conv1.6 [256,112,112] 32->64", 64)):
        h = 112
        d = hip.conv_desc(N, h, h, 32, cout, 3, 3, 1, 1)
        dref = ctypes.byref(d)
        assert lib.icamd_conv3x3_thin_supported(dref) == 1
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(N, h, h, 32, generator=g, device=dev).clamp_min(0).to(torch.bfloat16)
        dy = torch.randn(N, h, h, cout, generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn(cout, 3, 3, 32, generator=g, device=dev) * (2.0 / (9 * cout)) ** 0.5).to(torch.bfloat16)
        w_t = w.permute(3, 1, 2, 0).contiguous()
        y = torch.empty(N, h, h, cout, dtype=torch.bfloat16, device=dev)
        dx = torch.empty(N, h, h, 32, dtype=torch.bfloat16, device=dev)
        stats = torch.empty(max(lib.icamd_conv3x3_thin_stats_rows(dref), lib.icamd_conv2d_stats_rows(dref)), 2, cout, device=dev)
        dw = torch.empty(cout, 3, 3, 32, device=dev)
        tneed, gneed = lib.icamd_conv3x3_thin_wgrad_workspace_bytes(dref), lib.icamd_conv2d_wgrad_workspace_bytes(dref)
        tws = torch.empty(tneed, dtype=torch.uint8, device=dev)
        gws = torch.empty(gneed, dtype=torch.uint8, device=dev)
        ops = {
            "fwd": (lambda: chk(lib.icamd_conv3x3_thin_fwd(dref, x.data_ptr(), w.data_ptr(), y.data_ptr(), None, stats.data_ptr(), 0, s)),
                    lambda: chk(lib.icamd_conv2d_fwd(dref, x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None, stats.data_ptr(), s))),
            "dgrad": (lambda: chk(lib.icamd_conv3x3_thin_dgrad(dref, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), s)),
                      lambda: chk(lib.icamd_conv2d_dgrad(dref, dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), None, None, s))),
            "wgrad": (lambda: chk(lib.icamd_conv3x3_thin_wgrad(dref, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, tws.data_ptr(),
                                                               tneed, s)),
                      lambda: chk(lib.icamd_conv2d_wgrad(dref, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, gws.data_ptr(), gneed, s))),
        }
        act_bytes = 2.0 * N * h * h * (32 + cout)
        for op, (thin, general) in ops.items():
            tt, tg = [], []
            for _ in range(args.rounds):
                tt.append(timed(thin, args.warmup, args.reps))
                tg.append(timed(general, args.warmup, args.reps))
            ut, ug = statistics.median(tt), statistics.median(tg)
            stem_us[(name, op)] = (ut, ug)
            line(name, op, ut, act_bytes + (4.0 if op == "wgrad" else 2.0) * cout * 9 * 32, ug)
        del x, dy, w, w_t, y, dx, dw, tws, gws
        torch.cuda.empty_cache()

    # conv1.0 on the general route (no data gradient: it reads the image)
    print("# layer                      op     general_us  alg_GB/s   roof_us  roof%")
    d = hip.conv_desc(N, 224, 224, 8, 32, 3, 3, 2, 1)
    dref = ctypes.byref(d)
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(N, 224, 224, 8, generator=g, device=dev).to(torch.bfloat16)
    x[..., 3:] = 0
    w = (torch.randn(32, 3, 3, 8, generator=g, device=dev) * 0.1).to(torch.bfloat16)
    y = torch.empty(N, 112, 112, 32, dtype=torch.bfloat16, device=dev)
    dy = torch.randn(N, 112, 112, 32, generator=g, device=dev).to(torch.bfloat16)
    stats = torch.empty(lib.icamd_conv2d_stats_rows(dref), 2, 32, device=dev)
    dw = torch.empty(32, 3, 3, 8, device=dev)
    gneed = lib.icamd_conv2d_wgrad_workspace_bytes(dref)
    gws = torch.empty(gneed, dtype=torch.uint8, device=dev)
    nbytes = 2.0 * N * (224 * 224 * 8 + 112 * 112 * 32)
    c0_fwd = median_of(lambda: chk(lib.icamd_conv2d_fwd(dref, x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None, stats.data_ptr(), s)),
                       args)
    c0_wg = median_of(lambda: chk(lib.icamd_conv2d_wgrad(dref, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, gws.data_ptr(), gneed, s)),
                      args)
    line("conv1.0 [256,224,224] 8->32 /2", "fwd", c0_fwd, nbytes)
    line("conv1.0 [256,224,224] 8->32 /2", "wgrad", c0_wg, nbytes)
    del x, y, dy, gws
    torch.cuda.empty_cache()
    for label, pick in (("thin", 0), ("general", 1)):
        convs = sum(v[pick] for v in stem_us.values())
        total = convs + c0_fwd + c0_wg
        print(f"# stem convolutions, {label} route for conv1.3 / conv1.6: {total:.0f} us; conv1.0 (fwd + wgrad) {c0_fwd + c0_wg:.0f} us = "
              f"{100.0 * (c0_fwd + c0_wg) / total:.1f} % of it (a kernel of its own is considered above 25 %)")

    # 2x2 average pool of the pooled shortcuts
    print("# pool                       op             us  alg_GB/s   roof_us  roof%")
    for h, c in ((56, 256), (28, 512), (14, 1024)):
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.randn(N, h, h, c, generator=g, device=dev).to(torch.bfloat16)
        add = torch.randn(N, h, h, c, generator=g, device=dev).to(torch.bfloat16)
        out = torch.empty(N, h // 2, h // 2, c, dtype=torch.bfloat16, device=dev)
        dout = torch.randn(N, h // 2, h // 2, c, generator=g, device=dev).to(torch.bfloat16)
        dx = torch.empty_like(x)
        full, quarter = 2.0 * N * h * h * c, 2.0 * N * (h // 2) * (h // 2) * c
        name = f"avgpool2x2 [256,{h},{h},{c}]"
        line(name, "fwd", median_of(lambda: chk(lib.icamd_avgpool2x2_fwd(x.data_ptr(), out.data_ptr(), N, h, h, c, s)), args),
             full + quarter)
        line(name, "bwd", median_of(lambda: chk(lib.icamd_avgpool2x2_bwd(dout.data_ptr(), None, dx.data_ptr(), N, h, h, c, s)), args),
             full + quarter)
        line(name, "bwd+add", median_of(lambda: chk(lib.icamd_avgpool2x2_bwd(dout.data_ptr(), add.data_ptr(), dx.data_ptr(), N, h, h, c,
                                                                             s)), args), 2 * full + quarter)
        del x, add, out, dout, dx
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
