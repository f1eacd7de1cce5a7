#!/usr/bin/env python3
"""Times the depthwise 7x7 kernels (csrc/dwconv.hip) on the stage shapes of convnext_atto, _femto and _nano at batch 256 and
224 x 224 -- (H, C) = (56, 40), (28, 80), (14, 160), (7, 320); (56, 48), (28, 96), (14, 192), (7, 384); (56, 80), (28, 160), (14, 320),
(7, 640) -- and, alternated with them in the same process on the same tensors,

    icamd_bn_apply (read one tensor, write one)   -> the streaming rate of this session, in TB/s: the byte roof
    torch's own depthwise convolution             F.conv2d(groups=C) on the channels-last bf16 tensor; backward: autograd.grad
                                                  for input, filter and bias, to be set against dgrad + wgrad_bias
    the same three kernels at the next width that is a multiple of 32, same H and W (only where C % 32 != 0), as us per channel

Algorithmic bytes: forward 4 B per element (x read, y written), data gradient with addend 6 B, weight + bias gradient 4 B (x and dy
read).  roof% = the time those bytes take at icamd_bn_apply's rate of the same shape, over the measured time.

Method: device events around `reps` back-to-back launches after `warmup` launches, the candidates alternated over `rounds` rounds;
min / median / max over the rounds.  A ratio inside the max / min spread of its own rows is not a measured difference.

    python tools/bench_dwconv_narrow.py [--reps 20] [--rounds 5] > profiles/convnext_narrow.txt
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclassification_amd import hip  # noqa: E402

N = 256
MODELS = [("atto", (40, 80, 160, 320)), ("femto", (48, 96, 192, 384)), ("nano", (80, 160, 320, 640))]
SIDES = (56, 28, 14, 7)
BYTES = {"fwd": 4.0, "dgrad": 6.0, "wgrad": 4.0}


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


class Case:
    """the tensors of one (H, C) and the launches on them"""

    def __init__(self, lib, hw, C, with_torch):
        dev, self.lib, self.hw, self.C, self.s = "cuda", lib, hw, C, hip.stream_ptr()
        g = torch.Generator(device=dev).manual_seed(1)
        self.x = torch.randn(N, hw, hw, C, generator=g, device=dev).to(torch.bfloat16)
        self.dy = (torch.randn(N, hw, hw, C, generator=g, device=dev) * 0.1).to(torch.bfloat16)
        self.ad = torch.randn(N, hw, hw, C, generator=g, device=dev).to(torch.bfloat16)
        self.w = (torch.randn(7, 7, C, generator=g, device=dev) * 0.1).to(torch.bfloat16)
        self.b = torch.randn(C, generator=g, device=dev)
        self.y = torch.empty_like(self.x)
        self.dw, self.db = torch.empty(7, 7, C, device=dev), torch.empty(C, device=dev)
        self.wsb = lib.icamd_dwconv7_wgrad_workspace_bytes(N, hw, hw, C)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.ones, self.zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        if not lib.icamd_dwconv7_wgrad_bias_supported(N, hw, hw, C):
            raise hip.IcamdError(f"{hw}x{hw}x{C}: the one-pass weight gradient is refused")
        if with_torch:      # NCHW views of the same channels-last memory; bf16 parameters, as autocast would hand them to the module
            self.xt = self.x.permute(0, 3, 1, 2).requires_grad_(True)
            self.dyt = self.dy.permute(0, 3, 1, 2)
            self.wt = self.w.permute(2, 0, 1).reshape(C, 1, 7, 7).contiguous().requires_grad_(True)
            self.bt = self.b.to(torch.bfloat16).requires_grad_(True)

    def chk(self, rc):
        if rc != 0:
            raise hip.IcamdError(f"{self.hw}x{self.hw}x{self.C}: rc {rc}")

    def stream(self):
        self.chk(self.lib.icamd_bn_apply(self.x.data_ptr(), self.ones.data_ptr(), self.zeros.data_ptr(), None, self.y.data_ptr(), None,
                                         self.x.numel(), self.C, 0, self.s))

    def fwd(self):
        self.chk(self.lib.icamd_dwconv7_fwd(self.x.data_ptr(), self.w.data_ptr(), self.b.data_ptr(), self.y.data_ptr(), N, self.hw,
                                            self.hw, self.C, self.s))

    def dgrad(self):
        self.chk(self.lib.icamd_dwconv7_dgrad(self.dy.data_ptr(), self.w.data_ptr(), self.ad.data_ptr(), self.y.data_ptr(), N, self.hw,
                                              self.hw, self.C, self.s))

    def wgrad(self):
        self.chk(self.lib.icamd_dwconv7_wgrad_bias(self.x.data_ptr(), self.dy.data_ptr(), self.dw.data_ptr(), self.db.data_ptr(), 0,
                                                   self.ws.data_ptr(), self.wsb, N, self.hw, self.hw, self.C, self.s))

    def torch_fwd(self):
        with torch.no_grad():
            F.conv2d(self.xt, self.wt, self.bt, padding=3, groups=self.C)

    def torch_fwd_bwd(self):      # autograd needs its own forward; torch_fwd is subtracted by the caller
        yt = F.conv2d(self.xt, self.wt, self.bt, padding=3, groups=self.C)
        torch.autograd.grad(yt, (self.xt, self.wt, self.bt), self.dyt)


def measure(case, names, args):
    ts = {k: [] for k in names}
    for _ in range(args.rounds):
        for k in names:
            reps = args.reps if not k.startswith("torch") else max(args.reps // 4, 3)
            ts[k].append(timed(getattr(case, k), args.warmup, reps))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="leave torch's depthwise convolution out")
    args = ap.parse_args()
    hip.require_gpu()
    lib = hip.load()
    print(f"# depthwise 7x7 (csrc/dwconv.hip) on the stage shapes of convnext_atto / _femto / _nano, batch {N}; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"# {args.reps} launches per measurement after {args.warmup}, {args.rounds} alternated rounds (min / median / max in us); "
          "torch: a quarter of the launches")
    print("# torch_us: forward = F.conv2d; dgrad and wgrad rows share ONE torch figure, autograd.grad for input + filter + bias "
          "(forward + backward minus forward), to be set against dgrad + wgrad_bias: the `both` row")
    print("# model  H    C   op      min_us  med_us  max_us  stream_TB/s  roof_us  roof%  us/ch   C32  C32_med  C32_us/ch  "
          "narrow/C32  torch_us  torch/ours")
    done = {}
    for model, dims in MODELS:
        for hw, C in zip(SIDES, dims):
            if (hw, C) in done:
                print(f"{model:6s} {hw:3d} {C:4d}  as {done[hw, C]}")
                continue
            done[hw, C] = model
            names = ["stream", "fwd", "dgrad", "wgrad"] + ([] if args.no_torch else ["torch_fwd", "torch_fwd_bwd"])
            case = Case(lib, hw, C, not args.no_torch)
            ts = measure(case, names, args)
            del case
            torch.cuda.empty_cache()
            C32 = (C + 31) // 32 * 32
            near = None
            if C32 != C:
                wide = Case(lib, hw, C32, False)
                near = measure(wide, ["fwd", "dgrad", "wgrad"], args)
                del wide
                torch.cuda.empty_cache()
            numel = float(N) * hw * hw * C
            tbs = 4.0 * numel / statistics.median(ts["stream"]) / 1e6
            t_torch = {}
            if not args.no_torch:
                t_torch["fwd"] = statistics.median(ts["torch_fwd"])
                t_torch["both"] = statistics.median([a - b for a, b in zip(ts["torch_fwd_bwd"], ts["torch_fwd"])])
            ts["both"] = [a + b for a, b in zip(ts["dgrad"], ts["wgrad"])]
            if near is not None:
                near["both"] = [a + b for a, b in zip(near["dgrad"], near["wgrad"])]
            for op in ("fwd", "dgrad", "wgrad", "both"):
                lo, med, hi = min(ts[op]), statistics.median(ts[op]), max(ts[op])
                line = f"{model:6s} {hw:3d} {C:4d}  {op:6s} {lo:7.1f} {med:7.1f} {hi:7.1f} {tbs:12.2f} "
                if op in BYTES:
                    roof_us = BYTES[op] * numel / (tbs * 1e6)
                    line += f"{roof_us:8.1f} {100.0 * roof_us / med:6.1f} "
                else:
                    line += f"{'-':>8s} {'-':>6s} "
                line += f"{med / C:6.3f} "
                if near is not None:
                    nmed = statistics.median(near[op])
                    line += f"{C32:5d} {nmed:8.1f} {nmed / C32:10.3f} {(med / C) / (nmed / C32):11.2f} "
                else:
                    line += f"{'-':>5s} {'-':>8s} {'-':>10s} {'-':>11s} "
                if op in t_torch:
                    line += f"{t_torch[op]:9.1f} {t_torch[op] / med:11.2f}"
                else:
                    line += f"{'-':>9s} {'-':>11s}"
                print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
