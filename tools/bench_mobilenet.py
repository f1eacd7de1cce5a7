#!/usr/bin/env python3
"""Times the MobileNetV2 kernels (csrc/dwconv3x3.hip) and the training step on one GPU, batch 256.

Kernels: the ten depthwise shapes of mobilenetv2_100 at 224 x 224 -- (C, H, stride) = (32, 112, 1), (96, 112, 2), (144, 56, 1),
(144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1), (576, 14, 1), (576, 14, 2), (960, 7, 1).  Per shape, alternated in the same
process on the same tensors:

    stream     icamd_bn_apply over the input tensor (read one tensor, write one): the streaming rate of this session, the byte roof
    fwd / wgrad, each ON-LOAD (raw x + scale / shift) and PLAIN (icamd_bn_apply_relu6 into a buffer, then the call on that buffer: the
               apply's time is part of the plain route); forward with statistics, as the model calls it
    dgrad      one form only (the gradient of the activated input)
    torch      F.conv2d(groups=C) on the channels-last bf16 tensor behind F.batch_norm (eval coefficients) + F.hardtanh; backward:
               autograd.grad for input and filter (forward + backward minus forward), to be set against dgrad + wgrad

Algorithmic bytes: forward 2 (in + out) B per element of each, statistics rows besides; data gradient the same; weight gradient in +
dy read.  roof% = the time those bytes take at `stream`'s rate over the measured median.  Medians of `rounds` alternated rounds with
min / max: a ratio inside the spread of its own rows is not a measured difference.

Step: mobilenetv2_100 and mobilenetv2_140 alternated twice with resnet50 through engine.train_one_epoch (AdamW, label smoothing,
synthetic data resident on the device), ms/step and img/s.

    python tools/bench_mobilenet.py [--reps 20] [--rounds 5] [--steps 12] > profiles/mobilenetv2.txt
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

N = 256
SHAPES = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1), (576, 14, 1), (576, 14, 2),
          (960, 7, 1)]


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
    """the tensors of one (C, H, stride) and the launches on them"""

    def __init__(self, lib, C, hw, stride, with_torch):
        dev, self.lib, self.C, self.hw, self.stride, self.s = "cuda", lib, C, hw, stride, hip.stream_ptr()
        oh = (hw - 1) // stride + 1
        g = torch.Generator(device=dev).manual_seed(1)
        self.x = torch.randn(N, hw, hw, C, generator=g, device=dev).to(torch.bfloat16)
        self.a = torch.empty_like(self.x)
        self.dy = (torch.randn(N, oh, oh, C, generator=g, device=dev) * 0.1).to(torch.bfloat16)
        self.w = (torch.randn(3, 3, C, generator=g, device=dev) * 0.3).to(torch.bfloat16)
        self.scale = 2.0 + 2.0 * torch.rand(C, generator=g, device=dev)
        self.shift = 0.5 + 0.5 * torch.randn(C, generator=g, device=dev)
        self.y = torch.empty(N, oh, oh, C, dtype=torch.bfloat16, device=dev)
        self.dx = torch.empty_like(self.x)
        self.dw = torch.empty(3, 3, C, device=dev)
        self.rows = lib.icamd_dwconv3_stats_rows(N, hw, hw, C, stride)
        self.stats = torch.empty(self.rows, 2, C, device=dev)
        self.wsb = lib.icamd_dwconv3_wgrad_workspace_bytes(N, hw, hw, C, stride)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.ones, self.zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        self.in_el, self.out_el = float(self.x.numel()), float(self.y.numel())
        if with_torch:      # NCHW views of the same channels-last memory; bf16 parameters, as autocast would hand them to the module
            self.xt = self.x.permute(0, 3, 1, 2).requires_grad_(True)
            self.dyt = self.dy.permute(0, 3, 1, 2)
            self.wt = self.w.permute(2, 0, 1).reshape(C, 1, 3, 3).contiguous().requires_grad_(True)
            self.rm, self.rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            self.g16, self.b16 = self.scale.to(torch.bfloat16), self.shift.to(torch.bfloat16)

    def chk(self, rc):
        if rc != 0:
            raise hip.IcamdError(f"{self.C} x {self.hw} / {self.stride}: rc {rc}")

    def stream(self):
        self.chk(self.lib.icamd_bn_apply(self.x.data_ptr(), self.ones.data_ptr(), self.zeros.data_ptr(), None, self.a.data_ptr(), None,
                                         self.x.numel(), self.C, 0, self.s))

    def _apply(self):
        self.chk(self.lib.icamd_bn_apply_relu6(self.x.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), self.a.data_ptr(),
                                               self.x.numel(), self.C, self.s))

    def _fwd(self, x, sc, sh):
        self.chk(self.lib.icamd_dwconv3_fwd(x, sc, sh, self.w.data_ptr(), self.y.data_ptr(), self.stats.data_ptr(), N, self.hw, self.hw,
                                            self.C, self.stride, self.s))

    def _wgrad(self, x, sc, sh):
        self.chk(self.lib.icamd_dwconv3_wgrad(x, sc, sh, self.dy.data_ptr(), self.dw.data_ptr(), 0, self.ws.data_ptr(), self.wsb, N,
                                              self.hw, self.hw, self.C, self.stride, self.s))

    def fwd_onload(self):
        self._fwd(self.x.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr())

    def fwd_plain(self):
        self._apply()
        self._fwd(self.a.data_ptr(), None, None)

    def wgrad_onload(self):
        self._wgrad(self.x.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr())

    def wgrad_plain(self):
        self._apply()
        self._wgrad(self.a.data_ptr(), None, None)

    def dgrad(self):
        self.chk(self.lib.icamd_dwconv3_dgrad(self.dy.data_ptr(), self.w.data_ptr(), self.dx.data_ptr(), N, self.hw, self.hw, self.C,
                                              self.stride, self.s))

    def _torch(self, x):
        a = F.hardtanh(F.batch_norm(x, self.rm, self.rv, self.g16, self.b16, False, 0.0, 1e-5), 0.0, 6.0)
        return F.conv2d(a, self.wt, None, self.stride, 1, 1, self.C)

    def torch_fwd(self):
        with torch.no_grad():
            self._torch(self.xt)

    def torch_fwd_bwd(self):      # autograd needs its own forward; torch_fwd is subtracted by the caller
        torch.autograd.grad(self._torch(self.xt), (self.xt, self.wt), self.dyt)


def kernels(lib, args):
    names = ["stream", "fwd_onload", "fwd_plain", "dgrad", "wgrad_onload", "wgrad_plain"]
    if not args.no_torch:
        names += ["torch_fwd", "torch_fwd_bwd"]
    print(f"# kernels: {args.reps} launches per measurement after {args.warmup}, {args.rounds} alternated rounds (min / median / max in "
          "us); torch: a quarter of the launches")
    print("# torch_us: fwd rows = batch_norm + hardtanh + conv2d(groups=C); the `bwd` row = autograd.grad for input + filter (forward + "
          "backward minus forward) against dgrad + wgrad_onload")
    print("#    C    H  s  op            min_us  med_us  max_us  stream_TB/s  roof_us  roof%  torch_us  torch/ours")
    verdict = {op: {"plain": [], "on-load": [], "neither": []} for op in ("fwd", "wgrad")}
    for C, hw, stride in SHAPES:
        case = Case(lib, C, hw, stride, not args.no_torch)
        ts = {k: [] for k in names}
        for _ in range(args.rounds):
            for k in names:
                reps = args.reps if not k.startswith("torch") else max(args.reps // 4, 3)
                ts[k].append(timed(getattr(case, k), args.warmup, reps))
        tbs = 4.0 * case.in_el / statistics.median(ts["stream"]) / 1e6
        stats_b = 8.0 * case.rows * C
        nbytes = {"fwd_onload": 2 * case.in_el + 2 * case.out_el + stats_b, "fwd_plain": 6 * case.in_el + 2 * case.out_el + stats_b,
                  "dgrad": 2 * case.in_el + 2 * case.out_el, "wgrad_onload": 2 * case.in_el + 2 * case.out_el,
                  "wgrad_plain": 6 * case.in_el + 2 * case.out_el}
        ts["bwd"] = [a + b for a, b in zip(ts["dgrad"], ts["wgrad_onload"])]
        t_torch = {}
        if not args.no_torch:
            t_torch["fwd_onload"] = statistics.median(ts["torch_fwd"])
            t_torch["bwd"] = statistics.median([a - b for a, b in zip(ts["torch_fwd_bwd"], ts["torch_fwd"])])
        for op in ("fwd_onload", "fwd_plain", "dgrad", "wgrad_onload", "wgrad_plain", "bwd"):
            lo, med, hi = min(ts[op]), statistics.median(ts[op]), max(ts[op])
            line = f"{C:6d} {hw:4d} {stride:2d}  {op:12s} {lo:7.1f} {med:7.1f} {hi:7.1f} {tbs:12.2f} "
            if op in nbytes:
                roof_us = nbytes[op] / (tbs * 1e6)
                line += f"{roof_us:8.1f} {100.0 * roof_us / med:6.1f} "
            else:
                line += f"{'-':>8s} {'-':>6s} "
            line += f"{t_torch[op]:9.1f} {t_torch[op] / med:11.2f}" if op in t_torch else f"{'-':>9s} {'-':>11s}"
            print(line, flush=True)
        for op in ("fwd", "wgrad"):     # the route decision: does one form beat the other by more than the spread of both rows?
            on, pl = ts[op + "_onload"], ts[op + "_plain"]
            if max(pl) < min(on):
                verdict[op]["plain"].append(f"({C}, {hw}, {stride}) {statistics.median(pl):.1f} < {statistics.median(on):.1f}")
            elif max(on) < min(pl):
                verdict[op]["on-load"].append(f"({C}, {hw}, {stride}) {statistics.median(on):.1f} < {statistics.median(pl):.1f}")
            else:
                verdict[op]["neither"].append(f"({C}, {hw}, {stride})")
        del case
        torch.cuda.empty_cache()
    from imageclassification_amd.mobilenet import DW_ONLOAD
    for op in ("fwd", "wgrad"):
        print(f"# route, {op} (us, beyond the spread of both rows): " + "; ".join(f"{k} wins at {len(v)}: " + ", ".join(v)
                                                                                 for k, v in verdict[op].items() if v))
    print(f"# mobilenet.DW_ONLOAD = {DW_ONLOAD}: the route the step below runs")


def step_times(args):
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.mobilenet import MobileNetV2
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
        for arch in ("mobilenetv2_100", "resnet50", "mobilenetv2_140", "resnet50"):
            net = MobileNetV2(arch, C, seed=88) if arch.startswith("mobilenetv2") else ResNet(arch, C, seed=88)
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
    ap.add_argument("--no-torch", action="store_true", help="leave torch's route out")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    args = ap.parse_args()
    hip.require_gpu()
    lib = hip.load()
    print(f"# MobileNetV2 (csrc/dwconv3x3.hip, imageclassification_amd/mobilenet.py), batch {N}; {torch.cuda.get_device_name(0)}")
    kernels(lib, args)
    if not args.no_step:
        step_times(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
