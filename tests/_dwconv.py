"""What the depthwise 3x3 / 5x5 and ReLU6 BatchNorm tests share: the launch geometry of csrc/dwconv3x3.hip and csrc/dwconv5x5.hip
mirrored in Python (one geometry: the two differ in the taps of a kernel row alone; so that a test can say which loop a shape drives
through more than one trip), seeded operands (3x3: with the clamp shares the tests require), and thin runners of the 3x3 entries.
Importing this module needs no GPU."""
import functools

import torch

import _harness
from _harness import DEV, dev, guarded
from oracle import ops_ref as R

RS = 16                                                    # output rows per item (dwconv3x3.hip, dwconv5x5.hip)
# 3x3, (N, H, W, C): the issue's six, then the two that drive what those do not (see trips())
SHAPES = [(2, 7, 7, 24), (3, 9, 11, 48), (2, 14, 14, 144), (2, 8, 8, 528), (1, 1, 5, 16), (3, 57, 57, 96), (2100, 3, 5, 16),
          (2, 5, 5, 1344)]
# 5x5, (N, H, W, C), each at stride 1 and 2: the issue's eight; trips(..., k=5) shows they run every loop more than once
SHAPES5 = [(2, 2, 3, 8), (1, 1, 5, 16), (2, 7, 7, 24), (3, 9, 11, 48), (2, 14, 14, 144), (3, 37, 41, 40), (2, 5, 5, 1152),
           (2100, 3, 5, 16)]


def cdiv(a, b):
    return (a + b - 1) // b


def geometry(N, H, W, C, stride, cap, pixels_per_row):
    """dw3_geometry and dw5_geometry, the same function: forward (cap 2048, 16 pixels per partial row) and weight gradient (1024, 64)"""
    OH, OW, cpr = (H - 1) // stride + 1, (W - 1) // stride + 1, C // 8
    cv = min(cpr, 256)
    while cpr % cv or (256 // cv) * cv < 192:
        cv -= 1
    lanes = 256 // cv
    colgroups, rowsegs = cdiv(OW, lanes), cdiv(OH, RS)
    items = N * rowsegs * colgroups
    target = min(cap, max(32, N * OH * OW // pixels_per_row))
    ipb = cdiv(items, target)
    return {"OH": OH, "OW": OW, "cv": cv, "lanes": lanes, "nslices": cpr // cv, "colgroups": colgroups, "rowsegs": rowsegs,
            "items": items, "ipb": ipb, "rows": cdiv(items, ipb)}


def fwd_geometry(N, H, W, C, stride):
    return geometry(N, H, W, C, stride, 2048, 16)


def wgrad_geometry(N, H, W, C, stride):
    return geometry(N, H, W, C, stride, 1024, 64)


def trips(N, H, W, C, stride, k=3):
    """trip count of every loop of dwconv{k}_fwd_kernel / dwconv{k}_wgrad_kernel whose length depends on the problem; a thread leaves
    the k taps of a kernel row times its 8 channels in the LDS (red[256 * 24], red[256 * 40])"""
    f, w = fwd_geometry(N, H, W, C, stride), wgrad_geometry(N, H, W, C, stride)
    return {"items of a workgroup, forward": f["ipb"], "items of a workgroup, weight gradient": w["ipb"],
            "rows of a segment": min(RS, f["OH"]), "row segments": f["rowsegs"], "column groups": f["colgroups"],
            "column lanes folded per output": f["lanes"], "LDS outputs of the statistics fold (o += 256)": cdiv(f["cv"] * 16, 256),
            "LDS outputs of a kernel row of taps (o += 256)": cdiv(w["cv"] * 8 * k, 256), "channel slices per pixel": f["nslices"],
            "partial rows, forward": f["rows"], "partial rows, weight gradient": w["rows"]}


def coeffs(C, seed):
    """scale U(2, 4), shift N(0.5, 0.5) with channel 0 pinned above 1: relu6(shift) there is what a wrongly padded tap would add"""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 + 2.0 * torch.rand(C, generator=g)
    shift = 0.5 + 0.5 * torch.randn(C, generator=g)
    shift[0] = 1.5
    return scale, shift


def clamp_shares(a):
    """(share of the activated elements at 6, share at 0)"""
    return float((a == 6).float().mean()), float((a == 0).float().mean())


@functools.lru_cache(maxsize=None)
def case(shape, stride, onload):
    """operands and the fp64 reference of one case, computed once: x (raw), scale / shift (onload), a (what the stencil sees), w
    [C,3,3], dy, and y / dx / dw of R.dwconv3_ref"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 + 7 * N + H + 3 * stride)
    x = R.bf16_round(1.5 * torch.randn(N, H, W, C, generator=g))
    w = R.bf16_round(0.3 * torch.randn(C, 3, 3, generator=g))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = R.bf16_round(torch.randn(N, OH, OW, C, generator=g))
    scale, shift = coeffs(C, 17 + C) if onload else (None, None)
    a = R.bn_relu6(x, scale, shift) if onload else x
    y, dx, dw = R.dwconv3_ref(a, w, dy, stride)
    return {"x": x, "w": w, "dy": dy, "scale": scale, "shift": shift, "a": a, "y": y, "dx": dx, "dw": dw, "OH": OH, "OW": OW}


@functools.lru_cache(maxsize=None)
def dw5_case(shape, stride):
    """operands and the fp64 reference of one 5x5 case, computed once"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(2000 + 7 * N + H + 3 * stride)
    x = R.bf16_round(1.5 * torch.randn(N, H, W, C, generator=g))
    w = R.bf16_round(0.2 * torch.randn(C, 5, 5, generator=g))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = R.bf16_round(torch.randn(N, OH, OW, C, generator=g))
    y, dx, dw = R.dwconv5_ref(x, w, dy, stride)
    return {"x": x, "w": w, "dy": dy, "y": y, "dx": dx, "dw": dw, "OH": OH, "OW": OW}


class Runner:
    """the 3x3 entries on device tensors; outputs are guarded and every call asserts its return code"""

    def __init__(self, lib, shape, stride):
        self.lib, self.hip, self.shape, self.stride = lib, _harness.hip(), shape, stride
        N, H, W, C = shape
        self.out_shape = (N, (H - 1) // stride + 1, (W - 1) // stride + 1, C)
        self.stats_rows = lib.icamd_dwconv3_stats_rows(N, H, W, C, stride)
        self.wsb = lib.icamd_dwconv3_wgrad_workspace_bytes(N, H, W, C, stride)

    def fwd(self, x, w33c, scale=None, shift=None, stats=False):
        hip, (N, H, W, C) = self.hip, self.shape
        y, gy = guarded(self.out_shape, torch.bfloat16)
        st, gs = guarded((self.stats_rows, 2, C), torch.float32) if stats else (None, None)
        rc = self.lib.icamd_dwconv3_fwd(hip.ptr(x), hip.ptr(scale), hip.ptr(shift), hip.ptr(w33c), hip.ptr(y), hip.ptr(st), N, H, W, C,
                                        self.stride, hip.stream_ptr())
        assert rc == 0, rc
        assert _harness.intact(gy), "guard band behind y written"
        assert gs is None or _harness.intact(gs), "guard band behind the statistics written"
        return y, st

    def dgrad(self, dy, w33c):
        hip, (N, H, W, C) = self.hip, self.shape
        dx, gx = guarded(self.shape, torch.bfloat16)
        assert self.lib.icamd_dwconv3_dgrad(hip.ptr(dy), hip.ptr(w33c), hip.ptr(dx), N, H, W, C, self.stride, hip.stream_ptr()) == 0
        assert _harness.intact(gx), "guard band behind dx written"
        return dx

    def wgrad(self, x, dy, scale=None, shift=None, base=None):
        """base None: accumulate = 0 into NaN; else accumulate = 1 onto `base`"""
        hip, (N, H, W, C) = self.hip, self.shape
        dw, gw = guarded((3, 3, C), torch.float32, fill=float("nan") if base is None else base)
        ws, gws = guarded((self.wsb,), torch.uint8, fill=0x7F)
        rc = self.lib.icamd_dwconv3_wgrad(hip.ptr(x), hip.ptr(scale), hip.ptr(shift), hip.ptr(dy), hip.ptr(dw), int(base is not None),
                                          hip.ptr(ws), self.wsb, N, H, W, C, self.stride, hip.stream_ptr())
        assert rc == 0, rc
        assert _harness.intact(gw), "guard band behind dw written"
        assert _harness.intact(gws), "guard band behind the workspace written"
        return dw


def device_operands(c):
    """x, w [3][3][C], dy, scale, shift on the device"""
    f32 = lambda t: None if t is None else t.to(DEV)     # noqa: E731
    return dev(c["x"]), dev(c["w"].permute(1, 2, 0).contiguous()), dev(c["dy"]), f32(c["scale"]), f32(c["shift"])
