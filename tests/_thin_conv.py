"""Shared by tests/test_resnet_d_kernels_gpu.py and tests/test_multitrip_gpu.py: the operands and fp64-accumulated references of a thin
3x3 convolution case (icamd_conv3x3_thin_*, csrc/conv_stem_deep.hip) and its three launches on guarded, NaN-filled outputs.
Importing it needs no GPU."""
import ctypes

import torch

from _harness import guarded, hip, intact, rnd_bf16
from oracle import ops_ref as R

_CACHE = {}


def thin_inputs(case):
    """Operands and fp64-accumulated references of a case, computed once and shared by the tests (never modified)."""
    if case in _CACHE:
        return _CACHE[case]
    N, H, W, Cout = case
    d = hip().conv_desc(N, H, W, 32, Cout, 3, 3, 1, 1)
    x = rnd_bf16(N, H, W, 32, seed=1)
    w = rnd_bf16(Cout, 3, 3, 32, scale=(1.0 / (9 * 32)) ** 0.5, seed=2)
    dy = rnd_bf16(N, H, W, Cout, seed=3)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(4))
    F64 = torch.float64
    ref = {"y": R.conv2d_fwd(x, w, 1, 1, acc=F64).float(),
           "dx": R.conv2d_dgrad(dy, w, (H, W), 1, 1, acc=F64).float(),
           "dw": R.conv2d_wgrad(x, dy, (3, 3), 1, 1, acc=F64)}
    z = R.conv2d_fwd(x, w, 1, 1, bias=bias, acc=F64).float()      # (rounded after the bias; ReLU commutes with the rounding)
    ref["z"], ref["zr"] = z, z.clamp_min(0)
    _CACHE[case] = (d, x, w, dy, bias, ref)
    return _CACHE[case]


def run_fwd(lib, d, xd, wd, bias=None, stats=None, relu=0):
    h = hip()
    y, g = guarded((d.N, d.OH, d.OW, d.Cout), torch.bfloat16)
    rc = lib.icamd_conv3x3_thin_fwd(ctypes.byref(d), h.ptr(xd), h.ptr(wd), h.ptr(y), h.ptr(bias), h.ptr(stats), relu,
                                    h.stream_ptr())
    assert rc == 0
    assert intact(g), "guard band behind y written"
    return y


def run_dgrad(lib, d, dyd, wd):
    h = hip()
    dx, g = guarded((d.N, d.IH, d.IW, d.Cin), torch.bfloat16)
    assert lib.icamd_conv3x3_thin_dgrad(ctypes.byref(d), h.ptr(dyd), h.ptr(wd), h.ptr(dx), h.stream_ptr()) == 0
    assert intact(g), "guard band behind dx written"
    return dx


def run_wgrad(lib, d, xd, dyd, prefill=None):
    h = hip()
    dw, g = guarded((d.Cout, 3, 3, 32), torch.float32)
    if prefill is not None:
        dw.copy_(prefill)
    need = lib.icamd_conv3x3_thin_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0 and need % (32 * 4) == 0
    ws, gw = guarded((need // (32 * 4), 32), torch.float32)          # rows of one tap's 32 input channels
    rc = lib.icamd_conv3x3_thin_wgrad(ctypes.byref(d), h.ptr(xd), h.ptr(dyd), h.ptr(dw), 0 if prefill is None else 1,
                                      h.ptr(ws), need, h.stream_ptr())
    assert rc == 0
    assert intact(g), "guard band behind dw written"
    assert intact(gw), "guard band behind the workspace written"
    return dw
