"""The grouped 3x3 convolution entries (icamd_gconv3x3_*) at the seven conv2 shapes of ResNeXt-50 32x4d at batch 256 and 224 x 224:
forward (with statistics), data gradient and weight gradient against the grouped convolution accumulated in fp64 on the GPU
from the same bf16 inputs, with the checkers of tests/_fullsize_check.py -- bf16 outputs on sample_rows (every 31st pixel row
plus the whole first, middle and last image), every element of dw."""
import ctypes

import pytest
import torch

from _fullsize_check import check_bf16, check_fp32, check_stats, require, sample_rows
from _harness import free_after_each  # noqa: F401
from _harness import lib  # noqa: F401
from _harness import rnd_dev as rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
N = 256
GROUPS = 32
# (C, input grid, stride): layer1.*, layer2.0, layer2.1-3, layer3.0, layer3.1-5, layer4.0, layer4.1-2
SHAPES = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


def _taps(xp, r, s, st, OH, OW):
    return xp[:, r:r + st * (OH - 1) + 1:st, s:s + st * (OW - 1) + 1:st]


def ref_fwd(x, w, st, OH, OW):
    """fp64 grouped convolution, NHWC, pad 1: [N*OH*OW, C]."""
    n, H, W, C = x.shape
    cg = w.shape[-1]
    xp = torch.nn.functional.pad(x.to(F64), (0, 0, 1, 1, 1, 1))
    wg = w.to(F64).reshape(C // cg, cg, 3, 3, cg)
    y = torch.zeros(n * OH * OW, C // cg, cg, dtype=F64, device=x.device)
    for r in range(3):
        for s in range(3):
            xs = _taps(xp, r, s, st, OH, OW).reshape(-1, C // cg, cg)
            y += torch.einsum("mgc,gkc->mgk", xs, wg[:, :, r, s])
    return y.reshape(-1, C)


def ref_dgrad(dy, w, st, H, W):
    n, OH, OW, C = dy.shape
    cg = w.shape[-1]
    wg = w.to(F64).reshape(C // cg, cg, 3, 3, cg)
    dyg = dy.to(F64).reshape(-1, C // cg, cg)
    dxp = torch.zeros(n, H + 2, W + 2, C, dtype=F64, device=dy.device)
    for r in range(3):
        for s in range(3):
            _taps(dxp, r, s, st, OH, OW).add_(torch.einsum("mgk,gkc->mgc", dyg, wg[:, :, r, s]).reshape(n, OH, OW, C))
    return dxp[:, 1:H + 1, 1:W + 1].reshape(-1, C)


def ref_wgrad(x, dy, st, cg):
    n, OH, OW, C = dy.shape
    xp = torch.nn.functional.pad(x.to(F64), (0, 0, 1, 1, 1, 1))
    dyg = dy.to(F64).reshape(-1, C // cg, cg)
    dw = torch.zeros(C // cg, cg, 3, 3, cg, dtype=F64, device=x.device)
    for r in range(3):
        for s in range(3):
            xs = _taps(xp, r, s, st, OH, OW).reshape(-1, C // cg, cg)
            dw[:, :, r, s] = torch.einsum("mgk,mgc->gkc", dyg, xs)
    return dw.reshape(C, 9 * cg)


def _id(c):
    return f"{c[0]}x{c[1]}s{c[2]}"


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_resnext50_conv2_forward(lib, shape):
    from imageclassification_amd import hip
    C, h, st = shape
    cg = C // GROUPS
    d = hip.conv_desc(N, h, h, C, C, 3, 3, st, 1)
    x = rnd((N, h, h, C), 1, relu=True)
    w = rnd((C, 3, 3, cg), 2, scale=(2.0 / (9 * cg)) ** 0.5)
    y = torch.full((N, d.OH, d.OW, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
    stats = torch.full((rows, 2, C), float("nan"), device=DEV)
    assert lib.icamd_gconv3x3_fwd(ctypes.byref(d), GROUPS, x.data_ptr(), w.data_ptr(), y.data_ptr(), stats.data_ptr(),
                                  hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    ref = ref_fwd(x, w, st, d.OH, d.OW).to(torch.bfloat16).float()
    idx = sample_rows(N * d.OH * d.OW, d.OH * d.OW, device=DEV)
    require(check_bf16(y.float().reshape(-1, C), ref, rows=idx), "grouped forward")
    assert bool(torch.isfinite(y.float()).all())
    require(check_stats(stats, y), "grouped forward statistics")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_resnext50_conv2_dgrad(lib, shape):
    from imageclassification_amd import hip
    C, h, st = shape
    cg = C // GROUPS
    d = hip.conv_desc(N, h, h, C, C, 3, 3, st, 1)
    dy = rnd((N, d.OH, d.OW, C), 3)
    w = rnd((C, 3, 3, cg), 4, scale=(1.0 / (9 * cg)) ** 0.5)
    dx = torch.full((N, h, h, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_gconv3x3_dgrad(ctypes.byref(d), GROUPS, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    ref = ref_dgrad(dy, w, st, h, h).to(torch.bfloat16).float()
    idx = sample_rows(N * h * h, h * h, device=DEV)
    require(check_bf16(dx.float().reshape(-1, C), ref, rows=idx), "grouped data gradient")
    assert bool(torch.isfinite(dx.float()).all())          # NaN-filled before: every element written


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_resnext50_conv2_wgrad(lib, shape):
    from imageclassification_amd import hip
    C, h, st = shape
    cg = C // GROUPS
    d = hip.conv_desc(N, h, h, C, C, 3, 3, st, 1)
    x = rnd((N, h, h, C), 5, relu=True)
    dy = rnd((N, d.OH, d.OW, C), 6)
    need = lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), GROUPS)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dw = torch.full((C, 9 * cg), float("nan"), device=DEV)
    assert lib.icamd_gconv3x3_wgrad(ctypes.byref(d), GROUPS, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), need,
                                    hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    require(check_fp32(dw, ref_wgrad(x, dy, st, cg)), "grouped weight gradient")       # every element
