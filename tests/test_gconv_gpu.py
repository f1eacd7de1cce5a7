"""Grouped 3x3 convolution kernels (csrc/conv_grouped.hip: icamd_gconv3x3_*) against torch.nn.functional.conv2d(groups=...)
and its autograd in fp64 on bf16-rounded inputs, rounded once where the kernel rounds.

Tolerances are the project's own (tests/test_kernels_gpu.py: test_conv_fwd_with_stats_bias_addend, test_conv_dgrad,
test_conv_wgrad): bf16 outputs rel_l2 <= 1e-3 and R.bf16_close; fp32 dw rel_l2 <= 1e-4; statistics allclose(rtol 1e-5,
atol 1e-3) against the sums of the values the kernel itself stored."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _harness
from _harness import dev, rnd_bf16, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"

# N, H, W, C, groups, stride
CASES = [
    (2, 8, 8, 128, 32, 1),
    (3, 9, 7, 128, 32, 1),
    (1, 5, 5, 64, 16, 1),
    (2, 12, 12, 256, 32, 2),
    (2, 13, 11, 256, 32, 2),
    (4, 28, 28, 256, 32, 1),
    (2, 14, 14, 512, 32, 1),
    (2, 15, 15, 512, 32, 2),
    (2, 7, 7, 1024, 32, 1),
    (2, 14, 14, 1024, 32, 2),
    (2, 8, 8, 256, 8, 1),
    # beyond the issue's list: Cg = 4 at stride 2, a half-filled last 64-channel slice (C = 96), wide images (64- and 32-pixel
    # sub-tiles, 32-pixel weight-gradient tiles)
    (2, 10, 9, 128, 32, 2),
    (3, 6, 6, 96, 3, 1),
    (1, 3, 120, 64, 4, 2),
    (1, 3, 130, 64, 4, 2),
    # the last stages of a 64 x 64 input: 4 x 4 -> 2 x 2 and 2 x 2 grids
    (8, 4, 4, 1024, 32, 2),
    (8, 2, 2, 1024, 32, 1),
    (8, 4, 4, 512, 32, 1),
]


def inputs(case):
    N, H, W, C, groups, st = case
    hip = _harness.hip()
    d = hip.conv_desc(N, H, W, C, C, 3, 3, st, 1)
    cg = C // groups
    x = rnd_bf16(N, H, W, C, seed=1)
    w = rnd_bf16(C, 3, 3, cg, scale=(1.0 / (9 * cg)) ** 0.5, seed=2)
    dy = rnd_bf16(N, d.OH, d.OW, C, seed=3)
    return d, x, w, dy


def ref_all(case, x, w, dy):
    """fp64 y (NHWC, unrounded), dx (NHWC), dw ([C][3][3][Cg])."""
    N, H, W, C, groups, st = case
    xt = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = w.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xt, wt, None, st, 1, 1, groups)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1).contiguous(), xt.grad.permute(0, 2, 3, 1).contiguous(),
            wt.grad.permute(0, 2, 3, 1).contiguous())


def run_fwd(lib, d, groups, xd, wd, stats=None):
    hip = _harness.hip()
    y = torch.full((d.N, d.OH, d.OW, d.Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.icamd_gconv3x3_fwd(ctypes.byref(d), groups, hip.ptr(xd), hip.ptr(wd), hip.ptr(y), hip.ptr(stats), hip.stream_ptr())
    assert rc == 0
    sync()
    return y


def run_dgrad(lib, d, groups, dyd, wd):
    hip = _harness.hip()
    dx = torch.full((d.N, d.IH, d.IW, d.Cin), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.icamd_gconv3x3_dgrad(ctypes.byref(d), groups, hip.ptr(dyd), hip.ptr(wd), hip.ptr(dx), hip.stream_ptr())
    assert rc == 0
    sync()
    return dx


def run_wgrad(lib, d, groups, xd, dyd, dw=None, accumulate=0):
    hip = _harness.hip()
    cg = d.Cin // groups
    if dw is None:
        dw = torch.full((d.Cin, 3, 3, cg), float("nan"), device=DEV)
    need = lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), groups)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.icamd_gconv3x3_wgrad(ctypes.byref(d), groups, hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw), accumulate, hip.ptr(ws),
                                  need, hip.stream_ptr())
    assert rc == 0
    sync()
    return dw


@pytest.mark.parametrize("case", CASES)
def test_gconv_fwd_stats_and_act(lib, case):
    hip = _harness.hip()
    N, H, W, C, groups, st = case
    d, x, w, dy = inputs(case)
    assert lib.icamd_gconv3x3_supported(ctypes.byref(d), groups) == 1
    y64, _, _ = ref_all(case, x, w, dy)
    ref = R.bf16_round(y64.float())
    xd, wd = dev(x), dev(w)
    got = run_fwd(lib, d, groups, xd, wd).float().cpu()
    print(case, "fwd rel_l2", R.rel_l2(got, ref))
    assert torch.isfinite(got).all()
    assert R.rel_l2(got, ref) <= 1e-3
    assert R.bf16_close(got, ref)
    # with statistics: same y, the partial rows sum to the sums of the stored values
    rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
    stats = torch.full((rows, 2, C), float("nan"), device=DEV)
    y2 = run_fwd(lib, d, groups, xd, wd, stats)
    assert torch.equal(y2, run_fwd(lib, d, groups, xd, wd))          # bit-identical with / without stats and run to run
    got2 = y2.float().cpu()
    assert torch.equal(got2, got)
    s = stats.cpu().double().sum(0)
    flat = got.double().reshape(-1, C)
    assert torch.isfinite(stats).all()
    assert torch.allclose(s[0], flat.sum(0), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[1], (flat * flat).sum(0), rtol=1e-5, atol=1e-3)
    # inference epilogue: bias, ReLU on and off, one rounding
    bias = torch.randn(C, generator=torch.Generator().manual_seed(4))
    bd = bias.to(DEV)
    for relu in (0, 1):
        z = y64 + bias.double()
        if relu:
            z = z.clamp_min(0)
        zr = R.bf16_round(z.float())
        out = torch.full((N, d.OH, d.OW, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        rc = lib.icamd_gconv3x3_fwd_act(ctypes.byref(d), groups, hip.ptr(xd), hip.ptr(wd), hip.ptr(out), hip.ptr(bd), relu,
                                        hip.stream_ptr())
        assert rc == 0
        sync()
        o = out.float().cpu()
        assert torch.isfinite(o).all()
        assert R.rel_l2(o, zr) <= 1e-3
        assert R.bf16_close(o, zr)


@pytest.mark.parametrize("case", CASES)
def test_gconv_dgrad(lib, case):
    N, H, W, C, groups, st = case
    d, x, w, dy = inputs(case)
    _, dx64, _ = ref_all(case, x, w, dy)
    ref = R.bf16_round(dx64.float())
    dyd, wd = dev(dy), dev(w)
    dx = run_dgrad(lib, d, groups, dyd, wd)
    got = dx.float().cpu()
    print(case, "dgrad rel_l2", R.rel_l2(got, ref))
    assert torch.isfinite(got).all()         # dx was NaN-filled: every element is written
    assert R.rel_l2(got, ref) <= 1e-3
    assert R.bf16_close(got, ref)
    assert torch.equal(dx, run_dgrad(lib, d, groups, dyd, wd))


@pytest.mark.parametrize("case", CASES)
def test_gconv_wgrad(lib, case):
    hip = _harness.hip()
    N, H, W, C, groups, st = case
    d, x, w, dy = inputs(case)
    _, _, dw64 = ref_all(case, x, w, dy)
    xd, dyd = dev(x), dev(dy)
    dw = run_wgrad(lib, d, groups, xd, dyd)
    got = dw.cpu().double()
    print(case, "wgrad rel_l2", R.rel_l2(got, dw64))
    assert torch.isfinite(got).all()
    assert R.rel_l2(got, dw64) <= 1e-4
    assert torch.equal(dw, run_wgrad(lib, d, groups, xd, dyd))       # fixed-order reduction
    acc = run_wgrad(lib, d, groups, xd, dyd, dw.clone(), accumulate=1)
    assert R.rel_l2(acc.cpu().double(), 2 * dw64) <= 1e-4
    # a workspace one byte short is refused before anything is written
    need = lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), groups)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    sentinel = torch.full_like(dw, 7.0)
    rc = lib.icamd_gconv3x3_wgrad(ctypes.byref(d), groups, hip.ptr(xd), hip.ptr(dyd), hip.ptr(sentinel), 0, hip.ptr(ws),
                                  need - 1, hip.stream_ptr())
    sync()
    assert rc == 3
    assert bool((sentinel == 7.0).all())


@pytest.mark.parametrize("case", [(2, 9, 7, 128, 32, 1), (2, 9, 8, 128, 32, 2), (2, 8, 8, 256, 32, 1), (2, 7, 7, 512, 32, 2),
                                  (1, 7, 7, 1024, 32, 1), (1, 8, 9, 1024, 32, 2)])
def test_gconv_no_leakage_between_groups(lib, case):
    N, H, W, C, groups, st = case
    cg = C // groups
    d, x, w, dy = inputs(case)
    g = 5
    lo, hi = g * cg, (g + 1) * cg
    other = torch.ones(C, dtype=torch.bool)
    other[lo:hi] = False
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    y0 = run_fwd(lib, d, groups, xd, wd)
    dx0 = run_dgrad(lib, d, groups, dyd, wd)
    dw0 = run_wgrad(lib, d, groups, xd, dyd)
    x2 = x.clone()
    x2[..., lo:hi] = rnd_bf16(N, H, W, cg, scale=3.0, seed=11)
    y1 = run_fwd(lib, d, groups, dev(x2), wd)
    assert torch.equal(y1[..., other], y0[..., other])
    assert not torch.equal(y1[..., lo:hi], y0[..., lo:hi])
    dy2 = dy.clone()
    dy2[..., lo:hi] = rnd_bf16(N, d.OH, d.OW, cg, scale=3.0, seed=12)
    dy2d = dev(dy2)
    dx1 = run_dgrad(lib, d, groups, dy2d, wd)
    assert torch.equal(dx1[..., other], dx0[..., other])
    assert not torch.equal(dx1[..., lo:hi], dx0[..., lo:hi])
    dw1 = run_wgrad(lib, d, groups, xd, dy2d)
    assert torch.equal(dw1[other], dw0[other])
    assert not torch.equal(dw1[lo:hi], dw0[lo:hi])


def expand_block_diagonal(w, groups):
    """[C][3][3][Cg] -> dense [C][3][3][C] with zeros outside the groups."""
    C, _, _, cg = w.shape
    full = torch.zeros(C, 3, 3, C)
    for g in range(groups):
        full[g * cg:(g + 1) * cg, :, :, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    return full


@pytest.mark.parametrize("case", [(2, 12, 12, 256, 32, 2), (4, 28, 28, 256, 32, 1), (2, 7, 7, 1024, 32, 1), (2, 9, 7, 128, 32, 1),
                                  (2, 15, 15, 512, 32, 2)])
def test_gconv_agrees_with_dense_emulation(lib, case):
    hip = _harness.hip()
    N, H, W, C, groups, st = case
    cg = C // groups
    d, x, w, dy = inputs(case)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    wfull = expand_block_diagonal(w, groups)
    wfd = dev(wfull)
    wftd = dev(wfull.permute(3, 1, 2, 0).contiguous())
    y_dense = torch.empty(N, d.OH, d.OW, C, dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_conv2d_fwd(ctypes.byref(d), hip.ptr(xd), hip.ptr(wfd), hip.ptr(y_dense), None, None, None, hip.stream_ptr()) == 0
    dx_dense = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_conv2d_dgrad(ctypes.byref(d), hip.ptr(dyd), hip.ptr(wftd), hip.ptr(dx_dense), None, None, hip.stream_ptr()) == 0
    need = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dw_dense = torch.empty(C, 3, 3, C, device=DEV)
    assert lib.icamd_conv2d_wgrad(ctypes.byref(d), hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw_dense), 0, hip.ptr(ws), need,
                                  hip.stream_ptr()) == 0
    sync()
    assert R.bf16_close(run_fwd(lib, d, groups, xd, wd).float().cpu(), y_dense.float().cpu())
    assert R.bf16_close(run_dgrad(lib, d, groups, dyd, wd).float().cpu(), dx_dense.float().cpu())
    dw = run_wgrad(lib, d, groups, xd, dyd).cpu()
    dwd = dw_dense.cpu()
    diag = torch.stack([dwd[c, :, :, (c // cg) * cg:(c // cg + 1) * cg] for c in range(C)])
    assert R.rel_l2(dw, diag) <= 1e-4


def test_gconv_refusals_touch_nothing(lib):
    hip = _harness.hip()
    bad = [
        (hip.conv_desc(2, 8, 8, 256, 256, 3, 3, 1, 1), 4),      # Cg = 64
        (hip.conv_desc(2, 8, 8, 128, 128, 1, 1, 1, 0), 32),     # 1x1
        (hip.conv_desc(2, 8, 8, 128, 256, 3, 3, 1, 1), 32),     # Cin != Cout
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 1, 1), 24),     # groups does not divide C
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 1, 0), 32),     # pad 0
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 3, 1), 32),     # stride 3
    ]
    for d, groups in bad:
        assert lib.icamd_gconv3x3_supported(ctypes.byref(d), groups) == 0
        assert lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), groups) == 0
        big = 2 * 8 * 8 * 256
        x = torch.zeros(big, dtype=torch.bfloat16, device=DEV)
        w = torch.zeros(256 * 9 * 256, dtype=torch.bfloat16, device=DEV)
        y = torch.full((big,), 3.0, dtype=torch.bfloat16, device=DEV)
        dw = torch.full((256 * 9 * 256,), 3.0, device=DEV)
        st = torch.full((16 * 2 * 256,), 3.0, device=DEV)
        ws = torch.full((1 << 20,), 3, dtype=torch.uint8, device=DEV)
        s = hip.stream_ptr()
        assert lib.icamd_gconv3x3_fwd(ctypes.byref(d), groups, hip.ptr(x), hip.ptr(w), hip.ptr(y), hip.ptr(st), s) == 2
        assert lib.icamd_gconv3x3_fwd_act(ctypes.byref(d), groups, hip.ptr(x), hip.ptr(w), hip.ptr(y), None, 1, s) == 2
        assert lib.icamd_gconv3x3_dgrad(ctypes.byref(d), groups, hip.ptr(x), hip.ptr(w), hip.ptr(y), s) == 2
        assert lib.icamd_gconv3x3_wgrad(ctypes.byref(d), groups, hip.ptr(x), hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), 1 << 20, s) == 2
        sync()
        assert bool((y == 3.0).all()) and bool((dw == 3.0).all()) and bool((st == 3.0).all()) and bool((ws == 3).all())
