"""The ResNet-D kernels of csrc/conv_stem_deep.hip through the C ABI: the 2x2 average pool of the shortcut
(icamd_avgpool2x2_fwd / _bwd) and the thin 3x3 convolution of the deep stem (icamd_conv3x3_thin_*).

Pool: against F.avg_pool2d(2, 2, ceil_mode=True, count_include_pad=False) and its autograd in fp64 on bf16-rounded inputs.  The
arithmetic is exact up to the one rounding of the store, hence R.max_bf16_ulp <= 1.

Thin convolution: against R.conv2d_fwd / _dgrad / _wgrad under the bounds of tests/test_gconv_gpu.py (the same MFMA, fp32
accumulation and single rounding): bf16 outputs rel_l2 <= 1e-3 and R.bf16_close, fp32 dw rel_l2 <= 1e-4, statistics
allclose(rtol 1e-5, atol 1e-3) against the sums of the stored values, and through icamd_bn_train_finalize against
R.bn_train_coeffs under the bounds tests/test_fullsize_layers_gpu.py applies to that entry.

Every output is allocated with a guard band behind it that must come back untouched."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _harness
from _harness import UNSUPPORTED, dev, guarded, intact, rnd_bf16
from _harness import lib  # noqa: F401
from _thin_conv import run_dgrad, run_fwd, run_wgrad, thin_inputs
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAD_ARG = 1

# N, IH, IW, C
POOL_CASES = [(2, 8, 8, 64), (1, 7, 9, 32), (2, 5, 5, 8), (1, 1, 1, 8), (3, 15, 14, 256), (1, 2, 3, 1024)]
# N, H, W, Cout
THIN_CASES = [(2, 8, 8, 32), (1, 1, 1, 64), (1, 13, 17, 64), (1, 3, 40, 32), (2, 32, 32, 64), (3, 56, 40, 32), (1, 112, 112, 64),
              # wide images: the smaller tiles the LDS budget forces (Cout 64, W 200: 64-pixel data-gradient tiles on 61 KB of
              # LDS; Cout 32, W 400: 128-pixel tiles and 64-pixel weight-gradient tiles; W 450: 64-pixel tiles and 32-pixel
              # weight-gradient tiles)
              (1, 4, 200, 64), (1, 2, 400, 32), (1, 2, 450, 32)]


# ---------------------------------------------------------------------------------------------------------------- pool
def pool_ref(x, dout, addend):
    xt = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.avg_pool2d(xt, 2, 2, ceil_mode=True, count_include_pad=False)
    y.backward(dout.double().permute(0, 3, 1, 2))
    dx = xt.grad.permute(0, 2, 3, 1)
    return y.detach().permute(0, 2, 3, 1), dx, dx + addend.double()


@pytest.mark.parametrize("case", POOL_CASES)
def test_avgpool2x2_fwd_bwd(lib, case):
    hip = _harness.hip()
    N, IH, IW, C = case
    OH, OW = (IH + 1) // 2, (IW + 1) // 2
    x = rnd_bf16(N, IH, IW, C, seed=1)
    dout = rnd_bf16(N, OH, OW, C, seed=2)
    addend = rnd_bf16(N, IH, IW, C, seed=3)
    y64, dx64, dxa64 = pool_ref(x, dout, addend)
    xd, dd, ad = dev(x), dev(dout), dev(addend)
    s = hip.stream_ptr()
    out, g_out = guarded((N, OH, OW, C), torch.bfloat16)
    assert lib.icamd_avgpool2x2_fwd(hip.ptr(xd), hip.ptr(out), N, IH, IW, C, s) == 0
    assert intact(g_out)
    got = out.float().cpu()
    ulp = R.max_bf16_ulp(got, R.bf16_round(y64.float()))
    print(case, "pool fwd max ulp", ulp)
    assert torch.isfinite(got).all() and ulp <= 1.0
    out2, g2 = guarded((N, OH, OW, C), torch.bfloat16)
    assert lib.icamd_avgpool2x2_fwd(hip.ptr(xd), hip.ptr(out2), N, IH, IW, C, s) == 0
    assert intact(g2) and torch.equal(out.view(torch.int16), out2.view(torch.int16))
    for add_d, ref in ((None, dx64), (ad, dxa64)):
        dx, g_dx = guarded((N, IH, IW, C), torch.bfloat16)
        assert lib.icamd_avgpool2x2_bwd(hip.ptr(dd), hip.ptr(add_d), hip.ptr(dx), N, IH, IW, C, s) == 0
        assert intact(g_dx)
        gd = dx.float().cpu()
        ulp = R.max_bf16_ulp(gd, R.bf16_round(ref.float()))
        print(case, "pool bwd", "with addend" if add_d is not None else "plain", "max ulp", ulp)
        assert torch.isfinite(gd).all() and ulp <= 1.0      # dx was NaN-filled: every element is written
        dx2, g_dx2 = guarded((N, IH, IW, C), torch.bfloat16)
        assert lib.icamd_avgpool2x2_bwd(hip.ptr(dd), hip.ptr(add_d), hip.ptr(dx2), N, IH, IW, C, s) == 0
        assert intact(g_dx2) and torch.equal(dx.view(torch.int16), dx2.view(torch.int16))


def test_avgpool2x2_refuses_c12_and_writes_nothing(lib):
    hip = _harness.hip()
    N, IH, IW, C = 2, 6, 6, 12
    x = dev(rnd_bf16(N, IH, IW, 16, seed=1))
    out, g_out = guarded((N, IH, IW, 16), torch.bfloat16, fill=3.0)
    s = hip.stream_ptr()
    assert lib.icamd_avgpool2x2_fwd(hip.ptr(x), hip.ptr(out), N, IH, IW, C, s) == BAD_ARG
    assert lib.icamd_avgpool2x2_bwd(hip.ptr(x), None, hip.ptr(out), N, IH, IW, C, s) == BAD_ARG
    assert lib.icamd_avgpool2x2_bwd(hip.ptr(x), hip.ptr(x), hip.ptr(out), N, IH, IW, C, s) == BAD_ARG
    assert intact(g_out) and bool((out == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------- thin convolution
@pytest.mark.parametrize("case", THIN_CASES)
def test_thin_fwd_stats_and_act(lib, case):
    hip = _harness.hip()
    N, H, W, Cout = case
    d, x, w, dy, bias, ref = thin_inputs(case)
    assert lib.icamd_conv3x3_thin_supported(ctypes.byref(d)) == 1
    xd, wd = dev(x), dev(w)
    y = run_fwd(lib, d, xd, wd)
    got = y.float().cpu()
    print(case, "fwd rel_l2", R.rel_l2(got, ref["y"]))
    assert torch.isfinite(got).all()
    assert R.rel_l2(got, ref["y"]) <= 1e-3
    assert R.bf16_close(got, ref["y"])
    # with statistics: the same bytes; the partial rows sum to the sums of the stored values
    rows = lib.icamd_conv3x3_thin_stats_rows(ctypes.byref(d))
    assert rows > 0
    stats, gs = guarded((rows, 2, Cout), torch.float32)
    y2 = run_fwd(lib, d, xd, wd, stats=stats)
    assert intact(gs), "guard band behind the statistics written"
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16))
    stats_b, _ = guarded((rows, 2, Cout), torch.float32)
    assert torch.equal(run_fwd(lib, d, xd, wd, stats=stats_b).view(torch.int16), y.view(torch.int16))
    assert torch.equal(stats.view(torch.int32), stats_b.view(torch.int32))       # run to run
    assert torch.isfinite(stats).all()
    ssum = stats.cpu().double().sum(0)
    flat = got.double().reshape(-1, Cout)
    assert torch.allclose(ssum[0], flat.sum(0), rtol=1e-5, atol=1e-3)
    assert torch.allclose(ssum[1], (flat * flat).sum(0), rtol=1e-5, atol=1e-3)
    # ... and through the consumer of the contract
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    rm0, rv0 = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5
    gd, bd, rm, rv = gamma.to(DEV), beta.to(DEV), rm0.clone().to(DEV), rv0.clone().to(DEV)
    mean, invstd, scale, shift = (torch.empty(Cout, device=DEV) for _ in range(4))
    bws = torch.zeros(lib.icamd_bn_workspace_bytes(Cout), dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_train_finalize(hip.ptr(stats), rows, Cout, float(N * H * W), hip.ptr(gd), hip.ptr(bd), hip.ptr(rm),
                                       hip.ptr(rv), 0.1, 1e-5, hip.ptr(mean), hip.ptr(invstd), hip.ptr(scale), hip.ptr(shift),
                                       hip.ptr(bws), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    rmean, rinv, rscale, rshift, rrm, rrv = R.bn_train_coeffs(got, gamma, beta, rm0, rv0, 0.1, 1e-5)
    for name, a, b, rtol, atol in (("mean", mean, rmean, 1e-5, 1e-6), ("invstd", invstd, rinv, 1e-5, 0.0),
                                   ("scale", scale, rscale, 1e-5, 0.0), ("shift", shift, rshift, 1e-4, 1e-6),
                                   ("running_mean", rm, rrm, 1e-5, 1e-7), ("running_var", rv, rrv, 1e-5, 0.0)):
        assert torch.allclose(a.cpu(), b, rtol=rtol, atol=atol), name
    # folded-eval epilogue: bias, ReLU off and on, one rounding
    bd2 = bias.to(DEV)
    for relu, key in ((0, "z"), (1, "zr")):
        o = run_fwd(lib, d, xd, wd, bias=bd2, relu=relu).float().cpu()
        assert torch.isfinite(o).all()
        assert R.rel_l2(o, ref[key]) <= 1e-3
        assert R.bf16_close(o, ref[key])


@pytest.mark.parametrize("case", THIN_CASES)
def test_thin_dgrad(lib, case):
    d, x, w, dy, bias, ref = thin_inputs(case)
    dyd, wd = dev(dy), dev(w)
    dx = run_dgrad(lib, d, dyd, wd)
    got = dx.float().cpu()
    print(case, "dgrad rel_l2", R.rel_l2(got, ref["dx"]))
    assert torch.isfinite(got).all()         # dx was NaN-filled: every element is written
    assert R.rel_l2(got, ref["dx"]) <= 1e-3
    assert R.bf16_close(got, ref["dx"])
    assert torch.equal(dx.view(torch.int16), run_dgrad(lib, d, dyd, wd).view(torch.int16))


@pytest.mark.parametrize("case", THIN_CASES)
def test_thin_wgrad(lib, case):
    hip = _harness.hip()
    d, x, w, dy, bias, ref = thin_inputs(case)
    xd, dyd = dev(x), dev(dy)
    dw = run_wgrad(lib, d, xd, dyd)
    got = dw.cpu().double()
    print(case, "wgrad rel_l2", R.rel_l2(got, ref["dw"]))
    assert torch.isfinite(got).all()
    assert R.rel_l2(got, ref["dw"]) <= 1e-4
    assert torch.equal(dw.view(torch.int32), run_wgrad(lib, d, xd, dyd).view(torch.int32))       # fixed-order reduction
    old = torch.randn(d.Cout, 3, 3, 32, generator=torch.Generator().manual_seed(6))
    acc = run_wgrad(lib, d, xd, dyd, prefill=old.to(DEV))
    assert R.rel_l2(acc.cpu().double(), old.double() + ref["dw"].double()) <= 1e-4
    # a workspace one byte short is refused before anything is written
    need = lib.icamd_conv3x3_thin_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    sentinel = torch.full_like(dw, 7.0)
    rc = lib.icamd_conv3x3_thin_wgrad(ctypes.byref(d), hip.ptr(xd), hip.ptr(dyd), hip.ptr(sentinel), 0, hip.ptr(ws), need - 1,
                                      hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 3
    assert bool((sentinel == 7.0).all())


def test_thin_refusals_touch_nothing(lib):
    hip = _harness.hip()
    bad = [hip.conv_desc(2, 8, 8, 64, 64, 3, 3, 1, 1),      # Cin 64
           hip.conv_desc(2, 8, 8, 32, 32, 3, 3, 2, 1),      # stride 2
           hip.conv_desc(2, 8, 8, 32, 32, 3, 3, 1, 0),      # pad 0
           hip.conv_desc(2, 8, 8, 32, 48, 3, 3, 1, 1)]      # Cout 48
    for d in bad:
        assert lib.icamd_conv3x3_thin_supported(ctypes.byref(d)) == 0
        assert lib.icamd_conv3x3_thin_stats_rows(ctypes.byref(d)) == 0
        assert lib.icamd_conv3x3_thin_wgrad_workspace_bytes(ctypes.byref(d)) == 0
        big = 2 * 8 * 8 * 64
        x = torch.zeros(big, dtype=torch.bfloat16, device=DEV)
        w = torch.zeros(64 * 9 * 64, dtype=torch.bfloat16, device=DEV)
        y = torch.full((big,), 3.0, dtype=torch.bfloat16, device=DEV)
        dw = torch.full((64 * 9 * 64,), 3.0, device=DEV)
        st = torch.full((16 * 2 * 64,), 3.0, device=DEV)
        ws = torch.full((1 << 20,), 3, dtype=torch.uint8, device=DEV)
        s = hip.stream_ptr()
        assert lib.icamd_conv3x3_thin_fwd(ctypes.byref(d), hip.ptr(x), hip.ptr(w), hip.ptr(y), None, hip.ptr(st), 0, s) == UNSUPPORTED
        assert lib.icamd_conv3x3_thin_dgrad(ctypes.byref(d), hip.ptr(x), hip.ptr(w), hip.ptr(y), s) == UNSUPPORTED
        assert lib.icamd_conv3x3_thin_wgrad(ctypes.byref(d), hip.ptr(x), hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), 1 << 20,
                                            s) == UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((y == 3.0).all()) and bool((dw == 3.0).all()) and bool((st == 3.0).all()) and bool((ws == 3).all())
