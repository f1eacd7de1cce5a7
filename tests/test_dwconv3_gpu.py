"""icamd_dwconv3_fwd / _dgrad / _wgrad (csrc/dwconv3x3.hip) against F.conv2d(groups=C) in fp64 on the same bf16 operands, without
and with the on-load form a = relu6(x * scale + shift), at stride 1 and 2.

The shapes: odd sizes, OH = ceil(H / 2), a single row, C % 16 != 0 (24), C % 32 != 0 (48, 144, 528), C above 512, borders between
images.  The loops of dwconv3_fwd_kernel / dwconv3_wgrad_kernel whose trip count depends on the problem, and the shape that runs
each more than once (tests/_dwconv.py::trips mirrors the geometry; tests/test_mobilenetv2_cpu.py asserts these counts):

  rows of a segment (oh), row segments, column groups          (3, 57, 57, 96): 16 rows, 4 segments, 3 groups of 21 columns
  column lanes folded per output (l < lanes)                   every shape: 3 (C = 528, 1344) .. 128 (C = 16)
  LDS outputs of the statistics fold (o += 256 over 16 cv)     (2, 8, 8, 528): 5 trips (cv 66); (2, 14, 14, 144): 2
  LDS outputs of a kernel row of taps (o += 256 over 24 cv)    (3, 57, 57, 96): 2 trips (cv 12); (2, 8, 8, 528): 7
  items of a workgroup (it < it1), forward and weight gradient (2100, 3, 5, 16): 2 / 5 at stride 1, 3 / 11 at stride 2 -- the six
                                                               shapes of the issue stay below the row caps, this one passes them
  channel slices per pixel (blockIdx.x % nslices)              (2, 5, 5, 1344): 2 slices of 84 vectors
  partial rows folded by icamd_bn_train_finalize / the slab reducer   every shape with more than one item"""
import pytest
import torch

import _dwconv as D
import _harness
from _harness import DEV, guarded, intact, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

CASES = [(shape, stride, onload) for shape in D.SHAPES for stride in (1, 2) for onload in (False, True)]


def same_bits(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("shape,stride,onload", CASES)
def test_dwconv3_fwd_dgrad_wgrad(lib, shape, stride, onload):
    hip = _harness.hip()
    N, H, W, C = shape
    c = D.case(shape, stride, bool(onload))
    if onload:   # a condition on the inputs: without it ReLU6 is ReLU and a padded tap of relu6(shift) would go unseen
        at6, at0 = D.clamp_shares(c["a"])
        print(f"{shape} s{stride}: {at6:.1%} of the activated input at 6, {at0:.1%} at 0")
        assert at6 >= 0.02 and at0 >= 0.20 and float(c["shift"].max()) > 1.0
    assert lib.icamd_dwconv3_supported(N, H, W, C, stride) == 1
    run = D.Runner(lib, shape, stride)
    assert run.stats_rows > 0 and run.wsb > 0
    xd, wd, dyd, scd, shd = D.device_operands(c)
    # forward, with statistics
    y, stats = run.fwd(xd, wd, scd, shd, stats=True)
    got = y.float().cpu()
    print(f"{shape} s{stride} onload={onload}: y rel_l2 {R.rel_l2(got, c['y']):.2e}")
    assert R.rel_l2(got, c["y"]) <= 1e-3 and R.bf16_close(got, c["y"])
    y0, _ = run.fwd(xd, wd, scd, shd, stats=False)
    assert same_bits(y0, y)                                                      # the statistics do not change y
    # partial rows against fp64 sums of the kernel's own stored y, then through the consumer of the contract
    assert bool(torch.isfinite(stats).all())
    ssum = stats.cpu().double().sum(0)
    flat = got.double().reshape(-1, C)
    assert torch.allclose(ssum[0], flat.sum(0), rtol=1e-5, atol=1e-3)
    assert torch.allclose(ssum[1], (flat * flat).sum(0), rtol=1e-5, atol=1e-3)
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    gd, bd, rm, rv = gamma.to(DEV), beta.to(DEV), rm0.clone().to(DEV), rv0.clone().to(DEV)
    mean, invstd, scale, shift = (torch.empty(C, device=DEV) for _ in range(4))
    bws = torch.zeros(lib.icamd_bn_workspace_bytes(C), dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_train_finalize(hip.ptr(stats), run.stats_rows, C, float(flat.shape[0]), hip.ptr(gd), hip.ptr(bd), hip.ptr(rm),
                                       hip.ptr(rv), 0.1, 1e-5, hip.ptr(mean), hip.ptr(invstd), hip.ptr(scale), hip.ptr(shift),
                                       hip.ptr(bws), hip.stream_ptr()) == 0
    sync()
    rmean, rinv, rscale, rshift, rrm, rrv = R.bn_train_coeffs(got, gamma, beta, rm0, rv0, 0.1, 1e-5)
    for name, a, b, rtol, atol in (("mean", mean, rmean, 1e-5, 1e-6), ("invstd", invstd, rinv, 1e-5, 0.0),
                                   ("scale", scale, rscale, 1e-5, 0.0), ("shift", shift, rshift, 1e-4, 1e-6),
                                   ("running_mean", rm, rrm, 1e-5, 1e-7), ("running_var", rv, rrv, 1e-5, 0.0)):
        assert torch.allclose(a.cpu(), b, rtol=rtol, atol=atol), name
    # data gradient: every element of dx written (the NaN fill is gone), once per launch
    dx = run.dgrad(dyd, wd)
    gdx = dx.float().cpu()
    print(f"{shape} s{stride}: dx rel_l2 {R.rel_l2(gdx, c['dx']):.2e}")
    assert R.rel_l2(gdx, c["dx"]) <= 1e-3 and R.bf16_close(gdx, c["dx"])
    # weight gradient, accumulated onto a non-zero base
    dw = run.wgrad(xd, dyd, scd, shd, base=1.0)
    rdw = 1.0 + c["dw"].permute(1, 2, 0)
    print(f"{shape} s{stride} onload={onload}: dw rel_l2 {R.rel_l2(dw.cpu(), rdw):.2e}")
    assert R.rel_l2(dw.cpu(), rdw) <= 1e-4
    # two launches of every entry: the same bits
    y2, stats2 = run.fwd(xd, wd, scd, shd, stats=True)
    assert same_bits(y2, y) and same_bits(stats2, stats)
    assert same_bits(run.dgrad(dyd, wd), dx)
    assert same_bits(run.wgrad(xd, dyd, scd, shd, base=1.0), dw)
    dw0 = run.wgrad(xd, dyd, scd, shd)
    assert same_bits(run.wgrad(xd, dyd, scd, shd), dw0) and bool(torch.isfinite(dw0).all())


@pytest.mark.parametrize("shape,stride", [(shape, stride) for shape in D.SHAPES for stride in (1, 2)])
def test_onload_form_equals_apply_then_plain(lib, shape, stride):
    """forward (y and statistics) and weight gradient on the raw tensor with scale / shift == icamd_bn_apply_relu6 followed by the
    plain call, bit for bit; and the applied tensor is the reference's"""
    hip = _harness.hip()
    N, H, W, C = shape
    c = D.case(shape, stride, True)
    run = D.Runner(lib, shape, stride)
    xd, wd, dyd, scd, shd = D.device_operands(c)
    a, ga = guarded(shape, torch.bfloat16)
    assert lib.icamd_bn_apply_relu6(hip.ptr(xd), hip.ptr(scd), hip.ptr(shd), hip.ptr(a), xd.numel(), C, hip.stream_ptr()) == 0
    assert intact(ga)
    assert torch.equal(a.float().cpu(), c["a"])
    y_on, st_on = run.fwd(xd, wd, scd, shd, stats=True)
    y_pl, st_pl = run.fwd(a, wd, stats=True)
    assert same_bits(y_on, y_pl) and same_bits(st_on, st_pl)
    assert same_bits(run.wgrad(xd, dyd, scd, shd), run.wgrad(a, dyd))


@pytest.mark.parametrize("N,H,W,C,stride", [(2, 7, 7, 20, 1), (2, 7, 7, 24, 3), (2, 7, 7, 12, 2), (2, 7, 7, 24, 0)])
def test_unsupported_shapes_are_refused_with_nothing_written(lib, N, H, W, C, stride):
    hip = _harness.hip()
    assert lib.icamd_dwconv3_supported(N, H, W, C, stride) == 0
    assert lib.icamd_dwconv3_stats_rows(N, H, W, C, stride) == 0
    assert lib.icamd_dwconv3_wgrad_workspace_bytes(N, H, W, C, stride) == 0
    sent = 12288.0                                                               # on the bf16 grid
    x = torch.zeros(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    wd = torch.zeros(3, 3, C, dtype=torch.bfloat16, device=DEV)
    sc = torch.ones(C, device=DEV)
    y = torch.full((N, H, W, C), sent, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((N, H, W, C), sent, dtype=torch.bfloat16, device=DEV)
    dw, stats = torch.full((3, 3, C), sent, device=DEV), torch.full((64, 2, C), sent, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    s = hip.stream_ptr()
    for scp in (None, hip.ptr(sc)):
        assert lib.icamd_dwconv3_fwd(hip.ptr(x), scp, scp, hip.ptr(wd), hip.ptr(y), hip.ptr(stats), N, H, W, C, stride, s) != 0
        assert lib.icamd_dwconv3_wgrad(hip.ptr(x), scp, scp, hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), 1 << 20, N, H, W, C, stride, s) != 0
    assert lib.icamd_dwconv3_dgrad(hip.ptr(x), hip.ptr(wd), hip.ptr(dx), N, H, W, C, stride, s) != 0
    sync()
    for t in (y, dx, dw, stats):
        assert bool((t.float() == sent).all())
    assert bool((ws == 7).all())


def test_half_given_coefficients_and_short_workspace_are_refused(lib):
    hip = _harness.hip()
    N, H, W, C = 2, 7, 7, 24
    x = torch.zeros(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    wd = torch.zeros(3, 3, C, dtype=torch.bfloat16, device=DEV)
    sc = torch.ones(C, device=DEV)
    y = torch.full((N, H, W, C), 5.0, dtype=torch.bfloat16, device=DEV)
    dw = torch.full((3, 3, C), 5.0, device=DEV)
    wsb = lib.icamd_dwconv3_wgrad_workspace_bytes(N, H, W, C, 1)
    ws = torch.full((wsb,), 7, dtype=torch.uint8, device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_dwconv3_fwd(hip.ptr(x), hip.ptr(sc), None, hip.ptr(wd), hip.ptr(y), None, N, H, W, C, 1, s) == 1
    assert lib.icamd_dwconv3_wgrad(hip.ptr(x), None, hip.ptr(sc), hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), wsb, N, H, W, C, 1, s) == 1
    assert lib.icamd_dwconv3_wgrad(hip.ptr(x), None, None, hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), wsb - 1, N, H, W, C, 1, s) == 3
    sync()
    assert bool((y.float() == 5.0).all()) and bool((dw == 5.0).all()) and bool((ws == 7).all())
