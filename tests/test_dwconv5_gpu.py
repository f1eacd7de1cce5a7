"""icamd_dwconv5_fwd / _dgrad / _wgrad (csrc/dwconv5x5.hip) against F.conv2d(groups=C, padding=2) in fp64 on the same bf16 operands, at
stride 1 and 2, with the bounds of tests/test_dwconv3_gpu.py.

The shapes: an image smaller than the filter on both axes, a single row, odd sizes, OH = ceil(H / 2), C % 16 != 0 (24, 40), C % 32 != 0
(40, 48, 144), B0's widest 5x5 layer (1152), borders between images.  The loops of dwconv5_fwd_kernel / dwconv5_wgrad_kernel whose trip
count depends on the problem, and the shape that runs each more than once (tests/_dwconv.py::trips(..., k=5) mirrors the geometry;
tests/test_efficientnet_cpu.py asserts these counts):

  rows of a segment (oh), row segments                         (3, 37, 41, 40): 16 rows, 3 segments at stride 1, 2 at stride 2
  column groups                                                (2, 5, 5, 1152) at stride 1: 2 groups of 3 columns
  column lanes folded per output (l < lanes)                   every shape: 3 (C = 1152) .. 256 (C = 8)
  LDS outputs of the statistics fold (o += 256 over 16 cv)     (2, 14, 14, 144): 2 trips (cv 18); (2, 5, 5, 1152): 5 (cv 72)
  LDS outputs of a kernel row of taps (o += 256 over 40 cv)    (3, 9, 11, 48): cv 6, 1 trip; (2, 14, 14, 144): 3; (2, 5, 5, 1152): 12
  items of a workgroup (it < it1), forward and weight gradient (2100, 3, 5, 16): 2 / 5 at stride 1, 3 / 11 at stride 2
  channel slices per pixel (blockIdx.x % nslices)              (2, 5, 5, 1152): 2 slices of 72 vectors
  partial rows folded by icamd_bn_train_finalize / the slab reducer   every shape with more than one item"""
import pytest
import torch

import _dwconv as D
import _harness
from _harness import DEV, dev, guarded, intact, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

CASES = [(shape, stride) for shape in D.SHAPES5 for stride in (1, 2)]


def same_bits(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class Runner:
    """the entries on device tensors; outputs are guarded and NaN-filled, every call asserts its return code"""

    def __init__(self, lib, shape, stride):
        self.lib, self.hip, self.shape, self.stride = lib, _harness.hip(), shape, stride
        N, H, W, C = shape
        self.out_shape = (N, (H - 1) // stride + 1, (W - 1) // stride + 1, C)
        self.stats_rows = lib.icamd_dwconv5_stats_rows(N, H, W, C, stride)
        self.wsb = lib.icamd_dwconv5_wgrad_workspace_bytes(N, H, W, C, stride)

    def fwd(self, x, w55c, stats=False):
        hip, (N, H, W, C) = self.hip, self.shape
        y, gy = guarded(self.out_shape, torch.bfloat16)
        st, gs = guarded((self.stats_rows, 2, C), torch.float32) if stats else (None, None)
        rc = self.lib.icamd_dwconv5_fwd(hip.ptr(x), hip.ptr(w55c), hip.ptr(y), hip.ptr(st), N, H, W, C, self.stride, hip.stream_ptr())
        assert rc == 0, rc
        assert intact(gy), "guard band behind y written"
        assert gs is None or intact(gs), "guard band behind the statistics written"
        return y, st

    def dgrad(self, dy, w55c):
        hip, (N, H, W, C) = self.hip, self.shape
        dx, gx = guarded(self.shape, torch.bfloat16)
        assert self.lib.icamd_dwconv5_dgrad(hip.ptr(dy), hip.ptr(w55c), hip.ptr(dx), N, H, W, C, self.stride, hip.stream_ptr()) == 0
        assert intact(gx), "guard band behind dx written"
        return dx

    def wgrad(self, x, dy, base=None):
        """base None: accumulate = 0 into NaN; else accumulate = 1 onto `base`"""
        hip, (N, H, W, C) = self.hip, self.shape
        dw, gw = guarded((5, 5, C), torch.float32, fill=float("nan") if base is None else base)
        ws, gws = guarded((self.wsb,), torch.uint8, fill=0x7F)
        rc = self.lib.icamd_dwconv5_wgrad(hip.ptr(x), hip.ptr(dy), hip.ptr(dw), int(base is not None), hip.ptr(ws), self.wsb, N, H, W, C,
                                          self.stride, hip.stream_ptr())
        assert rc == 0, rc
        assert intact(gw), "guard band behind dw written"
        assert intact(gws), "guard band behind the workspace written"
        return dw


@pytest.mark.parametrize("shape,stride", CASES)
def test_dwconv5_fwd_dgrad_wgrad(lib, shape, stride):
    hip = _harness.hip()
    N, H, W, C = shape
    c = D.dw5_case(shape, stride)
    assert lib.icamd_dwconv5_supported(N, H, W, C, stride) == 1
    run = Runner(lib, shape, stride)
    assert run.stats_rows > 0 and run.wsb > 0
    xd, wd, dyd = dev(c["x"]), dev(c["w"].permute(1, 2, 0).contiguous()), dev(c["dy"])
    # forward, with statistics
    y, stats = run.fwd(xd, wd, stats=True)
    got = y.float().cpu()
    print(f"{shape} s{stride}: y rel_l2 {R.rel_l2(got, c['y']):.2e}")
    assert R.rel_l2(got, c["y"]) <= 1e-3 and R.bf16_close(got, c["y"])
    y0, _ = run.fwd(xd, wd, stats=False)
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
    dw = run.wgrad(xd, dyd, base=1.0)
    rdw = 1.0 + c["dw"].permute(1, 2, 0)
    print(f"{shape} s{stride}: dw rel_l2 {R.rel_l2(dw.cpu(), rdw):.2e}")
    assert R.rel_l2(dw.cpu(), rdw) <= 1e-4
    # two launches of every entry: the same bits
    y2, stats2 = run.fwd(xd, wd, stats=True)
    assert same_bits(y2, y) and same_bits(stats2, stats)
    assert same_bits(run.dgrad(dyd, wd), dx)
    assert same_bits(run.wgrad(xd, dyd, base=1.0), dw)
    dw0 = run.wgrad(xd, dyd)
    assert same_bits(run.wgrad(xd, dyd), dw0) and bool(torch.isfinite(dw0).all())


@pytest.mark.parametrize("N,H,W,C,stride", [(2, 7, 7, 20, 1), (2, 7, 7, 24, 3), (2, 7, 7, 24, 0)])
def test_unsupported_shapes_are_refused_with_nothing_written(lib, N, H, W, C, stride):
    hip = _harness.hip()
    assert lib.icamd_dwconv5_supported(N, H, W, C, stride) == 0
    assert lib.icamd_dwconv5_stats_rows(N, H, W, C, stride) == 0
    assert lib.icamd_dwconv5_wgrad_workspace_bytes(N, H, W, C, stride) == 0
    sent = 12288.0                                                               # on the bf16 grid
    x = torch.zeros(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    wd = torch.zeros(5, 5, C, dtype=torch.bfloat16, device=DEV)
    y = torch.full((N, H, W, C), sent, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((N, H, W, C), sent, dtype=torch.bfloat16, device=DEV)
    dw, stats = torch.full((5, 5, C), sent, device=DEV), torch.full((64, 2, C), sent, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_dwconv5_fwd(hip.ptr(x), hip.ptr(wd), hip.ptr(y), hip.ptr(stats), N, H, W, C, stride, s) != 0
    assert lib.icamd_dwconv5_wgrad(hip.ptr(x), hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), 1 << 20, N, H, W, C, stride, s) != 0
    assert lib.icamd_dwconv5_dgrad(hip.ptr(x), hip.ptr(wd), hip.ptr(dx), N, H, W, C, stride, s) != 0
    sync()
    for t in (y, dx, dw, stats):
        assert bool((t.float() == sent).all())
    assert bool((ws == 7).all())


def test_short_workspace_is_refused(lib):
    hip = _harness.hip()
    N, H, W, C = 2, 7, 7, 24
    x = torch.zeros(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    dw = torch.full((5, 5, C), 5.0, device=DEV)
    wsb = lib.icamd_dwconv5_wgrad_workspace_bytes(N, H, W, C, 1)
    ws = torch.full((wsb,), 7, dtype=torch.uint8, device=DEV)
    assert lib.icamd_dwconv5_wgrad(hip.ptr(x), hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), wsb - 1, N, H, W, C, 1, hip.stream_ptr()) == 3
    sync()
    assert bool((dw == 5.0).all()) and bool((ws == 7).all())
