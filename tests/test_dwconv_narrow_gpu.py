"""icamd_dwconv7_fwd / _dgrad / _wgrad / _wgrad_bias at widths that are no multiple of 32 (C % 8 == 0: the dims of ConvNeXt atto,
femto and nano) against oracle.ops_ref.dwconv7_fwd / dwconv7_bwd, with the bounds of
tests/test_kernels_gpu.py::test_dwconv7_fwd_dgrad_wgrad.

The weight gradient at these widths is dwconv7_wgrad_runs_kernel (csrc/dwconv.hip): a workgroup is `groups` = 256 / slice
(n, strip) items x `slice` channel pairs, slice = C / 2 or its largest divisor up to 256, the last 256 - groups * slice threads idle
(tests/_convnext_narrow.py::dw_wgrad_geometry mirrors it; tests/test_convnext_family_cpu.py asserts the counts below).  Its loops
whose trip count depends on the problem, and the case that runs each more than once:

  rows of the strip, first pass (base += 4) and second pass (base += 3)    (2, 29, 31, 40): 8 and 10 trips; every case with H > 4
  LDS outputs of a kernel row of taps (idx += 256 over 14 x slice)         (2, 14, 14, 40): 2 trips; (3, 33, 6, 200): 6; (2, 6, 6, 520): 8
  groups summed per output (g < groups)                                    (2, 14, 14, 40): 12; (70, 3, 5, 24): 21; (1, 1, 1, 8): 64
  LDS outputs of the bias row (idx += 256 over 2 x slice)                  (2, 6, 6, 520): 2 trips (slice 130)
  item blocks = partial rows the slab reducer folds                        (70, 3, 5, 24): 4; (3, 33, 6, 200): 2; (2, 6, 6, 520): 2
  channel slices per pixel (blockIdx.x % nslices)                          (2, 6, 6, 520): 2 slices of 130 pairs

The forward / data-gradient kernel is the one of the 32-multiple widths: its thread index is (t % (C / 2), strip, image), so a wave
spans 64 / (C / 2) strips ((1, 1, 1, 8): 4 pairs, the whole grid is 4 threads); (2, 29, 31, 40) splits the rows in two."""
import os
import subprocess
import sys

import pytest
import torch

import _harness
from _harness import dev as to_dev_bf16
from _harness import lib  # noqa: F401
from _harness import rnd_bf16, sync
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(2, 14, 14, 40), (3, 7, 7, 80), (2, 29, 31, 40), (5, 9, 8, 48), (1, 1, 1, 8), (70, 3, 5, 24), (3, 33, 6, 200), (2, 6, 6, 520),
          (2, 14, 14, 96)]


@pytest.mark.parametrize("shape", SHAPES)
def test_dwconv7_narrow_fwd_dgrad_wgrad(lib, shape):
    hip = _harness.hip()
    N, H, W, C = shape
    g = torch.Generator().manual_seed(130)
    x = rnd_bf16(N, H, W, C, seed=131)
    w = R.bf16_round(torch.randn(C, 7, 7, generator=g) * 0.15)
    bias = torch.randn(C, generator=g) * 0.1
    ry = R.dwconv7_fwd(x, w, bias)
    xd = to_dev_bf16(x)
    wd = to_dev_bf16(w.permute(1, 2, 0).contiguous())          # kernel layout [7][7][C]
    bd = bias.to(DEV)
    y = torch.full((N, H, W, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_dwconv7_fwd(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(y), N, H, W, C, hip.stream_ptr()) == 0
    sync()
    got = y.float().cpu()
    print(f"dwconv7 {shape}: y rel_l2 {R.rel_l2(got, ry):.2e}")
    assert R.rel_l2(got, ry) <= 1e-3 and R.bf16_close(got, ry)
    dy = rnd_bf16(N, H, W, C, seed=132)
    addend = rnd_bf16(N, H, W, C, seed=133)
    rdx, rdw = R.dwconv7_bwd(x, w, dy, addend)
    dyd, ad = to_dev_bf16(dy), to_dev_bf16(addend)
    dx = torch.full((N, H, W, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_dwconv7_dgrad(hip.ptr(dyd), hip.ptr(wd), hip.ptr(ad), hip.ptr(dx), N, H, W, C, hip.stream_ptr()) == 0
    wsb = lib.icamd_dwconv7_wgrad_workspace_bytes(N, H, W, C)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw = torch.full((7, 7, C), 1.0, device=DEV)
    assert lib.icamd_dwconv7_wgrad(hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw), 1, hip.ptr(ws), wsb, N, H, W, C, hip.stream_ptr()) == 0
    sync()
    print(f"dwconv7 {shape}: dx rel_l2 {R.rel_l2(dx.float().cpu(), rdx):.2e}, dw {R.rel_l2(dw.cpu(), 1.0 + rdw.permute(1, 2, 0)):.2e}")
    assert R.rel_l2(dx.float().cpu(), rdx) <= 1e-3 and R.bf16_close(dx.float().cpu(), rdx)
    assert R.rel_l2(dw.cpu(), 1.0 + rdw.permute(1, 2, 0)) <= 1e-4
    # filter and bias gradient out of one pass: wherever the rows form runs, which is every shape here
    assert lib.icamd_dwconv7_wgrad_bias_supported(N, H, W, C) == 1
    dw2 = torch.full((7, 7, C), float("nan"), device=DEV)
    db2 = torch.full((C,), float("nan"), device=DEV)
    rdb = dy.reshape(-1, C).double().sum(0).float()
    for acc, base in ((0, 0.0), (1, 1.0)):
        if acc:
            dw2.fill_(1.0); db2.fill_(1.0)
        assert lib.icamd_dwconv7_wgrad_bias(hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw2), hip.ptr(db2), acc, hip.ptr(ws), wsb, N, H, W, C,
                                            hip.stream_ptr()) == 0
        sync()
        assert R.rel_l2(dw2.cpu(), base + rdw.permute(1, 2, 0)) <= 1e-4
        assert torch.allclose(db2.cpu(), base + rdb, rtol=1e-5, atol=1e-4 * max(1.0, float(rdb.abs().max())))
    # two launches on the same inputs: the same bits (fixed-order sums, no float atomics)
    outs = []
    for _ in range(2):
        dw3 = torch.full((7, 7, C), float("nan"), device=DEV)
        db3 = torch.full((C,), float("nan"), device=DEV)
        ws.fill_(0x7F)
        assert lib.icamd_dwconv7_wgrad_bias(hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw3), hip.ptr(db3), 0, hip.ptr(ws), wsb, N, H, W, C,
                                            hip.stream_ptr()) == 0
        sync()
        outs.append((dw3, db3))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())


def _refusal(lib, N, H, W, C):
    """every entry refuses the shape; the sentinel outputs and the workspace stay as they were"""
    hip = _harness.hip()
    assert lib.icamd_dwconv7_wgrad_workspace_bytes(N, H, W, C) == 0
    assert lib.icamd_dwconv7_wgrad_bias_supported(N, H, W, C) == 0
    sent = 12345.0
    x = to_dev_bf16(rnd_bf16(N, H, W, C, seed=1))
    wd = to_dev_bf16(rnd_bf16(7, 7, C, seed=2))
    bd = torch.zeros(C, device=DEV)
    y = torch.full((N, H, W, C), sent, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((N, H, W, C), sent, dtype=torch.bfloat16, device=DEV)
    dw, db = torch.full((7, 7, C), sent, device=DEV), torch.full((C,), sent, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_dwconv7_fwd(hip.ptr(x), hip.ptr(wd), hip.ptr(bd), hip.ptr(y), N, H, W, C, s) != 0
    assert lib.icamd_dwconv7_dgrad(hip.ptr(x), hip.ptr(wd), hip.ptr(x), hip.ptr(dx), N, H, W, C, s) != 0
    assert lib.icamd_dwconv7_wgrad(hip.ptr(x), hip.ptr(x), hip.ptr(dw), 0, hip.ptr(ws), 1 << 20, N, H, W, C, s) != 0
    assert lib.icamd_dwconv7_wgrad_bias(hip.ptr(x), hip.ptr(x), hip.ptr(dw), hip.ptr(db), 0, hip.ptr(ws), 1 << 20, N, H, W, C, s) != 0
    sync()
    for t in (y, dx, dw, db):
        assert bool((t.float() == t.new_tensor(sent).float()).all())
    assert bool((ws == 7).all())


@pytest.mark.parametrize("C", [100, 12])
def test_width_that_is_no_multiple_of_8_is_refused(lib, C):
    _refusal(lib, 2, 9, 8, C)


def test_narrow_width_is_refused_by_the_lds_tile_form():
    """ICAMD_DWCONV_ROWS=0: the LDS-tile kernels work in 32-channel groups and are not built for narrower widths, so C = 40 is
    refused there before anything is written, and the model says so (child process: the switch is read once per process)."""
    if os.environ.get("ICAMD_DWCONV_ROWS") == "0":
        lib = _harness.load_lib()
        _refusal(lib, 2, 9, 8, 40)
        from imageclassification_amd.convnext import ConvNeXt
        net = ConvNeXt("convnext_test_narrow", 10)
        with pytest.raises(RuntimeError, match="no depthwise 7x7 kernel"):
            net.pack(torch.zeros(2, 3, 64, 64, device=DEV))
        return
    env = dict(os.environ, ICAMD_DWCONV_ROWS="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k",
                        "test_narrow_width_is_refused_by_the_lds_tile_form"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
