"""The full-size layer checkers (tests/_fullsize_check.py) can fail: on synthetic data shaped like a kernel output, each one
rejects a copy with one subtly wrong tile, one wrong row of the ragged last tile or one wrong in-tile row position, and
accepts the same operation accumulated in fp32 instead of fp64 (what a correct kernel differs by)."""
import pytest
import torch

from _fullsize_check import check_bf16, check_fp32, check_stats, sample_rows
from oracle import ops_ref as R

ROWS_PER_IMAGE = 49          # 7 x 7 pixels: images straddle the 64-row tiles
N_IMG = 21
M = ROWS_PER_IMAGE * N_IMG   # 1029 rows: ragged last tile (1029 % 64 = 5)
K, C = 600, 192


@pytest.fixture(scope="module")
def gemm():
    """bf16 operands, output rounded to bf16 after fp64 (reference) and fp32 (a correct kernel) accumulation; the
    fp32 weight gradient dw = dy^T x likewise."""
    g = torch.Generator().manual_seed(5)
    x = R.bf16_round(torch.randn(M, K, generator=g)).clamp_min(0)
    w = R.bf16_round(torch.randn(C, K, generator=g) * K ** -0.5)
    ref = R.bf16_round(x.double() @ w.double().t())
    f32 = R.bf16_round(x @ w.t())
    dy = R.bf16_round(torch.randn(M, C, generator=g))
    dw_ref = dy.double().t() @ x.double()
    dw_f32 = (dy.t() @ x).float()
    assert not torch.equal(ref, f32)    # the accumulation order does move some roundings
    return ref, f32, dw_ref, dw_f32


def _corruptions(t):
    """(name, corrupted copy) for a 2-D output [rows, cols] with a ragged last 64-row tile."""
    rows = t.shape[0]
    last = rows - 1
    assert rows % 64 != 0
    out = []
    a = t.clone()
    a[128:192, 64:128] *= 1.01
    out.append(("block scaled by 1.01", a))
    a = t.clone()
    a[64:128, 0:64] *= -1
    out.append(("block sign flipped", a))
    a = t.clone()
    a[last] = 0
    out.append(("ragged last tile row zeroed", a))
    a = t.clone()
    a[(rows // 64) * 64 + 2] = 0
    out.append(("another ragged-tile row zeroed", a))
    a = t.clone()
    pos = torch.arange(17, rows, 64)
    a[pos] = t[pos - 1]          # in-tile row 17 of every tile holds row 16 (a wrong row offset in one lane group)
    out.append(("in-tile row 17 wrong in every tile", a))
    return out


def _sampled(rows_total, r):
    return sample_rows(rows_total, ROWS_PER_IMAGE, r=r)


@pytest.mark.parametrize("rows_per_image,n_img", [(197, 256), (49, 256), (3136, 16)])
def test_sample_covers_every_in_tile_position_and_the_edges(rows_per_image, n_img):
    rows = rows_per_image * n_img
    for r in (0, 7, 30):
        s = sample_rows(rows, rows_per_image, r=r)
        assert bool((s[1:] > s[:-1]).all()) and int(s[0]) >= 0 and int(s[-1]) < rows
        tiles = s // 32
        assert torch.equal(torch.unique(tiles), torch.arange(rows // 32 + (rows % 32 > 0)))  # every 32-row tile is hit
        for tile in (32, 64, 128, 256):
            assert set((s % tile).tolist()) == set(range(tile))                      # every in-tile position
        have = set(s.tolist())
        for i in (0, n_img // 2, n_img - 1):
            assert set(range(i * rows_per_image, (i + 1) * rows_per_image)) <= have


@pytest.mark.parametrize("sampled", [False, True])
def test_bf16_checker_accepts_fp32_accumulation(gemm, sampled):
    ref, f32, _, _ = gemm
    rows = _sampled(M, 3) if sampled else None
    assert check_bf16(f32, ref, rows=rows) == []


@pytest.mark.parametrize("sampled", [False, True])
def test_bf16_checker_rejects_each_corruption(gemm, sampled):
    ref, f32, _, _ = gemm
    rows = _sampled(M, 3) if sampled else None
    for name, bad in _corruptions(f32):
        assert check_bf16(bad, ref, rows=rows) != [], name


def test_bf16_checker_block_bound_catches_what_the_global_norm_misses(gemm):
    ref, f32, _, _ = gemm
    bad = f32.clone()
    bad[128:192, 64:128] *= 1.005
    assert R.rel_l2(bad, ref) <= 1e-3          # the global norm alone would pass it
    fails = check_bf16(bad, ref)
    assert any("blocks" in f for f in fails), fails


def test_fp32_checker_accepts_fp32_accumulation_and_rejects_each_corruption(gemm):
    _, _, dw_ref, dw_f32 = gemm
    assert check_fp32(dw_f32, dw_ref) == []
    assert check_fp32(dw_f32.t().contiguous(), dw_ref.t().contiguous()) == []   # [k, co] view: 600 rows, ragged 64-row tile
    for name, bad in _corruptions(dw_f32.t().contiguous()):
        assert check_fp32(bad, dw_ref.t().contiguous()) != [], name
    bad = dw_f32.clone()
    bad[64:128, 0:64] *= 1.01
    fails = check_fp32(bad, dw_ref)
    assert R.rel_l2(bad, dw_ref) <= 1e-2 and any("blocks" in f for f in fails), fails


def test_stats_checker(gemm):
    ref, f32, _, _ = gemm
    y = f32 + 0.25                              # not zero-mean
    y = R.bf16_round(y)
    nrows = (M + 127) // 128
    yp = torch.cat([y.double(), torch.zeros(nrows * 128 - M, C, dtype=torch.float64)]).reshape(nrows, 128, C)
    part32 = torch.stack([yp.float().sum(1), (yp.float() ** 2).sum(1)], 1)      # fp32 partial rows, as a kernel leaves them
    assert check_stats(part32, y) == []
    bad = part32.clone()
    bad[-1] = 0                                 # the ragged last row of partials dropped
    assert check_stats(bad, y) != []
    bad = part32.clone()
    bad[:, 0, 70] *= 1.0001                     # one channel's sums off by 1e-4
    assert check_stats(bad, y) != []
    bad = part32.clone()
    bad[5, 1] = part32[6, 1]                    # one partial row's second moment stored twice
    assert check_stats(bad, y) != []
    # the (sum g, sum g * y) form of the BatchNorm backward partials
    gw = R.bf16_round(torch.randn(M, C, generator=torch.Generator().manual_seed(9)))
    gp = torch.cat([gw.double(), torch.zeros(nrows * 128 - M, C, dtype=torch.float64)]).reshape(nrows, 128, C)
    partg = torch.stack([gp.sum(1), (gp * yp).sum(1)], 1).float()
    assert check_stats(partg, gw, weight=y) == []
    partg[3, 1, 5] *= 1.001
    assert check_stats(partg, gw, weight=y) != []
