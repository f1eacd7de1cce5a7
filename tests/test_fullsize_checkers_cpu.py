"""The full-size layer checkers (tests/_fullsize_check.py) can fail: on synthetic data shaped like a kernel output, each one
rejects a copy with one subtly wrong tile, one wrong row of the ragged last tile or one wrong in-tile row position, and
accepts the same operation accumulated in fp32 instead of fp64 (what a correct kernel differs by)."""
import pytest
import torch

from _fullsize_check import (check_arena, check_bf16, check_bits, check_close, check_counts, check_fold, check_fp32, check_pred,
                             check_stats, check_transposed, lowest_argmax, sample_rows)
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


# ---- the checkers of the full-size step tests (tests/test_fullsize_step_gpu.py) ----
def _adamw_fp32(p, g, m, v, lr, wd, t, gs, b1=0.9, b2=0.999, eps=1e-8):
    """The fused kernel's operation order in fp32 (what a correct kernel differs from the fp64 reference by)."""
    f = torch.float32
    g = g * torch.tensor(gs, dtype=f)
    p = p * torch.tensor(1.0 - lr * wd, dtype=f)
    m = m + (g - m) * torch.tensor(1.0 - b1, dtype=f)
    v = v * torch.tensor(b2, dtype=f) + torch.tensor(1.0 - b2, dtype=f) * g * g
    denom = v.sqrt() / torch.tensor((1.0 - b2 ** t) ** 0.5, dtype=f) + torch.tensor(eps, dtype=f)
    return p - torch.tensor(lr / (1.0 - b1 ** t), dtype=f) * (m / denom), m, v


def test_arena_checker_rejects_a_slice_left_out_or_applied_twice_in_30m_elements():
    n = 30 * (1 << 20)
    g = torch.Generator().manual_seed(11)
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) * 0.1 for _ in range(3)]
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in (1, 2):                                  # the state in front of step 3, as the GPU test builds it
        p, m, v = R.optimizer_step_f64("adamw", p, grads[t - 1], m, v, 2.5e-4, 4.9e-4, t, gscale=0.185)
    p, m, v = p.float(), m.float(), v.float()
    rp, rm, rv = R.optimizer_step_f64("adamw", p, grads[2], m, v, 5e-4, 4.8e-4, 3, gscale=0.185)
    kp, km, kv = _adamw_fp32(p, grads[2], m, v, 5e-4, 4.8e-4, 3, 0.185)
    bounds = ((kp, rp, 2e-5, 1e-6), (km, rm, 1e-5, 1e-7), (kv, rv, 1e-5, 1e-9))
    for got, ref, rtol, atol in bounds:
        assert check_arena(got, ref, rtol, atol) == []
    lo = n // 2 + 4096
    sl = slice(lo, lo + 1024)
    for got, ref, rtol, atol, old in ((kp, rp, 2e-5, 1e-6, p), (km, rm, 1e-5, 1e-7, m), (kv, rv, 1e-5, 1e-9, v)):
        bad = got.clone()
        bad[sl] = old[sl]                             # a stride that skipped one slice
        fails = check_arena(bad, ref, rtol, atol)
        assert fails and f"first [{lo}" in fails[0], fails
    twice = _adamw_fp32(kp[sl], grads[2][sl], km[sl], kv[sl], 5e-4, 4.8e-4, 3, 0.185)
    for (got, ref, rtol, atol), again in zip(bounds, twice):
        bad = got.clone()
        bad[sl] = again                               # a slice two workgroups both applied
        assert check_arena(bad, ref, rtol, atol) != []
    nan = kp.clone()
    nan[n - 1] = float("nan")
    assert check_arena(nan, rp, 2e-5, 1e-6) != []
    assert check_bits(kp, kp.clone()) == [] and check_bits(kp, -kp) != []
    z = torch.zeros(4)
    assert check_bits(z, -z) != []                    # -0 is not +0


def test_transpose_table_checker_rejects_a_swapped_tile_and_a_stray_write():
    g = torch.Generator().manual_seed(12)
    shapes = [(128, 9, 64), (256, 1, 192), (96, 4, 96)]
    shadow = torch.randn(sum(a * b * c for a, b, c in shapes) + 64, generator=g).to(torch.bfloat16)
    sentinel = -12345
    descs, soff, toff = [], 64, 0
    for co, t, ci in shapes:
        descs.append([soff, toff, co, t, ci, 0, 0, 0])
        soff += co * t * ci
        toff += co * t * ci + 128
    shadow_t = torch.full((toff,), sentinel, dtype=torch.int16).view(torch.bfloat16)
    for src, dst, co, t, ci, *_ in descs:
        shadow_t[dst:dst + co * t * ci] = shadow[src:src + co * t * ci].view(co, t, ci).permute(2, 1, 0).reshape(-1)
    assert check_transposed(shadow, shadow_t, descs, sentinel) == []
    bad = shadow_t.clone()
    v = bad[descs[1][1]:descs[1][1] + 256 * 192].view(192, 1, 256)
    tile = v[64:128, 0, 0:64].clone()
    v[64:128, 0, 0:64] = v[64:128, 0, 64:128]         # one 64 x 64 tile swapped with its neighbour
    v[64:128, 0, 64:128] = tile
    fails = check_transposed(shadow, bad, descs, sentinel)
    assert len(fails) == 1 and fails[0].startswith("desc 1"), fails
    bad = shadow_t.clone()
    bad[descs[0][1] + 128 * 9 * 64 + 5] = 1.0         # a write just behind a layer's slot
    assert any("outside" in f for f in check_transposed(shadow, bad, descs, sentinel))
    over = [list(d) for d in descs]
    over[1][1] = descs[0][1] + 64                     # two slots sharing elements
    assert check_transposed(shadow, shadow_t, over, sentinel) != []


def test_fold_checker_accepts_an_fp32_scale_and_rejects_a_fold_one_row_off():
    g = torch.Generator().manual_seed(13)
    co, k = 192, 768
    w = torch.randn(co, k, generator=g) * 0.05
    gamma, rv = torch.rand(co, generator=g) + 0.5, torch.rand(co, generator=g) + 0.5
    rv[::37] = 1e-6
    beta, rm = torch.randn(co, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1
    scale64 = gamma.double() / torch.sqrt(rv.double() + 1e-5)
    ref = w.double() * scale64[:, None]
    scale32 = gamma / torch.sqrt(rv + 1e-5)
    got = (w * scale32[:, None]).to(torch.bfloat16)
    assert check_fold(got, ref) == []
    off = got.clone()
    off[1:] = (w[1:] * scale32[:-1, None]).to(torch.bfloat16)     # every row scaled with its neighbour's coefficient
    assert check_fold(off, ref) != []
    one = got.clone()
    one[100] = (w[100] * scale32[99]).to(torch.bfloat16)
    assert check_fold(one, ref) != []
    two = got.float()
    two[64:128, 64:128] += 2 * torch.exp2(torch.floor(torch.log2(two[64:128, 64:128].abs())) - 7)   # 2 ulp in one tile
    assert check_fold(two.to(torch.bfloat16), ref) != []
    # the shift: rtol 1e-5 and an absolute term of 1e-6 of the two magnitudes it is the difference of
    shift64 = beta.double() - rm.double() * scale64
    atol = 1e-6 * (beta.abs() + (rm * scale32).abs())
    assert check_close(beta - rm * scale32, shift64, 1e-5, atol) == []
    assert check_close((beta - rm * scale32).roll(1), shift64, 1e-5, atol) != []


def test_prediction_and_count_checkers_reject_the_highest_tied_index_and_exchanged_counts():
    g = torch.Generator().manual_seed(14)
    B, C = 256, 1000
    x = (torch.randn(B, C, generator=g) * 3).to(torch.bfloat16)
    top = x.float().max(1).values + 1
    ties = [(5, 64 + 3), (7, 71), (0, C - 1)]
    for r in range(B):
        for c in ties[r % 3]:
            x[r, c] = top[r]
    low = torch.tensor([ties[r % 3][0] for r in range(B)])
    high = torch.tensor([ties[r % 3][1] for r in range(B)])
    assert torch.equal(lowest_argmax(x), low)
    assert check_pred(low.int(), x) == [] and check_pred(high.int(), x) != []
    one = low.clone()
    one[B - 1] = high[B - 1]
    assert check_pred(one.int(), x) != []
    target = torch.randint(0, C, (B,), generator=g)
    target[::3] = 7
    pred = torch.where(torch.rand(B, generator=g) < 0.6, target, torch.randint(0, C, (B,), generator=g))
    hit = pred == target
    counts = torch.stack([torch.bincount(target[hit], minlength=C), torch.bincount(pred[~hit], minlength=C),
                          torch.bincount(target[~hit], minlength=C)]).int()
    assert int(counts[0, 7]) > 20                     # the class whose atomics collide
    assert check_counts(counts, pred, target, C) == [] and check_counts(2 * counts, pred, target, C, times=2) == []
    assert check_counts(counts[[1, 0, 2]], pred, target, C) != []      # TP and FP exchanged
    assert check_counts(counts[[0, 2, 1]], pred, target, C) != []      # FP and FN exchanged
    short = counts.clone()
    short[0, 7] -= 1                                  # one lost increment on the crowded class
    assert check_counts(short, pred, target, C) != []
