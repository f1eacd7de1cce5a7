"""The checks of tests/test_multitrip_gpu.py can fail, and its cases are multi-trip: on reference data (no GPU), each fault that a
grid-capped loop can have on its second and later trips is applied to a correct output and must be rejected by the check that is
there for it, while the unperturbed output passes.  The Python mirrors of the launch planners (tests/_multitrip.py) must give the
trip counts the cases were chosen for.

A "correct output" is the fp64 reference rounded the way the kernel stores it (bf16 outputs) or summed in fp32 (fp32 sums).
Where a plan depends on the number of heads or samples only through a cap, the data holds a few heads / samples of the case and the
plan is that of the whole case: every head and every sample is walked the same way."""
import pytest
import torch

import _multitrip as MT
from _fullsize_check import check_bf16, check_fp32, check_stats
from oracle.swin_ref import patch_merge_gather, patch_merge_ln_ref, window_attention_ref
from oracle import ops_ref as R

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------- planners
@pytest.mark.parametrize("case,want", list(MT.WINATTN_CASES.items()))
def test_window_attention_cases_are_multitrip(case, want):
    B, Hs, Ws, H, ws, shift = case
    nwin = MT.winattn_nwin(B, Hs, Ws, ws)
    gf, gb = MT.winattn_fwd_grid(nwin, H), MT.winattn_bwd_grid(nwin, H)
    assert (MT.winattn_trips(nwin, gf), MT.winattn_trips(nwin, gb)) == want
    assert 4 * gb < nwin and nwin % (4 * gb) != 0                  # backward: capped, ragged last trip
    if want[0] > 1:
        assert 4 * gf < nwin and nwin % (4 * gf) != 0


def test_window_attention_ragged_trip_is_the_one_described():
    """(45, 14, 21, 32, 7, 3): 270 windows in 68 chunks; forward grid 64, backward grid 32; on the last trip workgroups 0-2 are
    fully live, workgroup 3 has two live and two dead waves, every other workgroup is dead"""
    nwin = MT.winattn_nwin(45, 14, 21, 7)
    assert nwin == 270 and MT.cdiv(nwin, 4) == 68
    for grid, trips in ((MT.winattn_fwd_grid(nwin, 32), 2), (MT.winattn_bwd_grid(nwin, 32), 3)):
        assert grid == (64 if trips == 2 else 32)
        live = [sum(1 for w in range(4) if ((trips - 1) * grid + b) * 4 + w < nwin) for b in range(grid)]
        assert live[:4] == [4, 4, 4, 2] and not any(live[4:])


@pytest.mark.parametrize("case,want", list(MT.PATCH_MERGE_CASES.items()))
def test_patch_merge_cases_are_multitrip(case, want):
    N, H, W, C = case
    rows = MT.patch_merge_rows(N, H, W)
    gf, gb = MT.patch_merge_fwd_grid(rows), MT.patch_merge_bwd_grid(rows)
    assert (MT.patch_merge_trips(rows, gf), MT.patch_merge_trips(rows, gb)) == want
    assert 4 * gb < rows and rows % (4 * gb) != 0
    assert MT.patch_merge_sum_depth(rows) == want[1] + 4 + 512


def test_patch_merge_second_forward_trip_has_512_rows():
    rows = MT.patch_merge_rows(34, 32, 32)
    assert rows == 8704 and rows - 4 * MT.patch_merge_fwd_grid(rows) == 512


@pytest.mark.parametrize("case,want", list(MT.SE_CASES.items()))
def test_se_cases_take_the_paths_they_are_there_for(case, want):
    N, HW, C, rd = case
    S, rps = MT.se_plan(N, HW)
    blocks = MT.se_blocks_per_sample(N, HW, C // 8)
    trips, last = MT.se_apply_trips(N, HW, C // 8)
    assert (S, rps, blocks, trips) == want
    assert (blocks * 256) % (C // 8) == 0                          # what keeps a thread on one channel group
    if N == 256:
        assert S == MT.cdiv(2048, N) and S < MT.cdiv(HW, 32)       # limited by N, not by HW / 32
        assert HW - (S - 1) * rps == 30                            # short last segment
    if case == (256, 289, 64, 8):
        assert last == 264
    if case == (256, 289, 192, 12):
        assert blocks * 256 == 96 * 24 and last == 24 and MT.se_jw(rd) == 8
    if C == 4096:
        assert C // 8 > 256                                        # second cg0 trip of se_reduce_kernel


@pytest.mark.parametrize("case,want", list(MT.THIN_CASES.items()))
def test_thin_cases_are_multitrip(case, want):
    N, H, W, Cout = case
    sbf, sbd, ntiles, sbw, ntw, S, tps = MT.thin_plan(N, H, W, Cout)
    assert (sbf, ntiles, sbw, ntw, S, tps) == want and sbd == sbf
    assert ntiles > 2 * 304                                        # more tiles than 2 x CUs of the largest card
    assert S < ntw and tps >= 3 and ntw % tps != 0                 # several tiles per split, short last split
    assert (N * H * W) % sbf != 0 and (N * H * W) % sbw != 0       # ragged last tile


# ---------------------------------------------------------------------------------------------------------------- window attention
WA_CASE = (45, 14, 21, 32, 7, 3)
WA_HEADS = 2                    # heads of data; the plan is that of the case's 32


@pytest.fixture(scope="module")
def winattn():
    B, Hs, Ws, H, ws, shift = WA_CASE
    g = torch.Generator().manual_seed(31)
    rows = B * Hs * Ws
    qkv = R.bf16_round(torch.randn(rows, 3 * WA_HEADS * 32, generator=g))
    dout = R.bf16_round(torch.randn(rows, WA_HEADS * 32, generator=g))
    bias = torch.randn(WA_HEADS, ws * ws, ws * ws, generator=g) * 0.5
    out, lse, dqkv, dbias = window_attention_ref(qkv, bias, B, Hs, Ws, WA_HEADS, ws, shift, dout=dout)
    nwin = MT.winattn_nwin(B, Hs, Ws, ws)
    tokwin = MT.winattn_token_window(B, Hs, Ws, ws, shift)
    # which token rows belong to windows of the LAST trip, forward and backward
    late = {}
    for name, grid in (("fwd", MT.winattn_fwd_grid(nwin, H)), ("bwd", MT.winattn_bwd_grid(nwin, H))):
        trip = MT.winattn_window_trip(nwin, grid)
        late[name] = (trip == trip.max())[tokwin]
        assert 0 < int(late[name].sum()) == (nwin - 4 * grid * int(trip.max())) * ws * ws
    # dbias without the last backward trip: those windows' dO zeroed (dP = delta = 0 there, so their dS vanishes)
    dout_cut = dout.clone()
    dout_cut[late["bwd"]] = 0
    dbias_cut = window_attention_ref(qkv, bias, B, Hs, Ws, WA_HEADS, ws, shift, dout=dout_cut)[3]
    return {"out": out.reshape(rows, -1), "dqkv": dqkv.reshape(rows, -1), "dbias": dbias, "dbias_cut": dbias_cut, "late": late}


def _wa_out_check(got, ref):
    return check_bf16(got, ref, rel=3e-3, block_rel=3e-3, atol_rms=8e-3, max_frac=1e-6)


def _wa_grad_check(got, ref):
    return [f for f in check_bf16(got, ref, rel=6e-3, block_rel=6e-3) if "elementwise" not in f]


def test_token_window_map_is_the_references(winattn):
    """winattn_token_window against window_partition of the rolled grid (what the reference does)"""
    from oracle.swin_ref import window_partition
    B, Hs, Ws, H, ws, shift = WA_CASE
    ids = torch.arange(B * Hs * Ws).view(B, Hs, Ws, 1)
    rolled = torch.roll(ids, shifts=(-shift, -shift), dims=(1, 2))
    per_window = window_partition(rolled, ws).view(-1, ws * ws)            # [nwin, T] token rows
    tokwin = MT.winattn_token_window(B, Hs, Ws, ws, shift)
    assert torch.equal(tokwin[per_window], torch.arange(per_window.shape[0])[:, None].expand_as(per_window))


def test_window_attention_checks_reject_unwritten_later_trips(winattn):
    out, dqkv = R.bf16_round(winattn["out"].float()), R.bf16_round(winattn["dqkv"].float())
    assert _wa_out_check(out, winattn["out"]) == []
    assert _wa_grad_check(dqkv, winattn["dqkv"]) == []
    for fill in (float("nan"), 0.0):
        bad = out.clone()
        bad[winattn["late"]["fwd"]] = fill
        assert _wa_out_check(bad, winattn["out"]) != [], fill
        bad = dqkv.clone()
        bad[winattn["late"]["bwd"]] = fill
        assert _wa_grad_check(bad, winattn["dqkv"]) != [], fill
    # one head of one late window is enough: the 64 x 64 blocks hold two heads of about one window
    rows = torch.nonzero(winattn["late"]["fwd"]).flatten()[:49]
    bad = out.clone()
    bad[rows, 32:64] = 0
    fails = _wa_out_check(bad, winattn["out"])
    assert any("blocks" in f for f in fails), fails


def test_dbias_check_rejects_a_missing_last_trip(winattn):
    T = WA_CASE[4] ** 2
    ref = winattn["dbias"].reshape(-1, T)
    assert check_fp32(ref.float(), ref, rel=6e-3, block_rel=6e-3) == []
    assert check_fp32(winattn["dbias_cut"].reshape(-1, T).float(), ref, rel=6e-3, block_rel=6e-3) != []


# ---------------------------------------------------------------------------------------------------------------- patch merging
def test_dgamma_dbeta_checks_reject_sums_of_each_waves_first_row_only():
    N, H, W, C = 9, 32, 34, 8
    rows = MT.patch_merge_rows(N, H, W)
    P = MT.patch_merge_bwd_grid(rows)
    g = torch.Generator().manual_seed(32)
    x = R.bf16_round(torch.randn(N, H, W, C, generator=g) * 2 + 0.5)
    gamma, beta = torch.rand(4 * C, generator=g) + 0.5, torch.randn(4 * C, generator=g) * 0.2
    dy = R.bf16_round(torch.randn(rows, 4 * C, generator=g))
    _, mean, rstd, _, rdg, rdb = patch_merge_ln_ref(x, gamma, beta, 1e-5, dy=dy)
    xhat = (patch_merge_gather(x.double()) - mean[:, None]) * rstd[:, None]
    tg, tb = dy.double() * xhat, dy.double()
    assert torch.allclose(tg.sum(0), rdg) and torch.allclose(tb.sum(0), rdb)
    depth = MT.patch_merge_sum_depth(rows)
    # a correct kernel: the same terms summed in fp32
    for terms, ref, what in ((tg, rdg, "dgamma"), (tb, rdb, "dbeta")):
        good = terms.float().sum(0)
        assert MT.check_fp32_sum(good, ref, terms.abs().sum(0), depth, what) == []
        assert R.rel_l2(good, ref) <= 1e-4
        # wave (b, w) of the 4 P waves sees rows 4 b + w, 4 b + w + 4 P, ...: only the first of them summed
        first = terms[:4 * P].float().sum(0)
        assert MT.check_fp32_sum(first, ref, terms.abs().sum(0), depth, what) != []
        assert R.rel_l2(first, ref) > 1e-4
        # one row of the second trip missing: the elementwise bound is the check that sees it
        one = (terms.sum(0) - terms[4 * P + 5]).float()
        assert MT.check_fp32_sum(one, ref, terms.abs().sum(0), depth, what) != []


# ---------------------------------------------------------------------------------------------------------------- SE
def test_se_out_check_rejects_a_drifting_channel_group():
    """(256, 289, 192, 12): four samples of it.  On trips >= 2 the thread's channel group is taken one too high."""
    N_plan, HW, C, rd = 256, 289, 192, 12
    N, cpr = 4, C // 8
    g = torch.Generator().manual_seed(33)
    y = R.bf16_round(torch.randn(N, HW, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g))
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    e = torch.sigmoid(torch.randn(N, C, generator=g) * 1.5)
    res = R.bf16_round(torch.randn(N, HW, C, generator=g))

    def apply(sc, sh, ee, dt):
        return R.bf16_round(torch.relu((y.to(dt) * sc.to(dt) + sh.to(dt)) * ee.to(dt) + res.to(dt)).float())

    ref = apply(scale, shift, e[:, None, :], F64).reshape(N * HW, C)       # rounded once, as the reference of the GPU test
    good = apply(scale, shift, e[:, None, :], torch.float32)               # a correct kernel: the same chain in fp32
    assert check_bf16(good.reshape(N * HW, C), ref, rel=1e-3) == [] and R.max_bf16_ulp(good, ref) <= 1.0
    roll = lambda t: t.reshape(*t.shape[:-1], cpr, 8).roll(-1, -2).reshape(t.shape)   # noqa: E731  group g <- group g + 1
    drift = apply(roll(scale), roll(shift), roll(e)[:, None, :], torch.float32)
    late = MT.se_later_trip_vectors(N_plan, HW, cpr).view(HW, cpr)
    assert 0 < int(late.sum()) < HW * cpr
    bad = torch.where(late[None, :, :, None].expand(N, HW, cpr, 8).reshape(N, HW, C), drift, good).reshape(N * HW, C)
    fails = check_bf16(bad, ref, rel=1e-3)
    assert any("blocks" in f for f in fails), fails
    # only the LAST trip (24 vectors = one pixel's row per sample): the global norm no longer sees it, the block term does
    last = torch.zeros(HW * cpr, dtype=torch.bool)
    last[-MT.se_apply_trips(N_plan, HW, cpr)[1]:] = True
    bad = torch.where(last.view(1, HW, cpr, 1).expand(N, HW, cpr, 8).reshape(N, HW, C), drift, good).reshape(N * HW, C)
    fails = check_bf16(bad, ref, rel=1.0)
    assert any("blocks" in f for f in fails), fails


# ---------------------------------------------------------------------------------------------------------------- thin 3x3
@pytest.fixture(scope="module")
def thin():
    N, H, W, Cout = case = (7, 111, 113, 64)
    x = R.bf16_round(torch.randn(N, H, W, 32, generator=torch.Generator().manual_seed(34)))
    w = R.bf16_round(torch.randn(Cout, 3, 3, 32, generator=torch.Generator().manual_seed(35)) * (1.0 / 288) ** 0.5)
    dy = R.bf16_round(torch.randn(N, H, W, Cout, generator=torch.Generator().manual_seed(36)))
    y = R.conv2d_fwd(x, w, 1, 1, acc=F64).reshape(-1, Cout)
    return case, x, dy, y


def _stats_rows(y, sb):
    M, C = y.shape
    nt = MT.cdiv(M, sb)
    yp = torch.cat([y, torch.zeros(nt * sb - M, C)]).reshape(nt, sb, C)
    return torch.stack([yp.sum(1), (yp * yp).sum(1)], 1)           # fp32 partial rows [tiles][2][C], as the kernel leaves them


def test_thin_forward_checks_reject_a_stale_second_trip_tile(thin):
    (N, H, W, Cout), x, dy, y = thin
    sb, _, ntiles = MT.thin_plan(N, H, W, Cout)[:3]
    grid = 2 * 256                                                 # 2 x CUs of an MI355X
    assert ntiles > grid
    stats = _stats_rows(y, sb)
    assert check_bf16(y, y, rel=1e-3) == [] and check_stats(stats, y) == []
    k = 7                                                          # workgroup 7: tiles 7 and grid + 7
    lo = (grid + k) * sb
    bad = y.clone()
    bad[lo:lo + sb] = y[k * sb:(k + 1) * sb]
    assert check_bf16(bad, y, rel=1e-3) != []
    stale = stats.clone()
    stale[grid + k] = stats[k]
    assert check_stats(stale, y) != []                             # the output right, its statistics row stale
    assert check_stats(stale, bad) == []                           # (consistent with the stale tile: both checks are needed)


def test_thin_wgrad_check_rejects_splits_that_drop_their_last_tile(thin):
    (N, H, W, Cout), x, dy, y = thin
    sbw, ntw, S, tps = MT.thin_plan(N, H, W, Cout)[3:]
    ref = R.conv2d_wgrad(x, dy, (3, 3), 1, 1, acc=F64).reshape(Cout, -1)
    assert check_fp32(ref.float(), ref) == []
    tile = MT.thin_tile_of_pixel(N * H * W, sbw)
    last_of_split = torch.tensor([min((s + 1) * tps, ntw) - 1 for s in range(S)])
    dropped = torch.isin(tile, last_of_split).view(N, H, W, 1)
    part = R.conv2d_wgrad(x, dy * dropped, (3, 3), 1, 1, acc=F64).reshape(Cout, -1)
    assert check_fp32((ref - part).float(), ref) != []
    # a single split's last tile (128 of 87801 pixels)
    one = (tile == last_of_split[100]).view(N, H, W, 1)
    part = R.conv2d_wgrad(x, dy * one, (3, 3), 1, 1, acc=F64).reshape(Cout, -1)
    assert check_fp32((ref - part).float(), ref) != []
