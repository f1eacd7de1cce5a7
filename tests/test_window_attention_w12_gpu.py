"""icamd_window_attention_fwd / _bwd and the relative-position gather / scatter for 12 x 12 windows (csrc/window_attention_w12.hip),
through the C ABI.

Reference, operands, guard bands, NaN-filled outputs and the parity check are those of tests/_window_attention.py (fp64
window_attention_ref of oracle/swin_ref.py, P and dS unrounded), shared with tests/test_window_attention_gpu.py, and so are the bounds: lse allclose(1e-4, 1e-4), out rel-L2 <= 3e-3,
dq / dk / dv / dbias rel-L2 <= 6e-3 -- the rounding points of the T = 144 kernels are the same (P and dS rounded to bf16 once as MFMA
operands, fp32 accumulation, one final rounding; dbias from the fp32 dS).  The multi-trip case adds the per 64 x 64 block checks of
tests/test_multitrip_gpu.py, which catch a trip that writes the right values to the wrong window."""
import pytest
import torch

import _swin_w12 as W12
import _window_attention as WA
from _fullsize_check import check_bf16, check_close, check_fp32, require, worst_block
from _harness import UNSUPPORTED, digest, guarded, hip, intact, rnd_bf16
from _harness import lib  # noqa: F401
from oracle.swin_ref import relative_position_index, window_attention_ref
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = WA.D
T = 144

# (B, Hs, Ws, heads, ws, shift)
CASES = [
    (2, 24, 24, 2, 12, 6),     # all nine regions and all four kinds of window
    (2, 24, 24, 2, 12, 0),     # no shift
    (1, 24, 36, 3, 12, 6),     # Hs != Ws
    (3, 12, 12, 2, 12, 0),     # one window per image: the last stage's shape
    (1, 12, 24, 1, 12, 11),    # the largest shift
]
# 68 windows x 32 heads: the forward runs 64 workgroups per head (2048 / 32) for 2 trips, the backward 16 (512 / 32) for 5; both
# last trips are ragged (4 of 64, 4 of 16 workgroups walk one).  One image fewer (64 windows) is a single forward trip.
MULTITRIP = (17, 24, 24, 32, 12, 6)


@pytest.mark.parametrize("case", CASES)
def test_window12_attention_matches_reference(lib, case):
    WA.check_case(lib, case)


def test_window12_attention_multitrip(lib):
    case = MULTITRIP
    B, Hs, Ws, H, ws, shift = case
    rows = B * Hs * Ws
    nwin = B * (Hs // ws) * (Ws // ws)
    # multi-trip, by the library's answer: P dbias partials per head = workgroups per head of the backward
    wsb = int(lib.icamd_window_attention_bwd_workspace_bytes(B, Hs, Ws, H, ws))
    P = wsb // (H * T * T * 4)
    assert P == W12.bwd_grid(nwin, H) == 16 and W12.trips(nwin, P) == 5 and nwin % P != 0
    # the forward cap has no query: icamd_window_attention_w12_fwd_launch, restated by W12.fwd_grid
    gf = W12.fwd_grid(nwin, H)
    assert gf == 64 and W12.trips(nwin, gf) == 2 and nwin % gf != 0
    assert W12.trips(nwin - 4, W12.fwd_grid(nwin - 4, H)) == 1       # one image fewer: a single forward trip

    qkv, dout, bias = (t.to(DEV) for t in WA.operands(B, Hs, Ws, H, ws))
    rc_f, rc_b, out, lse, dqkv, dbias = WA.run(lib, qkv, dout, bias, *case)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    ro, rlse, rdqkv, rdbias = window_attention_ref(qkv, bias, B, Hs, Ws, H, ws, shift, dout=dout)
    ro, rd = ro.reshape(rows, H * D), rdqkv.reshape(rows, 3 * H * D)
    got_o, got_d = out.float(), dqkv.float()
    HD = H * D
    parts = (("dq", slice(0, HD)), ("dk", slice(HD, 2 * HD)), ("dv", slice(2 * HD, 3 * HD)))
    print(f"case {case}: fwd grid {gf} x 2 trips, bwd grid {P} x 5 trips")
    print(f"    lse max abs err {float((lse.double().view(-1) - rlse.reshape(-1)).abs().max()):.3g}; "
          f"out rel_l2 {R.rel_l2(got_o, ro):.3g} worst block {worst_block(got_o, ro):.3g}")
    print("    " + "; ".join(f"{n} rel_l2 {R.rel_l2(got_d[:, s], rd[:, s]):.3g} worst block "
                             f"{worst_block(got_d[:, s].contiguous(), rd[:, s].contiguous()):.3g}" for n, s in parts))
    gb, rb = dbias.view(H * T, T), rdbias.reshape(H * T, T)
    print(f"    dbias rel_l2 {R.rel_l2(gb, rb):.3g} worst block {worst_block(gb, rb):.3g}")
    require(check_close(lse, rlse, 1e-4, 1e-4, "lse"), "window-12 attention lse")
    require(check_bf16(got_o, ro, rel=3e-3, block_rel=3e-3, atol_rms=8e-3, max_frac=1e-6), "window-12 attention fwd")
    for name, sl in parts:
        fails = [f for f in check_bf16(got_d[:, sl].contiguous(), rd[:, sl].contiguous(), rel=6e-3, block_rel=6e-3)
                 if "elementwise" not in f]
        require(fails, f"window-12 attention bwd {name}")
    require(check_fp32(gb, rb, rel=6e-3, block_rel=6e-3), "window-12 attention dbias")
    # a second run repeats every output bit for bit
    first = digest(out, lse, dqkv, dbias)
    rc_f, rc_b, out2, lse2, dqkv2, dbias2 = WA.run(lib, qkv, dout, bias, *case)
    assert rc_f == 0 and rc_b == 0
    assert digest(out2, lse2, dqkv2, dbias2) == first


def test_window12_accumulate_adds_onto_dbias(lib):
    case = CASES[0]
    B, Hs, Ws, H, ws, shift = case
    qkv, dout, bias = WA.operands(B, Hs, Ws, H, ws)
    rc_f, rc_b, _, _, _, fresh = WA.run(lib, qkv, dout, bias, *case)
    assert rc_f == 0 and rc_b == 0
    rc_f, rc_b, _, _, _, added = WA.run(lib, qkv, dout, bias, *case, accumulate=1, dbias_fill=1.5)
    assert rc_f == 0 and rc_b == 0
    assert torch.equal(added.cpu(), 1.5 + fresh.cpu())


def test_window12_attention_is_bitwise_reproducible(lib):
    case = CASES[0]
    B, Hs, Ws, H, ws, shift = case
    qkv, dout, bias = WA.operands(B, Hs, Ws, H, ws)

    def once():
        rc_f, rc_b, out, lse, dqkv, dbias = WA.run(lib, qkv, dout, bias, *case)
        assert rc_f == 0 and rc_b == 0
        return digest(out, lse, dqkv, dbias)

    assert once() == once()


@pytest.mark.parametrize("B,Hs,Ws,H,ws,shift,d", [(1, 18, 18, 2, 9, 4, 32), (1, 26, 26, 2, 13, 6, 32), (1, 32, 32, 2, 16, 8, 32),
                                                  (1, 24, 24, 2, 12, 6, 64), (1, 30, 24, 2, 12, 6, 32), (1, 24, 24, 2, 12, 12, 32)])
def test_window12_neighbours_are_refused_and_write_nothing(lib, B, Hs, Ws, H, ws, shift, d):
    Tw = ws * ws
    qkv = rnd_bf16(B * Hs * Ws, 3 * H * d, seed=1)
    dout = rnd_bf16(B * Hs * Ws, H * d, seed=2)
    bias = torch.zeros(H, Tw, Tw)
    rc_f, rc_b, out, lse, dqkv, dbias = WA.run(lib, qkv, dout, bias, B, Hs, Ws, H, ws, shift, d=d)
    assert rc_f == UNSUPPORTED and rc_b == UNSUPPORTED, (rc_f, rc_b)
    for t in (out, lse, dqkv, dbias):
        assert bool(torch.isnan(t.float()).all()), "a refused call wrote to an output"


@pytest.mark.parametrize("H", [1, 3])
def test_window12_relpos_gather_and_scatter(lib, H):
    h = hip()
    ws = 12
    L = 2 * ws - 1
    g = torch.Generator().manual_seed(7 * ws + H)
    table = torch.randn(L * L, H, generator=g)
    idx = relative_position_index(ws)
    want = table[idx.view(-1)].view(T, T, H).permute(2, 0, 1).contiguous()
    td = table.to(DEV)
    bias, bias_g = guarded((H * T, T), torch.float32, float("nan"))
    assert lib.icamd_relpos_bias_gather(h.ptr(td), h.ptr(bias), H, ws, h.stream_ptr()) == 0
    assert intact(bias_g)
    assert torch.equal(bias.cpu().view(H, T, T), want)                     # bit for bit
    d = torch.randn(H, T, T, generator=g)
    want_t = torch.zeros(L * L, H, dtype=torch.float64).index_add_(0, idx.view(-1), d.double().permute(1, 2, 0).reshape(T * T, H))
    dd = d.to(DEV)
    dtab, dtab_g = guarded((L * L, H), torch.float32, float("nan"))
    assert lib.icamd_relpos_bias_scatter(h.ptr(dd), h.ptr(dtab), H, ws, 0, h.stream_ptr()) == 0
    assert intact(dtab_g)
    got_t = dtab.cpu().view(L * L, H).double()
    assert R.rel_l2(got_t, want_t) <= 1e-6
    assert lib.icamd_relpos_bias_scatter(h.ptr(dd), h.ptr(dtab), H, ws, 1, h.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert R.rel_l2(dtab.cpu().view(L * L, H).double(), 2 * want_t) <= 1e-6
    # <gather(t), d> == <t, scatter(d)> to fp32 rounding
    lhs = float((want.double() * d.double()).sum())
    rhs = float((table.double() * got_t).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((want.double().abs() * d.double().abs()).sum())


def test_window7_still_runs_on_the_single_wave_kernels(lib):
    """the dispatch on the window side did not capture small windows: a 7 x 7 case of tests/_window_attention.py against its
    reference under its bounds (the T = 144 kernels would index a 49-token window as if it had 144 slots)"""
    WA.check_case(lib, WA.CASES[0])
