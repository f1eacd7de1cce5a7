"""icamd_window_attention_fwd / _bwd and the relative-position gather / scatter (csrc/window_attention.hip), through the C ABI.

The reference (oracle/swin_ref.py window_attention_ref) does what timm does -- torch.roll, window_partition, the img_mask built by
slices, window_reverse, roll back -- in fp64 with P and dS unrounded.  Bounds are those tests/test_attention_long_gpu.py applies to
icamd_attention_fwd / _bwd against the same kind of oracle: the rounding points are the same (P and dS rounded to bf16 once as MFMA
operands, fp32 accumulation, one final rounding).  dbias is taken in fp32 before that rounding and is held to the bound of the
other gradients of the same backward.

Every output is allocated with a guard band behind it that must come back untouched (tests/_harness.py guarded).  Cases, operands,
the guarded launch and the parity check are in tests/_window_attention.py, which the window-12, multi-trip and range tests share.
"""
import pytest
import torch

from _harness import UNSUPPORTED, digest, guarded, hip, intact, rnd_bf16
from _harness import lib  # noqa: F401
from oracle.swin_ref import relative_position_index
from _window_attention import CASES, check_case, operands, run
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("case", CASES)
def test_window_attention_matches_reference(lib, case):
    check_case(lib, case)


def test_accumulate_adds_onto_dbias(lib):
    case = CASES[0]
    B, Hs, Ws, H, ws, shift = case
    qkv, dout, bias = operands(B, Hs, Ws, H, ws)
    _, _, _, _, _, fresh = run(lib, qkv, dout, bias, *case)
    rc_f, rc_b, _, _, _, added = run(lib, qkv, dout, bias, *case, accumulate=1, dbias_fill=1.5)
    assert rc_f == 0 and rc_b == 0
    assert torch.equal(added.cpu(), 1.5 + fresh.cpu())


@pytest.mark.parametrize("case", [CASES[0], CASES[6]])
def test_window_attention_is_bitwise_reproducible(lib, case):
    B, Hs, Ws, H, ws, shift = case
    qkv, dout, bias = operands(B, Hs, Ws, H, ws)

    def once():
        rc_f, rc_b, out, lse, dqkv, dbias = run(lib, qkv, dout, bias, *case)
        assert rc_f == 0 and rc_b == 0
        return digest(out, lse, dqkv, dbias)

    assert once() == once()


@pytest.mark.parametrize("B,Hs,Ws,H,ws,shift,d", [(1, 14, 14, 2, 7, 3, 64), (1, 18, 18, 2, 9, 4, 32), (1, 15, 14, 2, 7, 3, 32),
                                                  (1, 14, 14, 2, 7, 7, 32)])
def test_unsupported_shapes_are_refused_and_write_nothing(lib, B, Hs, Ws, H, ws, shift, d):
    T = ws * ws
    qkv = rnd_bf16(B * Hs * Ws, 3 * H * d, seed=1)
    dout = rnd_bf16(B * Hs * Ws, H * d, seed=2)
    bias = torch.zeros(H, T, T)
    rc_f, rc_b, out, lse, dqkv, dbias = run(lib, qkv, dout, bias, B, Hs, Ws, H, ws, shift, d=d)
    assert rc_f == UNSUPPORTED and rc_b == UNSUPPORTED, (rc_f, rc_b)
    for t in (out, lse, dqkv, dbias):
        assert bool(torch.isnan(t.float()).all()), "a refused call wrote to an output"


@pytest.mark.parametrize("ws", [4, 7, 8])
@pytest.mark.parametrize("H", [1, 3])
def test_relpos_gather_and_scatter(lib, ws, H):
    h = hip()
    T, L = ws * ws, 2 * ws - 1
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


def test_relpos_refuses_windows_it_does_not_take(lib):
    h = hip()
    t = torch.full((400,), float("nan"), device=DEV)
    o = torch.full((9 ** 4,), float("nan"), device=DEV)
    assert lib.icamd_relpos_bias_gather(h.ptr(t), h.ptr(o), 1, 9, h.stream_ptr()) == UNSUPPORTED
    assert lib.icamd_relpos_bias_scatter(h.ptr(o), h.ptr(t), 1, 9, 0, h.stream_ptr()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(t).all())
