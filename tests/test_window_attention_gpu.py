"""icamd_window_attention_fwd / _bwd and the relative-position gather / scatter (csrc/window_attention.hip), through the C ABI.

The reference (tests/_swin_ref.py window_attention_ref) does what timm does -- torch.roll, window_partition, the img_mask built by
slices, window_reverse, roll back -- in fp64 with P and dS unrounded.  Bounds are those tests/test_attention_long_gpu.py applies to
icamd_attention_fwd / _bwd against the same kind of oracle: the rounding points are the same (P and dS rounded to bf16 once as MFMA
operands, fp32 accumulation, one final rounding).  dbias is taken in fp32 before that rounding and is held to the bound of the
other gradients of the same backward.

Every output is allocated with a guard band behind it that must come back untouched, with the construction of the long-attention
tests.
"""
import hashlib
import os
import sys

import pytest
import torch

from oracle import ops_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _swin_ref import relative_position_index, window_attention_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 32
SCALE = D ** -0.5
BAND = 64
SENT16 = 0x5A5B
SENT32 = 0x4B5A5B5C
ICAMD_ERR_UNSUPPORTED = 2

# (B, Hs, Ws, heads, ws, shift)
CASES = [
    (2, 14, 14, 3, 7, 3),     # all nine regions and all four kinds of window
    (2, 14, 14, 3, 7, 0),     # no shift
    (1, 14, 21, 1, 7, 3),     # H != W
    (3, 7, 7, 2, 7, 0),       # one window
    (2, 8, 16, 2, 4, 2),      # T = 16
    (1, 16, 8, 2, 8, 4),      # T = 64 exactly, no padded columns
    (8, 56, 56, 3, 7, 3),     # 512 windows x 3 heads: 128 workgroups per head, under both caps (682 forward, 341 backward), so
                              # still ONE trip per workgroup; tests/test_multitrip_gpu.py has the multi-trip cases
]


@pytest.fixture(scope="module")
def lib():
    from imageclassification_amd import hip
    hip.require_gpu()
    return hip.load()


def _hip():
    from imageclassification_amd import hip
    return hip


def rnd_bf16(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return R.bf16_round(torch.randn(*shape, generator=g) * scale)


def guarded_bf16(rows, cols, fill):
    whole = torch.full(((rows + BAND) * cols,), SENT16, dtype=torch.int16, device=DEV)
    view = whole[:rows * cols].view(torch.bfloat16).view(rows, cols)
    view.fill_(fill)
    return view, whole


def guarded_f32(n, fill):
    whole = torch.full((n + BAND,), SENT32, dtype=torch.int32, device=DEV)
    view = whole[:n].view(torch.float32)
    view.fill_(fill)
    return view, whole


def band_intact(whole, n, sentinel):
    return bool((whole[n:] == sentinel).all())


def operands(B, Hs, Ws, H, ws):
    T = ws * ws
    qkv = rnd_bf16(B * Hs * Ws, 3 * H * D, seed=120)
    dout = rnd_bf16(B * Hs * Ws, H * D, seed=121)
    g = torch.Generator().manual_seed(122)
    bias = torch.randn(H, T, T, generator=g) * 0.5
    return qkv, dout, bias


def run(lib, qkv, dout, bias, B, Hs, Ws, H, ws, shift, d=D, accumulate=0, dbias_fill=float("nan")):
    """Forward + backward on guarded outputs.  Returns (rc_fwd, rc_bwd, out, lse, dqkv, dbias) and asserts the bands."""
    hip = _hip()
    T = ws * ws
    rows = B * Hs * Ws
    nwin = B * (Hs // ws) * (Ws // ws) if Hs % ws == 0 and Ws % ws == 0 else B
    qd = qkv.to(torch.bfloat16).to(DEV).contiguous()
    dd = dout.to(torch.bfloat16).to(DEV).contiguous()
    bd = bias.to(DEV).contiguous()
    nan = float("nan")
    out, out_w = guarded_bf16(rows, H * d, nan)
    lse, lse_w = guarded_f32(nwin * H * T, nan)
    dqkv, dqkv_w = guarded_bf16(rows, 3 * H * d, nan)
    dbias, dbias_w = guarded_f32(H * T * T, dbias_fill)
    wsb = max(int(lib.icamd_window_attention_bwd_workspace_bytes(B, Hs, Ws, H, ws)), 256)
    wsp = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    rc_f = lib.icamd_window_attention_fwd(hip.ptr(qd), hip.ptr(bd), hip.ptr(out), hip.ptr(lse), B, Hs, Ws, H, d, ws, shift, SCALE,
                                          hip.stream_ptr())
    rc_b = lib.icamd_window_attention_bwd(hip.ptr(qd), hip.ptr(bd), hip.ptr(out), hip.ptr(dd), hip.ptr(lse), hip.ptr(dqkv),
                                          hip.ptr(dbias), accumulate, hip.ptr(wsp), wsb, B, Hs, Ws, H, d, ws, shift, SCALE,
                                          hip.stream_ptr())
    torch.cuda.synchronize()
    assert band_intact(out_w, rows * H * d, SENT16), "guard band behind out written"
    assert band_intact(lse_w, nwin * H * T, SENT32), "guard band behind lse written"
    assert band_intact(dqkv_w, rows * 3 * H * d, SENT16), "guard band behind dqkv written"
    assert band_intact(dbias_w, H * T * T, SENT32), "guard band behind dbias written"
    return rc_f, rc_b, out, lse, dqkv, dbias


_REF = {}


def reference(case):
    """fp64 reference of a case, computed once and shared"""
    if case not in _REF:
        B, Hs, Ws, H, ws, shift = case
        qkv, dout, bias = operands(B, Hs, Ws, H, ws)
        _REF[case] = window_attention_ref(qkv, bias, B, Hs, Ws, H, ws, shift, dout=dout)
    return _REF[case]


@pytest.mark.parametrize("case", CASES)
def test_window_attention_matches_reference(lib, case):
    B, Hs, Ws, H, ws, shift = case
    T = ws * ws
    qkv, dout, bias = operands(B, Hs, Ws, H, ws)
    rc_f, rc_b, out, lse, dqkv, dbias = run(lib, qkv, dout, bias, B, Hs, Ws, H, ws, shift)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    ro, rlse, rdqkv, rdbias = reference(case)
    got = out.float().cpu()
    glse = lse.cpu().view(-1, H, T)
    gd = dqkv.float().cpu()
    gb = dbias.cpu().view(H, T, T)
    assert torch.isfinite(got).all() and torch.isfinite(glse).all() and torch.isfinite(gd).all() and torch.isfinite(gb).all()
    lse_err = float((glse.double() - rlse).abs().max())
    fwd = R.rel_l2(got, ro.reshape(got.shape))
    print(f"case {case}: lse max abs err {lse_err:.3g}, out rel_l2 {fwd:.3g}")
    errs = {}
    rd = rdqkv.reshape(gd.shape)
    for name, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, 2 * H * D)), ("dv", slice(2 * H * D, 3 * H * D))):
        errs[name] = R.rel_l2(gd[:, sl], rd[:, sl])
    errs["dbias"] = R.rel_l2(gb, rdbias)
    print("    " + ", ".join(f"{k} rel_l2 {v:.3g}" for k, v in errs.items()))
    assert torch.allclose(glse.double(), rlse, rtol=1e-4, atol=1e-4)
    assert fwd <= 3e-3
    for name in ("dq", "dk", "dv", "dbias"):
        assert errs[name] <= 6e-3, (name, errs[name])


def test_accumulate_adds_onto_dbias(lib):
    case = CASES[0]
    B, Hs, Ws, H, ws, shift = case
    qkv, dout, bias = operands(B, Hs, Ws, H, ws)
    _, _, _, _, _, fresh = run(lib, qkv, dout, bias, *case)
    rc_f, rc_b, _, _, _, added = run(lib, qkv, dout, bias, *case, accumulate=1, dbias_fill=1.5)
    assert rc_f == 0 and rc_b == 0
    assert torch.equal(added.cpu(), 1.5 + fresh.cpu())


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


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
    assert rc_f == ICAMD_ERR_UNSUPPORTED and rc_b == ICAMD_ERR_UNSUPPORTED, (rc_f, rc_b)
    for t in (out, lse, dqkv, dbias):
        assert bool(torch.isnan(t.float()).all()), "a refused call wrote to an output"


@pytest.mark.parametrize("ws", [4, 7, 8])
@pytest.mark.parametrize("H", [1, 3])
def test_relpos_gather_and_scatter(lib, ws, H):
    hip = _hip()
    T, L = ws * ws, 2 * ws - 1
    g = torch.Generator().manual_seed(7 * ws + H)
    table = torch.randn(L * L, H, generator=g)
    idx = relative_position_index(ws)
    want = table[idx.view(-1)].view(T, T, H).permute(2, 0, 1).contiguous()
    td = table.to(DEV)
    bias, bias_w = guarded_f32(H * T * T, float("nan"))
    assert lib.icamd_relpos_bias_gather(hip.ptr(td), hip.ptr(bias), H, ws, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert band_intact(bias_w, H * T * T, SENT32)
    assert torch.equal(bias.cpu().view(H, T, T), want)                     # bit for bit
    d = torch.randn(H, T, T, generator=g)
    want_t = torch.zeros(L * L, H, dtype=torch.float64).index_add_(0, idx.view(-1), d.double().permute(1, 2, 0).reshape(T * T, H))
    dd = d.to(DEV)
    dtab, dtab_w = guarded_f32(L * L * H, float("nan"))
    assert lib.icamd_relpos_bias_scatter(hip.ptr(dd), hip.ptr(dtab), H, ws, 0, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert band_intact(dtab_w, L * L * H, SENT32)
    got_t = dtab.cpu().view(L * L, H).double()
    assert R.rel_l2(got_t, want_t) <= 1e-6
    assert lib.icamd_relpos_bias_scatter(hip.ptr(dd), hip.ptr(dtab), H, ws, 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert R.rel_l2(dtab.cpu().view(L * L, H).double(), 2 * want_t) <= 1e-6
    # <gather(t), d> == <t, scatter(d)> to fp32 rounding
    lhs = float((want.double() * d.double()).sum())
    rhs = float((table.double() * got_t).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((want.double().abs() * d.double().abs()).sum())


def test_relpos_refuses_windows_it_does_not_take(lib):
    hip = _hip()
    t = torch.full((400,), float("nan"), device=DEV)
    o = torch.full((9 ** 4,), float("nan"), device=DEV)
    assert lib.icamd_relpos_bias_gather(hip.ptr(t), hip.ptr(o), 1, 9, hip.stream_ptr()) == ICAMD_ERR_UNSUPPORTED
    assert lib.icamd_relpos_bias_scatter(hip.ptr(o), hip.ptr(t), 1, 9, 0, hip.stream_ptr()) == ICAMD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(t).all())
