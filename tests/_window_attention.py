"""Shared by the window-attention tests (tests/test_window_attention_gpu.py, tests/test_window_attention_w12_gpu.py,
tests/test_multitrip_gpu.py, tests/test_attention_ranges_gpu.py): cases, seeded operands, the guarded forward + backward launch, the
cached fp64 reference (oracle/swin_ref.py window_attention_ref) and the parity check of one case.  Importing it needs no GPU."""
import torch

from _harness import DEV, guarded, hip, intact, rnd_bf16
from oracle.swin_ref import window_attention_ref
from oracle import ops_ref as R

D = 32
SCALE = D ** -0.5

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


def operands(B, Hs, Ws, H, ws):
    T = ws * ws
    qkv = rnd_bf16(B * Hs * Ws, 3 * H * D, seed=120)
    dout = rnd_bf16(B * Hs * Ws, H * D, seed=121)
    g = torch.Generator().manual_seed(122)
    bias = torch.randn(H, T, T, generator=g) * 0.5
    return qkv, dout, bias


def run(lib, qkv, dout, bias, B, Hs, Ws, H, ws, shift, d=D, accumulate=0, dbias_fill=float("nan")):
    """Forward + backward on guarded outputs.  Returns (rc_fwd, rc_bwd, out, lse, dqkv, dbias) and asserts the bands."""
    h = hip()
    T = ws * ws
    rows = B * Hs * Ws
    nwin = B * (Hs // ws) * (Ws // ws) if Hs % ws == 0 and Ws % ws == 0 else B
    qd = qkv.to(torch.bfloat16).to(DEV).contiguous()
    dd = dout.to(torch.bfloat16).to(DEV).contiguous()
    bd = bias.to(DEV).contiguous()
    nan = float("nan")
    out, out_g = guarded((rows, H * d), torch.bfloat16, nan)
    lse, lse_g = guarded((nwin * H, T), torch.float32, nan)
    dqkv, dqkv_g = guarded((rows, 3 * H * d), torch.bfloat16, nan)
    dbias, dbias_g = guarded((H * T, T), torch.float32, dbias_fill)
    lse, dbias = lse.view(-1), dbias.view(-1)
    wsb = max(int(lib.icamd_window_attention_bwd_workspace_bytes(B, Hs, Ws, H, ws)), 256)
    wsp = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    rc_f = lib.icamd_window_attention_fwd(h.ptr(qd), h.ptr(bd), h.ptr(out), h.ptr(lse), B, Hs, Ws, H, d, ws, shift, SCALE,
                                          h.stream_ptr())
    rc_b = lib.icamd_window_attention_bwd(h.ptr(qd), h.ptr(bd), h.ptr(out), h.ptr(dd), h.ptr(lse), h.ptr(dqkv),
                                          h.ptr(dbias), accumulate, h.ptr(wsp), wsb, B, Hs, Ws, H, d, ws, shift, SCALE,
                                          h.stream_ptr())
    assert intact(out_g), "guard band behind out written"
    assert intact(lse_g), "guard band behind lse written"
    assert intact(dqkv_g), "guard band behind dqkv written"
    assert intact(dbias_g), "guard band behind dbias written"
    return rc_f, rc_b, out, lse, dqkv, dbias


_REF = {}


def reference(case):
    """fp64 reference of a case, computed once and shared"""
    if case not in _REF:
        B, Hs, Ws, H, ws, shift = case
        qkv, dout, bias = operands(B, Hs, Ws, H, ws)
        _REF[case] = window_attention_ref(qkv, bias, B, Hs, Ws, H, ws, shift, dout=dout)
    return _REF[case]


def check_case(lib, case):
    """parity of one case with its fp64 reference: lse allclose(1e-4, 1e-4), out rel-L2 <= 3e-3, dq / dk / dv / dbias <= 6e-3"""
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
