"""The four attention kernel families outside the logit band `randn` operands keep them in: rows shifted by -160 ... +128 (lse from
about -157 to +134 inside one 16-row block), peaked and flat softmax, large and small v and dO.  Operands, references and bounds are
those of tests/_attention_ranges.py (checked on the CPU by tests/test_attention_ranges_cpu.py); the launches go through the
guarded-buffer run() helpers of tests/_attention_long.py and tests/_window_attention.py, so the guard bands are held too.

  resident (csrc/attention.hip)           <4>: T = 17, 50, 64 (64 has no pad keys); <13>: T = 100, 197, 208; and one case with more
                                          (image, head) pairs than the grid cap, so every persistent workgroup hands over to a second head
  tiled (csrc/attention_long.hip)         T = 209, 257, 333 (last key tile partly filled), 256 (filled)
  window <= 8 (csrc/window_attention.hip) three cases of the sibling file, the shift added to the rows of the bias table
  window 12 (csrc/window_attention_w12.hip)  the smallest sibling case, with and without the row shift, with and without window shift

Against the fp64 oracle, per case: everything finite; lse allclose(1e-4, 1e-4); out rel-L2 <= 3e-3; dq, dk, dv (dbias) rel-L2 <= 6e-3 --
the bounds of the sibling files, unchanged: a row shift does not change the mathematical problem.  In the shift regimes dk's D0 columns
(O(10^2 .. 10^3)) and its other columns are held separately and dq's D0 column, zero in exact arithmetic, absolutely.  Only the peaked
regime, where the rounding of P and dS to bf16 alone costs 5.5e-3 to 5.9e-3 on dq and dk, is held to max(that bound, 1.5 x e_round),
e_round being the rounding-point ORACLE against the exact one.

What this file found when it was written: both dQ kernels of the dense routes (attn_bwd_dq_kernel, attn_long_bwd_dq_kernel) formed
p = exp(0 - lse) for the zero-filled key rows past T without a mask; for a query with lse below about -88.7 that is +inf, dS = inf
* (0 - delta), and the K^T dS product spread 0 * inf = NaN over the whole dq row."""
import pytest
import torch

import _attention_long as AL
import _attention_ranges as AR
import _window_attention as WA
from _harness import lib  # noqa: F401
from oracle.swin_ref import window_attention_ref
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

D, SCALE = AR.D, AR.SCALE
assert (AL.D, AL.SCALE) == (D, SCALE)


def case_id(c):
    return "-".join(str(x) for x in c)


def check_dense(lib, case):
    regime, B, T, H = case
    ref = AR.reference(case)
    qkv, dout, ex = ref["qkv"], ref["dout"], ref["exact"]
    rc_f, rc_b, out, lse, delta, dqkv = AL.run(lib, qkv, dout, B, T, H)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    got, glse, gdelta, gd = out.float().cpu(), lse.cpu().double(), delta.cpu().double(), dqkv.float().cpu()
    bad = {n: int((~torch.isfinite(t)).sum()) for n, t in (("out", got), ("lse", glse), ("delta", gdelta), ("dqkv", gd))}
    HD = H * D
    bad_rows = {n: int((~torch.isfinite(gd[:, s])).any(-1).sum()) for n, s in (("dq", slice(0, HD)), ("dk", slice(HD, 2 * HD)),
                                                                             ("dv", slice(2 * HD, 3 * HD)))}
    e_round = ref["e_round"]
    measured = AR.errors(case, got, gd, ref)
    cap = AR.caps(case, e_round)
    lse_err = float((glse - ex["lse"]).abs().max())
    print(AR.table_row(case, e_round, measured, cap))
    print(f"    lse {float(ex['lse'].min()):.1f} .. {float(ex['lse'].max()):.1f}, max abs err {lse_err:.3g}; non-finite values {bad}, "
          f"rows of dq / dk / dv with one {bad_rows}")
    assert not any(bad.values()), (bad, bad_rows)
    assert torch.allclose(glse, ex["lse"], rtol=1e-4, atol=1e-4)
    # delta = rowsum(dout * out) of the values the forward stored: an fp32 sum of 64 products and two shuffles
    prod = dout.reshape(B, T, H, D).double() * got.reshape(B, T, H, D).double()
    rdelta, mag = prod.sum(-1).permute(0, 2, 1), prod.abs().sum(-1).permute(0, 2, 1)
    assert bool(((gdelta - rdelta).abs() <= 2.0 ** -17 * mag + 1e-37).all())
    for name, e in measured.items():
        assert e <= cap[name], (name, e, cap[name])
    if regime == "zero_q":
        # exactly uniform softmax, no oracle: P = 1 in bf16 exactly, so out is the fp32 sum of v over T, rounded once
        v = qkv.view(B, T, 3, H, D)[:, :, 2].double()
        mean = v.mean(1, keepdim=True).expand(B, T, H, D).reshape(B * T, HD)
        slack = AR.bf16_ulp(mean) + T * 2.0 ** -24 * v.abs().mean(1, keepdim=True).expand(B, T, H, D).reshape(B * T, HD)
        assert bool(((got.double() - mean).abs() <= slack).all())
        assert float((glse - torch.tensor(float(T)).double().log()).abs().max()) <= 1e-4


@pytest.mark.parametrize("case", AR.CASES, ids=case_id)
def test_dense_attention_ranges(lib, case):
    check_dense(lib, case)


def test_persistent_hand_over_under_row_shift(lib):
    """more (image, head) pairs than the grid of the resident kernels (one workgroup per CU): every workgroup walks a second head,
    whose fragments and lse arrive through the prefetch, and consecutive heads shift different rows"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = AR.persistent_case(cus)
    regime, B, T, H = case
    assert B * H > cus and T <= 208
    assert AR.head_offset(0) != AR.head_offset(cus), "a workgroup's first and second head would shift the same rows"
    check_dense(lib, case)


# ---- window kernels: the row shift goes into the bias table ----------------------------------------------------------------------
WINDOW_CASES = [(WA.CASES[0], True), (WA.CASES[4], True), (WA.CASES[5], True)]
assert [c for c, _ in WINDOW_CASES] == [(2, 14, 14, 3, 7, 3), (2, 8, 16, 2, 4, 2), (1, 16, 8, 2, 8, 4)]
W12_CASES = [((1, 12, 24, 1, 12, 11), True), ((1, 12, 24, 1, 12, 11), False), ((1, 12, 24, 1, 12, 0), True)]
_WREF = {}


def window_operands(case, shifted):
    B, Hs, Ws, H, ws, shift = case
    qkv, dout, bias = WA.operands(B, Hs, Ws, H, ws)
    return qkv, dout, AR.shifted_bias(bias) if shifted else bias


def window_reference(case, shifted):
    if (case, shifted) not in _WREF:
        B, Hs, Ws, H, ws, shift = case
        qkv, dout, bias = window_operands(case, shifted)
        _WREF[(case, shifted)] = window_attention_ref(qkv, bias, B, Hs, Ws, H, ws, shift, dout=dout)
    return _WREF[(case, shifted)]


@pytest.mark.parametrize("case,shifted", WINDOW_CASES + W12_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else f"rows{int(v)}")
def test_window_attention_ranges(lib, case, shifted):
    B, Hs, Ws, H, ws, shift = case
    T, Dw = ws * ws, WA.D
    qkv, dout, bias = window_operands(case, shifted)
    rc_f, rc_b, out, lse, dqkv, dbias = WA.run(lib, qkv, dout, bias, B, Hs, Ws, H, ws, shift)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    ro, rlse, rdqkv, rdbias = window_reference(case, shifted)
    got, glse, gd, gb = out.float().cpu(), lse.cpu().view(-1, H, T).double(), dqkv.float().cpu(), dbias.cpu().view(H, T, T)
    bad = {n: int((~torch.isfinite(t)).sum()) for n, t in (("out", got), ("lse", glse), ("dqkv", gd), ("dbias", gb))}
    errs = {"out": R.rel_l2(got, ro.reshape(got.shape))}
    rd = rdqkv.reshape(gd.shape)
    for name, sl in (("dq", slice(0, H * Dw)), ("dk", slice(H * Dw, 2 * H * Dw)), ("dv", slice(2 * H * Dw, 3 * H * Dw))):
        errs[name] = R.rel_l2(gd[:, sl], rd[:, sl])
    errs["dbias"] = R.rel_l2(gb, rdbias)
    print(f"window case {case} rows shifted {shifted}: lse {float(rlse.min()):.1f} .. {float(rlse.max()):.1f}, max abs err "
          f"{float((glse - rlse).abs().max()):.3g}; " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f"; non-finite {bad}")
    assert not any(bad.values()), bad
    assert torch.allclose(glse, rlse, rtol=1e-4, atol=1e-4)
    assert errs["out"] <= AR.OUT_BOUND
    for name in ("dq", "dk", "dv", "dbias"):
        assert errs[name] <= AR.GRAD_BOUND, (name, errs[name])
