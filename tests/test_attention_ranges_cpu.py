"""tests/_attention_ranges.py kept honest, without a GPU: the operands are what they claim, the shift reaches the range it is meant to
reach without changing the problem, and the rounding-point oracle alone stays under every cap tests/test_attention_ranges_gpu.py
applies to the kernels (a case whose reference misses its cap is ill-posed: the case changes, not the cap)."""
import math
import os
import sys

import pytest
import torch

from oracle import ops_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attention_ranges as AR  # noqa: E402

D, SCALE = AR.D, AR.SCALE
GPU_CASES = AR.CASES + [AR.persistent_case(256)]
SHIFT_T = sorted({c[2] for c in GPU_CASES if c[0] in AR.SHIFTED})


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: f"{c[0]}-T{c[2]}-B{c[1]}")
def test_operands_are_on_the_bf16_grid(case):
    regime, B, T, H = case
    qkv, dout = AR.operands(*case)
    assert qkv.shape == (B * T, 3 * H * D) and dout.shape == (B * T, H * D)
    assert torch.equal(R.bf16_round(qkv), qkv) and torch.equal(R.bf16_round(dout), dout)
    assert torch.isfinite(qkv).all() and torch.isfinite(dout).all()
    if regime in AR.SHIFTED:
        x = qkv.view(B, T, 3, H, D)
        assert bool((x[:, :, 1, :, AR.D0] == 1.0).all())
        # the product the kernels form for that dimension, times the scale, is c_i exactly
        c = x[:, :, 0, :, AR.D0].double() * SCALE
        assert set(c.flatten().tolist()) <= set(AR.CYCLE)
        if regime == "shift_heads":
            # a persistent workgroup's consecutive heads (pair, pair + 256) shift different rows
            assert not torch.equal(c[0, :, 0], c[256 // H, :, 256 % H])


@pytest.mark.parametrize("T", SHIFT_T)
def test_shift_reaches_both_ends_of_the_range(T):
    lse = AR.reference(("shift", AR.B, T, AR.H))["exact"]["lse"]
    print(f"T {T}: lse {float(lse.min()):.1f} .. {float(lse.max()):.1f}")
    assert float(lse.min()) < -120.0 and float(lse.max()) > 120.0
    # every kind of row in every 16-row block that is complete
    assert T < 16 or len(set(AR.shift_constants(T)[:16].tolist())) == len(AR.CYCLE)


@pytest.mark.parametrize("T", SHIFT_T)
def test_shift_leaves_the_problem_unchanged(T):
    """out, dv and dq / dk outside column D0 are those of the same operands with q[:, D0] = 0, to fp64 round-off; lse moves by c_i"""
    B, H = AR.B, AR.H
    qkv, dout = AR.operands("shift", B, T, H)
    plain = qkv.clone()
    plain.view(B, T, 3, H, D)[:, :, 0, :, AR.D0] = 0.0
    a = R.attention_written_out(qkv, dout, B, T, H, D, SCALE)
    b = R.attention_written_out(plain, dout, B, T, H, D, SCALE)
    HD = H * D
    cols, rest = AR.d0_columns(H)
    assert R.rel_l2(a["out64"], b["out64"]) <= 1e-11
    assert R.rel_l2(a["dqkv64"][:, 2 * HD:], b["dqkv64"][:, 2 * HD:]) <= 1e-11
    assert R.rel_l2(a["dqkv64"][:, :HD][:, rest], b["dqkv64"][:, :HD][:, rest]) <= 1e-11
    assert R.rel_l2(a["dqkv64"][:, HD:2 * HD][:, rest], b["dqkv64"][:, HD:2 * HD][:, rest]) <= 1e-11
    assert torch.allclose(a["lse"] - b["lse"], AR.shift_constants(T).double().expand(B, H, T), rtol=0, atol=1e-11)
    # column D0 of dq: zero up to the round-off of a sum of T terms of size |dS|
    dq0 = a["dqkv64"][:, :HD][:, cols]
    assert float(dq0.abs().max()) <= 1e-12 * float(a["ds"].abs().sum(-1).max())


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: f"{c[0]}-T{c[2]}-B{c[1]}")
def test_written_out_oracle_is_the_autograd_oracle(case):
    ref = AR.reference(case)
    regime, B, T, H = case
    w, ex = ref["written"], ref["exact"]
    assert torch.allclose(w["lse"], ex["lse"], rtol=1e-12, atol=1e-12)
    # both are fp64 results rounded to bf16 once: they may differ where round-off moves a value across a rounding boundary
    assert R.rel_l2(w["out"], ex["out"]) <= 1e-5
    HD = H * D
    cols, rest = AR.d0_columns(H)
    keep = torch.cat([rest if regime in AR.SHIFTED else torch.ones(HD, dtype=torch.bool), torch.ones(2 * HD, dtype=torch.bool)])
    assert R.rel_l2(w["dqkv"][:, keep], ex["dqkv"][:, keep]) <= 1e-5


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: f"{c[0]}-T{c[2]}-B{c[1]}")
def test_rounding_point_oracle_stays_under_the_caps(case):
    ref = AR.reference(case)
    e_round = ref["e_round"]
    cap = AR.caps(case, e_round)
    print(AR.table_row(case, e_round, e_round, cap))
    assert torch.isfinite(ref["points"]["out"]).all() and torch.isfinite(ref["points"]["dqkv"]).all()
    assert torch.allclose(ref["points"]["lse"], ref["exact"]["lse"], rtol=1e-12, atol=1e-12)
    for name, e in e_round.items():
        assert e <= cap[name], (name, e, cap[name])
    if case[0] != "peaked":
        assert cap == {n: (AR.OUT_BOUND if n == "out" else 1.0 if n == "dq_d0_excess" else AR.GRAD_BOUND) for n in cap}


def test_zero_q_is_the_uniform_softmax():
    for T in AR.ALL_REGIMES_T:
        ref = AR.reference(("zero_q", AR.B, T, AR.H))
        assert float((ref["exact"]["lse"] - math.log(T)).abs().max()) <= 1e-12


def test_shifted_bias_adds_the_cycle_to_rows():
    bias = torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(1)) * 0.5
    sb = AR.shifted_bias(bias)
    assert sb.dtype == torch.float32
    want = bias.double() + AR.shift_constants(16).double()[None, :, None]
    assert float((sb.double() - want).abs().max()) <= 2.0 ** -24 * 161
