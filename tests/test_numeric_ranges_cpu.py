"""Keeps tests/_numeric_ranges.py honest on the CPU: the builders produce what they claim, the fp64 references agree with torch in the
randn regime, the rounding-point reference of the BatchNorm statistics stays inside the shares and bounds the GPU tests grant, and
the fp32 restatements of the LayerNorm and cross-entropy kernels' own lines stay inside the bounds derived for them."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _numeric_ranges as NR  # noqa: E402
from oracle.convnext_ref import grn_closed_form  # noqa: E402
from oracle.swin_ref import patch_merge_ln_ref  # noqa: E402

F64 = torch.float64


# ---- oracle: the new fp64 paths -------------------------------------------------------------------------------------------------
def test_fp64_oracle_paths_agree_with_torch_and_leave_the_default_alone():
    g = torch.Generator().manual_seed(1)
    y = R.bf16_round(torch.randn(4, 6, 6, 64, generator=g))
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    rm0, rv0 = torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5
    d = R.bn_train_coeffs(y, gamma, beta, rm0, rv0, 0.1, 1e-5)
    w = R.bn_train_coeffs(y, gamma, beta, rm0, rv0, 0.1, 1e-5, acc=F64)
    assert all(t.dtype == torch.float32 for t in d) and all(t.dtype == F64 for t in w)
    for a, b in zip(d, w):
        assert torch.allclose(a.double(), b, rtol=1e-6, atol=1e-7)
    tm, tv = rm0.double().clone(), rv0.double().clone()
    out = F.batch_norm(y.double().reshape(-1, 64), tm, tv, gamma.double(), beta.double(), True, 0.1, 1e-5)
    assert torch.allclose(tm, w[4], rtol=1e-12, atol=1e-14) and torch.allclose(tv, w[5], rtol=1e-12)
    assert torch.allclose(out, y.double().reshape(-1, 64) * w[2] + w[3], rtol=1e-10, atol=1e-12)
    # cross-entropy
    x = R.bf16_round(torch.randn(6, 50, generator=g) * 3)
    y1 = torch.randint(0, 50, (6,), generator=g)
    l32, p32, g32 = R.softmax_xent(x, y1, y1.flip(0), 0.3, 0.1, 0.25)
    l64, p64, g64 = R.softmax_xent(x, y1, y1.flip(0), 0.3, 0.1, 0.25, acc=F64)
    assert l32.dtype == torch.float32 and l64.dtype == F64
    assert torch.allclose(l32.double(), l64, rtol=1e-6) and torch.equal(p32, p64) and R.max_bf16_ulp(g32, g64) <= 1.0
    ce = F.cross_entropy(x.double(), y1, label_smoothing=0.1, reduction="none")
    assert torch.allclose(R.softmax_xent(x, y1, None, 1.0, 0.1, 1.0, acc=F64)[0], ce, rtol=1e-12)


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------
def stats_rows(y):
    """one partial row per 128 output rows: the figure ASSUMED here for every statistics producer; the GPU file takes it from the
    library's *_stats_rows queries and asserts that it is this (produce())"""
    return -(-(y.numel() // y.shape[-1]) // 128)


@pytest.mark.parametrize("name", list(NR.BN_PRODUCERS))
def test_bn_operands_carry_the_offsets_they_claim(name):
    ops = NR.bn_operands(name)
    N, H, W, Cin, Cout, k, stride, pad, groups = NR.BN_PRODUCERS[name]
    cg = Cin // groups
    x, w, s, c = ops["x"], ops["w"], ops["s"], ops["c"]
    assert NR.on_bf16_grid(x) and NR.on_bf16_grid(w) and NR.on_bf16_grid(c) and NR.on_bf16_grid(ops["dout"])
    assert math.log2(s) == round(math.log2(s))
    for grp in range(groups):
        assert bool((x[..., grp * cg + NR.ONE % cg] == 1.0).all())
    taps = w[..., NR.ONE % cg].reshape(Cout, -1)
    centre = (k // 2) * k + k // 2
    assert torch.equal(taps[:, centre], c) and float(taps.abs().sum()) == float(c.abs().sum())
    assert [float(v) / s for v in c[:8]] == list(NR.OFFSET_CYCLE)
    # the shift reaches the output exactly: y - c is the unshifted problem up to the bf16 rounding of y (half an ulp at |c| + 4 s)
    w0 = w.clone()
    w0[..., NR.ONE % cg] = 0.0
    plain = NR._grouped_conv_ref(x, w0, stride, pad, groups)
    assert float((ops["y_ref"].double() - c.double() - plain.double()).abs().max()) <= 2.0 ** -8 * (64 * s + 6 * s)
    # measured, not assumed: the |mean| / std every channel really has after the bf16 rounding of y
    ratio = NR.mean_over_std(ops["y_ref"])
    rows = ops["y_ref"].numel() // Cout
    for cls, idx in NR.offset_classes(Cout).items():
        r = ratio[idx]
        print(f"{name}: offset {cls:2d} s, {rows} rows: |mean| / std {float(r.min()):.2f} .. {float(r.max()):.2f}")
        if cls:                      # (s is a power of two within sqrt(2) of the std; 9 or 25 rows scatter the sample std further)
            assert float(r.min()) >= cls / 3.0, (cls, r)
            assert rows < 100 or float(r.max()) <= 2.0 * cls, (cls, r)
        else:                        # (a ReLU output in front of the fused producer gives every channel a mean of its own)
            assert float(r.max()) <= (3.0 if name == "fused_1x1" else 1.0)


@pytest.mark.parametrize("name", list(NR.BN_PRODUCERS) + list(NR.BN_SPECIAL))
def test_bn_rounding_point_reference_stays_inside_what_the_gpu_tests_grant(name):
    """e_round per producer and offset class; the class-0 channels meet the existing tolerances outright; bf16_close's share for
    `out` and `dy` stays <= MAX_FRAC / 2 so that 2 x e_round is a share the issue allows"""
    ops = NR.bn_operands(name)
    y = ops["y_ref"]
    Cout = y.shape[-1]
    exact = NR.bn_exact(y, ops)
    points = NR.bn_points(y, ops, stats_rows(y), act=exact["out"])
    e_round = NR.bn_errors(points, exact, Cout)
    caps = NR.bn_caps(e_round)
    inv = NR.bn_invstd_rel_err(points["invstd"], exact, Cout)
    print(f"{name}: invstd e_round per class " + ", ".join(f"{c}: {v:.2e}" for c, v in inv.items()))
    for (q, cls), e in e_round.items():
        assert math.isfinite(e), (q, cls)
        if cls == 0 or q not in NR.BN_VARIANCE_BOUND:
            base = caps[(q, cls)]
            assert e <= base, (q, cls, e, base)
        if q.endswith("_share"):
            assert e <= NR.MAX_FRAC / 2, (q, cls, e)
    if name == "const_channel":
        assert float(exact["invstd"][NR.CONST_CH]) == pytest.approx(1.0 / math.sqrt(NR.BN_EPS), rel=1e-12)
        assert float(points["invstd"][NR.CONST_CH]) == pytest.approx(1.0 / math.sqrt(NR.BN_EPS), rel=1e-7)
        assert bool((y[..., NR.CONST_CH] == ops["c"][NR.CONST_CH]).all())
    if name == "count_1":
        assert torch.equal(exact["rv"], 0.9 * ops["rv0"].double())          # var = 0 and no n / (n - 1)


def test_bn_exact_agrees_with_autograd_in_the_randn_regime():
    ops = dict(NR.bn_operands("igemm"))
    y = NR.rnd_bf16(2, 9, 7, 128, seed=5)
    exact = NR.bn_exact(y, ops)
    yt = y.double().reshape(-1, 128).requires_grad_(True)
    gt, bt = ops["gamma"].double().requires_grad_(True), ops["beta"].double().requires_grad_(True)
    o = F.relu(F.batch_norm(yt, None, None, gt, bt, True, 0.1, NR.BN_EPS))
    o.backward(ops["dout"].double().reshape(-1, 128))
    assert R.rel_l2(exact["out"], R.bf16_round(o.detach().float()).reshape(y.shape)) <= 1e-6
    assert R.rel_l2(exact["dy"], R.bf16_round(yt.grad.float()).reshape(y.shape)) <= 1e-4
    assert R.rel_l2(exact["dgamma"], gt.grad) <= 1e-10 and R.rel_l2(exact["dbeta"], bt.grad) <= 1e-10


def test_gy_rounding_point_reference():
    """the second raw-product form on a stand-in g (the GPU test takes the kernel's own): e_round per offset class"""
    ops = NR.gy_operands()
    N, H, W, Cin, Cout = NR.GY_CASE
    assert NR.on_bf16_grid(ops["y"]) and float((ops["y"].reshape(-1, Cin).mean(0) - ops["c"]).abs().max()) <= 0.1
    g = R.bf16_round(R.conv2d_dgrad(ops["dy"], ops["w"], (H, W), 1, 0, ops["addend"] * ops["amask"], acc=F64) * ops["pmask"])
    exact = NR.gy_exact(g, ops["y"], ops["gamma"])
    points = NR.gy_points(g, ops["y"], exact, -(-(N * H * W) // 128))
    e_round = NR.gy_errors(points, exact, Cin)
    print("gy e_round: " + ", ".join(f"{q} {c}: {v:.2e}" for (q, c), v in e_round.items()))
    for (q, cls), e in e_round.items():
        assert math.isfinite(e)
        if cls == 0 or q == "dbeta":
            assert e <= NR.gy_caps(e_round)[(q, cls)], (q, cls, e)
        if q.endswith("_share"):
            assert e <= NR.MAX_FRAC / 2
    yt = ops["y"].double().reshape(-1, Cin).requires_grad_(True)
    gt = ops["gamma"].double().requires_grad_(True)
    F.batch_norm(yt, None, None, gt, torch.zeros(Cin, dtype=F64), True, 0.1, NR.BN_EPS).backward(g.double().reshape(-1, Cin))
    assert R.rel_l2(exact["dgamma"], gt.grad) <= 1e-9 and R.rel_l2(exact["dy"], R.bf16_round(yt.grad.float()).reshape(g.shape)) <= 1e-4


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", NR.LN_SHAPES)
def test_layernorm_rows_are_what_they_claim_and_the_restatement_meets_the_bounds(rows, C):
    ops = NR.ln_operands(rows, C)
    x, kinds = ops["x"], ops["kinds"]
    assert NR.on_bf16_grid(x) and NR.on_bf16_grid(ops["dy"]) and NR.on_bf16_grid(ops["addend"])
    seen = set()
    for shape in NR.LN_SHAPES:
        seen |= set(NR.ln_kind_of_row(shape[0]))
    assert seen == set(NR.LN_KINDS) and len(set(kinds)) == min(rows, len(NR.LN_KINDS))
    m, sd = x.double().mean(-1), x.double().std(-1)
    for r, kind in enumerate(kinds):
        if kind in NR.LN_CONST:
            assert bool((x[r] == NR.LN_CONST[kind]).all())
        elif kind in ("plus64", "minus64", "plus300"):
            want = {"plus64": 64.0, "minus64": -64.0, "plus300": 300.0}[kind]
            assert abs(float(m[r]) - want) <= 1.0 and 0.5 <= float(sd[r]) <= 2.0
        elif kind == "times2^20":
            assert 0.8 * 2 ** 20 <= float(sd[r]) <= 1.2 * 2 ** 20
        elif kind == "times2^-12":
            assert float(sd[r]) ** 2 <= 0.1 * min(NR.LN_EPS)                 # eps dominates the variance
    for eps in NR.LN_EPS:
        ry, rmean, rrstd = R.layernorm_fwd(x, ops["gamma"], ops["beta"], eps, acc=F64)
        if set(kinds) == {"randn"}:
            continue
        ky, kmean, krstd = NR.ln_fp32_restatement(x, ops["gamma"], ops["beta"], eps)
        atol = NR.ln_mean_atol(x, kinds)
        assert bool(((kmean.double() - rmean).abs() <= 1e-5 * rmean.abs() + atol).all())
        assert torch.allclose(krstd.double(), rrstd, rtol=1e-5, atol=1e-8)
        for r, kind in enumerate(kinds):
            if kind in NR.LN_CONST:
                bound = NR.ln_const_bound(NR.LN_CONST[kind], ops["gamma"], ops["beta"], eps)
                assert bool(((ky[r].double() - ops["beta"].double()).abs() <= bound).all()), (kind, eps)
                assert bool((bound <= 0.02 * ops["gamma"].abs() + 2.0 ** -7).all())       # the bound itself is small
            else:
                assert R.rel_l2(ky[r], ry[r]) <= 1e-3 and R.bf16_close(ky[r], ry[r]), (kind, eps)
    # torch in the randn rows
    idx = NR.ln_rows_of(kinds, ("randn",))
    if idx.numel():
        ry, _, _ = R.layernorm_fwd(x[idx], ops["gamma"], ops["beta"], 1e-6, acc=F64)
        assert R.max_bf16_ulp(ry, R.bf16_round(F.layer_norm(x[idx], (C,), ops["gamma"], ops["beta"], 1e-6))) <= 1.0


def test_patch_merge_scatter_inverts_the_gather():
    N, H, W, C = NR.PATCH_MERGE_SHAPE
    rows = N * (H // 2) * (W // 2)
    ops = NR.ln_operands(rows, 4 * C, seed=351)
    x = NR.patch_merge_scatter(ops["x"], N, H, W, C)
    ry, rmean, rrstd = patch_merge_ln_ref(x, ops["gamma"], ops["beta"], 1e-5)[:3]
    wy, wmean, wrstd = R.layernorm_fwd(ops["x"], ops["gamma"], ops["beta"], 1e-5, acc=F64)
    assert torch.allclose(rmean.double().flatten(), wmean, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rrstd.double().flatten(), wrstd, rtol=1e-12)
    assert R.max_bf16_ulp(R.bf16_round(ry.float()).reshape(rows, 4 * C), wy) <= 1.0


# ---- cross-entropy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,ld", NR.XENT_SHAPES)
def test_xent_rows_are_what_they_claim_and_the_restatement_meets_the_loss_bound(B, C, ld):
    seen = set()
    for start in NR.xent_batches(B):
        x, y1, y2, kinds = NR.xent_operands(B, C, start)
        seen |= set(kinds)
        assert NR.on_bf16_grid(x)
        lse = torch.logsumexp(x.double(), -1)
        for i, kind in enumerate(kinds):
            top = float(x[i].max())
            at_top = torch.nonzero(x[i] == top).flatten().tolist()
            if kind in NR.XENT_OFFSET:
                assert abs(float(lse[i]) - NR.XENT_OFFSET[kind]) <= 24.0
                if abs(NR.XENT_OFFSET[kind]) == 1024.0:
                    assert bool((x[i] % 4.0 == 0).all())                   # the bf16 grid at 1024: ties at the maximum abound
            elif kind == "peak_target":
                assert at_top == [int(y1[i])] and top - float(x[i].sort().values[-2]) >= 180.0
            elif kind == "peak_other":
                assert at_top == [(int(y1[i]) + 1) % C] and top - float(x[i].sort().values[-2]) >= 180.0
            elif kind == "equal":
                assert len(at_top) == C
            elif kind.startswith("tie"):
                assert sorted(at_top) == sorted(NR.tie_pair(kind, C))
        for smoothing, lam in ((0.0, 1.0), (0.1, 1.0), (0.1, 0.3)):
            ref = R.softmax_xent(x, y1, y2, lam, smoothing, 1.0, acc=F64)[0]
            got = NR.xent_fp32_restatement(x, y1, y2, lam, smoothing)
            e = (got.double() - ref).abs() / (1e-5 + 1e-4 * ref.abs())
            print(f"B {B} C {C} start {start} smoothing {smoothing} lam {lam}: fp32 restatement, loss excess per row "
                  + " ".join(f"{k}:{float(v):.2f}" for k, v in zip(kinds, e)))
            assert float(e.max()) <= 1.0, "the kernel's formula cannot meet allclose(1e-4, 1e-5) in fp32"
            equal = torch.tensor([k == "equal" for k in kinds])
            assert torch.allclose(ref[equal], ref.new_tensor(math.log(C)), rtol=1e-12)
    assert seen == set(NR.XENT_KINDS)


# ---- GRN, step kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,HW,C", NR.GRN_SHAPES)
def test_grn_operands(N, HW, C):
    ops = NR.grn_operands(N, HW, C)
    a, z = ops["a"], ops["z"]
    assert NR.on_bf16_grid(a) and NR.on_bf16_grid(z) and NR.on_bf16_grid(ops["dg"])
    assert float(a[:, :, NR.GRN_ZERO_CH].abs().max()) == 0.0 and float(a[N - 1].abs().max()) == 0.0
    assert float(z[:, :, NR.GRN_TAIL_CH].max()) <= -12.0
    G = (a[0].double() ** 2).sum(0).sqrt()
    live = [c for c in range(C) if c not in (NR.GRN_ZERO_CH, NR.GRN_TAIL_CH)]
    lg = torch.log2(G[live]) - ops["e"][live].double()
    assert float(lg.max() - lg.min()) <= 2.5                                  # the channel norms really span 2^-20 .. 2^10
    assert {int(v) for v in ops["e"][:8]} == set(NR.GRN_EXPONENTS)
    ref = grn_closed_form(a.double(), ops["gamma"].double(), ops["beta"].double(), ops["dg"].double())
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    assert float(ref["dweight"][NR.GRN_ZERO_CH]) == 0.0 and float(ref["da"][N - 1].sub(ops["dg"][N - 1].double()).abs().max()) == 0.0


def test_step_operands_and_reference():
    ops = NR.step_operands()
    n = NR.STEP_N
    assert n % 4 == 0 and ops["zero"].numel() >= 40
    e = torch.floor(torch.log2(ops["g"].abs().clamp_min(1e-300)))
    live = ops["g"] != 0
    for j, want in enumerate(NR.G_EXPONENTS):
        sel = live & (torch.arange(n) % 6 == j)
        assert abs(float(e[sel].float().median()) - want) <= 2
    pe = torch.log2(ops["p"].abs())
    assert float(pe.max()) >= 19 and float(pe.min()) <= -19
    assert bool((ops["p"][ops["zero"]].abs() <= 2.0 ** -17).all()) and bool((ops["v"] >= 0).all())
    # one fp64 step against torch.optim on these operands (the randn-regime pin is tests/test_oracle_cpu.py)
    p1, m1, v1 = R.optimizer_step_f64("adamw", ops["p"], ops["g"], torch.zeros(n), torch.zeros(n), 1e-3, 0.05, 1)
    tp = torch.nn.Parameter(ops["p"].double().clone())
    opt = torch.optim.AdamW([tp], lr=1e-3, weight_decay=0.05)
    tp.grad = ops["g"].double().clone()
    opt.step()
    assert torch.allclose(p1, tp.detach(), rtol=1e-12, atol=0.0)
