"""The kernels of csrc/window_attention.hip, csrc/se_ops.hip and csrc/conv_stem_deep.hip at the smallest shapes where their
grid-capped loops take SEVERAL trips per workgroup with a ragged last one -- what every training batch size does and no other
kernel test reaches: second and later trips, dead waves beside live ones, accumulators carried across trips (the dS accumulator of
the window-attention backward, dgamma / dbeta of patch merging, the register tiles of the thin weight gradient), LDS reused from
trip to trip, and the channel group of the SE elementwise passes, which holds only while the grid stride is a multiple of C / 8.

Every case first shows that it IS multi-trip, from the library's own workspace / row queries where there is one and from the
planner mirrors of tests/_multitrip.py otherwise (tests/test_multitrip_checks_cpu.py pins those mirrors to the trip counts below),
so that a change of a cap cannot quietly turn it into a one-trip test.

References are the ones of the kernels' own tests (oracle/swin_ref.py, tests/_se_kernels.py, oracle/ops_ref.py),
accumulated in fp64, on the GPU where the shape is large.  Bounds:
  * window attention: lse 1e-4 / 1e-4; out, dq, dk, dv, dbias global AND per 64 x 64 block under the bounds
    tests/test_fullsize_attention_long_gpu.py applies to icamd_attention_fwd / _bwd (3e-3 forward, 6e-3 backward, the
    gradients without the elementwise term);
  * patch merging, SE, thin 3x3: the bounds of tests/test_patch_merge_gpu.py, tests/test_se_kernels_gpu.py and
    tests/test_resnet_d_kernels_gpu.py plus the per-block term of tests/_fullsize_check.py (2e-3);
  * dgamma / dbeta of patch merging also per element: |got - ref| <= depth * 2^-24 * sum |terms|, depth = rows of a wave + 4 waves
    + P partials: the worst case of the fp32 summation chain the kernel forms (derived, not measured).
No bound here was set from a kernel's output.  Outputs are NaN-filled and carry guard bands that must come back untouched.

Like tests/test_fullsize_attention_long_gpu.py the module checks the default routing: an ICAMD_* variable in the environment is a
failure, not a skip."""
import ctypes

import pytest
import torch

import _harness
import _multitrip as MT
import _patch_merge as PM
import _se_kernels as SE
import _thin_conv as TC
import _window_attention as WA
from _fullsize_check import check_bf16, check_close, check_fp32, check_stats, require, worst_block
from _harness import INT, UNSUPPORTED, dev, digest, guarded, intact
from _harness import default_routing_lib as lib  # noqa: F401
from oracle.swin_ref import patch_merge_gather, patch_merge_ln_ref, window_attention_ref
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------- window attention
@pytest.mark.parametrize("case", list(MT.WINATTN_CASES))
def test_window_attention_multitrip(lib, case):
    B, Hs, Ws, H, ws, shift = case
    T, rows = ws * ws, B * Hs * Ws
    nwin = MT.winattn_nwin(B, Hs, Ws, ws)
    trips_f, trips_b = MT.WINATTN_CASES[case]
    # multi-trip, by the library's answer: P dbias partials per head = workgroups per head of the backward
    wsb = int(lib.icamd_window_attention_bwd_workspace_bytes(B, Hs, Ws, H, ws))
    P = wsb // (H * T * T * 4)
    assert P > 0 and 4 * P < nwin, (P, nwin)
    assert P == MT.winattn_bwd_grid(nwin, H) and MT.winattn_trips(nwin, P) == trips_b and nwin % (4 * P) != 0
    # the forward cap has no query: icamd_window_attention_fwd_launch, restated by MT.winattn_fwd_grid
    gf = MT.winattn_fwd_grid(nwin, H)
    assert MT.winattn_trips(nwin, gf) == trips_f and (trips_f == 1 or (4 * gf < nwin and nwin % (4 * gf) != 0))

    qkv, dout, bias = (t.to(DEV) for t in WA.operands(B, Hs, Ws, H, ws))
    rc_f, rc_b, out, lse, dqkv, dbias = WA.run(lib, qkv, dout, bias, *case)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    ro, rlse, rdqkv, rdbias = window_attention_ref(qkv, bias, B, Hs, Ws, H, ws, shift, dout=dout)
    if shift > 0:
        # all nine mask regions occur: rows [0, Hs - ws), [Hs - ws, Hs - shift), [Hs - shift, Hs) and the same in columns
        assert Hs > ws and Ws > ws and 0 < shift < ws
    ro, rd = ro.reshape(rows, H * WA.D), rdqkv.reshape(rows, 3 * H * WA.D)
    got_o, got_d = out.float(), dqkv.float()
    HD = H * WA.D
    parts = (("dq", slice(0, HD)), ("dk", slice(HD, 2 * HD)), ("dv", slice(2 * HD, 3 * HD)))
    print(f"case {case}: fwd grid {gf} x {trips_f} trips, bwd grid {P} x {trips_b} trips")
    print(f"    lse max abs err {float((lse.double().view(-1) - rlse.reshape(-1)).abs().max()):.3g}; "
          f"out rel_l2 {R.rel_l2(got_o, ro):.3g} worst block {worst_block(got_o, ro):.3g}")
    print("    " + "; ".join(f"{n} rel_l2 {R.rel_l2(got_d[:, s], rd[:, s]):.3g} worst block "
                             f"{worst_block(got_d[:, s].contiguous(), rd[:, s].contiguous()):.3g}" for n, s in parts))
    gb, rb = dbias.view(H * T, T), rdbias.reshape(H * T, T)
    print(f"    dbias rel_l2 {R.rel_l2(gb, rb):.3g} worst block {worst_block(gb, rb):.3g}")
    require(check_close(lse, rlse, 1e-4, 1e-4, "lse"), "window attention lse")
    require(check_bf16(got_o, ro, rel=3e-3, block_rel=3e-3, atol_rms=8e-3, max_frac=1e-6), "window attention fwd")
    for name, sl in parts:
        fails = [f for f in check_bf16(got_d[:, sl].contiguous(), rd[:, sl].contiguous(), rel=6e-3, block_rel=6e-3)
                 if "elementwise" not in f]
        require(fails, f"window attention bwd {name}")
    require(check_fp32(gb, rb, rel=6e-3, block_rel=6e-3), "window attention dbias")
    # accumulate = 1 adds the same sum onto what dbias held, bit for bit; a second run repeats every output bit for bit
    first = digest(out, lse, dqkv, dbias)
    fresh = dbias.clone()
    rc_f, rc_b, out2, lse2, dqkv2, added = WA.run(lib, qkv, dout, bias, *case, accumulate=1, dbias_fill=1.5)
    assert rc_f == 0 and rc_b == 0
    assert torch.equal(added, 1.5 + fresh)
    rc_f, rc_b, out3, lse3, dqkv3, dbias3 = WA.run(lib, qkv, dout, bias, *case)
    assert rc_f == 0 and rc_b == 0
    assert digest(out3, lse3, dqkv3, dbias3) == first


# ---------------------------------------------------------------------------------------------------------------- patch merging
@pytest.mark.parametrize("case", list(MT.PATCH_MERGE_CASES))
def test_patch_merge_ln_multitrip(lib, case):
    N, H, W, C = case
    rows = MT.patch_merge_rows(N, H, W)
    trips_f, trips_b = MT.PATCH_MERGE_CASES[case]
    # multi-trip, by the library's answer: P workgroups of four rows each, one partial [2][4C] per workgroup
    P = int(lib.icamd_patch_merge_ln_bwd_workspace_bytes(N, H, W, C)) // (8 * C * 4)
    assert P > 0 and 4 * P < rows, (P, rows)
    assert P == MT.patch_merge_bwd_grid(rows) and MT.patch_merge_trips(rows, P) == trips_b and rows % (4 * P) != 0
    # the forward cap has no query: icamd_patch_merge_ln_fwd_launch, restated by MT.patch_merge_fwd_grid
    assert MT.patch_merge_trips(rows, MT.patch_merge_fwd_grid(rows)) == trips_f

    x, gamma, beta, dy = PM.operands(N, H, W, C)
    ry, rmean, rrstd, rdx, rdg, rdb = patch_merge_ln_ref(x.to(DEV), gamma.to(DEV), beta.to(DEV), PM.EPS, dy=dy.to(DEV))
    rc_f, rc_b, y, mean, rstd, dx, grads = PM.run(lib, N, H, W, C, accs=(0, 1))
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    gy, gdx = y.float().view(rows, 4 * C), dx.float().view(N * H * W, C)
    ry, rdx = R.bf16_round(ry.float()), R.bf16_round(rdx.float()).reshape(N * H * W, C)
    xhat = (patch_merge_gather(x.to(DEV).double()) - rmean[:, None]) * rrstd[:, None]
    abs_g, abs_b = (dy.to(DEV).double() * xhat).abs().sum(0), dy.to(DEV).double().abs().sum(0)
    depth = MT.patch_merge_sum_depth(rows)
    dg, db = grads[0][0].to(DEV), grads[0][1].to(DEV)
    print(f"{case}: fwd {trips_f} trips, bwd grid {P} x {trips_b} trips; y rel_l2 {R.rel_l2(gy, ry):.3g} worst block "
          f"{worst_block(gy, ry):.3g}; dx rel_l2 {R.rel_l2(gdx, rdx):.3g} worst block {worst_block(gdx, rdx):.3g}")
    print(f"    dgamma rel_l2 {R.rel_l2(dg, rdg):.3g}, dbeta {R.rel_l2(db, rdb):.3g}; per element, in units of 2^-24 sum|terms| "
          f"(bound {depth}): dgamma {MT.sum_error_in_bound_units(dg, rdg, abs_g):.3g}, "
          f"dbeta {MT.sum_error_in_bound_units(db, rdb, abs_b):.3g}")
    assert torch.allclose(mean, rmean.float(), rtol=1e-5, atol=1e-6) and torch.allclose(rstd, rrstd.float(), rtol=1e-5)
    assert R.rel_l2(gy, ry) <= 1e-3 and R.bf16_close(gy, ry)
    assert R.rel_l2(gdx, rdx) <= 1e-3 and R.bf16_close(gdx, rdx)
    require(check_bf16(gy, ry, rel=1e-3), "patch merging y")                       # adds the per-block term
    require(check_bf16(gdx, rdx, rel=1e-3), "patch merging dx")
    for acc, (g1, b1) in enumerate(grads):      # the second call accumulates onto the first call's result
        assert R.rel_l2(g1, (1 + acc) * rdg.cpu()) <= 1e-4 and R.rel_l2(b1, (1 + acc) * rdb.cpu()) <= 1e-4, acc
    require(MT.check_fp32_sum(dg, rdg, abs_g, depth, "dgamma") + MT.check_fp32_sum(db, rdb, abs_b, depth, "dbeta"),
            "patch merging parameter gradients")
    # a second run repeats every output bit for bit
    rc_f, rc_b, y2, mean2, rstd2, dx2, grads2 = PM.run(lib, N, H, W, C, accs=(0,))
    assert rc_f == 0 and rc_b == 0
    assert digest(y, mean, rstd, dx, grads[0][0], grads[0][1]) == digest(y2, mean2, rstd2, dx2, grads2[0][0], grads2[0][1])


# ---------------------------------------------------------------------------------------------------------------- SE
_SE = {}


def se_case(case):
    """inputs of tests/_se_kernels.py for the shape, moved to the GPU, with its two references computed there"""
    if case not in _SE:
        c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in SE.inputs(*case).items()}
        c["ref"] = SE.tail(c, torch.float32)
        c["ref64"] = SE.tail(c, F64, c["ref"]["mask"])
        c["ysum64"] = c["y"].double().sum(1)
        _SE[case] = c
    return _SE[case]


def pack_bits(mask):
    w = 2 ** torch.arange(8, dtype=torch.int32, device=mask.device)
    return (mask.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def unpack_bits(bits):
    sh = torch.arange(8, dtype=torch.int32, device=bits.device)
    return ((bits.to(torch.int32).view(-1, 1) >> sh) & 1).flatten().bool()


def se_assert_multitrip(lib, case):
    N, HW, C, rd = case
    S_want, rps, blocks, trips = MT.SE_CASES[case]
    nb = int(lib.icamd_se_squeeze_workspace_bytes(N, HW, C))
    S = nb // (N * C * 4)
    assert S == S_want == MT.se_plan(N, HW)[0], (S, S_want)
    # the elementwise passes have no query: blocks_per_sample (csrc/se_ops.hip), restated by MT.se_blocks_per_sample
    assert MT.se_blocks_per_sample(N, HW, C // 8) == blocks and MT.se_apply_trips(N, HW, C // 8)[0] == trips
    assert (blocks * 256) % (C // 8) == 0
    if N == 256:
        assert S == MT.cdiv(2048, N) and S < MT.cdiv(HW, 32), "the segment plan must be limited by N here"
        assert HW % rps != 0 and trips >= 2 and (HW * (C // 8)) % (blocks * 256) != 0
    else:
        assert C // 8 > 256, "the second cg0 trip of se_reduce_kernel needs more than 256 channel groups"
    return nb


@pytest.mark.parametrize("case", list(MT.SE_CASES))
def test_se_forward_multitrip(lib, case):
    """icamd_se_squeeze, icamd_se_excite_fwd and icamd_se_bn_apply (plain residual and res_bn form) with the checks of
    tests/test_se_kernels_gpu.py test_squeeze_and_excite / test_gated_apply, plus the per-block term on out"""
    hip = _harness.hip()
    N, HW, C, rd = case
    nb = se_assert_multitrip(lib, case)
    c = se_case(case)
    ref = c["ref"]
    nan = float("nan")
    sp = hip.stream_ptr()
    yd = c["y"].to(torch.bfloat16)
    ysum, g_ysum = guarded((N, C), torch.float32, nan)
    ws, g_ws = guarded((nb,), torch.uint8, 0)
    assert lib.icamd_se_squeeze(hip.ptr(yd), hip.ptr(ysum), N, HW, C, hip.ptr(ws), nb, sp) == 0
    s, g_s = guarded((N, C), torch.float32, nan)
    e, g_e = guarded((N, C), torch.float32, nan)
    h, g_h = guarded((N, rd), torch.float32, nan)
    sc, sh = c["scale"].contiguous(), c["shift"].contiguous()
    w1, b1, w2, b2 = (c[k].contiguous() for k in ("W1", "b1", "W2", "b2"))
    assert lib.icamd_se_excite_fwd(hip.ptr(ysum), hip.ptr(sc), hip.ptr(sh), 1.0 / HW, hip.ptr(w1), hip.ptr(b1), hip.ptr(w2),
                                   hip.ptr(b2), hip.ptr(s), hip.ptr(h), hip.ptr(e), N, C, rd, sp) == 0
    for g in (g_ysum, g_ws, g_s, g_e, g_h):
        assert intact(g)
    errs = {"ysum": R.rel_l2(ysum, c["ysum64"]), "s": R.rel_l2(s, ref["s"]), "h": R.rel_l2(h, ref["h"]), "e": R.rel_l2(e, ref["e"])}
    print(case, {k: f"{v:.2e}" for k, v in errs.items()}, "gate range", float(ref["e"].min()), float(ref["e"].max()))
    assert float(ref["e"].min()) < 0.1 and float(ref["e"].max()) > 0.9 and float((ref["h"] > 0).float().mean()) > 0.2
    assert errs["ysum"] <= 1e-6
    assert errs["s"] <= 1e-5 and errs["h"] <= 1e-5 and errs["e"] <= 1e-5

    # the gated apply, fed the reference's gate
    eref = ref["e"].contiguous()
    resd = c["res"].to(torch.bfloat16)
    out, g_out = guarded((N * HW, C), torch.bfloat16, nan)
    bits, g_bits = guarded((N * HW * C // 8,), torch.uint8, 0xA5)
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(eref), hip.ptr(resd), None, None, hip.ptr(out),
                                 hip.ptr(bits), N, HW, C, 1, sp) == 0
    assert intact(g_out) and intact(g_bits)
    z, u = SE.apply_ref(c, c["res"])
    want = R.bf16_round(torch.relu(u)).view(N * HW, C)
    oc = out.float()
    print(case, "out: max ulp", R.max_bf16_ulp(oc, want), "rel-L2", R.rel_l2(oc, want), "worst block", worst_block(oc, want))
    assert R.max_bf16_ulp(oc, want) <= 1.0 and R.rel_l2(oc, want) <= 1e-3
    require(check_bf16(oc, want, rel=1e-3), "SE out")                              # adds the per-block term
    clear = (u != 0).flatten()
    assert float(clear.float().mean()) >= 0.99
    assert torch.equal(unpack_bits(bits)[clear], (u.flatten() > 0)[clear])
    assert torch.equal(unpack_bits(bits), oc.flatten() > 0)          # the bits are those of the stored output
    # the res_bn form == the plain form fed the shortcut icamd_bn_apply would have stored
    g = torch.Generator().manual_seed(77)
    raw = R.bf16_round(torch.randn(N, HW, C, generator=g) * 2 + 0.5).to(torch.bfloat16).to(DEV)
    rsc, rsh = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    pre = torch.empty_like(raw)
    assert lib.icamd_bn_apply(hip.ptr(raw), hip.ptr(rsc), hip.ptr(rsh), None, hip.ptr(pre), None, raw.numel(), C, 0, sp) == 0
    o1, g_o1 = guarded((N * HW, C), torch.bfloat16, nan)
    o2, g_o2 = guarded((N * HW, C), torch.bfloat16, nan)
    m1, g_m1 = guarded((N * HW * C // 8,), torch.uint8, 0xA5)
    m2, g_m2 = guarded((N * HW * C // 8,), torch.uint8, 0xA5)
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(eref), hip.ptr(raw), hip.ptr(rsc), hip.ptr(rsh),
                                 hip.ptr(o1), hip.ptr(m1), N, HW, C, 1, sp) == 0
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(eref), hip.ptr(pre), None, None, hip.ptr(o2),
                                 hip.ptr(m2), N, HW, C, 1, sp) == 0
    for g in (g_o1, g_o2, g_m1, g_m2):
        assert intact(g)
    assert R.max_bf16_ulp(o1.float(), o2.float()) <= 1.0 and R.rel_l2(o1.float(), o2.float()) <= 1e-3
    require(check_bf16(o1.float(), o2.float(), rel=1e-3), "SE out, res_bn form")
    assert torch.equal(unpack_bits(m1), o1.float().flatten() > 0)
    assert float(o1.float().abs().max()) > 0.0


def se_bwd_buffers(case, garbage):
    N, HW, C, rd = case
    shapes = {"dgamma": (C,), "dbeta": (C,), "dW1": (rd, C), "db1": (rd,), "dW2": (C, rd), "db2": (C,)}
    out, guards = {}, []
    for k, s in shapes.items():
        out[k], g = guarded(s, torch.float32, garbage)
        guards.append(g)
    out["dy"], g = guarded((N, HW, C), torch.bfloat16, float("nan"))
    return out, guards + [g]


@pytest.mark.parametrize("case", list(MT.SE_CASES))
def test_se_backward_multitrip(lib, case):
    """icamd_se_bn_bwd with the checks of tests/test_se_kernels_gpu.py test_backward, plus the per-block term on dy"""
    N, HW, C, rd = case
    se_assert_multitrip(lib, case)
    c = se_case(case)
    ref, ref64 = c["ref"], c["ref64"]
    noise = {k: R.rel_l2(ref[k], ref64[k].float()) for k in SE.GRADS + ("dy",)}
    print(case, "reference vs its fp64 copy:", {k: f"{v:.1e}" for k, v in noise.items()})
    for k in SE.GRADS + ("dy",):
        assert float(ref[k].abs().max()) > 0.0 and noise[k] <= 5e-5, (k, noise[k])
    dev = {k: c[k].contiguous() for k in ("mean", "invstd", "gamma", "beta", "W1", "W2")}
    dev.update(y=c["y"].to(torch.bfloat16), dout=c["dout"].to(torch.bfloat16), bits=pack_bits(ref["mask"]),
               ysum=c["y"].sum(1).contiguous(), s=ref["s"].contiguous(), h=ref["h"].contiguous(), e=ref["e"].contiguous())
    out, guards = se_bwd_buffers(case, 3.0)
    assert SE.run_bwd(lib, c, dev, out) == 0
    assert all(intact(g) for g in guards)
    errs = {k: R.rel_l2(out[k], ref[k]) for k in SE.GRADS}
    want_dy = R.bf16_round(ref["dy"]).view(N * HW, C)
    got_dy = out["dy"].float().view(N * HW, C)
    print(case, "HIP:", {k: f"{v:.1e}" for k, v in errs.items()}, "dy", f"{R.rel_l2(got_dy, want_dy):.1e}", "worst block",
          f"{worst_block(got_dy, want_dy):.3g}")
    assert R.rel_l2(got_dy, want_dy) <= 1e-3 and R.bf16_close(got_dy, want_dy)
    require(check_bf16(got_dy, want_dy, rel=1e-3), "SE dy")                        # adds the per-block term
    for k in SE.GRADS:
        assert errs[k] <= 1e-4, (k, errs[k])
    # two consecutive calls: bit-identical in every output
    out2, guards2 = se_bwd_buffers(case, -1.0)
    assert SE.run_bwd(lib, c, dev, out2) == 0
    for k in out:
        assert torch.equal(out[k].view(INT[out[k].element_size()]), out2[k].view(INT[out[k].element_size()])), k
    # accumulate = 1 on top of the first call: twice one call's worth
    assert SE.run_bwd(lib, c, dev, out2, accumulate=1) == 0
    assert all(intact(g) for g in guards2)
    for k in SE.GRADS:
        assert R.rel_l2(out2[k], 2.0 * out[k]) <= 1e-6, k
    assert torch.equal(out2["dy"].view(torch.int16), out["dy"].view(torch.int16))
    # gamma = beta = 0: the four SE gradients are exact zeros
    out0, _ = se_bwd_buffers(case, 5.0)
    zero = torch.zeros(C, device=DEV)
    assert SE.run_bwd(lib, c, dev, out0, gamma=zero, beta=zero) == 0
    for k in ("dW1", "db1", "dW2", "db2"):
        assert float(out0[k].abs().max()) == 0.0, k
    assert float(out0["dy"].float().abs().max()) == 0.0 and float(out0["dbeta"].abs().max()) > 0.0


@pytest.mark.parametrize("C,rd", [(4104, 16), (4096, 257)])
def test_se_refuses_what_is_past_the_contract_and_writes_nothing(lib, C, rd):
    """C = 4104 (a multiple of 8 past the 4096 limit) and rd = 257 (past 256)"""
    hip = _harness.hip()
    N, HW = 2, 4
    sp = hip.stream_ptr()
    f = lambda *shape: torch.full(shape, 7.0, device=DEV)                      # noqa: E731
    y = torch.full((N, HW, C), 7.0, dtype=torch.bfloat16, device=DEV)
    out, dy = torch.full_like(y, 7.0), torch.full_like(y, 7.0)
    bits = torch.full((N * HW * C // 8,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((1 << 22,), 7, dtype=torch.uint8, device=DEV)
    ysum, s, e, h = f(N, C), f(N, C), f(N, C), f(N, rd)
    vec = f(C)
    w1, w2, b1 = f(rd, C), f(C, rd), f(rd)
    grads = {k: f(*shp) for k, shp in (("dgamma", (C,)), ("dbeta", (C,)), ("dW1", (rd, C)), ("db1", (rd,)), ("dW2", (C, rd)),
                                       ("db2", (C,)))}
    if C > 4096:
        assert lib.icamd_se_squeeze(hip.ptr(y), hip.ptr(ysum), N, HW, C, hip.ptr(ws), ws.numel(), sp) == UNSUPPORTED
        assert lib.icamd_se_bn_apply(hip.ptr(y), hip.ptr(vec), hip.ptr(vec), hip.ptr(e), None, None, None, hip.ptr(out), hip.ptr(bits),
                                     N, HW, C, 1, sp) == UNSUPPORTED
    assert lib.icamd_se_excite_fwd(hip.ptr(ysum), hip.ptr(vec), hip.ptr(vec), 1.0 / HW, hip.ptr(w1), hip.ptr(b1), hip.ptr(w2),
                                   hip.ptr(vec), hip.ptr(s), hip.ptr(h), hip.ptr(e), N, C, rd, sp) == UNSUPPORTED
    assert lib.icamd_se_bn_bwd(hip.ptr(y), hip.ptr(bits), hip.ptr(y), hip.ptr(vec), hip.ptr(vec), hip.ptr(vec), hip.ptr(vec),
                               hip.ptr(ysum), hip.ptr(s), hip.ptr(h), hip.ptr(e), hip.ptr(w1), hip.ptr(w2), hip.ptr(grads["dgamma"]),
                               hip.ptr(grads["dbeta"]), hip.ptr(grads["dW1"]), hip.ptr(grads["db1"]), hip.ptr(grads["dW2"]),
                               hip.ptr(grads["db2"]), hip.ptr(dy), N, HW, C, rd, 0, hip.ptr(ws), ws.numel(), sp) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in [out, dy, ysum, s, e, h] + list(grads.values()):
        assert float(t.float().min()) == 7.0 and float(t.float().max()) == 7.0, "a refused call wrote to an output"
    assert bool((bits == 7).all()) and bool((ws == 7).all())


# ---------------------------------------------------------------------------------------------------------------- thin 3x3
def thin_assert_multitrip(lib, case):
    N, H, W, Cout = case
    d = TC.thin_inputs(case)[0]
    sbf, ntiles, sbw, ntw, S_want, tps = MT.THIN_CASES[case]
    assert MT.thin_plan(N, H, W, Cout) == (sbf, sbf, ntiles, sbw, ntw, S_want, tps)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # forward: one statistics row per tile; the persistent grid is 2 x CUs workgroups (launch_tile, csrc/conv_stem_deep.hip)
    rows = int(lib.icamd_conv3x3_thin_stats_rows(ctypes.byref(d)))
    assert rows == ntiles and rows > 2 * cus, (rows, cus)
    assert MT.cdiv(N * H * W, MT.thin_plan_tile(W, Cout * 2, 64)) > 2 * cus          # the data gradient's tiles (no query)
    # weight gradient: one fp32 slab per split
    need = int(lib.icamd_conv3x3_thin_wgrad_workspace_bytes(ctypes.byref(d)))
    S = need // (Cout * 9 * 32 * 4)
    assert S == S_want and S < ntw and MT.cdiv(ntw, S) == tps and ntw % tps != 0, (S, ntw)
    assert (N * H * W) % sbf != 0 and (N * H * W) % sbw != 0                          # ragged last tiles
    return d, rows


@pytest.mark.parametrize("case", list(MT.THIN_CASES))
def test_thin_forward_multitrip(lib, case):
    N, H, W, Cout = case
    d, rows = thin_assert_multitrip(lib, case)
    _, x, w, dy, bias, ref = TC.thin_inputs(case)
    xd, wd = dev(x), dev(w)
    stats, gs = guarded((rows, 2, Cout), torch.float32)
    y = TC.run_fwd(lib, d, xd, wd, stats=stats)
    assert intact(gs), "guard band behind the statistics written"
    got = y.float().cpu().reshape(-1, Cout)
    want = ref["y"].reshape(-1, Cout)
    print(case, "fwd rel_l2", R.rel_l2(got, want), "worst block", worst_block(got, want))
    assert R.rel_l2(got, want) <= 1e-3 and R.bf16_close(got, want)
    require(check_bf16(got, want, rel=1e-3), "thin fwd")                           # adds the per-block term
    assert torch.equal(TC.run_fwd(lib, d, xd, wd).view(torch.int16), y.view(torch.int16))      # without statistics: the same bytes
    stats_b, _ = guarded((rows, 2, Cout), torch.float32)
    assert torch.equal(TC.run_fwd(lib, d, xd, wd, stats=stats_b).view(torch.int16), y.view(torch.int16))
    assert torch.equal(stats.view(torch.int32), stats_b.view(torch.int32))         # run to run
    assert bool(torch.isfinite(stats).all())
    ssum = stats.cpu().double().sum(0)
    assert torch.allclose(ssum[0], got.double().sum(0), rtol=1e-5, atol=1e-3)
    assert torch.allclose(ssum[1], (got.double() ** 2).sum(0), rtol=1e-5, atol=1e-3)
    require(check_stats(stats.cpu(), got), "thin fwd statistics")
    # every partial row is the sum over ITS tile (a stale row of a later trip would keep the totals of another tile)
    sb = MT.THIN_CASES[case][0]
    yp = torch.cat([got.double(), torch.zeros(rows * sb - got.shape[0], Cout, dtype=F64)]).reshape(rows, sb, Cout)
    per_tile = torch.stack([yp.sum(1), (yp * yp).sum(1)], 1)
    scale = torch.stack([yp.abs().sum(1), (yp * yp).sum(1)], 1)
    assert bool(((stats.cpu().double() - per_tile).abs() <= sb * 2.0 ** -24 * scale).all()), "a statistics row is not its tile's"
    bd = bias.to(DEV)
    for relu, key in ((0, "z"), (1, "zr")):
        o = TC.run_fwd(lib, d, xd, wd, bias=bd, relu=relu).float().cpu().reshape(-1, Cout)
        assert R.rel_l2(o, ref[key].reshape(-1, Cout)) <= 1e-3 and R.bf16_close(o, ref[key])
        require(check_bf16(o, ref[key].reshape(-1, Cout), rel=1e-3), f"thin fwd with bias, relu {relu}")


@pytest.mark.parametrize("case", list(MT.THIN_CASES))
def test_thin_dgrad_multitrip(lib, case):
    d, _ = thin_assert_multitrip(lib, case)
    _, x, w, dy, bias, ref = TC.thin_inputs(case)
    dyd, wd = dev(dy), dev(w)
    dx = TC.run_dgrad(lib, d, dyd, wd)
    got, want = dx.float().cpu().reshape(-1, 32), ref["dx"].reshape(-1, 32)
    print(case, "dgrad rel_l2", R.rel_l2(got, want), "worst block", worst_block(got, want))
    assert R.rel_l2(got, want) <= 1e-3 and R.bf16_close(got, want)
    require(check_bf16(got, want, rel=1e-3), "thin dgrad")                         # adds the per-block term
    assert torch.equal(dx.view(torch.int16), TC.run_dgrad(lib, d, dyd, wd).view(torch.int16))


@pytest.mark.parametrize("case", list(MT.THIN_CASES))
def test_thin_wgrad_multitrip(lib, case):
    """through icamd_conv3x3_thin_wgrad itself: the models route this layer elsewhere by default, the entry is part of the ABI"""
    N, H, W, Cout = case
    d, _ = thin_assert_multitrip(lib, case)
    _, x, w, dy, bias, ref = TC.thin_inputs(case)
    xd, dyd = dev(x), dev(dy)
    dw = TC.run_wgrad(lib, d, xd, dyd)
    got, want = dw.cpu().double().reshape(Cout, -1), ref["dw"].reshape(Cout, -1)
    print(case, "wgrad rel_l2", R.rel_l2(got, want), "worst block", worst_block(got, want))
    assert R.rel_l2(got, want) <= 1e-4
    require(check_fp32(got, want, rel=1e-4), "thin wgrad")                         # adds the per-block term
    assert torch.equal(dw.view(torch.int32), TC.run_wgrad(lib, d, xd, dyd).view(torch.int32))       # fixed-order reduction
    old = torch.randn(Cout, 3, 3, 32, generator=torch.Generator().manual_seed(6))
    acc = TC.run_wgrad(lib, d, xd, dyd, prefill=old.to(DEV))
    assert R.rel_l2(acc.cpu().double(), old.double() + ref["dw"].double()) <= 1e-4
