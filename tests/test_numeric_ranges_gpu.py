"""The normalisation, loss, GELU / GRN, pooling and step kernels outside the band `randn` inputs keep them in.  Operands, fp64
references and bounds are those of tests/_numeric_ranges.py (tests/test_numeric_ranges_cpu.py keeps that file honest); every case
asserts the regime it claims (route, measured |mean| / std, lse range, tie positions, zero channel) before it compares numbers.

  BatchNorm      every statistics producer with channel offsets of 0, +-4, +-16, +-64 standard deviations inside one 8-channel vector:
                 finalize, apply, backward in its act / bits / recompute modes against fp64 references formed from the kernel's own
                 stored y with the centred variance; a constant channel (var = 0 exactly); count = 1; the backward's cancelling
                 forms (icamd_bn_bwd_from_gy_partials, icamd_conv2d_dgrad_bnbwd with the mask recomputed from y, icamd_conv1x1_bn_bwd_fused)
  LayerNorm      rows shifted by +-64 and +300, constant rows, rows times 2^20 and 2^-12 side by side in one wave's row group
  cross-entropy  logits shifted by +-64 and +-1024, peaked, all-equal, exact two-way ties at the maximum across lanes
  GELU           backward with da = 2^10, 2^-20; the fc1 epilogue with pre-activations shifted by +-12
  GRN, SE        channel norms from 2^-20 to 2^10, a zero channel, a zero sample, a channel in GELU's lower tail; SE with the channel
                 offsets and gates saturated at exactly 0 and 1
  max-pool       all-negative, mixed-sign and -0.0 / +0.0 inputs, values and recorded positions against F.max_pool2d
  step kernels   icamd_grad_norm -> clip -> every optimizer with gradients of element magnitude 2^-60 .. 2^20 and parameters of 2^+-20

What this file found when it was written (no kernel fault; the raw-moment BatchNorm variance is good to 1.3e-6 at every offset because
the sums are taken over bf16 values; optimizer scalars cross the C ABI as fp32) is under "Numeric-range tests" in DESIGN.md section 4."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _harness
import _numeric_ranges as NR
import _se_kernels as SE
from oracle.convnext_ref import GRN_EPS, gelu_grad, grn_closed_form
from _harness import dev as dev16
from _harness import lib, sync  # noqa: F401
from oracle.swin_ref import patch_merge_ln_ref
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


def finite(**tensors):
    bad = {n: int((~torch.isfinite(t.float())).sum()) for n, t in tensors.items()}
    assert not any(bad.values()), bad


# ======================================================================================================== BatchNorm
FORCED = {"pw_resident": {"ICAMD_PW_RESIDENT": "2"}, "gemm_nt": {"ICAMD_GEMM_NT": "2"}, "halo": {"ICAMD_CONV3X3_HALO": "2"}}
IN_PROCESS = [n for n in NR.BN_PRODUCERS if n not in FORCED]
# (K, N) pairs csrc/conv1x1_resident.hip instantiates (its pick())
_PW_PICK = lambda N, K: ((K in (64, 128, 256) and N % 256 == 0) or (K, N) in ((64, 64), (256, 64)) or (K == 256 and N % 128 == 0)  # noqa: E731
                         or (K == 512 and N % 128 == 0))


def conv2d_fwd_route(case):
    """Which kernel icamd_conv2d_fwd gives a statistics-form launch (no bias, no addend) of this small problem: the rules of
    conv_fwd_impl (csrc/capi.hip) in their order, with the route switches this process runs under.  The library has no query for
    it; this mirror holds for the shapes of this file only (no size floor is reached: every M here is far below them).  It is a copy
    of those rules (conv_fwd_impl, icamd_halo3x3_wanted, icamd_pw_resident_wanted and its pick(), icamd_pw_resident_ext_wanted,
    icamd_gemm_nt_wanted): asserting it checks what the test expects, not what the library launched, and it has to follow any change
    of the routing."""
    N, H, W, Cin, Cout, k, stride, pad, groups = case
    env = lambda n: int(os.environ.get(n, "1"))  # noqa: E731
    M = N * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
    if k == 3 and stride == 1 and pad == 1 and env("ICAMD_CONV3X3_HALO") != 0 and Cin % 64 == 0 and Cout % 8 == 0 and W >= 3 and H >= 3:
        resident = env("ICAMD_CONV3X3_RESIDENT") != 0 and Cin == 64 and Cout == 64 and W % 8 == 0 and 128 + 2 * W + 2 <= 255
        if resident:
            return "halo_resident"
        if (env("ICAMD_CONV3X3_HALO") != 1 or Cin >= 256) and 2 * W + 3 + 128 <= 256:
            return "halo"
    if k == 1 and pad == 0 and env("ICAMD_PW_RESIDENT") == 2 and _PW_PICK(Cout, Cin):
        return "pw_resident"
    assert M < 8192, "the size floors of the default routes are not mirrored"
    if k == 1 and stride == 1 and pad == 0 and env("ICAMD_GEMM_NT") == 2 and Cin % 32 == 0 and Cout % 8 == 0:
        return "gemm_nt"
    return "igemm"


def produce(lib, name, ops):
    """runs the statistics producer `name` on the operands: (y [N,OH,OW,C] bf16 on the device, partial rows [rows,2,C], rows)"""
    hip = _harness.hip()
    case = {**NR.BN_PRODUCERS, **NR.BN_SPECIAL}[name]
    N, H, W, Cin, Cout, k, stride, pad, groups = case
    d = hip.conv_desc(N, H, W, Cin, Cout, k, k, stride, pad)
    s = hip.stream_ptr()
    y = torch.full((N, d.OH, d.OW, Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    xd, wd = dev16(ops["x"]), dev16(ops["w"])
    if name == "gconv":
        assert lib.icamd_gconv3x3_supported(ctypes.byref(d), groups) == 1
        rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
        stats = torch.full((rows, 2, Cout), float("nan"), device=DEV)
        assert lib.icamd_gconv3x3_fwd(ctypes.byref(d), groups, hip.ptr(xd), hip.ptr(wd), hip.ptr(y), hip.ptr(stats), s) == 0
    elif name == "thin":
        assert lib.icamd_conv3x3_thin_supported(ctypes.byref(d)) == 1
        rows = lib.icamd_conv3x3_thin_stats_rows(ctypes.byref(d))
        stats = torch.full((rows, 2, Cout), float("nan"), device=DEV)
        assert lib.icamd_conv3x3_thin_fwd(ctypes.byref(d), hip.ptr(xd), hip.ptr(wd), hip.ptr(y), None, hip.ptr(stats), 0, s) == 0
    elif name == "stem7x7":
        rows = lib.icamd_stem7x7s2_stats_rows(N, H, W)
        stats = torch.full((rows, 2, Cout), float("nan"), device=DEV)
        x4 = torch.empty(N, H, W + 8, 4, dtype=torch.bfloat16, device=DEV)
        xn = ops["x"].permute(0, 3, 1, 2).contiguous().to(DEV)
        assert lib.icamd_pack_input_rgb4(hip.ptr(xn), hip.ptr(x4), N, 3, H, W, 0, 1.0, 0, 0, 0, 0, s) == 0
        wp = torch.zeros(Cout, 8, 8, 4)
        wp[:, :7, :7, :3] = ops["w"]
        wpd = dev16(wp)
        assert lib.icamd_stem7x7s2_fwd(hip.ptr(x4), hip.ptr(wpd), hip.ptr(y), None, hip.ptr(stats), 0, N, H, W, Cout, s) == 0
    elif name == "fused_1x1":
        # the block end in front of the convolution is the identity here: relu(x * 1 + 0 + 0) of the non-negative operand x
        assert lib.icamd_bn_apply_conv1x1_fused_supported(ctypes.byref(d)) == 1 and float(ops["x"].min()) >= 0.0
        rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
        stats = torch.full((rows, 2, Cout), float("nan"), device=DEV)
        one, zero, res = torch.ones(Cin, device=DEV), torch.zeros(Cin, device=DEV), torch.zeros_like(xd)
        out = torch.full_like(xd, float("nan"))
        bits = torch.zeros(xd.numel() // 8, dtype=torch.uint8, device=DEV)
        assert lib.icamd_bn_apply_conv1x1_fused(ctypes.byref(d), hip.ptr(xd), hip.ptr(one), hip.ptr(zero), hip.ptr(res), None, None,
                                                hip.ptr(out), hip.ptr(bits), hip.ptr(wd), hip.ptr(y), hip.ptr(stats), s) == 0
        sync()
        assert torch.equal(out, xd)
    else:
        want = {"const_channel": "igemm", "count_1": "igemm", "igemm_c2048": "igemm"}.get(name, name)
        assert conv2d_fwd_route(case) == want, (name, conv2d_fwd_route(case))
        rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
        stats = torch.full((rows, 2, Cout), float("nan"), device=DEV)
        assert lib.icamd_conv2d_fwd(ctypes.byref(d), hip.ptr(xd), hip.ptr(wd), hip.ptr(y), None, None, hip.ptr(stats), s) == 0
    sync()
    assert rows == -(-(N * d.OH * d.OW) // 128)
    return y, stats, rows


def run_bn_case(lib, name):
    """one producer: the regime, then finalize / apply / backward against the exact fp64 reference of the kernel's own y.
    Prints one line per offset class for the table in DESIGN.md; returns nothing, asserts everything."""
    hip = _harness.hip()
    ops = NR.bn_operands(name)
    y, stats, rows = produce(lib, name, ops)
    C = y.shape[-1]
    cnt = y.numel() // C
    yc = y.float().cpu()
    finite(y=yc, stats=stats.cpu())
    assert R.rel_l2(yc, ops["y_ref"]) <= 1e-3 and R.bf16_close(yc, ops["y_ref"])          # the producer computed the convolution
    ratio = NR.mean_over_std(yc)
    classes = NR.offset_classes(C)
    if name not in NR.BN_SPECIAL:
        for cls, idx in classes.items():
            if cls:
                assert float(ratio[idx].min()) >= cls / 3.0, (cls, float(ratio[idx].min()))
    # the partial rows are the sums of the values the kernel stored
    s1, s2 = R.conv2d_stats(yc)
    st = stats.double().cpu().sum(0)
    assert torch.allclose(st[0], s1, rtol=1e-5, atol=1e-3 * ops["s"]) and torch.allclose(st[1], s2, rtol=1e-5, atol=1e-3 * ops["s"] ** 2)

    s = hip.stream_ptr()
    gd, bd = ops["gamma"].to(DEV), ops["beta"].to(DEV)
    rmd, rvd = ops["rm0"].clone().to(DEV), ops["rv0"].clone().to(DEV)
    mean, invstd, scale, shift = (torch.full((C,), float("nan"), device=DEV) for _ in range(4))
    ws = torch.zeros(lib.icamd_bn_workspace_bytes(C), dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_train_finalize(hip.ptr(stats), rows, C, float(cnt), hip.ptr(gd), hip.ptr(bd), hip.ptr(rmd), hip.ptr(rvd),
                                       NR.BN_MOMENTUM, NR.BN_EPS, hip.ptr(mean), hip.ptr(invstd), hip.ptr(scale), hip.ptr(shift),
                                       hip.ptr(ws), s) == 0
    out = torch.full_like(y, float("nan"))
    bits = torch.zeros(y.numel() // 8, dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_apply(hip.ptr(y), hip.ptr(scale), hip.ptr(shift), None, hip.ptr(out), hip.ptr(bits), y.numel(), C, 1, s) == 0
    sync()
    oc = out.float().cpu()
    got = {"mean": mean.cpu(), "invstd": invstd.cpu(), "scale": scale.cpu(), "shift": shift.cpu(), "rm": rmd.cpu(), "rv": rvd.cpu(),
           "out": oc}
    finite(**got)
    # the apply kernel by itself, as test_bn_train_apply_and_bwd holds it: one fma of ITS coefficients, rounded once
    own = R.bn_apply(yc, got["scale"], got["shift"], None, True)
    assert R.max_bf16_ulp(oc, own) <= 1.0
    unpacked = ((bits.cpu().view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).flatten().bool()
    assert torch.equal(unpacked, oc.flatten() > 0)

    exact = NR.bn_exact(yc, ops, act=oc)
    points = NR.bn_points(yc, ops, rows, act=oc)
    doutd = dev16(ops["dout"])
    wsb = lib.icamd_bn_bwd_workspace_bytes(cnt, C)
    bws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    per_mode = {}
    for mode in ("act", "bits", "recompute"):
        dgam, dbet = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        dy, gout = torch.full_like(y, float("nan")), torch.full_like(y, float("nan"))
        assert lib.icamd_bn_bwd(hip.ptr(doutd), hip.ptr(out) if mode == "act" else None, hip.ptr(y), hip.ptr(mean), hip.ptr(invstd),
                                hip.ptr(scale), hip.ptr(shift), hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dy), hip.ptr(gout),
                                hip.ptr(bits) if mode == "bits" else None, cnt, C, 1, 0, hip.ptr(bws), wsb, s) == 0
        sync()
        per_mode[mode] = {"dy": dy.float().cpu(), "dgamma": dgam.cpu(), "dbeta": dbet.cpu()}
        finite(**per_mode[mode])
        assert torch.equal(gout.float().cpu(), R.bf16_round(ops["dout"] * (oc > 0)))

    e_round = NR.bn_errors(points, exact, C)
    caps = NR.bn_caps(e_round)
    inv_round, inv_got = NR.bn_invstd_rel_err(points["invstd"], exact, C), NR.bn_invstd_rel_err(got["invstd"], exact, C)
    for cls, idx in classes.items():
        r = ratio[idx]
        print(f"bn {name:13s} rows {cnt:5d} partial rows {rows:3d} offset {cls:2d} s: |mean|/std {float(r.min()):7.2f} .. "
              f"{float(r.max()):7.2f}  invstd rel err e_round {inv_round[cls]:.2e} kernel {inv_got[cls]:.2e}")
    failures = []
    for mode, bw in per_mode.items():
        measured = NR.bn_errors({**got, **bw}, exact, C)
        for key, e in measured.items():
            if not e <= caps[key]:
                failures.append((mode, key, e, caps[key], e_round[key]))
    assert not failures, failures
    if name == "const_channel":
        k = NR.CONST_CH
        assert bool((yc[..., k] == ops["c"][k]).all())                                      # the regime: var = 0 exactly
        assert float(got["invstd"][k]) == pytest.approx(1.0 / math.sqrt(NR.BN_EPS), rel=1e-6)
        assert float(got["mean"][k]) == float(ops["c"][k])
        for bw in per_mode.values():                       # xhat = (y - mean) * invstd = 0 exactly
            assert float(bw["dgamma"][k]) == 0.0
    if name == "count_1":
        assert cnt == 1 and bool((got["invstd"] == got["invstd"][0]).all())
        assert float(got["invstd"][0]) == pytest.approx(1.0 / math.sqrt(NR.BN_EPS), rel=1e-6)


@pytest.mark.parametrize("name", IN_PROCESS + list(NR.BN_SPECIAL))
def test_bn_statistics_under_channel_offsets(lib, name):
    run_bn_case(lib, name)


def test_bn_statistics_under_channel_offsets_forced_routes():
    """the resident pointwise, large-tile GEMM and 3x3 halo kernels take problems this small only when their switches force them,
    and the switches are read once per process: one child process runs the three cases (conv2d_fwd_route is asserted in it)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_numeric_ranges_gpu as T\n"
            "import _harness\n"
            "lib = _harness.load_lib()\n"
            "for name in T.FORCED:\n"
            "    T.run_bn_case(lib, name)\n"
            "print('forced-ok')\n") % (here, os.path.dirname(here))
    env = dict(os.environ)
    for switches in FORCED.values():
        env.update(switches)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "forced-ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]


def test_bn_bwd_from_gy_partials_under_channel_offsets(lib):
    """the backward's own raw-product form: icamd_conv2d_dgrad_bnred writes fp32 partial sums of g and g y, and
    icamd_bn_bwd_from_gy_partials turns them into sum g xhat = invstd (sum g y - mean sum g); y = randn + c_k, c_k up to +-64"""
    hip = _harness.hip()
    N, H, W, Cin, Cout = NR.GY_CASE
    d = hip.conv_desc(N, H, W, Cin, Cout, 1, 1, 1, 0)
    assert lib.icamd_conv2d_dgrad_bnred_supported(ctypes.byref(d)) == 1                    # the route
    M = N * H * W
    ops = NR.gy_operands()
    y, pmask, amask = ops["y"], ops["pmask"], ops["amask"]
    ratio = NR.mean_over_std(y)
    for cls, idx in NR.offset_classes(Cin).items():
        assert cls * 0.8 <= float(ratio[idx].min()) + 0.2 and float(ratio[idx].max()) <= cls * 1.2 + 0.2      # the regime
    pack = lambda m: (m.reshape(-1, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)  # noqa: E731
    dyd, wtd = dev16(ops["dy"]), dev16(ops["w"].permute(3, 1, 2, 0).contiguous())
    ad, yd, abits, pbits = dev16(ops["addend"]), dev16(y), pack(amask).to(DEV), pack(pmask).to(DEV)
    rows = lib.icamd_conv2d_dgrad_stats_rows(ctypes.byref(d))
    assert rows == -(-M // 128)
    part = torch.full((rows, 2, Cin), float("nan"), device=DEV)
    g = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_conv2d_dgrad_bnred(ctypes.byref(d), hip.ptr(dyd), hip.ptr(wtd), hip.ptr(g), hip.ptr(ad), hip.ptr(abits), 0,
                                        hip.ptr(yd), hip.ptr(pbits), hip.ptr(part), s) == 0
    sync()
    gc, pt = g.float().cpu(), part.double().cpu()
    finite(g=gc, part=pt)
    g_ref = R.conv2d_dgrad(ops["dy"], ops["w"], (H, W), 1, 0, ops["addend"] * amask, acc=F64) * pmask
    assert R.rel_l2(gc, g_ref) <= 1e-3 and R.bf16_close(gc, g_ref)
    sg, sgy = gc.double().reshape(-1, Cin).sum(0), (gc.double() * y.double()).reshape(-1, Cin).sum(0)
    assert torch.allclose(pt[:, 0].sum(0), sg, rtol=1e-5, atol=1e-2) and torch.allclose(pt[:, 1].sum(0), sgy, rtol=1e-5, atol=1e-2)
    exact = NR.gy_exact(gc, y, ops["gamma"])
    points = NR.gy_points(gc, y, exact, rows)
    md, isd, scd = exact["mean"].float().to(DEV), exact["invstd"].float().to(DEV), exact["scale"].float().to(DEV)
    dgam, dbet = torch.full((Cin,), float("nan"), device=DEV), torch.full((Cin,), float("nan"), device=DEV)
    dyo = torch.full_like(g, float("nan"))
    wsb = lib.icamd_bn_bwd_apply_workspace_bytes(Cin)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_bwd_from_gy_partials(hip.ptr(part), rows, hip.ptr(g), hip.ptr(yd), hip.ptr(md), hip.ptr(isd), hip.ptr(scd),
                                             hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dyo), M, Cin, 0, hip.ptr(ws), wsb, s) == 0
    sync()
    got = {"dy": dyo.float().cpu(), "dgamma": dgam.cpu(), "dbeta": dbet.cpu()}
    finite(**got)
    e_round, measured = NR.gy_errors(points, exact, Cin), NR.gy_errors(got, exact, Cin)
    caps = NR.gy_caps(e_round)
    for cls in NR.OFFSET_CLASSES:
        print(f"bn gy_partials    rows {M:5d} partial rows {rows:3d} offset {cls:2d} s: dgamma rel-L2 e_round {e_round[('dgamma', cls)]:.2e} "
              f"kernel {measured[('dgamma', cls)]:.2e}   dy e_round {e_round[('dy', cls)]:.2e} kernel {measured[('dy', cls)]:.2e}")
    bad = [(k, e, caps[k], e_round[k]) for k, e in measured.items() if not e <= caps[k]]
    assert not bad, bad


def test_conv_dgrad_bnbwd_under_channel_offsets(lib):
    """icamd_conv2d_dgrad_bnbwd + icamd_bn_bwd_from_partials with the BatchNorm input y = randn + c_k and the ReLU mask recomputed
    from y (y * scale + shift cancels to 1 part in 64 there): the masked gradient against the oracle's, the sums and dy against the
    fp64 BatchNorm backward of the g the kernel stored, under the bounds of test_conv_dgrad_with_fused_bn_backward"""
    hip = _harness.hip()
    N, H, W, Cin, Cout, k, st, pad = 3, 9, 7, 64, 128, 3, 1, 1
    d = hip.conv_desc(N, H, W, Cin, Cout, k, k, st, pad)
    gen = torch.Generator().manual_seed(396)
    dy = NR.rnd_bf16(N, d.OH, d.OW, Cout, seed=397)
    w = NR.rnd_bf16(Cout, k, k, Cin, scale=(1.0 / (k * k * Cout)) ** 0.5, seed=398)
    addend = NR.rnd_bf16(N, H, W, Cin, seed=399)
    c = torch.tensor([NR.OFFSET_CYCLE[i % 8] for i in range(Cin)])
    ybn = R.bf16_round(NR.rnd_bf16(N, H, W, Cin, seed=400) + c)
    ratio = NR.mean_over_std(ybn)
    for cls, idx in NR.offset_classes(Cin).items():
        assert cls * 0.7 <= float(ratio[idx].min()) + 0.3 and float(ratio[idx].max()) <= cls * 1.4 + 0.3      # the regime
    gamma, beta = torch.rand(Cin, generator=gen) + 0.5, torch.randn(Cin, generator=gen) * 0.3
    mean, invstd, scale, shift, _, _ = (t.float() for t in R.bn_train_coeffs(ybn, gamma, beta, torch.zeros(Cin), torch.ones(Cin), 0.1,
                                                                              NR.BN_EPS, acc=F64))
    act = R.bn_apply(ybn, scale, shift, None, True)        # one fp32 fma, as the kernel recomputes it
    assert 0.2 <= float((act > 0).float().mean()) <= 0.8
    dout = R.conv2d_dgrad(dy, w, (H, W), st, pad, addend, acc=F64)
    rg = R.bf16_round(dout * (act > 0))
    dyd, wtd, addd, ybnd = dev16(dy), dev16(w.permute(3, 1, 2, 0).contiguous()), dev16(addend), dev16(ybn)
    md, isd, scd, shd = mean.to(DEV), invstd.to(DEV), scale.to(DEV), shift.to(DEV)
    rows = lib.icamd_conv2d_dgrad_stats_rows(ctypes.byref(d))
    part = torch.full((rows, 2, Cin), float("nan"), device=DEV)
    gout = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=DEV)
    f = hip.BnBwdFuse(hip.ptr(ybnd), None, hip.ptr(md), hip.ptr(isd), hip.ptr(scd), hip.ptr(shd), hip.ptr(part), 1)
    s = hip.stream_ptr()
    assert lib.icamd_conv2d_dgrad_bnbwd(ctypes.byref(d), hip.ptr(dyd), hip.ptr(wtd), hip.ptr(gout), hip.ptr(addd), ctypes.byref(f), s) == 0
    wsb = lib.icamd_bn_bwd_apply_workspace_bytes(Cin)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    dgam, dbet = torch.full((Cin,), float("nan"), device=DEV), torch.full((Cin,), float("nan"), device=DEV)
    dyo = torch.full_like(gout, float("nan"))
    assert lib.icamd_bn_bwd_from_partials(hip.ptr(part), rows, hip.ptr(gout), hip.ptr(ybnd), hip.ptr(md), hip.ptr(isd), hip.ptr(scd),
                                          hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dyo), N * H * W, Cin, 0, hip.ptr(ws), wsb, s) == 0
    sync()
    gg, got = gout.float().cpu(), dyo.float().cpu()
    finite(g=gg, part=part.cpu(), dy=got, dgamma=dgam.cpu(), dbeta=dbet.cpu())
    assert R.rel_l2(gg, rg) <= 1e-3 and R.bf16_close(gg, rg)
    exact = NR.gy_exact(gg, ybn, gamma)
    for cls, idx in NR.offset_classes(Cin).items():
        eg, eb = R.rel_l2(dgam.cpu()[idx], exact["dgamma"][idx]), R.rel_l2(dbet.cpu()[idx], exact["dbeta"][idx])
        ed = R.rel_l2(got[..., idx], exact["dy"][..., idx])
        print(f"bn dgrad_bnbwd    offset {cls:2d} s: dgamma {eg:.2e} dbeta {eb:.2e} dy {ed:.2e}")
        assert eg <= 1e-4 and eb <= 1e-4, (cls, eg, eb)
        assert ed <= 2e-3 and R.bf16_close(got[..., idx], exact["dy"][..., idx], ulps=2.0, atol_rms=4e-3), (cls, ed)


def test_conv1x1_bn_bwd_fused_under_channel_offsets(lib):
    """icamd_conv1x1_bn_bwd_fused at its smallest routed shape with the BatchNorm input y = randn + c_k: from (sum g, sum g y) partial
    rows as icamd_conv2d_dgrad_bnred leaves them (fp32 sums per 128 rows), and with partials = NULL, where it forms sum g xhat itself;
    dgamma, dbeta, dx, dw against the fp64 chain BatchNorm backward -> data gradient / weight gradient, bounds of the sibling test"""
    hip = _harness.hip()
    N, H, W, Cin, Cout = 3, 75, 75, 64, 256
    d = hip.conv_desc(N, H, W, Cin, Cout, 1, 1, 1, 0)
    assert lib.icamd_conv1x1_bn_bwd_fused_supported(ctypes.byref(d)) == 1                  # the route
    M = N * H * W
    gen = torch.Generator().manual_seed(401)
    c = torch.tensor([NR.OFFSET_CYCLE[i % 8] for i in range(Cout)])
    g = NR.rnd_bf16(N, H, W, Cout, seed=402) * (torch.rand(N, H, W, Cout, generator=gen) > 0.45)
    y = R.bf16_round(NR.rnd_bf16(N, H, W, Cout, seed=403) + c)
    x = NR.rnd_bf16(N, H, W, Cin, seed=404).clamp_min(0)
    w = NR.rnd_bf16(Cout, 1, 1, Cin, scale=(1.0 / Cin) ** 0.5, seed=405)
    gamma = 0.5 + torch.rand(Cout, generator=gen)
    ratio = NR.mean_over_std(y)
    classes = NR.offset_classes(Cout)
    for cls, idx in classes.items():
        assert cls * 0.8 <= float(ratio[idx].min()) + 0.2 and float(ratio[idx].max()) <= cls * 1.2 + 0.2      # the regime
    exact = NR.gy_exact(g, y, gamma)
    rdx = R.conv2d_dgrad(exact["dy"], w, (H, W), 1, 0, None, acc=F64)
    rdw = R.conv2d_wgrad(x, exact["dy"], (1, 1), 1, 0, acc=F64)
    rows = -(-M // 128)
    g2, y2 = g.reshape(-1, Cout), y.reshape(-1, Cout)
    part = torch.stack([NR.fp32_partial_sums(g2, rows), NR.fp32_partial_sums(g2 * y2, rows)], 1).to(DEV).contiguous()
    e_round = NR.gy_errors(NR.gy_points(g, y, exact, rows), exact, Cout)
    gd, yd, xd, wtd = dev16(g), dev16(y), dev16(x), dev16(w.permute(3, 1, 2, 0).contiguous())
    md, isd, scd = exact["mean"].float().to(DEV), exact["invstd"].float().to(DEV), exact["scale"].float().to(DEV)
    s = hip.stream_ptr()
    wsb = lib.icamd_conv1x1_bn_bwd_fused_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    small = lib.icamd_bn_bwd_apply_workspace_bytes(Cout), lib.icamd_bn_bwd_workspace_bytes(M, Cout)
    for form, (partp, nrows, bwsb) in {"partials": (hip.ptr(part), rows, small[0]), "own sums": (None, 0, small[1])}.items():
        bws = torch.zeros(bwsb, dtype=torch.uint8, device=DEV)
        dx = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=DEV)
        dw = torch.full((Cout, Cin), float("nan"), device=DEV)
        dgam, dbet = torch.full((Cout,), float("nan"), device=DEV), torch.full((Cout,), float("nan"), device=DEV)
        assert lib.icamd_conv1x1_bn_bwd_fused(ctypes.byref(d), partp, nrows, hip.ptr(gd), hip.ptr(yd), hip.ptr(md), hip.ptr(isd),
                                              hip.ptr(scd), hip.ptr(dgam), hip.ptr(dbet), hip.ptr(xd), hip.ptr(wtd), hip.ptr(dx),
                                              hip.ptr(dw), 0, hip.ptr(bws), bwsb, hip.ptr(ws), wsb, s) == 0
        sync()
        gx, gw, gg, gb = dx.float().cpu(), dw.cpu().reshape(Cout, 1, 1, Cin), dgam.cpu(), dbet.cpu()
        finite(dx=gx, dw=gw, dgamma=gg, dbeta=gb)
        assert R.rel_l2(gx, rdx) <= 1e-3 and R.bf16_close(gx, rdx), (form, R.rel_l2(gx, rdx))
        for cls, idx in classes.items():
            eg, eb, ew = R.rel_l2(gg[idx], exact["dgamma"][idx]), R.rel_l2(gb[idx], exact["dbeta"][idx]), R.rel_l2(gw[idx], rdw[idx])
            print(f"bn conv1x1_bn_bwd_fused ({form}) offset {cls:2d} s: dgamma {eg:.2e} (e_round {e_round[('dgamma', cls)]:.2e}) "
                  f"dbeta {eb:.2e} dw {ew:.2e}")
            assert eg <= max(1e-4, 2.0 * e_round[("dgamma", cls)] if cls else 0.0) and eb <= 1e-4 and ew <= 1e-3, (form, cls, eg, eb, ew)


# ======================================================================================================== LayerNorm
def check_ln_forward(ops, eps, y, mean, rstd):
    x, kinds, gamma, beta = ops["x"], ops["kinds"], ops["gamma"], ops["beta"]
    ry, rmean, rrstd = R.layernorm_fwd(x, gamma, beta, eps, acc=F64)
    gy, gm, gr = y.float().cpu(), mean.cpu().double(), rstd.cpu().double()
    finite(y=gy, mean=gm, rstd=gr)
    assert bool(((gm - rmean).abs() <= 1e-5 * rmean.abs() + NR.ln_mean_atol(x, kinds)).all()), (gm - rmean).abs()
    assert torch.allclose(gr, rrstd, rtol=1e-5, atol=1e-8), ((gr - rrstd) / rrstd).abs().max()
    for kind in sorted(set(kinds)):
        idx = NR.ln_rows_of(kinds, (kind,))
        if kind in NR.LN_CONST:
            assert bool((x[idx] == NR.LN_CONST[kind]).all())
            bound = NR.ln_const_bound(NR.LN_CONST[kind], gamma, beta, eps)
            err = (gy[idx].double() - beta.double()).abs()
            assert bool((err <= bound).all()), (kind, float((err / bound).max()))
        else:
            assert R.rel_l2(gy[idx], ry[idx]) <= 1e-3 and R.bf16_close(gy[idx], ry[idx]), (kind, R.rel_l2(gy[idx], ry[idx]))
    return rmean, rrstd


def check_ln_backward(ops, eps, run_bwd, variants=NR.LN_BWD_VARIANTS):
    """run_bwd(dy, addend or None, mean, rstd) -> (dx [rows, C] fp32 cpu, dgamma, dbeta).  The backward takes the row statistics as
    inputs: it gets the fp64 reference's, rounded to fp32, so that it is held by itself (in a constant row the forward's own mean is
    off by up to |c| 2^-23, which rstd = 1 / sqrt(eps) turns into an xhat of a few 1e-3 where the exact one is 0)."""
    x, kinds, gamma = ops["x"], ops["kinds"], ops["gamma"]
    _, rmean, rrstd = R.layernorm_fwd(x, gamma, ops["beta"], eps, acc=F64)
    for dy_scale, use_addend in variants:
        dy = ops["dy"] * dy_scale
        rdx, rdg, rdb = R.layernorm_bwd(dy, x, gamma, eps, acc=F64)
        if use_addend:
            xf = x.double().requires_grad_(True)
            F.layer_norm(xf, (x.shape[-1],), gamma.double(), None, eps).backward(dy.double())
            rdx = R.bf16_round(xf.grad + ops["addend"].double())
        dx, dg, db = run_bwd(dy, ops["addend"] if use_addend else None, rmean.float(), rrstd.float())
        finite(dx=dx, dgamma=dg, dbeta=db)
        for kind in sorted(set(kinds)):
            idx = NR.ln_rows_of(kinds, (kind,))
            e = R.rel_l2(dx[idx], rdx[idx])
            assert e <= 1e-3 and R.bf16_close(dx[idx], rdx[idx]), (kind, dy_scale, use_addend, e)
        assert R.rel_l2(dg, rdg) <= 1e-4 and R.rel_l2(db, rdb) <= 1e-4, (dy_scale, R.rel_l2(dg, rdg), R.rel_l2(db, rdb))


@pytest.mark.parametrize("eps", NR.LN_EPS)
@pytest.mark.parametrize("rows,C", NR.LN_SHAPES)
def test_layernorm_ranges(lib, rows, C, eps):
    hip = _harness.hip()
    ops = NR.ln_operands(rows, C)
    xd, gd, bd = dev16(ops["x"]), ops["gamma"].to(DEV), ops["beta"].to(DEV)
    y = torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.full((rows,), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_layernorm_fwd(hip.ptr(xd), hip.ptr(gd), hip.ptr(bd), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), rows, C, eps, s) == 0
    sync()
    check_ln_forward(ops, eps, y, mean, rstd)
    wsb = lib.icamd_layernorm_bwd_workspace_bytes(rows, C)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)

    def run_bwd(dy, addend, rmean, rrstd):
        dyd, md, rd = dev16(dy), rmean.to(DEV), rrstd.to(DEV)
        ad = None if addend is None else dev16(addend)
        dx = torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        assert lib.icamd_layernorm_bwd(hip.ptr(dyd), hip.ptr(xd), hip.ptr(md), hip.ptr(rd), hip.ptr(gd), hip.ptr(ad), hip.ptr(dx),
                                       hip.ptr(dg), hip.ptr(db), rows, C, 0, hip.ptr(ws), wsb, s) == 0
        sync()
        return dx.float().cpu(), dg.cpu(), db.cpu()

    check_ln_backward(ops, eps, run_bwd)


@pytest.mark.parametrize("eps", NR.LN_EPS)
def test_patch_merge_layernorm_ranges(lib, eps):
    """the same rows through the 2x2 gather: x is the scatter of the merged matrix, so merged row r is of kind r % 9 (8 rows of 384)"""
    hip = _harness.hip()
    N, H, W, C = NR.PATCH_MERGE_SHAPE
    rows, C4 = N * (H // 2) * (W // 2), 4 * C
    ops = NR.ln_operands(rows, C4, seed=351)
    x = NR.patch_merge_scatter(ops["x"], N, H, W, C)
    ry = patch_merge_ln_ref(x, ops["gamma"], ops["beta"], eps)[0]
    assert R.max_bf16_ulp(R.bf16_round(ry.float()).reshape(rows, C4), R.layernorm_fwd(ops["x"], ops["gamma"], ops["beta"], eps,
                                                                                   acc=F64)[0]) <= 1.0      # the layout
    xd, gd, bd = dev16(x), ops["gamma"].to(DEV), ops["beta"].to(DEV)
    y = torch.full((rows, C4), float("nan"), dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.full((rows,), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_patch_merge_ln_fwd(hip.ptr(xd), hip.ptr(gd), hip.ptr(bd), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), N, H, W, C,
                                        eps, s) == 0
    sync()
    check_ln_forward(ops, eps, y, mean, rstd)
    wsb = max(int(lib.icamd_patch_merge_ln_bwd_workspace_bytes(N, H, W, C)), 256)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)

    def run_bwd(dy, addend, rmean, rrstd):
        dyd, md, rd = dev16(dy), rmean.to(DEV), rrstd.to(DEV)
        dx = torch.full((N, H, W, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        dg, db = torch.full((C4,), float("nan"), device=DEV), torch.full((C4,), float("nan"), device=DEV)
        assert lib.icamd_patch_merge_ln_bwd(hip.ptr(dyd), hip.ptr(xd), hip.ptr(md), hip.ptr(rd), hip.ptr(gd), hip.ptr(dx), hip.ptr(dg),
                                            hip.ptr(db), N, H, W, C, 0, hip.ptr(ws), wsb, s) == 0
        sync()
        # back to merged rows: the gather of dx
        dxc = dx.float().cpu()
        merged = torch.stack([dxc[:, a::2, b::2] for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))], 3).reshape(rows, C4)
        return merged, dg.cpu(), db.cpu()

    check_ln_backward(ops, eps, run_bwd, variants=tuple(v for v in NR.LN_BWD_VARIANTS if not v[1]))      # this entry has no addend


# ======================================================================================================== cross-entropy
@pytest.mark.parametrize("smoothing,lam", [(0.0, 1.0), (0.1, 1.0), (0.0, 0.3), (0.1, 0.3)])
@pytest.mark.parametrize("B,C,ld", NR.XENT_SHAPES)
def test_softmax_xent_ranges(lib, B, C, ld, smoothing, lam):
    hip = _harness.hip()
    s = hip.stream_ptr()
    for start in NR.xent_batches(B):
        x, y1, y2, kinds = NR.xent_operands(B, C, start)
        lp = torch.zeros(B, ld)
        lp[:, :C] = x
        lpd, y1d, y2d = dev16(lp), y1.to(DEV), y2.to(DEV)
        t = R.soft_targets(y1, y1 if lam == 1.0 else y2, lam, smoothing, C, dtype=F64)
        lse = torch.logsumexp(x.double(), -1)
        for i, kind in enumerate(kinds):                   # the regime, per row
            if kind in NR.XENT_OFFSET:
                assert abs(float(lse[i]) - NR.XENT_OFFSET[kind]) <= 24.0
            elif kind.startswith("peak"):
                assert float(x[i].max()) - float(x[i].sort().values[-2]) >= 180.0 and float(lse[i]) >= 180.0
            elif kind == "equal":
                assert float(lse[i]) == pytest.approx(2.5 + math.log(C), rel=1e-12)
        for gs in NR.XENT_GSCALES:
            gscale = 1.0 / B if gs == "1/B" else gs
            loss_rows = torch.full((B,), float("nan"), device=DEV)
            pred = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            dl = torch.full((B, ld), float("nan"), dtype=torch.bfloat16, device=DEV)
            assert lib.icamd_softmax_xent(hip.ptr(lpd), ld, B, C, hip.ptr(y1d), hip.ptr(y2d) if lam != 1.0 else None, lam, smoothing,
                                          gscale, hip.ptr(loss_rows), hip.ptr(pred), hip.ptr(dl), s) == 0
            sync()
            rl, rp, rd = R.softmax_xent(x, y1, y2 if lam != 1.0 else None, lam, smoothing, gscale, acc=F64)
            gl, gp, gd = loss_rows.cpu().double(), pred.cpu().long(), dl.float().cpu()
            finite(loss=gl, dlogits=gd)
            e = (gl - rl).abs() / (1e-5 + 1e-4 * rl.abs())
            if gs == "1/B":
                print(f"xent B {B} C {C} start {start} smoothing {smoothing} lam {lam}: lse {float(lse.min()):.1f} .. {float(lse.max()):.1f}, "
                      f"loss {float(rl.min()):.3g} .. {float(rl.max()):.3g}, loss excess " + " ".join(f"{k}:{float(v):.2f}" for k, v in zip(kinds, e)))
            assert float(e.max()) <= 1.0, list(zip(kinds, e.tolist()))                     # allclose(rtol 1e-4, atol 1e-5)
            assert torch.equal(gp, rp), (kinds, gp, rp)                                     # the lowest index wins a tie
            assert torch.equal(gd[:, C:], torch.zeros(B, ld - C))
            assert R.rel_l2(gd[:, :C], rd) <= 2e-3, R.rel_l2(gd[:, :C], rd)
            # element by element: the rounding and the fast exponential, whatever the row's neighbours weigh in the norm above
            x64 = x.double().requires_grad_(True)
            (-(t * F.log_softmax(x64, -1)).sum() * gscale).backward()
            big = torch.maximum(gd[:, :C].double().abs(), x64.grad.abs())
            slack = NR.bf16_ulp(big) + NR.xent_grad_slack(x64.grad, gscale, x, t)
            assert bool(((gd[:, :C].double() - x64.grad).abs() <= slack).all())
            for i, kind in enumerate(kinds):
                if kind == "equal":                        # analytic, no oracle
                    assert abs(float(gl[i]) - math.log(C)) <= 1e-5 + 1e-4 * math.log(C) and int(gp[i]) == 0
                    want = (1.0 / C - t[i]) * gscale
                    assert bool(((gd[i, :C].double() - want).abs() <= NR.bf16_ulp(want) + 2.0 ** -20 * gscale).all())
                elif kind.startswith("tie"):
                    a, b = NR.tie_pair(kind, C)
                    assert float(x[i, a]) == float(x[i, b]) == float(x[i].max()) and int(gp[i]) == min(a, b)


def test_step_metrics_folds_losses_of_0_001_and_400(lib):
    """icamd_step_metrics over the losses of such a batch: the fp64 fold sees 1e-3 and 4e2 together"""
    hip = _harness.hip()
    B, C, ld = NR.XENT_SHAPES[0]
    x, y1, y2, kinds = NR.xent_operands(B, C, 0)
    i, j = kinds.index("peak_target"), kinds.index("peak_other")
    x[i] = 0.0
    x[i, int(y1[i])] = 14.0                                # loss = log(1 + 999 e^-14) = 8.3e-4
    x[j, (int(y1[j]) + 1) % C] += 200.0                    # 400 above the rest
    x = R.bf16_round(x)
    rl, rp, _ = R.softmax_xent(x, y1, None, 1.0, 0.0, 1.0, acc=F64)
    assert 5e-4 <= float(rl.min()) <= 2e-3 and 380.0 <= float(rl.max()) <= 420.0
    lp = torch.zeros(B, ld)
    lp[:, :C] = x
    lpd, y1d = dev16(lp), y1.to(DEV)
    loss_rows, pred = torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_softmax_xent(hip.ptr(lpd), ld, B, C, hip.ptr(y1d), None, 1.0, 0.0, 1.0, hip.ptr(loss_rows), hip.ptr(pred), None, s) == 0
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    counts = torch.zeros(3, C, dtype=torch.int32, device=DEV)
    loss_out, fin = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.icamd_step_metrics(hip.ptr(loss_rows), hip.ptr(pred), hip.ptr(y1d), B, C, hip.ptr(loss_out), hip.ptr(fin), hip.ptr(acc),
                                  hip.ptr(counts), None, 0, 0, 1, s) == 0
    sync()
    assert int(fin.item()) == 1
    assert torch.allclose(loss_rows.cpu().double(), rl, rtol=1e-4, atol=1e-5)
    want = float(loss_rows.cpu().double().mean())          # of the values the kernel stored, folded in fp64
    assert abs(loss_out.item() - want) <= 2.0 ** -23 * want and abs(acc[0].item() - loss_out.item()) <= 1e-12 * want
    correct = int((rp == y1).sum())
    assert acc[3].item() == correct and acc[4].item() == B


# ======================================================================================================== GELU
def gelu_exact(z):
    zz = z.double()
    cdf = 0.5 * (1.0 + torch.erf(zz / 2 ** 0.5))
    return zz * cdf, cdf + zz * torch.exp(-0.5 * zz * zz) / (2 * math.pi) ** 0.5


@pytest.mark.parametrize("da_scale", [2.0 ** 10, 2.0 ** -20])
def test_gelu_bwd_scaled_upstream_gradient(lib, da_scale):
    """dz = da gelu'(z) over every finite bf16 z with |z| <= 16 and da = +-da_scale: the bound of test_gelu_and_colsum_rows scaled
    by |da| (|err| <= |da| (2^-8 |gelu'| + 1e-6)), which is exact for a power of two"""
    hip = _harness.hip()
    allz = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    allz = allz[torch.isfinite(allz) & (allz.abs() <= 16.0)]
    allz = torch.cat([allz, torch.zeros((-allz.numel()) % 8)])
    da = torch.full_like(allz, da_scale)
    da[1::2] = -da_scale
    zd, dad = dev16(allz), dev16(da)
    dz = torch.full_like(zd, float("nan"))
    assert lib.icamd_gelu_bwd(hip.ptr(dad), hip.ptr(zd), hip.ptr(dz), allz.numel(), hip.stream_ptr()) == 0
    sync()
    got = dz.float().cpu().double()
    finite(dz=got)
    exact = da.double() * gelu_exact(allz)[1]
    err = (got - exact).abs()
    assert bool((err <= exact.abs() * 2.0 ** -8 + 1e-6 * da_scale).all()), float((err / (exact.abs() * 2.0 ** -8 + 1e-6 * da_scale)).max())


GELU_Z_CYCLE = (0.0, 12.0, -12.0, 0.0, 4.0, -4.0, 12.0, -12.0)


def test_conv_gelu_epilogue_with_shifted_preactivations(lib):
    """icamd_conv2d_fwd_gelu at (2,8,8,96->384) with z offsets of +-12 carried through a constant input channel: z against the fp64
    convolution, a against the exact GELU of the z the kernel stored, under the bound of test_gelu_and_colsum_rows"""
    hip = _harness.hip()
    N, H, W, Cin, Cout = 2, 8, 8, 96, 384
    d = hip.conv_desc(N, H, W, Cin, Cout, 1, 1, 1, 0)
    # the route: M = 128 is below the floor (8192 rows) of the K = 96 resident form and K below the large-tile GEMM's 768
    assert conv2d_fwd_route((N, H, W, Cin, Cout, 1, 1, 0, 1)) == "igemm"
    x = NR.rnd_bf16(N, H, W, Cin, seed=361)
    w = NR.rnd_bf16(Cout, 1, 1, Cin, scale=(1.0 / Cin) ** 0.5, seed=362)
    c = torch.tensor([GELU_Z_CYCLE[k % 8] for k in range(Cout)])
    x[..., NR.ONE] = 1.0
    w[:, 0, 0, NR.ONE] = c
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(363)) * 0.1
    xd, wd, bd = dev16(x), dev16(w), bias.to(DEV)
    z = torch.full((N, H, W, Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    a, a_only = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
    s = hip.stream_ptr()
    assert lib.icamd_conv2d_fwd_gelu(ctypes.byref(d), hip.ptr(xd), hip.ptr(wd), hip.ptr(z), hip.ptr(a), hip.ptr(bd), s) == 0
    assert lib.icamd_conv2d_fwd_gelu(ctypes.byref(d), hip.ptr(xd), hip.ptr(wd), None, hip.ptr(a_only), hip.ptr(bd), s) == 0
    sync()
    zc, ac = z.float().cpu(), a.float().cpu()
    finite(z=zc, a=ac)
    m = zc.reshape(-1, Cout).mean(0)
    assert float((m - c - bias).abs().max()) <= 1.0 and float(zc.min()) <= -14.0 and float(zc.max()) >= 14.0     # the regime
    rz = R.conv2d_fwd(x, w, 1, 0, bias, None, acc=F64)
    assert R.rel_l2(zc, rz) <= 1e-3 and R.bf16_close(zc, rz)
    exact = gelu_exact(zc)[0]
    err = (ac.double() - exact).abs()
    assert bool((err <= exact.abs() * 2.0 ** -8 + 1e-6).all()), float(err.max())
    assert torch.equal(a, a_only)


# ======================================================================================================== GRN
@pytest.mark.parametrize("with_gelu", [False, True])
@pytest.mark.parametrize("N,HW,C", NR.GRN_SHAPES)
def test_grn_ranges(lib, N, HW, C, with_gelu):
    hip = _harness.hip()
    assert lib.icamd_grn_supported(N, HW, C) == 1
    ops = NR.grn_operands(N, HW, C)
    a, z, dg, gamma, beta = ops["a"], ops["z"], ops["dg"], ops["gamma"], ops["beta"]
    zc, tc = NR.GRN_ZERO_CH, NR.GRN_TAIL_CH
    assert float(a[:, :, zc].abs().max()) == 0.0 and float(a[N - 1].abs().max()) == 0.0 and float(z[:, :, tc].max()) <= -12.0
    ad, zd, dgd, gd, bd = dev16(a), dev16(z), dev16(dg), gamma.to(DEV), beta.to(DEV)
    nbytes = lib.icamd_grn_workspace_bytes(N, HW, C)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    g = torch.full_like(ad, float("nan"))
    gx = torch.full((N, C), float("nan"), device=DEV)
    dx = torch.full_like(ad, float("nan"))
    dgam, dbet = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_grn_fwd(ad.data_ptr(), gd.data_ptr(), bd.data_ptr(), g.data_ptr(), gx.data_ptr(), N, HW, C, GRN_EPS, ws.data_ptr(),
                             nbytes, s) == 0
    assert lib.icamd_grn_bwd(dgd.data_ptr(), ad.data_ptr(), gx.data_ptr(), gd.data_ptr(), zd.data_ptr() if with_gelu else None,
                             dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), 0, N, HW, C, GRN_EPS, ws.data_ptr(), nbytes, s) == 0
    sync()
    gc, gxc, dxc, dgc, dbc = g.float().cpu(), gx.cpu(), dx.float().cpu(), dgam.cpu(), dbet.cpu()
    finite(g=gc, gx=gxc, dx=dxc, dgamma=dgc, dbeta=dbc)
    ref = grn_closed_form(a.double(), gamma.double(), beta.double(), dg.double())
    r32 = grn_closed_form(a.float(), gamma, beta, dg.float())
    want_dx = ref["da"] * gelu_grad(z.double()) if with_gelu else ref["da"]
    # exact zeros where exact arithmetic gives them
    assert float(gxc[:, zc].abs().max()) == 0.0 and float(gxc[N - 1].abs().max()) == 0.0
    assert float(dgc[zc]) == 0.0
    if not with_gelu:                                      # da = dg * 1 + 0 * t in the zero channel and in the zero sample
        assert torch.equal(dxc[:, :, zc], dg[:, :, zc]) and torch.equal(dxc[N - 1], dg[N - 1])
    else:                                                  # the same da = dg through gelu'(z), under the GELU bound scaled by |da|
        for got_z, dg_z, z_z in ((dxc[:, :, zc], dg[:, :, zc], z[:, :, zc]), (dxc[N - 1], dg[N - 1], z[N - 1])):
            want = dg_z.double() * gelu_grad(z_z.double())
            assert bool(((got_z.double() - want).abs() <= want.abs() * 2.0 ** -8 + 1e-6 * dg_z.double().abs()).all())
    assert torch.equal(gc[N - 1], R.bf16_round(beta).expand(HW, C))           # g = 0 * s + beta
    # per channel magnitude: a norm over all channels would be the 2^10 channels' alone
    e = ops["e"]
    for ex in NR.GRN_EXPONENTS:
        idx = torch.nonzero(e == ex).flatten()
        idx = idx[(idx != zc) & (idx != tc)]
        for name, got, want in (("g", gc, ref["g"]), ("dx", dxc, want_dx)):
            err = R.rel_l2(got[:, :, idx], R.bf16_round(want[:, :, idx].float()))
            assert err <= 1e-3, (name, ex, err)
        for name, got, key in (("gx", gxc, "gx"), ("dgamma", dgc, "dweight"), ("dbeta", dbc, "dbias")):
            sel = (slice(None), idx) if name == "gx" else (idx,)
            err, floor = R.rel_l2(got[sel], ref[key][sel]), R.rel_l2(r32[key][sel], ref[key][sel])
            assert err <= max(10.0 * floor, 1e-6), (name, ex, err, floor)
    # the tail channel: |a| <= 12 Phi(-12) 2^e ~ 1e-32, whose square is below fp32: the kernels see Gx = 0 and take it for a zero
    # channel (the exact da keeps a term -K a / Gx, a unit vector times the sample's scalar K, which only means something if a
    # gradient could pass GELU at z <= -12: gelu'(z) ~ 1e-31).  Held: g = beta there, and with the GELU pass dz is nothing.
    assert float((gc[:N - 1, :, tc].double() - R.bf16_round(beta)[tc].double()).abs().max()) <= float(NR.bf16_ulp(beta[tc].double()))
    if with_gelu:
        assert float(dxc[:, :, tc].abs().max()) <= 1e-20 and float(want_dx[:, :, tc].abs().max()) <= 1e-20


# ======================================================================================================== squeeze-excitation
def se_case():
    """the smallest case of tests/_se_kernels.py that has more than one pixel per sample, with the channel offsets of the BatchNorm part added to y (in units of each
    channel's own width) and b2 = +-100 in two channels: gates of exactly 1 and exactly 0, whose backward contribution is 0"""
    N, HW, C, rd = min((c for c in SE.CASES if c[1] > 1), key=lambda c: c[0] * c[1] * c[2])
    c = SE.inputs(N, HW, C, rd)
    width = c["y"].double().std((0, 1)).float()
    off = torch.tensor([NR.OFFSET_CYCLE[k % 8] for k in range(C)])
    c["y"] = R.bf16_round(c["y"] + off * torch.exp2(torch.round(torch.log2(width))))
    c["b2"][SE_ONE], c["b2"][SE_ZERO] = 100.0, -100.0
    yy = c["y"].double()
    mean = yy.mean((0, 1))
    invstd = 1.0 / torch.sqrt(((yy - mean) ** 2).mean((0, 1)) + SE.EPS)
    c["mean"], c["invstd"] = mean.float(), invstd.float()
    c["scale"] = c["gamma"] * c["invstd"]
    c["shift"] = c["beta"] - c["mean"] * c["scale"]
    c["ref"] = SE.tail(c, F64)
    c["ysum64"] = yy.sum(1)
    return c


SE_ONE, SE_ZERO = 9, 22


def test_squeeze_excitation_ranges(lib):
    c = se_case()
    N, HW, C, rd = c["shape"]
    ref = c["ref"]
    ratio = NR.mean_over_std(c["y"])
    for cls, idx in NR.offset_classes(C).items():
        if cls:                                            # (each sample has a shift of its own: the ratio is not the nominal one)
            assert float(ratio[idx].min()) >= cls / 3.0
    pre = ref["h"] @ c["W2"].double().t() + c["b2"].double()
    assert float(pre[:, SE_ONE].min()) >= 90.0 and float(pre[:, SE_ZERO].max()) <= -90.0          # the regime
    _, _, _, ysum, s, h, e = SE.forward_on_gpu(lib, c)
    ysum, s, h, e = ysum.cpu(), s.cpu(), h.cpu(), e.cpu()
    finite(ysum=ysum, s=s, h=h, e=e)
    assert bool((e[:, SE_ONE] == 1.0).all()) and bool((e[:, SE_ZERO] == 0.0).all())
    assert R.rel_l2(ysum, c["ysum64"]) <= 1e-6
    # s = scale * ysum / HW + shift cancels in the offset channels (64 gamma - 64 gamma + beta): its fp32 restatement against the
    # exact one is e_round, and the bound max(1e-5, 2 e_round) as for the BatchNorm coefficients; h and e follow s
    s_points = (c["scale"] * ysum * torch.tensor(1.0 / HW)) + c["shift"]
    e_round = R.rel_l2(s_points, ref["s"])
    errs = {"s": R.rel_l2(s, ref["s"]), "h": R.rel_l2(h, ref["h"]), "e": R.rel_l2(e, ref["e"])}
    print(f"se {c['shape']}: s e_round {e_round:.2e}, kernel " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= max(1e-5, 2.0 * e_round), (k, v, e_round)
    # backward, fed the exact forward (the kernel by itself, as test_backward feeds it)
    dev = SE.bwd_inputs(c)
    out = SE.bwd_buffers(c, garbage=3.0)
    assert SE.run_bwd(lib, c, dev, out) == 0
    got = {k: out[k].float().cpu() for k in out}
    finite(**got)
    want_dy = R.bf16_round(ref["dy"].float())
    assert R.rel_l2(got["dy"], want_dy) <= 1e-3 and R.bf16_close(got["dy"], want_dy), R.rel_l2(got["dy"], want_dy)
    for k in SE.GRADS:
        assert R.rel_l2(got[k], ref[k]) <= 1e-4, (k, R.rel_l2(got[k], ref[k]))
    # e (1 - e): nothing flows into the saturated gates.  The backward is fed the reference's e, which is 1 in fp32 in the one
    # channel (exact zeros) and the denormal sigmoid(-100) = 3.7e-44 in the other (nothing above 1e-40, and finite)
    assert float(got["dW2"][SE_ONE].abs().max()) == 0.0 and float(got["db2"][SE_ONE]) == 0.0
    assert float(got["dW2"][SE_ZERO].abs().max()) <= 1e-40 and abs(float(got["db2"][SE_ZERO])) <= 1e-40
    assert float(ref["dW2"][SE_ONE].abs().max()) <= 1e-40 and float(ref["dW2"][SE_ZERO].abs().max()) <= 1e-40


# ======================================================================================================== max-pool
def pool_inputs(kind):
    x = NR.rnd_bf16(3, 9, 11, 64, seed=371)
    if kind == "negative":
        return R.bf16_round(-x.abs() - 0.5)
    if kind == "zeros":
        g = torch.Generator().manual_seed(372)
        x = -x.abs()
        u = torch.rand(x.shape, generator=g)
        x[u < 0.25] = 0.0
        x[(u >= 0.25) & (u < 0.5)] = -0.0
        return x
    return x


@pytest.mark.parametrize("kind", ["negative", "mixed", "zeros"])
def test_maxpool_ranges(lib, kind):
    hip = _harness.hip()
    N, H, W, C = 3, 9, 11, 64
    x = pool_inputs(kind)
    if kind == "negative":
        assert float(x.max()) < 0
    elif kind == "zeros":
        assert int((x == 0).sum()) > 0.4 * x.numel() and bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())
    else:
        assert float(x.min()) < 0 < float(x.max())
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = dev16(x)
    out = torch.full((N, OH, OW, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    idx = torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_maxpool3x3s2_fwd(hip.ptr(xd), hip.ptr(out), hip.ptr(idx), N, H, W, C, s) == 0
    sync()
    ref, ridx = R.maxpool3x3s2_fwd(x)                      # ridx [N, C, OH, OW]: ih * W + iw
    assert torch.equal(out.float().cpu(), ref)
    k = idx.cpu().long()                                   # window position r * 3 + s
    oh, ow = torch.arange(OH).view(1, OH, 1, 1), torch.arange(OW).view(1, 1, OW, 1)
    flat = (2 * oh - 1 + k // 3) * W + (2 * ow - 1 + k % 3)
    assert torch.equal(flat, ridx.permute(0, 2, 3, 1))
    dout = NR.rnd_bf16(N, OH, OW, C, seed=373)
    dx = torch.full_like(xd, float("nan"))
    doutd = dev16(dout)
    assert lib.icamd_maxpool3x3s2_bwd(hip.ptr(doutd), hip.ptr(idx), hip.ptr(dx), N, H, W, C, s) == 0
    sync()
    rdx = R.maxpool3x3s2_bwd(dout, x, acc=F64)
    got = dx.float().cpu()
    assert R.max_bf16_ulp(got, rdx) <= 1.0 and R.rel_l2(got, rdx) <= 1e-3


def test_bn_relu_maxpool_fused_is_bit_identical_with_negative_scales(lib):
    hip = _harness.hip()
    N, H, W, C = 3, 9, 11, 64
    g = torch.Generator().manual_seed(374)
    y = dev16(NR.rnd_bf16(N, H, W, C, seed=375))
    scale = torch.rand(C, generator=g) + 0.5
    scale[1::3] *= -1.0
    shift = torch.randn(C, generator=g) * 0.3
    shift[5] = -9.0                                        # a channel ReLU empties: every window ties at zero
    assert int((scale < 0).sum()) >= C // 4
    scale, shift = scale.to(DEV), shift.to(DEV)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    act = torch.empty_like(y)
    p1 = torch.empty(N, OH, OW, C, dtype=torch.bfloat16, device=DEV)
    p2 = torch.empty_like(p1)
    i1 = torch.zeros(N, OH, OW, C, dtype=torch.uint8, device=DEV)
    i2 = torch.ones_like(i1)
    s = hip.stream_ptr()
    assert lib.icamd_bn_apply(hip.ptr(y), hip.ptr(scale), hip.ptr(shift), None, hip.ptr(act), None, y.numel(), C, 1, s) == 0
    assert lib.icamd_maxpool3x3s2_fwd(hip.ptr(act), hip.ptr(p1), hip.ptr(i1), N, H, W, C, s) == 0
    assert lib.icamd_bn_relu_maxpool3x3s2_fwd(hip.ptr(y), hip.ptr(scale), hip.ptr(shift), hip.ptr(p2), hip.ptr(i2), N, H, W, C, s) == 0
    sync()
    assert float(act[..., 5].float().abs().max()) == 0.0
    assert torch.equal(p1.view(torch.int16), p2.view(torch.int16)) and torch.equal(i1, i2)


# ======================================================================================================== step kernels
def run_grad_norm(lib, g, inv_scale, max_norm):
    hip = _harness.hip()
    ws = torch.empty(lib.icamd_grad_norm_workspace_bytes(), dtype=torch.uint8, device=DEV)
    out = torch.full((2,), float("nan"), device=DEV)
    gd = g.to(DEV)
    assert lib.icamd_grad_norm(hip.ptr(gd), g.numel(), inv_scale, max_norm, hip.ptr(ws), hip.ptr(out), hip.stream_ptr()) == 0
    sync()
    return out


@pytest.mark.parametrize("which", ["1e15_randn", "one_1e8_among_1e-4", "inv_scale_2^-10"])
def test_grad_norm_ranges(lib, which):
    n = NR.STEP_N + 3                                       # the scalar tail behind the last vector of four
    g = torch.randn(n, generator=torch.Generator().manual_seed(381))
    inv_scale, max_norm = 1.0, 5.0
    if which == "1e15_randn":
        g = g * 1e15
    elif which == "one_1e8_among_1e-4":
        g = torch.full((n,), 1e-4)
        g[1234] = 1e8
    else:
        inv_scale = 2.0 ** -10
    out = run_grad_norm(lib, g, inv_scale, max_norm).cpu().double()
    norm = float(torch.linalg.vector_norm(g.double())) * inv_scale
    coef = min(1.0, max_norm / (norm + 1e-6))
    assert math.isfinite(float(out[0])) and abs(float(out[0]) - norm) <= 1e-5 * norm, (float(out[0]), norm)
    assert abs(float(out[1]) - coef) <= 1e-5 * coef, (float(out[1]), coef)          # relative: the coefficient is 1e-18 in one case


def optimizer_call(lib, kind, p, g, m, v, ema, shadow, lr, wd, step, gscale, clip):
    hip = _harness.hip()
    s = hip.stream_ptr()
    n = p.numel()
    if kind == "adamw":
        return lib.icamd_adamw_ema(hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(ema), hip.ptr(shadow), n, lr, wd, 0.9, 0.999,
                                   1e-8, step, gscale, 0.9995, hip.ptr(clip), None, None, 1, s)
    return lib.icamd_optim_ema(R.OPT_KINDS[kind], hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(ema), hip.ptr(shadow), n, lr,
                               wd, 0.9, 0.999, 1e-8, step, gscale, 0.9995, hip.ptr(clip), None, None, 1, s)


def f32(v):
    """a scalar as the C ABI takes it: rounded to fp32 (1 - 0.999f is 1.3e-5 away from 1 - 0.999)"""
    return float(torch.tensor(v, dtype=torch.float32))


@pytest.mark.parametrize("lr", [1e-3, 0.0])
@pytest.mark.parametrize("binding", [True, False])
@pytest.mark.parametrize("t", NR.STEP_TS)
@pytest.mark.parametrize("kind", NR.STEP_KINDS)
def test_optimizer_chain_ranges(lib, kind, t, binding, lr):
    """icamd_grad_norm -> its out[] as the clip pointer -> one optimizer step, against R.optimizer_step_f64 on the clipped gradient
    with the scalars (lr, wd, betas, eps, gscale, EMA decay) rounded to fp32 as the C ABI takes them.

    Every output element is held to rtol x the largest term of its own update, each term with its coefficient (b1 m0 and (1 - b1) g
    for the Adam kinds' m, say) and the element itself included: rtol 2e-5 for p, 1e-5 for m, v and ema, the figures of test_adamw_ema_gradnorm / test_other_fused_optimizers.  Those tests add a fixed atol (1e-6 ..
    1e-9), which would pass anything in an element of 2^-20 or 2^-60 and is not used here; and they hold an element by its own size
    alone, which fp32 cannot meet where the terms cancel (m = 0.9 m0 + 0.1 g with m0 = -g / 9.0001 at magnitude 2^20 is a sum of
    rounding errors of 0.06): an element smaller than rtol x its largest term is held by that product instead."""
    ops = NR.step_operands()
    n, wd, gscale, decay = NR.STEP_N, f32(0.05), f32(0.5), f32(0.9995)
    b1, b2, eps, lr = f32(0.9), f32(0.999), f32(1e-8), f32(lr)
    adam = kind in ("adamw", "adam")
    p0, g0, ema0 = ops["p"], ops["g"], ops["ema"]
    m0 = torch.zeros(n) if t == 1 else ops["m"]
    v0 = torch.zeros(n) if t == 1 else ops["v"]
    norm = float(torch.linalg.vector_norm(g0.double()))
    max_norm = 1.0 if binding else 1e9
    coef = min(1.0, max_norm / (norm + 1e-6))
    assert (coef < 1e-6) if binding else (coef == 1.0)                                     # the regime
    clip = run_grad_norm(lib, g0, 1.0, max_norm)
    assert abs(float(clip[0]) - norm) <= 1e-5 * norm and abs(float(clip[1]) - coef) <= 1e-5 * coef
    p, g, m, ema = p0.clone().to(DEV), g0.clone().to(DEV), m0.clone().to(DEV), ema0.clone().to(DEV)
    v = v0.clone().to(DEV) if adam else None
    shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    assert optimizer_call(lib, kind, p, g, m, v, ema, shadow, lr, wd, t, gscale, clip) == 0
    sync()
    gp, gm, gema = p.cpu().double(), m.cpu().double(), ema.cpu().double()
    finite(p=gp, m=gm, ema=gema)
    assert float(g.abs().max()) == 0.0                                                     # zero_grad fused
    geff = g0.double() * (gscale * coef)
    rp, rm, rv = R.optimizer_step_f64(kind, p0, geff, m0, v0 if adam else None, lr, wd, t, betas=(b1, b2), eps=eps)
    rema = R.ema_step_f64(ema0, rp, decay)
    # the terms of the updates.  The L2 kinds see g + wd p, which cancels where the two are alike (clipped gradients of 1e-8 next to
    # 0.05 x 2^-20): gbig is the larger of the two summands, not their sum
    gbig = torch.maximum(geff.abs(), (wd * p0.double()).abs()) if kind in ("adam", "momentum", "nesterov") else geff.abs()
    if adam:
        denom = rv.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
        step_terms = [lr / (1.0 - b1 ** t) * b1 * m0.double() / denom, lr / (1.0 - b1 ** t) * (1.0 - b1) * gbig / denom]
    elif kind == "lion":
        step_terms = [torch.full((n,), lr, dtype=F64)]
    else:
        step_terms = [lr * b1 * m0.double(), lr * gbig]
    ok = (gp - rp).abs() <= NR.largest_term_bound(NR.P_RTOL, p0, rp, *step_terms)
    if kind == "lion":
        # sign(b1 m + (1 - b1) g) is anybody's where the two cancel to within fp32 rounding of their sizes; nowhere else
        mix, size = b1 * m0.double() + (1.0 - b1) * geff, b1 * m0.double().abs() + (1.0 - b1) * geff.abs()
        unsure = (mix.abs() <= 2.0 ** -20 * size) & (size > 0)
        assert int(unsure.sum()) <= 2
        ok = ok | unsure
        zero = ops["zero"]
        assert bool((geff[zero] == 0).all()) and bool((m0[zero] == 0).all())
        moved = gp[zero] - p0[zero].double() * (1.0 - lr * wd)
        assert bool((moved.abs() <= 2.0 ** -22 * p0[zero].double().abs()).all()), "sign(0) moved a parameter"   # lr = 1e-3 >> |p| = 2^-20
    assert bool(ok.all()), (int((~ok).sum()), torch.nonzero(~ok).flatten()[:8].tolist())
    if lr == 0.0:
        assert torch.equal(p.cpu(), p0)                                                    # nothing moves, bit for bit
    # m = b1 m0 + (1 - b1) g for the Adam kinds, b2 and 1 - b2 for Lion (its momentum's own beta), b1 m0 + g for SGD
    bm = b2 if kind == "lion" else b1
    m_terms = (b1 * m0.double(), gbig) if kind in ("momentum", "nesterov") else (bm * m0.double(), (1.0 - bm) * gbig)
    e = (gm - rm).abs() / (NR.largest_term_bound(1e-5, rm, *m_terms) + 1e-45)
    assert float(e.max()) <= 1.0, ("m", float(e.max()), int(e.argmax()))
    if adam:
        gv = v.cpu().double()
        finite(v=gv)
        # (a square below 2^-126 flushes to zero in fp32: hence that term)
        e = (gv - rv).abs() / (NR.largest_term_bound(1e-5, b2 * v0.double(), (1.0 - b2) * gbig * gbig, rv) + 2.0 ** -126)
        assert float(e.max()) <= 1.0, ("v", float(e.max()), int(e.argmax()))
    e = (gema - rema).abs() / (NR.largest_term_bound(1e-5, decay * ema0.double(), (1.0 - decay) * rp, rema) + 1e-45)
    assert float(e.max()) <= 1.0, ("ema", float(e.max()), int(e.argmax()))
    assert torch.equal(shadow.float().cpu(), R.bf16_round(p.cpu()))
