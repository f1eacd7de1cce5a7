"""The BatchNorm + SiLU and MBConv squeeze-and-excitation entries of csrc/dwconv5x5.hip, each against the fp64 reference of
oracle/ops_ref.py on the same operands (every entry takes the REFERENCE's arrays as inputs, so no error is carried from one
entry into the next).

  icamd_bn_apply_silu       equal to bf16(silu64(fma32(y, scale, shift))) but for at most 1e-3 of the elements, those one bf16 step off
                            (the kernel's silu is fp32: expf and an IEEE division, a few ulps; the share of elements that close to a
                            rounding boundary is printed); gated: the same rule on bf16(fp32(a * e))
  bf16 outputs              rel_l2 <= 1e-3 and bf16_close;   [N, C] fp32 arrays and parameter gradients: rel_l2 <= 1e-4
  icamd_bn_bwd_silu         dy rel_l2 <= 1e-3 and bf16_close, dgamma / dbeta rel_l2 <= 1e-4 (tests/test_bn_relu6_gpu.py's)

Loops whose trip count depends on the problem: row segments per sample S (1 at HW <= 32, 7 at 196, 98 at 3136), rows of a segment per
row lane (r += rlanes: (2, 3136, 96) 32 rows over 21 lanes = 2 trips), LDS outputs (o += 256 over 8 tcols: C = 1152 5 trips), the
channel-group loop (cg0 += 256: two trips at C = 2056, the second with one column and 256 row lanes), waves over rd (rd = 6, 10, 48, 80 > 4),
c += 256 (C >= 1152), samples per wave in the parameter-gradient kernel (N = 5 > 4) and its chunks of 1024 samples (N = 1100: two)."""
import pytest
import torch

import _harness
from _harness import DEV, dev, digest, guarded, intact, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

# the issue's seven, then the two that drive what those do not: C > 2048 (a second trip of the channel-group loop) and N > 1024 (a second
# chunk of samples in the parameter-gradient kernel)
SHAPES = [(3, 1, 16, 4), (2, 49, 144, 6), (5, 196, 240, 10), (2, 3136, 96, 4), (4, 9, 1152, 48), (2, 4, 1920, 80), (2, 2, 8, 1),
          (2, 5, 2056, 8), (1100, 1, 8, 2)]
EPS = 1e-5


def f32(t):
    return t.float().to(DEV).contiguous()


def operands(N, HW, C, rd, seed=0):
    g = torch.Generator().manual_seed(500 + C + seed)
    y = R.bf16_round(torch.randn(N, HW, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g))
    dout = R.bf16_round(torch.randn(N, HW, C, generator=g))
    gamma = 1.0 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    yd = y.double()
    mean = yd.mean((0, 1))
    invstd = 1.0 / torch.sqrt(yd.var((0, 1), unbiased=False) + EPS)
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * scale.double()).float()
    w1 = torch.randn(rd, C, generator=g) * (2.0 / C) ** 0.5 * 2
    b1 = torch.randn(rd, generator=g) * 0.5
    w2 = torch.randn(C, rd, generator=g) * (2.0 / rd) ** 0.5
    b2 = torch.randn(C, generator=g) * 0.5
    return {"y": y, "dout": dout, "mean": mean.float(), "invstd": invstd.float(), "scale": scale, "shift": shift, "w1": w1, "b1": b1,
            "w2": w2, "b2": b2}


def one_step_off(got, ref, what):
    """equal but for at most 1e-3 of the elements, and those within one bf16 step"""
    diff = got != ref
    share = float(diff.float().mean())
    print(f"{what}: {share:.2e} of the elements differ from the reference's rounding")
    assert share <= 1e-3
    assert R.max_bf16_ulp(got, ref) <= 1.0 if bool(diff.any()) else True
    assert R.rel_l2(got, ref) <= 1e-3 and R.bf16_close(got, ref)


def run_apply(lib, o, N, HW, C, e=None):
    hip = _harness.hip()
    out, go = guarded((N, HW, C), torch.bfloat16)
    rc = lib.icamd_bn_apply_silu(hip.ptr(o["yd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]), hip.ptr(e), hip.ptr(out), N, HW, C,
                                 hip.stream_ptr())
    assert rc == 0 and intact(go)
    return out


def run_rowsum(lib, o, N, HW, C, with_dout):
    hip = _harness.hip()
    q = lib.icamd_se_silu_bwd_reduce_workspace_bytes if with_dout else lib.icamd_bn_silu_squeeze_workspace_bytes
    wsb = q(N, HW, C)
    assert wsb > 0
    ws, gws = guarded((wsb,), torch.uint8, fill=0x7F)
    out, go = guarded((N, C), torch.float32)
    if with_dout:
        rc = lib.icamd_se_silu_bwd_reduce(hip.ptr(o["dd"]), hip.ptr(o["yd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]), hip.ptr(out), N, HW, C,
                                          hip.ptr(ws), wsb, hip.stream_ptr())
    else:
        rc = lib.icamd_bn_silu_squeeze(hip.ptr(o["yd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]), hip.ptr(out), N, HW, C, hip.ptr(ws), wsb,
                                       hip.stream_ptr())
    assert rc == 0 and intact(go) and intact(gws)
    return out


def run_excite_fwd(lib, asum, o, N, HW, C, rd):
    hip = _harness.hip()
    (s, gs), (h, gh), (e, ge) = guarded((N, C), torch.float32), guarded((N, rd), torch.float32), guarded((N, C), torch.float32)
    rc = lib.icamd_se_excite_silu_fwd(hip.ptr(asum), 1.0 / HW, hip.ptr(o["w1d"]), hip.ptr(o["b1d"]), hip.ptr(o["w2d"]), hip.ptr(o["b2d"]),
                                      hip.ptr(s), hip.ptr(h), hip.ptr(e), N, C, rd, hip.stream_ptr())
    assert rc == 0 and intact(gs) and intact(gh) and intact(ge)
    return s, h, e


def run_excite_bwd(lib, de, s, h, e, o, N, HW, C, rd, base=None):
    hip = _harness.hip()
    fill = float("nan") if base is None else base
    outs = [guarded(shape, torch.float32, fill=fill) for shape in ((rd, C), (rd,), (C, rd), (C,))]
    dsn, gd = guarded((N, C), torch.float32)
    rc = lib.icamd_se_excite_silu_bwd(hip.ptr(de), hip.ptr(s), hip.ptr(h), hip.ptr(e), hip.ptr(o["w1d"]), hip.ptr(o["w2d"]),
                                      *(hip.ptr(t) for t, _ in outs), hip.ptr(dsn), N, C, rd, 1.0 / HW, int(base is not None),
                                      hip.stream_ptr())
    assert rc == 0 and intact(gd) and all(intact(g) for _, g in outs)
    return [t for t, _ in outs] + [dsn]


def run_bn_bwd(lib, o, N, HW, C, e=None, dsn=None, acc=0, base=0.0, ws=None):
    hip = _harness.hip()
    wsb = lib.icamd_bn_bwd_silu_workspace_bytes(N, HW, C)
    assert wsb == lib.icamd_bn_bwd_workspace_bytes(N * HW, C) > 0
    if ws is None:
        ws = guarded((wsb,), torch.uint8, fill=0)           # arrival counters start at zero
    dy, gdy = guarded((N, HW, C), torch.bfloat16)
    dg, gdg = guarded((C,), torch.float32, fill=base if acc else float("nan"))
    db, gdb = guarded((C,), torch.float32, fill=base if acc else float("nan"))
    rc = lib.icamd_bn_bwd_silu(hip.ptr(o["dd"]), hip.ptr(o["yd"]), hip.ptr(o["md"]), hip.ptr(o["isd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]),
                               hip.ptr(e), hip.ptr(dsn), hip.ptr(dg), hip.ptr(db), hip.ptr(dy), N, HW, C, acc, hip.ptr(ws[0]), wsb,
                               hip.stream_ptr())
    assert rc == 0 and intact(gdy) and intact(gdg) and intact(gdb) and intact(ws[1])
    return dy, dg, db, ws


def to_device(o):
    o.update(yd=dev(o["y"]), dd=dev(o["dout"]), md=f32(o["mean"]), isd=f32(o["invstd"]), scd=f32(o["scale"]), shd=f32(o["shift"]),
             w1d=f32(o["w1"]), b1d=f32(o["b1"]), w2d=f32(o["w2"]), b2d=f32(o["b2"]))
    return o


def check_all(lib, o, N, HW, C, rd, tag):
    """every entry of the section on the operands `o`, each fed the reference's arrays"""
    y, dout, scale, shift = o["y"], o["dout"], o["scale"], o["shift"]
    a = R.bn_silu(y, scale, shift)
    print(f"{tag}: {R.boundary_share(y, scale, shift):.2e} of the elements within 8 fp32 ulps of a bf16 rounding boundary")
    assert bool(torch.isfinite(a).all())
    # forward: ungated apply, squeeze, excite, gated apply
    got_a = run_apply(lib, o, N, HW, C)
    one_step_off(got_a.float().cpu(), a, tag + " a")
    asum = a.double().sum(1)
    got_asum = run_rowsum(lib, o, N, HW, C, False)
    print(f"{tag}: asum rel_l2 {R.rel_l2(got_asum.cpu(), asum):.2e}")
    assert R.rel_l2(got_asum.cpu(), asum) <= 1e-4
    s, hpre, e = R.excite_fwd(asum, 1.0 / HW, o["w1"], o["b1"], o["w2"], o["b2"])
    gs, gh, ge = run_excite_fwd(lib, f32(asum), o, N, HW, C, rd)
    for name, g, r in (("s", gs, s), ("hpre", gh, hpre), ("e", ge, e)):
        print(f"{tag}: {name} rel_l2 {R.rel_l2(g.cpu(), r):.2e}")
        assert R.rel_l2(g.cpu(), r) <= 1e-4, name
    e32 = e.float()
    gated = R.bf16_round((a.double() * e32.double()[:, None, :]).float())
    got_gated = run_apply(lib, o, N, HW, C, f32(e32))
    one_step_off(got_gated.float().cpu(), gated, tag + " gated")
    # backward: gate gradient, excite backward, BatchNorm backward (gated and plain)
    de = (dout.double() * a.double()).sum(1)
    got_de = run_rowsum(lib, o, N, HW, C, True)
    print(f"{tag}: de rel_l2 {R.rel_l2(got_de.cpu(), de):.2e}")
    assert R.rel_l2(got_de.cpu(), de) <= 1e-4
    s32, h32, de32 = s.float(), hpre.float(), de.float()
    refs = R.excite_bwd(de32, s32, h32, e32, o["w1"], o["w2"], 1.0 / HW)
    for base in (None, 1.0):
        got = run_excite_bwd(lib, f32(de32), f32(s32), f32(h32), f32(e32), o, N, HW, C, rd, base)
        for name, g, r in zip(("dw1", "db1", "dw2", "db2", "dsn"), got, refs):
            want = r if base is None or name == "dsn" else r + base
            print(f"{tag} base={base}: {name} rel_l2 {R.rel_l2(g.cpu(), want):.2e}")
            assert R.rel_l2(g.cpu(), want) <= 1e-4, name
    dsn32 = refs[4].float()
    for gate in (None, (e32, dsn32)):
        ge_, gd_ = (None, None) if gate is None else (f32(gate[0]), f32(gate[1]))
        rdy, rdg, rdb = R.bn_bwd_silu(dout, y, o["mean"], o["invstd"], scale, shift, *(gate or ()))
        rdy = R.bf16_round(rdy.float())
        ws = None
        for acc, base in ((0, 0.0), (1, 1.5)):
            dy, dg, db, ws = run_bn_bwd(lib, o, N, HW, C, ge_, gd_, acc, base, ws)
            got = dy.float().cpu()
            print(f"{tag} gated={gate is not None} acc={acc}: dy rel_l2 {R.rel_l2(got, rdy):.2e}, dgamma "
                  f"{R.rel_l2(dg.cpu(), base + rdg):.2e}, dbeta {R.rel_l2(db.cpu(), base + rdb):.2e}")
            assert bool(torch.isfinite(got).all())
            assert R.rel_l2(got, rdy) <= 1e-3 and R.bf16_close(got, rdy)
            assert R.rel_l2(dg.cpu(), base + rdg) <= 1e-4 and R.rel_l2(db.cpu(), base + rdb) <= 1e-4
    return {"e": e32, "dsn": dsn32, "de": de32, "s": s32, "hpre": h32, "asum": asum.float()}


@pytest.mark.parametrize("N,HW,C,rd", SHAPES)
def test_every_entry_against_fp64(lib, N, HW, C, rd):
    o = to_device(operands(N, HW, C, rd))
    check_all(lib, o, N, HW, C, rd, f"({N}, {HW}, {C}, {rd})")


def test_extreme_pre_activations_stay_finite_and_within_the_bounds(lib):
    """z = 0, +-20, +-100 (constant channels), a constant channel, channels scaled by 2^20 and 2^-20: forward and backward finite and
    within the bounds of the other shapes"""
    N, HW, C, rd = 4, 33, 16, 4
    o = operands(N, HW, C, rd, seed=9)
    y, scale, shift = o["y"], o["scale"], o["shift"]
    for c, z in enumerate((0.0, 20.0, -20.0, 100.0, -100.0)):
        y[..., c], scale[c], shift[c] = 0.0, 1.0, z
    y[..., 5] = 1.5                                               # a constant channel with ordinary coefficients
    g = torch.Generator().manual_seed(11)
    y[..., 6] = R.bf16_round(2 * torch.rand(N, HW, generator=g) - 1)
    scale[6], shift[6] = 2.0 ** 20, 0.0                           # |z| up to 2^20
    scale[7], shift[7] = 2.0 ** -20, 0.0
    # the squeeze of those channels is as extreme as they are (s up to 2^19); the reduce filter takes them at a weight that leaves
    # the gates off saturation, so that the excitation backward is held on numbers, not on zeros
    o["w1"][:, 6] *= 2.0 ** -20
    o["w1"][:, 3] *= 0.01
    yd = y.double()
    o["mean"] = yd.mean((0, 1)).float()
    o["invstd"] = (1.0 / torch.sqrt(yd.var((0, 1), unbiased=False) + EPS)).float()
    z = R.fma32(y, scale, shift)
    assert float(z.abs().max()) >= 2.0 ** 19 and float(z[..., 3].min()) == 100.0 and float(z[..., 4].max()) == -100.0
    check_all(lib, to_device(o), N, HW, C, rd, "extremes")
    # NaN stays NaN
    hip = _harness.hip()
    o["yd"][0, 0, 8] = float("nan")
    out = run_apply(lib, o, N, HW, C)
    assert bool(torch.isnan(out[0, 0, 8])) and int(torch.isnan(out.float()).sum()) == 1
    del hip


def test_second_launch_gives_the_same_bits(lib):
    N, HW, C, rd = 5, 196, 240, 10
    o = to_device(operands(N, HW, C, rd))
    g = torch.Generator().manual_seed(3)
    e, dsn = f32(torch.rand(N, C, generator=g)), f32(torch.randn(N, C, generator=g) * 0.01)
    de, s, h = f32(torch.randn(N, C, generator=g)), f32(torch.randn(N, C, generator=g)), f32(torch.randn(N, rd, generator=g))
    seen = []
    for _ in range(2):
        outs = [run_apply(lib, o, N, HW, C), run_apply(lib, o, N, HW, C, e), run_rowsum(lib, o, N, HW, C, False),
                run_rowsum(lib, o, N, HW, C, True)]
        outs += list(run_excite_fwd(lib, de, o, N, HW, C, rd)) + run_excite_bwd(lib, de, s, h, e, o, N, HW, C, rd)
        outs += list(run_bn_bwd(lib, o, N, HW, C, e, dsn)[:3]) + list(run_bn_bwd(lib, o, N, HW, C)[:3])
        sync()
        seen.append(digest(*outs))
    assert seen[0] == seen[1]


@pytest.mark.parametrize("N,HW,C,rd", [(2, 9, 20, 4), (2, 9, 4104, 4), (2, 9, 16, 257)])
def test_refusals_write_nothing(lib, N, HW, C, rd):
    hip = _harness.hip()
    s_ = hip.stream_ptr()
    if rd <= 256:
        assert lib.icamd_bn_silu_squeeze_workspace_bytes(N, HW, C) == 0 and lib.icamd_se_silu_bwd_reduce_workspace_bytes(N, HW, C) == 0
        assert lib.icamd_bn_bwd_silu_workspace_bytes(N, HW, C) == 0
    sent = 12288.0
    big = torch.zeros(N * HW * C + 8, dtype=torch.bfloat16, device=DEV)
    vec = torch.ones((rd + N) * C + N * rd + 8, device=DEV)
    outb = torch.full((N * HW * C + 8,), sent, dtype=torch.bfloat16, device=DEV)
    outs = [torch.full(((rd + N) * C + N * rd + 8,), sent, device=DEV) for _ in range(5)]
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    p, v, w = hip.ptr(big), hip.ptr(vec), hip.ptr(ws)
    o = [hip.ptr(t) for t in outs]
    if rd <= 256:
        assert lib.icamd_bn_apply_silu(p, v, v, None, hip.ptr(outb), N, HW, C, s_) != 0
        assert lib.icamd_bn_apply_silu(p, v, v, v, hip.ptr(outb), N, HW, C, s_) != 0
        assert lib.icamd_bn_silu_squeeze(p, v, v, o[0], N, HW, C, w, 1 << 20, s_) != 0
        assert lib.icamd_se_silu_bwd_reduce(p, p, v, v, o[0], N, HW, C, w, 1 << 20, s_) != 0
        assert lib.icamd_bn_bwd_silu(p, p, v, v, v, v, None, None, o[0], o[1], hip.ptr(outb), N, HW, C, 0, w, 1 << 20, s_) != 0
    assert lib.icamd_se_excite_silu_fwd(v, 1.0, v, v, v, v, o[0], o[1], o[2], N, C, rd, s_) != 0
    assert lib.icamd_se_excite_silu_bwd(v, v, v, v, v, v, o[0], o[1], o[2], o[3], o[4], N, C, rd, 1.0, 0, s_) != 0
    sync()
    assert bool((outb.float() == sent).all()) and all(bool((t == sent).all()) for t in outs) and bool((ws == 7).all())


def test_short_workspaces_and_half_given_gate_are_refused(lib):
    hip = _harness.hip()
    N, HW, C = 2, 49, 144
    o = to_device(operands(N, HW, C, 6))
    s_ = hip.stream_ptr()
    out = torch.full((N, C), 5.0, device=DEV)
    dy = torch.full((N, HW, C), 5.0, dtype=torch.bfloat16, device=DEV)
    wsb = lib.icamd_bn_silu_squeeze_workspace_bytes(N, HW, C)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_silu_squeeze(hip.ptr(o["yd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]), hip.ptr(out), N, HW, C, hip.ptr(ws), wsb - 1,
                                     s_) == 3
    assert lib.icamd_se_silu_bwd_reduce(hip.ptr(o["dd"]), hip.ptr(o["yd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]), hip.ptr(out), N, HW, C,
                                        hip.ptr(ws), wsb - 1, s_) == 3
    bwb = lib.icamd_bn_bwd_silu_workspace_bytes(N, HW, C)
    args = (hip.ptr(o["dd"]), hip.ptr(o["yd"]), hip.ptr(o["md"]), hip.ptr(o["isd"]), hip.ptr(o["scd"]), hip.ptr(o["shd"]))
    assert lib.icamd_bn_bwd_silu(*args, None, None, hip.ptr(out), hip.ptr(out), hip.ptr(dy), N, HW, C, 0, hip.ptr(ws), bwb - 1, s_) == 3
    assert lib.icamd_bn_bwd_silu(*args, hip.ptr(out), None, hip.ptr(out), hip.ptr(out), hip.ptr(dy), N, HW, C, 0, hip.ptr(ws), bwb, s_) == 1
    sync()
    assert bool((out == 5.0).all()) and bool((dy.float() == 5.0).all()) and bool((ws == 7).all())
