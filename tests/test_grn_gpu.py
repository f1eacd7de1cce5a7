"""icamd_grn_fwd / icamd_grn_bwd (csrc/grn.hip) against the fp64 closed form of oracle/convnext_ref.py, evaluated on the bf16
inputs and rounded to bf16 once, where the kernels round.

Bounds: g, da and dz1 rel-L2 <= 1e-3 (the project's kernel bound; an fp32 and an fp64 evaluation, both rounded, differ by <= 4e-5).
gx, dgamma, dbeta (fp32): at most 10 x the rel-L2 error of a plain fp32 torch evaluation of the same closed form against fp64 on
the same inputs, floor 1e-6 -- the margin is for summation order; a lost row segment or sample is O(1 / segments)."""
import pytest
import torch

from _convnext_narrow import grn_plan
from oracle.convnext_ref import GRN_EPS, gelu_grad, grn_closed_form

pytestmark = pytest.mark.gpu

UNSUPPORTED, WORKSPACE = 2, 3

# id -> (N, HW, C, variant)
CASES = {
    "1x1x128": (1, 1, 128, None),
    "3x49x256": (3, 49, 256, None),
    "2x3136x384": (2, 3136, 384, None),
    "2x196x6144": (2, 196, 6144, None),
    "multitrip_40x784x768": (40, 784, 768, None),
    "batch_capped_512x160x128": (512, 160, 128, None),
    "zero_sample_zero_channel": (3, 49, 256, "zeros"),
    "scaled_2^-12": (2, 196, 384, 2.0 ** -12),
    "scaled_2^8": (2, 196, 384, 2.0 ** 8),
}


def rel_l2(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-300))


def _inputs(N, HW, C, variant, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(N, HW, C, device="cuda", generator=g).to(torch.bfloat16)
    a = torch.nn.functional.gelu(z.float()).to(torch.bfloat16)
    if variant == "zeros":
        a[0, :, 5] = 0
        a[-1] = 0
    elif variant is not None:
        a = (a.float() * variant).to(torch.bfloat16)        # a power of two: exact
    dg = torch.randn(N, HW, C, device="cuda", generator=g).to(torch.bfloat16)
    gamma = 0.5 * torch.randn(C, device="cuda", generator=g)
    beta = 0.1 * torch.randn(C, device="cuda", generator=g)
    return z, a, dg, gamma, beta


class Grn:
    """The two entries on tensors."""

    def __init__(self, N, HW, C):
        from imageclassification_amd import hip
        self.hip, self.lib = hip, hip.load()
        self.N, self.HW, self.C = N, HW, C
        self.bytes = self.lib.icamd_grn_workspace_bytes(N, HW, C)
        self.ws = torch.empty(max(self.bytes, 256), dtype=torch.uint8, device="cuda")

    def fwd(self, a, gamma, beta, g=None, gx=None, ws_bytes=None):
        g = torch.empty_like(a) if g is None else g
        gx = torch.empty(self.N, self.C, device="cuda") if gx is None else gx
        rc = self.lib.icamd_grn_fwd(a.data_ptr(), gamma.data_ptr(), beta.data_ptr(), g.data_ptr(), gx.data_ptr(), self.N, self.HW,
                                    self.C, GRN_EPS, self.ws.data_ptr(), self.bytes if ws_bytes is None else ws_bytes,
                                    self.hip.stream_ptr())
        return rc, g, gx

    def bwd(self, dg, a, gx, gamma, z=None, dx=None, dgamma=None, dbeta=None, accumulate=0, ws_bytes=None):
        dx = torch.empty_like(a) if dx is None else dx
        dgamma = torch.empty(self.C, device="cuda") if dgamma is None else dgamma
        dbeta = torch.empty(self.C, device="cuda") if dbeta is None else dbeta
        rc = self.lib.icamd_grn_bwd(dg.data_ptr(), a.data_ptr(), gx.data_ptr(), gamma.data_ptr(), None if z is None else z.data_ptr(),
                                    dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), accumulate, self.N, self.HW, self.C, GRN_EPS,
                                    self.ws.data_ptr(), self.bytes if ws_bytes is None else ws_bytes, self.hip.stream_ptr())
        return rc, dx, dgamma, dbeta


@pytest.mark.parametrize("case", list(CASES))
def test_grn_matches_fp64_closed_form(case):
    """Forward, backward without and with the fused GELU backward, two launches bit for bit, accumulate.

    multitrip_40x784x768 is derived from the launch geometry (grn_plan mirrors icamd_grn_plan): 25 row segments of 32 rows and 72
    row blocks of 11 rows per sample, 96 vector columns with 2 row lanes.  It drives every problem-sized loop of csrc/grn.hip more
    than once but one: the row loop of the reductions 16 times, their LDS output loop 3 (6) times over 2 row lanes, the prologue's
    fold over 25 partial rows, the vector loop of the apply passes 5 times, the sample loop of the parameter-gradient launch 10
    times.  The prologue's channel loops take four channels per thread and trip, so they repeat only above 1024 channels, where a
    reduction workgroup has one row lane: 2x196x6144 runs them 6 times, over 3 column tiles per row.  (tests/test_convnextv2_cpu.py
    asserts these counts.)  batch_capped_512x160x128 is the shape at which the batch, not the image, caps the segments (4 of 40
    rows) and the row blocks (3)."""
    N, HW, C, variant = CASES[case]
    assert Grn(N, HW, C).lib.icamd_grn_supported(N, HW, C) == 1
    z, a, dg, gamma, beta = _inputs(N, HW, C, variant)
    k = Grn(N, HW, C)
    ref = grn_closed_form(a.double(), gamma.double(), beta.double(), dg.double())
    r32 = grn_closed_form(a.float(), gamma, beta, dg.float())
    rc, g, gx = k.fwd(a, gamma, beta)
    assert rc == 0
    rc, da, dgam, dbet = k.bwd(dg, a, gx, gamma)
    assert rc == 0
    rc, dz, dgam_z, dbet_z = k.bwd(dg, a, gx, gamma, z=z)
    assert rc == 0
    torch.cuda.synchronize()
    for t in (g, gx, da, dz, dgam, dbet):
        assert bool(torch.isfinite(t.float()).all())
    want = {"g": ref["g"].to(torch.bfloat16), "da": ref["da"].to(torch.bfloat16),
            "dz1": (ref["da"] * gelu_grad(z.double())).to(torch.bfloat16)}
    errs = {"g": rel_l2(g, want["g"]), "da": rel_l2(da, want["da"]), "dz1": rel_l2(dz, want["dz1"])}
    stats = {}
    for name, got, key in (("gx", gx, "gx"), ("dgamma", dgam, "dweight"), ("dbeta", dbet, "dbias")):
        stats[name] = (rel_l2(got, ref[key]), rel_l2(r32[key], ref[key]))
    print(f"grn {case}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()) + "; "
          + ", ".join(f"{n} {e:.2e} (fp32 torch {t:.2e})" for n, (e, t) in stats.items()))
    for n, e in errs.items():
        assert e <= 1e-3, (n, e)
    for n, (e, t) in stats.items():
        assert e <= max(10.0 * t, 1e-6), (n, e, t)
    assert torch.equal(dgam, dgam_z) and torch.equal(dbet, dbet_z)
    # two launches: identical bits for every output
    _, g2, gx2 = k.fwd(a, gamma, beta)
    _, dz2, dgam2, dbet2 = k.bwd(dg, a, gx2, gamma, z=z)
    _, da2, _, _ = k.bwd(dg, a, gx2, gamma)
    torch.cuda.synchronize()
    for x, y in ((g, g2), (gx, gx2), (dz, dz2), (da, da2), (dgam, dgam2), (dbet, dbet2)):
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32),
                           y.view(torch.int16) if y.dtype == torch.bfloat16 else y.view(torch.int32))
    # accumulate adds onto prior contents
    prior_g, prior_b = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    acc_g, acc_b = prior_g.clone(), prior_b.clone()
    rc, _, _, _ = k.bwd(dg, a, gx, gamma, dgamma=acc_g, dbeta=acc_b, accumulate=1)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(acc_g, prior_g + dgam) and torch.equal(acc_b, prior_b + dbet)


@pytest.mark.parametrize("shape", [(2, 49, 96), (2, 49, 64), (2, 49, 6208), (2, 49, 200)])
def test_grn_unsupported_shape_writes_nothing(shape):
    N, HW, C = shape
    k = Grn(N, HW, C)
    assert k.lib.icamd_grn_supported(N, HW, C) == 0 and k.bytes == 0
    a = torch.randn(N, HW, C, device="cuda").to(torch.bfloat16)
    gamma, beta = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    sent = 12345.0
    g, dx = torch.full_like(a, sent), torch.full_like(a, sent)
    gx, dgam, dbet = torch.full((N, C), sent, device="cuda"), torch.full((C,), sent, device="cuda"), torch.full((C,), sent, device="cuda")
    k.ws.fill_(7)
    assert k.fwd(a, gamma, beta, g=g, gx=gx, ws_bytes=1 << 20)[0] == UNSUPPORTED
    assert k.bwd(a, a, torch.ones(N, C, device="cuda"), gamma, dx=dx, dgamma=dgam, dbeta=dbet, ws_bytes=1 << 20)[0] == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (g, dx, gx, dgam, dbet):
        assert bool((t.float() == t.new_tensor(sent).float()).all())
    assert bool((k.ws == 7).all())


def test_grn_workspace_one_byte_short_is_an_error():
    N, HW, C = 3, 49, 256
    k = Grn(N, HW, C)
    assert k.bytes > 0
    _, a, dg, gamma, beta = _inputs(N, HW, C, None)
    sent = 12345.0
    g, dx = torch.full_like(a, sent), torch.full_like(a, sent)
    gx, dgam, dbet = torch.full((N, C), sent, device="cuda"), torch.full((C,), sent, device="cuda"), torch.full((C,), sent, device="cuda")
    assert k.fwd(a, gamma, beta, g=g, gx=gx, ws_bytes=k.bytes - 1)[0] == WORKSPACE
    assert k.bwd(dg, a, torch.ones(N, C, device="cuda"), gamma, dx=dx, dgamma=dgam, dbeta=dbet, ws_bytes=k.bytes - 1)[0] == WORKSPACE
    torch.cuda.synchronize()
    for t in (g, dx, gx, dgam, dbet):
        assert bool((t.float() == t.new_tensor(sent).float()).all())
    assert k.fwd(a, gamma, beta, g=g, gx=gx)[0] == 0
    torch.cuda.synchronize()


def test_grn_plan_mirror_sizes_the_workspace():
    """The Python mirror of the planner agrees with the library: workspace = [N][S][2][C] + [N][2][C] floats, 256 B aligned."""
    from imageclassification_amd import hip
    lib = hip.load()
    for N, HW, C, _ in CASES.values():
        p = grn_plan(N, HW, C)
        up = lambda v: (v + 255) // 256 * 256
        assert lib.icamd_grn_workspace_bytes(N, HW, C) == up(N * p["S"] * 2 * C * 4) + up(N * 2 * C * 4)
