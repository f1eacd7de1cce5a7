"""icamd_grn_fwd / icamd_grn_bwd at C = 160 (C % 64 == 32: ConvNeXt V2 atto's first stage, 4 dim = 160) against the fp64 closed form of
oracle/convnext_ref.py, with the bounds of tests/test_grn_gpu.py::test_grn_matches_fp64_closed_form: bf16 outputs rel-L2 <= 1e-3;
fp32 statistics at most 10 x the error of a plain fp32 torch evaluation of the same closed form, floor 1e-6; two launches bit-equal.

At C = 160 a row has 20 vectors of 8 channels: a reduction workgroup is 20 vector columns x 12 row lanes with 16 idle threads, and
the parameter-gradient launch has ceil(160 / 64) = 3 workgroups, the last with 32 live channels.  (3, 200, 160) gives the
reductions 7 row segments per sample and every row lane more than one row; (2, 49, 160) has two segments, of 25 and 24 rows."""
import pytest
import torch

from _convnext_narrow import Grn
from oracle.convnext_ref import gelu_grad, grn_closed_form

pytestmark = pytest.mark.gpu


def rel_l2(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-300))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("shape", [(2, 49, 160), (3, 200, 160)])
def test_grn_160_matches_fp64_closed_form(shape):
    N, HW, C = shape
    k = Grn(N, HW, C)
    assert k.lib.icamd_grn_supported(N, HW, C) == 1 and k.bytes > 0
    gen = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(N, HW, C, device="cuda", generator=gen).to(torch.bfloat16)
    a = torch.nn.functional.gelu(z.float()).to(torch.bfloat16)
    dg = torch.randn(N, HW, C, device="cuda", generator=gen).to(torch.bfloat16)
    gamma = 0.5 * torch.randn(C, device="cuda", generator=gen)
    beta = 0.1 * torch.randn(C, device="cuda", generator=gen)
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
    print(f"grn {shape}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()) + "; "
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
        assert torch.equal(_bits(x), _bits(y))
    # accumulate adds onto prior contents, and nothing is written behind channel 159 (the last workgroup's dead half)
    prior = torch.randn(2, C + 64, device="cuda")
    acc = prior.clone()
    rc, _, _, _ = k.bwd(dg, a, gx, gamma, dgamma=acc[0], dbeta=acc[1], accumulate=1)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(acc[:, :C], prior[:, :C] + torch.stack([dgam, dbet])) and torch.equal(acc[:, C:], prior[:, C:])


def test_unsupported_widths_stay_unsupported():
    from imageclassification_amd import hip
    lib = hip.load()
    for C in (96, 64, 200, 6208):
        assert lib.icamd_grn_supported(2, 49, C) == 0 and lib.icamd_grn_workspace_bytes(2, 49, C) == 0
    for C in (128, 160, 192, 6144):
        assert lib.icamd_grn_supported(2, 49, C) == 1
