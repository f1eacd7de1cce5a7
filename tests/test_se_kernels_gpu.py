"""The squeeze-and-excitation kernels (csrc/se_ops.hip) through the C ABI, one entry at a time, against torch on the CPU.

Cases (N, HW, C, rd) are the smallest shapes where the kernels can go wrong: odd HW, HW = 1, one long sample (its HW split over
many workgroups), a narrow C and the widest C.  The inputs of a case and its references (fp32 autograd on the rounded inputs and
the fp64 copy of the same chain) are computed once and shared by the tests.

Bounds: bf16 outputs by the project's rule for bf16 outputs (max_bf16_ulp <= 1.0 and rel-L2 <= 1e-3; dy3: rel-L2 <= 1e-3 and
bf16_close), fp32 parameter gradients rel-L2 <= 1e-4 against fp32 autograd after that reference is shown to be within 5e-5 of its
fp64 copy, the [N, C] forward arrays <= 1e-5 and the sums <= 1e-6 against fp64."""
import functools

import pytest
import torch

from oracle import ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
CASES = [(3, 49, 256, 16), (2, 196, 512, 32), (5, 9, 2048, 128), (4, 1, 256, 16), (1, 3136, 256, 16), (3, 35, 64, 8)]
GRADS = ("dgamma", "dbeta", "dW1", "db1", "dW2", "db2")


@pytest.fixture(scope="module")
def lib():
    from imageclassification_amd import hip
    hip.require_gpu()
    return hip.load()


def _hip():
    from imageclassification_amd import hip
    return hip


def _tail(c, dt, mask=None):
    """The block tail in dtype dt on the case's (already rounded) inputs, with autograd.  mask None: the ReLU's own; given: that
    mask (so that the fp64 copy differentiates the same function as the fp32 reference)."""
    t = {k: c[k].to(dt).clone().requires_grad_() for k in ("y", "gamma", "beta", "W1", "b1", "W2", "b2")}
    y = t["y"]
    # BatchNorm in training mode: the statistics are functions of y
    m = y.mean((0, 1))
    v = ((y - m) ** 2).mean((0, 1))
    yhat = (y - m) / torch.sqrt(v + EPS)
    z = yhat * t["gamma"] + t["beta"]
    s = z.mean(1)
    h = torch.relu(s @ t["W1"].t() + t["b1"])
    e = torch.sigmoid(h @ t["W2"].t() + t["b2"])
    u = z * e[:, None, :] + c["res"].to(dt)
    if mask is None:
        mask = (u > 0).detach()
    out = u * mask
    out.backward(c["dout"].to(dt))
    r = {"z": z.detach(), "s": s.detach(), "h": h.detach(), "e": e.detach(), "u": u.detach(), "mask": mask, "dy": y.grad,
         "dgamma": t["gamma"].grad, "dbeta": t["beta"].grad, "dW1": t["W1"].grad, "db1": t["b1"].grad, "dW2": t["W2"].grad,
         "db2": t["b2"].grad}
    return r


def _inputs(N, HW, C, rd):
    """The (rounded) inputs of a case, without references"""
    g = torch.Generator().manual_seed(1000 + N * 7 + HW + C)
    c = {"shape": (N, HW, C, rd)}
    # a raw convolution output with per-channel offsets and widths and a per-sample shift (so that s differs between samples)
    y = torch.randn(N, HW, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g) \
        + 0.7 * torch.randn(N, 1, C, generator=g)
    c["y"] = R.bf16_round(y)
    c["gamma"] = torch.rand(C, generator=g) + 0.5
    c["beta"] = torch.randn(C, generator=g) * 0.3
    c["mean"] = c["y"].mean((0, 1))
    c["invstd"] = 1.0 / torch.sqrt(c["y"].var((0, 1), unbiased=False) + EPS)
    c["scale"] = c["gamma"] * c["invstd"]
    c["shift"] = c["beta"] - c["mean"] * c["scale"]
    # weights and biases sized so that the gate spreads over (0.05, 0.95)
    c["W1"] = torch.randn(rd, C, generator=g) * (1.5 / C ** 0.5)
    c["b1"] = torch.randn(rd, generator=g) * 0.3 + 0.3
    c["W2"] = torch.randn(C, rd, generator=g) * (1.0 / rd ** 0.5)
    c["b2"] = torch.randn(C, generator=g) * 1.2
    c["res"] = R.bf16_round(torch.randn(N, HW, C, generator=g))              # both signs
    c["dout"] = R.bf16_round(torch.randn(N, HW, C, generator=g) * 0.1)
    return c


@functools.lru_cache(maxsize=None)
def _case(N, HW, C, rd):
    c = _inputs(N, HW, C, rd)
    c["ref"] = _tail(c, torch.float32)
    c["ref64"] = _tail(c, torch.float64, c["ref"]["mask"])
    c["ysum64"] = c["y"].double().sum(1)
    return c


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _pack_bits(mask):
    m = mask.flatten().to(torch.uint8).view(-1, 8)
    return (m << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)


def _unpack_bits(bits):
    return ((bits.cpu().view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).flatten().bool()


def _apply_ref(c, res):
    """u = fma(fma(y, scale, shift), e, res) with the reference's e: each fused multiply-add formed exactly in fp64 and rounded to
    fp32 once, which is what the kernel's two fp32 FMAs do.  Returns (z, u)."""
    z = (c["y"].double() * c["scale"].double() + c["shift"].double()).float()
    u = z.double() * c["ref"]["e"].double()[:, None, :]
    if res is not None:
        u = u + res.double()
    return z, u.float()


def _forward_on_gpu(lib, c):
    hip = _hip()
    N, HW, C, rd = c["shape"]
    yd = _dev(c["y"], torch.bfloat16)
    ysum = torch.full((N, C), float("nan"), device=DEV)
    nb = lib.icamd_se_squeeze_workspace_bytes(N, HW, C)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    assert lib.icamd_se_squeeze(hip.ptr(yd), hip.ptr(ysum), N, HW, C, hip.ptr(ws), nb, hip.stream_ptr()) == 0
    sc, sh = _dev(c["scale"]), _dev(c["shift"])
    w1, b1, w2, b2 = (_dev(c[k]) for k in ("W1", "b1", "W2", "b2"))
    s, e = (torch.full((N, C), float("nan"), device=DEV) for _ in range(2))
    h = torch.full((N, rd), float("nan"), device=DEV)
    assert lib.icamd_se_excite_fwd(hip.ptr(ysum), hip.ptr(sc), hip.ptr(sh), 1.0 / HW, hip.ptr(w1), hip.ptr(b1), hip.ptr(w2),
                                   hip.ptr(b2), hip.ptr(s), hip.ptr(h), hip.ptr(e), N, C, rd, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    return yd, sc, sh, ysum, s, h, e


@pytest.mark.parametrize("case", CASES)
def test_squeeze_and_excite(lib, case):
    c = _case(*case)
    ref = c["ref"]
    _, _, _, ysum, s, h, e = _forward_on_gpu(lib, c)
    errs = {"ysum": R.rel_l2(ysum.cpu(), c["ysum64"]), "s": R.rel_l2(s.cpu(), ref["s"]), "h": R.rel_l2(h.cpu(), ref["h"]),
            "e": R.rel_l2(e.cpu(), ref["e"])}
    print(case, {k: f"{v:.2e}" for k, v in errs.items()}, "gate range", float(ref["e"].min()), float(ref["e"].max()))
    assert float(ref["e"].min()) < 0.1 and float(ref["e"].max()) > 0.9 and float((ref["h"] > 0).float().mean()) > 0.2
    assert errs["ysum"] <= 1e-6
    assert errs["s"] <= 1e-5 and errs["h"] <= 1e-5 and errs["e"] <= 1e-5


@pytest.mark.parametrize("case", CASES)
def test_gated_apply(lib, case):
    """out and the mask bits of icamd_se_bn_apply, fed the reference's gate (the gate kernel has its own test), against the same
    arithmetic at the same rounding points: both fused multiply-adds formed exactly and rounded to fp32 once (_apply_ref), so the
    sign of the reference's pre-activation u is the kernel's.  The mask is compared with [u_ref > 0] wherever u_ref != 0 (|u_ref|
    exceeds a bf16 ulp of itself there); such positions must be >= 99 % of all."""
    hip = _hip()
    c = _case(*case)
    ref = c["ref"]
    N, HW, C, rd = c["shape"]
    yd, sc, sh = _dev(c["y"], torch.bfloat16), _dev(c["scale"]), _dev(c["shift"])
    e = _dev(ref["e"])
    resd = _dev(c["res"], torch.bfloat16)
    out = torch.empty_like(yd)
    bits = torch.zeros(yd.numel() // 8, dtype=torch.uint8, device=DEV)
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(e), hip.ptr(resd), None, None, hip.ptr(out),
                                 hip.ptr(bits), N, HW, C, 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    z, u = _apply_ref(c, c["res"])
    want = R.bf16_round(torch.relu(u))
    oc = out.float().cpu()
    print(case, "out: max ulp", R.max_bf16_ulp(oc, want), "rel-L2", R.rel_l2(oc, want))
    assert R.max_bf16_ulp(oc, want) <= 1.0 and R.rel_l2(oc, want) <= 1e-3
    clear = (u != 0).flatten()
    assert float(clear.float().mean()) >= 0.99
    assert torch.equal(_unpack_bits(bits)[clear], (u.flatten() > 0)[clear])
    assert torch.equal(_unpack_bits(bits), oc.flatten() > 0)          # the bits are those of the stored output
    # the res_bn form: the residual is a raw shortcut convolution output normalised on the fly == the plain form fed the
    # shortcut icamd_bn_apply would have stored
    g = torch.Generator().manual_seed(77)
    raw = _dev(R.bf16_round(torch.randn(N, HW, C, generator=g) * 2 + 0.5), torch.bfloat16)
    rsc, rsh = _dev(torch.rand(C, generator=g) + 0.5), _dev(torch.randn(C, generator=g) * 0.2)
    pre = torch.empty_like(raw)
    assert lib.icamd_bn_apply(hip.ptr(raw), hip.ptr(rsc), hip.ptr(rsh), None, hip.ptr(pre), None, raw.numel(), C, 0,
                              hip.stream_ptr()) == 0
    o1, o2 = torch.empty_like(yd), torch.empty_like(yd)
    m1, m2 = (torch.zeros(yd.numel() // 8, dtype=torch.uint8, device=DEV) for _ in range(2))
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(e), hip.ptr(raw), hip.ptr(rsc), hip.ptr(rsh),
                                 hip.ptr(o1), hip.ptr(m1), N, HW, C, 1, hip.stream_ptr()) == 0
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(e), hip.ptr(pre), None, None, hip.ptr(o2),
                                 hip.ptr(m2), N, HW, C, 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert R.max_bf16_ulp(o1.float().cpu(), o2.float().cpu()) <= 1.0 and R.rel_l2(o1.float().cpu(), o2.float().cpu()) <= 1e-3
    assert float(o1.float().abs().max()) > 0.0


def test_gated_apply_no_relu_no_residual(lib):
    hip = _hip()
    c = _case(*CASES[0])
    ref = c["ref"]
    N, HW, C, rd = c["shape"]
    yd, sc, sh, e = _dev(c["y"], torch.bfloat16), _dev(c["scale"]), _dev(c["shift"]), _dev(ref["e"])
    out = torch.empty_like(yd)
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(e), None, None, None, hip.ptr(out), None, N, HW, C,
                                 0, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    want = R.bf16_round(_apply_ref(c, None)[1])
    oc = out.float().cpu()
    assert float((oc < 0).float().mean()) > 0.1
    assert R.max_bf16_ulp(oc, want) <= 1.0 and R.rel_l2(oc, want) <= 1e-3


def _bwd_buffers(c, garbage=0.0):
    N, HW, C, rd = c["shape"]
    shapes = {"dgamma": (C,), "dbeta": (C,), "dW1": (rd, C), "db1": (rd,), "dW2": (C, rd), "db2": (C,)}
    out = {k: torch.full(s, garbage, device=DEV) for k, s in shapes.items()}
    out["dy"] = torch.full((N, HW, C), 7.0, dtype=torch.bfloat16, device=DEV)
    return out


def _run_bwd(lib, c, dev, out, accumulate=0, gamma=None, beta=None, ws=None):
    hip = _hip()
    N, HW, C, rd = c["shape"]
    nb = lib.icamd_se_bn_bwd_workspace_bytes(N, HW, C)
    assert nb > 0
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    rc = lib.icamd_se_bn_bwd(hip.ptr(dev["dout"]), hip.ptr(dev["bits"]), hip.ptr(dev["y"]), hip.ptr(dev["mean"]), hip.ptr(dev["invstd"]),
                             hip.ptr(dev["gamma"] if gamma is None else gamma), hip.ptr(dev["beta"] if beta is None else beta),
                             hip.ptr(dev["ysum"]), hip.ptr(dev["s"]), hip.ptr(dev["h"]), hip.ptr(dev["e"]), hip.ptr(dev["W1"]),
                             hip.ptr(dev["W2"]), hip.ptr(out["dgamma"]), hip.ptr(out["dbeta"]), hip.ptr(out["dW1"]),
                             hip.ptr(out["db1"]), hip.ptr(out["dW2"]), hip.ptr(out["db2"]), hip.ptr(out["dy"]), N, HW, C, rd,
                             accumulate, hip.ptr(ws), nb, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _bwd_inputs(c):
    """The backward's inputs from the fp32 reference (the kernel is tested on its own, not behind the forward kernels)."""
    ref = c["ref"]
    dev = {k: _dev(c[k]) for k in ("mean", "invstd", "gamma", "beta", "W1", "W2")}
    dev.update(y=_dev(c["y"], torch.bfloat16), dout=_dev(c["dout"], torch.bfloat16), bits=_pack_bits(ref["mask"]).to(DEV),
               ysum=_dev(c["y"].sum(1)), s=_dev(ref["s"]), h=_dev(ref["h"]), e=_dev(ref["e"]))
    return dev


@pytest.mark.parametrize("case", CASES)
def test_backward(lib, case):
    c = _case(*case)
    ref, ref64 = c["ref"], c["ref64"]
    # the yardstick first: fp32 autograd on the rounded inputs against its fp64 copy
    noise = {k: R.rel_l2(ref[k], ref64[k].float()) for k in GRADS + ("dy",)}
    print(case, "reference vs its fp64 copy:", {k: f"{v:.1e}" for k, v in noise.items()})
    for k in GRADS + ("dy",):
        assert float(ref[k].abs().max()) > 0.0 and noise[k] <= 5e-5, (k, noise[k])
    dev = _bwd_inputs(c)
    out = _bwd_buffers(c, garbage=3.0)
    assert _run_bwd(lib, c, dev, out) == 0
    errs = {k: R.rel_l2(out[k].cpu(), ref[k]) for k in GRADS}
    want_dy = R.bf16_round(ref["dy"])
    got_dy = out["dy"].float().cpu()
    print(case, "HIP:", {k: f"{v:.1e}" for k, v in errs.items()}, "dy", f"{R.rel_l2(got_dy, want_dy):.1e}")
    assert R.rel_l2(got_dy, want_dy) <= 1e-3 and R.bf16_close(got_dy, want_dy)
    for k in GRADS:
        assert errs[k] <= 1e-4, (k, errs[k])
    # two consecutive calls: bit-identical in every output
    out2 = _bwd_buffers(c, garbage=-1.0)
    assert _run_bwd(lib, c, dev, out2) == 0
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    # accumulate = 1 on top of the first call: twice one call's worth
    assert _run_bwd(lib, c, dev, out2, accumulate=1) == 0
    for k in GRADS:
        assert R.rel_l2(out2[k].cpu(), 2.0 * out[k].cpu()) <= 1e-6, k
    assert torch.equal(out2["dy"], out["dy"])
    # gamma = beta = 0: the four SE gradients are exact zeros
    out0 = _bwd_buffers(c, garbage=5.0)
    zero = torch.zeros(case[2], device=DEV)
    assert _run_bwd(lib, c, dev, out0, gamma=zero, beta=zero) == 0
    for k in ("dW1", "db1", "dW2", "db2"):
        assert float(out0[k].abs().max()) == 0.0, k
    assert float(out0["dy"].float().abs().max()) == 0.0 and float(out0["dbeta"].abs().max()) > 0.0


def test_bad_arguments(lib):
    hip = _hip()
    c = _case(*CASES[0])
    N, HW, C, rd = c["shape"]
    dev = _bwd_inputs(c)
    out = _bwd_buffers(c, garbage=3.0)
    nb = lib.icamd_se_bn_bwd_workspace_bytes(N, HW, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    sp = hip.stream_ptr()
    BAD, UNSUPPORTED, WORKSPACE = 1, 2, 3

    def bwd(y=hip.ptr(dev["y"]), dy=hip.ptr(out["dy"]), dw1=hip.ptr(out["dW1"]), C=C, rd=rd, nbytes=nb, wsp=hip.ptr(ws)):
        return lib.icamd_se_bn_bwd(hip.ptr(dev["dout"]), hip.ptr(dev["bits"]), y, hip.ptr(dev["mean"]), hip.ptr(dev["invstd"]),
                                   hip.ptr(dev["gamma"]), hip.ptr(dev["beta"]), hip.ptr(dev["ysum"]), hip.ptr(dev["s"]),
                                   hip.ptr(dev["h"]), hip.ptr(dev["e"]), hip.ptr(dev["W1"]), hip.ptr(dev["W2"]),
                                   hip.ptr(out["dgamma"]), hip.ptr(out["dbeta"]), dw1, hip.ptr(out["db1"]), hip.ptr(out["dW2"]),
                                   hip.ptr(out["db2"]), dy, N, HW, C, rd, 0, wsp, nbytes, sp)

    assert bwd(y=None) == BAD and bwd(dy=None) == BAD and bwd(dw1=None) == BAD and bwd(wsp=None) == BAD
    assert bwd(C=12) == UNSUPPORTED and bwd(C=8192) == UNSUPPORTED and bwd(rd=512) == UNSUPPORTED
    assert bwd(nbytes=nb - 1) == WORKSPACE and bwd(nbytes=0) == WORKSPACE
    ysum = torch.full((N, C), 9.0, device=DEV)
    sq = lib.icamd_se_squeeze_workspace_bytes(N, HW, C)
    assert lib.icamd_se_squeeze(None, hip.ptr(ysum), N, HW, C, hip.ptr(ws), nb, sp) == BAD
    assert lib.icamd_se_squeeze(hip.ptr(dev["y"]), None, N, HW, C, hip.ptr(ws), nb, sp) == BAD
    assert lib.icamd_se_squeeze(hip.ptr(dev["y"]), hip.ptr(ysum), N, HW, 12, hip.ptr(ws), nb, sp) == UNSUPPORTED
    assert lib.icamd_se_squeeze(hip.ptr(dev["y"]), hip.ptr(ysum), N, HW, C, hip.ptr(ws), sq - 1, sp) == WORKSPACE
    e = dev["e"]
    assert lib.icamd_se_excite_fwd(hip.ptr(ysum), hip.ptr(dev["gamma"]), hip.ptr(dev["beta"]), 1.0, hip.ptr(dev["W1"]), None,
                                   hip.ptr(dev["W2"]), hip.ptr(dev["beta"]), hip.ptr(dev["s"]), hip.ptr(dev["h"]), hip.ptr(e), N, C,
                                   rd, sp) == BAD
    assert lib.icamd_se_excite_fwd(hip.ptr(ysum), hip.ptr(dev["gamma"]), hip.ptr(dev["beta"]), 1.0, hip.ptr(dev["W1"]),
                                   hip.ptr(dev["beta"]), hip.ptr(dev["W2"]), hip.ptr(dev["beta"]), hip.ptr(dev["s"]),
                                   hip.ptr(dev["h"]), hip.ptr(e), N, C, 257, sp) == UNSUPPORTED
    o = torch.full((N, HW, C), 7.0, dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_se_bn_apply(hip.ptr(dev["y"]), hip.ptr(dev["gamma"]), hip.ptr(dev["beta"]), None, None, None, None, hip.ptr(o),
                                 None, N, HW, C, 1, sp) == BAD
    assert lib.icamd_se_bn_apply(hip.ptr(dev["y"]), hip.ptr(dev["gamma"]), hip.ptr(dev["beta"]), hip.ptr(e), None, hip.ptr(dev["gamma"]),
                                 hip.ptr(dev["beta"]), hip.ptr(o), None, N, HW, C, 1, sp) == BAD      # res_bn without a residual
    assert lib.icamd_se_bn_apply(hip.ptr(dev["y"]), hip.ptr(dev["gamma"]), hip.ptr(dev["beta"]), hip.ptr(e), None, None, None,
                                 hip.ptr(o), None, N, HW, 12, 1, sp) == UNSUPPORTED
    torch.cuda.synchronize()
    # no launch happened: every output still holds what it was filled with
    assert float(ysum.min()) == 9.0 and float(o.float().min()) == 7.0 and float(out["dy"].float().min()) == 7.0
    assert all(float(out[k].min()) == 3.0 and float(out[k].max()) == 3.0 for k in GRADS)
