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

import _harness
from _harness import lib  # noqa: F401
from _se_kernels import (CASES, GRADS, apply_ref, bwd_buffers, bwd_inputs, forward_on_gpu, inputs, run_bwd, tail,
                         to_dev)
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(N, HW, C, rd):
    c = inputs(N, HW, C, rd)
    c["ref"] = tail(c, torch.float32)
    c["ref64"] = tail(c, torch.float64, c["ref"]["mask"])
    c["ysum64"] = c["y"].double().sum(1)
    return c


def _unpack_bits(bits):
    return ((bits.cpu().view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).flatten().bool()


@pytest.mark.parametrize("case", CASES)
def test_squeeze_and_excite(lib, case):
    c = _case(*case)
    ref = c["ref"]
    _, _, _, ysum, s, h, e = forward_on_gpu(lib, c)
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
    hip = _harness.hip()
    c = _case(*case)
    ref = c["ref"]
    N, HW, C, rd = c["shape"]
    yd, sc, sh = to_dev(c["y"], torch.bfloat16), to_dev(c["scale"]), to_dev(c["shift"])
    e = to_dev(ref["e"])
    resd = to_dev(c["res"], torch.bfloat16)
    out = torch.empty_like(yd)
    bits = torch.zeros(yd.numel() // 8, dtype=torch.uint8, device=DEV)
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(e), hip.ptr(resd), None, None, hip.ptr(out),
                                 hip.ptr(bits), N, HW, C, 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    z, u = apply_ref(c, c["res"])
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
    raw = to_dev(R.bf16_round(torch.randn(N, HW, C, generator=g) * 2 + 0.5), torch.bfloat16)
    rsc, rsh = to_dev(torch.rand(C, generator=g) + 0.5), to_dev(torch.randn(C, generator=g) * 0.2)
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
    hip = _harness.hip()
    c = _case(*CASES[0])
    ref = c["ref"]
    N, HW, C, rd = c["shape"]
    yd, sc, sh, e = to_dev(c["y"], torch.bfloat16), to_dev(c["scale"]), to_dev(c["shift"]), to_dev(ref["e"])
    out = torch.empty_like(yd)
    assert lib.icamd_se_bn_apply(hip.ptr(yd), hip.ptr(sc), hip.ptr(sh), hip.ptr(e), None, None, None, hip.ptr(out), None, N, HW, C,
                                 0, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    want = R.bf16_round(apply_ref(c, None)[1])
    oc = out.float().cpu()
    assert float((oc < 0).float().mean()) > 0.1
    assert R.max_bf16_ulp(oc, want) <= 1.0 and R.rel_l2(oc, want) <= 1e-3


@pytest.mark.parametrize("case", CASES)
def test_backward(lib, case):
    c = _case(*case)
    ref, ref64 = c["ref"], c["ref64"]
    # the yardstick first: fp32 autograd on the rounded inputs against its fp64 copy
    noise = {k: R.rel_l2(ref[k], ref64[k].float()) for k in GRADS + ("dy",)}
    print(case, "reference vs its fp64 copy:", {k: f"{v:.1e}" for k, v in noise.items()})
    for k in GRADS + ("dy",):
        assert float(ref[k].abs().max()) > 0.0 and noise[k] <= 5e-5, (k, noise[k])
    dev = bwd_inputs(c)
    out = bwd_buffers(c, garbage=3.0)
    assert run_bwd(lib, c, dev, out) == 0
    errs = {k: R.rel_l2(out[k].cpu(), ref[k]) for k in GRADS}
    want_dy = R.bf16_round(ref["dy"])
    got_dy = out["dy"].float().cpu()
    print(case, "HIP:", {k: f"{v:.1e}" for k, v in errs.items()}, "dy", f"{R.rel_l2(got_dy, want_dy):.1e}")
    assert R.rel_l2(got_dy, want_dy) <= 1e-3 and R.bf16_close(got_dy, want_dy)
    for k in GRADS:
        assert errs[k] <= 1e-4, (k, errs[k])
    # two consecutive calls: bit-identical in every output
    out2 = bwd_buffers(c, garbage=-1.0)
    assert run_bwd(lib, c, dev, out2) == 0
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    # accumulate = 1 on top of the first call: twice one call's worth
    assert run_bwd(lib, c, dev, out2, accumulate=1) == 0
    for k in GRADS:
        assert R.rel_l2(out2[k].cpu(), 2.0 * out[k].cpu()) <= 1e-6, k
    assert torch.equal(out2["dy"], out["dy"])
    # gamma = beta = 0: the four SE gradients are exact zeros
    out0 = bwd_buffers(c, garbage=5.0)
    zero = torch.zeros(case[2], device=DEV)
    assert run_bwd(lib, c, dev, out0, gamma=zero, beta=zero) == 0
    for k in ("dW1", "db1", "dW2", "db2"):
        assert float(out0[k].abs().max()) == 0.0, k
    assert float(out0["dy"].float().abs().max()) == 0.0 and float(out0["dbeta"].abs().max()) > 0.0


def test_bad_arguments(lib):
    hip = _harness.hip()
    c = _case(*CASES[0])
    N, HW, C, rd = c["shape"]
    dev = bwd_inputs(c)
    out = bwd_buffers(c, garbage=3.0)
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
