"""Shared by tests/test_se_kernels_gpu.py, tests/test_multitrip_gpu.py and tests/test_numeric_ranges_gpu.py: the cases of the
squeeze-and-excitation kernels (csrc/se_ops.hip), their seeded inputs, the torch reference of the block tail, and the launches of
the forward chain and of icamd_se_bn_bwd.  Importing it needs no GPU."""
import torch

import _harness
from _harness import DEV
from oracle import ops_ref as R

EPS = 1e-5
CASES = [(3, 49, 256, 16), (2, 196, 512, 32), (5, 9, 2048, 128), (4, 1, 256, 16), (1, 3136, 256, 16), (3, 35, 64, 8)]
GRADS = ("dgamma", "dbeta", "dW1", "db1", "dW2", "db2")


def tail(c, dt, mask=None):
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


def inputs(N, HW, C, rd):
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


def to_dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def pack_bits(mask):
    m = mask.flatten().to(torch.uint8).view(-1, 8)
    return (m << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)


def apply_ref(c, res):
    """u = fma(fma(y, scale, shift), e, res) with the reference's e: each fused multiply-add formed exactly in fp64 and rounded to
    fp32 once, which is what the kernel's two fp32 FMAs do.  Returns (z, u)."""
    z = (c["y"].double() * c["scale"].double() + c["shift"].double()).float()
    u = z.double() * c["ref"]["e"].double()[:, None, :]
    if res is not None:
        u = u + res.double()
    return z, u.float()


def forward_on_gpu(lib, c):
    hip = _harness.hip()
    N, HW, C, rd = c["shape"]
    yd = to_dev(c["y"], torch.bfloat16)
    ysum = torch.full((N, C), float("nan"), device=DEV)
    nb = lib.icamd_se_squeeze_workspace_bytes(N, HW, C)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    assert lib.icamd_se_squeeze(hip.ptr(yd), hip.ptr(ysum), N, HW, C, hip.ptr(ws), nb, hip.stream_ptr()) == 0
    sc, sh = to_dev(c["scale"]), to_dev(c["shift"])
    w1, b1, w2, b2 = (to_dev(c[k]) for k in ("W1", "b1", "W2", "b2"))
    s, e = (torch.full((N, C), float("nan"), device=DEV) for _ in range(2))
    h = torch.full((N, rd), float("nan"), device=DEV)
    assert lib.icamd_se_excite_fwd(hip.ptr(ysum), hip.ptr(sc), hip.ptr(sh), 1.0 / HW, hip.ptr(w1), hip.ptr(b1), hip.ptr(w2),
                                   hip.ptr(b2), hip.ptr(s), hip.ptr(h), hip.ptr(e), N, C, rd, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    return yd, sc, sh, ysum, s, h, e


def bwd_buffers(c, garbage=0.0):
    N, HW, C, rd = c["shape"]
    shapes = {"dgamma": (C,), "dbeta": (C,), "dW1": (rd, C), "db1": (rd,), "dW2": (C, rd), "db2": (C,)}
    out = {k: torch.full(s, garbage, device=DEV) for k, s in shapes.items()}
    out["dy"] = torch.full((N, HW, C), 7.0, dtype=torch.bfloat16, device=DEV)
    return out


def run_bwd(lib, c, dev, out, accumulate=0, gamma=None, beta=None, ws=None):
    hip = _harness.hip()
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


def bwd_inputs(c):
    """The backward's inputs from the fp32 reference (the kernel is tested on its own, not behind the forward kernels)."""
    ref = c["ref"]
    dev = {k: to_dev(c[k]) for k in ("mean", "invstd", "gamma", "beta", "W1", "W2")}
    dev.update(y=to_dev(c["y"], torch.bfloat16), dout=to_dev(c["dout"], torch.bfloat16), bits=pack_bits(ref["mask"]).to(DEV),
               ysum=to_dev(c["y"].sum(1)), s=to_dev(ref["s"]), h=to_dev(ref["h"]), e=to_dev(ref["e"]))
    return dev
