"""What the token models share beyond the arenas: the GEMM / LayerNorm steps of a forward and a backward pass on raw pointers
(ViT, Swin, ConvNeXt), and the pre-LayerNorm transformer block of ViT and Swin -- its parameters, its activations and its two
chains, each written once.

  Forward    one forward pass: linear, linear_gelu, layernorm, residual (a branch that stochastic depth may drop), and `block`
             norm1 -> qkv -> attention -> proj (+ x) -> norm2 -> fc1 + GELU -> fc2 (+ x1)
  Backward   one backward pass: gemm (weight and bias gradient on the side lane, then the data gradient), layernorm, and `block`,
             the same chain in reverse

A model supplies what is its own: the attention launches (callables), the LayerNorm epsilon, its scratch buffers and its SideLane
(streams.py; a model without a second stream passes a lane that is never enabled, whose launches stay on the main stream).
Stochastic depth is Swin's: a block whose `keep` masks are None (every ViT block) has its residual adds in the GEMM epilogues.
"""
import ctypes

import torch

from . import hip
from .arena import Lin


def lin_builder(lins, param):
    """-> lin(name, cin, cout, cout_p=None, bias=True): a Lin appended to `lins`, its weight and bias from param(name, torch shape,
    kind, padded shape) -- Layout.add for a model that lays out as it goes, a lookup for one that has laid out before."""
    def lin(name, cin, cout, cout_p=None, bias=True):
        l = Lin(name, cin, cout, cout_p)
        l.w = param(name + ".weight", (cout, cin), "lin", (l.cout_p, cin))
        l.b = param(name + ".bias", (cout,), "vec", (l.cout_p,)) if bias else None
        lins.append(l)
        return l
    return lin


def block_params(n, dim, hidden, param, lin):
    """The parameters of block `n`, in timm's order."""
    blk = {"name": n}
    blk["n1w"], blk["n1b"] = param(f"{n}.norm1.weight", (dim,), "vec", (dim,)), param(f"{n}.norm1.bias", (dim,), "vec", (dim,))
    blk["qkv"] = lin(f"{n}.attn.qkv", dim, 3 * dim)
    blk["proj"] = lin(f"{n}.attn.proj", dim, dim)
    blk["n2w"], blk["n2b"] = param(f"{n}.norm2.weight", (dim,), "vec", (dim,)), param(f"{n}.norm2.bias", (dim,), "vec", (dim,))
    blk["fc1"] = lin(f"{n}.mlp.fc1", dim, hidden)
    blk["fc2"] = lin(f"{n}.mlp.fc2", hidden, dim)
    return blk


def block_workspace(dev, rows, dim, hidden, lse_elems):
    """The activations one block keeps for its backward pass."""
    def act(c):
        return torch.empty(rows, c, dtype=torch.bfloat16, device=dev)

    def f32(n):
        return torch.empty(n, dtype=torch.float32, device=dev)

    return {"h": act(dim), "qkv": act(3 * dim), "ao": act(dim), "x1": act(dim), "h2": act(dim), "z": act(hidden), "a": act(hidden),
            "x2": act(dim), "lse": f32(lse_elems), "st1": f32(2 * rows), "st2": f32(2 * rows), "keep1": None, "keep2": None}


def loss_workspace(ws, B, ncls_p, dev):
    """The tensors the loss kernels read and write (engine.py): padded logits and their gradient, per-row loss, prediction."""
    ws["logits"] = torch.zeros(B, ncls_p, dtype=torch.bfloat16, device=dev)
    ws["dlogits"] = torch.zeros(B, ncls_p, dtype=torch.bfloat16, device=dev)
    ws["loss_rows"] = torch.empty(B, dtype=torch.float32, device=dev)
    ws["pred"] = torch.empty(B, dtype=torch.int32, device=dev)


def patch_embed_desc(model, B, dim, patch):
    """The patch-embedding convolution (patch x patch, stride patch, on the 8-channel packed input) at batch B."""
    key = ("pe", B)
    d = model._ws.get(key)
    if d is None:
        d = model._ws[key] = hip.conv_desc(B, model.img_size, model.img_size, 8, dim, patch, patch, patch, 0)
    return d


class Forward:
    """The steps of one forward pass of `model` on the current stream.  logits_only: no backward will read this pass's activations,
    so the pre-GELU ones are not written."""

    def __init__(self, model, ws, eps, logits_only=False):
        self.m, self.lib, self.ws, self.eps, self.logits_only = model, model.lib, ws, eps, logits_only
        self.s = hip.stream_ptr()

    def linear(self, l, desc, x_ptr, y_ptr, addend_ptr=None):
        """y = x W^T (+ b) (+ addend) in one kernel"""
        m = self.m
        hip.check(self.lib.icamd_conv2d_fwd(ctypes.byref(desc), x_ptr, m._w(l), y_ptr, None if l.b is None else m._pf(l.b),
                                            addend_ptr, None, self.s), l.name)

    def linear_gelu(self, l, desc, x_ptr, z_ptr, a_ptr):
        """z = x W^T + b, a = gelu(z) in one kernel"""
        hip.check(self.lib.icamd_conv2d_fwd_gelu(ctypes.byref(desc), x_ptr, self.m._w(l), None if self.logits_only else z_ptr,
                                                 a_ptr, self.m._pf(l.b), self.s), l.name + " + gelu")

    def layernorm(self, x_ptr, wp, bp, y_ptr, st, rows, C):
        """`st`: pointer to the row statistics, rows means and then rows reciprocal standard deviations"""
        hip.check(self.lib.icamd_layernorm_fwd(x_ptr, self.m._pf(wp), self.m._pf(bp), y_ptr, st, st + 4 * rows, rows, C, self.eps,
                                               self.s), wp.name)

    def residual(self, l, desc, x_ptr, res_ptr, y_ptr, keep, tmp_ptr, rows, C, tokens_per_image):
        """y = res + x W^T + b in one kernel -- or, under a stochastic-depth mask `keep` (float [B], 0 or 1 / keep_prob), the branch
        into the scratch `tmp` and y = res + keep * branch"""
        if keep is None:
            return self.linear(l, desc, x_ptr, y_ptr, res_ptr)
        self.linear(l, desc, x_ptr, tmp_ptr)
        hip.check(self.lib.icamd_layerscale_fwd(tmp_ptr, res_ptr, self.m.ones.data_ptr(), keep.data_ptr(), y_ptr, rows, C,
                                                tokens_per_image, self.s), "drop path")

    def block(self, blk, b, x, rows, dim, attn_fwd, keep1=None, keep2=None, tokens_per_image=None):
        """One block on the tensor `x`; returns its output b["x2"].  attn_fwd(blk, b) launches qkv -> ao (and lse).  keep1 / keep2:
        this step's per-sample stochastic-depth masks of the two branches (float [B], 0 or 1 / keep_prob), None for a branch that
        is never dropped."""
        b["keep1"], b["keep2"], b["x"] = keep1, keep2, x
        h, h2, x1 = b["h"].data_ptr(), b["h2"].data_ptr(), b["x1"].data_ptr()
        self.layernorm(x.data_ptr(), blk["n1w"], blk["n1b"], h, b["st1"].data_ptr(), rows, dim)
        self.linear(blk["qkv"], blk["qkv"].desc(rows), h, b["qkv"].data_ptr())
        attn_fwd(blk, b)
        proj, fc2 = blk["proj"], blk["fc2"]
        # x1 = x + keep1 * proj(attn); a dropped branch passes through h2's buffer (LayerNorm 2 overwrites it next)
        self.residual(proj, proj.desc(rows), b["ao"].data_ptr(), x.data_ptr(), x1, keep1, h2, rows, dim, tokens_per_image)
        self.layernorm(x1, blk["n2w"], blk["n2b"], h2, b["st2"].data_ptr(), rows, dim)
        self.linear_gelu(blk["fc1"], blk["fc1"].desc(rows), h2, b["z"].data_ptr(), b["a"].data_ptr())
        # x2 = x1 + keep2 * mlp; every buffer of the block is still needed by the backward: a dropped branch has a scratch of its own
        t = None if keep2 is None else self.m._branch_tmp(self.ws).data_ptr()
        self.residual(fc2, fc2.desc(rows), b["a"].data_ptr(), x1, b["x2"].data_ptr(), keep2, t, rows, dim, tokens_per_image)
        return b["x2"]


class Backward:
    """The steps of one backward pass of `model` on the current stream; weight gradients go through `lane` (streams.py), which this
    begins.  A buffer a pending side launch still reads is waited for before the main stream overwrites it (`writes`)."""

    def __init__(self, model, ws, lane, accumulate):
        self.m, self.lib, self.ws, self.lane = model, model.lib, ws, lane
        self.s = hip.stream_ptr()
        self.acc = int(bool(accumulate))
        self.wg = ws["wg_ws"].data_ptr(), ws["wg_bytes"]
        self.ln = ws["ln_ws"].data_ptr(), ws["ln_bytes"]
        lane.begin(getattr(model, "wgrad_side_stream", True))

    def writes(self, ptr):
        """`ptr` is about to be overwritten on the main stream: wait for the side-lane launches that still read it."""
        self.lane.before_write(ptr)
        return ptr

    def gemm(self, l, desc, x_ptr, dy_ptr, dx_ptr, gelu_z=None):
        """Weight and bias gradients of y = x W^T + b on the side lane, then the data gradient into dx when given; gelu_z: dx =
        (dy W) * gelu'(z), the GELU backward riding in the data-gradient kernel's store pass."""
        m, lib, acc = self.m, self.lib, self.acc
        wsp, wsb = self.wg
        d = ctypes.byref(desc)
        if l.b is None:
            self.lane.launch(lambda st: hip.check(lib.icamd_conv2d_wgrad(d, x_ptr, dy_ptr, m._gf(l.w), acc, wsp, wsb, st),
                                                  l.name + " wgrad"), reads=(dy_ptr,))
        else:
            self.lane.launch(lambda st: hip.check(lib.icamd_conv2d_wgrad_bias(d, x_ptr, dy_ptr, m._gf(l.w), m._gf(l.b), acc, wsp,
                                                                              wsb, st), l.name + " wgrad+bias"), reads=(dy_ptr,))
        if dx_ptr is None:
            return
        if gelu_z is None:
            hip.check(lib.icamd_conv2d_dgrad(d, dy_ptr, m._wt(l), self.writes(dx_ptr), None, None, self.s), l.name + " dgrad")
        else:
            hip.check(lib.icamd_conv2d_dgrad_gelu(d, dy_ptr, m._wt(l), gelu_z, self.writes(dx_ptr), self.s),
                      l.name + " dgrad + gelu bwd")

    def layernorm(self, dy_ptr, x_ptr, st, wp, bp, addend_ptr, dx_ptr, rows, C):
        """dx = LayerNorm'(dy) (+ addend), and the gradients of the weight and the bias"""
        m = self.m
        hip.check(self.lib.icamd_layernorm_bwd(dy_ptr, x_ptr, st, st + 4 * rows, m._pf(wp), addend_ptr, self.writes(dx_ptr),
                                               m._gf(wp), m._gf(bp), rows, C, self.acc, *self.ln, self.s), wp.name + " bwd")

    def drop_path(self, dout_ptr, keep, dz_ptr, rows, C, tokens_per_image):
        """gradient of a dropped branch (Swin's two, ConvNeXt V2's): dz = dout * keep (the entry's dgamma goes to a scratch vector)"""
        m, ws = self.m, self.ws
        hip.check(self.lib.icamd_layerscale_bwd(dout_ptr, dout_ptr, m.ones.data_ptr(), keep.data_ptr(), self.writes(dz_ptr),
                                                ws["ls_dg"].data_ptr(), rows, C, tokens_per_image, 0, ws["ls_ws"].data_ptr(),
                                                ws["ls_bytes"], self.s), "drop path bwd")
        return dz_ptr

    def block(self, blk, b, rows, dim, dx, scratch, attn_bwd, tokens_per_image=None):
        """One block: `dx` (pointer) holds the gradient of its output and receives that of its input.  scratch: pointers (t0, t1,
        t2, dz, dqkv) -- three [rows][dim] (t2 only for a dropped branch), one [rows][hidden], one [rows][3 dim].
        attn_bwd(blk, b, dao, dqkv) launches the attention's backward from d(ao) into d(qkv)."""
        t0, t1, t2, dz, dqkv = scratch
        d2 = dx                                                                    # gradient of x2 = x1 + keep2 * fc2(a)
        if b["keep2"] is not None:
            d2 = self.drop_path(dx, b["keep2"], t2, rows, dim, tokens_per_image)
        self.gemm(blk["fc2"], blk["fc2"].desc(rows), b["a"].data_ptr(), d2, dz, gelu_z=b["z"].data_ptr())      # d z
        self.gemm(blk["fc1"], blk["fc1"].desc(rows), b["h2"].data_ptr(), dz, t0)                               # d h2
        dx1 = t1                                                                   # = LN2'(dh2) + dx
        self.layernorm(t0, b["x1"].data_ptr(), b["st2"].data_ptr(), blk["n2w"], blk["n2b"], dx, dx1, rows, dim)
        d1 = dx1
        if b["keep1"] is not None:
            d1 = self.drop_path(dx1, b["keep1"], t2, rows, dim, tokens_per_image)
        self.gemm(blk["proj"], blk["proj"].desc(rows), b["ao"].data_ptr(), d1, t0)                             # d attention out
        attn_bwd(blk, b, t0, self.writes(dqkv))
        self.gemm(blk["qkv"], blk["qkv"].desc(rows), b["h"].data_ptr(), dqkv, t0)                              # d h
        # dx is dead after LayerNorm 2's backward: dx = LN1'(dh) + dx1
        self.layernorm(t0, b["x"].data_ptr(), b["st1"].data_ptr(), blk["n1w"], blk["n1b"], dx1, dx, rows, dim)
