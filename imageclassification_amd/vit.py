"""ViT-B/16 (timm `vit_base_patch16_224`) on the gfx950 kernels: hand-written forward and backward.

The reference builds the model with timm.create_model(args.model) (/root/reference/train.py:194); BASELINE.json's
configs[3] is ViT-B/16 bf16 at 224x224.  Architecture restated from timm (absent here, see oracle/vit_ref.py):
16x16/16 patch-embedding conv + bias, class token, learned position embedding, 12 pre-LayerNorm blocks
(LayerNorm eps 1e-6, 12-head attention with fused QKV projection, exact-GELU MLP x4), final LayerNorm, class-token
pooling, linear head.  Parameter names follow timm (`cls_token`, `pos_embed`, `patch_embed.proj.*`,
`blocks.N.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.*`, `norm.*`, `head.*`).

Every Linear is the 1x1 case of the implicit-GEMM convolution kernels on a [B*T, 1, 1, C] "image" (bias and the
residual add fused in the epilogue); LayerNorm / GELU / attention are the token kernels of include/icamd.h.
The flat arenas (fp32 parameters and gradients, bf16 shadow weights and their transposes) are arena.py's; the block (parameters,
activations, forward and backward chain) and the GEMM / LayerNorm steps are blocks.py's.  What is written here: the configurations,
the tokens (class token, position embedding, class-token pooling and their gradients), the attention launches and the scratch.
"""
import ctypes
import math
from collections import OrderedDict

import torch

from . import hip
from .arena import ArenaModel, Layout, Lin
from .blocks import Backward, Forward, block_params, block_workspace, lin_builder, loss_workspace, patch_embed_desc
from .streams import side_lane

LN_EPS = 1e-6
SCALE = 64 ** -0.5      # of the attention scores: the head dimension is 64

CONFIGS = {
    # name: (patch, dim, depth, heads, mlp_ratio)
    "vit_base_patch16_224": (16, 768, 12, 12, 4),
    "vit_small_patch16_224": (16, 384, 12, 6, 4),
    "vit_base_patch16_384": (16, 768, 12, 12, 4),    # the _224 architectures at their fine-tuning resolution (T = 577)
    "vit_small_patch16_384": (16, 384, 12, 6, 4),
    "vit_tiny_test": (16, 128, 2, 2, 4),   # small configuration for parity tests
}


# input size a name is built at when none is given (timm: the model's default_cfg; 224 for every other name)
NATIVE_SIZE = {"vit_base_patch16_384": 384, "vit_small_patch16_384": 384}


class VisionTransformer(ArenaModel):
    def __init__(self, arch="vit_base_patch16_224", num_classes=1000, device="cuda", img_size=None, seed=None):
        super().__init__(arch, num_classes, device)
        self.patch, self.dim, self.depth, self.heads, mlp_ratio = CONFIGS[arch]
        if self.dim // self.heads != 64:
            raise ValueError("the attention kernel is built for a head dimension of 64")
        self.hidden = self.dim * mlp_ratio
        if img_size is None:
            img_size = NATIVE_SIZE.get(arch, 224)
        if img_size < self.patch or img_size % self.patch != 0:
            raise ValueError(f"img_size {img_size} is not a positive multiple of the patch size {self.patch}")
        self.img_size = img_size
        self.grid = img_size // self.patch
        self.T = self.grid * self.grid + 1
        self._build()
        self.init_weights(seed)

    # ------------------------------------------------------------------ structure / arenas
    def _build(self):
        D = self.dim
        layout = Layout()
        add = layout.add
        self.lins = []
        lin = lin_builder(self.lins, add)
        self.p_cls = add("cls_token", (1, 1, D), "vec", (D,))
        self.p_pos = add("pos_embed", (1, self.T, D), "vec", (self.T * D,))
        self.pe = Lin("patch_embed.proj", 8, D)      # the patch-embedding convolution; its descriptor is _pe_desc's
        self.pe.w = add("patch_embed.proj.weight", (D, 3, self.patch, self.patch), "conv", (D, self.patch, self.patch, 8))
        self.pe.b = add("patch_embed.proj.bias", (D,), "vec", (D,))
        self.blocks = [block_params(f"blocks.{i}", D, self.hidden, add, lin) for i in range(self.depth)]
        self.p_nw = add("norm.weight", (D,), "vec", (D,))
        self.p_nb = add("norm.bias", (D,), "vec", (D,))
        self.head = lin("head", D, self.num_classes, self.ncls_p)
        self._allocate(layout, [(l, l.cout_p, 1, l.cin) for l in self.lins])

    def _ctor_kwargs(self):
        return {"arch": self.arch, "num_classes": self.num_classes, "img_size": self.img_size}

    def init_weights(self, seed=None):
        """timm's default ViT init: trunc_normal(std .02) weights / pos_embed, zero biases, cls_token std 1e-6, LayerNorm
        1 / 0; the patch-embedding conv keeps torch's Conv2d default (Kaiming-uniform, a = sqrt(5))."""
        g = torch.Generator()
        g.manual_seed(seed if seed is not None else torch.initial_seed() % (2 ** 63))
        sd = OrderedDict()

        def tn(shape, std):
            return torch.nn.init.trunc_normal_(torch.empty(shape), std=std, generator=g)

        for name, p in self.params.items():
            if name == "cls_token":
                sd[name] = torch.randn(p.torch_shape, generator=g) * 1e-6
            elif name == "pos_embed":
                sd[name] = tn(p.torch_shape, 0.02)
            elif name == "patch_embed.proj.weight":
                fan_in = 3 * self.patch * self.patch
                bound = 1.0 / math.sqrt(fan_in)
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) * bound
            elif name == "patch_embed.proj.bias":
                bound = 1.0 / math.sqrt(3 * self.patch * self.patch)
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) * bound
            elif p.kind == "lin":
                sd[name] = tn(p.torch_shape, 0.02)
            elif name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
                sd[name] = torch.ones(p.torch_shape)
            else:
                sd[name] = torch.zeros(p.torch_shape)
        self.load_state_dict(sd)

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is not None:
            return ws
        dev, lib = self.device, self.lib
        D, T, Hd = self.dim, self.T, self.hidden
        M = B * T

        def act(r, c):
            return torch.empty(r, c, dtype=torch.bfloat16, device=dev)

        ws = {"B": B, "M": M}
        ws["x8"] = torch.empty(B, self.img_size, self.img_size, 8, dtype=torch.bfloat16, device=dev)
        ws["patches"] = act(B * (T - 1), D)
        ws["x0"] = act(M, D)
        ws["blocks"] = [block_workspace(dev, M, D, Hd, B * self.heads * T) for _ in range(self.depth)]
        ws["cls_rows"] = act(B, D)
        ws["pooled"] = act(B, D)
        ws["stf"] = torch.empty(2 * B, dtype=torch.float32, device=dev)
        loss_workspace(ws, B, self.ncls_p, dev)
        # backward scratch
        ws["g768"] = [act(M, D) for _ in range(3)]
        ws["g3072"] = act(M, Hd)
        ws["g3072b"] = act(M, Hd)
        ws["g2304"] = act(M, 3 * D)
        ws["dpooled"] = act(B, D)
        ws["dcls"] = act(B, D)
        ws["delta"] = torch.empty(B * self.heads * T, dtype=torch.float32, device=dev)
        wg = 0
        for l in self.lins:
            wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(l.desc(B if l is self.head else M))))
        dpe = self._pe_desc(B)
        wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(dpe)))
        ws["wg_ws"] = torch.empty(wg, dtype=torch.uint8, device=dev)
        ws["wg_bytes"] = wg
        ws["ln_bytes"] = lib.icamd_layernorm_bwd_workspace_bytes(M, D)
        ws["ln_ws"] = torch.zeros(ws["ln_bytes"], dtype=torch.uint8, device=dev)
        ws["cs_bytes"] = lib.icamd_colsum_rows_workspace_bytes(M, 3 * D if 3 * D > Hd else Hd)
        ws["cs_ws"] = torch.zeros(ws["cs_bytes"], dtype=torch.uint8, device=dev)
        self._ws[B] = ws
        return ws

    def _pe_desc(self, B):
        return patch_embed_desc(self, B, self.dim, self.patch)

    def pack(self, x_nchw, mix=None):
        B, C, H, W = x_nchw.shape
        assert H == self.img_size and W == self.img_size, "ViT position embedding is built for a fixed input size"
        return self._pack_input(self._workspace(B), x_nchw, mix)

    # ------------------------------------------------------------------ forward
    def forward_packed(self, ws, logits_only=False):
        """logits_only: a forward whose activations no backward will read (the reference's second, accuracy-only forward under
        mixup): tensors kept only for the backward pass (the pre-GELU Mlp activations) are not written."""
        f = Forward(self, ws, LN_EPS, logits_only)
        lib, s = self.lib, f.s
        B, M, D, T = ws["B"], ws["M"], self.dim, self.T
        f.linear(self.pe, self._pe_desc(B), ws["x8"].data_ptr(), ws["patches"].data_ptr())
        hip.check(lib.icamd_vit_tokens_fwd(ws["patches"].data_ptr(), self._pf(self.p_cls), self._pf(self.p_pos),
                                           ws["x0"].data_ptr(), B, T, D, s), "tokens")

        def attn_fwd(blk, b):
            hip.check(lib.icamd_attention_fwd(b["qkv"].data_ptr(), b["ao"].data_ptr(), b["lse"].data_ptr(), B, T, self.heads, 64,
                                              SCALE, s), "attention")

        x = ws["x0"]
        for blk, b in zip(self.blocks, ws["blocks"]):
            x = f.block(blk, b, x, M, D, attn_fwd)
        ws["x_last"] = x
        # final LayerNorm only on the class-token rows (the only rows the head reads)
        hip.check(lib.icamd_strided_rows_copy(x.data_ptr(), T * D, ws["cls_rows"].data_ptr(), D, B, D, s), "cls gather")
        f.layernorm(ws["cls_rows"].data_ptr(), self.p_nw, self.p_nb, ws["pooled"].data_ptr(), ws["stf"].data_ptr(), B, D)
        f.linear(self.head, self.head.desc(B), ws["pooled"].data_ptr(), ws["logits"].data_ptr())
        return ws["logits"]

    # ------------------------------------------------------------------ backward
    def backward_packed(self, ws, accumulate=False):
        # the side lane is opt-in for ViT: its main-stream chain is itself MFMA-bound GEMMs + attention, so concurrent
        # weight-gradient GEMMs only compete with it (measured 54.1 -> 54.7 ms/step at batch 256); the CNNs default to on
        lane = side_lane(self, "ICAMD_WGRAD_STREAM_VIT", False)
        bw = Backward(self, ws, lane, accumulate)
        lib, s, acc = self.lib, bw.s, bw.acc
        B, M, D, T = ws["B"], ws["M"], self.dim, self.T
        hook = self.grad_ready_hook

        def attn_bwd(blk, b, dao, dqkv):
            hip.check(lib.icamd_attention_bwd(b["qkv"].data_ptr(), b["ao"].data_ptr(), dao, b["lse"].data_ptr(),
                                              ws["delta"].data_ptr(), dqkv, B, T, self.heads, 64, SCALE, s), "attention bwd")

        g0, g1, g2 = (g.data_ptr() for g in ws["g768"])
        bw.gemm(self.head, self.head.desc(B), ws["pooled"].data_ptr(), ws["dlogits"].data_ptr(), ws["dpooled"].data_ptr())
        bw.layernorm(ws["dpooled"].data_ptr(), ws["cls_rows"].data_ptr(), ws["stf"].data_ptr(), self.p_nw, self.p_nb, None,
                     ws["dcls"].data_ptr(), B, D)
        if hook:
            hook(self.p_nw.offset, self.n_params, lane.events())
        dx = g0
        hip.check(lib.icamd_fill_zero(dx, M * D * 2, s), "zero")
        hip.check(lib.icamd_strided_rows_copy(ws["dcls"].data_ptr(), D, dx, T * D, B, D, s), "cls scatter")
        scratch = (g1, g2, None, ws["g3072b"].data_ptr(), ws["g2304"].data_ptr())
        for blk, b in zip(reversed(self.blocks), reversed(ws["blocks"])):
            bw.block(blk, b, M, D, dx, scratch, attn_bwd)
            if hook:
                hook(blk["n1w"].offset, None, lane.events())
        # tokens -> cls_token, pos_embed, patches
        hip.check(lib.icamd_batch_sum(dx, T * D, B, T * D, self._gf(self.p_pos), acc, s), "pos_embed grad")
        hip.check(lib.icamd_batch_sum(dx, T * D, B, D, self._gf(self.p_cls), acc, s), "cls_token grad")
        dpatch = ws["patches"].data_ptr()   # forward value no longer needed
        hip.check(lib.icamd_strided_rows_copy(dx + 2 * D, T * D, dpatch, (T - 1) * D, B, (T - 1) * D, s), "patch grads")
        bw.gemm(self.pe, self._pe_desc(B), ws["x8"].data_ptr(), dpatch, None)
        lane.join()
        if hook:
            hook(0, None)
