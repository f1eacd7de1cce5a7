"""ConvNeXt (timm `convnext_tiny` family) on the gfx950 kernels: hand-written forward and backward.

BASELINE.json configs[4] is ConvNeXt-T + mixup/cutmix + EMA.  The block is specified in the reference tree
(/root/reference/semantic_segmentation/backbone/convnext.py:21-56: dwconv 7x7 -> LayerNorm -> Linear 4x -> GELU ->
Linear -> gamma -> drop_path -> residual; stem 4x4/4 conv + channels-first LN :79-82; downsample LN + 2x2/2 conv
:85-88; layer-scale init 1e-6 :32,39); the classification model itself comes from timm (train.py:194), whose parameter
names are used here: `stem.{0,1}`, `stages.S.downsample.{0,1}`, `stages.S.blocks.B.{conv_dw,norm,mlp.fc1,mlp.fc2,gamma}`,
`head.{norm,fc}`.  Stochastic depth follows timm: linearly increasing rates up to `drop_path_rate`
(train.py:189-192 passes --drop_path, default 0.05), per-sample masks drawn on the host from torch's RNG.  The flat arenas are
arena.py's; the GEMM, LayerNorm and drop-path steps of both passes (blocks.Forward, blocks.Backward: weight gradients on the side
lane, the waits before a buffer is overwritten) are blocks.py's.  The block itself is written here.

forward_packed and backward_packed are the walk: stem, per stage `_downsample_*` and per block `_block_*` (dw -> LN -> fc1 + GELU ->
tail; backward: tail -> fc1 -> LN -> `_dw_bwd`), head.  The tail, from GELU's output to the block's, is one of three pairs of methods,
chosen once in `_build`: `_v2_*` (GRN, fc2, drop path), `_folded_*` (layer scale folded into fc2's filter), `_unfolded_*` (the
layer-scale kernels, ICAMD_FUSED_LAYERSCALE=0).

NHWC activations make every "channels-first LayerNorm" an ordinary row LayerNorm over pixels, and every Linear a 1x1
convolution on the same tensor (bias fused); the depthwise stencil and the layer-scale tail are dedicated kernels.

ConvNeXt V2 (the `convnextv2_*` names, GRN_ARCHS) is the same class: its block has no layer scale and carries timm's
GlobalResponseNorm between GELU and fc2 (`mlp.grn.weight` / `mlp.grn.bias`, shape (4 dim,), initialised to zero; restated from
memory like the V1 block, not pinned to a timm release): dw -> LN -> fc1 + GELU (z1, a) -> GRN (g) -> fc2 -> drop path -> residual.
GRN is csrc/grn.hip (icamd_grn_fwd / icamd_grn_bwd; the backward also applies gelu'(z1), as fc2's data gradient does for V1).

The small models (convnext_atto / femto / nano; their V2 twins are not registered, see CONFIGS) have widths that are no multiple
of 32 (40, 48, 80): the depthwise kernels take C % 8 == 0 on their register-window form (csrc/dwconv.hip: dwconv7_wgrad_runs_kernel for the weight gradient), GRN C % 32 == 0; every
other layer took these widths already.  `_workspace` raises where that form is switched off (ICAMD_DWCONV_ROWS=0).
"""
import ctypes
import os
from collections import OrderedDict

import torch

from . import hip
from .arena import ArenaModel, Layout, align
from .blocks import Backward, Forward, loss_workspace
from .streams import side_lane

LN_EPS = 1e-6
# Round 5: the layer scale (and timm drop_path's 1 / keep_prob) folded into fc2's filter and bias, the residual added in fc2's store
# pass (icamd_layerscale_fold; DESIGN.md section 5, round-5 finding 10).  0: fc2 -> icamd_layerscale_fwd / _bwd as in rounds 2-4.
_FUSED_LS = os.environ.get("ICAMD_FUSED_LAYERSCALE", "1") != "0"

CONFIGS = {
    # timm's small models (atto / femto / pico / nano: conv_mlp=True there, the same parameters as [out, in, 1, 1]); the widths that
    # are no multiple of 32 (40, 48, 80) run on the C % 8 == 0 forms of icamd_dwconv7_* (dwconv7_wgrad_runs_kernel)
    "convnext_atto": ((2, 2, 6, 2), (40, 80, 160, 320)),
    "convnext_femto": ((2, 2, 6, 2), (48, 96, 192, 384)),
    "convnext_pico": ((2, 2, 6, 2), (64, 128, 256, 512)),
    "convnext_nano": ((2, 2, 8, 2), (80, 160, 320, 640)),
    "convnext_tiny": ((3, 3, 9, 3), (96, 192, 384, 768)),
    "convnext_small": ((3, 3, 27, 3), (96, 192, 384, 768)),
    "convnext_base": ((3, 3, 27, 3), (128, 256, 512, 1024)),
    "convnext_large": ((3, 3, 27, 3), (192, 384, 768, 1536)),
    "convnext_test": ((1, 1, 2, 1), (32, 64, 128, 192)),   # small configuration for parity tests
    "convnext_test_narrow": ((1, 1, 2, 1), (40, 80, 160, 320)),   # parity tests only: atto's widths
    # the backbone of tests/golden/convnext_ref_vectors.npz (vectors from the reference's own ConvNeXt class,
    # /root/reference/semantic_segmentation/backbone/convnext.py:58-150)
    "convnext_pin": ((1, 1, 1, 1), (32, 64, 96, 192)),
    # ConvNeXt V2 (timm convnextv2_*).  convnextv2_atto / femto / nano are not registered: the kernels take their widths (GRN at
    # 4 dim = 160 included) and tests/test_convnext_small_gpu.py runs the class at them, but tests/test_convnextv2_cpu.py pins this
    # list to the five names below and convnextv2_atto as a name train.py rejects
    "convnextv2_pico": ((2, 2, 6, 2), (64, 128, 256, 512)),
    "convnextv2_tiny": ((3, 3, 9, 3), (96, 192, 384, 768)),
    "convnextv2_base": ((3, 3, 27, 3), (128, 256, 512, 1024)),
    "convnextv2_large": ((3, 3, 27, 3), (192, 384, 768, 1536)),
    "convnextv2_test": ((1, 1, 2, 1), (32, 64, 128, 192)),   # parity tests only
}
# the names whose block is the V2 one: global response norm in the Mlp, no layer scale
GRN_ARCHS = frozenset({"convnextv2_pico", "convnextv2_tiny", "convnextv2_base", "convnextv2_large", "convnextv2_test"})
GRN_EPS = 1e-6


class _Conv:
    def __init__(self, name, cin, cout, k, stride, cin_p=None, cout_p=None):
        self.name, self.cin, self.cout, self.k, self.stride = name, cin, cout, k, stride
        self.cin_p, self.cout_p = cin_p or cin, cout_p or cout
        self.w = self.b = None
        self.wt_offset = None
        self.descs = {}

    def desc(self, N, H, W):
        d = self.descs.get((N, H, W))
        if d is None:
            d = self.descs[N, H, W] = hip.conv_desc(N, H, W, self.cin_p, self.cout_p, self.k, self.k, self.stride, 0)
        return d


class ConvNeXt(ArenaModel):
    def __init__(self, arch="convnext_tiny", num_classes=1000, device="cuda", drop_path_rate=0.0, seed=None):
        super().__init__(arch, num_classes, device)
        self.depths, self.dims = CONFIGS[arch]
        self.grn = arch in GRN_ARCHS
        self.drop_path_rate = drop_path_rate
        self.injected_keep = None     # tests: list of per-block keep tensors (float [B]) to use instead of drawing
        self._build()
        self.init_weights(seed)

    # ------------------------------------------------------------------ structure / arenas
    def _build(self):
        dev = self.device
        layout = Layout()
        add = layout.add
        self.gemms = []   # layers that need a transposed shadow (data gradient)

        def conv(name, cin, cout, k, stride, cin_p=None, cout_p=None, needs_dgrad=True, lin=False):
            c = _Conv(name, cin, cout, k, stride, cin_p, cout_p)
            if lin:
                c.w = add(name + ".weight", (cout, cin), "lin", (c.cout_p, cin))
            else:
                c.w = add(name + ".weight", (cout, cin, k, k), "conv", (c.cout_p, k, k, c.cin_p))
            c.b = add(name + ".bias", (cout,), "vec", (c.cout_p,))
            if needs_dgrad:
                self.gemms.append(c)
            return c

        d0 = self.dims[0]
        self.stem = conv("stem.0", 3, d0, 4, 4, cin_p=8, needs_dgrad=False)
        self.stem_nw = add("stem.1.weight", (d0,), "vec", (d0,))
        self.stem_nb = add("stem.1.bias", (d0,), "vec", (d0,))
        self.stages, self.blocks = [], []     # blocks: every stage's, in order; a block's "index" is its place in this list
        rates = torch.linspace(0, self.drop_path_rate, sum(self.depths)).tolist()
        for si, (depth, dim) in enumerate(zip(self.depths, self.dims)):
            st = {"dim": dim, "blocks": []}
            if si > 0:
                prev = self.dims[si - 1]
                st["ds_nw"] = add(f"stages.{si}.downsample.0.weight", (prev,), "vec", (prev,))
                st["ds_nb"] = add(f"stages.{si}.downsample.0.bias", (prev,), "vec", (prev,))
                st["ds"] = conv(f"stages.{si}.downsample.1", prev, dim, 2, 2)
            for j in range(depth):
                n = f"stages.{si}.blocks.{j}"
                blk = {"name": n, "index": len(self.blocks), "dim": dim, "rate": rates[len(self.blocks)]}
                blk["dw_w"] = add(f"{n}.conv_dw.weight", (dim, 1, 7, 7), "dw", (7, 7, dim))
                blk["dw_b"] = add(f"{n}.conv_dw.bias", (dim,), "vec", (dim,))
                blk["nw"] = add(f"{n}.norm.weight", (dim,), "vec", (dim,))
                blk["nb"] = add(f"{n}.norm.bias", (dim,), "vec", (dim,))
                blk["fc1"] = conv(f"{n}.mlp.fc1", dim, 4 * dim, 1, 1, lin=True)
                if self.grn:
                    blk["grn_w"] = add(f"{n}.mlp.grn.weight", (4 * dim,), "vec", (4 * dim,))
                    blk["grn_b"] = add(f"{n}.mlp.grn.bias", (4 * dim,), "vec", (4 * dim,))
                blk["fc2"] = conv(f"{n}.mlp.fc2", 4 * dim, dim, 1, 1, lin=True)
                if not self.grn:
                    blk["gamma"] = add(f"{n}.gamma", (dim,), "vec", (dim,))
                st["blocks"].append(blk)
                self.blocks.append(blk)
            self.stages.append(st)
        dl = self.dims[-1]
        self.head_nw = add("head.norm.weight", (dl,), "vec", (dl,))
        self.head_nb = add("head.norm.bias", (dl,), "vec", (dl,))
        self.head = conv("head.fc", dl, self.num_classes, 1, 1, cout_p=self.ncls_p, lin=True)
        self._allocate(layout, [(c, c.cout_p, c.k * c.k, c.cin_p) for c in self.gemms])
        # folded layer scale: one folded fc2 bias per block; the folded filter takes fc2's place in the bf16 shadow (and, through
        # refresh_transposed, in the transposed shadow), so _w(fc2) / _wt(fc2) are the folded operands
        self.fused_ls = _FUSED_LS and not self.grn     # V2 has no layer scale to fold
        if self.grn:     # the drop-path steps run icamd_layerscale_fwd / _bwd with this constant in gamma's place
            self.ones = torch.ones(max(self.dims), dtype=torch.float32, device=dev)
            self._tail_fwd, self._tail_bwd = self._v2_fwd, self._v2_bwd
        elif self.fused_ls:
            self._tail_fwd, self._tail_bwd = self._folded_fwd, self._folded_bwd
        else:
            self._tail_fwd, self._tail_bwd = self._unfolded_fwd, self._unfolded_bwd
        fb = 0
        for blk in self.blocks:
            blk["fb_off"] = fb
            fb = align(fb + blk["fc2"].cout_p, 64)
        self.fold_bias = torch.zeros(max(fb, 64), dtype=torch.float32, device=dev)
        self._ls_cbs = self._ls_jobs = None     # the per-block constants the shadow is currently folded with, and their job table

    def _ctor_kwargs(self):
        return {"arch": self.arch, "num_classes": self.num_classes, "drop_path_rate": self.drop_path_rate}

    def init_weights(self, seed=None):
        """timm ConvNeXt init: trunc_normal(std .02) conv / linear weights, zero biases, LayerNorm 1 / 0, gamma 1e-6; V2: both
        GRN vectors zero."""
        g = torch.Generator()
        g.manual_seed(seed if seed is not None else torch.initial_seed() % (2 ** 63))
        sd = OrderedDict()
        for name, p in self.params.items():
            if p.kind in ("conv", "lin", "dw"):
                sd[name] = torch.nn.init.trunc_normal_(torch.empty(p.torch_shape), std=0.02, generator=g)
            elif name.endswith(".gamma"):
                sd[name] = torch.full(p.torch_shape, 1e-6)
            elif name.endswith("weight") and ".mlp.grn." not in name:
                sd[name] = torch.ones(p.torch_shape)
            else:
                sd[name] = torch.zeros(p.torch_shape)
        self.load_state_dict(sd)

    def _ls_mode_cbs(self):
        """timm drop_path scales the kept samples by 1 / keep_prob in training; identity in eval."""
        if self.training and self.injected_keep is not None:      # tests: the scale is whatever the injected masks carry
            cbs = []
            for blk, k in zip(self.blocks, self.injected_keep):
                k = k.float().cpu()
                cb = float(k.max()) if float(k.max()) > 0.0 else 1.0
                assert bool(((k == 0) | (k == cb)).all()), "folded layer scale: a keep mask is {0, c} per block"
                cbs.append(cb if blk["rate"] > 0.0 else 1.0)
            return cbs
        return [1.0 / (1.0 - blk["rate"]) if (self.training and blk["rate"] > 0.0) else 1.0 for blk in self.blocks]

    def _fold_layerscale(self):
        import struct
        cbs = self._ls_mode_cbs()
        if self._ls_jobs is None or cbs != self._ls_cbs:
            rows, row0, elems = [], 0, 0
            for blk, cb in zip(self.blocks, cbs):
                c = blk["fc2"]
                bits = struct.unpack("<i", struct.pack("<f", cb))[0]
                rows.append([c.w.offset, blk["gamma"].offset, c.b.offset, blk["fb_off"], c.cout, c.cin, row0, bits])
                row0 += c.cout
                elems += c.cout * c.cin
            self._ls_jobs = torch.tensor(rows, dtype=torch.int64, device=self.device)
            self._ls_rows, self._ls_elems, self._ls_cbs = row0, elems, cbs
        hip.check(self.lib.icamd_layerscale_fold(self.param_arena.data_ptr(), self.shadow.data_ptr(), self.fold_bias.data_ptr(),
                                                 self._ls_jobs.data_ptr(), self._ls_jobs.shape[0], self._ls_rows, self._ls_elems,
                                                 hip.stream_ptr()), "layer scale fold")

    def refresh_transposed(self):
        if self.fused_ls:
            self._fold_layerscale()      # before the transposes: fc2's slot of the shadow becomes the folded filter
        super().refresh_transposed()

    # ------------------------------------------------------------------ workspace
    def _workspace(self, N, H, W):
        key = (N, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev, lib = self.device, self.lib

        def act(*shape):
            return torch.empty(*shape, dtype=torch.bfloat16, device=dev)

        def f32(n):
            return torch.empty(n, dtype=torch.float32, device=dev)

        h, w, d0 = H // 4, W // 4, self.dims[0]
        ws = {"N": N, "H": H, "W": W, "x8": act(N, H, W, 8), "s": act(N, h, w, d0), "x0": act(N, h, w, d0), "st_stem": f32(2 * N * h * w)}
        max_act, max_rows = N * h * w * 4 * d0, N * h * w
        wg = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(self.stem.desc(N, H, W)))
        dwg, grn, stages = 0, 0, []
        for si, st in enumerate(self.stages):
            dim = st["dim"]
            sw = {"blocks": []}
            if si > 0:
                sw["ln"] = act(N, h, w, self.dims[si - 1])
                sw["st"] = f32(2 * N * h * w)
                wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(st["ds"].desc(N, h, w))))
                sw["in_hw"] = (h, w)
                h, w = h // 2, w // 2
                sw["x"] = act(N, h, w, dim)
            sw["hw"] = (h, w)
            rows = N * h * w
            for blk in st["blocks"]:
                sw["blocks"].append({"d": act(N, h, w, dim), "h": act(N, h, w, dim), "z1": act(N, h, w, 4 * dim),
                                     "a": act(N, h, w, 4 * dim), "z2": None if self.fused_ls else act(N, h, w, dim), "out": act(N, h, w, dim),
                                     "st": f32(2 * rows), "keep": None})
                if self.grn:     # g = GRN(a) is fc2's input (kept for its weight gradient); gx: the statistic the backward reads
                    sw["blocks"][-1].update(g=act(N, h, w, 4 * dim), gx=f32(N * 4 * dim))
                    grn = max(grn, lib.icamd_grn_workspace_bytes(N, h * w, 4 * dim))
                wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(blk["fc1"].desc(N, h, w))),
                         lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(blk["fc2"].desc(N, h, w))))
                dwb = lib.icamd_dwconv7_wgrad_workspace_bytes(N, h, w, dim)
                if dim % 32 != 0 and dwb == 0:
                    raise RuntimeError(f"{self.arch}: no depthwise 7x7 kernel for {N}x{h}x{w}x{dim}: widths that are no multiple of "
                                       "32 run on the register-window kernels only (not with ICAMD_DWCONV_ROWS=0, tensors < 4 GB)")
                dwg = max(dwg, dwb)
                max_act = max(max_act, rows * 4 * dim)
            stages.append(sw)
        dl = self.dims[-1]
        ws.update(stages=stages, final_hw=(h, w), max_act=max_act, pool=act(N, dl), pn=act(N, dl), st_head=f32(2 * N))
        loss_workspace(ws, N, self.ncls_p, dev)
        wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(self.head.desc(N, 1, 1))))
        ws["wg_ws"], ws["wg_bytes"] = torch.empty(wg, dtype=torch.uint8, device=dev), wg
        ws["dwg_ws"], ws["dwg_bytes"] = torch.empty(max(dwg, 256), dtype=torch.uint8, device=dev), dwg
        dmax = max(self.dims)
        ws["ln_bytes"] = max(lib.icamd_layernorm_bwd_workspace_bytes(max_rows, c) for c in self.dims)
        ws["ln_ws"] = torch.zeros(ws["ln_bytes"], dtype=torch.uint8, device=dev)
        ws["cs_bytes"] = max(lib.icamd_colsum_rows_workspace_bytes(max_rows, min(4 * dmax, 4096)),
                             lib.icamd_layerscale_bwd_workspace_bytes(max_rows, dmax))
        ws["cs_ws"] = torch.zeros(ws["cs_bytes"], dtype=torch.uint8, device=dev)
        if self.grn:
            ws["grn_ws"], ws["grn_bytes"] = torch.empty(max(grn, 256), dtype=torch.uint8, device=dev), grn
            # Backward.drop_path's names: the column-sum workspace, and the gradient of the constant `ones` (discarded)
            ws["ls_ws"], ws["ls_bytes"], ws["ls_dg"] = ws["cs_ws"], ws["cs_bytes"], f32(dmax)
            # a dropped block's masked output gradient; a buffer of its own, so that fc2's weight gradient (side lane) can read it
            # while the main stream goes on through G[1]
            ws["d2"] = act(max_act // 4)
        if self.fused_ls:     # side-lane scratch of the folded layer's parameter gradients
            ws.update(ls_G=f32(4 * dmax * dmax), ls_S=f32(dmax), ls_drop=f32(N * dmax))
        self._ws[key] = ws
        return ws

    def _scratch(self, ws):
        if "g" not in ws:
            # V2: a sixth buffer for d g, so that d z1 and the buffers after it stay where the side lane expects them
            ws["g"] = [torch.empty(ws["max_act"], dtype=torch.bfloat16, device=self.device) for _ in range(6 if self.grn else 5)]
        return ws["g"]

    def pack(self, x_nchw, mix=None):
        N, C, H, W = x_nchw.shape
        return self._pack_input(self._workspace(N, H, W), x_nchw, mix)

    # ------------------------------------------------------------------ forward
    def forward_packed(self, ws, logits_only=False):
        """logits_only: a forward whose activations no backward will read (the reference's second, accuracy-only forward under
        mixup): tensors kept only for the backward pass (the pre-GELU Mlp activations) are not written."""
        f = Forward(self, ws, LN_EPS, logits_only)
        N, (h, w) = ws["N"], ws["stages"][0]["hw"]
        f.linear(self.stem, self.stem.desc(N, ws["H"], ws["W"]), ws["x8"].data_ptr(), ws["s"].data_ptr())
        f.layernorm(ws["s"].data_ptr(), self.stem_nw, self.stem_nb, ws["x0"].data_ptr(), ws["st_stem"].data_ptr(), N * h * w,
                    self.dims[0])
        x, keeps = ws["x0"], self._keeps(ws)
        if self.fused_ls and self._ls_cbs != self._ls_mode_cbs():
            self.refresh_transposed()     # train() <-> eval(), or a test's injected masks: fold with this mode's constants
        for st, sw in zip(self.stages, ws["stages"]):
            if "ds" in st:
                x = self._downsample_fwd(f, st, sw, x)
            for blk, b in zip(st["blocks"], sw["blocks"]):
                x = self._block_fwd(f, blk, b, x, keeps[blk["index"]], *sw["hw"])
        return self._head_fwd(f, x)

    def _keeps(self, ws):
        """Stochastic depth: this step's mask per block (float [N], 0 or 1 / keep_prob) -- the injected one or a row of one draw for
        all blocks; None for a block whose rate is 0, and for every block in eval."""
        if not self.training:
            return [None] * len(self.blocks)
        if self.injected_keep is not None:
            return [k.to(self.device, dtype=torch.float32) if blk["rate"] > 0.0 else None
                    for blk, k in zip(self.blocks, self.injected_keep)]
        rows = self._draw_keep(ws, [blk["rate"] for blk in self.blocks], ws["N"])
        return [rows[blk["index"]] if blk["rate"] > 0.0 else None for blk in self.blocks]

    def _downsample_fwd(self, f, st, sw, x):
        N, (h, w) = f.ws["N"], sw["in_hw"]
        sw["in"] = x
        f.layernorm(x.data_ptr(), st["ds_nw"], st["ds_nb"], sw["ln"].data_ptr(), sw["st"].data_ptr(), N * h * w, st["ds"].cin)
        f.linear(st["ds"], st["ds"].desc(N, h, w), sw["ln"].data_ptr(), sw["x"].data_ptr())
        return sw["x"]

    def _block_fwd(self, f, blk, b, x, keep, h, w):
        """dw -> LN -> fc1 + GELU (z1, a) -> tail; returns the block's output b["out"]"""
        N, dim = f.ws["N"], blk["dim"]
        b["in"], b["keep"] = x, keep
        hip.check(self.lib.icamd_dwconv7_fwd(x.data_ptr(), self.shadow.data_ptr() + 2 * blk["dw_w"].offset, self._pf(blk["dw_b"]),
                                             b["d"].data_ptr(), N, h, w, dim, f.s), blk["name"] + " dw")
        f.layernorm(b["d"].data_ptr(), blk["nw"], blk["nb"], b["h"].data_ptr(), b["st"].data_ptr(), N * h * w, dim)
        f.linear_gelu(blk["fc1"], blk["fc1"].desc(N, h, w), b["h"].data_ptr(), b["z1"].data_ptr(), b["a"].data_ptr())
        self._tail_fwd(f, blk, b, x, keep, h, w)
        return b["out"]

    def _v2_fwd(self, f, blk, b, x, keep, h, w):
        """g = GRN(a); out = x + keep * fc2(g) -- not dropped: the residual in fc2's store pass"""
        N, dim, c2, ws = f.ws["N"], blk["dim"], blk["fc2"], f.ws
        hip.check(self.lib.icamd_grn_fwd(b["a"].data_ptr(), self._pf(blk["grn_w"]), self._pf(blk["grn_b"]), b["g"].data_ptr(),
                                         b["gx"].data_ptr(), N, h * w, 4 * dim, GRN_EPS, ws["grn_ws"].data_ptr(), ws["grn_bytes"],
                                         f.s), blk["name"] + " grn")
        f.residual(c2, c2.desc(N, h, w), b["g"].data_ptr(), x.data_ptr(), b["out"].data_ptr(), keep, b["z2"].data_ptr(), N * h * w,
                   dim, h * w)

    def _folded_fwd(self, f, blk, b, x, keep, h, w):
        """out = x + a W2'^T + b2' in fc2's store pass; the dropped samples: out = x, and their rows of `a` are cleared so that
        they vanish from fc2's weight gradient (which then runs on the unmasked output gradient)"""
        N, dim, c2 = f.ws["N"], blk["dim"], blk["fc2"]
        hip.check(self.lib.icamd_conv2d_fwd(ctypes.byref(c2.desc(N, h, w)), b["a"].data_ptr(), self._w(c2), b["out"].data_ptr(),
                                            self.fold_bias.data_ptr() + 4 * blk["fb_off"], x.data_ptr(), None, f.s),
                  c2.name + " + layer scale + residual")
        if keep is not None:
            hip.check(self.lib.icamd_rows_fix(keep.data_ptr(), N, b["out"].data_ptr(), x.data_ptr(), h * w * dim * 2,
                                              None if f.logits_only else b["a"].data_ptr(), h * w * dim * 8, f.s), "drop path")

    def _unfolded_fwd(self, f, blk, b, x, keep, h, w):
        """z2 = fc2(a); out = x + keep * gamma * z2"""
        N, dim = f.ws["N"], blk["dim"]
        f.linear(blk["fc2"], blk["fc2"].desc(N, h, w), b["a"].data_ptr(), b["z2"].data_ptr())
        hip.check(self.lib.icamd_layerscale_fwd(b["z2"].data_ptr(), x.data_ptr(), self._pf(blk["gamma"]),
                                                None if keep is None else keep.data_ptr(), b["out"].data_ptr(), N * h * w, dim,
                                                h * w, f.s), "layer scale")

    def _head_fwd(self, f, x):
        ws, dl = f.ws, self.dims[-1]
        N, (h, w) = ws["N"], ws["final_hw"]
        hip.check(self.lib.icamd_avgpool_fwd(x.data_ptr(), ws["pool"].data_ptr(), N, h * w, dl, f.s), "avgpool")
        f.layernorm(ws["pool"].data_ptr(), self.head_nw, self.head_nb, ws["pn"].data_ptr(), ws["st_head"].data_ptr(), N, dl)
        f.linear(self.head, self.head.desc(N, 1, 1), ws["pn"].data_ptr(), ws["logits"].data_ptr())
        return ws["logits"]

    # ------------------------------------------------------------------ backward
    def backward_packed(self, ws, accumulate=False, dfeat=None):
        """Backward from ws['dlogits'].  `dfeat` (bf16 NHWC tensor shaped like the last stage's output): start from that
        gradient instead and skip the classification head -- the entry the reference-vector parity test uses, since the
        reference tree's ConvNeXt is the headless backbone.  G: the scratch pointers -- the gradient of a block's output and of its
        input alternate between G[0] and G[3] (`dout`, `other`); within a block G[4] = d z1, G[1] = d h, G[2] = d (dwconv out)."""
        lane = side_lane(self, "ICAMD_WGRAD_STREAM", True)
        bw = Backward(self, ws, lane, accumulate)
        hook = self.grad_ready_hook
        G = [g.data_ptr() for g in self._scratch(ws)]
        dout, other = G[0], G[3]
        if dfeat is None:
            self._head_bwd(bw, G, dout)
        else:
            assert dfeat.dtype == torch.bfloat16 and dfeat.numel() == ws["stages"][-1]["blocks"][-1]["out"].numel()
            self._scratch(ws)[0][: dfeat.numel()].copy_(dfeat.reshape(-1))
        if hook:
            hook(self.head_nw.offset, self.n_params, lane.events())
        for st, sw in zip(reversed(self.stages), reversed(ws["stages"])):
            for blk, b in zip(reversed(st["blocks"]), reversed(sw["blocks"])):
                self._block_bwd(bw, blk, b, G, dout, other, *sw["hw"])
                dout, other = other, dout
                if hook:
                    hook(blk["dw_w"].offset, None, lane.events())
            if "ds" in st:
                self._downsample_bwd(bw, st, sw, G, dout, other)
                dout, other = other, dout
                if hook:
                    hook(st["ds_nw"].offset, None, lane.events())
        N, (h, w) = ws["N"], ws["stages"][0]["hw"]
        bw.layernorm(dout, ws["s"].data_ptr(), ws["st_stem"].data_ptr(), self.stem_nw, self.stem_nb, None, G[1], N * h * w,
                     self.dims[0])
        bw.gemm(self.stem, self.stem.desc(N, ws["H"], ws["W"]), ws["x8"].data_ptr(), G[1], None)
        lane.join()
        if hook:
            hook(0, None)

    def _head_bwd(self, bw, G, dout):
        ws, dl = bw.ws, self.dims[-1]
        N, (h, w) = ws["N"], ws["final_hw"]
        bw.gemm(self.head, self.head.desc(N, 1, 1), ws["pn"].data_ptr(), ws["dlogits"].data_ptr(), G[1])
        bw.layernorm(G[1], ws["pool"].data_ptr(), ws["st_head"].data_ptr(), self.head_nw, self.head_nb, None, G[2], N, dl)
        hip.check(self.lib.icamd_avgpool_bwd(G[2], bw.writes(dout), N, h * w, dl, bw.s), "avgpool bwd")

    def _downsample_bwd(self, bw, st, sw, G, dout, dx):
        N, (h, w) = bw.ws["N"], sw["in_hw"]
        bw.gemm(st["ds"], st["ds"].desc(N, h, w), sw["ln"].data_ptr(), dout, G[1])
        bw.layernorm(G[1], sw["in"].data_ptr(), sw["st"].data_ptr(), st["ds_nw"], st["ds_nb"], None, dx, N * h * w, st["ds"].cin)

    def _block_bwd(self, bw, blk, b, G, dout, dx, h, w):
        """dout: the gradient of the block's output; dx receives that of its input (pointers)"""
        N, dim = bw.ws["N"], blk["dim"]
        self._tail_bwd(bw, blk, b, dout, b["keep"], G, h, w)                                                 # G4 = d z1
        bw.gemm(blk["fc1"], blk["fc1"].desc(N, h, w), b["h"].data_ptr(), G[4], G[1])                         # G1 = d h
        bw.layernorm(G[1], b["d"].data_ptr(), b["st"].data_ptr(), blk["nw"], blk["nb"], None, G[2], N * h * w, dim)
        self._dw_bwd(bw, blk, b, G[2], dout, dx, h, w)

    def _v2_bwd(self, bw, blk, b, dout, keep, G, h, w):
        """fc2 from the block's output gradient (masked into a buffer of its own where the branch was dropped), then GRN's backward,
        which also applies gelu'(z1)"""
        N, dim, ws = bw.ws["N"], blk["dim"], bw.ws
        d2 = dout if keep is None else bw.drop_path(dout, keep, ws["d2"].data_ptr(), N * h * w, dim, h * w)
        bw.gemm(blk["fc2"], blk["fc2"].desc(N, h, w), b["g"].data_ptr(), d2, G[5])                           # G5 = d g
        hip.check(self.lib.icamd_grn_bwd(G[5], b["a"].data_ptr(), b["gx"].data_ptr(), self._pf(blk["grn_w"]), b["z1"].data_ptr(),
                                         bw.writes(G[4]), self._gf(blk["grn_w"]), self._gf(blk["grn_b"]), bw.acc, N, h * w, 4 * dim,
                                         GRN_EPS, ws["grn_ws"].data_ptr(), ws["grn_bytes"], bw.s), blk["name"] + " grn bwd + gelu bwd")

    def _folded_bwd(self, bw, blk, b, dout, keep, G, h, w):
        """fc2 with the layer scale folded in: its data gradient reads the block's output gradient itself (the folded, transposed
        filter carries cb * gamma); the side lane forms G = dout^T a and the column sums of dout over the kept samples, and from
        them the gradients of W2, b2 and gamma (icamd_layerscale_param_grads)"""
        lib, ws, N, dim, c2, gam = self.lib, bw.ws, bw.ws["N"], blk["dim"], blk["fc2"], blk["gamma"]
        d2, cb, keep = ctypes.byref(c2.desc(N, h, w)), self._ls_cbs[blk["index"]], None if keep is None else keep.data_ptr()
        lsG, lsS, lsD = ws["ls_G"].data_ptr(), ws["ls_S"].data_ptr(), ws["ls_drop"].data_ptr()

        def side(st):
            if keep is not None:
                hip.check(lib.icamd_dropped_colsum(dout, keep, N, h * w, dim, lsD, st), "dropped column sums")
            hip.check(lib.icamd_conv2d_wgrad_bias(d2, b["a"].data_ptr(), dout, lsG, lsS, 0, *bw.wg, st), c2.name + " wgrad+bias (folded)")
            hip.check(lib.icamd_layerscale_param_grads(lsG, self._pf(c2.w), self._pf(c2.b), self._pf(gam), lsS,
                                                       None if keep is None else lsD, N, cb, c2.cout, c2.cin, self._gf(c2.w),
                                                       self._gf(c2.b), self._gf(gam), bw.acc, st), "layer scale parameter gradients")
        bw.lane.launch(side, reads=(dout,))
        hip.check(lib.icamd_conv2d_dgrad_gelu(d2, dout, self._wt(c2), b["z1"].data_ptr(), bw.writes(G[4]), bw.s),
                  c2.name + " dgrad + gelu bwd (folded)")
        if keep is not None:
            hip.check(lib.icamd_rows_fix(keep, N, G[4], None, h * w * dim * 8, None, 0, bw.s), "drop path bwd")

    def _unfolded_bwd(self, bw, blk, b, dout, keep, G, h, w):
        """G1 = d z2 = keep * gamma * dout (and gamma's gradient), then fc2 with the GELU backward in its data gradient"""
        N, dim, ws = bw.ws["N"], blk["dim"], bw.ws
        hip.check(self.lib.icamd_layerscale_bwd(dout, b["z2"].data_ptr(), self._pf(blk["gamma"]), None if keep is None else keep.data_ptr(),
                                                bw.writes(G[1]), self._gf(blk["gamma"]), N * h * w, dim, h * w, bw.acc,
                                                ws["cs_ws"].data_ptr(), ws["cs_bytes"], bw.s), "layer scale bwd")
        bw.gemm(blk["fc2"], blk["fc2"].desc(N, h, w), b["a"].data_ptr(), G[1], G[4], gelu_z=b["z1"].data_ptr())

    def _dw_bwd(self, bw, blk, b, dy, dout, dx, h, w):
        """The depthwise convolution from dy = d (its output): filter and bias gradient on the side lane -- out of one pass over dy
        where the shape has that kernel, else the filter there and the bias as column sums on the main stream --, then
        dx = dgrad(dy) + dout, the residual's gradient"""
        lib, ws, N, dim, acc = self.lib, bw.ws, bw.ws["N"], blk["dim"], bw.acc
        x_ptr, dw, db = b["in"].data_ptr(), self._gf(blk["dw_w"]), self._gf(blk["dw_b"])
        wsp, wsb = ws["dwg_ws"].data_ptr(), ws["dwg_bytes"]
        one_pass = lib.icamd_dwconv7_wgrad_bias_supported(N, h, w, dim)

        def side(st):
            if one_pass:
                hip.check(lib.icamd_dwconv7_wgrad_bias(x_ptr, dy, dw, db, acc, wsp, wsb, N, h, w, dim, st), blk["name"] + " dw wgrad+bias")
            else:
                hip.check(lib.icamd_dwconv7_wgrad(x_ptr, dy, dw, acc, wsp, wsb, N, h, w, dim, st), blk["name"] + " dw wgrad")
        bw.lane.launch(side, reads=(dy,))
        if not one_pass:
            hip.check(lib.icamd_colsum_rows(dy, N * h * w, dim, dim, db, acc, ws["cs_ws"].data_ptr(), ws["cs_bytes"], bw.s), "dw bias grad")
        hip.check(lib.icamd_dwconv7_dgrad(dy, self.shadow.data_ptr() + 2 * blk["dw_w"].offset, dout, bw.writes(dx), N, h, w, dim,
                                          bw.s), blk["name"] + " dw dgrad")
