"""Swin Transformer (timm `swin_*_patch4_window7_224` and `swin_base_patch4_window12_384`) on the gfx950 kernels: hand-written
forward and backward.

The reference builds every model with timm.create_model(args.model) (/root/reference/train.py:194).  Architecture restated from
the published source (timm is absent; parity is against tests/_swin_ref.py, "timm-unpinned" like ViT and ResNet here):
4x4/4 patch-embedding conv + bias and a LayerNorm, four stages of pre-LayerNorm blocks (eps 1e-5) whose attention runs inside
7x7 (or 12x12: CONFIGS_W12) windows with 32-wide heads, a learned relative-position bias and, in every second block, a cyclic
shift by half the window with its region mask; stage i > 0 opens with patch merging (2x2 gather -> LayerNorm(4C) -> bias-free Linear 4C -> 2C, current timm's placement);
final LayerNorm, mean over tokens, linear head.  Parameter names follow timm: `patch_embed.{proj,norm}.*`,
`layers.I.downsample.{norm,reduction}.*`, `layers.I.blocks.J.{norm1,attn.relative_position_bias_table,attn.qkv,attn.proj,norm2,
mlp.fc1,mlp.fc2}.*`, `norm.*`, `head.fc.*`.  The relative-position index and the attention mask are not state: the kernels compute
them (csrc/window_attention.hip), and `window_geometry` / `relative_position_index` below are the host-side statement of the same
rules.

Tokens stay in their natural [B][H][W][C] order through the whole network: the window kernels do the roll, the partition and their
inverses as address arithmetic, so every Linear is the 1x1 case of the convolution kernels on a [rows, 1, 1, C] "image" exactly as in
vit.py (bias, GELU and the residual add fused in the epilogue).  The flat arenas are arena.py's.  Stochastic depth
is timm's (rates rising linearly to `drop_path_rate`, one per-sample mask per residual branch, drawn on the host by
ArenaModel._draw_keep and applied with icamd_layerscale_fwd / _bwd and a vector of ones); with rate 0 the residual rides in the GEMM epilogue.
"""
import ctypes
from collections import OrderedDict

import torch

from . import hip
from .arena import ArenaModel, Layout, Lin, align

LN_EPS = 1e-5
HEAD_DIM = 32

CONFIGS = {
    # name: (embed dim, depths, heads, window)
    "swin_tiny_patch4_window7_224": (96, (2, 2, 6, 2), (3, 6, 12, 24), 7),
    "swin_small_patch4_window7_224": (96, (2, 2, 18, 2), (3, 6, 12, 24), 7),
    "swin_base_patch4_window7_224": (128, (2, 2, 18, 2), (4, 8, 16, 32), 7),
    "swin_test": (32, (2, 2), (1, 2), 7),   # small configuration for parity tests (56^2 input: 14^2 then 7^2 tokens)
}
# the window-12 models, fine-tuned at 384 x 384 in the paper (a table of their own: CONFIGS is what the window-7 tests enumerate)
CONFIGS_W12 = {
    "swin_base_patch4_window12_384": (128, (2, 2, 18, 2), (4, 8, 16, 32), 12),
    "swin_test_w12": (32, (2, 2), (1, 2), 12),   # parity tests (96^2 input: 24^2 then 12^2 tokens; 192^2: 48^2 then 24^2)
}
# names that carry their input size are built at that size when none is given (every other name: 224)
NATIVE_SIZE = {"swin_base_patch4_window12_384": 384}
PATCH = 4


def config(arch):
    """(embed dim, depths, heads, window) of a name of either table; KeyError for any other"""
    return CONFIGS[arch] if arch in CONFIGS else CONFIGS_W12[arch]


def native_size(arch):
    return NATIVE_SIZE.get(arch, 224)


# ---------------------------------------------------------------------------------------------------- host-side geometry (no GPU)
def window_geometry(Hs, Ws, ws, shift):
    """For every token of an [Hs][Ws] grid, in natural order: the number of its window, its slot in the window and its mask
    region id (int64 tensors of Hs * Ws entries), for windows of side `ws` on the grid rolled by (-shift, -shift).  Window numbers
    and slots are those of timm's window_partition of the rolled tensor; the region ids those of its img_mask (per axis the slices
    [0, L - ws), [L - ws, L - shift), [L - shift, L) of the ROLLED grid, id = 3 * row slice + column slice; all zero without a shift)."""
    if Hs % ws or Ws % ws or not 0 <= shift < ws:
        raise ValueError(f"window {ws} / shift {shift} does not tile a {Hs} x {Ws} grid")
    r = torch.arange(Hs).view(-1, 1).expand(Hs, Ws)
    c = torch.arange(Ws).view(1, -1).expand(Hs, Ws)
    rr, rc = (r - shift) % Hs, (c - shift) % Ws          # where the token sits after the roll
    win = (rr // ws) * (Ws // ws) + rc // ws
    slot = (rr % ws) * ws + rc % ws
    if shift > 0:
        def sl(x, L):
            return (x >= L - ws).long() + (x >= L - shift).long()
        region = 3 * sl(rr, Hs) + sl(rc, Ws)
    else:
        region = torch.zeros(Hs, Ws, dtype=torch.int64)
    return win.reshape(-1).long(), slot.reshape(-1).long(), region.reshape(-1).long()


def relative_position_index(ws):
    """timm's relative_position_index: [ws^2][ws^2] int64, (dr + ws - 1) * (2 ws - 1) + (dc + ws - 1) with (dr, dc) the coordinates
    of token i minus those of token j."""
    i = torch.arange(ws * ws)
    r, c = i // ws, i % ws
    dr = r.view(-1, 1) - r.view(1, -1)
    dc = c.view(-1, 1) - c.view(1, -1)
    return ((dr + ws - 1) * (2 * ws - 1) + dc + ws - 1).long()


def stage_plan(arch, img_size=None):
    """[(tokens per side, window, shift of the odd blocks)] per stage; raises ValueError for an input size the windows do not tile.
    img_size None: the name's own size."""
    embed, depths, heads, window = config(arch)
    if img_size is None:
        img_size = native_size(arch)
    if img_size < PATCH or img_size % PATCH:
        raise ValueError(f"img_size {img_size} is not a positive multiple of the patch size {PATCH}")
    res = img_size // PATCH
    plan = []
    for i in range(len(depths)):
        if i > 0:
            if res % 2:
                raise ValueError(f"{arch} at {img_size}x{img_size}: stage {i - 1} has {res} tokens per side, which patch merging "
                                 "cannot halve")
            res //= 2
        if res <= window:
            plan.append((res, res, 0))
        elif res % window == 0:
            plan.append((res, window, window // 2))
        else:
            raise ValueError(f"{arch} at {img_size}x{img_size}: every stage's resolution must be a multiple of the window, or <= the "
                             f"window; stage {i} has {res} tokens per side and the window is {window} " +
                             ("(224 and 448 work, 384 does not)" if window == 7 else "(192 and 384 work, 224 does not)"))
        if plan[-1][1] < 2:
            raise ValueError(f"{arch} at {img_size}x{img_size}: stage {i} has a single token")
    return plan


def _param_list(arch, num_classes, img_size=None):
    """(name, torch shape, kind) of every parameter, in timm's order."""
    embed, depths, heads, _ = config(arch)
    plan = stage_plan(arch, img_size)
    out = [("patch_embed.proj.weight", (embed, 3, PATCH, PATCH), "conv"), ("patch_embed.proj.bias", (embed,), "vec"),
           ("patch_embed.norm.weight", (embed,), "vec"), ("patch_embed.norm.bias", (embed,), "vec")]
    for i, depth in enumerate(depths):
        dim = embed << i
        if i > 0:
            prev = dim // 2
            out += [(f"layers.{i}.downsample.norm.weight", (4 * prev,), "vec"), (f"layers.{i}.downsample.norm.bias", (4 * prev,), "vec"),
                    (f"layers.{i}.downsample.reduction.weight", (dim, 4 * prev), "lin")]
        ws = plan[i][1]
        for j in range(depth):
            n = f"layers.{i}.blocks.{j}"
            out += [(f"{n}.norm1.weight", (dim,), "vec"), (f"{n}.norm1.bias", (dim,), "vec"),
                    (f"{n}.attn.relative_position_bias_table", ((2 * ws - 1) ** 2, heads[i]), "vec"),
                    (f"{n}.attn.qkv.weight", (3 * dim, dim), "lin"), (f"{n}.attn.qkv.bias", (3 * dim,), "vec"),
                    (f"{n}.attn.proj.weight", (dim, dim), "lin"), (f"{n}.attn.proj.bias", (dim,), "vec"),
                    (f"{n}.norm2.weight", (dim,), "vec"), (f"{n}.norm2.bias", (dim,), "vec"),
                    (f"{n}.mlp.fc1.weight", (4 * dim, dim), "lin"), (f"{n}.mlp.fc1.bias", (4 * dim,), "vec"),
                    (f"{n}.mlp.fc2.weight", (dim, 4 * dim), "lin"), (f"{n}.mlp.fc2.bias", (dim,), "vec")]
    last = embed << (len(depths) - 1)
    out += [("norm.weight", (last,), "vec"), ("norm.bias", (last,), "vec"),
            ("head.fc.weight", (num_classes, last), "lin"), ("head.fc.bias", (num_classes,), "vec")]
    return out


def param_shapes(arch, num_classes=1000, img_size=None):
    """OrderedDict name -> shape of every parameter (what state_dict() holds), without a GPU."""
    return OrderedDict((n, tuple(s)) for n, s, _ in _param_list(arch, num_classes, img_size))


class SwinTransformer(ArenaModel):
    def __init__(self, arch="swin_tiny_patch4_window7_224", num_classes=1000, device="cuda", img_size=None, drop_path_rate=0.1,
                 seed=None):
        self.plan = stage_plan(arch, img_size)          # before anything touches the GPU: a bad size is a ValueError everywhere
        super().__init__(arch, num_classes, device)
        self.embed, self.depths, self.heads, self.window = config(arch)
        self.img_size = native_size(arch) if img_size is None else img_size
        self.drop_path_rate = drop_path_rate
        self.injected_keep = None     # tests: list of per-branch keep tensors (float [B], two per block) used instead of drawing
        self._build()
        self.init_weights(seed)

    # ------------------------------------------------------------------ structure / arenas
    def _build(self):
        dev = self.device
        layout = Layout()
        for name, shape, kind in _param_list(self.arch, self.num_classes, self.img_size):
            if kind == "conv":
                layout.add(name, shape, kind, (shape[0], PATCH, PATCH, 8))
            elif name.startswith("head.fc."):
                layout.add(name, shape, kind, (self.ncls_p,) + tuple(shape[1:]))
            else:
                layout.add(name, shape, kind)
        P = layout.params
        self.lins = []

        def lin(name, cin, cout, cout_p=None, bias=True):
            l = Lin(name, cin, cout, cout_p)
            l.w = P[name + ".weight"]
            l.b = P[name + ".bias"] if bias else None
            self.lins.append(l)
            return l

        self.pe_w, self.pe_b = P["patch_embed.proj.weight"], P["patch_embed.proj.bias"]
        self.pe_nw, self.pe_nb = P["patch_embed.norm.weight"], P["patch_embed.norm.bias"]
        self.stages = []
        nblocks = sum(self.depths)
        rates = torch.linspace(0, self.drop_path_rate, nblocks).tolist()
        bi, boff = 0, 0
        for i, depth in enumerate(self.depths):
            dim = self.embed << i
            res, ws, shift = self.plan[i]
            st = {"dim": dim, "res": res, "ws": ws, "heads": self.heads[i], "blocks": []}
            if dim // self.heads[i] != HEAD_DIM:
                raise ValueError("the window attention kernel is built for a head dimension of 32")
            if i > 0:
                prev = dim // 2
                st["ds_nw"], st["ds_nb"] = P[f"layers.{i}.downsample.norm.weight"], P[f"layers.{i}.downsample.norm.bias"]
                st["ds"] = lin(f"layers.{i}.downsample.reduction", 4 * prev, dim, bias=False)
            for j in range(depth):
                n = f"layers.{i}.blocks.{j}"
                blk = {"name": n, "rate": rates[bi], "shift": shift if j % 2 else 0, "bias_off": boff}
                blk["n1w"], blk["n1b"] = P[f"{n}.norm1.weight"], P[f"{n}.norm1.bias"]
                blk["table"] = P[f"{n}.attn.relative_position_bias_table"]
                blk["qkv"] = lin(f"{n}.attn.qkv", dim, 3 * dim)
                blk["proj"] = lin(f"{n}.attn.proj", dim, dim)
                blk["n2w"], blk["n2b"] = P[f"{n}.norm2.weight"], P[f"{n}.norm2.bias"]
                blk["fc1"] = lin(f"{n}.mlp.fc1", dim, 4 * dim)
                blk["fc2"] = lin(f"{n}.mlp.fc2", 4 * dim, dim)
                st["blocks"].append(blk)
                boff = align(boff + self.heads[i] * ws ** 4, 64)
                bi += 1
            self.stages.append(st)
        self.last_dim = self.embed << (len(self.depths) - 1)
        self.p_nw, self.p_nb = P["norm.weight"], P["norm.bias"]
        self.head = lin("head.fc", self.last_dim, self.num_classes, self.ncls_p)
        self._allocate(layout, [(l, l.cout_p, 1, l.cin) for l in self.lins])
        # the gathered relative-position bias of every block, fp32 [heads][ws^2][ws^2]: refreshed with the transposed shadow,
        # i.e. after every load and every optimizer step -- the only places the tables move
        self.bias_arena = torch.zeros(max(boff, 64), dtype=torch.float32, device=dev)
        self.ones = torch.ones(max(st["dim"] for st in self.stages), dtype=torch.float32, device=dev)

    def _ctor_kwargs(self):
        return {"arch": self.arch, "num_classes": self.num_classes, "img_size": self.img_size,
                "drop_path_rate": self.drop_path_rate}

    def init_weights(self, seed=None):
        """timm's Swin init: trunc_normal(std .02) Linear weights and bias tables, zero biases, LayerNorm 1 / 0; the patch-embedding
        conv keeps torch's Conv2d default (Kaiming-uniform, a = sqrt(5))."""
        g = torch.Generator()
        g.manual_seed(seed if seed is not None else torch.initial_seed() % (2 ** 63))
        sd = OrderedDict()
        bound = 1.0 / (3 * PATCH * PATCH) ** 0.5
        for name, p in self.params.items():
            if name.startswith("patch_embed.proj"):
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) * bound
            elif p.kind == "lin" or name.endswith("relative_position_bias_table"):
                sd[name] = torch.nn.init.trunc_normal_(torch.empty(p.torch_shape), std=0.02, generator=g)
            elif name.endswith("weight"):        # the LayerNorms
                sd[name] = torch.ones(p.torch_shape)
            else:
                sd[name] = torch.zeros(p.torch_shape)
        self.load_state_dict(sd)

    def refresh_transposed(self):
        """What follows every change of the parameters (load, optimizer step): the transposed bf16 filters of the data gradients
        and the relative-position bias of every block, gathered from its table."""
        super().refresh_transposed()
        s = hip.stream_ptr()
        for st in self.stages:
            for blk in st["blocks"]:
                hip.check(self.lib.icamd_relpos_bias_gather(self._pf(blk["table"]), self._bias(blk), st["heads"], st["ws"], s),
                          blk["name"] + " bias gather")

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is not None:
            return ws
        dev, lib = self.device, self.lib

        def act(r, c):
            return torch.empty(r, c, dtype=torch.bfloat16, device=dev)

        def f32(n):
            return torch.empty(n, dtype=torch.float32, device=dev)

        ws = {"B": B}
        ws["x8"] = torch.empty(B, self.img_size, self.img_size, 8, dtype=torch.bfloat16, device=dev)
        r0 = self.plan[0][0]
        M0 = B * r0 * r0
        ws["s"] = act(M0, self.embed)
        ws["x0"] = act(M0, self.embed)
        ws["st_stem"] = f32(2 * M0)
        wg = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(self._pe_desc(B)))
        wa, pm, max_mc = 0, 256, M0 * self.embed
        stages = []
        for i, st in enumerate(self.stages):
            dim, res, wsz, H = st["dim"], st["res"], st["ws"], st["heads"]
            M = B * res * res
            sw = {"M": M, "blocks": []}
            if i > 0:
                sw["ln"] = act(M, 2 * dim)                 # LayerNorm(gathered 4 C_prev) = 2 * dim channels
                sw["st"] = f32(2 * M)
                sw["x"] = act(M, dim)
                wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(st["ds"].desc(M))))
                pm = max(pm, lib.icamd_patch_merge_ln_bwd_workspace_bytes(B, 2 * res, 2 * res, dim // 2))
            nwin = B * (res // wsz) ** 2
            for blk in st["blocks"]:
                sw["blocks"].append({"h": act(M, dim), "qkv": act(M, 3 * dim), "ao": act(M, dim), "x1": act(M, dim),
                                     "h2": act(M, dim), "z": act(M, 4 * dim), "a": act(M, 4 * dim), "x2": act(M, dim),
                                     "lse": f32(nwin * H * wsz * wsz), "st1": f32(2 * M), "st2": f32(2 * M),
                                     "keep1": None, "keep2": None})
                for l in (blk["qkv"], blk["proj"], blk["fc1"], blk["fc2"]):
                    wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(l.desc(M))))
            wa = max(wa, lib.icamd_window_attention_bwd_workspace_bytes(B, res, res, H, wsz))
            max_mc = max(max_mc, M * dim)
            stages.append(sw)
        ws["stages"] = stages
        ML = stages[-1]["M"]
        ws["normed"] = act(ML, self.last_dim)
        ws["st_f"] = f32(2 * ML)
        ws["pooled"] = act(B, self.last_dim)
        ws["logits"] = torch.zeros(B, self.ncls_p, dtype=torch.bfloat16, device=dev)
        ws["dlogits"] = torch.zeros(B, self.ncls_p, dtype=torch.bfloat16, device=dev)
        ws["loss_rows"] = f32(B)
        ws["pred"] = torch.empty(B, dtype=torch.int32, device=dev)
        wg = max(wg, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(self.head.desc(B))))
        ws["wg_ws"] = torch.empty(wg, dtype=torch.uint8, device=dev)
        ws["wg_bytes"] = wg
        ws["wa_ws"] = torch.empty(max(wa, 256), dtype=torch.uint8, device=dev)
        ws["wa_bytes"] = wa
        ws["pm_ws"] = torch.empty(pm, dtype=torch.uint8, device=dev)
        ws["pm_bytes"] = pm
        ws["dbias"] = f32(max(st["heads"] * st["ws"] ** 4 for st in self.stages))
        dims = [st["dim"] for st in self.stages]
        max_rows = max(sw["M"] for sw in stages)
        ws["ln_bytes"] = max(lib.icamd_layernorm_bwd_workspace_bytes(max_rows, c) for c in dims)
        ws["ln_ws"] = torch.zeros(ws["ln_bytes"], dtype=torch.uint8, device=dev)
        ws["ls_bytes"] = max(lib.icamd_layerscale_bwd_workspace_bytes(max_rows, c) for c in dims)
        ws["ls_ws"] = torch.zeros(max(ws["ls_bytes"], 256), dtype=torch.uint8, device=dev)
        ws["ls_dg"] = f32(max(dims))
        ws["max_mc"] = max_mc
        self._ws[B] = ws
        return ws

    def _scratch(self, ws):
        """backward scratch, made at the first backward: four [rows][C], one [rows][3C], two [rows][4C] at the largest stage"""
        if "g" not in ws:
            n = ws["max_mc"]
            e = lambda k: torch.empty(k * n, dtype=torch.bfloat16, device=self.device)
            ws["g"] = [e(1), e(1), e(1), e(1)]
            ws["g3"] = e(3)
            ws["g4"] = [e(4), e(4)]
        return ws["g"], ws["g3"], ws["g4"]

    def _pe_desc(self, B):
        key = ("pe", B)
        d = self._ws.get(key)
        if d is None:
            d = hip.conv_desc(B, self.img_size, self.img_size, 8, self.embed, PATCH, PATCH, PATCH, 0)
            self._ws[key] = d
        return d

    # ------------------------------------------------------------------ helpers
    def _bias(self, blk):
        return self.bias_arena.data_ptr() + 4 * blk["bias_off"]

    def pack(self, x_nchw, mix=None):
        B, C, H, W = x_nchw.shape
        if H != self.img_size or W != self.img_size:
            raise ValueError(f"this model's window plan is built for {self.img_size}x{self.img_size} inputs, not {H}x{W}")
        return self._pack_input(self._workspace(B), x_nchw, mix)

    def _linear(self, l, x_ptr, y_ptr, rows, addend_ptr, s):
        hip.check(self.lib.icamd_conv2d_fwd(ctypes.byref(l.desc(rows)), x_ptr, self._w(l), y_ptr,
                                            None if l.b is None else self._pf(l.b), addend_ptr, None, s), l.name)

    def _ln(self, x_ptr, wp, bp, y_ptr, st, rows, C, s):
        hip.check(self.lib.icamd_layernorm_fwd(x_ptr, self._pf(wp), self._pf(bp), y_ptr, st.data_ptr(), st.data_ptr() + 4 * rows,
                                               rows, C, LN_EPS, s), wp.name)

    # ------------------------------------------------------------------ forward
    def forward_packed(self, ws, logits_only=False):
        """logits_only: a forward whose activations no backward will read (the reference's second, accuracy-only forward under
        mixup): the pre-GELU Mlp activations are not written."""
        lib, s = self.lib, hip.stream_ptr()
        B = ws["B"]
        scale = HEAD_DIM ** -0.5
        hip.check(lib.icamd_conv2d_fwd(ctypes.byref(self._pe_desc(B)), ws["x8"].data_ptr(),
                                       self.shadow.data_ptr() + 2 * self.pe_w.offset, ws["s"].data_ptr(), self._pf(self.pe_b),
                                       None, None, s), "patch_embed")
        M0 = ws["stages"][0]["M"]
        self._ln(ws["s"].data_ptr(), self.pe_nw, self.pe_nb, ws["x0"].data_ptr(), ws["st_stem"], M0, self.embed, s)
        x = ws["x0"]
        drop_rows = None
        if self.training and self.injected_keep is None:
            # one per-sample mask per residual branch: two per block
            drop_rows = self._draw_keep(ws, [blk["rate"] for st in self.stages for blk in st["blocks"] for _ in (0, 1)], B)
        bi = 0
        for i, (st, sw) in enumerate(zip(self.stages, ws["stages"])):
            dim, res, wsz, H, M = st["dim"], st["res"], st["ws"], st["heads"], sw["M"]
            if i > 0:
                sw["in"] = x
                hip.check(lib.icamd_patch_merge_ln_fwd(x.data_ptr(), self._pf(st["ds_nw"]), self._pf(st["ds_nb"]),
                                                       sw["ln"].data_ptr(), sw["st"].data_ptr(), sw["st"].data_ptr() + 4 * M, B,
                                                       2 * res, 2 * res, dim // 2, LN_EPS, s), "patch merging")
                self._linear(st["ds"], sw["ln"].data_ptr(), sw["x"].data_ptr(), M, None, s)
                x = sw["x"]
            tok = res * res
            for blk, b in zip(st["blocks"], sw["blocks"]):
                keep1 = keep2 = None
                if self.training and blk["rate"] > 0.0:
                    if self.injected_keep is not None:
                        keep1 = self.injected_keep[2 * bi].to(self.device, dtype=torch.float32)
                        keep2 = self.injected_keep[2 * bi + 1].to(self.device, dtype=torch.float32)
                    else:
                        keep1, keep2 = drop_rows[2 * bi], drop_rows[2 * bi + 1]
                b["keep1"], b["keep2"], b["x"] = keep1, keep2, x
                self._ln(x.data_ptr(), blk["n1w"], blk["n1b"], b["h"].data_ptr(), b["st1"], M, dim, s)
                self._linear(blk["qkv"], b["h"].data_ptr(), b["qkv"].data_ptr(), M, None, s)
                hip.check(lib.icamd_window_attention_fwd(b["qkv"].data_ptr(), self._bias(blk), b["ao"].data_ptr(),
                                                         b["lse"].data_ptr(), B, res, res, H, HEAD_DIM, wsz, blk["shift"], scale,
                                                         s), blk["name"] + " window attention")
                if keep1 is None:
                    self._linear(blk["proj"], b["ao"].data_ptr(), b["x1"].data_ptr(), M, x.data_ptr(), s)   # x1 = x + proj(attn)
                else:     # x1 = x + keep * proj(attn); the branch passes through h2's buffer (LayerNorm 2 overwrites it next)
                    self._linear(blk["proj"], b["ao"].data_ptr(), b["h2"].data_ptr(), M, None, s)
                    hip.check(lib.icamd_layerscale_fwd(b["h2"].data_ptr(), x.data_ptr(), self.ones.data_ptr(), keep1.data_ptr(),
                                                       b["x1"].data_ptr(), M, dim, tok, s), "drop path")
                self._ln(b["x1"].data_ptr(), blk["n2w"], blk["n2b"], b["h2"].data_ptr(), b["st2"], M, dim, s)
                l1 = blk["fc1"]                                                   # z = fc1(h2), a = gelu(z): one kernel
                hip.check(lib.icamd_conv2d_fwd_gelu(ctypes.byref(l1.desc(M)), b["h2"].data_ptr(), self._w(l1),
                                                    None if logits_only else b["z"].data_ptr(), b["a"].data_ptr(), self._pf(l1.b),
                                                    s), l1.name + " + gelu")
                if keep2 is None:
                    self._linear(blk["fc2"], b["a"].data_ptr(), b["x2"].data_ptr(), M, b["x1"].data_ptr(), s)   # x2 = x1 + mlp
                else:     # x2 = x1 + keep * mlp; every buffer of the block is still needed by the backward: a scratch of its own
                    t = self._branch_tmp(ws)
                    self._linear(blk["fc2"], b["a"].data_ptr(), t.data_ptr(), M, None, s)
                    hip.check(lib.icamd_layerscale_fwd(t.data_ptr(), b["x1"].data_ptr(), self.ones.data_ptr(), keep2.data_ptr(),
                                                       b["x2"].data_ptr(), M, dim, tok, s), "drop path")
                x = b["x2"]
                bi += 1
        ws["x_last"] = x
        sl = ws["stages"][-1]
        ML, DL = sl["M"], self.last_dim
        self._ln(x.data_ptr(), self.p_nw, self.p_nb, ws["normed"].data_ptr(), ws["st_f"], ML, DL, s)
        hip.check(lib.icamd_avgpool_fwd(ws["normed"].data_ptr(), ws["pooled"].data_ptr(), B, ML // B, DL, s), "avgpool")
        self._linear(self.head, ws["pooled"].data_ptr(), ws["logits"].data_ptr(), B, None, s)
        return ws["logits"]

    def _branch_tmp(self, ws):
        t = ws.get("branch_tmp")
        if t is None:
            t = ws["branch_tmp"] = torch.empty(ws["max_mc"], dtype=torch.bfloat16, device=self.device)
        return t

    # ------------------------------------------------------------------ backward
    def backward_packed(self, ws, accumulate=False):
        lib, s = self.lib, hip.stream_ptr()
        B = ws["B"]
        acc = int(bool(accumulate))
        hook = self.grad_ready_hook
        wsp, wsb = ws["wg_ws"].data_ptr(), ws["wg_bytes"]
        lnp, lnb = ws["ln_ws"].data_ptr(), ws["ln_bytes"]
        scale = HEAD_DIM ** -0.5
        (g0, g1, g2, g3), gq, (gz, _) = self._scratch(ws)

        def lin_bwd(l, x_ptr, dy_ptr, rows, dx_ptr, gelu_z=None):
            """weight, bias gradients (+ data gradient into dx when given) of y = x W^T + b"""
            d = l.desc(rows)
            if l.b is None:
                hip.check(lib.icamd_conv2d_wgrad(ctypes.byref(d), x_ptr, dy_ptr, self._gf(l.w), acc, wsp, wsb, s), l.name + " wgrad")
            else:
                hip.check(lib.icamd_conv2d_wgrad_bias(ctypes.byref(d), x_ptr, dy_ptr, self._gf(l.w), self._gf(l.b), acc, wsp, wsb,
                                                      s), l.name + " wgrad+bias")
            if dx_ptr is None:
                return
            if gelu_z is None:
                hip.check(lib.icamd_conv2d_dgrad(ctypes.byref(d), dy_ptr, self._wt(l), dx_ptr, None, None, s), l.name + " dgrad")
            else:   # dx = (dy W) * gelu'(z): the GELU backward rides in the data-gradient kernel's store pass
                hip.check(lib.icamd_conv2d_dgrad_gelu(ctypes.byref(d), dy_ptr, self._wt(l), gelu_z, dx_ptr, s),
                          l.name + " dgrad + gelu bwd")

        def ln_bwd(dy_ptr, x_ptr, st, wp, bp, addend_ptr, dx_ptr, rows, C):
            hip.check(lib.icamd_layernorm_bwd(dy_ptr, x_ptr, st.data_ptr(), st.data_ptr() + 4 * rows, self._pf(wp), addend_ptr,
                                              dx_ptr, self._gf(wp), self._gf(bp), rows, C, acc, lnp, lnb, s), wp.name + " bwd")

        def drop_bwd(dout_ptr, keep, dz_ptr, rows, C, tok):
            """gradient of the dropped branch: dz = dout * keep (the entry's dgamma goes to a scratch vector)"""
            hip.check(lib.icamd_layerscale_bwd(dout_ptr, dout_ptr, self.ones.data_ptr(), keep.data_ptr(), dz_ptr,
                                               ws["ls_dg"].data_ptr(), rows, C, tok, 0, ws["ls_ws"].data_ptr(), ws["ls_bytes"], s),
                      "drop path bwd")

        sl = ws["stages"][-1]
        ML, DL = sl["M"], self.last_dim
        dpooled = g1.data_ptr()
        lin_bwd(self.head, ws["pooled"].data_ptr(), ws["dlogits"].data_ptr(), B, dpooled)
        hip.check(lib.icamd_avgpool_bwd(dpooled, g2.data_ptr(), B, ML // B, DL, s), "avgpool bwd")
        ln_bwd(g2.data_ptr(), ws["x_last"].data_ptr(), ws["st_f"], self.p_nw, self.p_nb, None, g0.data_ptr(), ML, DL)
        if hook:
            hook(self.p_nw.offset, self.n_params, ())
        dx, free = g0, [g1, g2, g3]
        for i in range(len(self.stages) - 1, -1, -1):
            st, sw = self.stages[i], ws["stages"][i]
            dim, res, wsz, H, M = st["dim"], st["res"], st["ws"], st["heads"], sw["M"]
            tok = res * res
            for blk, b in zip(reversed(st["blocks"]), reversed(sw["blocks"])):
                t0, t1, t2 = free
                # dx = gradient of x2 = x1 + keep2 * fc2(a)
                d2 = dx.data_ptr()
                if b["keep2"] is not None:
                    drop_bwd(dx.data_ptr(), b["keep2"], t2.data_ptr(), M, dim, tok)
                    d2 = t2.data_ptr()
                lin_bwd(blk["fc2"], b["a"].data_ptr(), d2, M, gz.data_ptr(), gelu_z=b["z"].data_ptr())        # d z
                lin_bwd(blk["fc1"], b["h2"].data_ptr(), gz.data_ptr(), M, t0.data_ptr())                       # d h2
                ln_bwd(t0.data_ptr(), b["x1"].data_ptr(), b["st2"], blk["n2w"], blk["n2b"], dx.data_ptr(), t1.data_ptr(), M, dim)
                dx1 = t1                                                                                       # = LN2'(dh2) + dx
                d1 = dx1.data_ptr()
                if b["keep1"] is not None:
                    drop_bwd(dx1.data_ptr(), b["keep1"], t2.data_ptr(), M, dim, tok)
                    d1 = t2.data_ptr()
                lin_bwd(blk["proj"], b["ao"].data_ptr(), d1, M, t0.data_ptr())                                 # d attention out
                hip.check(lib.icamd_window_attention_bwd(b["qkv"].data_ptr(), self._bias(blk), b["ao"].data_ptr(), t0.data_ptr(),
                                                         b["lse"].data_ptr(), gq.data_ptr(), ws["dbias"].data_ptr(), 0,
                                                         ws["wa_ws"].data_ptr(), ws["wa_bytes"], B, res, res, H, HEAD_DIM, wsz,
                                                         blk["shift"], scale, s), blk["name"] + " window attention bwd")
                hip.check(lib.icamd_relpos_bias_scatter(ws["dbias"].data_ptr(), self._gf(blk["table"]), H, wsz, acc, s),
                          blk["name"] + " bias table grad")
                lin_bwd(blk["qkv"], b["h"].data_ptr(), gq.data_ptr(), M, t0.data_ptr())                        # d h
                ln_bwd(t0.data_ptr(), b["x"].data_ptr(), b["st1"], blk["n1w"], blk["n1b"], dx1.data_ptr(), dx.data_ptr(), M, dim)
                if hook:
                    hook(blk["n1w"].offset, None, ())
            if i > 0:
                t0, t1, t2 = free
                lin_bwd(st["ds"], sw["ln"].data_ptr(), dx.data_ptr(), M, gq.data_ptr())                        # d LayerNorm(4 C_prev)
                hip.check(lib.icamd_patch_merge_ln_bwd(gq.data_ptr(), sw["in"].data_ptr(), sw["st"].data_ptr(),
                                                       sw["st"].data_ptr() + 4 * M, self._pf(st["ds_nw"]), t0.data_ptr(),
                                                       self._gf(st["ds_nw"]), self._gf(st["ds_nb"]), B, 2 * res, 2 * res, dim // 2,
                                                       acc, ws["pm_ws"].data_ptr(), ws["pm_bytes"], s), "patch merging bwd")
                dx, free = t0, [dx, t1, t2]
                if hook:
                    hook(st["ds_nw"].offset, None, ())
        M0 = ws["stages"][0]["M"]
        t0 = free[0]
        ln_bwd(dx.data_ptr(), ws["s"].data_ptr(), ws["st_stem"], self.pe_nw, self.pe_nb, None, t0.data_ptr(), M0, self.embed)
        dpe = self._pe_desc(B)
        hip.check(lib.icamd_conv2d_wgrad_bias(ctypes.byref(dpe), ws["x8"].data_ptr(), t0.data_ptr(), self._gf(self.pe_w),
                                              self._gf(self.pe_b), acc, wsp, wsb, s), "patch_embed wgrad+bias")
        if hook:
            hook(0, None)
