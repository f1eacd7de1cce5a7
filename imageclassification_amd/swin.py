"""Swin Transformer (timm `swin_*_patch4_window7_224` and `swin_base_patch4_window12_384`) on the gfx950 kernels: hand-written
forward and backward.

The reference builds every model with timm.create_model(args.model) (/root/reference/train.py:194).  Architecture restated from
the published source (timm is absent; parity is against oracle/swin_ref.py, "timm-unpinned" like ViT and ResNet here):
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
vit.py (bias, GELU and the residual add fused in the epilogue).  The flat arenas are arena.py's; the block and the GEMM / LayerNorm
steps are blocks.py's, shared with vit.py: this file supplies the window attention launches (with the relative-position scatter),
patch merging, the bias arena and the loop over stages.  There is no side stream: the lane handed to blocks.Backward is never
enabled.  Stochastic depth
is timm's (rates rising linearly to `drop_path_rate`, one per-sample mask per residual branch, drawn on the host by
ArenaModel._draw_keep and applied by the block's keep1 / keep2 path with icamd_layerscale_fwd / _bwd and a vector of ones); with rate 0
the residual rides in the GEMM epilogue.
"""
import ctypes
from collections import OrderedDict

import torch

from . import hip, streams
from .arena import ArenaModel, Layout, Lin, align
from .blocks import Backward, Forward, block_params, block_workspace, lin_builder, loss_workspace, patch_embed_desc

LN_EPS = 1e-5
HEAD_DIM = 32
SCALE = HEAD_DIM ** -0.5      # of the attention scores

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
        param = lambda name, *shape: P[name]        # everything is laid out already
        lin = lin_builder(self.lins, param)
        self.pe = Lin("patch_embed.proj", 8, self.embed)      # the patch-embedding convolution; its descriptor is _pe_desc's
        self.pe.w, self.pe.b = P["patch_embed.proj.weight"], P["patch_embed.proj.bias"]
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
                blk = block_params(n, dim, 4 * dim, param, lin)
                blk.update(rate=rates[bi], shift=shift if j % 2 else 0, bias_off=boff,
                           table=P[f"{n}.attn.relative_position_bias_table"])
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
                sw["blocks"].append(block_workspace(dev, M, dim, 4 * dim, nwin * H * wsz * wsz))
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
        loss_workspace(ws, B, self.ncls_p, dev)
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
        """backward scratch, made at the first backward: four [rows][C], one [rows][3C], two [rows][4C] at the largest stage;
        returns the pointers of the four, of the [rows][3C] and of the first [rows][4C]"""
        if "g" not in ws:
            n = ws["max_mc"]
            e = lambda k: torch.empty(k * n, dtype=torch.bfloat16, device=self.device)
            ws["g"] = [e(1), e(1), e(1), e(1)]
            ws["g3"] = e(3)
            ws["g4"] = [e(4), e(4)]
        return [g.data_ptr() for g in ws["g"]], ws["g3"].data_ptr(), ws["g4"][0].data_ptr()

    def _pe_desc(self, B):
        return patch_embed_desc(self, B, self.embed, PATCH)

    def _branch_tmp(self, ws):
        """forward scratch of a dropped fc2 branch, made at the first step that drops one"""
        t = ws.get("branch_tmp")
        if t is None:
            t = ws["branch_tmp"] = torch.empty(ws["max_mc"], dtype=torch.bfloat16, device=self.device)
        return t

    def _bias(self, blk):
        return self.bias_arena.data_ptr() + 4 * blk["bias_off"]

    def pack(self, x_nchw, mix=None):
        B, C, H, W = x_nchw.shape
        if H != self.img_size or W != self.img_size:
            raise ValueError(f"this model's window plan is built for {self.img_size}x{self.img_size} inputs, not {H}x{W}")
        return self._pack_input(self._workspace(B), x_nchw, mix)

    # ------------------------------------------------------------------ forward
    def forward_packed(self, ws, logits_only=False):
        """logits_only: a forward whose activations no backward will read (the reference's second, accuracy-only forward under
        mixup): the pre-GELU Mlp activations are not written."""
        f = Forward(self, ws, LN_EPS, logits_only)
        lib, s = self.lib, f.s
        B = ws["B"]
        f.linear(self.pe, self._pe_desc(B), ws["x8"].data_ptr(), ws["s"].data_ptr())
        M0 = ws["stages"][0]["M"]
        f.layernorm(ws["s"].data_ptr(), self.pe_nw, self.pe_nb, ws["x0"].data_ptr(), ws["st_stem"].data_ptr(), M0, self.embed)
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
                f.linear(st["ds"], st["ds"].desc(M), sw["ln"].data_ptr(), sw["x"].data_ptr())
                x = sw["x"]

            def attn_fwd(blk, b):
                hip.check(lib.icamd_window_attention_fwd(b["qkv"].data_ptr(), self._bias(blk), b["ao"].data_ptr(),
                                                         b["lse"].data_ptr(), B, res, res, H, HEAD_DIM, wsz, blk["shift"], SCALE,
                                                         s), blk["name"] + " window attention")

            for blk, b in zip(st["blocks"], sw["blocks"]):
                keep1 = keep2 = None
                if self.training and blk["rate"] > 0.0:
                    if self.injected_keep is not None:
                        keep1 = self.injected_keep[2 * bi].to(self.device, dtype=torch.float32)
                        keep2 = self.injected_keep[2 * bi + 1].to(self.device, dtype=torch.float32)
                    else:
                        keep1, keep2 = drop_rows[2 * bi], drop_rows[2 * bi + 1]
                x = f.block(blk, b, x, M, dim, attn_fwd, keep1, keep2, res * res)
                bi += 1
        ws["x_last"] = x
        sl = ws["stages"][-1]
        ML, DL = sl["M"], self.last_dim
        f.layernorm(x.data_ptr(), self.p_nw, self.p_nb, ws["normed"].data_ptr(), ws["st_f"].data_ptr(), ML, DL)
        hip.check(lib.icamd_avgpool_fwd(ws["normed"].data_ptr(), ws["pooled"].data_ptr(), B, ML // B, DL, s), "avgpool")
        f.linear(self.head, self.head.desc(B), ws["pooled"].data_ptr(), ws["logits"].data_ptr())
        return ws["logits"]

    # ------------------------------------------------------------------ backward
    def backward_packed(self, ws, accumulate=False):
        (g0, g1, g2, g3), gq, gz = self._scratch(ws)
        # Swin has no second stream: its lane is never enabled, so every weight gradient stays on the main stream
        bw = Backward(self, ws, streams.SideLane(self.device, enabled=False), accumulate)
        lib, s, acc = self.lib, bw.s, bw.acc
        B = ws["B"]
        hook = self.grad_ready_hook
        sl = ws["stages"][-1]
        ML, DL = sl["M"], self.last_dim
        bw.gemm(self.head, self.head.desc(B), ws["pooled"].data_ptr(), ws["dlogits"].data_ptr(), g1)       # d pooled
        hip.check(lib.icamd_avgpool_bwd(g1, g2, B, ML // B, DL, s), "avgpool bwd")
        bw.layernorm(g2, ws["x_last"].data_ptr(), ws["st_f"].data_ptr(), self.p_nw, self.p_nb, None, g0, ML, DL)
        if hook:
            hook(self.p_nw.offset, self.n_params, ())
        dx, free = g0, [g1, g2, g3]
        for i in range(len(self.stages) - 1, -1, -1):
            st, sw = self.stages[i], ws["stages"][i]
            dim, res, wsz, H, M = st["dim"], st["res"], st["ws"], st["heads"], sw["M"]

            def attn_bwd(blk, b, dao, dqkv):
                hip.check(lib.icamd_window_attention_bwd(b["qkv"].data_ptr(), self._bias(blk), b["ao"].data_ptr(), dao,
                                                         b["lse"].data_ptr(), dqkv, ws["dbias"].data_ptr(), 0,
                                                         ws["wa_ws"].data_ptr(), ws["wa_bytes"], B, res, res, H, HEAD_DIM, wsz,
                                                         blk["shift"], SCALE, s), blk["name"] + " window attention bwd")
                hip.check(lib.icamd_relpos_bias_scatter(ws["dbias"].data_ptr(), self._gf(blk["table"]), H, wsz, acc, s),
                          blk["name"] + " bias table grad")

            for blk, b in zip(reversed(st["blocks"]), reversed(sw["blocks"])):
                bw.block(blk, b, M, dim, dx, (*free, gz, gq), attn_bwd, res * res)
                if hook:
                    hook(blk["n1w"].offset, None, ())
            if i > 0:
                t0, t1, t2 = free
                bw.gemm(st["ds"], st["ds"].desc(M), sw["ln"].data_ptr(), dx, gq)                            # d LayerNorm(4 C_prev)
                hip.check(lib.icamd_patch_merge_ln_bwd(gq, sw["in"].data_ptr(), sw["st"].data_ptr(),
                                                       sw["st"].data_ptr() + 4 * M, self._pf(st["ds_nw"]), t0,
                                                       self._gf(st["ds_nw"]), self._gf(st["ds_nb"]), B, 2 * res, 2 * res, dim // 2,
                                                       acc, ws["pm_ws"].data_ptr(), ws["pm_bytes"], s), "patch merging bwd")
                dx, free = t0, [dx, t1, t2]
                if hook:
                    hook(st["ds_nw"].offset, None, ())
        M0 = ws["stages"][0]["M"]
        t0 = free[0]
        bw.layernorm(dx, ws["s"].data_ptr(), ws["st_stem"].data_ptr(), self.pe_nw, self.pe_nb, None, t0, M0, self.embed)
        bw.gemm(self.pe, self._pe_desc(B), ws["x8"].data_ptr(), t0, None)
        if hook:
            hook(0, None)
