"""EfficientNet-B0 / B1 on the HIP kernels: timm's `efficientnet_b0` / `efficientnet_b1` (MBConv blocks with squeeze-and-excitation,
depthwise 3x3 and 5x5, SiLU; symmetric padding k // 2, BatchNorm eps 1e-5 / momentum 0.1 -- not the `tf_` variants), restated.

    conv_stem 3x3/2 -> bn1 + SiLU
    blocks.0.B   depthwise-separable: conv_dw 3x3 -> bn1 + SiLU -> se -> conv_pw 1x1 -> bn2 (+ input when in = out: B1's blocks.0.1)
    blocks.S.B   inverted residual:   conv_pw 1x1 (in -> 6 in) -> bn1 + SiLU -> conv_dw k x k / s -> bn2 + SiLU -> se -> conv_pwl 1x1
                 -> bn3 (+ input when s = 1 and in = out)
    se           gate = sigmoid(conv_expand(silu(conv_reduce(mean_hw(a))))), a the ACTIVATED depthwise output; the reduced width is a
                 quarter of the block's INPUT width; the projection convolution reads a * gate
    conv_head 1x1 -> bn2 + SiLU -> global average pool -> classifier

No dropout and no stochastic depth (timm's defaults for the family; the reference passes --drop_path elsewhere only).

What is stored per block: y1 (raw conv_pw output), y2 (raw depthwise output), the GATED projection input bf16(a2 * gate), y3 and the
block output, plus the [N, C]-sized fp32 arrays of the excitation (s, hpre, gate).  The ungated a2 = silu(bn2(y2)) is never stored:
icamd_bn_silu_squeeze sums it, icamd_bn_apply_silu writes it gated, and the backward recomputes it (and silu') from y2.  The expanded
a1 = silu(bn1(y1)) goes through the model's one scratch buffer in front of the depthwise call and is recomputed for the weight
gradient, as MobileNetV2's plain route does (profiles/mobilenetv2.txt measured the on-load form slower; it is not built for 5x5).

Launches of an inverted-residual block.  Forward: conv_pw, finalize, apply_silu (a1), depthwise, finalize, squeeze, excite, gated
apply, conv_pwl, finalize, apply (+ input).  Backward: bn3 backward, conv_pwl weight + data gradient, gate-gradient reduce, excite
backward, bn2 + SiLU backward (reduce, finalize, apply), depthwise data gradient, apply_silu (a1 again), depthwise weight gradient,
bn1 + SiLU backward, conv_pw weight + data gradient.  One stream; eval walks the same graph with icamd_bn_eval_coeffs' scale / shift.
"""
import ctypes
import math
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import hip
from .bnmodel import _BN, _Conv, BatchNormModel

# (kernel, first stride, out channels, repeats) of stages 1..6; name -> (stem, (stage 0 out, repeats), stages, head)
_B0 = ((3, 2, 24, 2), (5, 2, 40, 2), (3, 2, 80, 3), (5, 1, 112, 3), (5, 2, 192, 4), (3, 1, 320, 1))


def _scaled(depth):
    return tuple((k, s, c, int(math.ceil(depth * n))) for k, s, c, n in _B0)


CONFIGS = {"efficientnet_b0": (32, (16, 1), _scaled(1.0), 1280), "efficientnet_b1": (32, (16, 2), _scaled(1.1), 1280)}
# parity-test member: one block of every kind -- the depthwise-separable one, 3x3 and 5x5 at stride 2, stride-1 blocks with the skip
CONFIGS["efficientnet_test"] = (16, (8, 1), ((3, 2, 16, 2), (5, 2, 24, 1), (5, 1, 32, 2)), 64)


def block_plan(arch):
    """(stem width, [(name, kind, kernel, in, mid, out, stride, rd)], head width); kind "ds" (mid = in) or "ir" (mid = 6 in); rd, the
    reduced width of the block's squeeze-and-excitation, is a quarter of the block INPUT width"""
    stem, (first, first_n), stages, head = CONFIGS[arch]
    blocks, cin = [], stem
    for bi in range(first_n):
        blocks.append((f"blocks.0.{bi}", "ds", 3, cin, cin, first, 1, max(1, cin // 4)))
        cin = first
    for si, (k, stride, out, repeats) in enumerate(stages, 1):
        for bi in range(repeats):
            blocks.append((f"blocks.{si}.{bi}", "ir", k, cin, cin * 6, out, stride if bi == 0 else 1, max(1, cin // 4)))
            cin = out
    return stem, blocks, head


def se_shapes(name, c, rd):
    return [(name + ".conv_reduce.weight", (rd, c, 1, 1)), (name + ".conv_reduce.bias", (rd,)),
            (name + ".conv_expand.weight", (c, rd, 1, 1)), (name + ".conv_expand.bias", (c,))]


def param_shapes(arch, num_classes=1000):
    """[(name, torch shape)] in timm's module order (parameters only)"""
    stem, blocks, head = block_plan(arch)
    bn = lambda n, c: [(n + ".weight", (c,)), (n + ".bias", (c,))]     # noqa: E731
    out = [("conv_stem.weight", (stem, 3, 3, 3))] + bn("bn1", stem)
    for name, kind, k, cin, mid, cout, _, rd in blocks:
        if kind == "ds":
            out += [(name + ".conv_dw.weight", (cin, 1, k, k))] + bn(name + ".bn1", cin) + se_shapes(name + ".se", cin, rd)
            out += [(name + ".conv_pw.weight", (cout, cin, 1, 1))] + bn(name + ".bn2", cout)
        else:
            out += [(name + ".conv_pw.weight", (mid, cin, 1, 1))] + bn(name + ".bn1", mid)
            out += [(name + ".conv_dw.weight", (mid, 1, k, k))] + bn(name + ".bn2", mid) + se_shapes(name + ".se", mid, rd)
            out += [(name + ".conv_pwl.weight", (cout, mid, 1, 1))] + bn(name + ".bn3", cout)
    out += [("conv_head.weight", (head, blocks[-1][5], 1, 1))] + bn("bn2", head)
    return out + [("classifier.weight", (num_classes, head)), ("classifier.bias", (num_classes,))]


class _DW:
    """Depthwise k x k record: filter [k][k][C] in the arena (kind "dw")."""

    def __init__(self, name, c, k, stride):
        self.name, self.c, self.k, self.stride = name, c, k, stride
        self.w = None


class _SE:
    """Squeeze-and-excitation record: conv_reduce [rd][C] + bias, conv_expand [C][rd] + bias, fp32 in the parameter arena in torch
    layout; the excite kernels read the fp32 masters (the bf16 shadow slice is written by the optimizer and read by nothing)."""

    def __init__(self, name, c, rd):
        self.name, self.c, self.rd = name, c, rd
        self.w1 = self.b1 = self.w2 = self.b2 = None


class EfficientNet(BatchNormModel):
    """HIP EfficientNet. `model(x)` runs the forward and returns bf16 logits [B, num_classes] (a view)."""

    def __init__(self, arch="efficientnet_b0", num_classes=1000, device="cuda", seed=None):
        super().__init__(arch, num_classes, device)
        self._build()
        self.init_weights(seed=seed)

    # ------------------------------------------------------------------ structure
    def _build(self):
        stem, plan, head = block_plan(self.arch)
        self.bns, self.convs = [], []
        order = []          # records in module order

        def conv(name, cin, cout, k=1, stride=1, pad=0, cin_p=None, cout_p=None, bias=False):
            c = _Conv(name, cin, cout, k, stride, pad, cin_p, cout_p, bias)
            self.convs.append(c)
            order.append(c)
            return c

        def bn(name, c):
            b = _BN(name, c)
            self.bns.append(b)
            order.append(b)
            return b

        def dw(name, c, k, stride):
            d = _DW(name, c, k, stride)
            order.append(d)
            return d

        def se(name, c, rd):
            m = _SE(name, c, rd)
            order.append(m)
            return m

        self.stem_conv = conv("conv_stem", 3, stem, 3, 2, 1, cin_p=8)
        self.stem_bn = bn("bn1", stem)
        self.blocks = []
        for name, kind, k, cin, mid, cout, stride, rd in plan:
            blk = SimpleNamespace(name=name, kind=kind, cin=cin, mid=mid, cout=cout, stride=stride,
                                  residual=stride == 1 and cin == cout)
            if kind == "ds":
                blk.dw, blk.bn_dw = dw(name + ".conv_dw", cin, k, stride), bn(name + ".bn1", cin)
                blk.se = se(name + ".se", cin, rd)
                blk.pwl, blk.bn_out = conv(name + ".conv_pw", cin, cout), bn(name + ".bn2", cout)
            else:
                blk.pw, blk.bn_pw = conv(name + ".conv_pw", cin, mid), bn(name + ".bn1", mid)
                blk.dw, blk.bn_dw = dw(name + ".conv_dw", mid, k, stride), bn(name + ".bn2", mid)
                blk.se = se(name + ".se", mid, rd)
                blk.pwl, blk.bn_out = conv(name + ".conv_pwl", mid, cout), bn(name + ".bn3", cout)
            self.blocks.append(blk)
        self.head_conv = conv("conv_head", plan[-1][5], head)
        self.head_bn = bn("bn2", head)
        self.feat_dim = head
        self.fc = conv("classifier", head, self.num_classes, cout_p=self.ncls_p, bias=True)
        self.bn_width = max(b.c for b in self.bns)
        # transposed filters for the data gradients of every pointwise convolution and the classifier (the stem needs none)
        self._layout_arenas(order, [(m, m.cout_p, 1, m.cin_p) for m in self.convs if m is not self.stem_conv])

    def _add_record(self, add, m):
        """The two kinds of record of its own: a depthwise filter, tap-major in the arena, and a squeeze-and-excitation module."""
        if isinstance(m, _DW):
            m.w = add(m.name + ".weight", (m.c, 1, m.k, m.k), "dw", (m.k, m.k, m.c))
            return
        (n1, s1), (nb1, sb1), (n2, s2), (nb2, sb2) = se_shapes(m.name, m.c, m.rd)
        m.w1 = add(n1, s1, "conv", (m.rd, 1, 1, m.c))     # [rd][1][1][C] is torch's (rd, C, 1, 1) memory
        m.b1 = add(nb1, sb1, "vec", sb1)
        m.w2 = add(n2, s2, "conv", (m.c, 1, 1, m.rd))
        m.b2 = add(nb2, sb2, "vec", sb2)

    # ------------------------------------------------------------------ parameters
    def init_weights(self, seed=None):
        """timm's _init_weight_goog: convolutions (those of the squeeze-and-excitation included) N(0, sqrt(2 / fan_out)) with fan_out =
        k k Cout / groups and zero bias, BatchNorm 1 / 0, classifier weight U(+-1 / sqrt(num_classes)) and bias 0."""
        g = torch.Generator()
        g.manual_seed(seed if seed is not None else torch.initial_seed() % (2 ** 63))
        sd = OrderedDict()
        for name, p in self.params.items():
            if p.kind == "conv":
                cout, _, k, _ = p.torch_shape
                sd[name] = torch.randn(p.torch_shape, generator=g) * math.sqrt(2.0 / (k * k * cout))
            elif p.kind == "dw":
                k = p.torch_shape[-1]
                sd[name] = torch.randn(p.torch_shape, generator=g) * math.sqrt(2.0 / (k * k))
            elif name == "classifier.weight":
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) / math.sqrt(self.num_classes)
            elif name.endswith(".weight"):
                sd[name] = torch.ones(p.torch_shape)
            else:
                sd[name] = torch.zeros(p.torch_shape)
        self._fresh_buffers(sd)
        self.load_state_dict(sd)

    # ------------------------------------------------------------------ workspaces
    def _dw_entries(self, dw):
        """(supported, stats_rows, wgrad_workspace_bytes) of the depthwise kernels of this filter size"""
        lib = self.lib
        if dw.k == 3:
            return lib.icamd_dwconv3_supported, lib.icamd_dwconv3_stats_rows, lib.icamd_dwconv3_wgrad_workspace_bytes
        return lib.icamd_dwconv5_supported, lib.icamd_dwconv5_stats_rows, lib.icamd_dwconv5_wgrad_workspace_bytes

    def _workspace(self, N, H, W):
        key = (N, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev, lib = self.device, self.lib
        ws = {"N": N, "H": H, "W": W}
        sizes = SimpleNamespace(act=0, stats=0, wgrad=0, bnb=0, se=0, nc=0)

        def act(h, w, c):
            sizes.act = max(sizes.act, N * h * w * c)
            return torch.empty(N, h, w, c, dtype=torch.bfloat16, device=dev)

        def conv_out(conv, h, w):
            d = conv.desc(N, h, w)
            sizes.stats = max(sizes.stats, lib.icamd_conv2d_stats_rows(ctypes.byref(d)) * 2 * conv.cout_p)
            sizes.wgrad = max(sizes.wgrad, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
            sizes.bnb = max(sizes.bnb, lib.icamd_bn_bwd_workspace_bytes(N * d.OH * d.OW, conv.cout_p))
            return act(d.OH, d.OW, conv.cout_p), d.OH, d.OW

        def dw_out(dw, h, w):
            supported, stats_rows, wgrad_bytes = self._dw_entries(dw)
            if not supported(N, h, w, dw.c, dw.stride):
                raise hip.IcamdError(f"{dw.name}: no depthwise {dw.k}x{dw.k} kernel for {(N, h, w, dw.c)} at stride {dw.stride}")
            oh, ow = (h - 1) // dw.stride + 1, (w - 1) // dw.stride + 1
            sizes.stats = max(sizes.stats, stats_rows(N, h, w, dw.c, dw.stride) * 2 * dw.c)
            sizes.wgrad = max(sizes.wgrad, wgrad_bytes(N, h, w, dw.c, dw.stride))
            sizes.bnb = max(sizes.bnb, lib.icamd_bn_bwd_workspace_bytes(N * oh * ow, dw.c))
            return act(oh, ow, dw.c), oh, ow

        ws["x8"] = act(H, W, 8)
        ws["y0"], h, w = conv_out(self.stem_conv, H, W)
        ws["stem_hw"] = (h, w)
        blocks_ws = []
        for bi, blk in enumerate(self.blocks):
            b = {"in_hw": (h, w)}
            if blk.kind == "ir":
                b["y1"], h, w = conv_out(blk.pw, h, w)
            b["dw_hw"] = (h, w)
            b["y2"], h, w = dw_out(blk.dw, h, w)
            b["a2"] = act(h, w, blk.dw.c)          # the gated projection input
            se = blk.se
            for key_, width in (("se_asum", se.c), ("se_s", se.c), ("se_h", se.rd), ("se_e", se.c)):
                b[key_] = torch.empty(N, width, dtype=torch.float32, device=dev)
            sizes.se = max(sizes.se, lib.icamd_bn_silu_squeeze_workspace_bytes(N, h * w, se.c),
                           lib.icamd_se_silu_bwd_reduce_workspace_bytes(N, h * w, se.c))
            sizes.nc = max(sizes.nc, N * se.c)
            b["y3"], h, w = conv_out(blk.pwl, h, w)
            b["out"] = act(h, w, blk.cout)
            blocks_ws.append(b)
        ws["blocks"] = blocks_ws
        ws["final_hw"] = (h, w)
        ws["yh"], _, _ = conv_out(self.head_conv, h, w)
        ws["ah"] = act(h, w, self.feat_dim)
        ws["pooled"] = torch.empty(N, self.feat_dim, dtype=torch.bfloat16, device=dev)
        ws["logits"] = torch.zeros(N, self.ncls_p, dtype=torch.bfloat16, device=dev)
        dfc = self.fc.desc(N, 1, 1)
        sizes.wgrad = max(sizes.wgrad, lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(dfc)))
        ws["stats"] = torch.empty(max(sizes.stats, 64), dtype=torch.float32, device=dev)
        self._bn_workspaces(ws)
        ws["wgrad_ws"] = torch.empty(sizes.wgrad, dtype=torch.uint8, device=dev)
        ws["wgrad_ws_bytes"] = sizes.wgrad
        ws["bnb_ws"] = torch.zeros(sizes.bnb, dtype=torch.uint8, device=dev)
        ws["bnb_ws_bytes"] = sizes.bnb
        ws["se_ws"] = torch.empty(max(sizes.se, 64), dtype=torch.uint8, device=dev)
        ws["se_ws_bytes"] = sizes.se
        ws["se_de"] = torch.empty(sizes.nc, dtype=torch.float32, device=dev)       # gate gradient and dsn of the block in hand
        ws["se_dsn"] = torch.empty(sizes.nc, dtype=torch.float32, device=dev)
        # scale 1 | shift 0: the data gradient of a depthwise-separable block with a skip is added to the skip's by icamd_bn_apply
        ws["ident"] = torch.cat([torch.ones(self.bn_width, device=dev), torch.zeros(self.bn_width, device=dev)])
        ws["max_act"] = sizes.act
        # loss / metric scratch
        ws["loss_rows"] = torch.empty(N, dtype=torch.float32, device=dev)
        ws["pred"] = torch.empty(N, dtype=torch.int32, device=dev)
        ws["dlogits"] = torch.zeros(N, self.ncls_p, dtype=torch.bfloat16, device=dev)
        ws["dpooled"] = torch.empty(N, self.feat_dim, dtype=torch.bfloat16, device=dev)
        self._ws[key] = ws
        return ws

    def _scratch(self, ws, name):
        """Activation-sized scratch buffers, allocated on first use: "g0".."g2" of the backward pass, "a1" in front of a depthwise call"""
        if name not in ws:
            ws[name] = torch.empty(ws["max_act"], dtype=torch.bfloat16, device=self.device)
        return ws[name]

    # ------------------------------------------------------------------ primitives
    def _conv_bn(self, fw, conv, bn, x, h, w, y):
        """y = conv(x) (raw, with statistic rows when training); -> (OH, OW, scale, shift) of the BatchNorm over y"""
        d = conv.desc(fw.N, h, w)
        hip.check(self.lib.icamd_conv2d_fwd(ctypes.byref(d), x.data_ptr(), self._w(conv), y.data_ptr(), None, None, fw.stats, fw.s),
                  conv.name)
        rows = self.lib.icamd_conv2d_stats_rows(ctypes.byref(d)) if fw.training else 0
        return (d.OH, d.OW) + self._bn_coeffs(fw, bn, rows, fw.N * d.OH * d.OW)

    def _apply_silu(self, s, y, scale, shift, out, what, gate=None):
        """out = silu(y * scale + shift), times gate[n][c] when given; y [N][h][w][C]"""
        N, C = y.shape[0], y.shape[-1]
        hip.check(self.lib.icamd_bn_apply_silu(y.data_ptr(), scale, shift, gate, out, N, y.numel() // (N * C), C, s), what)

    def _a1(self, ws, src, coeffs, s):
        """silu(bn(src)) in the model's one scratch buffer: the input of a depthwise call; -> its pointer"""
        a1 = self._scratch(ws, "a1").data_ptr()
        self._apply_silu(s, src, coeffs[0], coeffs[1], a1, "a1")
        return a1

    def _dw_bn(self, fw, dw, bn, x, h, w, y):
        """y = depthwise(x), x a device pointer; -> (OH, OW, scale, shift) of `bn` over y"""
        lib, N = self.lib, fw.N
        wp = self.shadow.data_ptr() + 2 * dw.w.offset
        if dw.k == 3:
            rc = lib.icamd_dwconv3_fwd(x, None, None, wp, y.data_ptr(), fw.stats, N, h, w, dw.c, dw.stride, fw.s)
        else:
            rc = lib.icamd_dwconv5_fwd(x, wp, y.data_ptr(), fw.stats, N, h, w, dw.c, dw.stride, fw.s)
        hip.check(rc, dw.name)
        oh, ow = y.shape[1], y.shape[2]
        rows = self._dw_entries(dw)[1](N, h, w, dw.c, dw.stride) if fw.training else 0
        return (oh, ow) + self._bn_coeffs(fw, bn, rows, N * oh * ow)

    def _se_gate(self, fw, blk, b, scale, shift, hw):
        """the squeeze pass over y2, the excitation, the gated apply pass: b["a2"] = bf16(silu(bn(y2)) * gate)"""
        lib, ws, N, s, se = self.lib, fw.ws, fw.N, fw.s, blk.se
        hip.check(lib.icamd_bn_silu_squeeze(b["y2"].data_ptr(), scale, shift, b["se_asum"].data_ptr(), N, hw, se.c,
                                            ws["se_ws"].data_ptr(), ws["se_ws_bytes"], s), se.name + " squeeze")
        hip.check(lib.icamd_se_excite_silu_fwd(b["se_asum"].data_ptr(), 1.0 / hw, self._pf(se.w1), self._pf(se.b1), self._pf(se.w2),
                                               self._pf(se.b2), b["se_s"].data_ptr(), b["se_h"].data_ptr(), b["se_e"].data_ptr(), N,
                                               se.c, se.rd, s), se.name + " excite")
        self._apply_silu(s, b["y2"], scale, shift, b["a2"].data_ptr(), se.name + " apply", gate=b["se_e"].data_ptr())

    # ------------------------------------------------------------------ forward
    def pack(self, x_nchw, mix=None):
        """fp32 NCHW device tensor -> packed NHWC bf16 (channels zero-padded to 8), with optional mixup/cutmix."""
        N, C, H, W = x_nchw.shape
        return self._pack_input(self._workspace(N, H, W), x_nchw, mix)

    def _forward_begin(self, ws):
        if self.training:
            self.num_batches_tracked += 1
        return SimpleNamespace(ws=ws, N=ws["N"], s=hip.stream_ptr(), training=self.training,
                               stats=ws["stats"].data_ptr() if self.training else None)

    def forward_packed(self, ws, logits_only=False):   # logits_only: accepted for interface parity (BatchNorm needs every output)
        """Stem, blocks, head -> ws["logits"]: training (batch statistics) or eval (running statistics), the same walk."""
        fw = self._forward_begin(ws)
        lib, s = self.lib, fw.s
        h, w, *coeffs = self._conv_bn(fw, self.stem_conv, self.stem_bn, ws["x8"], ws["H"], ws["W"], ws["y0"])
        x = None                       # None: the block input is silu(stem_bn(y0)), formed in front of blocks.0.0.conv_dw
        for blk, b in zip(self.blocks, ws["blocks"]):
            if blk.kind == "ir":
                h, w, *coeffs = self._conv_bn(fw, blk.pw, blk.bn_pw, x, h, w, b["y1"])
                dw_in = self._a1(ws, b["y1"], coeffs, s)
            else:
                dw_in = self._a1(ws, ws["y0"], coeffs, s) if x is None else x.data_ptr()
            h, w, sc, sh = self._dw_bn(fw, blk.dw, blk.bn_dw, dw_in, h, w, b["y2"])
            self._se_gate(fw, blk, b, sc, sh, h * w)
            h, w, sc, sh = self._conv_bn(fw, blk.pwl, blk.bn_out, b["a2"], h, w, b["y3"])
            res = x.data_ptr() if blk.residual and x is not None else None
            hip.check(lib.icamd_bn_apply(b["y3"].data_ptr(), sc, sh, res, b["out"].data_ptr(), None, b["y3"].numel(), blk.cout, 0, s),
                      blk.bn_out.name)
            x = b["out"]
        h, w, sc, sh = self._conv_bn(fw, self.head_conv, self.head_bn, x, h, w, ws["yh"])
        self._apply_silu(s, ws["yh"], sc, sh, ws["ah"].data_ptr(), "bn2")
        return self._fwd_head(fw, ws["ah"], h, w)

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, run, bn, dout, y, dy, silu, gate=None, dsn=None):
        """dy = BatchNorm backward of `bn` over y from dout: behind a SiLU (silu' recomputed from y; the upstream gradient is dout *
        gate + dsn when the two [N, C] arrays are given) or behind nothing"""
        mean, invstd, scale, shift = self._stats(bn)
        c, N = bn.c, y.shape[0]
        rows = y.numel() // c
        if silu:
            rc = self.lib.icamd_bn_bwd_silu(dout, y.data_ptr(), mean, invstd, scale, shift, gate, dsn, self._gf(bn.weight),
                                            self._gf(bn.bias), dy, N, rows // N, c, run.acc, run.bws, run.bwb, run.s)
        else:
            rc = self.lib.icamd_bn_bwd(dout, None, y.data_ptr(), mean, invstd, scale, shift, self._gf(bn.weight), self._gf(bn.bias),
                                       dy, None, None, rows, c, 0, run.acc, run.bws, run.bwb, run.s)
        hip.check(rc, bn.name + " bwd")

    def _conv_bwd(self, run, conv, x, h, w, dy, dx, addend=None):
        """weight gradient of `conv` from its input x and dy; data gradient into dx (+ addend) unless dx is None"""
        d = conv.desc(run.N, h, w)
        hip.check(self.lib.icamd_conv2d_wgrad(ctypes.byref(d), x, dy, self._gf(conv.w), run.acc, run.wsp, run.wsb, run.s),
                  conv.name + " wgrad")
        if dx is not None:
            hip.check(self.lib.icamd_conv2d_dgrad(ctypes.byref(d), dy, self._wt(conv), dx, addend, None, run.s), conv.name + " dgrad")

    def _se_bn_bwd(self, run, blk, b, dgated, dy):
        """from the gradient of the gated tensor: the gate-gradient pass, the excitation backward (its parameter gradients and dsn),
        and the BatchNorm + SiLU backward of the depthwise BatchNorm under dout * gate + dsn -> dy = d y2"""
        lib, ws, N, se = self.lib, run.ws, run.N, blk.se
        y2 = b["y2"]
        hw = y2.shape[1] * y2.shape[2]
        _, _, scale, shift = self._stats(blk.bn_dw)
        de, dsn = ws["se_de"].data_ptr(), ws["se_dsn"].data_ptr()
        hip.check(lib.icamd_se_silu_bwd_reduce(dgated, y2.data_ptr(), scale, shift, de, N, hw, se.c, ws["se_ws"].data_ptr(),
                                               ws["se_ws_bytes"], run.s), se.name + " gate gradient")
        hip.check(lib.icamd_se_excite_silu_bwd(de, b["se_s"].data_ptr(), b["se_h"].data_ptr(), b["se_e"].data_ptr(), self._pf(se.w1),
                                               self._pf(se.w2), self._gf(se.w1), self._gf(se.b1), self._gf(se.w2), self._gf(se.b2), dsn,
                                               N, se.c, se.rd, 1.0 / hw, run.acc, run.s), se.name + " excite bwd")
        self._bn_bwd(run, blk.bn_dw, dgated, y2, dy, True, gate=b["se_e"].data_ptr(), dsn=dsn)

    def _dw_bwd(self, run, dw, x, h, w, dy, dx):
        """depthwise data gradient into dx (the gradient of the depthwise input) and weight gradient from the input x (a pointer)"""
        lib, N = self.lib, run.N
        wp = self.shadow.data_ptr() + 2 * dw.w.offset
        if dw.k == 3:
            hip.check(lib.icamd_dwconv3_dgrad(dy, wp, dx, N, h, w, dw.c, dw.stride, run.s), dw.name + " dgrad")
            rc = lib.icamd_dwconv3_wgrad(x, None, None, dy, self._gf(dw.w), run.acc, run.wsp, run.wsb, N, h, w, dw.c, dw.stride, run.s)
        else:
            hip.check(lib.icamd_dwconv5_dgrad(dy, wp, dx, N, h, w, dw.c, dw.stride, run.s), dw.name + " dgrad")
            rc = lib.icamd_dwconv5_wgrad(x, dy, self._gf(dw.w), run.acc, run.wsp, run.wsb, N, h, w, dw.c, dw.stride, run.s)
        hip.check(rc, dw.name + " wgrad")

    def backward_packed(self, ws, accumulate=False):
        """Backward from ws['dlogits'] (bf16 [N, ncls_p]); fills the flat fp32 gradient arena.  Gradients become final in reverse
        layer order; `grad_ready_hook(lo, hi, events)` is called as ranges complete (hi None: to the start of the previous range)."""
        lib, N, s = self.lib, ws["N"], hip.stream_ptr()
        run = SimpleNamespace(ws=ws, N=N, s=s, acc=int(bool(accumulate)), wsp=ws["wgrad_ws"].data_ptr(), wsb=ws["wgrad_ws_bytes"],
                              bws=ws["bnb_ws"].data_ptr(), bwb=ws["bnb_ws_bytes"])
        hook = self.grad_ready_hook
        g0, g1, g2 = (self._scratch(ws, k).data_ptr() for k in ("g0", "g1", "g2"))
        # classifier, pool, head
        dl = ws["dlogits"].data_ptr()
        dfc = self.fc.desc(N, 1, 1)
        hip.check(lib.icamd_conv2d_wgrad(ctypes.byref(dfc), ws["pooled"].data_ptr(), dl, self._gf(self.fc.w), run.acc, run.wsp, run.wsb,
                                         s), "classifier wgrad")
        hip.check(lib.icamd_colsum(dl, N, self.ncls_p, self.ncls_p, self._gf(self.fc.b), run.acc, s), "classifier bias grad")
        hip.check(lib.icamd_conv2d_dgrad(ctypes.byref(dfc), dl, self._wt(self.fc), ws["dpooled"].data_ptr(), None, None, s),
                  "classifier dgrad")
        fh, fw_ = ws["final_hw"]
        hip.check(lib.icamd_avgpool_bwd(ws["dpooled"].data_ptr(), g1, N, fh * fw_, self.feat_dim, s), "avgpool bwd")
        self._bn_bwd(run, self.head_bn, g1, ws["yh"], g2, True)
        self._conv_bwd(run, self.head_conv, ws["blocks"][-1]["out"].data_ptr(), fh, fw_, g2, g0)
        if hook:
            hook(self.head_conv.w.offset, self.n_params, ())
        dout, t1, t2 = g0, g1, g2
        for bi in range(len(self.blocks) - 1, -1, -1):
            blk, b = self.blocks[bi], ws["blocks"][bi]
            h, w = b["y2"].shape[1], b["y2"].shape[2]
            self._bn_bwd(run, blk.bn_out, dout, b["y3"], t1, False)                                   # t1 = d y3
            self._conv_bwd(run, blk.pwl, b["a2"].data_ptr(), h, w, t1, t2)                            # t2 = d gated
            self._se_bn_bwd(run, blk, b, t2, t1)                                                      # t1 = d y2
            dh, dw_ = b["dw_hw"]
            if blk.kind == "ir":
                _, _, sc1, sh1 = self._stats(blk.bn_pw)
                self._dw_bwd(run, blk.dw, self._a1(ws, b["y1"], (sc1, sh1), s), dh, dw_, t1, t2)              # t2 = d a1
                self._bn_bwd(run, blk.bn_pw, t2, b["y1"], t1, True)                                   # t1 = d y1
                x_in = ws["blocks"][bi - 1]["out"]
                self._conv_bwd(run, blk.pw, x_in.data_ptr(), *b["in_hw"], t1, t2, dout if blk.residual else None)   # t2 = d in
                first = blk.pw.w.offset
            elif bi == 0:
                _, _, sc0, sh0 = self._stats(self.stem_bn)
                self._dw_bwd(run, blk.dw, self._a1(ws, ws["y0"], (sc0, sh0), s), dh, dw_, t1, t2)             # t2 = d a0
                first = blk.dw.w.offset
            else:
                x_in = ws["blocks"][bi - 1]["out"]
                self._dw_bwd(run, blk.dw, x_in.data_ptr(), dh, dw_, t1, t2)                             # t2 = d in, without the skip's
                if blk.residual:     # t1 = t2 + dout, rounded once more (the depthwise data gradient takes no addend)
                    one = ws["ident"].data_ptr()
                    hip.check(lib.icamd_bn_apply(t2, one, one + 4 * self.bn_width, dout, t1, None, x_in.numel(), blk.cin, 0, s),
                              blk.name + " skip gradient")
                    t1, t2 = t2, t1
                first = blk.dw.w.offset
            dout, t2 = t2, dout
            if hook:
                hook(first, None, ())
        # stem: dout = d a0
        self._bn_bwd(run, self.stem_bn, dout, ws["y0"], t1, True)
        self._conv_bwd(run, self.stem_conv, ws["x8"].data_ptr(), ws["H"], ws["W"], t1, None)
        if hook:
            hook(0, None, ())
