"""MobileNetV2 on the HIP kernels: timm's `mobilenetv2_*` (inverted residuals, depthwise 3x3, ReLU6), restated.

    conv_stem 3x3/2 -> bn1 + ReLU6
    blocks.0.0   depthwise-separable: conv_dw 3x3 -> bn1 + ReLU6 -> conv_pw 1x1 -> bn2
    blocks.S.B   inverted residual:   conv_pw 1x1 (in -> 6 in) -> bn1 + ReLU6 -> conv_dw 3x3 / s -> bn2 + ReLU6 -> conv_pwl 1x1 -> bn3
                 (+ input when s = 1 and in = out)
    conv_head 1x1 -> bn2 + ReLU6 -> global average pool -> classifier

Every channel count is make_divisible(c * width multiplier, 8), so every pointwise layer runs on the general convolution entries
(Cin % 8 == 0, Cout % 8 == 0) and every depthwise one on icamd_dwconv3_* (C % 8 == 0).  No stochastic depth and no dropout.

What is stored per inverted-residual block: y1 (raw conv_pw output, six times the block's width), y2 (raw depthwise output), a2 =
relu6(bn2(y2)), y3 and the block output.  The activated a1 = relu6(bn1(y1)) is NEVER stored per block: the depthwise forward and weight
gradient either form it on load from y1 and bn1's scale / shift, or icamd_bn_apply_relu6 writes it into the model's one scratch buffer
right in front of them (DW_ONLOAD; the same bits either way), and the BatchNorm + ReLU6 backward recomputes its mask from y and the
same scale / shift.  The same holds for the stem's activation in
front of blocks.0.0.conv_dw.  One stream; eval walks the same graph with icamd_bn_eval_coeffs' scale / shift (no filter folding).
"""
import ctypes
import math
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import hip
from .bnmodel import _BN, _Conv, BatchNormModel

# Does a depthwise layer form relu6(bn(y)) on load ("fwd": icamd_dwconv3_fwd, "wgrad": icamd_dwconv3_wgrad), or read a tensor that
# icamd_bn_apply_relu6 wrote first (into ONE scratch buffer of the model: it is recomputed for the weight gradient, so the expanded
# activation is not stored per block either way)?  A module constant per operation, not an environment variable; both routes give
# the same bits (tests/test_dwconv3_gpu.py, tests/test_mobilenetv2_gpu.py).  Measured (profiles/mobilenetv2.txt, the ten shapes of
# mobilenetv2_100 at batch 256): apply + plain beats the on-load form beyond the spread at all ten shapes for the forward and at nine
# for the weight gradient -- a thread activates the three columns under its output, so the on-load kernels do that arithmetic three times and
# are VALU-bound on it -- so both default to the plain route.
DW_ONLOAD = {"fwd": False, "wgrad": False}

# (repeats, first stride, out channels) of stages 1..6; name -> (width multiplier, stem, stage 0 out, stages, head)
_STAGES = ((2, 2, 24), (3, 2, 32), (4, 2, 64), (3, 1, 96), (3, 2, 160), (1, 1, 320))
CONFIGS = {f"mobilenetv2_{tag}": (m, 32, 16, _STAGES, 1280) for tag, m in (("035", 0.35), ("050", 0.5), ("075", 0.75), ("100", 1.0),
                                                                           ("140", 1.4))}
# parity-test member: a stride-2 block, a stride-1 block with and without residual, the depthwise-separable block
CONFIGS["mobilenetv2_test"] = (1.0, 16, 8, ((2, 2, 16), (1, 2, 24), (2, 1, 32)), 64)


def make_divisible(v, divisor=8, round_limit=0.9):
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new < round_limit * v:
        new += divisor
    return new


def block_plan(arch):
    """(stem width, [(name, kind, in, mid, out, stride)], head width); kind "ds" (mid = in) or "ir" (mid = make_divisible(6 in))"""
    mult, stem, first, stages, head = CONFIGS[arch]
    r = lambda c: make_divisible(c * mult)     # noqa: E731
    cin = r(stem)
    blocks = [("blocks.0.0", "ds", cin, cin, r(first), 1)]
    plan_stem, cin = cin, r(first)
    for si, (repeats, stride, out) in enumerate(stages, 1):
        for bi in range(repeats):
            blocks.append((f"blocks.{si}.{bi}", "ir", cin, make_divisible(cin * 6), r(out), stride if bi == 0 else 1))
            cin = r(out)
    return plan_stem, blocks, (head if arch == "mobilenetv2_test" else max(head, r(head)))


def param_shapes(arch, num_classes=1000):
    """[(name, torch shape)] in timm's module order (parameters only)"""
    stem, blocks, head = block_plan(arch)
    bn = lambda n, c: [(n + ".weight", (c,)), (n + ".bias", (c,))]     # noqa: E731
    out = [("conv_stem.weight", (stem, 3, 3, 3))] + bn("bn1", stem)
    for name, kind, cin, mid, cout, _ in blocks:
        if kind == "ds":
            out += [(name + ".conv_dw.weight", (cin, 1, 3, 3))] + bn(name + ".bn1", cin)
            out += [(name + ".conv_pw.weight", (cout, cin, 1, 1))] + bn(name + ".bn2", cout)
        else:
            out += [(name + ".conv_pw.weight", (mid, cin, 1, 1))] + bn(name + ".bn1", mid)
            out += [(name + ".conv_dw.weight", (mid, 1, 3, 3))] + bn(name + ".bn2", mid)
            out += [(name + ".conv_pwl.weight", (cout, mid, 1, 1))] + bn(name + ".bn3", cout)
    out += [("conv_head.weight", (head, blocks[-1][4], 1, 1))] + bn("bn2", head)
    return out + [("classifier.weight", (num_classes, head)), ("classifier.bias", (num_classes,))]


class _DW:
    """Depthwise 3x3 record: filter [3][3][C] in the arena (kind "dw")."""

    def __init__(self, name, c, stride):
        self.name, self.c, self.stride = name, c, stride
        self.w = None


class MobileNetV2(BatchNormModel):
    """HIP MobileNetV2. `model(x)` runs the forward and returns bf16 logits [B, num_classes] (a view)."""

    def __init__(self, arch="mobilenetv2_100", num_classes=1000, device="cuda", seed=None):
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

        def dw(name, c, stride):
            d = _DW(name, c, stride)
            order.append(d)
            return d

        self.stem_conv = conv("conv_stem", 3, stem, 3, 2, 1, cin_p=8)
        self.stem_bn = bn("bn1", stem)
        self.blocks = []
        for name, kind, cin, mid, cout, stride in plan:
            blk = SimpleNamespace(name=name, kind=kind, cin=cin, mid=mid, cout=cout, stride=stride,
                                  residual=kind == "ir" and stride == 1 and cin == cout)
            if kind == "ds":
                blk.dw, blk.bn_dw = dw(name + ".conv_dw", cin, stride), bn(name + ".bn1", cin)
                blk.pwl, blk.bn_out = conv(name + ".conv_pw", cin, cout), bn(name + ".bn2", cout)
            else:
                blk.pw, blk.bn_pw = conv(name + ".conv_pw", cin, mid), bn(name + ".bn1", mid)
                blk.dw, blk.bn_dw = dw(name + ".conv_dw", mid, stride), bn(name + ".bn2", mid)
                blk.pwl, blk.bn_out = conv(name + ".conv_pwl", mid, cout), bn(name + ".bn3", cout)
            self.blocks.append(blk)
        self.head_conv = conv("conv_head", plan[-1][4], head)
        self.head_bn = bn("bn2", head)
        self.feat_dim = head
        self.fc = conv("classifier", head, self.num_classes, cout_p=self.ncls_p, bias=True)
        self.bn_width = max(b.c for b in self.bns)
        # transposed filters for the data gradients of every pointwise convolution and the classifier (the stem needs none)
        self._layout_arenas(order, [(m, m.cout_p, 1, m.cin_p) for m in self.convs if m is not self.stem_conv])

    def _add_record(self, add, m):
        """The one kind of record of its own: a depthwise filter, tap-major in the arena."""
        m.w = add(m.name + ".weight", (m.c, 1, 3, 3), "dw", (3, 3, m.c))

    # ------------------------------------------------------------------ parameters
    def init_weights(self, seed=None):
        """timm's _init_weight_goog: convolutions N(0, sqrt(2 / fan_out)) with fan_out = k k Cout / groups, BatchNorm 1 / 0,
        classifier weight U(+-1 / sqrt(num_classes)) and bias 0."""
        g = torch.Generator()
        g.manual_seed(seed if seed is not None else torch.initial_seed() % (2 ** 63))
        sd = OrderedDict()
        for name, p in self.params.items():
            if p.kind == "conv":
                cout, _, k, _ = p.torch_shape
                sd[name] = torch.randn(p.torch_shape, generator=g) * math.sqrt(2.0 / (k * k * cout))
            elif p.kind == "dw":
                sd[name] = torch.randn(p.torch_shape, generator=g) * math.sqrt(2.0 / 9.0)
            elif name == "classifier.weight":
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) / math.sqrt(self.num_classes)
            elif name.endswith(".weight"):
                sd[name] = torch.ones(p.torch_shape)
            else:
                sd[name] = torch.zeros(p.torch_shape)
        self._fresh_buffers(sd)
        self.load_state_dict(sd)

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, N, H, W):
        key = (N, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev, lib = self.device, self.lib
        ws = {"N": N, "H": H, "W": W}
        sizes = SimpleNamespace(act=0, stats=0, wgrad=0, bnb=0)

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
            if not lib.icamd_dwconv3_supported(N, h, w, dw.c, dw.stride):
                raise hip.IcamdError(f"{dw.name}: no depthwise 3x3 kernel for {(N, h, w, dw.c)} at stride {dw.stride}")
            oh, ow = (h - 1) // dw.stride + 1, (w - 1) // dw.stride + 1
            sizes.stats = max(sizes.stats, lib.icamd_dwconv3_stats_rows(N, h, w, dw.c, dw.stride) * 2 * dw.c)
            sizes.wgrad = max(sizes.wgrad, lib.icamd_dwconv3_wgrad_workspace_bytes(N, h, w, dw.c, dw.stride))
            sizes.bnb = max(sizes.bnb, lib.icamd_bn_bwd_workspace_bytes(N * oh * ow, dw.c))
            return act(oh, ow, dw.c), oh, ow

        ws["x8"] = act(H, W, 8)
        ws["y0"], h, w = conv_out(self.stem_conv, H, W)
        ws["stem_hw"] = (h, w)
        blocks_ws = []
        for blk in self.blocks:
            b = {"in_hw": (h, w)}
            if blk.kind == "ir":
                b["y1"], h, w = conv_out(blk.pw, h, w)
            b["dw_hw"] = (h, w)
            b["y2"], h, w = dw_out(blk.dw, h, w)
            b["a2"] = act(h, w, blk.dw.c)
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
        ws["max_act"] = sizes.act
        # loss / metric scratch
        ws["loss_rows"] = torch.empty(N, dtype=torch.float32, device=dev)
        ws["pred"] = torch.empty(N, dtype=torch.int32, device=dev)
        ws["dlogits"] = torch.zeros(N, self.ncls_p, dtype=torch.bfloat16, device=dev)
        ws["dpooled"] = torch.empty(N, self.feat_dim, dtype=torch.bfloat16, device=dev)
        self._ws[key] = ws
        return ws

    def _scratch(self, ws, name):
        """Activation-sized scratch buffers, allocated on first use: "g0".."g2" of the backward pass, "a1" of a plain depthwise route"""
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

    def _dw_input(self, ws, op, src, coeffs, s):
        """(x, scale, shift) arguments of a depthwise entry whose input is relu6(bn(src)): on load, or applied into the scratch"""
        if DW_ONLOAD[op]:
            return src.data_ptr(), coeffs[0], coeffs[1]
        a1 = self._scratch(ws, "a1")
        c = src.shape[-1]
        hip.check(self.lib.icamd_bn_apply_relu6(src.data_ptr(), coeffs[0], coeffs[1], a1.data_ptr(), src.numel(), c, s), "a1")
        return a1.data_ptr(), None, None

    def _dw_bn(self, fw, dw, bn, src, coeffs, h, w, y):
        """y = depthwise(relu6(bn_src(src))); -> (OH, OW, scale, shift) of `bn` over y"""
        lib, N = self.lib, fw.N
        x, sc, sh = self._dw_input(fw.ws, "fwd", src, coeffs, fw.s)
        hip.check(lib.icamd_dwconv3_fwd(x, sc, sh, self.shadow.data_ptr() + 2 * dw.w.offset, y.data_ptr(), fw.stats, N, h, w, dw.c,
                                        dw.stride, fw.s), dw.name)
        oh, ow = y.shape[1], y.shape[2]
        rows = lib.icamd_dwconv3_stats_rows(N, h, w, dw.c, dw.stride) if fw.training else 0
        return (oh, ow) + self._bn_coeffs(fw, bn, rows, N * oh * ow)

    def _apply_relu6(self, fw, y, scale, shift, out, what):
        hip.check(self.lib.icamd_bn_apply_relu6(y.data_ptr(), scale, shift, out.data_ptr(), y.numel(), y.shape[-1], fw.s), what)

    # ------------------------------------------------------------------ forward
    def pack(self, x_nchw, mix=None):
        """fp32 NCHW device tensor -> packed NHWC bf16 (channels zero-padded to 8), with optional mixup/cutmix."""
        N, C, H, W = x_nchw.shape
        return self._pack_input(self._workspace(N, H, W), x_nchw, mix)

    def _forward_begin(self, ws):
        if self.training:
            self.num_batches_tracked += 1
        fw = SimpleNamespace(ws=ws, N=ws["N"], s=hip.stream_ptr(), training=self.training,
                             stats=ws["stats"].data_ptr() if self.training else None)
        return fw

    def forward_packed(self, ws, logits_only=False):   # logits_only: accepted for interface parity (BatchNorm needs every output)
        """Stem, blocks, head -> ws["logits"]: training (batch statistics) or eval (running statistics), the same walk."""
        fw = self._forward_begin(ws)
        lib, s = self.lib, fw.s
        h, w, *coeffs = self._conv_bn(fw, self.stem_conv, self.stem_bn, ws["x8"], ws["H"], ws["W"], ws["y0"])
        src = ws["y0"]                 # raw: the consumer (blocks.0.0.conv_dw) activates it
        x = None
        for blk, b in zip(self.blocks, ws["blocks"]):
            if blk.kind == "ir":
                h, w, *coeffs = self._conv_bn(fw, blk.pw, blk.bn_pw, x, h, w, b["y1"])
                src = b["y1"]
            h, w, sc, sh = self._dw_bn(fw, blk.dw, blk.bn_dw, src, coeffs, h, w, b["y2"])
            self._apply_relu6(fw, b["y2"], sc, sh, b["a2"], blk.bn_dw.name)
            h, w, sc, sh = self._conv_bn(fw, blk.pwl, blk.bn_out, b["a2"], h, w, b["y3"])
            hip.check(lib.icamd_bn_apply(b["y3"].data_ptr(), sc, sh, x.data_ptr() if blk.residual else None, b["out"].data_ptr(),
                                         None, b["y3"].numel(), blk.cout, 0, s), blk.bn_out.name)
            x = b["out"]
        h, w, sc, sh = self._conv_bn(fw, self.head_conv, self.head_bn, x, h, w, ws["yh"])
        self._apply_relu6(fw, ws["yh"], sc, sh, ws["ah"], "bn2")
        return self._fwd_head(fw, ws["ah"], h, w)

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, run, bn, dout, y, dy, relu6):
        """dy = BatchNorm backward of `bn` over y from dout, behind a ReLU6 (mask recomputed from y) or behind nothing"""
        mean, invstd, scale, shift = self._stats(bn)
        c, rows = bn.c, y.numel() // bn.c
        if relu6:
            rc = self.lib.icamd_bn_bwd_relu6(dout, y.data_ptr(), mean, invstd, scale, shift, self._gf(bn.weight), self._gf(bn.bias),
                                             dy, rows, c, run.acc, run.bws, run.bwb, run.s)
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

    def _dw_bwd(self, run, dw, src, src_bn, h, w, dy, dx):
        """depthwise data gradient into dx (the gradient of the activated input) and weight gradient, the input formed from src"""
        lib, N = self.lib, run.N
        wp = self.shadow.data_ptr() + 2 * dw.w.offset
        hip.check(lib.icamd_dwconv3_dgrad(dy, wp, dx, N, h, w, dw.c, dw.stride, run.s), dw.name + " dgrad")
        _, _, scale, shift = self._stats(src_bn)
        x, sc, sh = self._dw_input(run.ws, "wgrad", src, (scale, shift), run.s)
        hip.check(lib.icamd_dwconv3_wgrad(x, sc, sh, dy, self._gf(dw.w), run.acc, run.wsp, run.wsb, N, h, w, dw.c, dw.stride, run.s),
                  dw.name + " wgrad")

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
            self._conv_bwd(run, blk.pwl, b["a2"].data_ptr(), h, w, t1, t2)                            # t2 = d a2
            self._bn_bwd(run, blk.bn_dw, t2, b["y2"], t1, True)                                       # t1 = d y2
            dh, dw_ = b["dw_hw"]
            if blk.kind == "ir":
                self._dw_bwd(run, blk.dw, b["y1"], blk.bn_pw, dh, dw_, t1, t2)                        # t2 = d a1
                self._bn_bwd(run, blk.bn_pw, t2, b["y1"], t1, True)                                   # t1 = d y1
                x_in = ws["blocks"][bi - 1]["out"]
                self._conv_bwd(run, blk.pw, x_in.data_ptr(), *b["in_hw"], t1, t2, dout if blk.residual else None)   # t2 = d in
                first = blk.pw.w.offset
            else:
                self._dw_bwd(run, blk.dw, ws["y0"], self.stem_bn, dh, dw_, t1, t2)                    # t2 = d a0
                first = blk.dw.w.offset
            dout, t2 = t2, dout
            if hook:
                hook(first, None, ())
        # stem: dout = d a0
        self._bn_bwd(run, self.stem_bn, dout, ws["y0"], t1, True)
        self._conv_bwd(run, self.stem_conv, ws["x8"].data_ptr(), ws["H"], ws["W"], t1, None)
        if hook:
            hook(0, None, ())
