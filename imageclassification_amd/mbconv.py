"""What the MBConv families (mobilenet.py's MobileNetV2, efficientnet.py's EfficientNet) share on top of BatchNormModel, defined once:
timm's stem, depthwise-separable block, inverted-residual blocks, 1x1 head, pool and classifier as records, weights, workspaces and
ONE forward and ONE backward walk.

    conv_stem 3x3/2 -> bn1 + act
    "ds" block   conv_dw k x k -> bn1 + act [-> se] -> conv_pw 1x1 -> bn2 (+ input where the model's rule says so)
    "ir" block   conv_pw 1x1 (in -> mid) -> bn1 + act -> conv_dw k x k / s -> bn2 + act [-> se] -> conv_pwl 1x1 -> bn3 (+ input)
    conv_head 1x1 -> bn2 + act -> global average pool -> classifier

A model derives from MBConvModel and supplies its `block_plan` -- (stem width, [(name, kind, k, in, mid, out, stride, rd)], head
width), rd the reduced width of the block's squeeze-and-excitation or None -- and what differs:

    _residual                        which blocks add their input
    _apply_act, _bn_act_bwd          the activation: the activated BatchNorm apply and the activated BatchNorm backward
    _dw_input, _dw_bwd               how the activated input of a depthwise layer is formed, and where in its backward
    _after_dw_fwd, _after_dw_bwd     what stands behind the depthwise BatchNorm: the activation alone, or the gate as well
    _se_record, _block_workspace, _extra_workspaces     the records and buffers of a squeeze-and-excitation (none by default)

The activated input of a depthwise layer is never stored per block; the two module docstrings say what is stored and what is
recomputed.  One stream; eval walks the same graph with icamd_bn_eval_coeffs' scale / shift (no filter folding).
"""
import ctypes
import math
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import hip
from .bnmodel import _BN, _Conv, BatchNormModel


def param_shapes(plan, num_classes, se_shapes=None):
    """[(name, torch shape)] in timm's module order (parameters only) of a block_plan; se_shapes(name, c, rd): the rows of a
    squeeze-and-excitation, behind the depthwise BatchNorm of every block whose rd is not None"""
    stem, blocks, head = plan
    bn = lambda n, c: [(n + ".weight", (c,)), (n + ".bias", (c,))]     # noqa: E731
    out = [("conv_stem.weight", (stem, 3, 3, 3))] + bn("bn1", stem)
    for name, kind, k, cin, mid, cout, _, rd in blocks:
        n = 1
        if kind == "ir":
            out += [(name + ".conv_pw.weight", (mid, cin, 1, 1))] + bn(name + ".bn1", mid)
            n = 2
        out += [(name + ".conv_dw.weight", (mid, 1, k, k))] + bn(f"{name}.bn{n}", mid)
        if rd is not None:
            out += se_shapes(name + ".se", mid, rd)
        out += [(name + (".conv_pwl" if kind == "ir" else ".conv_pw") + ".weight", (cout, mid, 1, 1))] + bn(f"{name}.bn{n + 1}", cout)
    out += [("conv_head.weight", (head, blocks[-1][5], 1, 1))] + bn("bn2", head)
    return out + [("classifier.weight", (num_classes, head)), ("classifier.bias", (num_classes,))]


class _DW:
    """Depthwise k x k record: filter [k][k][C] in the arena (kind "dw")."""

    def __init__(self, name, c, k, stride):
        self.name, self.c, self.k, self.stride = name, c, k, stride
        self.w = None


class MBConvModel(BatchNormModel):
    """`model(x)` runs the forward and returns bf16 logits [B, num_classes] (a view)."""

    def __init__(self, arch, num_classes, device, seed):
        super().__init__(arch, num_classes, device)
        lib = self.lib
        # the depthwise entries by filter size; the 3x3 forward and weight gradient take two more pointers (_dw_call)
        self._dw_entries = {
            3: SimpleNamespace(supported=lib.icamd_dwconv3_supported, stats_rows=lib.icamd_dwconv3_stats_rows,
                               wgrad_workspace_bytes=lib.icamd_dwconv3_wgrad_workspace_bytes, fwd=lib.icamd_dwconv3_fwd,
                               dgrad=lib.icamd_dwconv3_dgrad, wgrad=lib.icamd_dwconv3_wgrad),
            5: SimpleNamespace(supported=lib.icamd_dwconv5_supported, stats_rows=lib.icamd_dwconv5_stats_rows,
                               wgrad_workspace_bytes=lib.icamd_dwconv5_wgrad_workspace_bytes, fwd=lib.icamd_dwconv5_fwd,
                               dgrad=lib.icamd_dwconv5_dgrad, wgrad=lib.icamd_dwconv5_wgrad)}
        self._build()
        self.init_weights(seed=seed)

    # ------------------------------------------------------------------ structure
    def _residual(self, kind, cin, cout, stride):
        """Does a block of this kind and these widths add its input?"""
        raise NotImplementedError

    def _se_record(self, name, c, rd):
        """The squeeze-and-excitation record of a block whose plan row has a reduced width."""
        raise NotImplementedError(f"{type(self).__name__} has no squeeze-and-excitation ({name})")

    def _build(self):
        stem, plan, head = self.block_plan(self.arch)
        self.bns, self.convs = [], []
        order = []          # records in module order

        def add(m):
            order.append(m)
            if isinstance(m, (_Conv, _BN)):
                (self.convs if isinstance(m, _Conv) else self.bns).append(m)
            return m

        def pw(name, cin, cout):
            return add(_Conv(name, cin, cout, 1, 1, 0))

        self.stem_conv = add(_Conv("conv_stem", 3, stem, 3, 2, 1, cin_p=8))
        self.stem_bn = add(_BN("bn1", stem))
        self.blocks = []
        for name, kind, k, cin, mid, cout, stride, rd in plan:
            blk = SimpleNamespace(name=name, kind=kind, cin=cin, mid=mid, cout=cout, stride=stride,
                                  residual=self._residual(kind, cin, cout, stride))
            n = 1
            if kind == "ir":
                blk.pw, blk.bn_pw = pw(name + ".conv_pw", cin, mid), add(_BN(name + ".bn1", mid))
                n = 2
            blk.dw, blk.bn_dw = add(_DW(name + ".conv_dw", mid, k, stride)), add(_BN(f"{name}.bn{n}", mid))
            if rd is not None:
                blk.se = add(self._se_record(name + ".se", mid, rd))
            blk.pwl, blk.bn_out = pw(name + (".conv_pwl" if kind == "ir" else ".conv_pw"), mid, cout), add(_BN(f"{name}.bn{n + 1}", cout))
            self.blocks.append(blk)
        self.head_conv = pw("conv_head", plan[-1][5], head)
        self.head_bn = add(_BN("bn2", head))
        self.feat_dim = head
        self.fc = add(_Conv("classifier", head, self.num_classes, 1, 1, 0, cout_p=self.ncls_p, bias=True))
        self.bn_width = max(b.c for b in self.bns)
        # transposed filters for the data gradients of every pointwise convolution and the classifier (the stem needs none)
        self._layout_arenas(order, [(m, m.cout_p, 1, m.cin_p) for m in self.convs if m is not self.stem_conv])

    def _add_record(self, add, m):
        """The one kind of record of its own: a depthwise filter, tap-major in the arena."""
        if not isinstance(m, _DW):
            return super()._add_record(add, m)
        m.w = add(m.name + ".weight", (m.c, 1, m.k, m.k), "dw", (m.k, m.k, m.c))

    # ------------------------------------------------------------------ parameters
    def init_weights(self, seed=None):
        """timm's _init_weight_goog: convolutions (those of a squeeze-and-excitation included) N(0, sqrt(2 / fan_out)) with fan_out =
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
    def _block_workspace(self, blk, b, N, hw, sizes):
        """What a block keeps besides y1, y2, a2, y3 and its output: `b` gains it, `sizes` the maxima _extra_workspaces needs."""

    def _extra_workspaces(self, ws, sizes):
        """What the workspace holds besides the shared buffers."""

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
            e = self._dw_entries.get(dw.k)
            if e is None or not e.supported(N, h, w, dw.c, dw.stride):
                raise hip.IcamdError(f"{dw.name}: no depthwise {dw.k}x{dw.k} kernel for {(N, h, w, dw.c)} at stride {dw.stride}")
            oh, ow = (h - 1) // dw.stride + 1, (w - 1) // dw.stride + 1
            sizes.stats = max(sizes.stats, e.stats_rows(N, h, w, dw.c, dw.stride) * 2 * dw.c)
            sizes.wgrad = max(sizes.wgrad, e.wgrad_workspace_bytes(N, h, w, dw.c, dw.stride))
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
            b["a2"] = act(h, w, blk.dw.c)          # the projection input: activated, and gated where the block has a gate
            self._block_workspace(blk, b, N, h * w, sizes)
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
        self._extra_workspaces(ws, sizes)
        ws["max_act"] = sizes.act
        # loss / metric scratch
        ws["loss_rows"] = torch.empty(N, dtype=torch.float32, device=dev)
        ws["pred"] = torch.empty(N, dtype=torch.int32, device=dev)
        ws["dlogits"] = torch.zeros(N, self.ncls_p, dtype=torch.bfloat16, device=dev)
        ws["dpooled"] = torch.empty(N, self.feat_dim, dtype=torch.bfloat16, device=dev)
        self._ws[key] = ws
        return ws

    def _scratch(self, ws, name):
        """Activation-sized scratch buffers, allocated on first use: "g0".."g2" of the backward pass, "a1" in front of a depthwise
        call that does not activate its input on load"""
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

    def _apply_act(self, s, y, scale, shift, out, what):
        """out (a pointer) = act(y * scale + shift), y a tensor [N][h][w][C]"""
        raise NotImplementedError

    def _dw_input(self, ws, op, src, coeffs, s):
        """(x, scale, shift) arguments of the depthwise entry `op` ("fwd" or "wgrad") whose input is act(bn(src)): the raw tensor and
        the coefficients that activate it on load, or a tensor written here and two NULLs"""
        raise NotImplementedError

    def _dw_call(self, dw, op, dw_in, *rest):
        """The forward or weight gradient of `dw` on dw_in = (x, scale, shift); only the 3x3 entries take the scale / shift"""
        entry = getattr(self._dw_entries[dw.k], op)
        x, scale, shift = dw_in
        if dw.k == 3:
            return entry(x, scale, shift, *rest)
        if scale is not None or shift is not None:
            raise hip.IcamdError(f"{dw.name}: the depthwise {dw.k}x{dw.k} kernels do not activate their input on load")
        return entry(x, *rest)

    def _dw_bn(self, fw, dw, bn, dw_in, h, w, y):
        """y = depthwise(dw_in), dw_in = (x, scale, shift) as _dw_input gives them; -> (OH, OW, scale, shift) of `bn` over y"""
        N = fw.N
        hip.check(self._dw_call(dw, "fwd", dw_in, self.shadow.data_ptr() + 2 * dw.w.offset, y.data_ptr(), fw.stats, N, h, w, dw.c,
                                dw.stride, fw.s), dw.name)
        oh, ow = y.shape[1], y.shape[2]
        rows = self._dw_entries[dw.k].stats_rows(N, h, w, dw.c, dw.stride) if fw.training else 0
        return (oh, ow) + self._bn_coeffs(fw, bn, rows, N * oh * ow)

    def _after_dw_fwd(self, fw, blk, b, scale, shift):
        """b["a2"], the projection input, from b["y2"] and the depthwise BatchNorm's scale / shift"""
        raise NotImplementedError

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
        src = ws["y0"]                 # raw: the consumer (blocks.0.0.conv_dw) activates it
        x = None                       # None: the block input is act(stem_bn(y0)), never stored
        for blk, b in zip(self.blocks, ws["blocks"]):
            if blk.kind == "ir":
                h, w, *coeffs = self._conv_bn(fw, blk.pw, blk.bn_pw, x, h, w, b["y1"])
                src = b["y1"]
            if blk.kind == "ir" or x is None:
                dw_in = self._dw_input(ws, "fwd", src, coeffs, s)
            else:                      # a depthwise-separable block beyond the first reads the stored block input
                dw_in = (x.data_ptr(), None, None)
            h, w, sc, sh = self._dw_bn(fw, blk.dw, blk.bn_dw, dw_in, h, w, b["y2"])
            self._after_dw_fwd(fw, blk, b, sc, sh)
            h, w, sc, sh = self._conv_bn(fw, blk.pwl, blk.bn_out, b["a2"], h, w, b["y3"])
            res = x.data_ptr() if blk.residual and x is not None else None
            hip.check(lib.icamd_bn_apply(b["y3"].data_ptr(), sc, sh, res, b["out"].data_ptr(), None, b["y3"].numel(), blk.cout, 0, s),
                      blk.bn_out.name)
            x = b["out"]
        h, w, sc, sh = self._conv_bn(fw, self.head_conv, self.head_bn, x, h, w, ws["yh"])
        self._apply_act(s, ws["yh"], sc, sh, ws["ah"].data_ptr(), "bn2")
        return self._fwd_head(fw, ws["ah"], h, w)

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, run, bn, dout, y, dy):
        """dy = BatchNorm backward of `bn` over y from dout, behind no activation"""
        mean, invstd, scale, shift = self._stats(bn)
        hip.check(self.lib.icamd_bn_bwd(dout, None, y.data_ptr(), mean, invstd, scale, shift, self._gf(bn.weight), self._gf(bn.bias),
                                        dy, None, None, y.numel() // bn.c, bn.c, 0, run.acc, run.bws, run.bwb, run.s), bn.name + " bwd")

    def _bn_act_bwd(self, run, bn, dout, y, dy):
        """dy = BatchNorm backward of `bn` over y from dout, behind the activation (its derivative recomputed from y)"""
        raise NotImplementedError

    def _after_dw_bwd(self, run, blk, b, da2, dy):
        """dy = d y2 from da2, the gradient of the projection input: what _after_dw_fwd did, backward"""
        raise NotImplementedError

    def _conv_bwd(self, run, conv, x, h, w, dy, dx, addend=None):
        """weight gradient of `conv` from its input x and dy; data gradient into dx (+ addend) unless dx is None"""
        d = conv.desc(run.N, h, w)
        hip.check(self.lib.icamd_conv2d_wgrad(ctypes.byref(d), x, dy, self._gf(conv.w), run.acc, run.wsp, run.wsb, run.s),
                  conv.name + " wgrad")
        if dx is not None:
            hip.check(self.lib.icamd_conv2d_dgrad(ctypes.byref(d), dy, self._wt(conv), dx, addend, None, run.s), conv.name + " dgrad")

    def _dw_dgrad(self, run, dw, h, w, dy, dx):
        """depthwise data gradient into dx: the gradient of the depthwise input"""
        hip.check(self._dw_entries[dw.k].dgrad(dy, self.shadow.data_ptr() + 2 * dw.w.offset, dx, run.N, h, w, dw.c, dw.stride, run.s),
                  dw.name + " dgrad")

    def _dw_wgrad(self, run, dw, dw_in, h, w, dy):
        """depthwise weight gradient from the input dw_in = (x, scale, shift)"""
        hip.check(self._dw_call(dw, "wgrad", dw_in, dy, self._gf(dw.w), run.acc, run.wsp, run.wsb, run.N, h, w, dw.c, dw.stride, run.s),
                  dw.name + " wgrad")

    def _dw_bwd(self, run, dw, src, src_bn, h, w, dy, dx):
        """_dw_dgrad into dx and _dw_wgrad of a depthwise layer whose input is act(src_bn(src)), formed again by _dw_input from the
        saved scale / shift of src_bn; where among the two the input is formed is the model's"""
        raise NotImplementedError

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
        self._bn_act_bwd(run, self.head_bn, g1, ws["yh"], g2)
        self._conv_bwd(run, self.head_conv, ws["blocks"][-1]["out"].data_ptr(), fh, fw_, g2, g0)
        if hook:
            hook(self.head_conv.w.offset, self.n_params, ())
        dout, t1, t2 = g0, g1, g2
        for bi in range(len(self.blocks) - 1, -1, -1):
            blk, b = self.blocks[bi], ws["blocks"][bi]
            h, w = b["y2"].shape[1], b["y2"].shape[2]
            self._bn_bwd(run, blk.bn_out, dout, b["y3"], t1)                                          # t1 = d y3
            self._conv_bwd(run, blk.pwl, b["a2"].data_ptr(), h, w, t1, t2)                            # t2 = d a2
            self._after_dw_bwd(run, blk, b, t2, t1)                                                   # t1 = d y2
            dh, dw_ = b["dw_hw"]
            x_in = ws["blocks"][bi - 1]["out"] if bi else None
            if blk.kind == "ir":
                self._dw_bwd(run, blk.dw, b["y1"], blk.bn_pw, dh, dw_, t1, t2)                        # t2 = d a1
                self._bn_act_bwd(run, blk.bn_pw, t2, b["y1"], t1)                                     # t1 = d y1
                self._conv_bwd(run, blk.pw, x_in.data_ptr(), *b["in_hw"], t1, t2, dout if blk.residual else None)   # t2 = d in
                first = blk.pw.w.offset
            elif x_in is None:
                self._dw_bwd(run, blk.dw, ws["y0"], self.stem_bn, dh, dw_, t1, t2)                    # t2 = d a0
                first = blk.dw.w.offset
            else:                    # a depthwise-separable block beyond the first: its input is stored
                self._dw_dgrad(run, blk.dw, dh, dw_, t1, t2)                                          # t2 = d in, without the skip's
                self._dw_wgrad(run, blk.dw, (x_in.data_ptr(), None, None), dh, dw_, t1)
                if blk.residual:     # t1 = t2 + dout, rounded once more (the depthwise data gradient takes no addend); the model
                    one = ws["ident"].data_ptr()     # whose plan has such a block keeps scale 1 | shift 0 in ws["ident"]
                    hip.check(lib.icamd_bn_apply(t2, one, one + 4 * self.bn_width, dout, t1, None, x_in.numel(), blk.cin, 0, s),
                              blk.name + " skip gradient")
                    t1, t2 = t2, t1
                first = blk.dw.w.offset
            dout, t2 = t2, dout
            if hook:
                hook(first, None, ())
        # stem: dout = d a0
        self._bn_act_bwd(run, self.stem_bn, dout, ws["y0"], t1)
        self._conv_bwd(run, self.stem_conv, ws["x8"].data_ptr(), ws["H"], ws["W"], t1, None)
        if hook:
            hook(0, None, ())
