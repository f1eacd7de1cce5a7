"""What the BatchNorm families (nets.py's ResNets; mobilenet.py's MobileNetV2 and efficientnet.py's EfficientNet, through mbconv.py)
share between ArenaModel and the model, defined once: the convolution and BatchNorm records, their slices of the arenas, the running statistics in the state_dict, the saved batch
statistics, the BatchNorm coefficients of a forward pass, and the head (global average pool + classifier).

A model derives from BatchNormModel, builds its records (`convs`, `bns`, the classifier `fc`), hands them to `_layout_arenas` in
module order with `_add_record` for the kinds of its own, and sets `bn_width`.  Its forward and backward walks stay its own.
"""
import ctypes
from collections import OrderedDict

import torch

from . import hip
from .arena import ArenaModel, Layout, align

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


class _Conv:
    """Convolution record. weight param in arena layout [Cout_p][KH][KW][Cin_p / groups] (groups > 1: ResNeXt's 3x3, which runs on
    the icamd_gconv3x3_* entries with this same filter for forward, data gradient and weight gradient)."""

    def __init__(self, name, cin, cout, k, stride, pad, cin_p=None, cout_p=None, bias=False, k_p=None, groups=1):
        self.name = name
        self.groups = groups
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, pad
        self.cin_p = cin_p or cin
        self.cout_p = cout_p or cout
        self.k_p = k_p or k        # kernel extent of the arena layout (ResNet's stem stores 7x7 filters as 8x8x4)
        self.has_bias = bias
        self.w = None      # arena.Param
        self.b = None
        self.wt_offset = None  # offset into the transposed shadow arena (None: no data gradient needed)
        self.descs = {}    # (N, IH, IW) -> ConvDesc
        self.thin = False  # 3x3 / stride 1 with 32 input channels (deep stem): the icamd_conv3x3_thin_* entries where routed
        self.stem7 = False # the 7x7 / stride 2 stem on the rgb4 layout: the icamd_stem7x7s2_* entries

    def desc(self, N, IH, IW):
        key = (N, IH, IW)
        d = self.descs.get(key)
        if d is None:
            d = hip.conv_desc(N, IH, IW, self.cin_p, self.cout_p, self.k, self.k, self.stride, self.pad)
            self.descs[key] = d
        return d


class _BN:
    def __init__(self, name, c):
        self.name, self.c = name, c
        self.weight = self.bias = None  # arena.Param
        self.buf_offset = None          # running_mean at buf_offset, running_var at buf_offset + c
        self.stat_offset = None         # mean, invstd, scale, shift in the per-model stat arena (4*c floats)


class BatchNormModel(ArenaModel):
    # an upper bound of the model's BatchNorm widths: it sizes the finalize workspace and the eval coefficient pair, whose shift sits
    # this many floats behind its scale
    bn_width = None

    # ------------------------------------------------------------------ structure
    def _add_record(self, add, m):
        """The arena slices of a record that is neither convolution, BatchNorm nor classifier."""
        raise TypeError(type(m).__name__)

    def _layout_arenas(self, order, transposed):
        """The arenas for the records `order` (module order: the parameter order of the state_dict) and the transposed filters of
        `transposed` (plan_transposes' argument); the running statistics and the saved batch statistics of every BatchNorm start at
        multiples of 64 elements of `buffer_arena` / `stat_arena`."""
        layout = Layout()
        add = layout.add
        boff = soff = 0
        for m in order:
            if m is self.fc:      # nn.Linear: a 2-D weight in the state_dict, the 1x1 filter [ncls_p][1][1][feat] in the arena
                m.w = add(m.name + ".weight", (m.cout, m.cin), "lin", (m.cout_p, 1, 1, m.cin_p))
                m.b = add(m.name + ".bias", (m.cout,), "vec", (m.cout_p,))
            elif isinstance(m, _Conv):
                m.w = add(m.name + ".weight", (m.cout, m.cin // m.groups, m.k, m.k), "conv",
                          (m.cout_p, m.k_p, m.k_p, m.cin_p // m.groups))
                if m.has_bias:
                    m.b = add(m.name + ".bias", (m.cout,), "vec", (m.cout_p,))
            elif isinstance(m, _BN):
                m.weight = add(m.name + ".weight", (m.c,), "vec", (m.c,))
                m.bias = add(m.name + ".bias", (m.c,), "vec", (m.c,))
                m.buf_offset = boff          # running_mean, then running_var
                boff = align(boff + 2 * m.c, 64)
                m.stat_offset = soff         # mean, invstd, scale, shift of the last training forward
                soff = align(soff + 4 * m.c, 64)
            else:
                self._add_record(add, m)
        self._allocate(layout, transposed, buffer_elems=boff)
        self.stat_arena = torch.zeros(max(soff, 64), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ parameters / state_dict
    def _ctor_kwargs(self):
        return {"arch": self.arch, "num_classes": self.num_classes}

    def _fresh_buffers(self, sd):
        """Adds the buffers of a new model to `sd`: running mean 0, running variance 1, no batch seen."""
        for b in self.bns:
            sd[b.name + ".running_mean"] = torch.zeros(b.c)
            sd[b.name + ".running_var"] = torch.ones(b.c)
            sd[b.name + ".num_batches_tracked"] = torch.tensor(0)

    def _buffer_keys(self):
        return [f"{b.name}.{key}" for b in self.bns for key in ("running_mean", "running_var")]

    def _load_buffers(self, sd):
        bufs = self.buffer_arena.cpu()
        for b in self.bns:
            for j, key in enumerate(("running_mean", "running_var")):
                k = f"{b.name}.{key}"
                if k in sd:
                    bufs[b.buf_offset + j * b.c: b.buf_offset + (j + 1) * b.c] = sd[k].detach().float().cpu()
        self.buffer_arena.copy_(bufs)
        k = f"{self.bns[0].name}.num_batches_tracked"
        if k in sd:
            self.num_batches_tracked = int(sd[k])

    def state_dict(self):
        """Parameters in module order, each BatchNorm's buffers right after its bias (torch's key order)."""
        bufs = self.buffer_arena.cpu()
        bn_of_bias = {b.name + ".bias": b for b in self.bns}
        sd = OrderedDict()
        for name, t in super().state_dict().items():
            sd[name] = t
            b = bn_of_bias.get(name)
            if b is not None:
                sd[b.name + ".running_mean"] = bufs[b.buf_offset:b.buf_offset + b.c].clone()
                sd[b.name + ".running_var"] = bufs[b.buf_offset + b.c:b.buf_offset + 2 * b.c].clone()
                sd[b.name + ".num_batches_tracked"] = torch.tensor(self.num_batches_tracked)
        return sd

    # ------------------------------------------------------------------ forward
    def _bn_workspaces(self, ws):
        """What _bn_coeffs needs in a workspace: the finalize kernel's counters (they start at zero) and the eval coefficient pair."""
        ws["bn_ws"] = torch.zeros(self.lib.icamd_bn_workspace_bytes(self.bn_width), dtype=torch.uint8, device=self.device)
        ws["scale_shift_eval"] = torch.empty(2 * self.bn_width, dtype=torch.float32, device=self.device)

    def _stats(self, bn):
        """(mean, invstd, scale, shift) pointers of a BatchNorm's saved batch statistics."""
        st = self.stat_arena.data_ptr() + 4 * bn.stat_offset
        c = bn.c
        return st, st + 4 * c, st + 8 * c, st + 12 * c

    def _bn_coeffs(self, fw, bn, rows, count):
        """(scale, shift) of `bn`: from the `rows` statistic rows over `count` values per channel that the producer just wrote
        (training; also the saved mean / invstd and the running statistics), or from the running statistics (eval).  `fw`: the
        record of the forward pass (ws, s, training, stats)."""
        lib, c = self.lib, bn.c
        rm = self.buffer_arena.data_ptr() + 4 * bn.buf_offset
        if fw.training:
            mean, invstd, scale, shift = self._stats(bn)
            hip.check(lib.icamd_bn_train_finalize(fw.stats, rows, c, float(count), self._pf(bn.weight), self._pf(bn.bias), rm,
                                                  rm + 4 * c, BN_MOMENTUM, BN_EPS, mean, invstd, scale, shift,
                                                  fw.ws["bn_ws"].data_ptr(), fw.s), bn.name)
            return scale, shift
        # eval: one coefficient pair for the whole walk -- on the one stream every pair is consumed before the next is formed
        scale = fw.ws["scale_shift_eval"].data_ptr()
        shift = scale + 4 * self.bn_width
        hip.check(lib.icamd_bn_eval_coeffs(c, self._pf(bn.weight), self._pf(bn.bias), rm, rm + 4 * c, BN_EPS, scale, shift, fw.s),
                  bn.name)
        return scale, shift

    def _fwd_head(self, fw, x, h, w):
        """Global average pool of x [N][h][w][feat_dim] + classifier with bias -> ws["logits"]."""
        lib, ws, N, s = self.lib, fw.ws, fw.N, fw.s
        hip.check(lib.icamd_avgpool_fwd(x.data_ptr(), ws["pooled"].data_ptr(), N, h * w, self.feat_dim, s), "avgpool")
        dfc = self.fc.desc(N, 1, 1)
        hip.check(lib.icamd_conv2d_fwd(ctypes.byref(dfc), ws["pooled"].data_ptr(), self._w(self.fc),
                                       ws["logits"].data_ptr(), self._pf(self.fc.b), None, None, s), self.fc.name)
        return ws["logits"]
