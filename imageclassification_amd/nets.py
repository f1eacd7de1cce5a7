"""The ResNet family (ResNet-18/34/50/101/152, wide ResNet-50/101-2, ResNeXt-50/101 32x4d, SE-ResNet-50/101/152,
SE-ResNeXt-50/101 32x4d, and the "D" variants ResNet-18d/34d/26d/50d/101d/152d/200d, SE-ResNet-152d, SE-ResNeXt-26d 32x4d) on
the gfx950 kernels: static layer lists with hand-written forward and backward.

The reference builds its network with timm.create_model (/root/reference/train.py:194) and runs it through
autograd (engine.py:48,51,64,72); there is no model code in the reference tree.  Here a model is a flat list
of layer records over four flat arenas (fp32 parameters, fp32 gradients, bf16 "shadow" filters the conv
kernels read, fp32 BatchNorm buffers; the arena protocol is arena.py's) and every layer's forward/backward is one or more C-ABI calls
(include/icamd.h).  No autograd graph, no torch ops on the step path.

Architecture = timm/torchvision ResNet v1.5 (stride on the 3x3 of a bottleneck), BatchNorm eps 1e-5,
momentum 0.1, parameter names identical to timm's (`conv1.weight`, `layer1.0.bn1.weight`, ..., `fc.bias`) so
state_dicts interchange with the CPU oracle and with timm checkpoints.

Data layout in HBM: activations NHWC bf16; filters [Cout][KH][KW][Cin] (stem Cin zero-padded 3->8, FC rows
zero-padded to a multiple of 64); everything 256 B aligned inside the arenas.
"""
import ctypes
import itertools
import math
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import hip
from .bnmodel import BN_EPS, BN_MOMENTUM, _BN, _Conv, BatchNormModel      # noqa: F401  (the names stay importable from here)
from .streams import side_lane

_FUSED_BNBWD = os.environ.get("ICAMD_FUSED_BNBWD", "0") == "1"
_WGRAD_STREAM = os.environ.get("ICAMD_WGRAD_STREAM", "1") != "0"
_DUAL_BNBWD = os.environ.get("ICAMD_DUAL_BNBWD", "1") != "0"
_SUB2_SHORTCUT = os.environ.get("ICAMD_SUB2_SHORTCUT", "1") != "0"
# stem max-pool backward folded into the BatchNorm backward (icamd_bn_bwd_maxpool3x3s2, bit-identical): the 411 MB pooled
# gradient at full resolution is never written or read.  On by default since the gather reads the pooled rows from LDS
# (norm_pool.hip, PoolGather): measured on one MI355X in one call (profiles/r06_stem_tail_ab.txt), 183 + 210 = 393 us for the two
# folded passes against 195 + 164 + 197 = 555 us for pool backward + the two BatchNorm passes of the parent library, and
# 17.78 against 18.06 ms per step.  (Round 2, gather from global memory: -0.20 ms of pooling, +0.27 ms of BatchNorm backward.)
# ICAMD_FUSED_POOL_BWD=0 forces the two-call route.
_FUSED_POOL_BWD = os.environ.get("ICAMD_FUSED_POOL_BWD", "1") != "0"
# The thin 3x3 kernels (csrc/conv_stem_deep.hip) under the second and third convolution of a D variant's deep stem, per operation.
# ICAMD_STEM_THIN (read once per process): unset / 1 = the defaults below, wherever icamd_conv3x3_thin_supported says so; 0 = every
# operation on icamd_conv2d_fwd / _dgrad / _wgrad; 2 = every operation on the thin kernels.  A default is False where the thin
# kernel measured slower than the general route (tools/bench_stem_deep.py, profiles/resnet_d.txt): at batch 256,
# 112 x 112 the thin forward is 2.0x / 1.4x (32 -> 32 / 32 -> 64) and the thin data gradient 2.2x / 1.7x faster than the general
# route, the thin weight gradient 0.71x / 0.66x (401 / 474 us against 286 / 311 us) -- so the weight gradient stays on
# icamd_conv2d_wgrad unless ICAMD_STEM_THIN=2.
_STEM_THIN_DEFAULT = {"fwd": True, "dgrad": True, "wgrad": False}
_STEM_THIN_ENV = os.environ.get("ICAMD_STEM_THIN", "1")
_STEM_THIN = {op: (_STEM_THIN_ENV == "2" or (_STEM_THIN_ENV != "0" and on)) for op, on in _STEM_THIN_DEFAULT.items()}

# name -> (block, blocks per stage, cardinality, base width), as timm / torchvision: a bottleneck's inner width is
# floor(planes * base_width / 64) * cardinality and its 3x3 convolution has `cardinality` groups
ARCHS = {
    "resnet18": ("basic", [2, 2, 2, 2], 1, 64),
    "resnet34": ("basic", [3, 4, 6, 3], 1, 64),
    "resnet50": ("bottleneck", [3, 4, 6, 3], 1, 64),
    "resnet101": ("bottleneck", [3, 4, 23, 3], 1, 64),
    "resnet152": ("bottleneck", [3, 8, 36, 3], 1, 64),
    "wide_resnet50_2": ("bottleneck", [3, 4, 6, 3], 1, 128),
    "wide_resnet101_2": ("bottleneck", [3, 4, 23, 3], 1, 128),
    "resnext50_32x4d": ("bottleneck", [3, 4, 6, 3], 32, 4),
    "resnext101_32x4d": ("bottleneck", [3, 4, 23, 3], 32, 4),
    # a fifth entry True: squeeze-and-excitation on the output of every block's last BatchNorm (timm attn_layer='se')
    "seresnet50": ("bottleneck", [3, 4, 6, 3], 1, 64, True),
    "seresnet101": ("bottleneck", [3, 4, 23, 3], 1, 64, True),
    "seresnet152": ("bottleneck", [3, 8, 36, 3], 1, 64, True),
    "seresnext50_32x4d": ("bottleneck", [3, 4, 6, 3], 32, 4, True),
    "seresnext101_32x4d": ("bottleneck", [3, 4, 23, 3], 32, 4, True),
    # a sixth entry True: the "D" variant of "Bag of Tricks" (timm stem_width=32, stem_type='deep', avg_down=True): the 7x7 stem
    # becomes three 3x3 convolutions (3 -> 32 stride 2, 32 -> 32, 32 -> 64), and a projection shortcut becomes
    # AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False) -> 1x1 stride-1 convolution -> BatchNorm
    "resnet18d": ("basic", [2, 2, 2, 2], 1, 64, False, True),
    "resnet34d": ("basic", [3, 4, 6, 3], 1, 64, False, True),
    "resnet26d": ("bottleneck", [2, 2, 2, 2], 1, 64, False, True),
    "resnet50d": ("bottleneck", [3, 4, 6, 3], 1, 64, False, True),
    "resnet101d": ("bottleneck", [3, 4, 23, 3], 1, 64, False, True),
    "resnet152d": ("bottleneck", [3, 8, 36, 3], 1, 64, False, True),
    "resnet200d": ("bottleneck", [3, 24, 36, 3], 1, 64, False, True),
    "seresnet152d": ("bottleneck", [3, 8, 36, 3], 1, 64, True, True),
    "seresnext26d_32x4d": ("bottleneck", [2, 2, 2, 2], 32, 4, True, True),
}
SE_REDUCTION = 16   # timm SEModule: rd_channels = make_divisible(C / 16, 8, round_limit=0) = C / 16 for C in 256 .. 2048


def has_se(arch):
    row = ARCHS[arch]
    return len(row) > 4 and bool(row[4])


def is_d(arch):
    row = ARCHS[arch]
    return len(row) > 5 and bool(row[5])


def stem_specs(arch):
    """The stem as [((conv tuple), (bn tuple))] in module order; conv tuple as in block_specs."""
    if not is_d(arch):
        return [(("conv1", 3, 64, 7, 2, 3, 1), ("bn1", 64))]
    # nn.Sequential(conv, bn, relu, conv, bn, relu, conv) named conv1, then bn1: indices 2 and 5 are the ReLUs
    return [(("conv1.0", 3, 32, 3, 2, 1, 1), ("conv1.1", 32)), (("conv1.3", 32, 32, 3, 1, 1, 1), ("conv1.4", 32)),
            (("conv1.6", 32, 64, 3, 1, 1, 1), ("bn1", 64))]


def block_specs(arch):
    """The residual blocks of `arch` as plain data (no GPU, no arenas): one dict per block with
    convs: [(name, cin, cout, k, stride, pad, groups)], bns: [(name, channels)], down: None or ((conv tuple), (bn tuple)),
    se: None or (name, channels, reduced channels).  D variants only: the shortcut is Sequential(pool or Identity, conv, bn) --
    its convolution is 1x1 / stride 1 under the names downsample.1 / downsample.2 -- and every dict has pool: True where the
    shortcut starts with the 2x2 average pool (the stride-2 blocks), False elsewhere."""
    block, layers, cardinality, base_width = ARCHS[arch][:4]
    se = has_se(arch)
    deep = is_d(arch)
    expansion = 4 if block == "bottleneck" else 1
    specs = []
    inplanes = 64
    for li, (planes, nblocks) in enumerate(zip([64, 128, 256, 512], layers)):
        for bi in range(nblocks):
            stride = 2 if (bi == 0 and li > 0) else 1
            name = f"layer{li + 1}.{bi}"
            outplanes = planes * expansion
            if block == "bottleneck":
                width = int(math.floor(planes * base_width / 64)) * cardinality
                convs = [(f"{name}.conv1", inplanes, width, 1, 1, 0, 1),
                         (f"{name}.conv2", width, width, 3, stride, 1, cardinality),
                         (f"{name}.conv3", width, outplanes, 1, 1, 0, 1)]
                bns = [(f"{name}.bn1", width), (f"{name}.bn2", width), (f"{name}.bn3", outplanes)]
            else:
                convs = [(f"{name}.conv1", inplanes, planes, 3, stride, 1, 1),
                         (f"{name}.conv2", planes, planes, 3, 1, 1, 1)]
                bns = [(f"{name}.bn1", planes), (f"{name}.bn2", planes)]
            down = None
            if (stride != 1 or inplanes != outplanes) and deep:
                down = ((f"{name}.downsample.1", inplanes, outplanes, 1, 1, 0, 1), (f"{name}.downsample.2", outplanes))
            elif stride != 1 or inplanes != outplanes:
                down = ((f"{name}.downsample.0", inplanes, outplanes, 1, stride, 0, 1), (f"{name}.downsample.1", outplanes))
            specs.append({"name": name, "stride": stride, "convs": convs, "bns": bns, "down": down,
                          "se": (f"{name}.se", outplanes, outplanes // SE_REDUCTION) if se else None})
            if deep:
                specs[-1]["pool"] = down is not None and stride != 1
            inplanes = outplanes
    return specs


def param_shapes(arch, num_classes=1000):
    """[(parameter name, torch shape)] of `arch` in module order, from ARCHS alone (what state_dict() / the arenas hold)."""
    def bn(name, c):
        return [(name + ".weight", (c,)), (name + ".bias", (c,))]

    def conv(name, cin, cout, k, stride, pad, groups):
        return [(name + ".weight", (cout, cin // groups, k, k))]

    out = []
    for c, b in stem_specs(arch):
        out += conv(*c) + bn(*b)
    feat = 64
    for blk in block_specs(arch):
        for c, b in zip(blk["convs"], blk["bns"]):
            out += conv(*c) + bn(*b)
        if blk["se"] is not None:
            out += se_shapes(*blk["se"])
        if blk["down"] is not None:
            out += conv(*blk["down"][0]) + bn(*blk["down"][1])
        feat = blk["convs"][-1][2]
    return out + [("fc.weight", (num_classes, feat)), ("fc.bias", (num_classes,))]


def se_shapes(name, c, rd):
    """The four tensors of a block's SE module (two 1x1 nn.Conv2d with bias), in module order."""
    return [(name + ".fc1.weight", (rd, c, 1, 1)), (name + ".fc1.bias", (rd,)),
            (name + ".fc2.weight", (c, rd, 1, 1)), (name + ".fc2.bias", (c,))]


class _SE:
    """Squeeze-and-excitation record: fc1 [rd][C] + bias, fc2 [C][rd] + bias, fp32 in the parameter arena in torch layout.  The
    excite kernels read the fp32 masters.  The bf16 shadow arena mirrors the whole parameter arena, so it holds a slice for these
    tensors too (written by the optimizer kernel with every other element); nothing reads it, and there is no transposed copy."""

    def __init__(self, name, c, rd):
        self.name, self.c, self.rd = name, c, rd
        self.w1 = self.b1 = self.w2 = self.b2 = None  # arena.Param


class ResNet(BatchNormModel):
    """HIP ResNet. `model(x)` runs the forward and returns bf16 logits [B, num_classes] (a view)."""
    bn_width = 2048     # layer4 of a bottleneck model

    def __init__(self, arch="resnet50", num_classes=1000, device="cuda", zero_init_last=True, seed=None):
        super().__init__(arch, num_classes, device)
        self._fold_dirty = True
        # eval forwards use BatchNorm-folded filters (ICAMD_EVAL_FOLD=0 keeps the separate BatchNorm pass)
        self.fold_eval = os.environ.get("ICAMD_EVAL_FOLD", "1") != "0"
        block = ARCHS[arch][0]
        self.block = block
        self.se = has_se(arch)
        self.deep = is_d(arch)
        self.expansion = 4 if block == "bottleneck" else 1
        self._build_graph()
        self._build_arenas()
        self.wgrad_side_stream = True   # bench.py turns this off for its per-kernel timing pass
        self.init_weights(zero_init_last=zero_init_last, seed=seed)

    # ------------------------------------------------------------------ structure
    def _build_graph(self):
        self.convs, self.bns = [], []
        # The stem as conv + BatchNorm pairs: the 7x7 / stride 2 one, or the deep stem's three 3x3 ones.  The 7x7 filters live as
        # [64][8][8][4] (row 7, column 7, channel 3 zero): the layout icamd_stem7x7s2_fwd / _wgrad reduce over, on the [N][H][W+8][4]
        # image icamd_pack_input_rgb4 writes.  The deep stem's first convolution reads the 8-channel packed image (icamd_pack_input)
        # on the general entries, the other two are the thin 3x3 problems.  stem_conv is what reads the image; stem_bn is bn1, whose
        # apply is fused with the max-pool
        self.stem_pairs = []
        for (n, cin, cout, k, st, pad, g), (bn_name, bn_c) in stem_specs(self.arch):
            conv = self._conv(n, cin, cout, k, st, pad, cin_p=(4 if k == 7 else 8) if cin == 3 else None, k_p=8 if k == 7 else None)
            conv.stem7, conv.thin = k == 7, cin == 32
            self.stem_pairs.append((conv, self._bn(bn_name, bn_c)))
        self.stem_conv = self.stem_pairs[0][0]
        self.stem_bn = self.stem_pairs[-1][1]
        self.blocks = []
        inplanes = 64
        for spec in block_specs(self.arch):
            blk = {"name": spec["name"], "stride": spec["stride"]}
            # (record order: the block's convolutions, its BatchNorms, then the shortcut pair -- as before the specs existed)
            blk["convs"] = [self._conv(n, cin, cout, k, st, pad, groups=g) for n, cin, cout, k, st, pad, g in spec["convs"]]
            blk["bns"] = [self._bn(n, c) for n, c in spec["bns"]]
            if spec["se"] is not None:
                blk["se"] = _SE(*spec["se"])
            if spec["down"] is not None:
                (n, cin, cout, k, st, pad, g), (bn_name, bn_c) = spec["down"]
                blk["down_conv"] = self._conv(n, cin, cout, k, st, pad, groups=g)
                blk["down_bn"] = self._bn(bn_name, bn_c)
            if spec.get("pool"):
                blk["pool"] = True     # 2x2 average pool in front of the shortcut convolution (which is then 1x1 / stride 1)
            self.blocks.append(blk)
            inplanes = spec["convs"][-1][2]
        self.feat_dim = inplanes
        self.fc = self._conv("fc", inplanes, self.num_classes, 1, 1, 0, cout_p=self.ncls_p, bias=True)

    def _conv(self, name, cin, cout, k, stride, pad, cin_p=None, cout_p=None, bias=False, k_p=None, groups=1):
        c = _Conv(name, cin, cout, k, stride, pad, cin_p, cout_p, bias, k_p, groups)
        self.convs.append(c)
        return c

    def _bn(self, name, c):
        b = _BN(name, c)
        self.bns.append(b)
        return b

    def conv_bn_pairs(self):
        """[(conv, bn)] in module order: the stem, then each block's convolutions, then its shortcut pair."""
        pairs = list(self.stem_pairs)
        for blk in self.blocks:
            pairs += zip(blk["convs"], blk["bns"])
            if "down_conv" in blk:
                pairs.append((blk["down_conv"], blk["down_bn"]))
        return pairs

    def _build_arenas(self):
        # parameter order = timm/torchvision module order (conv, bn, ..., se, downsample, fc)
        order = [m for pair in self.stem_pairs for m in pair]
        for blk in self.blocks:
            order += [m for pair in zip(blk["convs"], blk["bns"]) for m in pair]
            if "se" in blk:
                order.append(blk["se"])
            if "down_conv" in blk:
                order += [blk["down_conv"], blk["down_bn"]]
        order.append(self.fc)
        # transposed filters for the data-gradient kernels (every conv except the stem's first and the grouped ones, whose data
        # gradient reads the forward layout; so does the thin route of the deep stem's other two, but those keep their 2 x 18 KB:
        # ICAMD_STEM_THIN=0 and images too wide for the thin kernels' LDS tile run on icamd_conv2d_dgrad)
        self._layout_arenas(order, [(m, m.cout_p, m.k * m.k, m.cin_p) for m in self.convs
                                    if m is not self.stem_conv and m.groups == 1])

    def _add_record(self, add, se):
        """The one kind of record of its own: a block's squeeze-and-excitation module."""
        (n1, s1), (nb1, sb1), (n2, s2), (nb2, sb2) = se_shapes(se.name, se.c, se.rd)
        se.w1 = add(n1, s1, "conv", (se.rd, 1, 1, se.c))     # [rd][1][1][C] is torch's (rd, C, 1, 1) memory
        se.b1 = add(nb1, sb1, "vec", sb1)
        se.w2 = add(n2, s2, "conv", (se.c, 1, 1, se.rd))
        se.b2 = add(nb2, sb2, "vec", sb2)

    # ------------------------------------------------------------------ parameters / state_dict
    def init_weights(self, zero_init_last=True, seed=None):
        """timm ResNet.init_weights: Kaiming-normal (fan_out, relu) convs, BN weight 1 / bias 0, zero-init of the
        last BN weight of each residual block, nn.Linear default init for the classifier; SE convolutions as every nn.Conv2d."""
        g = torch.Generator()
        if seed is not None:
            g.manual_seed(seed)
        else:
            g.manual_seed(torch.initial_seed() % (2 ** 63))
        sd = OrderedDict()
        for name, p in self.params.items():
            if p.kind == "conv":
                cout, cin, k, _ = p.torch_shape
                std = math.sqrt(2.0 / (cout * k * k))
                sd[name] = torch.randn(p.torch_shape, generator=g) * std
            elif name == "fc.weight":
                bound = 1.0 / math.sqrt(p.torch_shape[1])
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) * bound
            elif name == "fc.bias":
                bound = 1.0 / math.sqrt(self.feat_dim)
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) * bound
            elif ".se." in name:      # the biases of the SE convolutions keep nn.Conv2d's default: U(+-1 / sqrt(fan_in))
                fan_in = self.params[name[:-len("bias")] + "weight"].torch_shape[1]
                sd[name] = (torch.rand(p.torch_shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
            elif name.endswith(".weight"):
                sd[name] = torch.ones(p.torch_shape)
            else:
                sd[name] = torch.zeros(p.torch_shape)
        if zero_init_last:
            for blk in self.blocks:
                sd[blk["bns"][-1].name + ".weight"].zero_()
        self._fresh_buffers(sd)
        self.load_state_dict(sd)

    def _load_buffers(self, sd):
        super()._load_buffers(sd)
        self._fold_dirty = True

    def train(self, mode=True):
        self._fold_dirty = True     # parameters / running statistics may move before the next eval forward
        return super().train(mode)

    # ------------------------------------------------------------------ inference form
    def fold_batchnorm(self):
        """Eval fast path: fold every BatchNorm (running statistics) into the bf16 filters of the convolution in front
        of it, so an eval forward is one kernel per convolution (bias = BN shift, residual add and ReLU in the epilogue)
        with no BatchNorm pass over the activations.  Re-done whenever the mode, the weights or the EMA changed."""
        dev = self.device
        if getattr(self, "shadow_eval", None) is None:
            self.shadow_eval = torch.empty_like(self.shadow)
            self.eval_shift = torch.zeros(sum(b.c for b in self.bns), dtype=torch.float32, device=dev)
            off = 0
            for b in self.bns:
                b.shift_offset = off
                off += b.c
        s = hip.stream_ptr()
        for conv, bn in self.conv_bn_pairs():
            rm = self.buffer_arena.data_ptr() + 4 * bn.buf_offset
            hip.check(self.lib.icamd_bn_fold_filters(self._pf(conv.w), self._pf(bn.weight), self._pf(bn.bias), rm,
                                                     rm + 4 * bn.c, BN_EPS, conv.cout_p, conv.w.numel // conv.cout_p,
                                                     self.shadow_eval.data_ptr() + 2 * conv.w.offset,
                                                     self.eval_shift.data_ptr() + 4 * bn.shift_offset, s), bn.name)
        self._fold_dirty = False

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, N, H, W):
        key = (N, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev = self.device
        lib = self.lib
        ws = {"N": N, "H": H, "W": W}

        def act(n, h, w, c):
            return torch.empty(n, h, w, c, dtype=torch.bfloat16, device=dev)

        # The image: 8 channels packed, or for the 7x7 stem the rgb4 layout (3 + 5 zero columns per row); there an odd width gets one
        # more zero column -- part of the convolution's own padding -- and the stem kernels run on the even width Ws.
        # stem_in[i] / stem_y[i] = input / raw output of the i-th stem convolution, stem_a[i] = its BatchNorm + ReLU output (the last
        # one's goes through the fused max-pool and is never stored: y0 is stem_y[-1]); the batch statistics sit in the stat arena
        # (_stats(bn))
        rgb4 = self.stem_conv.stem7
        Ws = W + (W & 1) if rgb4 else W
        ws["Ws"] = Ws
        ws["x8"] = act(N, H, Ws + 8, 4) if rgb4 else act(N, H, W, 8)
        ws["stem_y"], ws["stem_a"], ws["stem_in"], ws["stem_hw"] = [], [], [ws["x8"]], []
        max_act, max_stats, max_wg, max_bnb = ws["x8"].numel(), 0, 0, 0
        sh_, sw_ = H, Ws
        for i, (conv, bn) in enumerate(self.stem_pairs):
            d0 = conv.desc(N, sh_, sw_)
            ws["stem_hw"].append((sh_, sw_))
            ws["stem_y"].append(act(N, d0.OH, d0.OW, conv.cout_p))
            if i + 1 < len(self.stem_pairs):
                ws["stem_a"].append(act(N, d0.OH, d0.OW, conv.cout_p))
                ws["stem_in"].append(ws["stem_a"][-1])
            max_act = max(max_act, ws["stem_y"][-1].numel())
            max_stats = max(max_stats, self._stats_rows(conv, d0) * 2 * conv.cout_p)
            max_wg = max(max_wg, self._wgrad_workspace_bytes(conv, d0))
            max_bnb = max(max_bnb, lib.icamd_bn_bwd_workspace_bytes(N * d0.OH * d0.OW, conv.cout_p))
            sh_, sw_ = d0.OH, d0.OW
        ws["y0"] = ws["stem_y"][-1]
        ws["a0"] = act(N, d0.OH, d0.OW, 64)
        PH, PW = (d0.OH - 1) // 2 + 1, (d0.OW - 1) // 2 + 1
        ws["p0"] = act(N, PH, PW, 64)
        ws["p0_idx"] = torch.empty(N, PH, PW, 64, dtype=torch.uint8, device=dev)
        h, w = PH, PW
        blocks_ws = []
        max_se = max_fused = 0
        for blk in self.blocks:
            b = {}
            ih, iw = h, w
            ys, acts, launches = [], [], []
            for conv in blk["convs"]:
                d = conv.desc(N, ih, iw)
                ys.append(act(N, d.OH, d.OW, conv.cout_p))
                acts.append(act(N, d.OH, d.OW, conv.cout_p))
                max_act = max(max_act, ys[-1].numel())
                launches.append((conv, d))
                ih, iw = d.OH, d.OW
            b["y"], b["a"] = ys, acts
            b["hw"] = [(d.IH, d.IW) for _, d in launches]     # input size of each convolution
            b["mask"] = torch.empty(acts[-1].numel() // 8, dtype=torch.uint8, device=dev)   # ReLU mask of the block output
            if "down_conv" in blk:
                sh_, sw_ = h, w
                if blk.get("pool"):
                    sh_, sw_ = (h + 1) // 2, (w + 1) // 2
                    b["xp"] = act(N, sh_, sw_, blk["down_conv"].cin_p)     # pooled block input: what the shortcut convolution reads
                b["short_hw"] = (sh_, sw_)
                dd = blk["down_conv"].desc(N, sh_, sw_)
                b["yd"] = act(N, dd.OH, dd.OW, blk["down_conv"].cout_p)
                b["ad"] = act(N, dd.OH, dd.OW, blk["down_conv"].cout_p)
                launches.append((blk["down_conv"], dd))
            for conv, d in launches:      # every convolution of the block, shortcut included
                if conv.groups > 1 and not lib.icamd_gconv3x3_supported(ctypes.byref(d), conv.groups):
                    raise hip.IcamdError(f"{conv.name}: no grouped 3x3 kernel for {d.key()} with {conv.groups} groups")
                max_stats = max(max_stats, self._stats_rows(conv, d) * 2 * conv.cout_p)
                max_wg = max(max_wg, self._wgrad_workspace_bytes(conv, d))
                max_bnb = max(max_bnb, lib.icamd_bn_bwd_workspace_bytes(N * d.OH * d.OW, conv.cout_p))
            if self.block == "bottleneck" and "se" not in blk:
                # what the fused convolution + BatchNorm backward may take (_bwd_last_bn): the last convolution and a stride-1 shortcut
                for conv, d in launches[len(ys) - 1:]:
                    if conv.stride == 1 and lib.icamd_conv1x1_bn_bwd_fused_supported(ctypes.byref(d)):
                        max_fused = max(max_fused, lib.icamd_conv1x1_bn_bwd_fused_workspace_bytes(ctypes.byref(d)))
            if "se" in blk:
                se = blk["se"]
                hw_out = ih * iw
                for key, width in (("se_ysum", se.c), ("se_s", se.c), ("se_h", se.rd), ("se_e", se.c)):
                    b[key] = torch.empty(N, width, dtype=torch.float32, device=dev)
                max_se = max(max_se, lib.icamd_se_squeeze_workspace_bytes(N, hw_out, se.c),
                             lib.icamd_se_bn_bwd_workspace_bytes(N, hw_out, se.c))
            blocks_ws.append(b)
            h, w = ih, iw
        ws["blocks"] = blocks_ws
        ws["final_hw"] = (h, w)
        ws["pooled"] = torch.empty(N, self.feat_dim, dtype=torch.bfloat16, device=dev)
        ws["logits"] = torch.zeros(N, self.ncls_p, dtype=torch.bfloat16, device=dev)
        dfc = self.fc.desc(N, 1, 1)
        max_wg = max(max_wg, self._wgrad_workspace_bytes(self.fc, dfc))
        ws["stats"] = torch.empty(max_stats, dtype=torch.float32, device=dev)
        self._bn_workspaces(ws)
        ws["wgrad_ws"] = torch.empty(max_wg, dtype=torch.uint8, device=dev)
        ws["wgrad_ws_bytes"] = max_wg
        ws["bnb_part"] = torch.empty(max_stats + 4 * 2 * 2048, dtype=torch.float32, device=dev)
        ws["bna_ws_bytes"] = lib.icamd_bn_bwd_apply_workspace_bytes(2048)
        ws["bna_ws"] = torch.zeros(ws["bna_ws_bytes"], dtype=torch.uint8, device=dev)
        ws["bnb_ws"] = torch.zeros(max_bnb, dtype=torch.uint8, device=dev)
        ws["bnb_ws2"] = torch.zeros(max_bnb, dtype=torch.uint8, device=dev)   # second BatchNorm of icamd_bn_bwd_dual
        ws["bnb_ws_bytes"] = max_bnb
        ws["max_act"] = max_act
        if max_fused > 0:     # slab workspace of icamd_conv1x1_bn_bwd_fused (main stream; the side stream's wgrads own wgrad_ws)
            ws["fused_ws"] = torch.empty(max_fused, dtype=torch.uint8, device=dev)
            ws["fused_ws_bytes"] = max_fused
        if self.se:
            ws["se_ws"] = torch.empty(max_se, dtype=torch.uint8, device=dev)
            ws["se_ws_bytes"] = max_se
            ws["se_ident"] = torch.cat([torch.ones(4096, device=dev), torch.zeros(4096, device=dev)])   # scale 1 | shift 0
        # loss / metric scratch
        ws["loss_rows"] = torch.empty(N, dtype=torch.float32, device=dev)
        ws["pred"] = torch.empty(N, dtype=torch.int32, device=dev)
        ws["dlogits"] = torch.zeros(N, self.ncls_p, dtype=torch.bfloat16, device=dev)
        ws["dpooled"] = torch.empty(N, self.feat_dim, dtype=torch.bfloat16, device=dev)
        self._ws[key] = ws
        return ws

    def _grad_buffers(self, ws):
        """Activation-sized scratch buffers shared by the whole backward pass (allocated on first use): D0, D1, T, DA and a
        pool of four conv-output-gradient buffers (the fused variant uses the first seven as before)."""
        if "gbuf" not in ws:
            n = ws["max_act"]
            ws["gbuf"] = [torch.empty(n, dtype=torch.bfloat16, device=self.device) for _ in range(8)]
        return ws["gbuf"]

    def _grad_view(self, ws, ptr, like):
        """The scratch buffer of _grad_buffers that starts at `ptr`, viewed with the shape of the activation `like`."""
        for buf in ws["gbuf"]:
            if buf.data_ptr() == ptr:
                return buf[:like.numel()].view(like.shape)
        raise KeyError(ptr)

    # ------------------------------------------------------------------ primitive wrappers
    # The stem / grouped / dense dispatch on a convolution, once per kind of launch.  `d` is conv.desc(...) of the input shape.
    def _thin(self, conv, d, op):
        """Does `op` ("fwd", "dgrad", "wgrad") of this convolution run on the thin 3x3 kernels?"""
        return conv.thin and _STEM_THIN[op] and bool(self.lib.icamd_conv3x3_thin_supported(ctypes.byref(d)))

    def _stats_rows(self, conv, d):
        """Rows of the BatchNorm partial sums the forward of `conv` writes."""
        if self._thin(conv, d, "fwd"):
            return self.lib.icamd_conv3x3_thin_stats_rows(ctypes.byref(d))
        return self.lib.icamd_conv2d_stats_rows(ctypes.byref(d))

    def _conv_fwd(self, conv, d, x, w, y, s, stats=None, shift=None, residual=None, relu=0):
        """y = conv(x) with filters `w`.  Training form (shift None): the raw output, BatchNorm statistic rows to `stats`.  Folded
        eval form: + shift (+ residual) (+ ReLU) in the epilogue."""
        lib = self.lib
        if conv.stem7:
            rc = lib.icamd_stem7x7s2_fwd(x, w, y, shift, stats, relu, d.N, d.IH, d.IW, conv.cout_p, s)
        elif self._thin(conv, d, "fwd"):
            assert residual is None
            rc = lib.icamd_conv3x3_thin_fwd(ctypes.byref(d), x, w, y, shift, stats, relu, s)
        elif conv.groups > 1 and shift is None:
            rc = lib.icamd_gconv3x3_fwd(ctypes.byref(d), conv.groups, x, w, y, stats, s)
        elif conv.groups > 1:
            assert residual is None
            rc = lib.icamd_gconv3x3_fwd_act(ctypes.byref(d), conv.groups, x, w, y, shift, relu, s)
        elif shift is None:
            rc = lib.icamd_conv2d_fwd(ctypes.byref(d), x, w, y, None, None, stats, s)
        else:
            rc = lib.icamd_conv2d_fwd_act(ctypes.byref(d), x, w, y, shift, residual, relu, s)
        hip.check(rc, conv.name)

    def _wgrad_workspace_bytes(self, conv, d):
        lib = self.lib
        if conv.stem7:
            return lib.icamd_stem7x7s2_wgrad_workspace_bytes(d.N, d.IH, d.IW, conv.cout_p)
        if self._thin(conv, d, "wgrad"):
            return lib.icamd_conv3x3_thin_wgrad_workspace_bytes(ctypes.byref(d))
        if conv.groups > 1:
            return lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), conv.groups)
        return lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))

    def _wgrad(self, conv, d, x, dy, acc, wsp, wsb, s):
        lib = self.lib
        if conv.stem7:
            rc = lib.icamd_stem7x7s2_wgrad(x, dy, self._gf(conv.w), acc, wsp, wsb, d.N, d.IH, d.IW, conv.cout_p, s)
        elif self._thin(conv, d, "wgrad"):
            rc = lib.icamd_conv3x3_thin_wgrad(ctypes.byref(d), x, dy, self._gf(conv.w), acc, wsp, wsb, s)
        elif conv.groups > 1:
            rc = lib.icamd_gconv3x3_wgrad(ctypes.byref(d), conv.groups, x, dy, self._gf(conv.w), acc, wsp, wsb, s)
        else:
            rc = lib.icamd_conv2d_wgrad(ctypes.byref(d), x, dy, self._gf(conv.w), acc, wsp, wsb, s)
        hip.check(rc, conv.name + " wgrad")

    def _dgrad(self, conv, d, dy, dx, addend, addend_bits, s):
        """dx = data gradient of conv (+ addend, where the 1-bit mask `addend_bits` is set when given)."""
        if self._thin(conv, d, "dgrad"):
            assert addend is None
            rc = self.lib.icamd_conv3x3_thin_dgrad(ctypes.byref(d), dy, self._w(conv), dx, s)
        elif conv.groups > 1:
            assert addend is None
            rc = self.lib.icamd_gconv3x3_dgrad(ctypes.byref(d), conv.groups, dy, self._w(conv), dx, s)
        else:
            rc = self.lib.icamd_conv2d_dgrad(ctypes.byref(d), dy, self._wt(conv), dx, addend, addend_bits, s)
        hip.check(rc, conv.name + " dgrad")

    # The per-layer primitives of the forward walk.  `fw` is _forward_begin's record; x, y, out are activation tensors, residual and
    # mask pointers (or None), res_bn the (scale, shift) pointers of a BatchNorm to apply to the residual on the way (or None).
    def _conv_folded(self, fw, conv, bn, x, ih, iw, out, relu, residual=None):
        """Folded form: out = act(conv(x) + shift (+ residual)) on the BatchNorm-folded filters, one launch."""
        d = conv.desc(fw.N, ih, iw)
        self._conv_fwd(conv, d, x.data_ptr(), self.shadow_eval.data_ptr() + 2 * conv.w.offset, out.data_ptr(), fw.s,
                       shift=self.eval_shift.data_ptr() + 4 * bn.shift_offset, residual=residual, relu=int(relu))
        return d

    def _conv_bn_coeffs(self, fw, conv, bn, d):
        """(scale, shift) of `bn` over the raw output of `conv`, whose forward just ran on descriptor `d`."""
        rows = self._stats_rows(conv, d) if fw.training else 0
        return self._bn_coeffs(fw, bn, rows, fw.N * d.OH * d.OW)

    def _conv_coeffs(self, fw, conv, bn, x, ih, iw, y):
        """y = conv(x) with what turns y into the BatchNorm output, always as (d, scale, shift), for a caller that fuses the apply
        into a kernel of its own.  Folded form: the filters carry the BatchNorm, so y is its output already and the coefficients
        are the identity (SE models, the only ones that ask: ws["se_ident"])."""
        if fw.folded:
            one = fw.ws["se_ident"].data_ptr()
            return self._conv_folded(fw, conv, bn, x, ih, iw, y, False), one, one + 4 * 4096
        d = conv.desc(fw.N, ih, iw)
        self._conv_fwd(conv, d, x.data_ptr(), self._w(conv), y.data_ptr(), fw.s, stats=fw.stats)
        return (d,) + self._conv_bn_coeffs(fw, conv, bn, d)

    def _bn_apply(self, fw, bn, y, scale, shift, out, relu, residual=None, res_bn=None, mask=None):
        """out = act(y * scale + shift (+ residual, through its own BatchNorm where res_bn is given)); mask: the ReLU bits."""
        if res_bn is not None:   # residual = raw shortcut conv output; its BatchNorm is applied inside the same pass
            rc = self.lib.icamd_bn_apply_res_bn(y.data_ptr(), scale, shift, residual, res_bn[0], res_bn[1], out.data_ptr(), mask,
                                                y.numel(), bn.c, int(relu), fw.s)
        else:
            rc = self.lib.icamd_bn_apply(y.data_ptr(), scale, shift, residual, out.data_ptr(), mask, y.numel(), bn.c, int(relu), fw.s)
        hip.check(rc, bn.name)

    def _conv_bn_act(self, fw, conv, bn, x, ih, iw, y, out, relu, residual=None, res_bn=None, mask=None):
        """out = act(bn(conv(x)) (+ residual)): the folded convolution alone, or convolution + coefficients into y, then the apply."""
        if fw.folded:
            return self._conv_folded(fw, conv, bn, x, ih, iw, out, relu, residual)
        d, scale, shift = self._conv_coeffs(fw, conv, bn, x, ih, iw, y)
        self._bn_apply(fw, bn, y, scale, shift, out, relu, residual, res_bn, mask)
        return d

    def _se_tail(self, fw, blk, b, scale, shift, res, res_bn, HW):
        """The SE block's tail on the raw output y of its last convolution: per-sample sums of y, the excitation from them, then
        out = relu((y * scale + shift) * e[n, c] + shortcut) in one pass (the BatchNorm output itself is never stored)."""
        lib, ws, N, s, se, y = self.lib, fw.ws, fw.N, fw.s, blk["se"], b["y"][-1]
        hip.check(lib.icamd_se_squeeze(y.data_ptr(), b["se_ysum"].data_ptr(), N, HW, se.c, ws["se_ws"].data_ptr(),
                                       ws["se_ws_bytes"], s), se.name + " squeeze")
        hip.check(lib.icamd_se_excite_fwd(b["se_ysum"].data_ptr(), scale, shift, 1.0 / HW, self._pf(se.w1), self._pf(se.b1),
                                          self._pf(se.w2), self._pf(se.b2), b["se_s"].data_ptr(), b["se_h"].data_ptr(),
                                          b["se_e"].data_ptr(), N, se.c, se.rd, s), se.name + " excite")
        hip.check(lib.icamd_se_bn_apply(y.data_ptr(), scale, shift, b["se_e"].data_ptr(), res, res_bn[0] if res_bn else None,
                                        res_bn[1] if res_bn else None, b["a"][-1].data_ptr(),
                                        b["mask"].data_ptr() if fw.training else None, N, HW, se.c, 1, s), se.name + " apply")

    # ------------------------------------------------------------------ forward
    def pack(self, x_nchw, mix=None):
        """fp32 NCHW device tensor -> packed NHWC bf16 (channels zero-padded to 8), with optional mixup/cutmix."""
        N, C, H, W = x_nchw.shape
        # the deep stem's first convolution reads the plain 8-channel packed image, the 7x7 stem the rgb4 layout
        return self._pack_input(self._workspace(N, H, W), x_nchw, mix, rgb4=self.stem_conv.stem7)

    def forward_packed(self, ws, logits_only=False):   # logits_only: accepted for interface parity (BatchNorm needs every conv output)
        """Stem, residual blocks, average pool + classifier -> ws["logits"], in one of three forms: training (batch statistics), eval
        with running statistics, or -- fold_eval, the default -- eval on BatchNorm-folded filters, one kernel per convolution."""
        fw = self._forward_begin(ws)
        x, h, w = self._fwd_stem(fw)
        pending = None
        for bi in range(len(self.blocks)):
            x, h, w, pending = self._fwd_block(fw, bi, x, h, w, pending)
        return self._fwd_head(fw, x, h, w)

    def _forward_begin(self, ws):
        """What the steps of one forward pass share."""
        s = hip.stream_ptr()
        folded = not self.training and self.fold_eval
        if folded and self._fold_dirty:
            self.fold_batchnorm()
        if self.training:
            self.num_batches_tracked += 1
        return SimpleNamespace(ws=ws, N=ws["N"], s=s, training=self.training, folded=folded,
                               stats=ws["stats"].data_ptr() if self.training else None)

    def _fwd_stem(self, fw):
        """conv -> BatchNorm + ReLU per stem pair; the last pair's BatchNorm + ReLU runs in one pass with the max-pool over the conv
        output (the 112x112 activation is never stored: backward recomputes the ReLU mask from y0 and the pooling argmax is
        recorded).  Folded: the last convolution applies its ReLU and a plain max-pool follows.  Returns the pooled x, h, w."""
        lib, ws, N, s = self.lib, fw.ws, fw.N, fw.s
        for i, (conv, bn) in enumerate(self.stem_pairs[:-1]):
            self._conv_bn_act(fw, conv, bn, ws["stem_in"][i], *ws["stem_hw"][i], ws["stem_y"][i], ws["stem_a"][i], True)
        conv, bn = self.stem_pairs[-1]
        if fw.folded:
            d = self._conv_folded(fw, conv, bn, ws["stem_in"][-1], *ws["stem_hw"][-1], ws["a0"], True)
            hip.check(lib.icamd_maxpool3x3s2_fwd(ws["a0"].data_ptr(), ws["p0"].data_ptr(), None, N, d.OH, d.OW, 64, s), "maxpool")
        else:
            d, scale, shift = self._conv_coeffs(fw, conv, bn, ws["stem_in"][-1], *ws["stem_hw"][-1], ws["y0"])
            hip.check(lib.icamd_bn_relu_maxpool3x3s2_fwd(ws["y0"].data_ptr(), scale, shift, ws["p0"].data_ptr(),
                                                         ws["p0_idx"].data_ptr() if fw.training else None, N, d.OH, d.OW, 64, s),
                      "stem bn+relu+maxpool")
        return ws["p0"], ws["p0"].shape[1], ws["p0"].shape[2]

    def _fwd_shortcut(self, fw, blk, b, x, h, w):
        """The block's residual as (tensor, res_bn).  A projection shortcut reads the block input or (D variants, stride-2 blocks)
        its 2x2 average b["xp"].  Training: convolution + statistics only -- its BatchNorm is applied inside the block's last
        BatchNorm pass (res_bn), the normalised shortcut is never stored (backward needs yd and the block mask, not it)."""
        if "down_conv" not in blk:
            return x, None
        dc, dbn = blk["down_conv"], blk["down_bn"]
        if blk.get("pool"):
            hip.check(self.lib.icamd_avgpool2x2_fwd(x.data_ptr(), b["xp"].data_ptr(), fw.N, h, w, dc.cin_p, fw.s),
                      blk["name"] + " shortcut pool")
            x = b["xp"]
        if fw.training:
            _, scale, shift = self._conv_coeffs(fw, dc, dbn, x, *b["short_hw"], b["yd"])
            return b["yd"], (scale, shift)
        self._conv_bn_act(fw, dc, dbn, x, *b["short_hw"], b["yd"], b["ad"], False)
        return b["ad"], None

    def _defers_apply(self, fw, bi, h, w):
        """May block bi's last BatchNorm apply (+ shortcut + ReLU + mask) wait for the next block's first convolution
        (icamd_bn_apply_conv1x1_fused: the block output is written once and multiplied while it is in LDS instead of being
        re-read by that convolution)?  h, w: the size of the block output."""
        if not (fw.training and self.block == "bottleneck" and bi + 1 < len(self.blocks)):
            return False
        dn = self.blocks[bi + 1]["convs"][0].desc(fw.N, h, w)
        return bool(self.lib.icamd_bn_apply_conv1x1_fused_supported(ctypes.byref(dn)))

    def _fwd_block(self, fw, bi, x, h, w, pending):
        """One residual block on its input x (h x w).  pending: None, or the previous block's deferred last apply -- then x is the
        buffer that apply will fill, and it runs inside this block's first convolution.  Returns the block output, its size, and
        this block's own deferred apply or None."""
        N, s = fw.N, fw.s
        blk, b = self.blocks[bi], fw.ws["blocks"][bi]
        b["in"], b["in_hw"] = x, (h, w)
        convs, bns = blk["convs"], blk["bns"]
        first = 0
        if pending is not None:
            # end of the previous block + this block's conv1 (+ the statistics of its bn1) in one launch, then bn1 as usual
            p, d = pending, convs[0].desc(N, h, w)
            res_scale, res_shift = p.res_bn or (None, None)
            hip.check(self.lib.icamd_bn_apply_conv1x1_fused(ctypes.byref(d), p.y.data_ptr(), p.scale, p.shift, p.residual, res_scale,
                                                            res_shift, x.data_ptr(), p.mask, self._w(convs[0]), b["y"][0].data_ptr(),
                                                            fw.stats, s), p.bn.name + " apply + " + convs[0].name)
            self._bn_apply(fw, bns[0], b["y"][0], *self._conv_bn_coeffs(fw, convs[0], bns[0], d), b["a"][0], True)
            x, h, w, first = b["a"][0], d.OH, d.OW, 1
        idn, res_bn = self._fwd_shortcut(fw, blk, b, b["in"], *b["in_hw"])
        mask = b["mask"].data_ptr() if fw.training else None
        deferred = None
        for i in range(first, len(convs)):
            conv, bn, y, out = convs[i], bns[i], b["y"][i], b["a"][i]
            if i < len(convs) - 1:
                d = self._conv_bn_act(fw, conv, bn, x, h, w, y, out, True)
            elif "se" in blk:
                # the gated apply takes the coefficients: no deferral into the next block
                d, scale, shift = self._conv_coeffs(fw, conv, bn, x, h, w, y)
                self._se_tail(fw, blk, b, scale, shift, idn.data_ptr(), res_bn, d.OH * d.OW)
            elif self._defers_apply(fw, bi, h, w):
                # convolution + statistics + finalize now; `out` is filled inside the next block's first convolution
                d, scale, shift = self._conv_coeffs(fw, conv, bn, x, h, w, y)
                deferred = SimpleNamespace(bn=bn, y=y, scale=scale, shift=shift, residual=idn.data_ptr(), res_bn=res_bn, mask=mask)
            else:
                d = self._conv_bn_act(fw, conv, bn, x, h, w, y, out, True, idn.data_ptr(), res_bn, mask)
            x, h, w = out, d.OH, d.OW
        return x, h, w, deferred

    # ------------------------------------------------------------------ backward
    def backward_packed(self, ws, accumulate=False):
        """Backward from ws['dlogits'] (bf16 [N, ncls_p]); fills the flat fp32 gradient arena.
        Gradients become final in reverse layer order; `grad_ready_hook(lo, hi, events)` is called as ranges complete (hi None:
        to the end of the range of the previous call; events: what a consumer on another stream waits for besides the main one).

        Weight gradients run on a second HIP stream (streams.SideLane; ICAMD_WGRAD_STREAM=0 keeps one stream): a layer's wgrad
        only needs that layer's output gradient and its saved input, nothing downstream needs its result before the optimizer,
        and it is MFMA/latency-bound while the BatchNorm-backward passes the main stream runs next are HBM-bound -- side by side
        they fill both.  The output-gradient buffers rotate through a small pool so the main stream can run ahead; an
        event per buffer keeps it from overwriting one a pending wgrad still reads."""
        if _FUSED_BNBWD:
            if self.se:
                raise hip.IcamdError("ICAMD_FUSED_BNBWD=1 has no squeeze-and-excitation backward")
            if self.deep:
                raise hip.IcamdError("ICAMD_FUSED_BNBWD=1 has no average-pool shortcut backward")
            return self._backward_packed_fused(ws, accumulate)
        run = self._backward_begin(ws, accumulate, _WGRAD_STREAM and self.wgrad_side_stream)
        bufs = self._grad_buffers(ws)
        dout, other, run.T, run.DA = (b.data_ptr() for b in bufs[:4])
        run.ypool = itertools.cycle([b.data_ptr() for b in bufs[4:]])
        self._bwd_classifier(run, dout)
        # `fused_rows` > 0: the residual data gradient of the block just done also did pass 1 of the next block's last BatchNorm
        # backward (icamd_conv2d_dgrad_bnred), so `dout` already holds g = that block's masked output gradient and
        # ws["bnb_part"] its partial sums (sum g, sum g*y): the block starts with the apply pass only
        fused_rows = 0
        for bi in range(len(self.blocks) - 1, -1, -1):
            dy, dy2, shortcut_done = self._bwd_last_bn(run, bi, dout, fused_rows)
            dy = self._bwd_inner_convs(run, bi, dy)
            fused_rows = self._bwd_conv1_shortcut(run, bi, dy, dy2, shortcut_done, dout, other)
            if run.hook:
                run.hook(self.blocks[bi]["convs"][0].w.offset, None, run.lane.events())
            dout, other = other, dout
        self._bwd_stem(run, dout, self._next_y(run), _FUSED_POOL_BWD)
        if run.hook:
            run.hook(0, None, run.lane.events())
        run.lane.join()

    def _backward_begin(self, ws, accumulate, side):
        """What the steps of one backward pass share; `side`: weight gradients on the side lane."""
        lane = side_lane(self, "ICAMD_WGRAD_STREAM", True)
        lane.begin(side)
        return SimpleNamespace(ws=ws, N=ws["N"], acc=int(bool(accumulate)), lane=lane, s=lane.main.cuda_stream,
                               hook=self.grad_ready_hook, wsp=ws["wgrad_ws"].data_ptr(), wsb=ws["wgrad_ws_bytes"],
                               bws=ws["bnb_ws"].data_ptr(), bwb=ws["bnb_ws_bytes"])

    def _next_y(self, run):
        """The next output-gradient buffer of the pool, once no pending weight gradient reads it any more."""
        y = next(run.ypool)
        run.lane.before_write(y)
        return y

    def _side_wgrad(self, run, conv, d, x, dy):
        run.lane.launch(lambda st: self._wgrad(conv, d, x, dy, run.acc, run.wsp, run.wsb, st), reads=(dy,))

    def _bn_bwd(self, run, bn, dout, act, y, dy, gout, relu, maskbits=None):
        mean, invstd, scale, shift = self._stats(bn)
        c = bn.c
        hip.check(self.lib.icamd_bn_bwd(dout, act, y.data_ptr(), mean, invstd, scale, shift, self._gf(bn.weight),
                                        self._gf(bn.bias), dy, gout, maskbits, y.numel() // c, c, int(relu), run.acc, run.bws,
                                        run.bwb, run.s), bn.name + " bwd")

    def _fused_conv_bn(self, run, conv, bn, d, partials, nrows, g, y, x, dx, bn_ws, bn_ws_bytes):
        """BatchNorm-backward apply + data gradient + weight gradient of `conv` -> `bn` in one pass over g (already masked) and y
        (round 5, icamd_conv1x1_bn_bwd_fused); main stream, on the slab workspace _workspace sized for it (ws["fused_ws"])."""
        ws = run.ws
        mean, invstd, scale, _ = self._stats(bn)
        hip.check(self.lib.icamd_conv1x1_bn_bwd_fused(ctypes.byref(d), partials, nrows, g, y.data_ptr(), mean, invstd, scale,
                                                 self._gf(bn.weight), self._gf(bn.bias), x, self._wt(conv), dx, self._gf(conv.w),
                                                 run.acc, bn_ws, bn_ws_bytes, ws["fused_ws"].data_ptr(), ws["fused_ws_bytes"], run.s),
                  bn.name + " + " + conv.name + " bwd (fused)")

    def _bwd_classifier(self, run, dout):
        lib, ws, N, s = self.lib, run.ws, run.N, run.s
        dl = ws["dlogits"].data_ptr()
        dfc = self.fc.desc(N, 1, 1)
        self._side_wgrad(run, self.fc, dfc, ws["pooled"].data_ptr(), dl)
        hip.check(lib.icamd_colsum(dl, N, self.ncls_p, self.ncls_p, self._gf(self.fc.b), run.acc, s), "fc bias grad")
        self._dgrad(self.fc, dfc, dl, ws["dpooled"].data_ptr(), None, None, s)
        if run.hook:
            run.hook(self.fc.w.offset, self.n_params, run.lane.events())
        fh, fw = ws["final_hw"]
        hip.check(lib.icamd_avgpool_bwd(ws["dpooled"].data_ptr(), dout, N, fh * fw, self.feat_dim, s), "avgpool bwd")

    def _bwd_last_bn(self, run, bi, dout, fused_rows):
        """Backward of the block's last BatchNorm (+ residual + ReLU): g = dout * [block output > 0] via the 1-bit mask the forward
        stored; g itself is never written: the shortcut consumers re-apply the same bits to `dout`.
        Returns (dy, dy2, shortcut_done).  dy: gradient of the last convolution's output, or None where that convolution's
        backward came out of the same launch (its input's gradient is in run.DA, its filter gradient in the arena).  dy2: the same
        for the shortcut convolution where its BatchNorm was done here.  shortcut_done: the shortcut's filter gradient is done and
        run.T holds its full-size data gradient."""
        lib, ws, N = self.lib, run.ws, run.N
        blk, b = self.blocks[bi], ws["blocks"][bi]
        conv3, bn3, y3 = blk["convs"][-1], blk["bns"][-1], b["y"][-1]
        down = "down_conv" in blk
        mask = b["mask"].data_ptr()
        dy = self._next_y(run)
        dy2, shortcut_done = None, False
        d3 = conv3.desc(N, *b["hw"][-1])
        if "se" in blk:
            # gated BatchNorm + excitation backward: a reduce and an apply pass over (dout, mask bits, y3) with the [N, C]-sized
            # work between them; the SE gradients are final on the main stream when the call returns.  A projection shortcut's
            # BatchNorm takes the same dout + mask through icamd_bn_bwd (_bwd_conv1_shortcut)
            se = blk["se"]
            mean, invstd, _, _ = self._stats(bn3)
            hip.check(lib.icamd_se_bn_bwd(dout, mask, y3.data_ptr(), mean, invstd, self._pf(bn3.weight), self._pf(bn3.bias),
                                          b["se_ysum"].data_ptr(), b["se_s"].data_ptr(), b["se_h"].data_ptr(),
                                          b["se_e"].data_ptr(), self._pf(se.w1), self._pf(se.w2), self._gf(bn3.weight),
                                          self._gf(bn3.bias), self._gf(se.w1), self._gf(se.b1), self._gf(se.w2), self._gf(se.b2),
                                          dy, N, d3.OH * d3.OW, se.c, se.rd, run.acc, ws["se_ws"].data_ptr(), ws["se_ws_bytes"],
                                          run.s), se.name + " + " + bn3.name + " bwd")
            return dy, None, False
        if (self.block == "bottleneck" and fused_rows > 0 and lib.icamd_conv1x1_bn_bwd_fused_supported(ctypes.byref(d3))):
            # conv3 + bn3 backward in one pass over g and y3: BatchNorm finalize from the partial sums, dy3 only in LDS,
            # d(a2) -> DA and the filter gradient out of the same launch
            self._fused_conv_bn(run, conv3, bn3, d3, ws["bnb_part"].data_ptr(), fused_rows, dout, y3, b["a"][-2].data_ptr(), run.DA,
                                ws["bna_ws"].data_ptr(), ws["bna_ws_bytes"])
            dy = None
            if down:
                # the shortcut's BatchNorm takes the same g -- its convolution + BatchNorm fused as well where it is a 1x1 /
                # stride-1 layer of a routed shape (layer1.0), else its BatchNorm backward alone (no mask: g is masked already)
                dc = blk["down_conv"]
                ddc = dc.desc(N, *b.get("short_hw", b["in_hw"]))
                if dc.stride == 1 and lib.icamd_conv1x1_bn_bwd_fused_supported(ctypes.byref(ddc)):
                    # (run.T: on the pooled grid where the shortcut starts with the average pool)
                    self._fused_conv_bn(run, dc, blk["down_bn"], ddc, None, 0, dout, b["yd"], b.get("xp", b["in"]).data_ptr(),
                                        run.T, run.bws, run.bwb)
                    shortcut_done = True
                else:
                    dy2 = self._next_y(run)
                    self._bn_bwd(run, blk["down_bn"], dout, None, b["yd"], dy2, None, False)
        elif down and _DUAL_BNBWD:
            # the block's last BatchNorm and its shortcut's BatchNorm take the same masked gradient: one reduce and one
            # apply pass for both (dout and the mask bits are read twice instead of four times)
            dy2 = self._next_y(run)
            bnB = blk["down_bn"]
            meanA, invstdA, scaleA, _ = self._stats(bn3)
            meanB, invstdB, scaleB, _ = self._stats(bnB)
            c = bn3.c
            hip.check(lib.icamd_bn_bwd_dual(dout, mask, y3.data_ptr(), meanA, invstdA, scaleA, self._gf(bn3.weight),
                                            self._gf(bn3.bias), dy, b["yd"].data_ptr(), meanB, invstdB, scaleB,
                                            self._gf(bnB.weight), self._gf(bnB.bias), dy2, y3.numel() // c, c, run.acc, run.bws,
                                            ws["bnb_ws2"].data_ptr(), run.bwb, run.s), bn3.name + " + shortcut bwd")
        elif fused_rows:
            mean, invstd, scale, _ = self._stats(bn3)
            c = bn3.c
            hip.check(lib.icamd_bn_bwd_from_gy_partials(ws["bnb_part"].data_ptr(), fused_rows, dout, y3.data_ptr(), mean, invstd,
                                                        scale, self._gf(bn3.weight), self._gf(bn3.bias), dy, y3.numel() // c, c,
                                                        run.acc, ws["bna_ws"].data_ptr(), ws["bna_ws_bytes"], run.s),
                      bn3.name + " bwd (apply, sums from the data gradient)")
        else:
            self._bn_bwd(run, bn3, dout, None, y3, dy, None, True, mask)
        return dy, dy2, shortcut_done

    def _bwd_inner_convs(self, run, bi, dy):
        """Every convolution but the first, last to second, each followed by the backward of the BatchNorm + ReLU in front of it
        (no residual in front of that ReLU: mask recomputed from y).  dy None: the last convolution is done, run.DA holds its
        data gradient.  Returns the gradient of the first convolution's output."""
        blk, b = self.blocks[bi], run.ws["blocks"][bi]
        convs, bns = blk["convs"], blk["bns"]
        for i in range(len(convs) - 1, 0, -1):
            if dy is not None:
                # wgrad first: measured, it overlaps best with the data-gradient kernel of the same layer (issued after it,
                # i.e. beside the next BatchNorm backward whose 1024 workgroups fill every wave slot, the gain disappears)
                d = convs[i].desc(run.N, *b["hw"][i])
                self._side_wgrad(run, convs[i], d, b["a"][i - 1].data_ptr(), dy)
                self._dgrad(convs[i], d, dy, run.DA, None, None, run.s)
            dy = self._next_y(run)
            self._bn_bwd(run, bns[i - 1], run.DA, None, b["y"][i - 1], dy, None, True)
        return dy

    def _prev_takes_g(self, N, bi, h, w):
        """May the conv1 data gradient of block bi (input h x w) hand the PREVIOUS block g = its masked output gradient plus the
        (sum g, sum g*y) rows of its last BatchNorm (icamd_conv2d_dgrad_bnred)?  Identity blocks always take them; a projection
        block only through the fused conv3 + bn3 backward (its other path, icamd_bn_bwd_dual, wants the unmasked gradient and no
        sums)."""
        if bi == 0 or self.block != "bottleneck":
            return False
        pblk = self.blocks[bi - 1]
        if "se" in pblk:      # its backward reduces per sample and applies the gate: it takes the unmasked gradient
            return False
        if "down_conv" not in pblk:
            return True
        dp3 = pblk["convs"][-1].desc(N, h, w)
        return bool(self.lib.icamd_conv1x1_bn_bwd_fused_supported(ctypes.byref(dp3)))

    def _bwd_conv1_shortcut(self, run, bi, dy, dy2, shortcut_done, dout, other):
        """The block's first convolution and its shortcut: `other` = gradient of the block input.  Returns fused_rows for the
        previous block: > 0 when `other` is already its g and ws["bnb_part"] holds the sums of its last BatchNorm."""
        lib, ws, N, s = self.lib, run.ws, run.N, run.s
        blk, b = self.blocks[bi], ws["blocks"][bi]
        conv1 = blk["convs"][0]
        h, w = b["in_hw"]
        xin = b["in"].data_ptr()
        d1 = conv1.desc(N, h, w)
        self._side_wgrad(run, conv1, d1, xin, dy)
        if blk.get("pool"):
            # D variant, stride-2 block: the shortcut convolution lives on the pooled grid.  Its weight gradient reads the pooled
            # input, its data gradient is a plain pointwise one there (run.T), and the average pool's backward spreads that over the
            # 1, 2 or 4 pixels of each window ON TOP of the main branch's data gradient (run.DA is free here), which finishes the
            # block-input gradient.  No even-grid / BatchNorm-reduce fusion: their addend would have to be the spread gradient.
            dc = blk["down_conv"]
            ddc = dc.desc(N, *b["short_hw"])
            if not shortcut_done:
                if dy2 is None:
                    dy2 = self._next_y(run)
                    self._bn_bwd(run, blk["down_bn"], dout, None, b["yd"], dy2, None, True, b["mask"].data_ptr())
                self._side_wgrad(run, dc, ddc, b["xp"].data_ptr(), dy2)
                self._dgrad(dc, ddc, dy2, run.T, None, None, s)
            self._dgrad(conv1, d1, dy, run.DA, None, None, s)
            hip.check(lib.icamd_avgpool2x2_bwd(run.T, run.DA, other, N, h, w, dc.cin_p, s), blk["name"] + " shortcut pool bwd")
            return 0
        if shortcut_done:
            self._dgrad(conv1, d1, dy, other, run.T, None, s)
            return 0
        if "down_conv" not in blk:
            addend, bits, on_even_grid = dout, b["mask"].data_ptr(), 0
        else:
            dc = blk["down_conv"]
            ddc = dc.desc(N, h, w)
            if dy2 is None:
                dy2 = self._next_y(run)
                # ("relu" = the block's mask bits)
                self._bn_bwd(run, blk["down_bn"], dout, None, b["yd"], dy2, None, True, b["mask"].data_ptr())
            self._side_wgrad(run, dc, ddc, xin, dy2)
            if not (_SUB2_SHORTCUT and dc.k == 1 and dc.stride == 2 and dc.pad == 0):
                self._dgrad(dc, ddc, dy2, run.T, None, None, s)
                self._dgrad(conv1, d1, dy, other, run.T, None, s)
                return 0
            # a 1x1 stride-2 shortcut sends gradient to the even pixels only: compute it on the [OH][OW] grid (a
            # plain pointwise data gradient) and let the main branch's data gradient add it there
            # (icamd_conv2d_dgrad_sub2); the 3/4 zeros of the full-size tensor are never written or read
            key = ("sub2", N, ddc.OH, ddc.OW)
            deven = dc.descs.get(key)
            if deven is None:
                deven = dc.descs[key] = hip.conv_desc(N, ddc.OH, ddc.OW, dc.cin_p, dc.cout_p, 1, 1, 1, 0)
            self._dgrad(dc, deven, dy2, run.T, None, None, s)
            addend, bits, on_even_grid = run.T, None, 1
        if self._prev_takes_g(N, bi, h, w) and lib.icamd_conv2d_dgrad_bnred_supported(ctypes.byref(d1)):
            # `other` becomes g of the previous block (its ReLU mask applied, which every consumer of d(block output)
            # applies anyway) and the sums its last BatchNorm's backward needs come out of the same launch
            pb = ws["blocks"][bi - 1]
            hip.check(lib.icamd_conv2d_dgrad_bnred(ctypes.byref(d1), dy, self._wt(conv1), other, addend, bits, on_even_grid,
                                                   pb["y"][-1].data_ptr(), pb["mask"].data_ptr(), ws["bnb_part"].data_ptr(), s),
                      conv1.name + " dgrad + bn reduce")
            return lib.icamd_conv2d_dgrad_stats_rows(ctypes.byref(d1))
        if on_even_grid:
            hip.check(lib.icamd_conv2d_dgrad_sub2(ctypes.byref(d1), dy, self._wt(conv1), other, addend, s),
                      conv1.name + " dgrad + shortcut")
        else:
            self._dgrad(conv1, d1, dy, other, addend, bits, s)
        return 0

    def _bwd_stem(self, run, dout, dy, fused_pool):
        """maxpool -> BN+ReLU -> conv (no data gradient for the image); dy: buffer for the stem convolution's output gradient."""
        lib, ws, N, s = self.lib, run.ws, run.N, run.s
        last = self.stem_pairs[-1][0]
        d0 = last.desc(N, *ws["stem_hw"][-1])
        bn0 = self.stem_bn
        if fused_pool:
            # max-pool backward folded into both BatchNorm-backward passes: the 112x112 gradient is never materialised
            mean, invstd, scale, shift = self._stats(bn0)
            hip.check(lib.icamd_bn_bwd_maxpool3x3s2(dout, ws["p0_idx"].data_ptr(), ws["y0"].data_ptr(), mean, invstd, scale, shift,
                                                    self._gf(bn0.weight), self._gf(bn0.bias), dy, N, d0.OH, d0.OW, bn0.c, run.acc,
                                                    run.bws, run.bwb, s), "stem maxpool + bn bwd")
        else:
            hip.check(lib.icamd_maxpool3x3s2_bwd(dout, ws["p0_idx"].data_ptr(), run.DA, N, d0.OH, d0.OW, 64, s), "maxpool bwd")
            self._bn_bwd(run, bn0, run.DA, None, ws["y0"], dy, None, True)
        # The stem's convolutions, last to first: weight gradient (side lane) + data gradient, then the BatchNorm + ReLU in front
        # (mask recomputed from y); the first convolution reads the image: weight gradient only.  The two data gradients go to
        # different scratch buffers (run.DA, run.T) and ws["stem_dy"][i] / ws["stem_dx"][i] name the gradient of the i-th
        # convolution's output / input, so that all of them can be read back after the pass (tests/test_resnet_d_gpu.py)
        name_views = "stem_dy" not in ws      # once per workspace: the scratch buffers rotate the same way in every pass
        if name_views:
            ws["stem_dy"], ws["stem_dx"] = [None] * len(self.stem_pairs), [None] * len(self.stem_pairs)
        for i in range(len(self.stem_pairs) - 1, -1, -1):
            conv = self.stem_pairs[i][0]
            d = conv.desc(N, *ws["stem_hw"][i])
            if name_views:
                ws["stem_dy"][i] = self._grad_view(ws, dy, ws["stem_y"][i])
            self._side_wgrad(run, conv, d, ws["stem_in"][i].data_ptr(), dy)
            if i == 0:
                break
            dx = run.DA if i == len(self.stem_pairs) - 1 else run.T
            if name_views:
                ws["stem_dx"][i] = self._grad_view(ws, dx, ws["stem_in"][i])
            self._dgrad(conv, d, dy, dx, None, None, s)
            dy = self._next_y(run)
            self._bn_bwd(run, self.stem_pairs[i - 1][1], dx, None, ws["stem_y"][i - 1], dy, None, True)

    def _backward_packed_fused(self, ws, accumulate=False):
        """Variant that fuses each BatchNorm backward's mask + reduction pass into the epilogue of the data-gradient
        kernel that produces its output gradient (icamd_conv2d_dgrad_bnbwd + icamd_bn_bwd_from_partials).  Fewer HBM
        bytes, but the un-pipelined epilogue makes it latency-bound on MI355X today (profiles/ r01 notes): opt-in with
        ICAMD_FUSED_BNBWD=1.  One stream: the side lane stays off."""
        lib = self.lib
        run = self._backward_begin(ws, accumulate, False)
        N, s, acc = run.N, run.s, run.acc
        dout, other, G, T, Y, Y2, run.DA = (b.data_ptr() for b in self._grad_buffers(ws)[:7])
        DA = run.DA
        P, aws, pw_bytes = ws["bnb_part"].data_ptr(), ws["bna_ws"].data_ptr(), ws["bna_ws_bytes"]

        def dgrad_bnbwd(conv, d, dy_ptr, g_ptr, addend, bn, y, mask_src):
            """data gradient whose output is the output-gradient of `bn` + ReLU: fused mask + pass-1 reductions."""
            f = hip.BnBwdFuse(y.data_ptr(), mask_src, *self._stats(bn), P, 1)
            hip.check(lib.icamd_conv2d_dgrad_bnbwd(ctypes.byref(d), dy_ptr, self._wt(conv), g_ptr, addend, ctypes.byref(f), s),
                      conv.name + " dgrad+bnbwd")
            return lib.icamd_conv2d_dgrad_stats_rows(ctypes.byref(d))

        def bn_bwd_from_partials(bn, nrows, g_ptr, y, dy_ptr):
            mean, invstd, scale, _ = self._stats(bn)
            hip.check(lib.icamd_bn_bwd_from_partials(P, nrows, g_ptr, y.data_ptr(), mean, invstd, scale,
                                                     self._gf(bn.weight), self._gf(bn.bias), dy_ptr, y.numel() // bn.c, bn.c, acc,
                                                     aws, pw_bytes, s), bn.name + " bwd(apply)")

        self._bwd_classifier(run, dout)
        nblk = len(self.blocks)
        pending_rows = 0   # partial rows left in P by the previous block's fused data gradient (for this block's last BN)
        for bi in range(nblk - 1, -1, -1):
            blk, b = self.blocks[bi], ws["blocks"][bi]
            convs, bns = blk["convs"], blk["bns"]
            h, w = b["in_hw"]
            xin = b["in"].data_ptr()
            if bi == nblk - 1:
                # last block: its output gradient comes from the average pool: two-pass BN backward with the mask
                self._bn_bwd(run, bns[-1], dout, b["a"][-1].data_ptr(), b["y"][-1], Y, G, True)
                g_ptr = G
            else:
                # `dout` already holds g = masked output gradient and P its pass-1 sums (fused in the producer)
                bn_bwd_from_partials(bns[-1], pending_rows, dout, b["y"][-1], Y)
                g_ptr = dout
            for i in range(len(convs) - 1, 0, -1):
                d = convs[i].desc(N, *b["hw"][i])
                self._side_wgrad(run, convs[i], d, b["a"][i - 1].data_ptr(), Y)
                if convs[i].groups > 1:
                    # the grouped data gradient has no fused BatchNorm reduction: plain data gradient, two-pass BatchNorm backward
                    self._dgrad(convs[i], d, Y, DA, None, None, s)
                    self._bn_bwd(run, bns[i - 1], DA, None, b["y"][i - 1], Y, None, True)
                    continue
                nrows = dgrad_bnbwd(convs[i], d, Y, DA, None, bns[i - 1], b["y"][i - 1], None)
                bn_bwd_from_partials(bns[i - 1], nrows, DA, b["y"][i - 1], Y)
            d1 = convs[0].desc(N, h, w)
            self._side_wgrad(run, convs[0], d1, xin, Y)
            if "down_conv" in blk:
                dc = blk["down_conv"]
                ddc = dc.desc(N, h, w)
                self._bn_bwd(run, blk["down_bn"], g_ptr, None, b["yd"], Y2, None, False)
                self._side_wgrad(run, dc, ddc, xin, Y2)
                self._dgrad(dc, ddc, Y2, T, None, None, s)
                addend = T
            else:
                addend = g_ptr
            if bi > 0:
                pb, pblk = ws["blocks"][bi - 1], self.blocks[bi - 1]
                pending_rows = dgrad_bnbwd(convs[0], d1, Y, other, addend, pblk["bns"][-1], pb["y"][-1], xin)
            else:
                self._dgrad(convs[0], d1, Y, other, addend, None, s)
            if run.hook:
                run.hook(convs[0].w.offset, None, ())
            dout, other = other, dout
        self._bwd_stem(run, dout, Y, False)
        if run.hook:
            run.hook(0, None, ())
