"""CPU oracle: the whole ResNet family in plain torch (TEST INFRASTRUCTURE ONLY -- never imported by the product).

The reference has no model code: it calls timm.create_model(args.model) and timm is neither in the reference tree nor
installed, so this file restates the architectures timm implements under the names of ARCHS, with timm's parameter names:

  * resnet18/34/50/101/152: ResNet v1.5: 7x7/2 stem, 3x3/2 max-pool, [Basic|Bottleneck] blocks with the stride on the 3x3,
    1x1/stride projection shortcut + BN, global average pool, linear head; BatchNorm eps 1e-5 momentum 0.1; Kaiming-normal
    fan_out conv init, zero-init of each block's last BN weight.
  * wide_resnet*_2, resnext*_32x4d: a bottleneck's inner width is floor(planes * base_width / 64) * cardinality and conv2 gets
    `cardinality` groups (timm / torchvision Bottleneck).  Grouped convolutions are torch.nn.functional.conv2d(groups=...) and
    nothing else.
  * seresnet*, seresnext*: timm's Bottleneck with attn_layer='se'.  The SE module is two 1x1 nn.Conv2d with bias around a ReLU
    and a sigmoid, reduction C / 16, applied to bn3's output before the shortcut add; module order ... bn3, se, downsample.
  * the "D" members (timm stem_width=32, stem_type='deep', avg_down=True, "Bag of Tricks"): deep stem conv1 =
    nn.Sequential(conv 3->32 /2, bn, relu, conv 32->32, bn, relu, conv 32->64), then bn1, relu, max-pool; projection shortcut
    nn.Sequential(pool, conv 1x1 stride 1, bn) with pool = AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) in the
    stride-2 blocks and nn.Identity() in layer1.0.

Pinned against torch itself only (the published parameter counts are checked in tests/test_oracle_cpu.py and the family's
CPU tests): "parity unpinned" with respect to timm, which cannot be imported.  ARCHS is written out here independently of the
product's table; the CPU tests compare the two.

`bf16_points=True` inserts the rounding points of the HIP path (inputs, filters, every stored activation, every convolution
output and every stored activation-gradient rounded to bf16; accumulation, BatchNorm statistics and weight gradients in
fp32), so that logits/gradients can be compared at the 1e-3 level instead of bf16's 4e-3 per-op noise.  The pooled shortcut
input of a D block is stored, so it is rounded once.  In an SE block conv3's output is bf16 as everywhere; the BatchNorm
output z, the pooled s, h and e are fp32 and never rounded; the block output is rounded to bf16 once; the SE weights are fp32
masters used as they are (no bf16 copy).  A .double() copy (copy.deepcopy(ref).double()) runs the same forward.
"""

import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class _RoundBF16(torch.autograd.Function):
    """Round to the bf16 grid, keeping the working dtype (fp32, or fp64 for the re-association calibration run)."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _RoundWeight(torch.autograd.Function):
    """bf16 filter copy of an fp32 master weight; the gradient stays fp32 (straight through)."""

    @staticmethod
    def forward(ctx, w):
        return w.to(torch.bfloat16).to(w.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _r(x, on):
    return _RoundBF16.apply(x) if on else x


def _w(w, on):
    return _RoundWeight.apply(w) if on else w


# name -> (block, blocks per stage, cardinality, base width, se, deep): the published definitions
ARCHS = {
    "resnet18": ("basic", [2, 2, 2, 2], 1, 64, False, False),
    "resnet34": ("basic", [3, 4, 6, 3], 1, 64, False, False),
    "resnet50": ("bottleneck", [3, 4, 6, 3], 1, 64, False, False),
    "resnet101": ("bottleneck", [3, 4, 23, 3], 1, 64, False, False),
    "resnet152": ("bottleneck", [3, 8, 36, 3], 1, 64, False, False),
    "wide_resnet50_2": ("bottleneck", [3, 4, 6, 3], 1, 128, False, False),
    "wide_resnet101_2": ("bottleneck", [3, 4, 23, 3], 1, 128, False, False),
    "resnext50_32x4d": ("bottleneck", [3, 4, 6, 3], 32, 4, False, False),
    "resnext101_32x4d": ("bottleneck", [3, 4, 23, 3], 32, 4, False, False),
    "seresnet50": ("bottleneck", [3, 4, 6, 3], 1, 64, True, False),
    "seresnet101": ("bottleneck", [3, 4, 23, 3], 1, 64, True, False),
    "seresnet152": ("bottleneck", [3, 8, 36, 3], 1, 64, True, False),
    "seresnext50_32x4d": ("bottleneck", [3, 4, 6, 3], 32, 4, True, False),
    "seresnext101_32x4d": ("bottleneck", [3, 4, 23, 3], 32, 4, True, False),
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


class SEModule(nn.Module):
    def __init__(self, channels, rd_channels):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, rd_channels, 1, bias=True)
        self.fc2 = nn.Conv2d(rd_channels, channels, 1, bias=True)

    def gate(self, z):
        s = z.mean((2, 3), keepdim=True)
        return torch.sigmoid(self.fc2(F.relu(self.fc1(s))))

    def forward(self, z):
        return z * self.gate(z)


class _Block(nn.Module):
    def __init__(self, kind, inplanes, planes, stride, bf16_points, cardinality=1, base_width=64, se=False, deep=False):
        super().__init__()
        self.kind, self.q = kind, bf16_points
        self.trace, self.trace_name = None, ""
        out = planes * (4 if kind == "bottleneck" else 1)
        if kind == "bottleneck":
            width = int(math.floor(planes * base_width / 64)) * cardinality
            self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(width)
            self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=cardinality, bias=False)
            self.bn2 = nn.BatchNorm2d(width)
            self.conv3 = nn.Conv2d(width, out, 1, bias=False)
            self.bn3 = nn.BatchNorm2d(out)
        else:
            assert cardinality == 1 and base_width == 64 and not se
            self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(planes)
            self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes)
        self.se = SEModule(out, out // 16) if se else None          # module order: ... bn3, se, downsample
        self.downsample = None
        if stride != 1 or inplanes != out:
            if deep:
                pool = nn.AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False) if stride != 1 else nn.Identity()
                self.downsample = nn.Sequential(pool, nn.Conv2d(inplanes, out, 1, 1, bias=False), nn.BatchNorm2d(out))
            else:
                self.downsample = nn.Sequential(nn.Conv2d(inplanes, out, 1, stride, bias=False), nn.BatchNorm2d(out))

    def _cb(self, conv, bn, x, tag):
        y = _r(F.conv2d(x, _w(conv.weight, self.q), None, conv.stride, conv.padding, 1, conv.groups), self.q)
        if self.trace is not None:
            self.trace[f"{self.trace_name}.{tag}.y"] = y.detach()
        return bn(y)

    def _keep(self, tag, t):
        if self.trace is not None:
            self.trace[f"{self.trace_name}.{tag}"] = t.detach()
        return t

    def forward(self, x):
        q = self.q
        idn = x
        if self.downsample is not None:
            *pool, conv, bn = self.downsample
            s = x
            if pool and isinstance(pool[0], nn.AvgPool2d):
                s = self._keep("down.x", _r(pool[0](x), q))         # the pooled input is stored: rounded once
            idn = self._keep("down.a", _r(self._cb(conv, bn, s, "down"), q))
        o = self._keep("0.a", _r(F.relu(self._cb(self.conv1, self.bn1, x, "0")), q))
        if self.kind == "bottleneck":
            o = self._keep("1.a", _r(F.relu(self._cb(self.conv2, self.bn2, o, "1")), q))
            o = self._cb(self.conv3, self.bn3, o, "2")
            last = "2.a"
        else:
            o = self._cb(self.conv2, self.bn2, o, "1")
            last = "1.a"
        if self.se is not None:
            o = self.se(o)
        return self._keep(last, _r(F.relu(o + idn), q))

    @property
    def last_bn(self):
        return self.bn3 if self.kind == "bottleneck" else self.bn2


class ResNetRef(nn.Module):
    def __init__(self, arch="resnet50", num_classes=1000, bf16_points=False, zero_init_last=True):
        super().__init__()
        kind, layers, cardinality, base_width, se, deep = ARCHS[arch]
        self.q = bf16_points
        if deep:
            self.conv1 = nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                       nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                       nn.Conv2d(32, 64, 3, 1, 1, bias=False))
        else:
            self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        exp = 4 if kind == "bottleneck" else 1
        for li, (planes, n) in enumerate(zip([64, 128, 256, 512], layers)):
            blocks = []
            for bi in range(n):
                blocks.append(_Block(kind, inplanes, planes, 2 if (bi == 0 and li > 0) else 1, bf16_points, cardinality,
                                     base_width, se, deep))
                inplanes = planes * exp
            setattr(self, f"layer{li + 1}", nn.Sequential(*blocks))
        self.fc = nn.Linear(inplanes, num_classes)
        # timm ResNet.init_weights: every nn.Conv2d weight, the SE ones included; their biases keep nn.Conv2d's default
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if zero_init_last:
            for m in self.modules():
                if isinstance(m, _Block):
                    nn.init.zeros_(m.last_bn.weight)

    def set_trace(self, trace):
        """trace: dict that receives every stored intermediate (NCHW), keyed like the HIP workspace."""
        self.trace = trace
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self, f"layer{li}")):
                blk.trace, blk.trace_name = trace, f"layer{li}.{bi}"

    def forward(self, x):
        q = self.q
        tr = getattr(self, "trace", None)
        x = _r(x, q)
        stem = {}
        last = self.conv1
        if isinstance(last, nn.Sequential):      # deep stem: two conv + bn + relu, each stored, in front of the last convolution
            for i, (conv, bn) in enumerate(((last[0], last[1]), (last[3], last[4]))):
                y = _r(F.conv2d(x, _w(conv.weight, q), None, conv.stride, conv.padding), q)
                x = _r(F.relu(bn(y)), q)
                stem[f"stem_y{i}"], stem[f"stem_a{i}"] = y.detach(), x.detach()
            last = last[6]
        y = _r(F.conv2d(x, _w(last.weight, q), None, last.stride, last.padding), q)
        a0 = _r(F.relu(self.bn1(y)), q)
        p0 = F.max_pool2d(a0, 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(p0))))
        pooled = _r(x.mean(dim=(2, 3)), q)
        logits = _r(F.linear(pooled, _w(self.fc.weight, q), self.fc.bias), q)
        if tr is not None:
            tr.update(stem)
            tr.update({"y0": y.detach(), "a0": a0.detach(), "p0": p0.detach(), "pooled": pooled.detach(),
                       "logits": logits.detach()})
        return logits
