"""Tests-side reference of the "D" members of the ResNet family (resnet18d/34d/26d/50d/101d/152d/200d, seresnet152d,
seresnext26d_32x4d) in plain torch, on tests/_resnext_ref.py and tests/_seresnet_ref.py: timm's ResNet with stem_width=32,
stem_type='deep', avg_down=True ("Bag of Tricks").

  * deep stem: conv1 = nn.Sequential(conv 3->32 /2, bn, relu, conv 32->32, bn, relu, conv 32->64), then bn1, relu, max-pool;
  * projection shortcut: nn.Sequential(pool, conv 1x1 stride 1, bn) with pool = AvgPool2d(2, 2, ceil_mode=True,
    count_include_pad=False) in the stride-2 blocks and nn.Identity() in layer1.0.

Rounding points are those of oracle/resnet_ref.py: every stored activation and convolution output rounded to bf16; the pooled
shortcut input is stored, so it is rounded once.  A .double() copy (copy.deepcopy(ref).double()) runs the same forward."""
import torch.nn as nn
import torch.nn.functional as F

from _resnext_ref import ResNetFamilyRef, _GroupedBlock
from _seresnet_ref import _SEBlock
from oracle.resnet_ref import _Block, _r, _w

# name -> (block, blocks per stage, cardinality, base width, SE): the published definitions, restated independently of the product
D_FAMILY = {
    "resnet18d": ("basic", [2, 2, 2, 2], 1, 64, False),
    "resnet34d": ("basic", [3, 4, 6, 3], 1, 64, False),
    "resnet26d": ("bottleneck", [2, 2, 2, 2], 1, 64, False),
    "resnet50d": ("bottleneck", [3, 4, 6, 3], 1, 64, False),
    "resnet101d": ("bottleneck", [3, 4, 23, 3], 1, 64, False),
    "resnet152d": ("bottleneck", [3, 8, 36, 3], 1, 64, False),
    "resnet200d": ("bottleneck", [3, 24, 36, 3], 1, 64, False),
    "seresnet152d": ("bottleneck", [3, 8, 36, 3], 1, 64, True),
    "seresnext26d_32x4d": ("bottleneck", [2, 2, 2, 2], 32, 4, True),
}


class _DShortcut:
    """Mixin: replaces the block's shortcut by Sequential(pool | Identity, conv 1x1 stride 1, bn).  The block forwards of the base
    classes call self._cb(downsample[0], downsample[1], x, "down"); that call is re-routed here."""

    def _make_d_shortcut(self, inplanes, out, stride):
        if self.downsample is None:
            return
        pool = nn.AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False) if stride != 1 else nn.Identity()
        # (assigning to the existing key keeps the module order: ... bn3, [se,] downsample)
        self.downsample = nn.Sequential(pool, nn.Conv2d(inplanes, out, 1, 1, bias=False), nn.BatchNorm2d(out))

    def _cb(self, conv, bn, x, tag=None):
        if tag == "down":
            pool, conv, bn = self.downsample
            if isinstance(pool, nn.AvgPool2d):
                x = self._keep("down.x", _r(pool(x), self.q))
        return super()._cb(conv, bn, x, tag)


class _DBlock(_DShortcut, _GroupedBlock):
    def __init__(self, kind, inplanes, planes, stride, bf16_points, cardinality=1, base_width=64):
        super().__init__(kind, inplanes, planes, stride, bf16_points, cardinality, base_width)
        self._make_d_shortcut(inplanes, planes * (4 if kind == "bottleneck" else 1), stride)


class _SEDBlock(_DShortcut, _SEBlock):
    def __init__(self, kind, inplanes, planes, stride, bf16_points, cardinality=1, base_width=64):
        super().__init__(kind, inplanes, planes, stride, bf16_points, cardinality, base_width)
        self._make_d_shortcut(inplanes, planes * 4, stride)


class ResNetDRef(ResNetFamilyRef):
    def __init__(self, arch="resnet50d", num_classes=1000, bf16_points=False, zero_init_last=True):
        nn.Module.__init__(self)
        kind, layers, cardinality, base_width, se = D_FAMILY[arch]
        self.q = bf16_points
        self.conv1 = nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                   nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                   nn.Conv2d(32, 64, 3, 1, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        exp = 4 if kind == "bottleneck" else 1
        block = _SEDBlock if se else _DBlock
        for li, (planes, n) in enumerate(zip([64, 128, 256, 512], layers)):
            blocks = []
            for bi in range(n):
                blocks.append(block(kind, inplanes, planes, 2 if (bi == 0 and li > 0) else 1, bf16_points, cardinality, base_width))
                inplanes = planes * exp
            setattr(self, f"layer{li + 1}", nn.Sequential(*blocks))
        self.fc = nn.Linear(inplanes, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if zero_init_last:
            for m in self.modules():
                if isinstance(m, _Block):
                    nn.init.zeros_(m.last_bn.weight)

    def forward(self, x):
        q = self.q
        tr = getattr(self, "trace", None)
        x = _r(x, q)
        c = self.conv1
        stem = {}
        for i, (ci, bi) in enumerate(((0, 1), (3, 4))):
            y = _r(F.conv2d(x, _w(c[ci].weight, q), None, c[ci].stride, 1), q)
            x = _r(F.relu(c[bi](y)), q)
            stem[f"stem_y{i}"], stem[f"stem_a{i}"] = y.detach(), x.detach()
        y = _r(F.conv2d(x, _w(c[6].weight, q), None, 1, 1), q)
        a0 = _r(F.relu(self.bn1(y)), q)
        p0 = F.max_pool2d(a0, 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(p0))))
        pooled = _r(x.mean(dim=(2, 3)), q)
        logits = _r(F.linear(pooled, _w(self.fc.weight, q), self.fc.bias), q)
        if tr is not None:
            tr.update(stem)
            tr.update({"y0": y.detach(), "a0": a0.detach(), "p0": p0.detach(), "pooled": pooled.detach(), "logits": logits.detach()})
        return logits
