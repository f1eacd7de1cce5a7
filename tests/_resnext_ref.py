"""Tests-side reference of the whole ResNet family (deeper / wider ResNets, ResNeXt) in plain torch, built on oracle.resnet_ref:
the same stem, head, rounding points and block forward; a bottleneck's convolutions are rebuilt with the inner width
floor(planes * base_width / 64) * cardinality and conv2 gets `cardinality` groups (timm / torchvision Bottleneck).  Grouped
convolutions are torch.nn.functional.conv2d(groups=...) and nothing else.  ResNetRef itself stays group-free."""
import math

import torch.nn as nn
import torch.nn.functional as F

from oracle.resnet_ref import ResNetRef, _Block, _r, _w

# name -> (block, blocks per stage, cardinality, base width): the published definitions, restated here independently of the product
FAMILY = {
    "resnet18": ("basic", [2, 2, 2, 2], 1, 64),
    "resnet34": ("basic", [3, 4, 6, 3], 1, 64),
    "resnet50": ("bottleneck", [3, 4, 6, 3], 1, 64),
    "resnet101": ("bottleneck", [3, 4, 23, 3], 1, 64),
    "resnet152": ("bottleneck", [3, 8, 36, 3], 1, 64),
    "wide_resnet50_2": ("bottleneck", [3, 4, 6, 3], 1, 128),
    "wide_resnet101_2": ("bottleneck", [3, 4, 23, 3], 1, 128),
    "resnext50_32x4d": ("bottleneck", [3, 4, 6, 3], 32, 4),
    "resnext101_32x4d": ("bottleneck", [3, 4, 23, 3], 32, 4),
}


class _GroupedBlock(_Block):
    def __init__(self, kind, inplanes, planes, stride, bf16_points, cardinality=1, base_width=64):
        super().__init__(kind, inplanes, planes, stride, bf16_points)
        if kind == "bottleneck":
            width = int(math.floor(planes * base_width / 64)) * cardinality
            self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(width)
            self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=cardinality, bias=False)
            self.bn2 = nn.BatchNorm2d(width)
            self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)

    def _cb(self, conv, bn, x, tag=None):
        y = _r(F.conv2d(x, _w(conv.weight, self.q), None, conv.stride, conv.padding, 1, conv.groups), self.q)
        if self.trace is not None and tag is not None:
            self.trace[f"{self.trace_name}.{tag}.y"] = y.detach()
        return bn(y)


class ResNetFamilyRef(ResNetRef):
    def __init__(self, arch="resnext50_32x4d", num_classes=1000, bf16_points=False, zero_init_last=True):
        nn.Module.__init__(self)
        kind, layers, cardinality, base_width = FAMILY[arch]
        self.q = bf16_points
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        exp = 4 if kind == "bottleneck" else 1
        for li, (planes, n) in enumerate(zip([64, 128, 256, 512], layers)):
            blocks = []
            for bi in range(n):
                blocks.append(_GroupedBlock(kind, inplanes, planes, 2 if (bi == 0 and li > 0) else 1, bf16_points, cardinality,
                                            base_width))
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
