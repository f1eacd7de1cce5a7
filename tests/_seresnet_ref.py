"""Tests-side reference of the SE members of the ResNet family (seresnet50/101/152, seresnext50/101_32x4d) in plain torch, on
tests/_resnext_ref.ResNetFamilyRef: timm's Bottleneck with attn_layer='se'.  The SE module is two 1x1 nn.Conv2d with bias around a
ReLU and a sigmoid, reduction C / 16, applied to bn3's output before the shortcut add; module order ... bn3, se, downsample.

Rounding points (shared with the HIP path): conv3's output is bf16 as everywhere; the BatchNorm output z, the pooled s, h and e are
fp32 and never rounded; the block output is rounded to bf16 once.  The SE weights are fp32 masters used as they are (no bf16 copy).
A .double() copy runs the same forward."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _resnext_ref import ResNetFamilyRef, _GroupedBlock
from oracle.resnet_ref import _Block, _r

# name -> (block, blocks per stage, cardinality, base width): the published definitions, restated independently of the product
SE_FAMILY = {
    "seresnet50": ("bottleneck", [3, 4, 6, 3], 1, 64),
    "seresnet101": ("bottleneck", [3, 4, 23, 3], 1, 64),
    "seresnet152": ("bottleneck", [3, 8, 36, 3], 1, 64),
    "seresnext50_32x4d": ("bottleneck", [3, 4, 6, 3], 32, 4),
    "seresnext101_32x4d": ("bottleneck", [3, 4, 23, 3], 32, 4),
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


class _SEBlock(_GroupedBlock):
    def __init__(self, kind, inplanes, planes, stride, bf16_points, cardinality=1, base_width=64):
        assert kind == "bottleneck"
        super().__init__(kind, inplanes, planes, stride, bf16_points, cardinality, base_width)
        down = self._modules.pop("downsample", None)        # module order: ... bn3, se, downsample
        self.se = SEModule(planes * 4, planes * 4 // 16)
        if down is not None:
            self.downsample = down

    def forward(self, x):
        q = self.q
        idn = x
        if self.downsample is not None:
            idn = self._keep("down.a", _r(self._cb(self.downsample[0], self.downsample[1], x, "down"), q))
        o = self._keep("0.a", _r(F.relu(self._cb(self.conv1, self.bn1, x, "0")), q))
        o = self._keep("1.a", _r(F.relu(self._cb(self.conv2, self.bn2, o, "1")), q))
        z = self._cb(self.conv3, self.bn3, o, "2")
        return self._keep("2.a", _r(F.relu(self.se(z) + idn), q))


class SEResNetRef(ResNetFamilyRef):
    def __init__(self, arch="seresnet50", num_classes=1000, bf16_points=False, zero_init_last=True):
        nn.Module.__init__(self)
        kind, layers, cardinality, base_width = SE_FAMILY[arch]
        self.q = bf16_points
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for li, (planes, n) in enumerate(zip([64, 128, 256, 512], layers)):
            blocks = []
            for bi in range(n):
                blocks.append(_SEBlock(kind, inplanes, planes, 2 if (bi == 0 and li > 0) else 1, bf16_points, cardinality,
                                       base_width))
                inplanes = planes * 4
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
