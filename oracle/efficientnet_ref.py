"""CPU oracle: EfficientNet-B0 / B1 in plain torch (TEST INFRASTRUCTURE ONLY -- never imported by the product).

timm's efficientnet_b0 / b1 restated from the layer list (timm is not importable here: parity with it is unpinned; the parameter
counts are checked against what torchvision publishes for the same architectures in tests/test_efficientnet_cpu.py).  The layer list
is written out here independently of the product's table, and this file imports nothing of the product: the CPU tests compare the two.

`bf16_points=True` inserts the rounding points of the HIP path (oracle/resnet_ref.py's `_r` / `_w`); the Tape, the stored-tensor
pass-through and the rounded convolution are oracle/mobilenet_ref.py's."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.mobilenet_ref import Tape, _conv, _pt  # noqa: F401  (Tape: the tests take it with the model)
from oracle.resnet_ref import _r, _w

# (kernel, first stride, out channels, repeats) of stages 1..6 of efficientnet_b0; b1: repeats ceil(1.1 r), blocks.0 twice
B0_STAGES = ((3, 2, 24, 2), (5, 2, 40, 2), (3, 2, 80, 3), (5, 1, 112, 3), (5, 2, 192, 4), (3, 1, 320, 1))
TEST_ARCH = {"stem": 16, "first": (8, 1), "stages": ((3, 2, 16, 2), (5, 2, 24, 1), (5, 1, 32, 2)), "head": 64}
PUBLISHED = {"efficientnet_b0": 5288548, "efficientnet_b1": 7794184}


def layer_list(arch):
    """stem width, [[(kind, kernel, in, mid, out, stride, rd)] per stage], head width; rd = a quarter of the block INPUT width"""
    if arch == "efficientnet_test":
        t = TEST_ARCH
        stem, (first, first_n), stages, head = t["stem"], t["first"], t["stages"], t["head"]
    else:
        depth = {"efficientnet_b0": 1.0, "efficientnet_b1": 1.1}[arch]
        stem, first, first_n, head = 32, 16, int(math.ceil(depth)), 1280
        stages = tuple((k, s, c, int(math.ceil(depth * n))) for k, s, c, n in B0_STAGES)
    out, cin = [], stem
    stage = []
    for i in range(first_n):
        stage.append(("ds", 3, cin, cin, first, 1, max(1, cin // 4)))
        cin = first
    out.append(stage)
    for k, s, c, n in stages:
        stage = []
        for i in range(n):
            stage.append(("ir", k, cin, cin * 6, c, s if i == 0 else 1, max(1, cin // 4)))
            cin = c
        out.append(stage)
    return stem, out, head


def param_count(arch, num_classes=1000):
    stem, stages, head = layer_list(arch)
    n = 27 * stem + 2 * stem
    for stage in stages:
        for kind, k, cin, mid, cout, _, rd in stage:
            se = mid * rd + rd + rd * mid + mid
            if kind == "ds":
                n += k * k * cin + 2 * cin + se + cin * cout + 2 * cout
            else:
                n += cin * mid + 2 * mid + k * k * mid + 2 * mid + se + mid * cout + 2 * cout
            last = cout
    return n + last * head + 2 * head + head * num_classes + num_classes


def _act(bn, y, q):
    """the activation silu(bn(y)) rounded once"""
    return _r(F.silu(bn(y)), q)


def _act_fused(bn, y, q):
    """the activation in front of a gate: its VALUE is rounded once (the squeeze sums and the gated apply multiplies bf16(a)), its
    GRADIENT is not -- the HIP path never materialises it: icamd_bn_bwd_silu forms dout * gate + dsn in registers"""
    return _w(F.silu(bn(y)), q)


class _SE(nn.Module):
    """fp32 throughout on the HIP path (the [N, C]-sized arrays are never rounded): mean of the rounded activation, 1x1 reduce + SiLU,
    1x1 expand + sigmoid"""

    def __init__(self, c, rd):
        super().__init__()
        self.conv_reduce = nn.Conv2d(c, rd, 1)
        self.conv_expand = nn.Conv2d(rd, c, 1)

    def forward(self, a):
        return torch.sigmoid(self.conv_expand(F.silu(self.conv_reduce(a.mean((2, 3), keepdim=True)))))


class _DS(nn.Module):
    def __init__(self, k, cin, cout, rd, q):
        super().__init__()
        self.q, self.tape, self.residual = q, None, cin == cout
        self.conv_dw = nn.Conv2d(cin, cin, k, 1, k // 2, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.se = _SE(cin, rd)
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)

    def forward(self, x):
        q = self.q
        a = _act_fused(self.bn1, _pt(self, _conv(x, self.conv_dw, q)), q)    # never stored: the gated tensor is
        gated = _pt(self, _r(a * self.se(a), q))
        o = self.bn2(_pt(self, _conv(gated, self.conv_pw, q)))
        return _pt(self, _r(o + x if self.residual else o, q))


class _IR(nn.Module):
    def __init__(self, k, cin, mid, cout, stride, rd, q):
        super().__init__()
        self.q, self.residual, self.tape = q, stride == 1 and cin == cout, None
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, k, stride, k // 2, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.se = _SE(mid, rd)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)

    def forward(self, x):
        q = self.q
        a1 = _act(self.bn1, _pt(self, _conv(x, self.conv_pw, q)), q)         # never stored, rounded once all the same
        a2 = _act_fused(self.bn2, _pt(self, _conv(a1, self.conv_dw, q)), q)  # never stored either
        gated = _pt(self, _r(a2 * self.se(a2), q))
        o = self.bn3(_pt(self, _conv(gated, self.conv_pwl, q)))
        return _pt(self, _r(o + x if self.residual else o, q))


class EfficientNetRef(nn.Module):
    """bf16_points: the rounding points of the HIP path (input, filters, every convolution output, every activation, the gated
    projection input, every block output, the pooled vector, the logits; their gradients likewise, but for the gradient of the
    activation in front of a gate: _act_fused).  The Tape sees the tensors the
    HIP path stores: packed input, y0, per block (y1,) y2, gated, y3, out, then yh, ah, pooled, logits."""

    def __init__(self, arch="efficientnet_b0", num_classes=1000, bf16_points=False):
        super().__init__()
        self.q, self.tape = bf16_points, None
        stem, stages, head = layer_list(arch)
        q = bf16_points
        self.conv_stem = nn.Conv2d(3, stem, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem)
        self.blocks = nn.Sequential(*[nn.Sequential(*[_DS(k, cin, cout, rd, q) if kind == "ds" else _IR(k, cin, mid, cout, s, rd, q)
                                                      for kind, k, cin, mid, cout, s, rd in stage]) for stage in stages])
        self.conv_head = nn.Conv2d(stages[-1][-1][4], head, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(head)
        self.classifier = nn.Linear(head, num_classes)
        for m in self.modules():                                  # timm's _init_weight_goog
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0.0, (2.0 / fan_out) ** 0.5)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        rng = 1.0 / num_classes ** 0.5
        nn.init.uniform_(self.classifier.weight, -rng, rng)
        nn.init.zeros_(self.classifier.bias)

    def set_tape(self, tape):
        for m in self.modules():
            if isinstance(m, (_IR, _DS, EfficientNetRef)):
                m.tape = tape

    def forward(self, x):
        q = self.q
        x = _act(self.bn1, _pt(self, _conv(_pt(self, _r(x, q)), self.conv_stem, q)), q)
        x = self.blocks(x)
        x = _pt(self, _act(self.bn2, _pt(self, _conv(x, self.conv_head, q)), q))
        pooled = _pt(self, _r(x.mean(dim=(2, 3)), q))
        return _pt(self, _r(F.linear(pooled, _w(self.classifier.weight, q), self.classifier.bias), q))


def perturb(ref, seed):
    """BatchNorm weights U(0.5, 1.5), biases N(0, 0.3), random running statistics; SE biases N(0, 1), so that the gates spread away
    from 0.5 without saturating"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            elif isinstance(m, _SE):
                for conv in (m.conv_reduce, m.conv_expand):
                    conv.bias.copy_(torch.randn(conv.bias.shape, generator=g))
    return ref
