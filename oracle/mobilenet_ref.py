"""CPU oracle: MobileNetV2 in plain torch (TEST INFRASTRUCTURE ONLY -- never imported by the product).

timm's mobilenetv2_* restated from its layer list (timm is not importable here: parity with it is unpinned; the published parameter
counts are checked in tests/test_mobilenetv2_cpu.py).  The layer list and make_divisible are written out here independently of the
product's table, and this file imports nothing of the product: the CPU tests compare the two.

`bf16_points=True` inserts the rounding points of the HIP path (oracle/resnet_ref.py's `_r` / `_w`: activations and their gradients
to bf16, filters straight through).  A Tape records the tensors a run stores, or puts those of another run in their place
(teacher forcing; the protocol built on it is in tests/_parity.py)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.resnet_ref import _r, _w

STAGES = ((2, 2, 24), (3, 2, 32), (4, 2, 64), (3, 1, 96), (3, 2, 160), (1, 1, 320))      # repeats, first stride, out
WIDTHS = {"mobilenetv2_035": 0.35, "mobilenetv2_050": 0.5, "mobilenetv2_075": 0.75, "mobilenetv2_100": 1.0, "mobilenetv2_140": 1.4}
TEST_ARCH = {"stem": 16, "first": 8, "stages": ((2, 2, 16), (1, 2, 24), (2, 1, 32)), "head": 64}


def make_divisible(v, divisor=8, round_limit=0.9):
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new + divisor if new < round_limit * v else new


def layer_list(arch):
    """stem width, [(kind, in, mid, out, stride)] per stage, head width"""
    if arch == "mobilenetv2_test":
        t = TEST_ARCH
        stem, first, stages, head = t["stem"], t["first"], t["stages"], t["head"]
    else:
        m = WIDTHS[arch]
        stem, first = make_divisible(32 * m), make_divisible(16 * m)
        stages = tuple((n, s, make_divisible(c * m)) for n, s, c in STAGES)
        head = max(1280, make_divisible(1280 * m))
    out, cin = [[("ds", stem, stem, first, 1)]], first
    for n, s, c in stages:
        stage = []
        for i in range(n):
            stage.append(("ir", cin, make_divisible(cin * 6), c, s if i == 0 else 1))
            cin = c
        out.append(stage)
    return stem, out, head


def param_count(arch, num_classes=1000):
    stem, stages, head = layer_list(arch)
    n = 27 * stem + 2 * stem
    for stage in stages:
        for kind, cin, mid, cout, _ in stage:
            if kind == "ds":
                n += 9 * cin + 2 * cin + cin * cout + 2 * cout
            else:
                n += cin * mid + 2 * mid + 9 * mid + 2 * mid + mid * cout + 2 * cout
            last = cout
    return n + last * head + 2 * head + head * num_classes + num_classes


class _Force(torch.autograd.Function):
    """value of `v`, gradient of `t`: a stored tensor of another run of the same network put in the place of this run's own"""

    @staticmethod
    def forward(ctx, t, v):
        return v.to(t.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class Tape:
    """The tensors a run STORES, in forward order: the packed input, every convolution output, the activations a2 / head (not the
    stem's and not the expanded a1, which the HIP path never stores), every block output, the pooled vector, the logits.
    Tape() records them; Tape(values) puts `values` in their place (teacher forcing): the run then sees the other run's tensors at
    every stored point, so the two cannot drift apart and ReLU6 masks and batch statistics are those of the same numbers."""

    def __init__(self, values=None):
        self.values, self.rec, self.i = (None if values is None else list(values)), [], 0

    def __call__(self, t):
        if self.values is None:
            self.rec.append(t.detach().clone())
            return t
        v = self.values[self.i]
        self.i += 1
        assert tuple(v.shape) == tuple(t.shape), (self.i, tuple(v.shape), tuple(t.shape))
        return _Force.apply(t, v)


def _pt(m, t):
    return t if m.tape is None else m.tape(t)


def _conv(x, conv, q):
    return _r(F.conv2d(x, _w(conv.weight, q), None, conv.stride, conv.padding, 1, conv.groups), q)


def _act(bn, y, q):
    """the stored (or formed-on-load) activation: relu6(bn(y)) rounded once"""
    return _r(F.hardtanh(bn(y), 0.0, 6.0), q)


class _DS(nn.Module):
    def __init__(self, cin, cout, q):
        super().__init__()
        self.q, self.tape = q, None
        self.conv_dw = nn.Conv2d(cin, cin, 3, 1, 1, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)

    def forward(self, x):
        a = _pt(self, _act(self.bn1, _pt(self, _conv(x, self.conv_dw, self.q)), self.q))
        return _pt(self, _r(self.bn2(_pt(self, _conv(a, self.conv_pw, self.q))), self.q))


class _IR(nn.Module):
    def __init__(self, cin, mid, cout, stride, q):
        super().__init__()
        self.q, self.residual = q, stride == 1 and cin == cout
        self.trace = self.tape = None
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, 3, stride, 1, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)

    def forward(self, x):
        q = self.q
        a1 = _act(self.bn1, _pt(self, _conv(x, self.conv_pw, q)), q)      # never stored by the HIP path, but rounded once all the same
        if self.trace is not None:
            self.trace.append(a1.detach())
        a2 = _pt(self, _act(self.bn2, _pt(self, _conv(a1, self.conv_dw, q)), q))
        o = self.bn3(_pt(self, _conv(a2, self.conv_pwl, q)))
        return _pt(self, _r(o + x if self.residual else o, q))


class MobileNetV2Ref(nn.Module):
    """bf16_points: the rounding points of the HIP path (input, filters, every convolution output, every activation -- the
    expanded one included --, every block output, the pooled vector, the logits; their gradients likewise)."""

    def __init__(self, arch="mobilenetv2_100", num_classes=1000, bf16_points=False):
        super().__init__()
        self.q, self.tape = bf16_points, None
        stem, stages, head = layer_list(arch)
        self.conv_stem = nn.Conv2d(3, stem, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem)
        self.blocks = nn.Sequential(*[nn.Sequential(*[_DS(cin, cout, bf16_points) if kind == "ds" else _IR(cin, mid, cout, s, bf16_points)
                                                      for kind, cin, mid, cout, s in stage]) for stage in stages])
        self.conv_head = nn.Conv2d(stages[-1][-1][3], head, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(head)
        self.classifier = nn.Linear(head, num_classes)
        for m in self.modules():                                  # timm's _init_weight_goog
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0.0, (2.0 / fan_out) ** 0.5)
        rng = 1.0 / num_classes ** 0.5
        nn.init.uniform_(self.classifier.weight, -rng, rng)
        nn.init.zeros_(self.classifier.bias)

    def set_trace(self, trace):
        """trace: a list that receives the expanded activation a1 of every inverted-residual block"""
        for m in self.modules():
            if isinstance(m, _IR):
                m.trace = trace

    def set_tape(self, tape):
        """tape: a Tape (or None) that every stored tensor of the forward passes through"""
        for m in self.modules():
            if isinstance(m, (_IR, _DS, MobileNetV2Ref)):
                m.tape = tape

    def forward(self, x):
        q = self.q
        x = _act(self.bn1, _pt(self, _conv(_pt(self, _r(x, q)), self.conv_stem, q)), q)
        x = self.blocks(x)
        x = _pt(self, _act(self.bn2, _pt(self, _conv(x, self.conv_head, q)), q))
        pooled = _pt(self, _r(x.mean(dim=(2, 3)), q))
        return _pt(self, _r(F.linear(pooled, _w(self.classifier.weight, q), self.classifier.bias), q))


def plain_sequential(arch, num_classes):
    """The same network out of nn.Conv2d / nn.BatchNorm2d / nn.ReLU6 alone (a residual wrapper where a block adds its input): what
    MobileNetV2Ref(bf16_points=False) must equal; parameters in the same order."""
    class Residual(nn.Module):
        def __init__(self, body):
            super().__init__()
            self.body = body

        def forward(self, x):
            return x + self.body(x)

    def cba(cin, cout, k, s, groups, act):
        return [nn.Conv2d(cin, cout, k, s, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)] + ([nn.ReLU6()] if act else [])

    stem, stages, head = layer_list(arch)
    mods = cba(3, stem, 3, 2, 1, True)
    for stage in stages:
        for kind, cin, mid, cout, s in stage:
            if kind == "ds":
                mods += cba(cin, cin, 3, 1, cin, True) + cba(cin, cout, 1, 1, 1, False)
            else:
                body = nn.Sequential(*(cba(cin, mid, 1, 1, 1, True) + cba(mid, mid, 3, s, mid, True) + cba(mid, cout, 1, 1, 1, False)))
                mods.append(Residual(body) if s == 1 and cin == cout else body)
            last = cout
    mods += cba(last, head, 1, 1, 1, True) + [nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(head, num_classes)]
    return nn.Sequential(*mods)


def perturb(ref, seed):
    """BatchNorm weights U(2, 3), biases N(0.3, 0.2), random running statistics: ReLU6 clamps at both ends"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(2.0 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.3 + 0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return ref
