"""What the EfficientNet tests share (TEST INFRASTRUCTURE ONLY): the launch geometry of csrc/dwconv5x5.hip mirrored in Python, the
fp64 references of the depthwise 5x5, BatchNorm + SiLU and MBConv squeeze-and-excitation entries, and timm's efficientnet_b0 / b1
restated in plain torch from the layer list (timm is not importable here; the parameter counts are checked against what torchvision
publishes for the same architectures in tests/test_efficientnet_cpu.py).  Imports nothing of the product; importing needs no GPU."""
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ops_ref as R
from oracle.mobilenet_ref import Tape  # noqa: F401  (the tests take it from here)
from oracle.resnet_ref import _r, _w

# ---------------------------------------------------------------------------------------------------------------- depthwise 5x5
RS = 16                                                    # output rows per item (dwconv5x5.hip)
# (N, H, W, C), each at stride 1 and 2: the issue's eight; trips() below shows they run every loop more than once
SHAPES = [(2, 2, 3, 8), (1, 1, 5, 16), (2, 7, 7, 24), (3, 9, 11, 48), (2, 14, 14, 144), (3, 37, 41, 40), (2, 5, 5, 1152),
          (2100, 3, 5, 16)]


def cdiv(a, b):
    return (a + b - 1) // b


def geometry(N, H, W, C, stride, cap, pixels_per_row):
    """dw5_geometry: forward (cap 2048, 16 pixels per partial row) and weight gradient (1024, 64)"""
    OH, OW, cpr = (H - 1) // stride + 1, (W - 1) // stride + 1, C // 8
    cv = min(cpr, 256)
    while cpr % cv or (256 // cv) * cv < 192:
        cv -= 1
    lanes = 256 // cv
    colgroups, rowsegs = cdiv(OW, lanes), cdiv(OH, RS)
    items = N * rowsegs * colgroups
    target = min(cap, max(32, N * OH * OW // pixels_per_row))
    ipb = cdiv(items, target)
    return {"OH": OH, "OW": OW, "cv": cv, "lanes": lanes, "nslices": cpr // cv, "colgroups": colgroups, "rowsegs": rowsegs,
            "items": items, "ipb": ipb, "rows": cdiv(items, ipb)}


def fwd_geometry(N, H, W, C, stride):
    return geometry(N, H, W, C, stride, 2048, 16)


def wgrad_geometry(N, H, W, C, stride):
    return geometry(N, H, W, C, stride, 1024, 64)


def trips(N, H, W, C, stride):
    """trip count of every loop of dwconv5_fwd_kernel / dwconv5_wgrad_kernel whose length depends on the problem"""
    f, w = fwd_geometry(N, H, W, C, stride), wgrad_geometry(N, H, W, C, stride)
    return {"items of a workgroup, forward": f["ipb"], "items of a workgroup, weight gradient": w["ipb"],
            "rows of a segment": min(RS, f["OH"]), "row segments": f["rowsegs"], "column groups": f["colgroups"],
            "column lanes folded per output": f["lanes"], "LDS outputs of the statistics fold (o += 256)": cdiv(f["cv"] * 16, 256),
            "LDS outputs of a kernel row of taps (o += 256)": cdiv(w["cv"] * 40, 256), "channel slices per pixel": f["nslices"],
            "partial rows, forward": f["rows"], "partial rows, weight gradient": w["rows"]}


def dwconv5_ref(x_nhwc, w_c55, dy_nhwc, stride):
    """F.conv2d(groups=C, padding=2) in fp64 and autograd: y and dx on the bf16 grid, dw [C,5,5]"""
    C = x_nhwc.shape[-1]
    a = R.nhwc_to_nchw(x_nhwc.double()).requires_grad_(True)
    w = w_c55.double().reshape(C, 1, 5, 5).clone().requires_grad_(True)
    y = F.conv2d(a, w, None, stride, 2, 1, C)
    y.backward(R.nhwc_to_nchw(dy_nhwc.double()))
    return R.bf16_round(R.nchw_to_nhwc(y.detach())), R.bf16_round(R.nchw_to_nhwc(a.grad)), w.grad.reshape(C, 5, 5)


@functools.lru_cache(maxsize=None)
def dw5_case(shape, stride):
    """operands and the fp64 reference of one case, computed once"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(2000 + 7 * N + H + 3 * stride)
    x = R.bf16_round(1.5 * torch.randn(N, H, W, C, generator=g))
    w = R.bf16_round(0.2 * torch.randn(C, 5, 5, generator=g))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = R.bf16_round(torch.randn(N, OH, OW, C, generator=g))
    y, dx, dw = dwconv5_ref(x, w, dy, stride)
    return {"x": x, "w": w, "dy": dy, "y": y, "dx": dx, "dw": dw, "OH": OH, "OW": OW}


# ---------------------------------------------------------------------------------------------------------------- BatchNorm + SiLU, SE
def silu64(z):
    z = z.double()
    return z * torch.sigmoid(z)


def silu_grad64(z):
    sg = torch.sigmoid(z.double())
    return sg * (1.0 + z.double() * (1.0 - sg))


def bn_silu(y, scale, shift):
    """a = bf16(silu(fma32(y, scale, shift))), the silu in fp64 on the kernel's fp32 z: what icamd_bn_apply_silu stores"""
    return R.bf16_round(silu64(R.fma32(y, scale, shift)).float())


def boundary_share(y, scale, shift):
    """share of the elements whose fp64 silu(z) sits within 2^-13 (relative: 8 fp32 ulps) of the midpoint between two bf16 values: where
    a kernel whose fp32 silu is a few ulps off may round the other way"""
    v = silu64(R.fma32(y, scale, shift))
    lo = v.float().view(torch.int32).bitwise_and(-65536).view(torch.float32).double()        # truncated to the bf16 grid
    step = torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-300))) - 7)
    mid = lo + torch.sign(v) * step / 2
    return float(((v - mid).abs() <= v.abs() * 2.0 ** -13).float().mean())


def excite_fwd(asum, inv_hw, w1, b1, w2, b2):
    """fp64: s, hpre, e"""
    s = asum.double() * inv_hw
    hpre = s @ w1.double().t() + b1.double()
    e = torch.sigmoid(silu64(hpre) @ w2.double().t() + b2.double())
    return s, hpre, e


def excite_bwd(de, s, hpre, e, w1, w2, inv_hw):
    """fp64, the kernels' form: dw1, db1, dw2, db2, dsn"""
    de, s, hpre, e, w1, w2 = (t.double() for t in (de, s, hpre, e, w1, w2))
    dp2 = de * e * (1 - e)
    dw2, db2 = dp2.t() @ silu64(hpre), dp2.sum(0)
    dh = (dp2 @ w2) * silu_grad64(hpre)
    dw1, db1 = dh.t() @ s, dh.sum(0)
    return dw1, db1, dw2, db2, (dh @ w1) * inv_hw


def bn_bwd_silu(dout, y, mean, invstd, scale, shift, e=None, dsn=None, fp32_z=True):
    """fp64, the kernels' two passes: g = upstream * silu'(z); (dgamma, dbeta) = (sum g xhat, sum g); dy = scale (g - mean g - xhat mean
    (g xhat)).  dout, y [N][HW][C]; e, dsn [N][C]"""
    z = R.fma32(y, scale, shift).double() if fp32_z else y.double() * scale.double() + shift.double()
    up = dout.double() if e is None else dout.double() * e.double()[:, None, :] + dsn.double()[:, None, :]
    g = up * silu_grad64(z)
    xhat = (y.double() - mean.double()) * invstd.double()
    M = y.shape[0] * y.shape[1]
    dbeta, dgamma = g.sum((0, 1)), (g * xhat).sum((0, 1))
    dy = scale.double() * (g - dbeta / M - xhat * (dgamma / M))
    return dy, dgamma, dbeta


def se_block_two_pass(y, gamma, beta, w1, b1, w2, b2, dout, eps=1e-5):
    """BatchNorm (batch statistics) + SiLU + SE gate and its backward in fp64 without rounding, in the order the kernels take: squeeze
    pass, excite, apply pass; gate-gradient pass, excite backward, reduce pass, apply pass.  y, dout [N][HW][C]"""
    y = y.double()
    N, HW, C = y.shape
    mean, var = y.mean((0, 1)), y.var((0, 1), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    a = silu64(y * scale + shift)
    s, hpre, e = excite_fwd(a.sum(1), 1.0 / HW, w1, b1, w2, b2)
    out = a * e[:, None, :]
    de = (dout.double() * a).sum(1)
    dw1, db1, dw2, db2, dsn = excite_bwd(de, s, hpre, e, w1, w2, 1.0 / HW)
    dy, dgamma, dbeta = bn_bwd_silu(dout, y, mean, invstd, scale, shift, e, dsn, fp32_z=False)
    return out, {"y": dy, "gamma": dgamma, "beta": dbeta, "w1": dw1, "b1": db1, "w2": dw2, "b2": db2}


def se_block_autograd(y, gamma, beta, w1, b1, w2, b2, dout, eps=1e-5):
    """the plain expression under fp64 autograd"""
    t = {k: v.double().clone().requires_grad_(True) for k, v in (("y", y), ("gamma", gamma), ("beta", beta), ("w1", w1), ("b1", b1),
                                                                 ("w2", w2), ("b2", b2))}
    N, HW, C = y.shape
    a = F.silu(F.batch_norm(t["y"].reshape(N * HW, C), None, None, t["gamma"], t["beta"], True, 0.0, eps)).reshape(N, HW, C)
    gate = torch.sigmoid(F.linear(F.silu(F.linear(a.mean(1), t["w1"], t["b1"])), t["w2"], t["b2"]))
    out = a * gate[:, None, :]
    (out * dout.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in t.items()}


# ---------------------------------------------------------------------------------------------------------------- the model
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


def _pt(m, t):
    return t if m.tape is None else m.tape(t)


def _conv(x, conv, q):
    return _r(F.conv2d(x, _w(conv.weight, q), None, conv.stride, conv.padding, 1, conv.groups), q)


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


def efficientnet_pair(arch, C, perturbed, seed=0):
    from imageclassification_amd.efficientnet import EfficientNet
    torch.manual_seed(seed)
    ref = EfficientNetRef(arch, C, bf16_points=True)
    if perturbed:
        perturb(ref, seed + 1)
    net = EfficientNet(arch, C)
    net.load_state_dict(ref.state_dict())
    return ref, net
