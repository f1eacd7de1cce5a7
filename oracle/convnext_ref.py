"""CPU oracle: ConvNeXt V1 and V2 (timm `convnext_tiny` / `convnextv2_tiny` families) in plain torch, and the closed forms of V2's
Global Response Normalisation (TEST INFRASTRUCTURE ONLY).

Block / stem / downsample arithmetic follows the reference tree's own ConvNeXt definition
(/root/reference/semantic_segmentation/backbone/convnext.py:21-56 block, :79-88 stem and downsample, :158-182
LayerNorm) with timm's classification head (global average pool -> LayerNorm -> Linear) and timm's parameter names
[recall]; timm cannot be imported.  Parameter count 28,589,128 for convnext_tiny is
checked in tests/test_oracle_cpu.py.  Stochastic-depth masks are INJECTED (per block, float [B], already scaled by
1/keep_prob) so that parity tests do not depend on RNG streams.  `bf16_points=True`: see oracle/resnet_ref.py.

V2 is timm's change to the block: no layer scale, and `GlobalResponseNorm` between GELU and fc2 (parameter names `mlp.grn.weight` /
`mlp.grn.bias`, between `mlp.fc1.*` and `mlp.fc2.*`).  The expression is restated from memory, as oracle/swin_ref.py does for Swin.

  grn_timm          timm's expression, channels last (the autograd reference)
  grn_closed_form   the forward and backward the kernels of csrc/grn.hip implement, in whatever dtype the inputs have
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .resnet_ref import _RoundBF16, _RoundWeight

GRN_EPS = 1e-6

CONFIGS = {"convnext_tiny": ((3, 3, 9, 3), (96, 192, 384, 768)), "convnext_small": ((3, 3, 27, 3), (96, 192, 384, 768)),
           "convnext_test": ((1, 1, 2, 1), (32, 64, 128, 192)),
           # the configuration of tests/golden/convnext_ref_vectors.npz (generated from the reference's own backbone class)
           "convnext_pin": ((1, 1, 1, 1), (32, 64, 96, 192)),
           "convnextv2_pico": ((2, 2, 6, 2), (64, 128, 256, 512)),
           "convnextv2_tiny": ((3, 3, 9, 3), (96, 192, 384, 768)),
           "convnextv2_base": ((3, 3, 27, 3), (128, 256, 512, 1024)),
           "convnextv2_large": ((3, 3, 27, 3), (192, 384, 768, 1536)),
           "convnextv2_test": ((1, 1, 2, 1), (32, 64, 128, 192))}
V2_ARCHS = {name for name in CONFIGS if name.startswith("convnextv2_")}
PARAM_COUNTS = {"convnextv2_pico": 9066280, "convnextv2_tiny": 28635496, "convnextv2_base": 88717800,
                "convnextv2_large": 197956840}


def _r(x, on):
    return _RoundBF16.apply(x) if on else x


def _w(w, on):
    return _RoundWeight.apply(w) if on else w


def _ln2d(x, ln):
    return F.layer_norm(x.permute(0, 2, 3, 1), ln.normalized_shape, ln.weight, ln.bias, ln.eps).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- GRN
def grn_timm(a, weight, bias, eps=GRN_EPS):
    """timm GlobalResponseNorm(channels_last=True) on a [N, H, W, C] (or [N, HW, C]) tensor"""
    dims = tuple(range(1, a.dim() - 1))
    gx = a.norm(p=2, dim=dims, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + eps)
    return a + torch.addcmul(bias, weight, a * nx)


def grn_closed_form(a, weight, bias, dg=None, eps=GRN_EPS):
    """a, dg [N, HW, C]; -> dict(g, gx) and, with dg, da, dweight, dbias.  Evaluated in the dtype of the inputs."""
    C = a.shape[-1]
    G = (a * a).sum(1).sqrt()                                   # [N, C]
    m = G.mean(-1, keepdim=True) + eps
    Nx = G / m
    s = 1 + weight * Nx
    out = {"g": a * s[:, None, :] + bias, "gx": G}
    if dg is not None:
        P, Q = (dg * a).sum(1), dg.sum(1)
        dN = weight * P
        dG = dN / m - (dN * G).sum(-1, keepdim=True) / (C * m * m)
        t = torch.where(G > 0, dG / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
        out.update(da=dg * s[:, None, :] + a * t[:, None, :], dweight=(P * Nx).sum(0), dbias=Q.sum(0))
    return out


def gelu_grad(z):
    """d gelu(z) / dz, erf form"""
    return 0.5 * (1 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


# ---------------------------------------------------------------------------------------------------------------- model
class _Grn(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _Mlp(nn.Module):
    def __init__(self, dim, v2):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        fc2 = nn.Linear(4 * dim, dim)
        if v2:
            self.grn = _Grn(4 * dim)      # registered between fc1 and fc2: timm's order
        self.fc2 = fc2


class _Block(nn.Module):
    def __init__(self, dim, q, v2=False):
        super().__init__()
        self.q, self.v2 = q, v2
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, v2)
        if not v2:
            self.gamma = nn.Parameter(torch.full((dim,), 1e-6))
        self.keep = None   # injected per-sample stochastic-depth factor (float [B]) or None

    def forward(self, x):
        q = self.q
        d = _r(F.conv2d(x, _w(self.conv_dw.weight, q), self.conv_dw.bias, padding=3, groups=x.shape[1]), q)
        h = _r(self.norm(d.permute(0, 2, 3, 1)), q)
        z1 = _r(F.linear(h, _w(self.mlp.fc1.weight, q), self.mlp.fc1.bias), q)
        a = _r(F.gelu(z1), q)
        if self.v2:
            a = _r(grn_timm(a, self.mlp.grn.weight, self.mlp.grn.bias), q)
        z2 = _r(F.linear(a, _w(self.mlp.fc2.weight, q), self.mlp.fc2.bias), q)
        keep = None if self.keep is None else self.keep.to(x.dtype).view(-1, 1, 1, 1)
        if not self.v2:
            z2 = (1.0 if keep is None else keep) * self.gamma * z2
        elif keep is not None:
            z2 = keep * z2
        return _r(x + z2.permute(0, 3, 1, 2), q)


class _Stage(nn.Module):
    def __init__(self, prev, dim, depth, q, v2, first):
        super().__init__()
        self.downsample = nn.Identity() if first else nn.Sequential(nn.LayerNorm(prev, eps=1e-6), nn.Conv2d(prev, dim, 2, 2))
        self.blocks = nn.Sequential(*[_Block(dim, q, v2) for _ in range(depth)])


class _Head(nn.Module):
    def __init__(self, dim, num_classes):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.fc = nn.Linear(dim, num_classes)


class ConvNeXtRef(nn.Module):
    """`arch`: a name of CONFIGS (V2 where it starts with convnextv2_), or a (depths, dims) pair with `v2` given."""

    def __init__(self, arch="convnext_tiny", num_classes=1000, bf16_points=False, v2=None):
        super().__init__()
        if isinstance(arch, str):
            depths, dims = CONFIGS[arch]
            assert v2 is None or v2 == (arch in V2_ARCHS), (arch, v2)
            v2 = arch in V2_ARCHS
        else:
            assert v2 is not None, "a (depths, dims) pair says nothing of the version: pass v2="
            depths, dims = arch
        self.q, self.v2 = bf16_points, v2
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, 4), nn.LayerNorm(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[_Stage(dims[i - 1] if i else dims[0], dims[i], depths[i], bf16_points, v2, i == 0)
                                      for i in range(4)])
        self.head = _Head(dims[-1], num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def all_blocks(self):
        return [b for st in self.stages for b in st.blocks]

    def forward_features(self, x):
        """Raw output of every stage (reference backbone: convnext.py:138-150 before its per-output norms)."""
        q = self.q
        x = _r(x, q)
        s = _r(F.conv2d(x, _w(self.stem[0].weight, q), self.stem[0].bias, stride=4), q)
        x = _r(_ln2d(s, self.stem[1]), q)
        feats = []
        for st in self.stages:
            if not isinstance(st.downsample, nn.Identity):
                ln = _r(_ln2d(x, st.downsample[0]), q)
                x = _r(F.conv2d(ln, _w(st.downsample[1].weight, q), st.downsample[1].bias, stride=2), q)
            x = st.blocks(x)
            feats.append(x)
        return feats

    def forward(self, x):
        q = self.q
        x = self.forward_features(x)[-1]
        pool = _r(x.mean(dim=(2, 3)), q)
        pn = _r(self.head.norm(pool), q)
        return _r(F.linear(pn, _w(self.head.fc.weight, q), self.head.fc.bias), q)
