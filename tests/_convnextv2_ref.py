"""CPU oracle of ConvNeXt V2 in plain torch, and the closed forms of its Global Response Normalisation (TEST INFRASTRUCTURE ONLY).

The block follows oracle/convnext_ref.py with timm's V2 changes: no layer scale, and `GlobalResponseNorm` between GELU and fc2
(parameter names `mlp.grn.weight` / `mlp.grn.bias`, between `mlp.fc1.*` and `mlp.fc2.*`).  timm is not installed where these tests
run: the expression is restated from memory, as tests/_swin_ref.py does for Swin.

  grn_timm          timm's expression, channels last (the autograd reference)
  grn_closed_form   the forward and backward the kernels of csrc/grn.hip implement, in whatever dtype the inputs have
  grn_plan          Python mirror of icamd_grn_plan / reduce_tcols (csrc/grn.hip): the launch geometry and the trips of every loop
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.convnext_ref import _Head, _Mlp, _ln2d, _r, _w

GRN_EPS = 1e-6

CONFIGS = {
    "convnextv2_pico": ((2, 2, 6, 2), (64, 128, 256, 512)),
    "convnextv2_tiny": ((3, 3, 9, 3), (96, 192, 384, 768)),
    "convnextv2_base": ((3, 3, 27, 3), (128, 256, 512, 1024)),
    "convnextv2_large": ((3, 3, 27, 3), (192, 384, 768, 1536)),
    "convnextv2_test": ((1, 1, 2, 1), (32, 64, 128, 192)),
}
PARAM_COUNTS = {"convnextv2_pico": 9066280, "convnextv2_tiny": 28635496, "convnextv2_base": 88717800,
                "convnextv2_large": 197956840}


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


def cdiv(a, b):
    return (a + b - 1) // b


def grn_plan(N, HW, C):
    """icamd_grn_plan and reduce_tcols (csrc/grn.hip), and the trip count of every loop of its kernels whose length depends on
    the problem, for the busiest thread."""
    cpr = C // 8
    S = max(min(cdiv(2048, N), cdiv(HW, 32), 64), 1)
    rps = cdiv(HW, S)
    S = cdiv(HW, rps)
    B = max(min(cdiv(HW * cpr, 1024), cdiv(4096, N), cdiv(HW, 8)), 1)
    rpb = cdiv(HW, B)
    B = cdiv(HW, rpb)
    tcols = cpr if cpr <= 256 else max(t for t in range(8, 257, 8) if cpr % t == 0)
    rlanes = 256 // tcols
    return {"S": S, "rps": rps, "B": B, "rpb": rpb, "tcols": tcols, "ctiles": cpr // tcols, "rlanes": rlanes,
            "trips": {"reduce rows": cdiv(rps, rlanes),                  # grn_reduce_kernel: r += rlanes
                      "reduce lds outputs": cdiv(tcols * 8, 256),        # o += 256 (the backward's walks twice as far)
                      "reduce row lanes": rlanes,                        # l < rlanes
                      "prologue channels": cdiv(C, 1024),                # c4 += 256, four channels each (grn_stats, s / t loops)
                      "prologue segments": S,                            # s < S
                      "apply vectors": cdiv(rpb * cpr, 256),             # i += 256
                      "parameter-gradient samples": cdiv(N, 4)}}         # grn_param_grads_kernel: n += 4


# ---------------------------------------------------------------------------------------------------------------- model
class _Grn(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _MlpV2(_Mlp):
    def __init__(self, dim):
        super().__init__(dim)
        fc2 = self.fc2
        del self.fc2
        self.grn = _Grn(4 * dim)          # registered between fc1 and fc2: timm's order
        self.fc2 = fc2


class _BlockV2(nn.Module):
    def __init__(self, dim, q):
        super().__init__()
        self.q = q
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _MlpV2(dim)
        self.keep = None   # injected per-sample stochastic-depth factor (float [B]) or None

    def forward(self, x):
        q = self.q
        d = _r(F.conv2d(x, _w(self.conv_dw.weight, q), self.conv_dw.bias, padding=3, groups=x.shape[1]), q)
        h = _r(self.norm(d.permute(0, 2, 3, 1)), q)
        z1 = _r(F.linear(h, _w(self.mlp.fc1.weight, q), self.mlp.fc1.bias), q)
        a = _r(F.gelu(z1), q)
        g = _r(grn_timm(a, self.mlp.grn.weight, self.mlp.grn.bias), q)
        z2 = _r(F.linear(g, _w(self.mlp.fc2.weight, q), self.mlp.fc2.bias), q)
        if self.keep is None:
            return _r(x + z2.permute(0, 3, 1, 2), q)
        return _r(x + (self.keep.to(x.dtype).view(-1, 1, 1, 1) * z2).permute(0, 3, 1, 2), q)


class _StageV2(nn.Module):
    def __init__(self, prev, dim, depth, q, first):
        super().__init__()
        self.downsample = nn.Identity() if first else nn.Sequential(nn.LayerNorm(prev, eps=1e-6), nn.Conv2d(prev, dim, 2, 2))
        self.blocks = nn.Sequential(*[_BlockV2(dim, q) for _ in range(depth)])


class ConvNeXtV2Ref(nn.Module):
    def __init__(self, arch="convnextv2_tiny", num_classes=1000, bf16_points=False):
        super().__init__()
        depths, dims = CONFIGS[arch]
        self.q = bf16_points
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, 4), nn.LayerNorm(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[_StageV2(dims[i - 1] if i else dims[0], dims[i], depths[i], bf16_points, i == 0)
                                      for i in range(4)])
        self.head = _Head(dims[-1], num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def all_blocks(self):
        return [b for st in self.stages for b in st.blocks]

    def forward(self, x):
        q = self.q
        x = _r(x, q)
        s = _r(F.conv2d(x, _w(self.stem[0].weight, q), self.stem[0].bias, stride=4), q)
        x = _r(_ln2d(s, self.stem[1]), q)
        for st in self.stages:
            if not isinstance(st.downsample, nn.Identity):
                ln = _r(_ln2d(x, st.downsample[0]), q)
                x = _r(F.conv2d(ln, _w(st.downsample[1].weight, q), st.downsample[1].bias, stride=2), q)
            x = st.blocks(x)
        pool = _r(x.mean(dim=(2, 3)), q)
        pn = _r(self.head.norm(pool), q)
        return _r(F.linear(pn, _w(self.head.fc.weight, q), self.head.fc.bias), q)
