"""CPU oracle for the Swin Transformer family (TEST INFRASTRUCTURE ONLY): timm's `swin_*_patch4_window7_224` and
`swin_base_patch4_window12_384` in plain torch.

timm is absent, so the architecture is restated the way timm writes it -- `torch.roll`, `window_partition` / `window_reverse`, the
`img_mask` built by slices, the `relative_position_index` buffer, patch merging at the head of stages 1.. -- with timm's module and
parameter names ("timm-unpinned", like oracle/vit_ref.py).  `bf16_points=True` inserts the HIP path's rounding points (see
oracle/resnet_ref.py): every stored activation and every weight used in a product.  The softmax probabilities and dS stay fp32 here:
the attention bounds of the tests are the project's against exactly such an oracle.

Also the kernel-level references `window_attention_ref` and `patch_merge_ln_ref`.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .resnet_ref import _RoundBF16, _RoundWeight

# (embed dim, depths, heads, window)
CONFIGS = {
    "swin_tiny_patch4_window7_224": (96, (2, 2, 6, 2), (3, 6, 12, 24), 7),
    "swin_small_patch4_window7_224": (96, (2, 2, 18, 2), (3, 6, 12, 24), 7),
    "swin_base_patch4_window7_224": (128, (2, 2, 18, 2), (4, 8, 16, 32), 7),
    "swin_test": (32, (2, 2), (1, 2), 7),
    "swin_base_patch4_window12_384": (128, (2, 2, 18, 2), (4, 8, 16, 32), 12),
    "swin_test_w12": (32, (2, 2), (1, 2), 12),
}


def _r(x, on):
    return _RoundBF16.apply(x) if on else x


def _w(w, on):
    return _RoundWeight.apply(w) if on else w


def window_partition(x, ws):
    """[B, H, W, C] -> [B * nW, ws, ws, C]"""
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def window_reverse(windows, ws, H, W):
    C = windows.shape[-1]
    x = windows.view(-1, H // ws, W // ws, ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, H, W, C)


def relative_position_index(ws):
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = flat[:, :, None] - flat[:, None, :]
    rel = rel.permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def shifted_window_mask(H, W, ws, shift):
    """timm's attn_mask: [nW, ws^2, ws^2] with -100 between tokens of different regions, or None without a shift."""
    if shift == 0:
        return None
    img_mask = torch.zeros(1, H, W, 1)
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img_mask[:, h, w, :] = cnt
            cnt += 1
    mw = window_partition(img_mask, ws).view(-1, ws * ws)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)


class _WindowAttention(nn.Module):
    def __init__(self, dim, heads, ws):
        super().__init__()
        self.heads, self.ws = heads, ws
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) ** 2, heads))
        self.register_buffer("relative_position_index", relative_position_index(ws), persistent=False)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def bias(self):
        T = self.ws * self.ws
        b = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(T, T, -1)
        return b.permute(2, 0, 1).contiguous()


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, res, heads, ws, shift, q):
        super().__init__()
        self.q, self.res, self.ws, self.shift = q, res, ws, shift
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, heads, ws)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, 4 * dim)
        self.register_buffer("attn_mask", shifted_window_mask(res, res, ws, shift), persistent=False)
        self.keep = (None, None)      # injected drop-path masks (float [B], already divided by keep_prob), one per branch

    def _attn(self, h):
        q, a = self.q, self.attn
        B, H, W, C = h.shape
        ws, nh = self.ws, a.heads
        qkv = _r(F.linear(h, _w(a.qkv.weight, q), a.qkv.bias), q)
        sh = torch.roll(qkv, shifts=(-self.shift, -self.shift), dims=(1, 2)) if self.shift > 0 else qkv
        xw = window_partition(sh, ws).view(-1, ws * ws, 3 * C)
        B_, N, _ = xw.shape
        qq, kk, vv = xw.reshape(B_, N, 3, nh, -1).permute(2, 0, 3, 1, 4)
        att = (qq * (C // nh) ** -0.5) @ kk.transpose(-2, -1) + a.bias().unsqueeze(0)
        if self.attn_mask is not None:
            nW = self.attn_mask.shape[0]
            att = att.view(-1, nW, nh, N, N) + self.attn_mask.to(att.dtype).unsqueeze(1).unsqueeze(0)
            att = att.view(-1, nh, N, N)
        att = torch.softmax(att, dim=-1)
        o = (att @ vv).transpose(1, 2).reshape(B_, N, C)
        o = window_reverse(o.view(-1, ws, ws, C), ws, H, W)
        if self.shift > 0:
            o = torch.roll(o, shifts=(self.shift, self.shift), dims=(1, 2))
        ao = _r(o, q)
        return F.linear(ao, _w(a.proj.weight, q), a.proj.bias)

    def _dp(self, x, branch, keep):
        """x + drop_path(branch): without a mask the sum is rounded once (the residual rides in the GEMM epilogue); with one the
        branch is stored (rounded) first"""
        q = self.q
        if keep is None:
            return _r(x + branch, q)
        k = keep.to(branch.dtype).view(-1, 1, 1, 1)
        return _r(x + k * _r(branch, q), q)

    def forward(self, x):
        q = self.q
        x1 = self._dp(x, self._attn(_r(self.norm1(x), q)), self.keep[0])
        h2 = _r(self.norm2(x1), q)
        z = _r(F.linear(h2, _w(self.mlp.fc1.weight, q), self.mlp.fc1.bias), q)
        a = _r(F.gelu(z), q)
        return self._dp(x1, F.linear(a, _w(self.mlp.fc2.weight, q), self.mlp.fc2.bias), self.keep[1])


class _PatchMerging(nn.Module):
    def __init__(self, dim, q):
        super().__init__()
        self.q = q
        self.norm = nn.LayerNorm(4 * dim)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        q = self.q
        B, H, W, C = x.shape
        x = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3)     # x0 | x1 | x2 | x3
        x = _r(self.norm(x), q)
        return _r(F.linear(x, _w(self.reduction.weight, q)), q)


class _Stage(nn.Module):
    def __init__(self, dim, res, depth, heads, window, downsample, q):
        super().__init__()
        self.downsample = _PatchMerging(dim // 2, q) if downsample else nn.Identity()
        ws, shift = (res, 0) if res <= window else (window, window // 2)
        self.blocks = nn.Sequential(*[_Block(dim, res, heads, ws, 0 if j % 2 == 0 else shift, q) for j in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class _PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, 4, 4)
        self.norm = nn.LayerNorm(dim)


class _Head(nn.Module):
    def __init__(self, dim, num_classes):
        super().__init__()
        self.fc = nn.Linear(dim, num_classes)


class SwinRef(nn.Module):
    def __init__(self, arch="swin_tiny_patch4_window7_224", num_classes=1000, img_size=224, bf16_points=False):
        super().__init__()
        embed, depths, heads, window = CONFIGS[arch]
        self.q = bf16_points
        self.patch_embed = _PatchEmbed(embed)
        res = img_size // 4
        layers = []
        for i, depth in enumerate(depths):
            if i > 0:
                res //= 2
            layers.append(_Stage(embed << i, res, depth, heads[i], window, i > 0, bf16_points))
        self.layers = nn.Sequential(*layers)
        last = embed << (len(depths) - 1)
        self.norm = nn.LayerNorm(last)
        self.head = _Head(last, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def blocks(self):
        return [b for st in self.layers for b in st.blocks]

    def forward(self, x):
        q = self.q
        x = _r(x, q)
        pe = self.patch_embed
        x = _r(F.conv2d(x, _w(pe.proj.weight, q), pe.proj.bias, stride=4), q).permute(0, 2, 3, 1)      # NHWC from here on
        x = _r(pe.norm(x), q)
        x = self.layers(x)
        x = _r(self.norm(x), q)
        pooled = _r(x.mean(dim=(1, 2)), q)
        return _r(F.linear(pooled, _w(self.head.fc.weight, q), self.head.fc.bias), q)


# ---------------------------------------------------------------------------------------------------- kernel-level references
def window_attention_ref(qkv, bias, B, Hs, Ws, H, ws, shift, dout=None, acc=torch.float64):
    """qkv [B, Hs, Ws, 3*H*32] (bf16-representable), bias [H, ws^2, ws^2].  Returns out [B, Hs, Ws, H*32] and lse [B*nW, H, ws^2]
    (both `acc` precision, unrounded); with dout also (dqkv, dbias)."""
    D = 32
    x = qkv.detach().to(acc).reshape(B, Hs, Ws, 3 * H * D).requires_grad_(dout is not None)
    bb = bias.detach().to(acc).requires_grad_(dout is not None)
    sh = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else x
    xw = window_partition(sh, ws).view(-1, ws * ws, 3 * H * D)
    B_, N, _ = xw.shape
    q, k, v = xw.reshape(B_, N, 3, H, D).permute(2, 0, 3, 1, 4)
    att = (q @ k.transpose(-2, -1)) * D ** -0.5 + bb.unsqueeze(0)
    mask = shifted_window_mask(Hs, Ws, ws, shift)
    if mask is not None:
        nW = mask.shape[0]
        att = (att.view(-1, nW, H, N, N) + mask.to(att).unsqueeze(1).unsqueeze(0)).view(-1, H, N, N)
    lse = torch.logsumexp(att, dim=-1)
    o = (torch.softmax(att, dim=-1) @ v).transpose(1, 2).reshape(B_, N, H * D)
    o = window_reverse(o.view(-1, ws, ws, H * D), ws, Hs, Ws)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    if dout is None:
        return o.detach(), lse.detach()
    o.backward(dout.to(acc).reshape(o.shape))
    return o.detach(), lse.detach(), x.grad, bb.grad


def patch_merge_gather(x):
    """[N, H, W, C] -> [N * H/2 * W/2, 4C] in timm's x0 | x1 | x2 | x3 order"""
    N, H, W, C = x.shape
    x0, x1 = x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :]
    x2, x3 = x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]
    return torch.cat([x0, x1, x2, x3], -1).reshape(-1, 4 * C)


def patch_merge_ln_ref(x, gamma, beta, eps, dy=None, acc=torch.float64):
    """Returns y (unrounded), mean, rstd; with dy also dx [N, H, W, C], dgamma, dbeta."""
    xf = x.detach().to(acc).requires_grad_(dy is not None)
    g = gamma.detach().to(acc).requires_grad_(dy is not None)
    b = beta.detach().to(acc).requires_grad_(dy is not None)
    rows = patch_merge_gather(xf)
    mean = rows.mean(-1)
    rstd = torch.rsqrt(((rows - mean[:, None]) ** 2).mean(-1) + eps)
    y = F.layer_norm(rows, (rows.shape[-1],), g, b, eps)
    if dy is None:
        return y.detach(), mean.detach(), rstd.detach()
    y.backward(dy.to(acc))
    return y.detach(), mean.detach(), rstd.detach(), xf.grad, g.grad, b.grad
