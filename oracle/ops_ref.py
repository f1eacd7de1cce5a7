"""CPU oracle for the per-step device operations (TEST INFRASTRUCTURE ONLY -- never imported by the product).

Each function restates, with torch-CPU fp32 primitives, the arithmetic one C-ABI entry point of
include/icamd.h performs, with the SAME bf16 rounding points as the HIP path (inputs are bf16 values held in
fp32, accumulation is fp32, the result is rounded once).  The reference itself has no kernels: the arithmetic
it relies on is what torch runs for timm's layers under /root/reference/engine.py:48,51,64,72 and for
torch.optim.AdamW / timm ModelEmaV3 / timm Mixup (engine.py:44,68,74,77); torch-CPU is therefore the pin.
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package.
"""
import math

import torch
import torch.nn.functional as F


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nhwc_to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nchw_to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---- accumulation precision -------------------------------------------------------------------------
# Every function below accumulates in fp32 by default (acc=torch.float32: the pinned behaviour).  With acc=torch.float64 the
# same formula, with the same bf16 rounding points, is accumulated in fp64 -- the reference of the full-size layer tests,
# which run it on the GPU on tensors of any device.  Convolutions then run as one fp64 matmul per filter tap (fp64
# convolution has no vendor kernel there).
def _wide(acc):
    """True for the fp64 path; the default fp32 path otherwise.  Any other dtype would be a reference narrower than fp32."""
    assert acc in (torch.float32, torch.float64), acc
    return acc == torch.float64


def _taps(xp, KH, KW, stride, OH, OW):
    """(r, s, view of the padded NHWC input read by tap (r, s)) for every filter tap."""
    for r in range(KH):
        for s in range(KW):
            yield r, s, xp[:, r:r + stride * (OH - 1) + 1:stride, s:s + stride * (OW - 1) + 1:stride, :]


def _out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _conv_fwd_taps(x, w, stride, pad):
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    OH, OW = _out_hw(H, W, KH, KW, stride, pad)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    y = torch.zeros(N * OH * OW, Cout, dtype=x.dtype, device=x.device)
    for r, s, xs in _taps(xp, KH, KW, stride, OH, OW):
        y.addmm_(xs.reshape(-1, Cin), w[:, r, s, :].t())
    return y.reshape(N, OH, OW, Cout)


def _conv_dgrad_taps(dy, w, in_hw, stride, pad):
    N, OH, OW, Cout = dy.shape
    _, KH, KW, Cin = w.shape
    H, W = in_hw
    dxp = torch.zeros(N, H + 2 * pad + stride, W + 2 * pad + stride, Cin, dtype=dy.dtype, device=dy.device)
    dy2 = dy.reshape(-1, Cout)
    for r, s, view in _taps(dxp, KH, KW, stride, OH, OW):
        view += (dy2 @ w[:, r, s, :]).reshape(N, OH, OW, Cin)
    return dxp[:, pad:pad + H, pad:pad + W, :]


def _conv_wgrad_taps(x, dy, ksize, stride, pad):
    N, OH, OW, Cout = dy.shape
    Cin = x.shape[-1]
    KH, KW = ksize
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    dy2t = dy.reshape(-1, Cout).t()
    dw = torch.empty(Cout, KH, KW, Cin, dtype=x.dtype, device=x.device)
    for r, s, xs in _taps(xp, KH, KW, stride, OH, OW):
        dw[:, r, s, :] = dy2t @ xs.reshape(-1, Cin)
    return dw


# ---- convolution: icamd_conv2d_fwd / _dgrad / _wgrad -----------------------------------------------
def conv2d_fwd(x_nhwc, w_krsc, stride, pad, bias=None, addend=None, acc=torch.float32):
    """x [N,H,W,Cin], w [Cout,KH,KW,Cin] (bf16-representable fp32). Returns (y rounded to bf16 grid, fp32)."""
    if _wide(acc):
        y = _conv_fwd_taps(x_nhwc.to(acc), w_krsc.to(acc), stride, pad)
        if bias is not None:
            y = y + bias.to(acc)
        if addend is not None:
            y = y + addend.to(acc)
        return bf16_round(y)
    x = nhwc_to_nchw(x_nhwc.float())
    w = w_krsc.float().permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    y = nchw_to_nhwc(y)
    if bias is not None:
        y = y + bias.float()
    if addend is not None:
        y = y + addend.float()
    return bf16_round(y)


def conv2d_stats(y_nhwc):
    """Per-channel sum and sum of squares of the rounded output (fp64 accumulate)."""
    y = y_nhwc.double().reshape(-1, y_nhwc.shape[-1])
    return y.sum(0), (y * y).sum(0)


def conv2d_dgrad(dy_nhwc, w_krsc, in_hw, stride, pad, addend=None, acc=torch.float32):
    if _wide(acc):
        dx = _conv_dgrad_taps(dy_nhwc.to(acc), w_krsc.to(acc), in_hw, stride, pad)
        if addend is not None:
            dx = dx + addend.to(acc)
        return bf16_round(dx)
    dy = nhwc_to_nchw(dy_nhwc.float())
    w = w_krsc.float().permute(0, 3, 1, 2).contiguous()
    N = dy.shape[0]
    dx = torch.nn.grad.conv2d_input((N, w.shape[1], in_hw[0], in_hw[1]), w, dy, stride=stride, padding=pad)
    dx = nchw_to_nhwc(dx)
    if addend is not None:
        dx = dx + addend.float()
    return bf16_round(dx)


def conv2d_wgrad(x_nhwc, dy_nhwc, ksize, stride, pad, acc=torch.float32):
    """Returns dw [Cout,KH,KW,Cin] fp32 (not rounded: the HIP path keeps weight gradients in fp32); in `acc` if that is wider."""
    if _wide(acc):
        return _conv_wgrad_taps(x_nhwc.to(acc), dy_nhwc.to(acc), ksize, stride, pad)
    x = nhwc_to_nchw(x_nhwc.float())
    dy = nhwc_to_nchw(dy_nhwc.float())
    Cout, Cin = dy.shape[1], x.shape[1]
    dw = torch.nn.grad.conv2d_weight(x, (Cout, Cin, ksize[0], ksize[1]), dy, stride=stride, padding=pad)
    return dw.permute(0, 2, 3, 1).contiguous()


# ---- BatchNorm: icamd_bn_train_finalize / _apply / _bwd ---------------------------------------------
def bn_train_coeffs(y_nhwc, gamma, beta, running_mean, running_var, momentum, eps, acc=torch.float32):
    """Batch statistics of the (bf16-rounded) conv output; returns mean, invstd, scale, shift, new running stats.

    acc=torch.float32 (the pinned default): var = E[y^2] - mean^2 from fp64 raw moments, every result rounded to fp32 where the
    kernel stores one.  acc=torch.float64: the centred form var = mean((y - mean)^2), which does not cancel however far the channel
    mean lies from zero, and every result left in fp64 -- the exact reference of tests/_numeric_ranges.py."""
    C = y_nhwc.shape[-1]
    y = y_nhwc.double().reshape(-1, C)
    n = y.shape[0]
    mean = y.mean(0)
    if _wide(acc):
        var = ((y - mean) ** 2).mean(0)
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = gamma.double() * invstd
        shift = beta.double() - mean * scale
        unbiased = var * (n / (n - 1)) if n > 1 else var
        rm = (1 - momentum) * running_mean.double() + momentum * mean
        rv = (1 - momentum) * running_var.double() + momentum * unbiased
        return mean, invstd, scale, shift, rm, rv
    var = (y * y).mean(0) - mean * mean
    var = var.clamp_min(0)
    invstd = (1.0 / torch.sqrt(var + eps)).float()
    meanf = mean.float()
    scale = gamma.float() * invstd
    shift = beta.float() - meanf * scale
    unbiased = var * (n / (n - 1)) if n > 1 else var
    rm = (1 - momentum) * running_mean.float() + momentum * meanf
    rv = (1 - momentum) * running_var.float() + momentum * unbiased.float()
    return meanf, invstd, scale, shift, rm, rv


def bn_apply(y_nhwc, scale, shift, residual=None, relu=True, acc=torch.float32):
    if _wide(acc):
        out = y_nhwc.to(acc) * scale.to(acc) + shift.to(acc)
        if residual is not None:
            out = out + residual.to(acc)
        return bf16_round(out.clamp_min(0) if relu else out)
    out = torch.addcmul(shift.float(), y_nhwc.float(), scale.float())  # fma(y, scale, shift)
    if residual is not None:
        out = out + residual.float()
    if relu:
        out = out.clamp_min(0)
    return bf16_round(out)


def bn_bwd(dout, act, y, mean, invstd, scale, relu=True, acc=torch.float32):
    """dout, act (post-activation output, or None -> recompute the mask), y: NHWC. Returns dy, dgamma, dbeta, g."""
    C = y.shape[-1]
    if _wide(acc):
        g = dout.to(acc)
        if relu:
            if act is None:
                raise ValueError("oracle needs the activation for the mask")
            g = g * (act > 0)
        xhat = ((y.to(acc) - mean.to(acc)) * invstd.to(acc)).reshape(-1, C)
        g2 = g.reshape(-1, C)
        n = g2.shape[0]
        sg, sgx = g2.sum(0), (g2 * xhat).sum(0)
        dy = scale.to(acc) * (g2 - sg / n - xhat * (sgx / n))
        return bf16_round(dy.reshape(y.shape)), sgx, sg, bf16_round(g)
    g = dout.float()
    if relu:
        if act is not None:
            mask = act.float() > 0
        else:
            raise ValueError("oracle needs the activation for the mask")
        g = g * mask
    xhat = (y.float() - mean.float()) * invstd.float()
    g2 = g.reshape(-1, C)
    xh2 = xhat.reshape(-1, C)
    n = g2.shape[0]
    sg = g2.double().sum(0)
    sgx = (g2.double() * xh2.double()).sum(0)
    c1 = (sg / n).float()
    c2 = (sgx / n).float()
    dy = scale.float() * (g - c1 - xhat * c2)
    return bf16_round(dy), sgx.float(), sg.float(), bf16_round(g)


# ---- pooling ---------------------------------------------------------------------------------------
def maxpool3x3s2_fwd(x_nhwc):
    x = nhwc_to_nchw(x_nhwc.float())
    out, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    return nchw_to_nhwc(out), idx


def maxpool3x3s2_bwd(dout_nhwc, x_nhwc, acc=torch.float32):
    _wide(acc)
    x = nhwc_to_nchw(x_nhwc.detach().to(acc)).requires_grad_(True)
    out = F.max_pool2d(x, 3, 2, 1)
    out.backward(nhwc_to_nchw(dout_nhwc.to(acc)))
    return bf16_round(nchw_to_nhwc(x.grad))


def avgpool_fwd(x_nhwc, acc=torch.float32):
    _wide(acc)
    return bf16_round(x_nhwc.to(acc).mean(dim=(1, 2)))


def avgpool_bwd(dout_nc, hw):
    N, C = dout_nc.shape
    return bf16_round((dout_nc.float() / hw).reshape(N, 1, C).expand(N, hw, C).contiguous())


# ---- input packing + mixup / cutmix (timm.data.Mixup batch mode) ------------------------------------
def pack_input(x_nchw, mode=0, lam=1.0, box=None):
    x = x_nchw.float().clone()
    if mode == 1:
        x = x * lam + x.flip(0) * (1.0 - lam)
    elif mode == 2:
        yl, yh, xl, xh = box
        x[:, :, yl:yh, xl:xh] = x_nchw.float().flip(0)[:, :, yl:yh, xl:xh]
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, 8, device=x.device)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return bf16_round(out)


# ---- loss ------------------------------------------------------------------------------------------
def soft_targets(y1, y2, lam, smoothing, C, dtype=torch.float32):
    off = smoothing / C
    on = 1.0 - smoothing + off
    t1 = torch.full((y1.shape[0], C), off, dtype=dtype).scatter_(1, y1.view(-1, 1), on)
    t2 = torch.full((y2.shape[0], C), off, dtype=dtype).scatter_(1, y2.view(-1, 1), on)
    return t1 * lam + t2 * (1.0 - lam)


def softmax_xent(logits, y1, y2=None, lam=1.0, smoothing=0.0, gscale=1.0, acc=torch.float32):
    """logits [B,C] (bf16-representable). Returns per-row loss, argmax, dlogits (bf16 grid).  acc=torch.float64: the same formula in
    fp64 (loss rows stay fp64) -- under a common logit offset of 1024 the fp32 log_softmax alone is off by 1e-4."""
    _wide(acc)
    x = logits.detach().to(acc).clone().requires_grad_(True)
    B, C = x.shape
    t = soft_targets(y1, y1 if y2 is None else y2, lam, smoothing, C, dtype=acc)
    logp = F.log_softmax(x, dim=-1)
    loss_rows = -(t * logp).sum(-1)
    (loss_rows.sum() * gscale).backward()
    return loss_rows.detach(), x.detach().argmax(-1), bf16_round(x.grad)


# ---- optimizer -------------------------------------------------------------------------------------
def adamw_ema_steps(p0, grads, lrs, wds, betas=(0.9, 0.999), eps=1e-8, ema0=None, ema_decay=0.9995, gscale=1.0):
    """Runs torch.optim.AdamW on a flat parameter for len(grads) steps with per-step lr/wd injection
    (reference: /root/reference/engine.py:33-38) and the ModelEmaV3 lerp after every step."""
    p = torch.nn.Parameter(p0.clone().float())
    opt = torch.optim.AdamW([{"params": [p], "weight_decay": wds[0]}], lr=lrs[0], betas=betas, eps=eps, weight_decay=0.0)
    ema = None if ema0 is None else ema0.clone().float()
    for g, lr, wd in zip(grads, lrs, wds):
        for group in opt.param_groups:
            group["lr"] = lr
            if group["weight_decay"] > 0:
                group["weight_decay"] = wd
        p.grad = (g.float() * gscale).clone()
        opt.step()
        opt.zero_grad()
        if ema is not None:
            ema.lerp_(p.detach(), 1.0 - ema_decay)
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], ema


class LionRef(torch.optim.Optimizer):
    """timm.optim.Lion restated (timm is absent here; algorithm of Chen et al. 2023 as timm implements it and as the
    reference constructs it, /root/reference/optim_factory.py:76-77: betas=(0.9, 0.999), decoupled weight decay):
        p *= 1 - lr*wd ; p -= lr * sign(beta1*m + (1-beta1)*g) ; m = beta2*m + (1-beta2)*g.     Parity unpinned."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p)
                m = st["exp_avg"]
                p.mul_(1.0 - group["lr"] * group["weight_decay"])
                p.add_(torch.sign(m * b1 + p.grad * (1.0 - b1)), alpha=-group["lr"])
                m.lerp_(p.grad, 1.0 - b2)


def optimizer_ema_steps(name, p0, grads, lrs, wds, ema0=None, ema_decay=0.9995, gscale=1.0):
    """The reference's non-default optimizers (optim_factory.py:66-77) for len(grads) steps with the per-step lr / wd
    injection of engine.py:33-38 and the ModelEmaV3 lerp: name in sgd|nesterov|momentum|adam|lion.
    Returns (p, first-moment / momentum buffer, second moment or None, ema)."""
    p = torch.nn.Parameter(p0.clone().float())
    groups = [{"params": [p], "weight_decay": wds[0]}]
    if name in ("sgd", "nesterov"):
        opt = torch.optim.SGD(groups, lr=lrs[0], momentum=0.9, nesterov=True, weight_decay=0.0)
    elif name == "momentum":
        opt = torch.optim.SGD(groups, lr=lrs[0], momentum=0.9, nesterov=False, weight_decay=0.0)
    elif name == "adam":
        opt = torch.optim.Adam(groups, lr=lrs[0], weight_decay=0.0)
    elif name == "lion":
        opt = LionRef(groups, betas=(0.9, 0.999))
    else:
        raise ValueError(name)
    ema = None if ema0 is None else ema0.clone().float()
    for g, lr, wd in zip(grads, lrs, wds):
        for group in opt.param_groups:
            group["lr"] = lr
            if group["weight_decay"] > 0:
                group["weight_decay"] = wd
        p.grad = (g.float() * gscale).clone()
        opt.step()
        opt.zero_grad()
        if ema is not None:
            ema.lerp_(p.detach(), 1.0 - ema_decay)
    st = opt.state[p]
    m = st.get("momentum_buffer", st.get("exp_avg"))
    return p.detach(), m, st.get("exp_avg_sq"), ema


OPT_KINDS = {"adamw": 0, "adam": 1, "momentum": 2, "nesterov": 3, "lion": 4}


def optimizer_step_f64(name, p, g, m, v, lr, wd, t, betas=(0.9, 0.999), eps=1e-8, gscale=1.0):
    """ONE step of torch.optim.AdamW / Adam / SGD (momentum 0.9, dampening 0, Nesterov or not) / LionRef restated on flat
    tensors in fp64 (any device): t is the 1-based number of the step (the Adam bias corrections), m the first moment or
    momentum buffer (zeros in front of step 1), v the second moment (Adam kinds only, else ignored and returned as it
    came).  Returns new (p, m, v); nothing is modified in place.  Pinned against adamw_ema_steps / optimizer_ema_steps
    (torch.optim itself) in tests/test_oracle_cpu.py."""
    p, g, m = p.double(), g.double() * gscale, m.double()
    b1, b2 = betas
    if name in ("adamw", "adam"):
        v = v.double()
        if name == "adamw":
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
        return p - (lr / (1.0 - b1 ** t)) * (m / denom), m, v
    if name in ("momentum", "nesterov"):
        g = g + wd * p
        m = b1 * m + g
        return p - lr * (g + b1 * m if name == "nesterov" else m), m, v
    if name == "lion":
        p = p * (1.0 - lr * wd) - lr * torch.sign(m * b1 + g * (1.0 - b1))
        return p, m + (g - m) * (1.0 - b2), v
    raise ValueError(name)


def ema_step_f64(ema, p, ema_decay):
    """ModelEmaV3.update: ema.lerp_(p, 1 - decay), in fp64."""
    return ema.double() + (p.double() - ema.double()) * (1.0 - ema_decay)


def grad_norm(g, max_norm=0.0):
    norm = torch.linalg.vector_norm(g.double()).float()
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, max_norm / (float(norm) + 1e-6))
    return float(norm), coef


# ---- comparison helpers ----------------------------------------------------------------------------
def rel_l2(a, b):
    a = a.double().flatten()
    b = b.double().flatten()
    d = torch.linalg.vector_norm(a - b)
    n = torch.linalg.vector_norm(b)
    return float(d / n) if n > 0 else float(d)


def max_bf16_ulp(a, b):
    """Largest |a-b| in units of the bf16 spacing at |b| (both already on the bf16 grid)."""
    a = a.float().flatten()
    b = b.float().flatten()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return float(((a - b).abs() / ulp).max())


def bf16_close(a, b, ulps=2.0, atol_rms=2e-3, max_frac=0.0):
    """Elementwise: |a-b| <= ulps * bf16 spacing at |b| + atol_rms * rms(b).
    The absolute term covers outputs that are small differences of O(rms) terms (cancellation), where a
    different fp32 summation order legitimately moves the result by many ulps OF THE RESULT.
    max_frac: share of the elements that may sit outside the bound (tests over millions of elements whose operands pass
    through a bf16 rounding: a handful land one rounding step further out)."""
    a = a.float().flatten()
    b = b.float().flatten()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    rms = float(torch.sqrt((b.double() ** 2).mean()))
    # "not within the bound" (rather than "beyond it"): a NaN / Inf in either tensor compares False and counts as bad
    # (an Inf makes its own bound infinite, hence the explicit finiteness term)
    bad = ~((a - b).abs() <= ulps * ulp + atol_rms * rms) | ~torch.isfinite(a) | ~torch.isfinite(b)
    if max_frac <= 0.0:
        return not bool(bad.any())
    return bool(float(bad.float().mean()) <= max_frac)


# ---- token ops: LayerNorm / GELU / attention (ViT, ConvNeXt) ---------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, acc=torch.float32):
    """x [rows, C] bf16-representable. Returns y (bf16 grid), mean, rstd."""
    _wide(acc)
    xf = x.to(acc)
    mean = xf.mean(-1)
    var = ((xf - mean[:, None]) ** 2).mean(-1)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean[:, None]) * rstd[:, None] * gamma.to(acc) + beta.to(acc)
    return bf16_round(y), mean, rstd


def layernorm_bwd(dy, x, gamma, eps, acc=torch.float32):
    """Gradients through torch's own layer_norm (fp32): dx (bf16 grid), dgamma, dbeta."""
    _wide(acc)
    xf = x.detach().to(acc).requires_grad_(True)
    g = gamma.detach().to(acc).clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    y = F.layer_norm(xf, (x.shape[-1],), g, b, eps)
    y.backward(dy.to(acc))
    return bf16_round(xf.grad), g.grad, b.grad


def gelu_fwd(z, acc=torch.float32):
    _wide(acc)
    return bf16_round(F.gelu(z.to(acc)))


def gelu_bwd(da, z, acc=torch.float32):
    _wide(acc)
    zf = z.detach().to(acc).requires_grad_(True)
    F.gelu(zf).backward(da.to(acc))
    return bf16_round(zf.grad)


def attention_fwd(qkv, B, T, H, D, scale, acc=torch.float32):
    """qkv [B*T, 3*H*D] (timm layout: reshape(B, T, 3, H, D)). Returns out [B*T, H*D] (bf16 grid), lse [B,H,T]."""
    _wide(acc)
    q, k, v = qkv.to(acc).reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    o = p @ v
    return bf16_round(o.permute(0, 2, 1, 3).reshape(B * T, H * D)), lse


def attention_bwd(qkv, dout, B, T, H, D, scale, acc=torch.float32):
    _wide(acc)
    x = qkv.detach().to(acc).requires_grad_(True)
    q, k, v = x.reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    o = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
    o.permute(0, 2, 1, 3).reshape(B * T, H * D).backward(dout.to(acc))
    return bf16_round(x.grad)


def _bf16_grid(t):
    """fp64 values rounded to the bf16 grid and kept in fp64 (fp64 -> fp32 -> bf16 double-rounds only on an fp32 tie: 2^-30 of values)."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def attention_written_out(qkv, dout, B, T, H, D, scale, rounding_points=False):
    """Forward and backward of softmax attention written out product by product in fp64 (no autograd).

    rounding_points=False: exact arithmetic; out and dqkv equal attention_fwd / attention_bwd with acc=torch.float64.
    rounding_points=True: the operands the HIP kernels round to bf16 on their way into an MFMA are rounded here too, everything
    else stays fp64 -- the unnormalised exp(s - max) in front of P V (the row sum is taken unrounded), p in front of dV = P^T dO,
    dS = p (dP - delta) in front of dQ = dS K and dK = dS^T Q, and delta = rowsum(dO * out) of the ROUNDED out the forward stored.
    The distance between the two is what those roundings alone cost, whatever the kernels do.

    Returns a dict: out [B*T, H*D] and dqkv [B*T, 3*H*D] on the bf16 grid (fp32), the same two before that last rounding (out64,
    dqkv64), lse, delta [B, H, T] and ds [B, H, T, T] (the unrounded dS, without the softmax scale) in fp64."""
    rnd = _bf16_grid if rounding_points else (lambda t: t)
    q, k, v = qkv.to(torch.float64).reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    do = dout.to(torch.float64).reshape(B, T, H, D).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    o = (rnd(e) @ v) / l
    p = torch.exp(s - lse[..., None])
    delta = (do * rnd(o)).sum(-1)
    ds = p * (do @ v.transpose(-1, -2) - delta[..., None])
    dv = rnd(p).transpose(-1, -2) @ do
    dq = (rnd(ds) @ k) * scale
    dk = (rnd(ds).transpose(-1, -2) @ q) * scale
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * D)
    o = o.permute(0, 2, 1, 3).reshape(B * T, H * D)
    return {"out": bf16_round(o), "out64": o, "lse": lse, "delta": delta, "ds": ds, "dqkv": bf16_round(dqkv), "dqkv64": dqkv}


# ---- ConvNeXt pieces ------------------------------------------------------------------------------------------------
def dwconv7_fwd(x_nhwc, w_c77, bias, acc=torch.float32):
    """x [N,H,W,C], w [C,7,7] (torch depthwise layout), bias [C]. Returns y NHWC on the bf16 grid."""
    C = x_nhwc.shape[-1]
    if _wide(acc):     # one multiply-add pass per tap
        xp = F.pad(x_nhwc.to(acc), (0, 0, 3, 3, 3, 3))
        N, H, W, _ = x_nhwc.shape
        w = w_c77.to(acc)
        y = bias.to(acc).expand(N, H, W, C).clone()
        for r, s, xs in _taps(xp, 7, 7, 1, H, W):
            y += xs * w[:, r, s]
        return bf16_round(y)
    y = F.conv2d(nhwc_to_nchw(x_nhwc.float()), w_c77.float().reshape(C, 1, 7, 7), bias.float(), padding=3, groups=C)
    return bf16_round(nchw_to_nhwc(y))


def dwconv7_bwd(x_nhwc, w_c77, dy_nhwc, addend=None, acc=torch.float32):
    C = x_nhwc.shape[-1]
    if _wide(acc):     # one pass per tap: dx scatters dy through the tap, dw[:, r, s] reduces x * dy
        N, H, W, _ = x_nhwc.shape
        xp = F.pad(x_nhwc.to(acc), (0, 0, 3, 3, 3, 3))
        dyw = dy_nhwc.to(acc)
        w = w_c77.to(acc)
        dxp = torch.zeros_like(xp)
        dw = torch.empty(C, 7, 7, dtype=acc, device=x_nhwc.device)
        for (r, s, xs), (_, _, dxs) in zip(_taps(xp, 7, 7, 1, H, W), _taps(dxp, 7, 7, 1, H, W)):
            dxs += dyw * w[:, r, s]
            dw[:, r, s] = (xs * dyw).reshape(-1, C).sum(0)
        dx = dxp[:, 3:3 + H, 3:3 + W, :]
        if addend is not None:
            dx = dx + addend.to(acc)
        return bf16_round(dx), dw
    x = nhwc_to_nchw(x_nhwc.float()).requires_grad_(True)
    w = w_c77.float().reshape(C, 1, 7, 7).clone().requires_grad_(True)
    F.conv2d(x, w, None, padding=3, groups=C).backward(nhwc_to_nchw(dy_nhwc.float()))
    dx = nchw_to_nhwc(x.grad)
    if addend is not None:
        dx = dx + addend.float()
    return bf16_round(dx), w.grad.reshape(C, 7, 7)


def layerscale_fwd(z, inp, gamma, keep):
    k = 1.0 if keep is None else keep.float().reshape(-1, *([1] * (z.dim() - 1)))
    return bf16_round(inp.float() + k * gamma.float() * z.float())


def layerscale_bwd(dout, z, gamma, keep):
    k = 1.0 if keep is None else keep.float().reshape(-1, *([1] * (z.dim() - 1)))
    d = dout.float() * k
    return bf16_round(d * gamma.float()), (d * z.float()).reshape(-1, z.shape[-1]).double().sum(0).float()


# ---- MobileNet pieces (csrc/dwconv3x3.hip): BatchNorm + ReLU6 with the kernel's single rounding, depthwise 3x3 -------------------
def fma32(x, scale, shift):
    """fp32 fma(x, scale[c], shift[c]): the product of a bf16 and an fp32 value is exact in fp64 and the sum is rounded there to 53
    bits before the rounding to 24, which differs from the single rounding of an fma only on a 2^-29 share of the inputs"""
    return (x.double() * scale.double() + shift.double()).float()


def bn_relu6(x, scale, shift):
    """bf16(min(max(fma(x, scale, shift), 0), 6)): what icamd_bn_apply_relu6 stores and the on-load kernels form in registers"""
    return bf16_round(fma32(x, scale, shift).clamp(0.0, 6.0))


def dwconv_ref(a_nhwc, w_ckk, dy_nhwc, stride, k):
    """F.conv2d(groups=C, padding=k // 2) in fp64 on the (activated, rounded) input and autograd: y and dx on the bf16 grid, dw [C,k,k]"""
    C = a_nhwc.shape[-1]
    a = nhwc_to_nchw(a_nhwc.double()).requires_grad_(True)
    w = w_ckk.double().reshape(C, 1, k, k).clone().requires_grad_(True)
    y = F.conv2d(a, w, None, stride, k // 2, 1, C)
    y.backward(nhwc_to_nchw(dy_nhwc.double()))
    return bf16_round(nchw_to_nhwc(y.detach())), bf16_round(nchw_to_nhwc(a.grad)), w.grad.reshape(C, k, k)


def dwconv3_ref(a_nhwc, w_c33, dy_nhwc, stride):
    return dwconv_ref(a_nhwc, w_c33, dy_nhwc, stride, 3)


def dwconv5_ref(x_nhwc, w_c55, dy_nhwc, stride):
    return dwconv_ref(x_nhwc, w_c55, dy_nhwc, stride, 5)


# ---- EfficientNet pieces (csrc/dwconv5x5.hip): BatchNorm + SiLU and the MBConv squeeze-and-excitation, in fp64 -------------------
def silu64(z):
    z = z.double()
    return z * torch.sigmoid(z)


def silu_grad64(z):
    sg = torch.sigmoid(z.double())
    return sg * (1.0 + z.double() * (1.0 - sg))


def bn_silu(y, scale, shift):
    """a = bf16(silu(fma32(y, scale, shift))), the silu in fp64 on the kernel's fp32 z: what icamd_bn_apply_silu stores"""
    return bf16_round(silu64(fma32(y, scale, shift)).float())


def boundary_share(y, scale, shift):
    """share of the elements whose fp64 silu(z) sits within 2^-13 (relative: 8 fp32 ulps) of the midpoint between two bf16 values: where
    a kernel whose fp32 silu is a few ulps off may round the other way"""
    v = silu64(fma32(y, scale, shift))
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
    z = fma32(y, scale, shift).double() if fp32_z else y.double() * scale.double() + shift.double()
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
