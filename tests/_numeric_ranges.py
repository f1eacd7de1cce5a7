"""Operands that move the normalisation, loss, GELU / GRN, pooling and step kernels out of the band `randn` inputs keep them in, their
fp64 references, and the bounds the GPU tests hold the kernels to (tests/test_numeric_ranges_gpu.py; tests/test_numeric_ranges_cpu.py
keeps this file honest).  torch on the CPU only, fixed seeds; every bf16 operand is on the bf16 grid.

  BatchNorm    a per-channel offset carried THROUGH THE OPERANDS of the producing convolution, so that the convolution stays the randn
               problem: input channel ONE is the constant 1 and the filter's centre tap for it is c_k for output channel k (every
               other tap of that channel is zero; the centre tap always sees a real pixel).  c_k cycles inside each 8-channel vector
               through OFFSET_CYCLE x s, s = the unshifted output's standard deviation rounded to a power of two.
  LayerNorm    the rows of one wave's row group cycle through LN_KINDS
  cross-entropy  the rows of a batch cycle through XENT_KINDS
  GRN          per-channel magnitudes 2^e, a zero channel, a zero sample, a channel deep in GELU's lower tail
  step kernels gradients of element magnitude 2^e, parameters of magnitude 2^+-20

Bounds.  The tolerances of the sibling tests carry over unchanged.  Only the BatchNorm quantities that hang on the variance, which
the library forms from raw moments (fp32 sum and sum of squares per partial row, fp64 across rows, var = E[y^2] - mean^2), are held
to max(existing tolerance, 2 x e_round) in the offset channels: e_round is the error of bn_points() -- the same algorithm restated
with fp32 SEQUENTIAL sums inside a partial row, independent of any kernel -- against the exact centred fp64 reference; the factor 2
is for the order inside a partial row, which is the kernel's own (two fp32 orders of one n-term sum differ by a comparable amount).
The yardstick is always the exact reference, never the kernel."""
import math

import torch

from _harness import rnd_bf16
from oracle import ops_ref as R

F64 = torch.float64


def on_bf16_grid(t):
    return bool(torch.equal(R.bf16_round(t.float()), t.float()))


def bf16_ulp(x):
    """spacing of the bf16 grid at |x| (fp64 tensor)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def excess(got, ref, rtol, atol):
    """largest |got - ref| / (atol + rtol |ref|): <= 1 is torch.allclose(got, ref, rtol, atol); a non-finite value gives inf"""
    got, ref = got.double(), ref.double()
    if got.numel() == 0:
        return 0.0
    e = (got - ref).abs() / (atol + rtol * ref.abs())
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    return float(e.max())


def bad_share(a, b, ulps=2.0, atol_rms=2e-3):
    """share of the elements outside R.bf16_close's bound (0.0 is R.bf16_close(a, b))"""
    a, b = a.float().flatten(), b.float().flatten()
    if a.numel() == 0:
        return 0.0
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    rms = float(torch.sqrt((b.double() ** 2).mean()))
    bad = ~((a - b).abs() <= ulps * ulp + atol_rms * rms) | ~torch.isfinite(a) | ~torch.isfinite(b)
    return float(bad.float().mean())


# ======================================================================================================== BatchNorm
ONE = 1                                                   # the input channel that is the constant 1
OFFSET_CYCLE = (0.0, 4.0, -4.0, 16.0, -16.0, 64.0, -64.0, 0.0)
OFFSET_CLASSES = (0, 4, 16, 64)                           # |c_k| / s
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
MAX_FRAC = 1e-3                                           # the largest share R.bf16_close(max_frac=) may be given

# name -> (N, H, W, Cin, Cout, k, stride, pad, groups).  One case per statistics producer; the GPU test asserts the route.
BN_PRODUCERS = {
    "igemm": (2, 9, 7, 64, 128, 3, 1, 1, 1),
    "igemm_c2048": (2, 5, 5, 64, 2048, 1, 1, 0, 1),       # the finalize kernel's 64-channel groups (CG = 32 below 2048 channels)
    "pw_resident": (3, 12, 12, 64, 256, 1, 1, 0, 1),
    "gemm_nt": (2, 9, 9, 64, 264, 1, 1, 0, 1),            # a forced small-K case of test_pointwise_large_tile_gemm_forced_small_k
    "halo": (1, 3, 3, 64, 64, 3, 1, 1, 1),                # the smallest HALO_CASES entry
    "gconv": (1, 5, 5, 64, 64, 3, 1, 1, 16),              # the smallest case of tests/test_gconv_gpu.py
    "thin": (2, 8, 8, 32, 32, 3, 1, 1, 1),
    "stem7x7": (2, 16, 16, 3, 64, 7, 2, 3, 1),
    "fused_1x1": (3, 75, 75, 256, 64, 1, 1, 0, 1),        # icamd_bn_apply_conv1x1_fused
}
BN_SPECIAL = {
    "const_channel": (2, 9, 7, 64, 128, 3, 1, 1, 1),      # channel CONST_CH: filter row zero but c_k, so var = 0 exactly
    "count_1": (1, 1, 1, 64, 64, 1, 1, 0, 1),
}
CONST_CH = 13                                             # 13 % 8 = 5: c_k = +64 s


def offset_classes(Cout):
    """class (|c_k| / s) -> channel indices"""
    cyc = torch.tensor([abs(OFFSET_CYCLE[k % 8]) for k in range(Cout)])
    return {c: torch.nonzero(cyc == c).flatten() for c in OFFSET_CLASSES}


def _grouped_conv_ref(x, w, stride, pad, groups):
    """fp64 convolution of NHWC x with w [Cout][KH][KW][Cin / groups], rounded to the bf16 grid once"""
    if groups == 1:
        return R.conv2d_fwd(x, w, stride, pad, acc=F64)
    cg_in, cg_out = x.shape[-1] // groups, w.shape[0] // groups
    return torch.cat([R.conv2d_fwd(x[..., g * cg_in:(g + 1) * cg_in].contiguous(), w[g * cg_out:(g + 1) * cg_out].contiguous(),
                                   stride, pad, acc=F64) for g in range(groups)], -1)


_BN_OPS = {}


def bn_operands(name):
    """dict(x [N,H,W,Cin], w [Cout,KH,KW,Cin/groups], s, c [Cout], gamma, beta, rm0, rv0, dout, y_ref): fp32 tensors on the bf16
    grid where the kernels take bf16.  y_ref is the fp64 convolution rounded once: what a producer stores up to rounding flips."""
    if name in _BN_OPS:
        return _BN_OPS[name]
    N, H, W, Cin, Cout, k, stride, pad, groups = {**BN_PRODUCERS, **BN_SPECIAL}[name]
    cg = Cin // groups
    x = rnd_bf16(N, H, W, Cin, seed=301)
    w = rnd_bf16(Cout, k, k, cg, scale=(1.0 / (k * k * cg)) ** 0.5, seed=302)
    one = torch.arange(groups) * cg + (ONE % cg)          # the constant channel of every group
    if name == "fused_1x1":                               # this producer's input is a ReLU output
        x = x.clamp_min(0)
    x[..., one] = 1.0
    w[..., ONE % cg] = 0.0
    plain = _grouped_conv_ref(x, w, stride, pad, groups)
    std = float(plain.double().std()) if plain.numel() > Cout else 1.0
    s = 2.0 ** round(math.log2(std))
    c = torch.tensor([OFFSET_CYCLE[i % 8] for i in range(Cout)]) * s
    if name == "const_channel":
        w[CONST_CH] = 0.0
    w[:, k // 2, k // 2, ONE % cg] = c
    g = torch.Generator().manual_seed(303)
    ops = {"x": x, "w": w, "s": s, "c": c, "stride": stride, "pad": pad, "groups": groups,
           "gamma": torch.rand(Cout, generator=g) + 0.5, "beta": torch.randn(Cout, generator=g) * 0.1,
           "rm0": torch.randn(Cout, generator=g) * 0.1, "rv0": torch.rand(Cout, generator=g) + 0.5}
    ops["y_ref"] = _grouped_conv_ref(x, w, stride, pad, groups)
    ops["dout"] = rnd_bf16(*ops["y_ref"].shape, seed=304)
    _BN_OPS[name] = ops
    return ops


def mean_over_std(y):
    """|mean| / std per channel of y [..., C], measured in fp64 (inf for a constant non-zero channel)"""
    y2 = y.double().reshape(-1, y.shape[-1])
    m, sd = y2.mean(0), y2.std(0, unbiased=False)
    return torch.where(sd > 0, m.abs() / sd.clamp_min(1e-300), torch.where(m == 0, torch.zeros_like(m), torch.full_like(m, float("inf"))))


def bn_exact(y, ops, act=None):
    """Everything BatchNorm computes from the stored y [N,H,W,C] (bf16 grid), in fp64 with the centred variance.  act: the
    activation whose sign is the ReLU mask of the backward (default: this reference's own)."""
    mean, invstd, scale, shift, rm, rv = R.bn_train_coeffs(y, ops["gamma"], ops["beta"], ops["rm0"], ops["rv0"], BN_MOMENTUM, BN_EPS,
                                                           acc=F64)
    out = R.bn_apply(y, scale, shift, None, relu=True, acc=F64)
    dy, dgamma, dbeta, _ = R.bn_bwd(ops["dout"], out if act is None else act, y, mean, invstd, scale, relu=True, acc=F64)
    return {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "rm": rm, "rv": rv, "out": out, "dy": dy,
            "dgamma": dgamma, "dbeta": dbeta}


def fp32_partial_sums(t, rows):
    """[rows][C] fp32: t [M, C] (fp32 values) summed over `rows` partial rows of ceil(M / rows) consecutive values each, one value
    after the other in fp32"""
    M, C = t.shape
    chunk = -(-M // rows)
    tp = torch.zeros(rows * chunk, C)
    tp[:M] = t.float()
    tp = tp.reshape(rows, chunk, C)
    acc = torch.zeros(rows, C)
    for i in range(chunk):
        acc = acc + tp[:, i]
    return acc


def raw_moment_sums(y, rows):
    """[rows][2][C] fp32: sum and sum of squares of y [M, C] per partial row (the square of a bf16 value is exact in fp32)"""
    y = y.float()
    return torch.stack([fp32_partial_sums(y, rows), fp32_partial_sums(y * y, rows)], 1)


def bn_points(y, ops, rows, act=None):
    """The library's algorithm with its rounding points, restated independently of every kernel: fp32 raw moments over `rows` partial
    rows (raw_moment_sums), folded in fp64, var = E[y^2] - mean^2 clamped at zero, invstd and mean rounded to fp32, scale and shift
    formed in fp32, the apply as one fp32 fma; the backward in fp64 from those coefficients."""
    C = y.shape[-1]
    part = raw_moment_sums(y.reshape(-1, C), rows).double().sum(0)
    n = y.numel() // C
    mean = part[0] / n
    var = (part[1] / n - mean * mean).clamp_min(0)
    invstd = (1.0 / torch.sqrt(var + BN_EPS)).float()
    meanf = mean.float()
    scale = ops["gamma"].float() * invstd
    shift = ops["beta"].float() - meanf * scale
    unbiased = var * (n / (n - 1)) if n > 1 else var
    rm = (1 - BN_MOMENTUM) * ops["rm0"].float() + BN_MOMENTUM * meanf
    rv = (1 - BN_MOMENTUM) * ops["rv0"].float() + BN_MOMENTUM * unbiased.float()
    out = R.bn_apply(y, scale, shift, None, relu=True)
    dy, dgamma, dbeta, _ = R.bn_bwd(ops["dout"], out if act is None else act, y, meanf, invstd, scale, relu=True, acc=F64)
    return {"mean": meanf, "invstd": invstd, "scale": scale, "shift": shift, "rm": rm, "rv": rv, "out": out, "dy": dy,
            "dgamma": dgamma, "dbeta": dbeta}


# quantity -> (rtol, atol) of torch.allclose in test_bn_train_apply_and_bwd (atol 1e-8 is torch's default there)
BN_ALLCLOSE = {"mean": (1e-5, 1e-6), "invstd": (1e-5, 1e-8), "scale": (1e-5, 1e-8), "shift": (1e-4, 1e-6), "rm": (1e-5, 1e-7),
               "rv": (1e-5, 1e-8)}
BN_REL_L2 = {"out": 1e-3, "dy": 1e-3, "dgamma": 1e-4, "dbeta": 1e-4}
BN_VARIANCE_BOUND = ("invstd", "scale", "shift", "rv", "out", "dy", "dgamma", "out_share", "dy_share")


def bn_errors(got, exact, Cout):
    """{(quantity, class): error} of `got` (a dict like bn_exact's; keys may be missing) against the exact reference, per offset
    class: the per-channel quantities as excess() over their allclose tolerance, the tensors as rel-L2 over the class's channels,
    and "<tensor>_share" as bad_share()"""
    e = {}
    for cls, idx in offset_classes(Cout).items():
        if idx.numel() == 0:
            continue
        for q, (rtol, atol) in BN_ALLCLOSE.items():
            if q in got:
                e[(q, cls)] = excess(got[q][idx], exact[q][idx], rtol, atol)
        for q in BN_REL_L2:
            if q in got:
                a, b = got[q][..., idx], exact[q][..., idx]
                e[(q, cls)] = R.rel_l2(a, b) if bool(torch.isfinite(a.double()).all()) else float("inf")
                if q in ("out", "dy"):
                    e[(q + "_share", cls)] = bad_share(a, b)
    return e


def bn_caps(e_round):
    """the bound of every entry of bn_errors(): the existing one (1 for an excess, the rel-L2 bound, share 0); for what hangs on the
    raw-moment variance, in the offset classes, max(that, 2 x e_round), a share never above MAX_FRAC"""
    caps = {}
    for (q, cls), er in e_round.items():
        base = 1.0 if q in BN_ALLCLOSE else 0.0 if q.endswith("_share") else BN_REL_L2[q]
        cap = max(base, 2.0 * er) if (cls != 0 and q in BN_VARIANCE_BOUND) else base
        caps[(q, cls)] = min(cap, MAX_FRAC) if q.endswith("_share") else cap
    return caps


def bn_invstd_rel_err(got_invstd, exact, Cout):
    """class -> largest relative error of invstd (the figure of the DESIGN.md table)"""
    r = ((got_invstd.double() - exact["invstd"]) / exact["invstd"]).abs()
    return {cls: float(r[idx].max()) for cls, idx in offset_classes(Cout).items() if idx.numel()}


# ---- the second raw-product form: icamd_bn_bwd_from_gy_partials turns sum g y into sum g xhat = invstd (sum g y - mean sum g) ----------
GY_CASE = (4, 48, 48, 256, 64)                            # N, H, W, Cin (the BatchNorm's channels), Cout: the smallest routed shape


def gy_operands():
    """the operands of test_conv_dgrad_bnred with the BatchNorm input y = randn + c_k (s = 1), on the bf16 grid"""
    N, H, W, Cin, Cout = GY_CASE
    gen = torch.Generator().manual_seed(391)
    c = torch.tensor([OFFSET_CYCLE[k % 8] for k in range(Cin)])
    return {"dy": rnd_bf16(N, H, W, Cout, seed=392), "w": rnd_bf16(Cout, 1, 1, Cin, scale=(1.0 / Cout) ** 0.5, seed=393),
            "addend": rnd_bf16(N, H, W, Cin, seed=394), "y": R.bf16_round(rnd_bf16(N, H, W, Cin, seed=395) + c), "c": c,
            "amask": torch.rand(N, H, W, Cin, generator=gen) > 0.4, "pmask": torch.rand(N, H, W, Cin, generator=gen) > 0.45,
            "gamma": 0.5 + torch.rand(Cin, generator=gen)}


def gy_exact(g, y, gamma):
    """fp64: mean, invstd (centred), scale, and the BatchNorm backward of the stored g without a ReLU: dy, dgamma, dbeta"""
    C = y.shape[-1]
    yy = y.double().reshape(-1, C)
    mean = yy.mean(0)
    invstd = 1.0 / torch.sqrt(((yy - mean) ** 2).mean(0) + BN_EPS)
    scale = gamma.double() * invstd
    dy, dgamma, dbeta, _ = R.bn_bwd(g, None, y, mean, invstd, scale, relu=False, acc=F64)
    return {"mean": mean, "invstd": invstd, "scale": scale, "dy": dy, "dgamma": dgamma, "dbeta": dbeta}


def gy_points(g, y, exact, rows):
    """the algorithm's rounding points: fp32 sums of g and of g y (exact products of two bf16 values) per partial row, fp64 across
    rows, sum g xhat = invstd (sum g y - mean sum g) with the fp32 mean and invstd the kernel is given; dy in fp64 from those"""
    C = y.shape[-1]
    g2, y2 = g.float().reshape(-1, C), y.float().reshape(-1, C)
    n = g2.shape[0]
    t1 = fp32_partial_sums(g2, rows).double().sum(0)
    t2 = fp32_partial_sums(g2 * y2, rows).double().sum(0)
    mean, invstd = exact["mean"].float().double(), exact["invstd"].float().double()
    sgx = invstd * (t2 - mean * t1)
    xhat = (y2.double() - mean) * invstd
    dy = exact["scale"].float().double() * (g2.double() - t1 / n - xhat * (sgx / n))
    return {"dy": R.bf16_round(dy.reshape(y.shape)), "dgamma": sgx, "dbeta": t1}


def gy_errors(got, exact, C):
    e = {}
    for cls, idx in offset_classes(C).items():
        for q in ("dy", "dgamma", "dbeta"):
            e[(q, cls)] = R.rel_l2(got[q][..., idx], exact[q][..., idx]) if bool(torch.isfinite(got[q].double()).all()) else float("inf")
        e[("dy_share", cls)] = bad_share(got["dy"][..., idx], exact["dy"][..., idx])
    return e


def gy_caps(e_round):
    """existing bounds (dy 1e-3 and bf16_close, dgamma and dbeta 1e-4); dgamma, which is the cancelling form, and what follows from
    it in dy: max(that, 2 x e_round) in the offset classes"""
    caps = {}
    for (q, cls), er in e_round.items():
        base = 0.0 if q.endswith("_share") else BN_REL_L2[q]
        cap = max(base, 2.0 * er) if (cls != 0 and q != "dbeta") else base
        caps[(q, cls)] = min(cap, MAX_FRAC) if q.endswith("_share") else cap
    return caps


# ======================================================================================================== LayerNorm
LN_SHAPES = ((33, 96), (33, 384), (21, 768), (5, 1024))
LN_EPS = (1e-6, 1e-5)
LN_KINDS = ("randn", "plus64", "minus64", "plus300", "const0", "const1", "const_minus64", "times2^20", "times2^-12")
LN_CONST = {"const0": 0.0, "const1": 1.0, "const_minus64": -64.0}
# (dy scale, addend) of the backward runs
LN_BWD_VARIANTS = ((1.0, False), (2.0 ** 10, False), (2.0 ** -20, False), (1.0, True))
PATCH_MERGE_SHAPE = (2, 4, 4, 96)                         # the smallest case of tests/test_patch_merge_gpu.py: 8 rows of 384


def ln_kind_of_row(rows):
    """a 5-row matrix could not hold 9 kinds: it takes the kinds the other shapes' first rows do not reach first"""
    if rows >= len(LN_KINDS):
        return [LN_KINDS[r % len(LN_KINDS)] for r in range(rows)]
    return [LN_KINDS[(r + 4) % len(LN_KINDS)] for r in range(rows)]


def ln_operands(rows, C, seed=311):
    """x [rows, C] on the bf16 grid with the row kinds of ln_kind_of_row, gamma, beta, dy, addend"""
    x = rnd_bf16(rows, C, seed=seed)
    kinds = ln_kind_of_row(rows)
    for r, kind in enumerate(kinds):
        if kind == "plus64":
            x[r] += 64.0
        elif kind == "minus64":
            x[r] -= 64.0
        elif kind == "plus300":
            x[r] += 300.0
        elif kind in LN_CONST:
            x[r] = LN_CONST[kind]
        elif kind == "times2^20":
            x[r] *= 2.0 ** 20
        elif kind == "times2^-12":
            x[r] *= 2.0 ** -12
    x = R.bf16_round(x)
    g = torch.Generator().manual_seed(seed + 1)
    return {"x": x, "kinds": kinds, "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.2,
            "dy": rnd_bf16(rows, C, seed=seed + 2), "addend": rnd_bf16(rows, C, seed=seed + 3)}


def ln_rows_of(kinds, wanted):
    return torch.tensor([r for r, k in enumerate(kinds) if k in wanted], dtype=torch.long)


def ln_mean_atol(x, kinds):
    """[rows]: the absolute part of the bound on the row mean.  1e-6 (test_layernorm_fwd_bwd) for the randn rows; elsewhere at least
    that and 2^-19 mean|x|: a lane adds at most 24 values one after the other and the lanes fold in at most 6 more steps, each
    rounding step is off by at most 2^-24 of a partial sum <= sum|x|, hence <= 30 x 2^-24 < 2^-19 of mean|x|."""
    a = torch.maximum(torch.full((x.shape[0],), 1e-6, dtype=F64), 2.0 ** -19 * x.double().abs().mean(-1))
    a[ln_rows_of(kinds, ("randn",))] = 1e-6
    return a


def ln_const_bound(c, gamma, beta, eps):
    """[C]: what |y - beta| may reach in a constant row c.  Exactly y = beta.  The kernels form mean = sum * (1 / C) with a rounded
    reciprocal, so x - mean is off by at most |c| 2^-23 (the reciprocal and the product round once each), rstd <= 1 / sqrt(eps)
    multiplies that, and the stored value is rounded once more: one bf16 ulp at that size."""
    r = abs(c) * 2.0 ** -23 * gamma.double().abs() / math.sqrt(eps)
    return r + bf16_ulp(beta.double().abs() + r)


def ln_fp32_restatement(x, gamma, beta, eps):
    """the three lines of the forward kernels in fp32 (mean = sum * fl(1 / C); centred second pass; one fma-free product chain)"""
    C = x.shape[-1]
    inv_c = (torch.tensor(1.0) / torch.tensor(float(C))).float()
    xf = x.float()
    mean = xf.sum(-1) * inv_c
    d = xf - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(-1) * inv_c + eps)
    return R.bf16_round(d * rstd[:, None] * gamma.float() + beta.float()), mean, rstd


def patch_merge_scatter(merged, N, H, W, C):
    """x [N,H,W,C] whose 2x2 gather in timm's x0 | x1 | x2 | x3 order ((0,0), (1,0), (0,1), (1,1)) is merged [N*(H/2)*(W/2), 4C]"""
    m = merged.reshape(N, H // 2, W // 2, 4, C)
    x = torch.empty(N, H, W, C)
    for blk, (a, b) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        x[:, a::2, b::2] = m[:, :, :, blk]
    return x


# ======================================================================================================== cross-entropy
XENT_SHAPES = ((8, 1000, 1024), (5, 10, 16), (4, 130, 136))      # B, C, ld
XENT_KINDS = ("randn", "plus64", "minus64", "plus1024", "minus1024", "peak_target", "peak_other", "equal", "tie0", "tie1", "tie2")
XENT_OFFSET = {"plus64": 64.0, "minus64": -64.0, "plus1024": 1024.0, "minus1024": -1024.0}
XENT_GSCALES = ("1/B", 2.0 ** 10, 2.0 ** -20)
TIE_PAIRS = ((5, 70), (63, 64), ("C-1", 0))


def tie_pair(kind, C):
    """the two columns of an exact two-way tie at the maximum; pairs that do not fit C fall back to (C - 1, 0)"""
    a, b = TIE_PAIRS[int(kind[-1])]
    a = C - 1 if a == "C-1" else a
    return (a, b) if max(a, b) < C else (C - 1, 0)


def xent_batches(B):
    """starts of the batches that together show every kind: row i of the batch started at s is of kind (s + i) % 11"""
    return list(range(0, len(XENT_KINDS), B))


def xent_operands(B, C, start, seed=321):
    """logits [B, C] on the bf16 grid, y1, y2 (targets), kinds"""
    g = torch.Generator().manual_seed(seed + start)
    x = R.bf16_round(torch.randn(B, C, generator=g) * 3.0)
    y1 = torch.randint(0, C, (B,), generator=g)
    y2 = y1.flip(0).clone()
    kinds = [XENT_KINDS[(start + i) % len(XENT_KINDS)] for i in range(B)]
    for i, kind in enumerate(kinds):
        if kind in XENT_OFFSET:
            x[i] = R.bf16_round(x[i] + XENT_OFFSET[kind])
        elif kind == "peak_target":
            x[i, y1[i]] = x[i, y1[i]] + 200.0
        elif kind == "peak_other":
            x[i, (int(y1[i]) + 1) % C] += 200.0
        elif kind == "equal":
            x[i] = 2.5
        elif kind.startswith("tie"):
            a, b = tie_pair(kind, C)
            top = float(x[i].max()) + 1.0
            x[i, a] = top
            x[i, b] = top
    return R.bf16_round(x), y1, y2, kinds


def xent_fp32_restatement(x, y1, y2, lam, smoothing):
    """the loss lines of softmax_xent_kernel in fp32: lse = max + log(sum exp(x - max)); logp = x - lse; sum logp = sum x - C lse"""
    xf = x.float()
    C = xf.shape[1]
    mx = xf.max(-1).values
    lse = mx + torch.log(torch.exp(xf - mx[:, None]).sum(-1))
    on, off = torch.tensor(1.0 - smoothing).float(), torch.tensor(smoothing).float() / float(C)
    lp1, lp2 = xf.gather(1, y1.view(-1, 1)).flatten() - lse, xf.gather(1, y2.view(-1, 1)).flatten() - lse
    sum_logp = xf.sum(-1) - float(C) * lse
    return -(off * sum_logp + on * (lam * lp1 + (1.0 - lam) * lp2))


def xent_grad_slack(ref_grad64, gscale, x, t):
    """[B, C]: |dlogits - exact| may reach one bf16 ulp of the larger of the two (the final rounding falls on the other side) plus
    2^-14 gscale (p + t): the fast exponential is good to about |arg| 2^-22 relative (|arg| <= 30 where p matters), far below
    2^-14, and p - t cancels where they are close"""
    p = torch.softmax(x.double(), -1)
    return 2.0 ** -14 * gscale * (p + t.double())


# ======================================================================================================== GRN
GRN_SHAPES = ((2, 49, 128), (2, 49, 192))                 # the two smallest channel counts icamd_grn_supported admits
GRN_EXPONENTS = (-20, -6, 0, 4, 10)
GRN_ZERO_CH, GRN_TAIL_CH = 11, 21                         # sample 0 keeps them; sample N - 1 is all zero


def grn_operands(N, HW, C, seed=331):
    """z, a = gelu(z) scaled per channel by 2^e (exact), dg, gamma, beta; a[:, :, GRN_ZERO_CH] = 0, a[N - 1] = 0, and
    z[:, :, GRN_TAIL_CH] <= -12 (a = -0.0 or the smallest magnitudes of GELU's lower tail)"""
    z = rnd_bf16(N, HW, C, seed=seed)
    z[:, :, GRN_TAIL_CH] = -12.0 - z[:, :, GRN_TAIL_CH].abs()
    z = R.bf16_round(z)
    a = R.bf16_round(torch.nn.functional.gelu(z.double()).float())
    e = torch.tensor([GRN_EXPONENTS[c % len(GRN_EXPONENTS)] for c in range(C)], dtype=torch.float32)
    a = R.bf16_round(a * torch.exp2(e))
    a[:, :, GRN_ZERO_CH] = 0.0
    a[N - 1] = 0.0
    g = torch.Generator().manual_seed(seed + 1)
    return {"z": z, "a": a, "dg": rnd_bf16(N, HW, C, seed=seed + 2), "gamma": 0.5 * torch.randn(C, generator=g),
            "beta": 0.1 * torch.randn(C, generator=g), "e": e}


# ======================================================================================================== step kernels
STEP_N = 4096 + 64
G_EXPONENTS = (-60, -30, -10, 0, 10, 20)
STEP_KINDS = ("adamw", "adam", "momentum", "nesterov", "lion")
STEP_TS = (1, 2, 10 ** 6)
P_RTOL = 2e-5


def step_operands(seed=341):
    """p (magnitude 2^+-20 in alternating runs of 6), g (element magnitude 2^e, e cycling through G_EXPONENTS), a first moment and a
    second moment of the gradient's size, an EMA near p.  Elements STEP_ZERO (small-p runs) have g = m = 0: Lion's sign(0)."""
    g = torch.Generator().manual_seed(seed)
    n = STEP_N
    i = torch.arange(n)
    pe = torch.where((i // 6) % 2 == 0, 20.0, -20.0)
    ge = torch.tensor(G_EXPONENTS, dtype=torch.float32)[i % 6]
    p = torch.randn(n, generator=g) * torch.exp2(pe)
    grad = torch.randn(n, generator=g) * torch.exp2(ge)
    m = 0.5 * torch.randn(n, generator=g) * torch.exp2(ge)
    v = (0.5 * torch.randn(n, generator=g) * torch.exp2(ge)) ** 2
    ema = p * (1.0 + 0.01 * torch.randn(n, generator=g))
    zero = torch.nonzero(((i // 6) % 2 == 1) & (i % 7 == 3)).flatten()
    grad[zero] = 0.0
    m[zero] = 0.0
    return {"p": p, "g": grad, "m": m, "v": v, "ema": ema, "zero": zero}


def largest_term_bound(rtol, *terms):
    """rtol x the largest of |terms| per element: an element that is smaller than rtol x the largest term of its own update (a
    parameter of 2^-20 moved by a step of 1e-3, say) is held by that product instead of by its own size"""
    big = terms[0].double().abs()
    for t in terms[1:]:
        big = torch.maximum(big, t.double().abs())
    return rtol * big
