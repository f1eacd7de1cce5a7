"""Operands that move the softmax of the attention kernels out of the band `randn` keeps it in, their fp64 references, and the
bounds the GPU tests hold the kernels to (tests/test_attention_ranges_gpu.py; tests/test_attention_ranges_cpu.py keeps this file
honest).  torch on the CPU only; every operand is on the bf16 grid.

With q, k ~ randn every logit lies within a few units of zero and every log-sum-exp between 2 and 7.  The regimes:

  shift      softmax is invariant under a per-query constant, so one is added THROUGH THE OPERANDS and the mathematical problem stays
             the well-conditioned randn one: k[:, D0] = 1 for every key, q[i, D0] = c_i / scale with c_i cycling per query row through
             CYCLE, so that rows whose lse lies near -160 ... +128 share a workgroup and a 16-row block.  Every c_i / scale is an
             integer multiple of a power of two with at most 5 significant bits at head dimension 64: exact in bf16.
  shift_heads  the same with the cycle started at another position in every (image, head) pair, so that a persistent workgroup's
             consecutive heads shift different rows
  peaked     q and k times 4: logits of standard deviation 16, the largest probability of a row around 0.9
  flat       q and k divided by 64
  zero_q     q = 0: the softmax is exactly uniform, out = mean_j v_j and lse = log T without any oracle
  v64, do_big, do_small   the shift operands with v times 64, dO times 2^10, dO times 2^-20

In the shift regimes column D0 of dK is sum_i dS_ij c_i -- O(10^2 .. 10^3), it would dominate a norm over all of dK -- and column D0
of dQ is scale * sum_j dS_ij = 0 in exact arithmetic (rows of dS sum to zero).  errors() therefore takes the rel-L2 of dK over the D0
columns and over the others separately, and holds dQ's D0 column absolutely (dq_d0_excess)."""
import torch

from _harness import rnd_bf16
from oracle import ops_ref as R

D = 64
SCALE = D ** -0.5
D0 = 5                                             # the head dimension that carries the shift
CYCLE = (0.0, 40.0, -40.0, -100.0, -128.0, 128.0, -160.0, 96.0)
OUT_BOUND = 3e-3                                   # rel-L2 bounds of tests/test_attention_long_gpu.py, unchanged
GRAD_BOUND = 6e-3

SHIFTED = ("shift", "shift_heads", "v64", "do_big", "do_small")
REGIMES = ("shift", "peaked", "flat", "zero_q", "v64", "do_big", "do_small")

B, H = 2, 3
RESIDENT_4 = (17, 50, 64)                          # attn_*_kernel<4>: 64 rows resident, only T = 64 has no pad keys
RESIDENT_13 = (100, 197, 208)                      # attn_*_kernel<13>: 224 rows resident, pad keys at every T
TILED = (209, 256, 257, 333)                       # attention_long.hip: 64-row key tiles; 256 fills its last tile
ALL_REGIMES_T = (50, 197, 257)
# (regime, B, T, H)
CASES = [("shift", B, T, H) for T in RESIDENT_4 + RESIDENT_13 + TILED] + \
        [(r, B, T, H) for T in ALL_REGIMES_T for r in REGIMES if r != "shift"]
# One more, for the hand-over between the heads a persistent workgroup of attention.hip walks (the next head's lse travels through
# a prefetch): the launcher caps the grid at the number of CUs, so B * H must exceed that.  256 CUs on MI355X.
PERSISTENT_T, PERSISTENT_H = 50, 3


def persistent_case(cus):
    return ("shift_heads", cus // PERSISTENT_H + 1, PERSISTENT_T, PERSISTENT_H)


def head_offset(pair):
    """where pair (image * H + head) starts in CYCLE under shift_heads; pair and pair + 256 differ (256 % 7 = 4)"""
    return pair % 7


def shift_constants(T, offset=0):
    return torch.tensor([CYCLE[(i + offset) % len(CYCLE)] for i in range(T)])


def operands(regime, B, T, H):
    """(qkv [B*T, 3*H*D], dout [B*T, H*D]) in fp32, every value on the bf16 grid"""
    qkv, dout = rnd_bf16(B * T, 3 * H * D, seed=120), rnd_bf16(B * T, H * D, seed=121)
    x = qkv.view(B, T, 3, H, D)                    # [:, :, 0 / 1 / 2] = q / k / v
    if regime in SHIFTED:
        x[:, :, 1, :, D0] = 1.0
        for b in range(B):
            for h in range(H):
                off = head_offset(b * H + h) if regime == "shift_heads" else 0
                x[b, :, 0, h, D0] = shift_constants(T, off) / SCALE
        if regime == "v64":
            x[:, :, 2] *= 64.0
        elif regime == "do_big":
            dout *= 2.0 ** 10
        elif regime == "do_small":
            dout *= 2.0 ** -20
    elif regime == "peaked":
        x[:, :, 0:2] *= 4.0
    elif regime == "flat":
        x[:, :, 0:2] /= 64.0
    elif regime == "zero_q":
        x[:, :, 0] = 0.0
    else:
        raise ValueError(regime)
    return qkv, dout


def d0_columns(H):
    """columns of a [rows, H*D] slice (q, k, dq or dk) that hold dimension D0 of every head, and the mask of all the others"""
    cols = torch.arange(H) * D + D0
    rest = torch.ones(H * D, dtype=torch.bool)
    rest[cols] = False
    return cols, rest


def bf16_ulp(x):
    """spacing of the bf16 grid at |x| (fp64 tensor)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - 7)


def dq_d0_bound(ds, scale):
    """[B, H, T]: what |dq[i, D0]| may reach in a shift regime.  Exactly, dq[i, D0] = scale * sum_j dS_ij * 1 = 0.  The kernels round
    dS to bf16 (unit roundoff 2^-8) in front of that sum, so it is off by at most 2^-8 * scale * sum_j |dS_ij|, and the stored value
    is rounded once more: one bf16 ulp at that size.  The factor 2 is margin for the fp32 accumulation order."""
    r = 2.0 ** -8 * scale * ds.abs().sum(-1)
    return 2.0 * (r + bf16_ulp(r))


_REF = {}


def reference(case):
    """fp64 references of a case, computed once and shared, never modified: "exact" is R.attention_fwd / attention_bwd with fp64
    accumulation (autograd), "points" the written-out oracle with the kernels' rounding points, "ds" the exact dS, and "e_round"
    the errors() of points against exact: reference against reference, what the rounding points alone cost."""
    if case not in _REF:
        regime, B, T, H = case
        qkv, dout = operands(regime, B, T, H)
        out, lse = R.attention_fwd(qkv, B, T, H, D, SCALE, acc=torch.float64)
        exact = {"out": out, "lse": lse, "dqkv": R.attention_bwd(qkv, dout, B, T, H, D, SCALE, acc=torch.float64)}
        written = R.attention_written_out(qkv, dout, B, T, H, D, SCALE)
        points = R.attention_written_out(qkv, dout, B, T, H, D, SCALE, rounding_points=True)
        ref = {"qkv": qkv, "dout": dout, "exact": exact, "written": written, "points": points, "ds": written["ds"]}
        ref["e_round"] = errors(case, points["out"], points["dqkv"], ref)
        _REF[case] = ref
    return _REF[case]


def errors(case, out, dqkv, ref):
    """rel-L2 of out [B*T, H*D] and of the parts of dqkv [B*T, 3*H*D] against the exact reference: out, dq, dk, dv; in a shift
    regime dq is taken without its D0 columns and dk as dk_d0 and dk (the other columns), and dq_d0_excess is the largest
    |dq[i, D0]| / dq_d0_bound (<= 1 passes).  A non-finite value makes its entry NaN or inf, which no bound admits."""
    regime, B, T, H = case
    ex = ref["exact"]
    HD = H * D
    out, dqkv = out.double(), dqkv.double()
    dq, dk, dv = dqkv[:, :HD], dqkv[:, HD:2 * HD], dqkv[:, 2 * HD:]
    rq, rk, rv = ex["dqkv"][:, :HD], ex["dqkv"][:, HD:2 * HD], ex["dqkv"][:, 2 * HD:]
    e = {"out": R.rel_l2(out, ex["out"]), "dv": R.rel_l2(dv, rv)}
    if regime in SHIFTED:
        cols, rest = d0_columns(H)
        e["dq"] = R.rel_l2(dq[:, rest], rq[:, rest])
        e["dk"] = R.rel_l2(dk[:, rest], rk[:, rest])
        e["dk_d0"] = R.rel_l2(dk[:, cols], rk[:, cols])
        bound = dq_d0_bound(ref["ds"], SCALE).permute(0, 2, 1).reshape(B * T, H)      # [B, H, T] -> rows of dq
        e["dq_d0_excess"] = float((dq[:, cols].abs() / bound).max())
    else:
        e["dq"] = R.rel_l2(dq, rq)
        e["dk"] = R.rel_l2(dk, rk)
    return e


def caps(case, e_round):
    """the bound of every entry of errors().  The existing bounds everywhere; in the peaked regime, where the rounding points
    themselves cost about twice what they cost on randn, max(existing bound, 1.5 * e_round): the factor 1.5 covers the fp32
    accumulation order and the hardware exp2, and the yardstick is the rounding-point ORACLE, never the kernel."""
    regime = case[0]
    c = {}
    for name in e_round:
        base = OUT_BOUND if name == "out" else 1.0 if name == "dq_d0_excess" else GRAD_BOUND
        c[name] = max(base, 1.5 * e_round[name]) if regime == "peaked" and name != "dq_d0_excess" else base
    return c


def table_row(case, e_round, measured, cap):
    regime, B, T, H = case
    cells = "  ".join(f"{n} {e_round[n]:.2e}/{measured[n]:.2e}/{cap[n]:.2e}" for n in measured)
    return f"{regime:11s} B {B:3d} T {T:3d} H {H} (e_round/measured/cap): {cells}"


# ---- window kernels: the shift goes into the fp32 bias table, row by row, where it is exact to fp32 and stacks on the -100 mask ----
def shifted_bias(bias):
    """bias [H, T, T] with CYCLE added to its rows (query i gets c_i), as fp32: kernel and reference read the same table"""
    T = bias.shape[-1]
    return (bias + shift_constants(T)[None, :, None]).float()

