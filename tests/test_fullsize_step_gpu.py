"""Element-wise parity of the kernels every training step and every eval run ENDS in -- loss, metrics, gradient norm, the
fused optimizers with EMA and bf16 shadow, the EMA buffer lerp, the input packers and the filter preparation (transposes,
BatchNorm fold, layer-scale fold) -- at the sizes the benchmark produces, with default routing.

tests/test_fullsize_layers_gpu.py covers the per-layer kernels; these are the ones it leaves out.  A wrong value here does
not show up as a wrong activation, it corrupts the weights: a grid-stride loop that skips or double-applies a slice of an
86 M-element arena, a clip coefficient read from the wrong slot, a fold job that lands one row off.  Sizes come from the
models themselves (ResNet-50, ViT-B/16, ConvNeXt-T at 1000 classes: n_params, buffer_arena, ncls_p, the transpose and fold
job tables); every case launches the C-ABI entry the models and the engine launch and compares EVERY output element with
the operation written plainly in fp64 with torch on the GPU (oracle/ops_ref.py: optimizer_step_f64, ema_step_f64, pinned
on the CPU against torch.optim in tests/test_oracle_cpu.py), with the comparisons of tests/_fullsize_check.py.

Bounds and where they come from:
  optimizer p / m / v / ema   rtol 2e-5 atol 1e-6 / 1e-5, 1e-7 / 1e-5, 1e-9 / 1e-5, 1e-6: test_adamw_ema_gradnorm and
                              test_other_fused_optimizers (tests/test_kernels_gpu.py), here on every element, no outliers
  gradient norm, clip         rtol 1e-5, 1e-5 absolute: test_adamw_ema_gradnorm
  lerp                        rtol 1e-6 atol 1e-7: test_colsum_lerp_cast; the cast is bit-equal to torch's, as there
  loss rows, mean loss        rtol 1e-4 atol 1e-5, 1e-5 relative: test_softmax_xent_and_metrics; dlogits: check_bf16
  input packing               exact for modes 0 and 2, <= 1 bf16 ulp for mixup: test_pack_input_mixup_cutmix
  folded filters, shifts      <= 1 bf16 ulp and rel L2 <= 2e-3 per 64 x 64 block; rtol 1e-5 + 1e-6 of the magnitudes: see
                              test_resnet50_batchnorm_fold (the measured worst cases are written there)

Wall time on an MI355X: 4.6 - 5.0 s for the 91 cases (three runs), 0.7 s of it building the three models -- a fifth of the
layer module's 25 s.  The fp64 references of the 86.6 M-element arenas cost 0.03 s per ViT-B/16 optimizer case; the slowest
cases are the first loss case (0.4 s, first use of the fp64 softmax) and the first optimizer and gradient-norm cases (0.2 s).
"""
import re

import pytest
import torch

import _harness
from _fullsize_check import (check_arena, check_bf16, check_bits, check_close, check_counts, check_fold, check_pred,
                             check_transposed, lowest_argmax, require)
from _harness import default_routing_lib as lib  # noqa: F401
from _harness import free_after_each  # noqa: F401
from _harness import sync
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
MODELS = ["resnet50", "vit_b16", "convnext_t"]

# the step under test is optimizer step t = 3: two fp64 reference steps from zero moments come before it (lr = 0 on the
# first, as the warm-up produces; the values of test_adamw_ema_gradnorm)
LRS, WDS = (0.0, 2.5e-4, 5e-4), (5e-4, 4.9e-4, 4.8e-4)
B1, B2, EPS, DECAY = 0.9, 0.999, 1e-8, 0.9995
GSCALE, COEF = 0.5, 0.37
P_TOL, M_TOL, V_TOL, EMA_TOL = (2e-5, 1e-6), (1e-5, 1e-7), (1e-5, 1e-9), (1e-5, 1e-6)
ZERO_GRAD, NO_SKIP_COUNT = 1, 2


@pytest.fixture(scope="module")
def models(lib):
    """The three benchmark models, built once: their arena sizes and job tables are what the cases run on."""
    from imageclassification_amd.convnext import ConvNeXt
    from imageclassification_amd.nets import ResNet
    from imageclassification_amd.vit import VisionTransformer
    return {"resnet50": ResNet("resnet50", 1000), "vit_b16": VisionTransformer("vit_base_patch16_224", 1000),
            "convnext_t": ConvNeXt("convnext_tiny", 1000, drop_path_rate=0.05)}


def randn(n, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, generator=g, device=DEV) * scale


def urand(n, seed, lo, hi):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(n, generator=g, device=DEV) * (hi - lo) + lo


def randint(n, seed, hi):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, hi, (n,), generator=g, device=DEV)


def sliced(n, seed, lo_exp=-4.0, hi_exp=2.0, slices=16):
    """Seeded normal values whose magnitude varies by slice of the arena (1e-4 ... 1e+2), as the layers' gradients do."""
    t = randn(n, seed)
    scale = 10.0 ** torch.linspace(lo_exp, hi_exp, slices, device=DEV)
    idx = (torch.arange(n, device=DEV) * slices // n).clamp_max(slices - 1)
    return t * scale[idx]


def ok(rc, what):
    assert rc == 0, f"{what}: rc {rc}"


def i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ======================================== 1. optimizer, EMA, shadow ========================================
class OptState:
    """p, m, v, ema in front of optimizer step 3 (two fp64 reference steps of the same optimizer from zero moments, rounded
    to fp32), the gradient of step 3, and the fp64 reference of that step."""

    def __init__(self, name, n, seed, gs, with_ema=True):
        self.name, self.n, self.gs = name, n, gs
        self.adam = name in ("adamw", "adam")
        p = randn(n, seed).double()
        ema = p.clone()
        m, v = torch.zeros(n, dtype=F64, device=DEV), torch.zeros(n, dtype=F64, device=DEV)
        for t in (1, 2):
            p, m, v = R.optimizer_step_f64(name, p, randn(n, seed + t, 0.1), m, v, LRS[t - 1], WDS[t - 1], t, (B1, B2), EPS, gs)
            ema = R.ema_step_f64(ema, p, DECAY)
        self.p0, self.m0, self.ema0 = p.float(), m.float(), ema.float()
        self.v0 = v.float() if self.adam else None
        del p, m, v, ema
        g = randn(n, seed + 3, 0.1)
        if name == "lion":
            # sign() of an interpolated momentum within rounding of zero may flip between fp32 and fp64: the inputs are
            # built so that the reference has no such element (1e-4 is three orders above fp32 rounding here)
            u = self.m0.double() * B1 + g.double() * gs * (1.0 - B1)
            near = u.abs() < 1e-4
            sgn = torch.where(self.m0 >= 0, 1.0, -1.0)
            g = torch.where(near, sgn * (0.1 / gs), g)
            u = self.m0.double() * B1 + g.double() * gs * (1.0 - B1)
            assert float(u.abs().min()) >= 1e-4 and 0 < int(near.sum()) < n // 4
            del u, near, sgn
        self.g = g
        self.with_ema = with_ema

    def reference(self):
        z = torch.zeros(1, dtype=F64, device=DEV)
        rp, rm, rv = R.optimizer_step_f64(self.name, self.p0, self.g, self.m0, self.v0 if self.adam else z, LRS[2], WDS[2], 3,
                                          (B1, B2), EPS, self.gs)
        return rp, rm, (rv if self.adam else None), R.ema_step_f64(self.ema0, rp, DECAY)

    def buffers(self):
        """Fresh device copies for one launch: p, g, m, v, ema, shadow."""
        shadow = torch.full((self.n,), float("nan"), dtype=torch.bfloat16, device=DEV)
        return [self.p0.clone(), self.g.clone(), self.m0.clone(), self.v0.clone() if self.adam else None,
                self.ema0.clone() if self.with_ema else None, shadow]


def opt_launch(lib, name, bufs, n, step, gscale, clip, fin, skipped, flags, lo=0, hi=None, lr=LRS[2], wd=WDS[2]):
    hip = _harness.hip()
    hi = n if hi is None else hi
    p, g, m, v, ema, shadow = bufs

    def at(t, esz):
        return None if t is None else t.data_ptr() + esz * lo
    args = (at(p, 4), at(g, 4), at(m, 4), at(v, 4), at(ema, 4), at(shadow, 2), hi - lo, lr, wd, B1, B2, EPS, step, gscale,
            DECAY, hip.ptr(clip), hip.ptr(fin), hip.ptr(skipped), flags, hip.stream_ptr())
    if name == "adamw":
        ok(lib.icamd_adamw_ema(*args), "icamd_adamw_ema")
    else:
        ok(lib.icamd_optim_ema(R.OPT_KINDS[name], *args), f"icamd_optim_ema {name}")


def optimizer_step_case(lib, name, n, seed, with_clip):
    """One step at t = 3 with `skipped` = 1 and step = 4 attempted; with_clip: clip -> [norm, coef], EMA present; else
    clip = NULL and ema = NULL."""
    gs = GSCALE * COEF if with_clip else GSCALE
    st = OptState(name, n, seed, gs, with_ema=with_clip)
    bufs = st.buffers()
    clip = torch.tensor([123.0, COEF], device=DEV) if with_clip else None
    fin, skipped = i32(1), i32(1)
    opt_launch(lib, name, bufs, n, 4, GSCALE, clip, fin, skipped, ZERO_GRAD)
    sync()
    p, g, m, v, ema, shadow = bufs
    rp, rm, rv, rema = st.reference()
    require(check_arena(p, rp, *P_TOL, what="p") + check_arena(m, rm, *M_TOL, what="m"), f"{name} step")
    if st.adam:
        require(check_arena(v, rv, *V_TOL, what="v"), f"{name} step")
    if with_clip:
        require(check_arena(ema, rema, *EMA_TOL, what="ema"), f"{name} step")
        require(check_bits(clip, torch.tensor([123.0, COEF], device=DEV), "clip buffer"), f"{name} step")
    require(check_bits(shadow, p.to(torch.bfloat16), "bf16 shadow of the kernel's own p"), f"{name} step")
    require(check_bits(g, torch.zeros_like(g), "gradient arena after zero_grad"), f"{name} step")
    assert int(skipped) == 1 and int(fin) == 1
    return st, bufs, (rp, rm, rv, rema)


@pytest.mark.parametrize("with_clip", [True, False], ids=["clip-ema", "plain"])
@pytest.mark.parametrize("model", MODELS)
def test_adamw_ema_step(lib, models, model, with_clip):
    n = models[model].n_params
    assert n > 2048 * 256 * 4 * 2, "the arena must take the capped grid through several trips of its loop"
    optimizer_step_case(lib, "adamw", n, 100 + 10 * MODELS.index(model), with_clip)


@pytest.mark.parametrize("with_clip", [True, False], ids=["clip-ema", "plain"])
@pytest.mark.parametrize("name", ["adam", "momentum", "nesterov", "lion"])
def test_other_optimizers_step(lib, models, name, with_clip):
    optimizer_step_case(lib, name, models["resnet50"].n_params, 200 + 10 * R.OPT_KINDS[name], with_clip)


def test_the_arena_comparison_rejects_a_corrupted_slice_of_real_output(lib, models):
    """As tests/test_fullsize_checkers_cpu.py shows on synthetic data, on the kernel's own output: 1024 elements of p put
    back to what they were before the step make the comparison fail, and name the slice."""
    n = models["resnet50"].n_params
    st, bufs, (rp, _, _, _) = optimizer_step_case(lib, "adamw", n, 100, True)
    p = bufs[0]
    lo = (n // 2 // 1024) * 1024 + 512
    p[lo:lo + 1024] = st.p0[lo:lo + 1024]
    fails = check_arena(p, rp, *P_TOL, what="p")
    assert len(fails) == 1, fails
    found = re.match(r"p: (\d+) of \d+ off .*first \[(\d+)\].*last \[(\d+)\]", fails[0])
    assert found, fails
    count, first, last = (int(v) for v in found.groups())
    assert 900 <= count <= 1024 and lo <= first and last < lo + 1024, fails


@pytest.mark.parametrize("name,model", [("adamw", "vit_b16"), ("adam", "resnet50"), ("momentum", "resnet50"),
                                        ("nesterov", "resnet50"), ("lion", "resnet50")])
def test_skipped_step_leaves_every_arena_untouched(lib, models, name, model):
    """Flag down, NaN gradients: p, m, v, ema, shadow and the gradient arena bit-unchanged, `skipped` incremented once; with
    ICAMD_OPT_NO_SKIP_COUNT not incremented."""
    n = models[model].n_params
    st = OptState(name, n, 300 + R.OPT_KINDS[name], GSCALE * COEF)
    st.g = torch.full((n,), float("nan"), device=DEV)
    bufs = st.buffers()
    bufs[5] = randn(n, 7).to(torch.bfloat16)
    before = [None if t is None else t.clone() for t in bufs]
    clip = torch.tensor([123.0, COEF], device=DEV)
    fin, skipped = i32(0), i32(1)
    opt_launch(lib, name, bufs, n, 4, GSCALE, clip, fin, skipped, ZERO_GRAD)
    sync()
    assert int(skipped) == 2
    opt_launch(lib, name, bufs, n, 5, GSCALE, clip, fin, skipped, ZERO_GRAD | NO_SKIP_COUNT)
    sync()
    assert int(skipped) == 2 and int(fin) == 0
    for what, a, b in zip(("p", "g", "m", "v", "ema", "shadow"), bufs, before):
        if a is not None:
            require(check_bits(a, b, what), f"{name} skipped step")


def test_bucketed_adamw_is_bit_identical_to_one_launch(lib, models):
    """The data-parallel path applies the step range by range, one launch per gradient bucket (GradReducer's default sizes:
    1 MiB first, 25 MiB, 4 MiB last), every launch but one carrying ICAMD_OPT_NO_SKIP_COUNT."""
    from imageclassification_amd import ddp
    n = models["vit_b16"].n_params
    mib = (1 << 20) // 4
    buckets = ddp.make_buckets(n, 1 * mib, 25 * mib, last_bucket_elems=4 * mib)
    spans = sorted(buckets)
    assert spans[0][0] == 0 and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and len(spans) >= 4
    assert all((hi - lo) % 4 == 0 and lo % 4 == 0 for lo, hi in spans)
    st = OptState("adamw", n, 120, GSCALE * COEF)
    clip = torch.tensor([123.0, COEF], device=DEV)
    fin, skipped = i32(1), i32(1)
    one = st.buffers()
    opt_launch(lib, "adamw", one, n, 4, GSCALE, clip, fin, skipped, ZERO_GRAD)
    many = st.buffers()
    for i, (lo, hi) in enumerate(buckets):          # launch order: from the end of the arena backwards
        flags = ZERO_GRAD | (NO_SKIP_COUNT if i != len(buckets) - 1 else 0)
        opt_launch(lib, "adamw", many, n, 4, GSCALE, clip, fin, skipped, flags, lo, hi)
    sync()
    assert int(skipped) == 1
    for what, a, b in zip(("p", "g", "m", "v", "ema", "shadow"), many, one):
        require(check_bits(a, b, what), "bucketed AdamW")


def test_grad_guard_on_a_full_arena(lib, models):
    hip = _harness.hip()
    n = models["vit_b16"].n_params
    g = randn(n, 130)
    g[n - 1] = float("nan")
    g[n // 2] = float("inf")
    keep = g.clone()
    fin = i32(1)
    ok(lib.icamd_grad_guard(g.data_ptr(), n, fin.data_ptr(), hip.stream_ptr()), "grad_guard")
    sync()
    require(check_bits(g, keep, "gradients with the flag up"), "grad_guard")
    fin.zero_()
    ok(lib.icamd_grad_guard(g.data_ptr(), n, fin.data_ptr(), hip.stream_ptr()), "grad_guard")
    sync()
    require(check_bits(g, torch.zeros_like(g), "gradients with the flag down"), "grad_guard")


# ======================================== 2. gradient norm ========================================
@pytest.mark.parametrize("model,tail", [(m, 0) for m in MODELS] + [("convnext_t", 3)], ids=MODELS + ["convnext_t-minus3"])
def test_grad_norm(lib, models, model, tail):
    hip = _harness.hip()
    n = models[model].n_params - tail
    assert n // 4 > 512 * 256 * 2
    g = sliced(models[model].n_params, 140 + MODELS.index(model))[:n]
    ref = float(torch.linalg.vector_norm(g.double()))
    ws = torch.empty(lib.icamd_grad_norm_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for inv_scale in (1.0, 1.0 / 65536):
        norm = ref * inv_scale
        for max_norm in (0.0, 0.5 * norm, 2.0 * norm):
            out = torch.full((2,), float("nan"), device=DEV)
            ok(lib.icamd_grad_norm(g.data_ptr(), n, inv_scale, max_norm, ws.data_ptr(), out.data_ptr(), hip.stream_ptr()),
               "grad_norm")
            sync()
            got, coef = out.tolist()
            what = f"n {n} inv_scale {inv_scale:g} max_norm {max_norm:g}: norm {got:.9g} vs {norm:.9g}, coef {coef:.9g}"
            assert abs(got - norm) <= 1e-5 * norm, what
            if max_norm == 0.0:
                assert coef == 1.0, what
            else:
                assert abs(coef - min(1.0, max_norm / (norm + 1e-6))) <= 1e-5, what


# ======================================== 3. EMA buffers and casts ========================================
@pytest.mark.parametrize("which", ["vit_b16-params", "resnet50-buffers"])
def test_lerp(lib, models, which):
    hip = _harness.hip()
    n = models["vit_b16"].n_params if which == "vit_b16-params" else models["resnet50"].buffer_arena.numel()
    assert n > 50000
    dst0, src = randn(n, 150), randn(n, 151)
    w = 1.0 - 0.9995
    fin = i32(1)
    dst = dst0.clone()
    ok(lib.icamd_lerp(dst.data_ptr(), src.data_ptr(), n, w, fin.data_ptr(), hip.stream_ptr()), "lerp")
    sync()
    ref = dst0.double() + w * (src.double() - dst0.double())
    require(check_arena(dst, ref, 1e-6, 1e-7, what="lerp"), which)
    dst = dst0.clone()
    ok(lib.icamd_lerp(dst.data_ptr(), src.data_ptr(), n, 1.0, None, hip.stream_ptr()), "lerp")
    sync()
    require(check_bits(dst, src, "w = 1 is a copy"), which)
    dst, fin = dst0.clone(), i32(0)
    ok(lib.icamd_lerp(dst.data_ptr(), src.data_ptr(), n, w, fin.data_ptr(), hip.stream_ptr()), "lerp")
    sync()
    require(check_bits(dst, dst0, "flag down: untouched"), which)


# fp32 bit patterns whose bf16 rounding is where a hand-written cast goes wrong (round to nearest, ties to even)
CAST_EDGES = [0x3FFFFFFF, 0x3F7FFFFF, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF,
              0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00800000,
              0x00FF8000, 0x477FE000]
CAST_DENORMALS = [0x00000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x007F8000]


@pytest.mark.parametrize("model", MODELS)
def test_f32_to_bf16(lib, models, model):
    """Bit-equal to torch's cast on a whole parameter arena, with the edge patterns planted in the first, a later and the
    last trip of the grid-stride loop.  fp32 denormals (no parameter is ever that small) are reported, not asserted: the
    hardware conversion may flush them."""
    hip = _harness.hip()
    n = models[model].n_params
    assert n > 524288 * 2
    src = sliced(n, 160 + MODELS.index(model), -3.0, 1.0)
    pats = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in CAST_EDGES + CAST_DENORMALS], dtype=torch.int32,
                        device=DEV)
    k = pats.numel()
    starts = [0, 524288 + 17, n // 2 + 3, n - k]
    den = torch.zeros(n, dtype=torch.bool, device=DEV)
    for s in starts:
        src.view(torch.int32)[s:s + k] = pats
        den[s + len(CAST_EDGES):s + k] = True
    dst = torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_f32_to_bf16(src.data_ptr(), dst.data_ptr(), n, hip.stream_ptr()), "f32_to_bf16")
    sync()
    want = src.to(torch.bfloat16)
    diff = dst.view(torch.int16) != want.view(torch.int16)
    if bool((diff & den).any()):
        i = torch.nonzero(diff & den).flatten()[:6]
        print(f"f32_to_bf16 on fp32 denormals differs from torch at {int((diff & den).sum())} planted elements, e.g. "
              f"{[hex(v & 0xFFFFFFFF) for v in src.view(torch.int32)[i].tolist()]} -> "
              f"{[hex(v & 0xFFFF) for v in dst.view(torch.int16)[i].tolist()]} (torch "
              f"{[hex(v & 0xFFFF) for v in want.view(torch.int16)[i].tolist()]})")
    bad = diff & ~den
    assert not bool(bad.any()), (f"{int(bad.sum())} of {n} differ from torch's cast, first [{int(torch.nonzero(bad)[0])}] "
                                 f"{hex(int(src.view(torch.int32)[int(torch.nonzero(bad)[0])]) & 0xFFFFFFFF)}")


# ======================================== 4. loss and metrics ========================================
def tie_columns(C):
    """Per row (r % 3): the tied columns.  (a) the lowest index (5) sits in a higher lane than the other (64 + 3 -> lane 3);
    (b) both in lane 7, the second in the lane's next trip; (c) the first and the last column."""
    return [(5, 64 + 3), (7, 71), (0, C - 1)] if C > 72 else [(5, 3 + 4), (2, 7), (0, C - 1)]


def make_logits(kind, B, C, seed):
    """bf16 logits [B, C] and hard labels for them."""
    rows = torch.arange(B, device=DEV)
    y = randint(B, seed + 1, C)
    if kind == "normal":
        x = randn((B, C), seed, 3.0)
    elif kind == "late":
        # late training: one class per row at +30 ... +60, the rest around -10, the label on that class for three rows of
        # four.  In fp32 (the kernel's, and torch's own) softmax - onehot of such a row is exactly 0 at the label while
        # fp64 keeps the -1e-13 the other classes sum to; a 64 x 64 block holding nothing else has no scale to measure
        # that against.  So the fourth row of every four is misclassified, with its hot and label columns walking through
        # the column tiles: every block of the per-block bound then holds an O(gscale) entry, as real late-training
        # batches with a few percent of errors do.
        x = randn((B, C), seed, 1.5) - 10.0
        ntile = (C + 63) // 64
        width = C - (ntile - 1) * 64                  # of the last column tile: columns every tile has
        k = (rows % 64) // 4                          # the k-th misclassified row of its 64-row tile
        hot = (k % ntile) * 64 + (rows * 7) % width
        lab = ((k + ntile // 2) % ntile) * 64 + (rows * 11 + 3) % width
        wrong = rows % 4 == 3
        hot = torch.where(wrong, hot, y)
        lab = torch.where(lab == hot, (lab + 1) % C, lab)
        y = torch.where(wrong, lab, y)
        x[rows, hot] = urand(B, seed + 2, 30.0, 60.0)
    elif kind == "ties":
        x = randn((B, C), seed, 3.0).to(torch.bfloat16).float()
        top = (x.max(1).values + 1.0).to(torch.bfloat16).float()
        cols = torch.tensor(tie_columns(C), device=DEV)[rows % 3]
        x[rows, cols[:, 0]] = top
        x[rows, cols[:, 1]] = top
    else:
        raise ValueError(kind)
    return x.to(torch.bfloat16), y


def xent_ref(x, y1, y2, lam, smoothing, gscale):
    """fp64, from the bf16 logits: per-row loss and (softmax - t) * gscale, t = lam onehot_s(y1) + (1 - lam) onehot_s(y2)."""
    xd = x.double()
    C = xd.shape[1]
    t = torch.full_like(xd, smoothing / C)
    t.scatter_add_(1, y1.view(-1, 1), torch.full((len(y1), 1), (1.0 - smoothing) * lam, dtype=F64, device=x.device))
    t.scatter_add_(1, (y1 if y2 is None else y2).view(-1, 1),
                   torch.full((len(y1), 1), (1.0 - smoothing) * (1.0 - lam), dtype=F64, device=x.device))
    logp = torch.log_softmax(xd, -1)
    return -(t * logp).sum(-1), (logp.exp() - t) * gscale


SENTINEL = 0x7A5B      # bf16 bit pattern of the rows behind row B


def run_xent(lib, x, ld, y1, y2, lam, smoothing, gscale, want_pred=True, want_dl=True):
    hip = _harness.hip()
    B, C = x.shape
    lp = torch.zeros(B, ld, dtype=torch.bfloat16, device=DEV)
    lp[:, :C] = x
    loss = torch.full((B + 4,), float("nan"), device=DEV)
    pred = torch.full((B + 4,), -7, dtype=torch.int32, device=DEV) if want_pred else None
    dl = torch.full((B + 4, ld), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16) if want_dl else None
    ok(lib.icamd_softmax_xent(lp.data_ptr(), ld, B, C, y1.data_ptr(), hip.ptr(y2), lam, smoothing, gscale, loss.data_ptr(),
                              hip.ptr(pred), hip.ptr(dl), hip.stream_ptr()), "softmax_xent")
    sync()
    return loss, pred, dl


LOSS_SHAPES = [(256, 1000, 1024), (384, 1000, 1024), (250, 1000, 1024), (256, 10, 64)]
TARGET_FORMS = {"hard": (0.0, 1.0), "smooth": (0.1, 1.0), "mixup": (0.1, 0.3)}


@pytest.mark.parametrize("form", list(TARGET_FORMS))
@pytest.mark.parametrize("kind", ["normal", "late", "ties"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=[f"B{b}-C{c}" for b, c, _ in LOSS_SHAPES])
def test_softmax_xent(lib, shape, kind, form):
    B, C, ld = shape
    smoothing, lam = TARGET_FORMS[form]
    x, y1 = make_logits(kind, B, C, 170 + B + C)
    y2 = None
    if form == "mixup":
        for r in (3, 10):                 # rows whose two targets coincide
            y1[B - 1 - r] = y1[r]
        y2 = y1.flip(0).contiguous()
        assert int((y1 == y2).sum()) >= 4 and int((y1 != y2).sum()) > B // 2
    gscale = 1.0 / B
    loss, pred, dl = run_xent(lib, x, ld, y1, y2, lam, smoothing, gscale)
    rl, rd = xent_ref(x, y1, y2, lam, smoothing, gscale)
    require(check_close(loss[:B], rl, 1e-4, 1e-5, "loss rows"), "softmax_xent")
    assert bool(torch.isnan(loss[B:]).all()) and bool((pred[B:] == -7).all()), "rows behind B written"
    # the expected prediction is the lowest tied index: torch.argmax on the CPU against the explicit min(index of max)
    assert torch.equal(x.float().cpu().argmax(1), lowest_argmax(x).cpu())
    if kind == "ties":
        cols = torch.tensor(tie_columns(C), device=DEV)[torch.arange(B, device=DEV) % 3]
        assert torch.equal(lowest_argmax(x), cols.min(1).values)
    require(check_pred(pred[:B], x), "softmax_xent")
    ref = torch.zeros(B, ld, device=DEV)
    ref[:, :C] = R.bf16_round(rd.float())
    require(check_bf16(dl[:B].float(), ref, rel=2e-3), "dlogits")
    assert not bool(dl[:B, C:].view(torch.int16).any()), "padding columns of dlogits are not exactly zero"
    assert bool((dl[B:].view(torch.int16) == SENTINEL).all()), "rows of dlogits behind row B written"


@pytest.mark.parametrize("B", [256, 384])
def test_softmax_xent_call_forms_of_the_engine(lib, B):
    """pred = NULL (training steps that keep no predictions) and dlogits = NULL with gscale = 0 (eval, and the second,
    accuracy-only forward under mixup): the outputs that are asked for are bit-identical to the full call's."""
    C, ld = 1000, 1024
    x, y1 = make_logits("normal", B, C, 180)
    full = run_xent(lib, x, ld, y1, None, 1.0, 0.1, 1.0 / B)
    nopred = run_xent(lib, x, ld, y1, None, 1.0, 0.1, 1.0 / B, want_pred=False)
    require(check_bits(nopred[0], full[0], "loss rows") + check_bits(nopred[2], full[2], "dlogits"), "pred = NULL")
    nodl = run_xent(lib, x, ld, y1, None, 1.0, 0.0, 0.0, want_dl=False)
    rl, _ = xent_ref(x, y1, None, 1.0, 0.0, 0.0)
    require(check_close(nodl[0][:B], rl, 1e-4, 1e-5, "loss rows") + check_pred(nodl[1][:B], x), "dlogits = NULL")
    assert bool(torch.isnan(nodl[0][B:]).all()) and bool((nodl[1][B:] == -7).all())


def metrics_inputs(B, C, seed):
    """Loss rows, targets with one class holding a third of the batch (colliding atomics), predictions 60 % right and
    otherwise mostly on that class too."""
    loss = urand(B, seed, 0.5, 7.0)
    target = randint(B, seed + 1, C)
    target[::3] = 7
    wrong = torch.where(urand(B, seed + 2, 0, 1) < 0.5, torch.full_like(target, 7), randint(B, seed + 3, C))
    pred = torch.where(urand(B, seed + 4, 0, 1) < 0.6, target, wrong).int()
    return loss, pred, target


def metrics_call(lib, loss, pred, target, B, C, st, slot, respect_skip):
    hip = _harness.hip()
    ok(lib.icamd_step_metrics(hip.ptr(loss), hip.ptr(pred), target.data_ptr(), B, C, st["loss_out"].data_ptr(),
                              st["fin"].data_ptr(), st["acc"].data_ptr(), st["counts"].data_ptr(), st["log"].data_ptr(), slot,
                              8, respect_skip, hip.stream_ptr()), "step_metrics")
    sync()


def metrics_state(C):
    return {"loss_out": torch.full((1,), float("nan"), device=DEV), "fin": i32(-1),
            "acc": torch.zeros(8, dtype=F64, device=DEV), "counts": torch.zeros(3, C, dtype=torch.int32, device=DEV),
            "log": torch.full((16,), float("nan"), device=DEV)}


def expected_acc(loss_out, correct, B, times):
    """acc[0..4] after `times` identical accumulations from zero: sums of exactly representable values."""
    frac = float(torch.tensor(float(correct), dtype=torch.float32) / torch.tensor(float(B), dtype=torch.float32))
    return [times * float(loss_out), float(times), times * frac, float(times * correct), float(times * B), 0.0, 0.0, 0.0]


@pytest.mark.parametrize("B", [256, 384, 700])
def test_step_metrics(lib, B):
    C = 1000
    loss, pred, target = metrics_inputs(B, C, 190 + B)
    correct = int((pred.long() == target).sum())
    assert 0 < correct < B and int((target == 7).sum()) >= B // 3
    st = metrics_state(C)
    for rep in (1, 2):
        metrics_call(lib, loss, pred, target, B, C, st, 2 + rep, 1)
        mean = float(loss.double().mean())
        got = float(st["loss_out"])
        assert abs(got - mean) <= 1e-5 * mean and int(st["fin"]) == 1, (got, mean)
        assert st["acc"].tolist() == expected_acc(got, correct, B, rep), (st["acc"].tolist(), expected_acc(got, correct, B, rep))
        require(check_counts(st["counts"], pred, target, C, times=rep), "step_metrics")
    log = st["log"].tolist()
    frac = expected_acc(got, correct, B, 1)[2]
    assert log[3] == got and log[4] == got and log[8 + 3] == frac and log[8 + 4] == frac
    assert all(v != v for i, v in enumerate(log) if i not in (3, 4, 11, 12)), log
    # a non-finite loss row: the flag drops, nothing is accumulated
    bad = loss.clone()
    bad[B - 1] = float("nan")
    before = {k: v.clone() for k, v in st.items()}
    metrics_call(lib, bad, pred, target, B, C, st, 0, 1)
    assert int(st["fin"]) == 0 and float(st["loss_out"]) != float(st["loss_out"])
    require(check_bits(st["acc"], before["acc"], "accumulators") + check_bits(st["counts"], before["counts"], "counts"),
            "skipped step")


def test_step_metrics_three_call_sequence_of_the_data_parallel_path(lib):
    """Flag call (respect_skip = 2: loss, flag and log only), then the metrics-only accumulate call (loss_rows = NULL,
    respect_skip = 1 | 4: the loss is added exactly once); the same with the flag forced down in between (as the MIN over
    the ranks does when another rank's loss was not finite): nothing is accumulated."""
    B, C = 384, 1000
    loss, pred, target = metrics_inputs(B, C, 195)
    correct = int((pred.long() == target).sum())
    st = metrics_state(C)
    metrics_call(lib, loss, pred, target, B, C, st, 1, 2)
    got = float(st["loss_out"])
    assert abs(got - float(loss.double().mean())) <= 1e-5 * got and int(st["fin"]) == 1 and float(st["log"][1]) == got
    assert st["acc"].tolist() == [0.0] * 8 and not bool(st["counts"].any()), "the flag call accumulated"
    metrics_call(lib, None, pred, target, B, C, st, 1, 1 | 4)
    assert st["acc"].tolist() == expected_acc(got, correct, B, 1), st["acc"].tolist()
    require(check_counts(st["counts"], pred, target, C), "deferred accumulation")
    assert float(st["log"][8 + 1]) == expected_acc(got, correct, B, 1)[2] and float(st["loss_out"]) == got
    before = {k: v.clone() for k, v in st.items()}
    metrics_call(lib, loss * 2, pred, target, B, C, st, 2, 2)
    assert float(st["loss_out"]) != got and int(st["fin"]) == 1
    st["fin"].zero_()
    metrics_call(lib, None, pred, target, B, C, st, 2, 1 | 4)
    require(check_bits(st["acc"], before["acc"], "accumulators") + check_bits(st["counts"], before["counts"], "counts"),
            "flag forced down")
    # loss-only deferred form (pred = NULL): the loss alone, once
    st["fin"].fill_(1)
    metrics_call(lib, None, None, target, B, C, st, 2, 1 | 4)
    want = expected_acc(got, correct, B, 1)
    want[0] += float(st["loss_out"])
    want[1] += 1.0
    assert st["acc"].tolist() == want
    require(check_bits(st["counts"], before["counts"], "counts"), "loss-only deferred call")


# ======================================== 5. input packing ========================================
PACK_CASES = [("b256-plain", 256, 224, 0, None), ("b384-plain", 384, 224, 0, None), ("b256-mixup", 256, 224, 1, None),
              ("b256-cutmix", 256, 224, 2, (40, 150, 64, 200)), ("b256-cutmix-border", 256, 224, 2, (150, 224, 100, 224))]
PACK_CASES_RGB4 = PACK_CASES + [("b256-w223-cutmix-border", 256, 223, 2, (150, 224, 100, 223)), ("b256-w223-mixup", 256, 223, 1, None)]


def pack_check(got, ref, mode, what):
    """Modes 0 and 2 move fp32 pixels and round once: exact.  Mixup is `v * lam + o * (1 - lam)` in fp32 then one rounding;
    contracted into an fma it may differ from torch by one bf16 ulp on a few elements (test_pack_input_mixup_cutmix)."""
    if mode == 1:
        u, e = R.max_bf16_ulp(got, ref), R.rel_l2(got, ref)
        assert u <= 1.0 and e <= 1e-3, f"{what}: {u:.3g} bf16 ulp, rel L2 {e:.3g}"
    else:
        require(check_bits(got, ref, what), "pack")


@pytest.mark.parametrize("case", PACK_CASES, ids=[c[0] for c in PACK_CASES])
def test_pack_input(lib, case):
    hip = _harness.hip()
    _, B, W, mode, box = case
    H, lam = 224, 0.37
    x = randn((B, 3, H, W), 200 + B + mode)
    out = torch.full((B, H, W, 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_pack_input(x.data_ptr(), out.data_ptr(), B, 3, H, W, mode, lam, *(box or (0, 0, 0, 0)), hip.stream_ptr()),
       "pack_input")
    sync()
    ref = R.pack_input(x, mode, lam, box)
    assert ref.is_cuda
    if mode == 2:
        assert not torch.equal(ref, R.pack_input(x, 0)), "the box pasted nothing"
    got = out.float()
    pack_check(got[..., :3].contiguous(), ref[..., :3].contiguous(), mode, "pixels")
    assert not bool(out[..., 3:].contiguous().view(torch.int16).any()), "channels 3..7 are not exactly zero"


@pytest.mark.parametrize("case", PACK_CASES_RGB4, ids=[c[0] for c in PACK_CASES_RGB4])
def test_pack_input_rgb4(lib, case):
    hip = _harness.hip()
    _, B, W, mode, box = case
    H, lam = 224, 0.37
    We = W + (W & 1)
    x = randn((B, 3, H, W), 210 + B + mode + W)
    out = torch.full((B, H, We + 8, 4), float("nan"), dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_pack_input_rgb4(x.data_ptr(), out.data_ptr(), B, 3, H, W, mode, lam, *(box or (0, 0, 0, 0)), hip.stream_ptr()),
       "pack_input_rgb4")
    sync()
    ref = R.pack_input(x, mode, lam, box)[..., :3].contiguous()
    pack_check(out[:, :, 3:3 + W, :3].float().contiguous(), ref, mode, "pixels")
    bits = out.view(torch.int16)
    assert not bool(bits[..., 3].any()), "the zero channel"
    assert not bool(bits[:, :, :3].any()), "the 3 columns left of the image"
    assert bits[:, :, 3 + W:].shape[2] == (6 if W & 1 else 5) and not bool(bits[:, :, 3 + W:].any()), "the columns right of the image"


# ======================================== 6. filter preparation through the models' own tables ========================================
T_SENTINEL = -12345     # int16 bit pattern shadow_t is filled with: bf16 -6.7e9, no filter value


def seed_shadow(m, seed):
    m.shadow.copy_(randn(m.n_params, seed).to(torch.bfloat16))
    m.shadow_t.view(torch.int16).fill_(T_SENTINEL)


@pytest.mark.parametrize("model", MODELS)
def test_filter_transposes_of_the_models_own_tables(lib, models, model):
    m = models[model]
    descs = m._tr_descs.cpu().tolist()
    tiled = [d for d in descs if d[2] % 64 == 0 and d[4] % 64 == 0]
    # both kernels are really used: a routing change in the table builders must not hollow this case out
    assert m._tr_ntjobs > 0 and m._tr_ntjobs == sum(d[3] * (d[2] // 64) * (d[4] // 64) for d in tiled)
    njobs = getattr(m, "_tr_njobs", 0)
    assert (njobs > 0) == (len(tiled) < len(descs)) and (model != "convnext_t" or njobs > 0)
    assert len(descs) == {"resnet50": 53, "vit_b16": 49, "convnext_t": 40}[model]
    seed_shadow(m, 220 + MODELS.index(model))
    if model == "convnext_t":
        assert m.fused_ls
        m.train()
        m.param_arena.copy_(randn(m.n_params, 230, 0.05))
    before = m.shadow.clone()
    m.refresh_transposed()
    sync()
    require(check_transposed(m.shadow, m.shadow_t, descs, T_SENTINEL), f"{model} transposes")
    if model == "convnext_t":
        # fold, then transpose: fc2's transposed slot is the transpose of the FOLDED filter, not of what the shadow held
        blocks = [blk for st in m.stages for blk in st["blocks"]]
        for blk, cb in zip(blocks, m._ls_mode_cbs()):
            c = blk["fc2"]
            n = c.cout * c.cin
            old = before[c.w.offset:c.w.offset + n]
            new = m.shadow[c.w.offset:c.w.offset + n]
            assert not torch.equal(old, new), blk["name"]
            require(check_fold(new.view(c.cout, c.cin), fold_ref(m, blk, cb)[0], blk["name"]), "folded fc2 in front of the transpose")
            t = m.shadow_t[c.wt_offset:c.wt_offset + n].view(c.cin, c.cout)
            require(check_bits(t, new.view(c.cout, c.cin).t().contiguous(), blk["name"]), "transposed folded fc2")
    else:
        require(check_bits(m.shadow, before, "shadow"), f"{model}: refresh_transposed wrote the shadow")


def resnet_pairs(m):
    return m.conv_bn_pairs()


def test_resnet50_batchnorm_fold(lib, models):
    """ResNet.fold_batchnorm() on all 53 convolution + BatchNorm pairs: shadow_eval against bf16(w * gamma / sqrt(rv + eps))
    from fp64, eval_shift against fp64 beta - rm * scale.

    Bounds (new here; set from fp32-vs-fp64 arithmetic, not from the kernel's output).  The kernel forms the scale in fp32
    (a division and a square root: <= 2 roundings, ~1.2e-7 relative) and multiplies in fp32 (one more): the product is within
    ~2e-7 of the fp64 one, 2e-4 of half a bf16 step, so it can cross ONE rounding boundary and never two: <= 1 bf16 ulp
    (tests/test_fullsize_checkers_cpu.py: an fp32 scale passes, a neighbour's scale or 2 ulp in a tile do not), with rel L2
    <= 2e-3 in every 64 x 64 block, which ~1 element in 5000 crossing (3.9e-3 each) stays 30-fold under.  The shift is a
    difference of beta and rm * scale, each good to ~2e-7 relative in fp32: rtol 1e-5 of the result plus 1e-6 of the two
    magnitudes (5-fold margin on the absolute term; where the two cancel, rtol alone would ask for more than fp32 has).
    Measured on the MI355X over the 53 pairs: worst filter element 1 bf16 ulp (bound 1), worst shift error 0.043 of its
    bound; the test prints both."""
    m = models["resnet50"]
    pairs = resnet_pairs(m)
    assert len(pairs) == 53
    m.param_arena.copy_(randn(m.n_params, 240, 0.05))
    m.buffer_arena.copy_(urand(m.buffer_arena.numel(), 241, -0.1, 0.1))
    for i, (conv, bn) in enumerate(pairs):
        c = bn.c
        m.param_arena[bn.weight.offset:bn.weight.offset + c] = urand(c, 242 + i, 0.5, 1.5)
        m.param_arena[bn.bias.offset:bn.bias.offset + c] = urand(c, 342 + i, -0.2, 0.2)
        rv = urand(c, 442 + i, 0.5, 1.5)
        rv[i % 5::37] = 1e-6                   # channels whose variance is far below eps
        m.buffer_arena[bn.buf_offset + c:bn.buf_offset + 2 * c] = rv
    m.eval()
    m.fold_batchnorm()
    sync()
    from imageclassification_amd.nets import BN_EPS
    worst_ulp, worst_shift, K_max, C_max = 0.0, 0.0, 0, 0
    P = m.param_arena.double()
    for conv, bn in pairs:
        c, n = bn.c, conv.w.numel
        assert conv.cout_p == c
        K = n // c
        K_max, C_max = max(K, K_max), max(c, C_max)
        w = P[conv.w.offset:conv.w.offset + n].view(c, K)
        gamma, beta = P[bn.weight.offset:bn.weight.offset + c], P[bn.bias.offset:bn.bias.offset + c]
        rm = m.buffer_arena[bn.buf_offset:bn.buf_offset + c].double()
        rv = m.buffer_arena[bn.buf_offset + c:bn.buf_offset + 2 * c].double()
        scale = gamma / torch.sqrt(rv + BN_EPS)
        got = m.shadow_eval[conv.w.offset:conv.w.offset + n].view(c, K)
        ref = w * scale[:, None]
        worst_ulp = max(worst_ulp, R.max_bf16_ulp(got.float(), ref.to(torch.bfloat16).float()))
        require(check_fold(got, ref, bn.name), "BatchNorm fold")
        shift = m.eval_shift[bn.shift_offset:bn.shift_offset + c]
        rshift = beta - rm * scale
        bound = 1e-5 * rshift.abs() + 1e-6 * (beta.abs() + (rm * scale).abs())
        worst_shift = max(worst_shift, float(((shift.double() - rshift).abs() / bound).max()))
        require(check_close(shift, rshift, 1e-5, 1e-6 * (beta.abs() + (rm * scale).abs()), bn.name + " shift"), "BatchNorm fold")
    assert K_max == 4608 and C_max == 2048
    print(f"bn fold over 53 pairs: worst {worst_ulp:.3g} bf16 ulp (bound 1), worst shift error {worst_shift:.3g} of its bound")


def fold_ref(m, blk, cb):
    """fp64 cb * gamma[c] * W2[c, :] and cb * gamma[c] * b2[c] of one ConvNeXt block."""
    c = blk["fc2"]
    P = m.param_arena
    w = P[c.w.offset:c.w.offset + c.cout * c.cin].double().view(c.cout, c.cin)
    g = P[blk["gamma"].offset:blk["gamma"].offset + c.cout].double() * cb
    return w * g[:, None], P[c.b.offset:c.b.offset + c.cout].double() * g


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_convnext_layerscale_fold(lib, models, mode):
    """ConvNeXt._fold_layerscale(): 18 jobs in one launch (the kernel finds its job by a linear search over the first rows),
    K = 4C up to 3072, in training with a drop-path scale cb = 1 / (1 - rate) that differs per block, in eval with cb = 1.
    Same bounds as the BatchNorm fold (g = gamma * cb and g * w are two fp32 roundings); the bias is a pure product, so its
    absolute term is 1e-6 of its own magnitude.  Measured on the MI355X: worst filter element 1 bf16 ulp in training, 0 in
    eval (bound 1)."""
    m = models["convnext_t"]
    m.train(mode == "train")
    blocks = [blk for st in m.stages for blk in st["blocks"]]
    cbs = m._ls_mode_cbs()
    assert len(blocks) == 18 and max(b["fc2"].cin for b in blocks) == 3072
    assert len(set(cbs)) == (18 if mode == "train" else 1) and (mode == "train" or cbs[0] == 1.0)
    m.param_arena.copy_(randn(m.n_params, 250, 0.05))
    m.shadow.copy_(randn(m.n_params, 251).to(torch.bfloat16))
    m.fold_bias.fill_(float("nan"))
    before = m.shadow.clone()
    m._fold_layerscale()
    sync()
    assert m._ls_jobs.shape[0] == 18
    slot = torch.zeros(m.n_params, dtype=torch.bool, device=DEV)
    fb_slot = torch.zeros(m.fold_bias.numel(), dtype=torch.bool, device=DEV)
    worst = 0.0
    for blk, cb in zip(blocks, cbs):
        c = blk["fc2"]
        n = c.cout * c.cin
        rw, rb = fold_ref(m, blk, cb)
        got = m.shadow[c.w.offset:c.w.offset + n].view(c.cout, c.cin)
        worst = max(worst, R.max_bf16_ulp(got.float(), rw.to(torch.bfloat16).float()))
        require(check_fold(got, rw, blk["name"]), "layer-scale fold")
        require(check_close(m.fold_bias[blk["fb_off"]:blk["fb_off"] + c.cout], rb, 1e-5, 1e-6 * rb.abs(), blk["name"] + " bias"),
                "layer-scale fold")
        slot[c.w.offset:c.w.offset + n] = True
        fb_slot[blk["fb_off"]:blk["fb_off"] + c.cout] = True
    require(check_bits(m.shadow[~slot], before[~slot], "shadow outside the 18 fc2 slots"), "layer-scale fold")
    assert bool(torch.isnan(m.fold_bias[~fb_slot]).all()), "fold_bias written outside the blocks' slots"
    print(f"layer-scale fold ({mode}): worst {worst:.3g} bf16 ulp (bound 1)")
