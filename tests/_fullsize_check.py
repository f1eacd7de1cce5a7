"""Comparisons of the full-size layer and step tests (tests/test_fullsize_layers_gpu.py, tests/test_fullsize_step_gpu.py), kept apart so that
tests/test_fullsize_checkers_cpu.py can show on synthetic data that each of them rejects a subtly wrong output.

Every checker returns a list of failure messages (empty: accepted); `require` turns that into an assertion.
Outputs are 2-D: [rows, columns] for activations (pixels x channels, tokens x features), [co, k] for filters.
"""
import torch

from oracle import ops_ref as R

BLOCK = 64
BLOCK_REL_L2 = 2e-3
SAMPLE_STRIDE = 31


def require(failures, what):
    assert not failures, f"{what}: " + "; ".join(failures[:6])


def sample_rows(rows, rows_per_image, r=0, stride=SAMPLE_STRIDE, device=None):
    """Row indices of a sampled comparison: every row whose index is r (mod stride) -- a prime stride below 32 reaches
    every in-tile position of every power-of-two tile at least 32 rows high -- plus every row of the first, middle and
    last image (image borders and the ragged last tile)."""
    n_img = rows // rows_per_image
    idx = [torch.arange(r % stride, rows, stride)]
    for i in sorted({0, n_img // 2, n_img - 1}):
        idx.append(torch.arange(i * rows_per_image, (i + 1) * rows_per_image))
    return torch.unique(torch.cat(idx)).to(device)


def block_rel_l2(got, ref, row_ids=None, block=BLOCK):
    """rel L2 error of every (block x block) tile of a 2-D output.  row_ids: the original row index of each row of
    got / ref when they hold a sample of the rows (the tiles are those of the full output)."""
    got, ref = got.double(), ref.double()
    rows, cols = ref.shape
    if row_ids is None:
        row_ids = torch.arange(rows, device=ref.device)
    ncb = (cols + block - 1) // block
    pad = ncb * block - cols
    d2 = torch.nn.functional.pad((got - ref) ** 2, (0, pad)).reshape(rows, ncb, block).sum(-1)
    r2 = torch.nn.functional.pad(ref ** 2, (0, pad)).reshape(rows, ncb, block).sum(-1)
    tile = (row_ids.to(ref.device) // block).long()
    nrb = int(tile.max()) + 1
    D = torch.zeros(nrb, ncb, dtype=torch.float64, device=ref.device).index_add_(0, tile, d2)
    N = torch.zeros(nrb, ncb, dtype=torch.float64, device=ref.device).index_add_(0, tile, r2)
    present = torch.zeros(nrb, dtype=torch.bool, device=ref.device)
    present[tile] = True
    # a tile whose reference is exactly zero (masked gradients) must be exactly zero as well
    rel = torch.where(N > 0, torch.sqrt(D / N.clamp_min(1e-300)), torch.where(D > 0, float("inf"), 0.0))
    return rel, present


def worst_block(got, ref):
    """largest rel L2 error over the 64 x 64 blocks of an output (for the tests' printed figures)"""
    rel, present = block_rel_l2(got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1))
    return float(rel[present].max())


def _blocks(got, ref, row_ids, bound):
    rel, present = block_rel_l2(got, ref, row_ids)
    bad = ~(rel <= bound) & present[:, None]
    if bool(bad.any()):
        i, j = (int(v) for v in torch.nonzero(bad)[0])
        return [f"{int(bad.sum())} of {int(present.sum()) * rel.shape[1]} {BLOCK}x{BLOCK} blocks above rel_l2 {bound:g}, "
                f"first (row tile {i}, col tile {j}): {float(rel[i, j]):.3g}"]
    return []


def _rows(got, ref, rows):
    if rows is None:
        return got, ref, None
    rows = rows.to(ref.device)
    return got[rows], ref[rows], rows


def check_bf16(got, ref, rows=None, rel=1e-3, block_rel=BLOCK_REL_L2, ulps=2.0, atol_rms=2e-3, max_frac=0.0):
    """bf16 output against a reference with the same bf16 rounding points: global rel L2, elementwise bf16 closeness
    (R.bf16_close) and rel L2 in every 64 x 64 block.  rows: compare only these rows (sample_rows)."""
    g, r, ids = _rows(got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1), rows)
    out = []
    if not bool(torch.isfinite(g).all()):
        out.append("non-finite values")
    e = R.rel_l2(g, r)
    if not e <= rel:
        out.append(f"rel_l2 {e:.3g} > {rel:g}")
    if not R.bf16_close(g, r, ulps=ulps, atol_rms=atol_rms, max_frac=max_frac):
        out.append(f"elementwise bf16 bound (max_frac {max_frac:g})")
    return out + _blocks(g, r, ids, block_rel)


def check_fp32(got, ref, rows=None, rel=1e-4, block_rel=BLOCK_REL_L2):
    """fp32 output (weight gradients: [co, k]) against an fp64 reference: global and per-block rel L2."""
    g, r, ids = _rows(got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1), rows)
    out = []
    if not bool(torch.isfinite(g).all()):
        out.append("non-finite values")
    e = R.rel_l2(g, r)
    if not e <= rel:
        out.append(f"rel_l2 {e:.3g} > {rel:g}")
    return out + _blocks(g, r, ids, block_rel)


def check_stats(partials, y, weight=None, rtol=1e-5):
    """BatchNorm statistics partials [rows][2][C] (per-channel sum, sum of squares; or sum g, sum g*weight when weight
    is given) against fp64 sums of the stored output y [.., C]."""
    C = partials.shape[-1]
    p = partials.double().reshape(-1, 2, C).sum(0)
    yy = y.double().reshape(-1, C)
    second = yy * (yy if weight is None else weight.double().reshape(-1, C))
    ref = (yy.sum(0), second.sum(0))
    out = []
    for name, a, b in (("first", p[0], ref[0]), ("second", p[1], ref[1])):
        # the absolute term: rtol of the sum of magnitudes (a sum that cancels to ~0 is exact only to that)
        scale = (yy.abs() if name == "first" else second.abs()).sum(0)
        err = (a - b).abs()
        bad = ~(err <= rtol * b.abs() + 1e-7 * scale)
        if bool(bad.any()):
            c = int(torch.nonzero(bad)[0])
            out.append(f"{name} moment of {int(bad.sum())} channels off, channel {c}: {float(a[c]):.9g} vs {float(b[c]):.9g}")
    return out


def check_close(got, ref, rtol, atol=0.0, what="values"):
    """Small vectors (BatchNorm coefficients, LayerNorm row statistics, bias gradients)."""
    g, r = got.double().flatten(), ref.double().to(got.device).flatten()
    bad = ~((g - r).abs() <= rtol * r.abs() + _atol(atol, got.device))     # atol: a number, or one value per element
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return [f"{what}: {int(bad.sum())} of {r.numel()} off, [{i}] {float(g[i]):.9g} vs {float(r[i]):.9g}"]
    return []


# ---- comparisons of the full-size step tests (tests/test_fullsize_step_gpu.py): flat arenas, job tables, loss and metrics ----
def _atol(atol, device):
    return atol.double().to(device).flatten() if torch.is_tensor(atol) else atol


def check_arena(got, ref, rtol, atol, what="arena", chunk=1 << 24):
    """EVERY element of a flat arena within rtol * |ref| + atol of the reference, no outliers allowed (a NaN on either side
    counts as off).  Compared chunk by chunk, so that an 86 M-element arena needs no third fp64 copy."""
    g, r = got.flatten(), ref.flatten()
    if g.numel() != r.numel():
        return [f"{what}: {g.numel()} elements, reference has {r.numel()}"]
    nbad, first, last = 0, None, None
    for lo in range(0, r.numel(), chunk):
        gc, rc = g[lo:lo + chunk].double(), r[lo:lo + chunk].double().to(g.device)
        bad = ~((gc - rc).abs() <= rtol * rc.abs() + atol)
        k = int(bad.sum())
        if k:
            idx = torch.nonzero(bad).flatten()
            first = lo + int(idx[0]) if first is None else first
            last = lo + int(idx[-1])
            nbad += k
    if nbad:
        return [f"{what}: {nbad} of {r.numel()} off (rtol {rtol:g} atol {atol:g}), first [{first}] {float(g[first]):.9g} vs "
                f"{float(r[first]):.9g}, last [{last}]"]
    return []


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).flatten()


def check_bits(got, ref, what="values"):
    """Bit equality of two tensors of one dtype (-0 != +0, NaN payloads count)."""
    if got.dtype != ref.dtype or got.numel() != ref.numel():
        return [f"{what}: {got.dtype}[{got.numel()}] vs {ref.dtype}[{ref.numel()}]"]
    bad = _bits(got) != _bits(ref.to(got.device))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return [f"{what}: {int(bad.sum())} of {got.numel()} differ bitwise, first [{i}] {float(got.flatten()[i]):.9g} vs "
                f"{float(ref.flatten()[i]):.9g}"]
    return []


def check_transposed(shadow, shadow_t, descs, sentinel):
    """The models' transpose tables: for every desc row (src_off, dst_off, Cout, T, Cin, ...) the [Cin][T][Cout] slot of
    shadow_t is bit-equal to the transpose of the [Cout][T][Cin] slot of shadow; the slots do not overlap; every element of
    shadow_t outside all slots still holds `sentinel` (an int16 bit pattern shadow_t was filled with)."""
    s, t = _bits(shadow), _bits(shadow_t)
    out = []
    covered = torch.zeros(t.numel(), dtype=torch.bool, device=t.device)
    total = 0
    for i, (src, dst, co, taps, ci) in enumerate([tuple(int(v) for v in d[:5]) for d in descs]):
        n = co * taps * ci
        if src < 0 or dst < 0 or src + n > s.numel() or dst + n > t.numel():
            out.append(f"desc {i}: slot outside the arenas")
            continue
        want = s[src:src + n].view(co, taps, ci).permute(2, 1, 0)
        have = t[dst:dst + n].view(ci, taps, co)
        bad = have != want
        if bool(bad.any()):
            a, b, c = (int(v) for v in torch.nonzero(bad)[0])
            out.append(f"desc {i} ({co}x{taps}x{ci}): {int(bad.sum())} elements off, first (ci {a}, tap {b}, co {c})")
        covered[dst:dst + n] = True
        total += n
    if int(covered.sum()) != total:
        out.append("transposed slots overlap")
    stray = (t != sentinel) & ~covered
    if bool(stray.any()):
        out.append(f"{int(stray.sum())} elements outside every slot written, first [{int(torch.nonzero(stray)[0])}]")
    return out


def check_fold(got, ref64, what="folded filter", ulps=1.0, block_rel=BLOCK_REL_L2):
    """Folded bf16 filters [rows, K] against bf16(fp64 product): every element within `ulps` bf16 steps (the fp32 scale of
    the kernel can move a product across a rounding boundary, never further) and rel L2 of every 64 x 64 block."""
    r = ref64.to(torch.bfloat16).float()
    g = got.float().reshape(r.shape)
    out = []
    if not bool(torch.isfinite(g).all()):
        out.append(f"{what}: non-finite values")
    u = R.max_bf16_ulp(g, r)
    if not u <= ulps:
        out.append(f"{what}: {u:.3g} bf16 ulp > {ulps:g}")
    return out + [f"{what}: {m}" for m in _blocks(g, r, None, block_rel)]


def lowest_argmax(logits):
    """Index of the row maximum, the LOWEST one where it is tied -- written out, so that torch.argmax is not taken on trust."""
    x = logits.float()
    C = x.shape[1]
    idx = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, idx, C).min(1).values


def check_pred(pred, logits):
    want = lowest_argmax(logits)
    bad = pred.long().to(want.device) != want
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return [f"prediction of {int(bad.sum())} rows off, row {i}: {int(pred[i])} vs {int(want[i])}"]
    return []


def check_counts(counts, pred, target, C, times=1):
    """TP / FP / FN per class (int32 [3][C]) against torch.bincount of the predictions and targets, `times` steps of them."""
    p, t = pred.long().cpu(), target.long().cpu()
    hit = p == t
    want = torch.stack([torch.bincount(t[hit], minlength=C), torch.bincount(p[~hit], minlength=C),
                        torch.bincount(t[~hit], minlength=C)]) * times
    got = counts.long().cpu().reshape(3, C)
    out = []
    for k, name in enumerate(("TP", "FP", "FN")):
        bad = got[k] != want[k]
        if bool(bad.any()):
            c = int(torch.nonzero(bad)[0])
            out.append(f"{name}: {int(bad.sum())} classes off, class {c}: {int(got[k, c])} vs {int(want[k, c])}")
    return out
