"""Comparisons of the full-size layer tests (tests/test_fullsize_layers_gpu.py), kept apart so that
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
    bad = ~((g - r).abs() <= rtol * r.abs() + atol)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return [f"{what}: {int(bad.sum())} of {r.numel()} off, [{i}] {float(g[i]):.9g} vs {float(r[i]):.9g}"]
    return []
