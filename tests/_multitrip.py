"""Shared by tests/test_multitrip_gpu.py and tests/test_multitrip_checks_cpu.py: the cases at which the grid-capped loops of
csrc/window_attention.hip, csrc/se_ops.hip and csrc/conv_stem_deep.hip take more than one trip per workgroup, Python mirrors of
the launch planners (each names the C++ function it restates), the map from an output element to the trip that writes it, the
faults a multi-trip loop can have (applied to reference data, for the CPU test of the checks) and the derived bound on an fp32
summation chain.

Nothing here touches a GPU."""
import torch

# ---------------------------------------------------------------------------------------------------------------- cases
# (B, Hs, Ws, heads, ws, shift) -> (forward trips, backward trips)
WINATTN_CASES = {
    (45, 14, 21, 32, 7, 3): (2, 3),
    (20, 16, 16, 32, 4, 2): (2, 3),
    (9, 28, 28, 32, 7, 0): (1, 2),
}
# (N, H, W, C) -> (forward trips, backward trips)
PATCH_MERGE_CASES = {
    (9, 32, 34, 8): (1, 2),
    (34, 32, 32, 32): (2, 5),
    (5, 42, 42, 96): (1, 2),
    (3, 54, 54, 512): (1, 2),
}
# (N, HW, C, rd) -> (segments S, rows per segment, workgroups per sample of the elementwise passes, their trips)
SE_CASES = {
    (256, 289, 64, 8): (8, 37, 8, 2),
    (256, 289, 192, 12): (8, 37, 9, 4),
    (3, 9, 4096, 256): (1, 9, 18, 1),
}
# (N, H, W, Cout) -> (forward / data-gradient tile, tiles, weight-gradient tile, tiles, splits, tiles per split)
THIN_CASES = {
    (13, 111, 113, 32): (256, 637, 128, 1274, 255, 5),
    (7, 111, 113, 64): (128, 686, 128, 686, 229, 3),
}


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------- planners
WWAVES = 4          # windows (waves) per workgroup of the window-attention kernels


def winattn_nwin(B, Hs, Ws, ws):
    return B * (Hs // ws) * (Ws // ws)


def winattn_fwd_grid(nwin, H):
    """icamd_window_attention_fwd_launch (csrc/window_attention.hip): workgroups per head"""
    return min(cdiv(nwin, WWAVES), max(2048 // H, 1))


def winattn_bwd_grid(nwin, H):
    """icamd_window_attention_bwd_chunks (csrc/window_attention.hip): workgroups = dbias partials per head"""
    return min(cdiv(nwin, WWAVES), max(1024 // H, 1))


def winattn_trips(nwin, grid):
    """`iters` of winattn_fwd_kernel / winattn_bwd_kernel"""
    return cdiv(nwin, grid * WWAVES)


def winattn_window_trip(nwin, grid):
    """trip on which window wi is walked: wi = (it * grid + block) * 4 + wave"""
    return torch.arange(nwin) // (grid * WWAVES)


def winattn_token_window(B, Hs, Ws, ws, shift):
    """[B * Hs * Ws] -> window number (image, window row, window column) of each token row of the NATURAL order, by the rule of
    win_token (csrc/window_attention.hip): the token at (r, c) sits at ((r - shift) mod Hs, (c - shift) mod Ws) of the rolled grid"""
    r = (torch.arange(Hs) - shift) % Hs
    c = (torch.arange(Ws) - shift) % Ws
    w = (r // ws)[:, None] * (Ws // ws) + (c // ws)[None, :]
    nW = (Hs // ws) * (Ws // ws)
    return (torch.arange(B)[:, None, None] * nW + w[None]).reshape(-1)


def patch_merge_rows(N, H, W):
    return N * (H // 2) * (W // 2)


def patch_merge_fwd_grid(rows):
    """icamd_patch_merge_ln_fwd_launch (csrc/window_attention.hip)"""
    return min(cdiv(rows, 4), 2048)


def patch_merge_bwd_grid(rows):
    """icamd_patch_merge_ln_bwd_blocks (csrc/window_attention.hip)"""
    return min(cdiv(rows, 4), 512)


def patch_merge_trips(rows, grid):
    """trips of the row loop of patch_merge_ln_fwd_kernel / _bwd_kernel = rows of the busiest wave"""
    return cdiv(rows, 4 * grid)


def patch_merge_sum_depth(rows):
    """longest fp32 summation chain behind an element of dgamma / dbeta: rows of a wave, four waves, P partials"""
    P = patch_merge_bwd_grid(rows)
    return patch_merge_trips(rows, P) + 4 + P


def se_plan(N, HW):
    """icamd_se_plan (csrc/se_ops.hip): (segments per sample, rows per segment)"""
    s = max(min(cdiv(2048, N), cdiv(HW, 32)), 1)
    rps = cdiv(HW, s)
    return cdiv(HW, rps), rps


def se_blocks_per_sample(N, HW, cpr):
    """blocks_per_sample (csrc/se_ops.hip)"""
    import math
    blocks = max(min(cdiv(HW * cpr, 256), cdiv(2048, N)), 1)
    mult = cpr // math.gcd(cpr, 256)
    return cdiv(blocks, mult) * mult


def se_apply_trips(N, HW, cpr):
    """(trips of the vector loop of se_bn_apply_kernel / se_bwd_apply_kernel, 16 B vectors of the last trip)"""
    stride = se_blocks_per_sample(N, HW, cpr) * 256
    nvec = HW * cpr
    return cdiv(nvec, stride), nvec - (cdiv(nvec, stride) - 1) * stride


def se_jw(rd):
    """icamd_se_excite_fwd_launch (csrc/se_ops.hip): lanes that share a row of W2"""
    jw = 1
    while jw * 2 <= rd and jw * 2 <= 64:
        jw *= 2
    return jw


def _round16(v):
    return (v + 15) & ~15


def thin_plan_tile(W, in_row_bytes, out_row_bytes):
    """plan_tile (csrc/conv_stem_deep.hip): pixels per tile of the forward / data gradient"""
    for sb in (256, 128, 64):
        if sb == 256 and in_row_bytes + out_row_bytes > 128:
            continue
        lds = max(_round16(sb + 2 * W + 3) * in_row_bytes, sb * out_row_bytes, 16384)
        if lds <= 65536:
            return sb
    return 0


def thin_plan_wgrad(W, Cout):
    """plan_wgrad (csrc/conv_stem_deep.hip): pixels per tile of the weight gradient"""
    for sb in (128, 64, 32):
        if _round16(sb + 2 * W + 3) * 64 + sb * Cout * 2 <= 65536:
            return sb
    return 0


def thin_wgrad_split(M, sb):
    """wgrad_split (csrc/conv_stem_deep.hip): (splits, tiles per split, tiles)"""
    nt = cdiv(M, sb)
    want = max(min(256, nt), 1)
    tps = cdiv(nt, want)
    return cdiv(nt, tps), tps, nt


def thin_plan(N, H, W, Cout):
    """(forward tile, data-gradient tile, forward tiles, weight-gradient tile, tiles, splits, tiles per split)"""
    M = N * H * W
    sbf, sbd = thin_plan_tile(W, 64, Cout * 2), thin_plan_tile(W, Cout * 2, 64)
    sbw = thin_plan_wgrad(W, Cout)
    S, tps, nt = thin_wgrad_split(M, sbw)
    return sbf, sbd, cdiv(M, sbf), sbw, nt, S, tps


# ---------------------------------------------------------------------------------------------------------------- derived bound
def check_fp32_sum(got, ref, abs_sum, depth, what="sum"):
    """Every element of an fp32 sum against its fp64 value: |got - ref| <= depth * 2^-24 * sum |terms|, the worst case of a
    chain of `depth` fp32 additions (each adds a relative 2^-24 of a partial sum that never exceeds the sum of magnitudes)."""
    g, r = got.double().flatten(), ref.double().to(got.device).flatten()
    bound = depth * 2.0 ** -24 * abs_sum.double().to(got.device).flatten()
    bad = ~((g - r).abs() <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return [f"{what}: {int(bad.sum())} of {r.numel()} beyond {depth} * 2^-24 * sum|terms|, [{i}] {float(g[i]):.9g} vs "
                f"{float(r[i]):.9g} (bound {float(bound[i]):.3g})"]
    return []


def sum_error_in_bound_units(got, ref, abs_sum):
    """largest |got - ref| / (2^-24 * sum |terms|): the figure check_fp32_sum compares with `depth`"""
    g, r = got.double().flatten(), ref.double().to(got.device).flatten()
    return float(((g - r).abs() / (2.0 ** -24 * abs_sum.double().to(got.device).flatten()).clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------- faults
def se_later_trip_vectors(N_plan, HW, cpr):
    """bool [HW * cpr]: the 16 B vectors of one sample that the elementwise passes reach on their second and later trips"""
    stride = se_blocks_per_sample(N_plan, HW, cpr) * 256
    return torch.arange(HW * cpr) >= stride


def thin_tile_of_pixel(M, sb):
    return torch.arange(M) // sb
