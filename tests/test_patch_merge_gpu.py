"""icamd_patch_merge_ln_fwd / _bwd (csrc/window_attention.hip) through the C ABI: the 2x2 gather into 4C channels (timm's
x0 | x1 | x2 | x3 order) fused with LayerNorm(4C), against tests/_swin_ref.py patch_merge_ln_ref in fp64.  Bounds are those of
tests/test_kernels_gpu.py test_layernorm_fwd_bwd; outputs carry guard bands as in the long-attention tests."""
import hashlib
import os
import sys

import pytest
import torch

from oracle import ops_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _swin_ref import patch_merge_ln_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
BAND = 64
SENT16 = 0x5A5B
ICAMD_ERR_UNSUPPORTED = 2
# (N, H, W, C): two vectors per lane at most / odd vector count per block / 4C = 1536 (three per lane) / 4C = 2048 (the limit)
SHAPES = [(2, 4, 4, 96), (3, 6, 10, 32), (2, 14, 14, 384), (1, 8, 8, 512)]


@pytest.fixture(scope="module")
def lib():
    from imageclassification_amd import hip
    hip.require_gpu()
    return hip.load()


def _hip():
    from imageclassification_amd import hip
    return hip


def rnd_bf16(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return R.bf16_round(torch.randn(*shape, generator=g) * scale)


def guarded_bf16(numel, fill):
    whole = torch.full((numel + BAND * 64,), SENT16, dtype=torch.int16, device=DEV)
    view = whole[:numel].view(torch.bfloat16)
    view.fill_(fill)
    return view, whole


def operands(N, H, W, C):
    g = torch.Generator().manual_seed(100)
    x = R.bf16_round(rnd_bf16(N, H, W, C, scale=2.0, seed=101) + 0.5)
    gamma = torch.rand(4 * C, generator=g) + 0.5
    beta = torch.randn(4 * C, generator=g) * 0.2
    dy = rnd_bf16(N * (H // 2) * (W // 2), 4 * C, seed=102)
    return x, gamma, beta, dy


def run(lib, N, H, W, C, accs=(0,)):
    hip = _hip()
    x, gamma, beta, dy = operands(N, H, W, C)
    rows = N * (H // 2) * (W // 2)
    xd, gd, bd, dyd = x.to(torch.bfloat16).to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(torch.bfloat16).to(DEV)
    nan = float("nan")
    y, y_w = guarded_bf16(rows * 4 * C, nan)
    mean, rstd = torch.full((rows,), nan, device=DEV), torch.full((rows,), nan, device=DEV)
    rc_f = lib.icamd_patch_merge_ln_fwd(hip.ptr(xd), hip.ptr(gd), hip.ptr(bd), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), N, H, W, C,
                                        EPS, hip.stream_ptr())
    wsb = max(int(lib.icamd_patch_merge_ln_bwd_workspace_bytes(N, H, W, C)), 256)
    wsp = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dx, dx_w = guarded_bf16(N * H * W * C, nan)
    dg, db = torch.ones(4 * C, device=DEV), torch.ones(4 * C, device=DEV)
    grads = []
    rc_b = 0
    for acc in accs:
        rc_b = lib.icamd_patch_merge_ln_bwd(hip.ptr(dyd), hip.ptr(xd), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gd), hip.ptr(dx),
                                            hip.ptr(dg), hip.ptr(db), N, H, W, C, acc, hip.ptr(wsp), wsb, hip.stream_ptr())
        torch.cuda.synchronize()
        grads.append((dg.cpu().clone(), db.cpu().clone()))
    assert bool((y_w[rows * 4 * C:] == SENT16).all()), "guard band behind y written"
    assert bool((dx_w[N * H * W * C:] == SENT16).all()), "guard band behind dx written"
    return rc_f, rc_b, y, mean, rstd, dx, grads


@pytest.mark.parametrize("N,H,W,C", SHAPES)
def test_patch_merge_ln_fwd_bwd(lib, N, H, W, C):
    x, gamma, beta, dy = operands(N, H, W, C)
    ry, rmean, rrstd, rdx, rdg, rdb = patch_merge_ln_ref(x, gamma, beta, EPS, dy=dy)
    rc_f, rc_b, y, mean, rstd, dx, grads = run(lib, N, H, W, C, accs=(0, 1))
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    gy, gdx = y.float().cpu(), dx.float().cpu()
    ry, rdx = R.bf16_round(ry.float()).flatten(), R.bf16_round(rdx.float()).flatten()
    print(f"{(N, H, W, C)}: y rel_l2 {R.rel_l2(gy, ry):.3g}, dx rel_l2 {R.rel_l2(gdx, rdx):.3g}, "
          f"dgamma {R.rel_l2(grads[0][0], rdg):.3g}, dbeta {R.rel_l2(grads[0][1], rdb):.3g}")
    assert torch.allclose(mean.cpu(), rmean.float(), rtol=1e-5, atol=1e-6) and torch.allclose(rstd.cpu(), rrstd.float(), rtol=1e-5)
    assert R.rel_l2(gy, ry) <= 1e-3 and R.bf16_close(gy, ry)
    assert R.rel_l2(gdx, rdx) <= 1e-3 and R.bf16_close(gdx, rdx)
    for acc, (dg, db) in enumerate(grads):      # the second call accumulates onto the first call's result
        assert R.rel_l2(dg, (1 + acc) * rdg) <= 1e-4 and R.rel_l2(db, (1 + acc) * rdb) <= 1e-4, acc


@pytest.mark.parametrize("C", [516, 520])     # 520: a multiple of 8, so only the 4C <= 2048 limit refuses it
def test_too_wide_rows_are_refused_and_write_nothing(lib, C):
    rc_f, rc_b, y, mean, rstd, dx, grads = run(lib, 1, 4, 4, C)
    assert rc_f == ICAMD_ERR_UNSUPPORTED and rc_b == ICAMD_ERR_UNSUPPORTED
    for t in (y, mean, rstd, dx):
        assert bool(torch.isnan(t.float()).all()), "a refused call wrote to an output"
    assert torch.equal(grads[0][0], torch.ones(4 * C)) and torch.equal(grads[0][1], torch.ones(4 * C))


def test_patch_merge_ln_is_bitwise_reproducible(lib):
    def once():
        rc_f, rc_b, y, mean, rstd, dx, grads = run(lib, 2, 14, 14, 384)
        assert rc_f == 0 and rc_b == 0
        h = hashlib.sha256()
        for t in (y, mean, rstd, dx, grads[0][0], grads[0][1]):
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        return h.hexdigest()

    assert once() == once()
