"""icamd_patch_merge_ln_fwd / _bwd (csrc/window_attention.hip) through the C ABI: the 2x2 gather into 4C channels (timm's
x0 | x1 | x2 | x3 order) fused with LayerNorm(4C), against oracle/swin_ref.py patch_merge_ln_ref in fp64.  Bounds are those of
tests/test_kernels_gpu.py test_layernorm_fwd_bwd; outputs carry guard bands as in the long-attention tests."""
import pytest
import torch

from _harness import UNSUPPORTED, digest
from _harness import lib  # noqa: F401
from _patch_merge import EPS, operands, run
from oracle.swin_ref import patch_merge_ln_ref
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

# (N, H, W, C): two vectors per lane at most / odd vector count per block / 4C = 1536 (three per lane) / 4C = 2048 (the limit)
SHAPES = [(2, 4, 4, 96), (3, 6, 10, 32), (2, 14, 14, 384), (1, 8, 8, 512)]


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
    assert rc_f == UNSUPPORTED and rc_b == UNSUPPORTED
    for t in (y, mean, rstd, dx):
        assert bool(torch.isnan(t.float()).all()), "a refused call wrote to an output"
    assert torch.equal(grads[0][0], torch.ones(4 * C)) and torch.equal(grads[0][1], torch.ones(4 * C))


def test_patch_merge_ln_is_bitwise_reproducible(lib):
    def once():
        rc_f, rc_b, y, mean, rstd, dx, grads = run(lib, 2, 14, 14, 384)
        assert rc_f == 0 and rc_b == 0
        return digest(y, mean, rstd, dx, grads[0][0], grads[0][1])

    assert once() == once()
