"""icamd_bn_apply_relu6 and icamd_bn_bwd_relu6 (csrc/dwconv3x3.hip).

Apply: equal to bf16(clamp(fma(y, scale, shift), 0, 6)) computed by torch on the same operands.
Backward: against fp64 autograd of batch_norm(y) fed dout * mask, with the caps of tests/test_kernels_gpu.py::test_bn_train_apply_and_bwd.
The mask is the forward's own fp32 expression, 0 < fma(y, scale, shift) < 6 -- as that test takes the recomputed ReLU mask from the
kernel's own activation -- so an element whose pre-activation sits at a clamp boundary in fp32 is masked as the forward clamped it;
the share of elements where fp64 autograd of relu6(batch_norm(y)) would mask otherwise is printed and held below 0.1 %.

Loops whose trip count depends on the problem: rows of a block per row lane (r += rlanes): (6498, 96) 2 trips of 21 lanes, (50, 1344)
32 of 1; LDS outputs (o += 256 over 16 tcols): (394, 144) 2, (50, 1344) 11; row lanes per output: 85 at C = 24; blocks = partial rows
folded by the finalize kernel: 204 at 6498 rows."""
import pytest
import torch
import torch.nn.functional as F

import _harness
from _harness import DEV, dev, digest, guarded, intact, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(98, 24), (394, 144), (6498, 96), (50, 1344)]
EPS = 1e-5


def operands(rows, C):
    g = torch.Generator().manual_seed(300 + C)
    y = R.bf16_round(torch.randn(rows, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g))
    dout = R.bf16_round(torch.randn(rows, C, generator=g))
    gamma = 3.0 + 2.0 * torch.rand(C, generator=g)
    beta = 0.5 + 0.5 * torch.randn(C, generator=g)
    yd = y.double()
    mean = yd.mean(0)
    invstd = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + EPS)
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * scale.double()).float()
    return y, dout, gamma, beta, mean.float(), invstd.float(), scale, shift


@pytest.mark.parametrize("rows,C", SHAPES)
def test_bn_apply_relu6(lib, rows, C):
    hip = _harness.hip()
    y, _, _, _, _, _, scale, shift = operands(rows, C)
    ref = R.bn_relu6(y, scale, shift)
    at6, at0 = float((ref == 6).float().mean()), float((ref == 0).float().mean())
    print(f"({rows}, {C}): {at6:.1%} at 6, {at0:.1%} at 0")
    assert at6 >= 0.02 and at0 >= 0.20
    yd, scd, shd = dev(y), scale.to(DEV), shift.to(DEV)
    out, go = guarded((rows, C), torch.bfloat16)
    assert lib.icamd_bn_apply_relu6(hip.ptr(yd), hip.ptr(scd), hip.ptr(shd), hip.ptr(out), rows * C, C, hip.stream_ptr()) == 0
    assert intact(go)
    assert torch.equal(out.float().cpu(), ref)
    # refusals: a width that is no multiple of 8, a count that is no multiple of the width
    keep = out.clone()
    assert lib.icamd_bn_apply_relu6(hip.ptr(yd), hip.ptr(scd), hip.ptr(shd), hip.ptr(out), rows * C, 20, hip.stream_ptr()) != 0
    assert lib.icamd_bn_apply_relu6(hip.ptr(yd), hip.ptr(scd), hip.ptr(shd), hip.ptr(out), rows * C - 8, C, hip.stream_ptr()) != 0
    sync()
    assert torch.equal(out, keep)


@pytest.mark.parametrize("rows,C", SHAPES)
def test_bn_bwd_relu6(lib, rows, C):
    hip = _harness.hip()
    y, dout, gamma, beta, mean, invstd, scale, shift = operands(rows, C)
    z32 = R.fma32(y, scale, shift)
    mask = (z32 > 0) & (z32 < 6)
    at6, at0 = float((z32 >= 6).float().mean()), float((z32 <= 0).float().mean())
    assert at6 >= 0.02 and at0 >= 0.20
    # fp64 autograd of the BatchNorm behind the forward's mask
    yt = y.double().requires_grad_(True)
    gt, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    o = F.batch_norm(yt, None, None, gt, bt, True, 0.0, EPS)
    o.backward(dout.double() * mask)
    rdy, rdg, rdb = R.bf16_round(yt.grad), gt.grad, bt.grad
    # ... which is autograd of relu6(batch_norm(y)) but for the boundary elements
    yt2 = y.double().requires_grad_(True)
    o2 = F.hardtanh(F.batch_norm(yt2, None, None, gamma.double(), beta.double(), True, 0.0, EPS), 0.0, 6.0)
    o2.backward(dout.double())
    mask64 = (o2.detach() > 0) & (o2.detach() < 6)
    differ = float((mask64 != mask).float().mean())
    print(f"({rows}, {C}): fp32 and fp64 masks differ on {differ:.3%} of the elements")
    assert differ <= 1e-3

    yd, dd = dev(y), dev(dout)
    md, isd, scd, shd = mean.to(DEV), invstd.to(DEV), scale.to(DEV), shift.to(DEV)
    wsb = lib.icamd_bn_bwd_relu6_workspace_bytes(rows, C)
    assert wsb == lib.icamd_bn_bwd_workspace_bytes(rows, C) > 0
    ws, gws = guarded((wsb,), torch.uint8, fill=0)           # arrival counters start at zero
    seen = []
    for acc, base in ((0, 0.0), (1, 1.5), (0, 0.0)):
        dy, gdy = guarded((rows, C), torch.bfloat16)
        dg, gdg = guarded((C,), torch.float32, fill=base if acc else float("nan"))
        db, gdb = guarded((C,), torch.float32, fill=base if acc else float("nan"))
        assert lib.icamd_bn_bwd_relu6(hip.ptr(dd), hip.ptr(yd), hip.ptr(md), hip.ptr(isd), hip.ptr(scd), hip.ptr(shd), hip.ptr(dg),
                                      hip.ptr(db), hip.ptr(dy), rows, C, acc, hip.ptr(ws), wsb, hip.stream_ptr()) == 0
        assert intact(gdy) and intact(gdg) and intact(gdb) and intact(gws)
        got = dy.float().cpu()
        print(f"({rows}, {C}) acc={acc}: dy rel_l2 {R.rel_l2(got, rdy):.2e}, dgamma {R.rel_l2(dg.cpu(), base + rdg):.2e}, "
              f"dbeta {R.rel_l2(db.cpu(), base + rdb):.2e}")
        assert R.rel_l2(got, rdy) <= 1e-3 and R.bf16_close(got, rdy)
        assert R.rel_l2(dg.cpu(), base + rdg) <= 1e-4 and R.rel_l2(db.cpu(), base + rdb) <= 1e-4
        if not acc:
            seen.append(digest(dy, dg, db))
    assert seen[0] == seen[1]                                 # two launches: the same bits
    # refusals, with nothing written
    dy, _ = guarded((rows, C), torch.bfloat16, fill=3.0)
    dg = torch.full((C,), 3.0, device=DEV)
    args = (hip.ptr(dd), hip.ptr(yd), hip.ptr(md), hip.ptr(isd), hip.ptr(scd), hip.ptr(shd), hip.ptr(dg), hip.ptr(dg), hip.ptr(dy))
    assert lib.icamd_bn_bwd_relu6(*args, rows, C, 0, hip.ptr(ws), wsb - 1, hip.stream_ptr()) == 3
    assert lib.icamd_bn_bwd_relu6(*args, rows, 20, 0, hip.ptr(ws), wsb, hip.stream_ptr()) == 1
    sync()
    assert bool((dy.float() == 3.0).all()) and bool((dg == 3.0).all())


def test_existing_batchnorm_entries_unchanged_around_the_new_calls(lib):
    """icamd_bn_apply / icamd_bn_bwd (relu 1, mask recomputed) give the same bits before and after the ReLU6 entries ran in this process"""
    hip = _harness.hip()
    rows, C = 394, 144
    y, dout, gamma, beta, mean, invstd, scale, shift = operands(rows, C)
    yd, dd = dev(y), dev(dout)
    md, isd, scd, shd = mean.to(DEV), invstd.to(DEV), scale.to(DEV), shift.to(DEV)
    wsb = lib.icamd_bn_bwd_workspace_bytes(rows, C)

    def existing():
        out = torch.empty_like(yd)
        dy = torch.empty_like(yd)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        assert lib.icamd_bn_apply(hip.ptr(yd), hip.ptr(scd), hip.ptr(shd), None, hip.ptr(out), None, rows * C, C, 1, hip.stream_ptr()) == 0
        assert lib.icamd_bn_bwd(hip.ptr(dd), None, hip.ptr(yd), hip.ptr(md), hip.ptr(isd), hip.ptr(scd), hip.ptr(shd), hip.ptr(dg),
                                hip.ptr(db), hip.ptr(dy), None, None, rows, C, 1, 0, hip.ptr(ws), wsb, hip.stream_ptr()) == 0
        sync()
        return digest(out, dy, dg, db)

    before = existing()
    out6 = torch.empty_like(yd)
    dy6 = torch.empty_like(yd)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_apply_relu6(hip.ptr(yd), hip.ptr(scd), hip.ptr(shd), hip.ptr(out6), rows * C, C, hip.stream_ptr()) == 0
    assert lib.icamd_bn_bwd_relu6(hip.ptr(dd), hip.ptr(yd), hip.ptr(md), hip.ptr(isd), hip.ptr(scd), hip.ptr(shd), hip.ptr(dg), hip.ptr(db),
                                  hip.ptr(dy6), rows, C, 0, hip.ptr(ws), wsb, hip.stream_ptr()) == 0
    sync()
    assert existing() == before
    # and the ReLU6 apply differs from the ReLU apply exactly where it clamps at 6
    relu = torch.empty_like(yd)
    assert lib.icamd_bn_apply(hip.ptr(yd), hip.ptr(scd), hip.ptr(shd), None, hip.ptr(relu), None, rows * C, C, 1, hip.stream_ptr()) == 0
    sync()
    assert torch.equal(out6.float(), relu.float().clamp_max(6.0))
