"""The streaming kernels around the ResNet stem and at the end of the step, at the benchmark's sizes and at ragged ones:
max-pool backward folded into the stem's BatchNorm backward (LDS-staged gather), the stand-alone pooling kernels, the rgb4
input packing, the gradient norm and the FC bias gradient's column sums.

Bounds: everything that only moves data or adds in a stated order is compared with torch.equal; the rest keeps the bound of the
existing test of the same entry point (named at each place)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _harness
from _harness import rnd_bf16, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

DEV = "cuda"
gpu = pytest.mark.gpu

BENCH_STEM = (256, 112, 112, 64)
# windows cut by the border, odd sizes, one pixel, C = 128, W odd with H even, ranges of 32 rows per workgroup that start in
# the middle of an image row (40 x 13 x 9 pixels -> 32 rows per workgroup, 9 columns per image row), C/8 that does not divide
# 256, and widths whose pooled rows fit in LDS only two at a time (W = 300) or not at all (W = 700: gather from global memory)
RAGGED = [(3, 9, 7, 64), (5, 12, 10, 64), (1, 1, 1, 64), (2, 14, 14, 128), (2, 8, 11, 64), (40, 13, 9, 64), (2, 5, 6, 192),
          (1, 4, 300, 64), (1, 3, 700, 64)]
FOLD_SHAPES = [BENCH_STEM] + RAGGED
POOL_SHAPES = [BENCH_STEM] + RAGGED + [(1, 16, 16, 128)]


def pool_bwd_restated(dout, x):
    """What the pooling-backward kernels promise, restated: per full-resolution pixel, the covering windows (oh, ow) whose
    argmax (torch scan order, first maximum) it is, added in fp32 in (oh, ow) order, rounded to bf16 once.  NHWC in and out,
    on the device of its inputs."""
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _, idx = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)      # [N,C,OH,OW], flat h*W+w
    d = dout.float().permute(0, 3, 1, 2)
    hh, ww = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
    target = (hh[:, None] * W + ww[None, :]).to(idx.dtype)
    acc = torch.zeros(N, C, H, W, device=x.device)
    for a in (0, 1):            # window row h>>1, then (h+1)>>1 where that is another one
        oh = (hh >> 1) + a
        vh = (oh < OH) & ((hh & 1) == 1 if a else torch.ones_like(hh, dtype=torch.bool))
        for b in (0, 1):
            ow = (ww >> 1) + b
            vw = (ow < OW) & ((ww & 1) == 1 if b else torch.ones_like(ww, dtype=torch.bool))
            ohc, owc = oh.clamp_max(OH - 1), ow.clamp_max(OW - 1)
            hit = (idx[:, :, ohc][:, :, :, owc] == target) & (vh[:, None] & vw[None, :])
            acc += torch.where(hit, d[:, :, ohc][:, :, :, owc], torch.zeros((), device=x.device))
    return R.bf16_round(acc.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("shape", [(8,) + BENCH_STEM[1:]] + POOL_SHAPES[1:])
def test_restated_pool_backward_meets_the_oracle_bounds(shape):
    """No GPU: the restatement the GPU test compares with bit for bit is itself inside test_maxpool's bounds against the
    oracle, on every shape used (images are independent, so the benchmark geometry is checked at batch 8)."""
    N, H, W, C = shape
    x = rnd_bf16(N, H, W, C, seed=30).clamp_min(0)
    dout = rnd_bf16(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, seed=31)
    got, ref = pool_bwd_restated(dout, x), R.maxpool3x3s2_bwd(dout, x)
    u, e = R.max_bf16_ulp(got, ref), R.rel_l2(got, ref)
    print(f"{shape}: {u:.3g} bf16 ulp, rel L2 {e:.3g}")
    assert u <= 1.0 and e <= 1e-3


def side_wgrad(lib, hip):
    """A ring weight gradient to keep a second stream's MFMAs busy (test_partial_sum_kernels_bits_do_not_depend_on_a_second_stream)."""
    g = torch.Generator(device=DEV).manual_seed(7)
    d = hip.conv_desc(256, 28, 28, 192, 768, 1, 1, 1, 0)
    M = 256 * 28 * 28
    xa = torch.randn(M, 192, device=DEV, generator=g).bfloat16()
    dya = torch.randn(M, 768, device=DEV, generator=g).bfloat16()
    wgb = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    wgw = torch.empty(wgb, dtype=torch.uint8, device=DEV)
    dw, db = torch.empty(768, 192, device=DEV), torch.empty(768, device=DEV)
    side = torch.cuda.Stream()
    keep = (xa, dya, wgw, dw, db, d)

    def run():
        for _ in range(3):
            assert lib.icamd_conv2d_wgrad_bias(ctypes.byref(d), hip.ptr(xa), hip.ptr(dya), hip.ptr(dw), hip.ptr(db), 0, hip.ptr(wgw),
                                               wgb, side.cuda_stream) == 0
    return run, keep


@gpu
@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=str)
def test_folded_stem_backward_is_bit_identical(lib, shape):
    """icamd_bn_bwd_maxpool3x3s2 == icamd_maxpool3x3s2_bwd + icamd_bn_bwd: dy, dgamma, dbeta torch.equal, at the benchmark's
    stem shape and at ragged ones; the same bits twice in a row and next to a ring weight gradient on a second stream."""
    hip = _harness.hip()
    N, H, W, C = shape
    g = torch.Generator().manual_seed(130)
    y = rnd_bf16(N, H, W, C, seed=131, device=DEV).to(torch.bfloat16)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.3).to(DEV)
    yf = y.float().reshape(-1, C)
    mean = yf.mean(0).contiguous()
    invstd = (1.0 / torch.sqrt(yf.var(0, unbiased=False) + 1e-5)).contiguous()
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    del yf
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    s = hip.stream_ptr()
    pooled = torch.empty(N, OH, OW, C, dtype=torch.bfloat16, device=DEV)
    idx = torch.empty(N, OH, OW, C, dtype=torch.uint8, device=DEV)
    assert lib.icamd_bn_relu_maxpool3x3s2_fwd(hip.ptr(y), hip.ptr(scale), hip.ptr(shift), hip.ptr(pooled), hip.ptr(idx), N, H, W, C,
                                              s) == 0
    dout = rnd_bf16(N, OH, OW, C, seed=132, device=DEV).to(torch.bfloat16)
    rows = N * H * W
    wsb = lib.icamd_bn_bwd_workspace_bytes(rows, C)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    da, dy1 = torch.empty_like(y), torch.empty_like(y)
    dg1, db1 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    assert lib.icamd_maxpool3x3s2_bwd(hip.ptr(dout), hip.ptr(idx), hip.ptr(da), N, H, W, C, s) == 0
    assert lib.icamd_bn_bwd(hip.ptr(da), None, hip.ptr(y), hip.ptr(mean), hip.ptr(invstd), hip.ptr(scale), hip.ptr(shift),
                            hip.ptr(dg1), hip.ptr(db1), hip.ptr(dy1), None, None, rows, C, 1, 0, hip.ptr(ws), wsb, s) == 0
    sync()
    assert bool(dg1.abs().sum() > 0) or rows == 1
    side, keep = side_wgrad(lib, hip)
    for with_side in (False, False, True):
        dy2 = torch.full_like(y, float("nan"))
        dg2, db2 = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        if with_side:
            side()
        assert lib.icamd_bn_bwd_maxpool3x3s2(hip.ptr(dout), hip.ptr(idx), hip.ptr(y), hip.ptr(mean), hip.ptr(invstd),
                                             hip.ptr(scale), hip.ptr(shift), hip.ptr(dg2), hip.ptr(db2), hip.ptr(dy2), N, H, W, C, 0,
                                             hip.ptr(ws), wsb, s) == 0
        sync()
        assert torch.equal(dy1.view(torch.int16), dy2.view(torch.int16)), with_side
        assert torch.equal(dg1, dg2) and torch.equal(db1, db2), with_side
    # accumulate = 1 adds to what is there, like the two-call route
    dg3, db3 = dg1.clone(), db1.clone()
    assert lib.icamd_bn_bwd(hip.ptr(da), None, hip.ptr(y), hip.ptr(mean), hip.ptr(invstd), hip.ptr(scale), hip.ptr(shift),
                            hip.ptr(dg3), hip.ptr(db3), hip.ptr(dy1), None, None, rows, C, 1, 1, hip.ptr(ws), wsb, s) == 0
    dg4, db4 = dg1.clone(), db1.clone()
    assert lib.icamd_bn_bwd_maxpool3x3s2(hip.ptr(dout), hip.ptr(idx), hip.ptr(y), hip.ptr(mean), hip.ptr(invstd), hip.ptr(scale),
                                         hip.ptr(shift), hip.ptr(dg4), hip.ptr(db4), hip.ptr(dy2), N, H, W, C, 1, hip.ptr(ws), wsb,
                                         s) == 0
    sync()
    assert torch.equal(dg3, dg4) and torch.equal(db3, db4)


@gpu
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=str)
def test_maxpool_forward_and_backward(lib, shape):
    """Forward value and argmax torch.equal to the oracle (as test_maxpool); backward torch.equal to the restatement above
    and inside test_maxpool's bounds (<= 1 bf16 ulp, rel-L2 <= 1e-3) against oracle.ops_ref.maxpool3x3s2_bwd."""
    hip = _harness.hip()
    N, H, W, C = shape
    big = N * H * W * C > 1 << 24
    dev = DEV if big else "cpu"          # the references of the benchmark-size case are computed on the GPU by torch
    x = rnd_bf16(N, H, W, C, seed=30, device=dev).clamp_min(0)     # post-ReLU input: many exact ties at zero
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = x.to(torch.bfloat16).to(DEV).contiguous()
    out = torch.empty(N, OH, OW, C, dtype=torch.bfloat16, device=DEV)
    idx = torch.empty(N, OH, OW, C, dtype=torch.uint8, device=DEV)
    assert lib.icamd_maxpool3x3s2_fwd(hip.ptr(xd), hip.ptr(out), hip.ptr(idx), N, H, W, C, hip.stream_ptr()) == 0
    sync()
    ref, ridx = R.maxpool3x3s2_fwd(x)
    assert torch.equal(out.float().to(dev), ref)
    # the kernel records the position in the window (r * 3 + s); the oracle the flat index in the input plane
    code = idx.to(dev).long().permute(0, 3, 1, 2)
    oh, ow = torch.arange(OH, device=dev)[:, None], torch.arange(OW, device=dev)[None, :]
    flat = (oh * 2 - 1 + code // 3) * W + (ow * 2 - 1 + code % 3)
    assert torch.equal(flat, ridx)
    dout = rnd_bf16(N, OH, OW, C, seed=31, device=dev)
    doutd = dout.to(torch.bfloat16).to(DEV).contiguous()
    dx = torch.full_like(xd, float("nan"))
    assert lib.icamd_maxpool3x3s2_bwd(hip.ptr(doutd), hip.ptr(idx), hip.ptr(dx), N, H, W, C, hip.stream_ptr()) == 0
    sync()
    got = dx.float().to(dev)
    assert torch.equal(got, pool_bwd_restated(dout, x))
    rdx = R.maxpool3x3s2_bwd(dout, x)
    u, e = R.max_bf16_ulp(got, rdx), R.rel_l2(got, rdx)
    print(f"{shape}: {u:.3g} bf16 ulp, rel L2 {e:.3g}")
    assert u <= 1.0 and e <= 1e-3


PACK_CASES = [  # B, H, W, mode, box
    (256, 224, 224, 0, None), (256, 224, 224, 1, None), (256, 224, 224, 2, (40, 180, 30, 201)),
    (3, 10, 13, 0, None), (3, 10, 13, 1, None), (3, 10, 13, 2, (2, 7, 0, 13)),     # odd width, box over the full width
    (5, 7, 12, 2, (0, 7, 3, 9)), (2, 5, 20, 1, None), (2, 3, 8, 0, None), (1, 1, 1, 0, None),
    (7, 9, 230, 2, (1, 8, 225, 230)),                                               # W % 4 != 0: the scalar-load route
]


@gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=str)
def test_pack_input_rgb4(lib, case):
    """[B][H][W + (W & 1) + 8][4] torch.equal to oracle.ops_ref.pack_input in every mode: modes 0 and 2 move fp32 pixels and round
    once, and the mixup is two rounded products and a rounded sum, as torch's (the kernel forbids their contraction).  Everything
    outside the image is exactly zero.  Also from a source that is only 4 B aligned (a view one float into a buffer)."""
    hip = _harness.hip()
    B, H, W, mode, box = case
    lam = 0.37
    We = W + (W & 1)
    for shift in (0, 1):
        buf = torch.randn(B * 3 * H * W + 4, generator=torch.Generator(device=DEV).manual_seed(210 + B + mode + W), device=DEV)
        x = buf[shift:shift + B * 3 * H * W].view(B, 3, H, W)
        out = torch.full((B, H, We + 8, 4), float("nan"), dtype=torch.bfloat16, device=DEV)
        assert lib.icamd_pack_input_rgb4(x.data_ptr(), out.data_ptr(), B, 3, H, W, mode, lam, *(box or (0, 0, 0, 0)),
                                         hip.stream_ptr()) == 0
        sync()
        ref = R.pack_input(x, mode, lam, box)[..., :3].contiguous()
        got = out[:, :, 3:3 + W, :3].float().contiguous()
        if mode == 2:
            assert not torch.equal(ref, R.pack_input(x, 0)[..., :3]) or B == 1, "the box pasted nothing"
        assert torch.equal(got, ref)
        bits = out.view(torch.int16)
        assert not bool(bits[..., 3].any()), "the zero channel"
        assert not bool(bits[:, :, :3].any()) and not bool(bits[:, :, 3 + W:].any()), "the columns beside the image"


@gpu
@pytest.mark.parametrize("n", [25557032 + 53120, 25557035, 1001, 7, 512 * 256 * 4 * 4 + 2, 3], ids=str)
def test_grad_norm(lib, n):
    """icamd_grad_norm against fp64 numpy of the same fp32 data to test_fullsize_step_gpu.py::test_grad_norm's bound (1e-5
    relative), for n % 4 != 0, n smaller than the grid, n about ResNet-50's arena; two calls give the same bits."""
    hip = _harness.hip()
    g = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(140), device=DEV)
    g = g * 10.0 ** torch.linspace(-4.0, 2.0, n, device=DEV)
    ref = float(np.sqrt((g.cpu().numpy().astype(np.float64) ** 2).sum()))
    ws = torch.empty(lib.icamd_grad_norm_workspace_bytes(), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((2,), float("nan"), device=DEV)
        assert lib.icamd_grad_norm(g.data_ptr(), n, 1.0, 0.5 * ref, ws.data_ptr(), out.data_ptr(), hip.stream_ptr()) == 0
        sync()
        outs.append(out)
    got, coef = outs[0].tolist()
    print(f"n {n}: norm {got:.9g} vs {ref:.9g}, coef {coef:.9g}")
    assert abs(got - ref) <= 1e-5 * ref
    assert abs(coef - min(1.0, 0.5 * ref / (ref + 1e-6))) <= 1e-5
    assert torch.equal(outs[0], outs[1])


@gpu
@pytest.mark.parametrize("case", [(256, 1024, 1024), (1, 1024, 1024), (37, 24, 20), (256, 1008, 1000), (100, 77, 45), (65, 33, 33),
                                  (64, 32, 32), (300, 40, 1)], ids=str)
def test_colsum(lib, case):
    """icamd_colsum as the FC bias gradient calls it (rows 256, ld = cols = 1024) and at ragged sizes: torch.equal to the fp32
    sum taken in row order (the kernel keeps that order), and test_colsum_lerp_cast's bound against torch's own sum."""
    hip = _harness.hip()
    rows, ld, cols = case
    x = rnd_bf16(rows, ld, seed=70)
    xd = x.to(torch.bfloat16).to(DEV).contiguous()
    inorder = torch.zeros(cols)
    for r in range(rows):
        inorder += x[r, :cols]
    for accumulate in (0, 1):
        out = torch.full((cols + 3,), 1.5, device=DEV)
        assert lib.icamd_colsum(hip.ptr(xd), rows, ld, cols, hip.ptr(out), accumulate, hip.stream_ptr()) == 0
        sync()
        got = out.cpu()
        assert torch.equal(got[cols:], torch.full((3,), 1.5)), "wrote past the last column"
        assert torch.equal(got[:cols], 1.5 + inorder if accumulate else inorder)
        assert torch.allclose(got[:cols], 1.5 * accumulate + x[:, :cols].sum(0), rtol=1e-5, atol=1e-5)
