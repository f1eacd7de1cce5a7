"""Element-wise parity of the C-ABI entries at the benchmark's own layer shapes (ResNet-50 train at batch 256 and eval at
batch 384, ViT-B/16 and ConvNeXt-T at batch 256), with default routing.

tests/test_kernels_gpu.py compares every entry with the oracle on small problems; at the benchmark's sizes the routing
(size floors, the weight-gradient and fused-backward planners, the XCD-chunked workgroup orders), the persistent loops
(attention over 3072 heads, the 8-phase GEMM tile walk) and the multi-chunk BatchNorm reduce take forms the small cases
never reach.  Here each case launches the entry the model launches for one layer, on seeded bf16 inputs made on the GPU,
and compares the WHOLE output (attention: a subset of images, see there) with oracle/ops_ref.py's formula -- same bf16
rounding points as the kernel -- accumulated in fp64 on the GPU.  Bounds are those test_kernels_gpu.py applies to the
same entry, plus rel L2 <= 2e-3 in every 64 x 64 block (tests/_fullsize_check.py), which one wrong tile cannot pass.
"""
import ctypes

import pytest
import torch

import _harness
from _fullsize_check import check_bf16, check_close, check_fp32, check_stats, require
from _harness import default_routing_lib as lib  # noqa: F401
from _harness import free_after_each  # noqa: F401
from _harness import rnd_dev as rnd
from _harness import sync
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64

# ResNet-50 convolutions (Cin, Cout, k, stride, Hin); the 7x7 stem runs on its own entries (resnet50_stem)
RESNET_CONVS = [
    (64, 64, 1, 1, 56), (64, 64, 3, 1, 56), (64, 256, 1, 1, 56), (256, 64, 1, 1, 56), (256, 128, 1, 1, 56),
    (128, 128, 3, 2, 56), (256, 512, 1, 2, 56), (128, 512, 1, 1, 28), (512, 128, 1, 1, 28), (128, 128, 3, 1, 28),
    (512, 256, 1, 1, 28), (256, 256, 3, 2, 28), (512, 1024, 1, 2, 28), (256, 1024, 1, 1, 14), (1024, 256, 1, 1, 14),
    (256, 256, 3, 1, 14), (1024, 512, 1, 1, 14), (512, 512, 3, 2, 14), (1024, 2048, 1, 2, 14), (512, 2048, 1, 1, 7),
    (2048, 512, 1, 1, 7), (512, 512, 3, 1, 7),
]
TRAIN_N, EVAL_N = 256, 384
VIT_B, VIT_T, VIT_H, VIT_D, VIT_DIM = 256, 197, 12, 64, 768
VIT_M = VIT_B * VIT_T                         # 50 432 token rows
CNX_N = 256
CNX_STAGES = [(96, 56), (192, 28), (384, 14), (768, 7)]


def urand(n, seed, lo, hi):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(n, generator=g, device=DEV) * (hi - lo) + lo


def ok(rc, what):
    assert rc == 0, f"{what}: rc {rc}"


def f2(t):
    """2-D view [rows, last dim] in fp32."""
    return t.float().reshape(-1, t.shape[-1])


def pack_bits(mask):
    return (mask.reshape(-1, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8, device=mask.device)).sum(1).to(torch.uint8)


def wgrad_ws(lib, d):
    n = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    return torch.empty(n, dtype=torch.uint8, device=DEV), n


# ============================================ ResNet-50, train, batch 256 ============================================
def _conv_id(c):
    cin, cout, k, st, h = c
    return f"{cin}to{cout}-{k}x{k}s{st}-{h}"


def resnet_conv_fwd_bn(lib, c, seed):
    """icamd_conv2d_fwd with statistics, then the BatchNorm that follows it: icamd_bn_train_finalize (multi-chunk reduce
    wherever M > 65 536), icamd_bn_apply (+ residual on the expansion convs, mask bits), icamd_bn_bwd."""
    hip = _harness.hip()
    cin, cout, k, st, h = c
    pad = k // 2
    N = TRAIN_N
    d = hip.conv_desc(N, h, h, cin, cout, k, k, st, pad)
    x = rnd((N, h, h, cin), seed, relu=True)
    w = rnd((cout, k, k, cin), seed + 1, scale=(2.0 / (k * k * cin)) ** 0.5)
    y = torch.empty(N, d.OH, d.OW, cout, dtype=torch.bfloat16, device=DEV)
    rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
    stats = torch.full((rows, 2, cout), float("nan"), device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None, stats.data_ptr(), s), "fwd")
    sync()
    ref = R.conv2d_fwd(x, w, st, pad, acc=F64)
    require(check_bf16(f2(y), f2(ref)), "conv fwd")
    require(check_stats(stats, y), "conv fwd statistics")
    del ref, x
    # BatchNorm over the stored output
    M = y.numel() // cout
    gamma, beta = urand(cout, seed + 2, 0.5, 1.5), urand(cout, seed + 3, -0.2, 0.2)
    rm0, rv0 = urand(cout, seed + 4, -0.1, 0.1), urand(cout, seed + 5, 0.5, 1.5)
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, scale, shift = (torch.empty(cout, device=DEV) for _ in range(4))
    ws = torch.zeros(lib.icamd_bn_workspace_bytes(cout), dtype=torch.uint8, device=DEV)
    ok(lib.icamd_bn_train_finalize(stats.data_ptr(), rows, cout, float(M), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                   rv.data_ptr(), 0.1, 1e-5, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(),
                                   shift.data_ptr(), ws.data_ptr(), s), "bn finalize")
    sync()
    rmean, rinv, rscale, rshift, rrm, rrv = R.bn_train_coeffs(y, gamma, beta, rm0, rv0, 0.1, 1e-5)
    require(check_close(mean, rmean, 1e-5, 1e-6, "mean") + check_close(invstd, rinv, 1e-5, 0, "invstd")
            + check_close(scale, rscale, 1e-5, 0, "scale") + check_close(shift, rshift, 1e-4, 1e-6, "shift")
            + check_close(rm, rrm, 1e-5, 1e-7, "running mean") + check_close(rv, rrv, 1e-5, 0, "running var"), "bn finalize")
    residual = rnd(y.shape, seed + 6, relu=True) if cout == 4 * cin or cout == 2 * cin and st == 2 else None
    out = torch.empty_like(y)
    bits = torch.empty(y.numel() // 8, dtype=torch.uint8, device=DEV)
    ok(lib.icamd_bn_apply(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), hip.ptr(residual), out.data_ptr(), bits.data_ptr(),
                          y.numel(), cout, 1, s), "bn apply")
    sync()
    require(check_bf16(f2(out), f2(R.bn_apply(y, scale, shift, residual, relu=True, acc=F64))), "bn apply")
    assert torch.equal(bits, pack_bits(out.reshape(-1) > 0)), "bn apply mask bits"
    del residual
    dout = rnd(y.shape, seed + 7)
    wsb = lib.icamd_bn_bwd_workspace_bytes(M, cout)
    bws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    dgam, dbet = torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV)
    dy, gout = torch.empty_like(y), torch.empty_like(y)
    ok(lib.icamd_bn_bwd(dout.data_ptr(), out.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(),
                        shift.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dy.data_ptr(), gout.data_ptr(), None, M, cout, 1, 0,
                        bws.data_ptr(), wsb, s), "bn bwd")
    sync()
    rdy, rdg, rdb, rg = R.bn_bwd(dout, out, y, mean, invstd, scale, relu=True, acc=F64)
    require(check_bf16(f2(dy), f2(rdy)), "bn bwd dy")
    assert torch.equal(gout.float(), rg), "bn bwd masked gradient"
    assert R.rel_l2(dgam, rdg) <= 1e-4 and R.rel_l2(dbet, rdb) <= 1e-4, "bn bwd dgamma / dbeta"


def resnet_conv_dgrad(lib, c, seed):
    """icamd_conv2d_dgrad plain, with a bf16 addend, and (1x1 stride-1 layers) with the mask-bit addend."""
    hip = _harness.hip()
    cin, cout, k, st, h = c
    pad = k // 2
    N = TRAIN_N
    d = hip.conv_desc(N, h, h, cin, cout, k, k, st, pad)
    dy = rnd((N, d.OH, d.OW, cout), seed)
    w = rnd((cout, k, k, cin), seed + 1, scale=(1.0 / (k * k * cout)) ** 0.5)
    w_t = w.permute(3, 1, 2, 0).contiguous()
    dx = torch.empty(N, h, h, cin, dtype=torch.bfloat16, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), None, None, s), "dgrad")
    sync()
    base = R.conv2d_dgrad(dy, w, (h, h), st, pad, acc=F64)   # fp64 accumulate; the addend forms add onto the unrounded sum
    require(check_bf16(f2(dx), f2(base)), "dgrad")
    del base
    addend = rnd((N, h, h, cin), seed + 2)
    ok(lib.icamd_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), addend.data_ptr(), None, s), "dgrad+a")
    sync()
    require(check_bf16(f2(dx), f2(R.conv2d_dgrad(dy, w, (h, h), st, pad, addend, acc=F64))), "dgrad + addend")
    if k == 1 and st == 1 and cin % 64 == 0:
        g = torch.Generator(device=DEV).manual_seed(seed + 3)
        mask = torch.rand(N, h, h, cin, generator=g, device=DEV) > 0.4
        bits = pack_bits(mask)
        ok(lib.icamd_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), addend.data_ptr(),
                                  bits.data_ptr(), s), "dgrad+bits")
        sync()
        require(check_bf16(f2(dx), f2(R.conv2d_dgrad(dy, w, (h, h), st, pad, addend * mask, acc=F64))), "dgrad + mask-bit addend")


def resnet_conv_wgrad(lib, c, seed):
    """icamd_conv2d_wgrad (planner-chosen kernel, split and workgroup order at the real grid) and its bias form."""
    hip = _harness.hip()
    cin, cout, k, st, h = c
    pad = k // 2
    N = TRAIN_N
    d = hip.conv_desc(N, h, h, cin, cout, k, k, st, pad)
    x = rnd((N, h, h, cin), seed, relu=True)
    dy = rnd((N, d.OH, d.OW, cout), seed + 1)
    ws, wsb = wgrad_ws(lib, d)
    dw = torch.full((cout, k, k, cin), float("nan"), device=DEV)
    ok(lib.icamd_conv2d_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), wsb,
                              hip.stream_ptr()), "wgrad")
    sync()
    ref = R.conv2d_wgrad(x, dy, (k, k), st, pad, acc=F64)
    require(check_fp32(dw.reshape(cout, -1), ref.reshape(cout, -1)), "wgrad")
    db = torch.full((cout,), float("nan"), device=DEV)
    dw.fill_(float("nan"))
    ok(lib.icamd_conv2d_wgrad_bias(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(),
                                   wsb, hip.stream_ptr()), "wgrad_bias")
    sync()
    require(check_fp32(dw.reshape(cout, -1), ref.reshape(cout, -1)), "wgrad (bias form)")
    bref = dy.double().reshape(-1, cout).sum(0)
    require(check_close(db, bref, 1e-4, 1e-3 * (float(bref.abs().max()) + 1), "bias gradient"), "wgrad (bias form)")


def resnet_stem(lib, seed):
    """The 7x7 / stride-2 stem on the rgb4 layout: forward with statistics, and the weight gradient."""
    hip = _harness.hip()
    N, H, Cout = TRAIN_N, 224, 64
    x = rnd((N, 3, H, H), seed).float()
    w = rnd((Cout, 7, 7, 3), seed + 1, scale=(1.0 / 147) ** 0.5).float()
    OH = 112
    x4 = torch.empty(N, H, H + 8, 4, dtype=torch.bfloat16, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_pack_input_rgb4(x.data_ptr(), x4.data_ptr(), N, 3, H, H, 0, 1.0, 0, 0, 0, 0, s), "pack")
    wp = torch.zeros(Cout, 8, 8, 4, device=DEV)
    wp[:, :7, :7, :3] = w
    wd = wp.to(torch.bfloat16)
    y = torch.empty(N, OH, OH, Cout, dtype=torch.bfloat16, device=DEV)
    rows = lib.icamd_stem7x7s2_stats_rows(N, H, H)
    stats = torch.full((rows, 2, Cout), float("nan"), device=DEV)
    ok(lib.icamd_stem7x7s2_fwd(x4.data_ptr(), wd.data_ptr(), y.data_ptr(), None, stats.data_ptr(), 0, N, H, H, Cout, s), "stem fwd")
    sync()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous()
    del x
    require(check_bf16(f2(y), f2(R.conv2d_fwd(x_nhwc, w, 2, 3, acc=F64))), "stem fwd")
    require(check_stats(stats, y), "stem statistics")
    dy = rnd((N, OH, OH, Cout), seed + 2)
    wsb = lib.icamd_stem7x7s2_wgrad_workspace_bytes(N, H, H, Cout)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw = torch.full((Cout, 8, 8, 4), 5.0, device=DEV)
    ok(lib.icamd_stem7x7s2_wgrad(x4.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), wsb, N, H, H, Cout, s), "stem wgrad")
    sync()
    rw = R.conv2d_wgrad(x_nhwc, dy, (7, 7), 2, 3, acc=F64)
    require(check_fp32(dw[:, :7, :7, :3].reshape(Cout, -1), rw.reshape(Cout, -1)), "stem wgrad")
    padv = dw.clone()
    padv[:, :7, :7, :3] = 0
    assert float(padv.abs().max()) == 0.0, "stem wgrad padding entries"


def resnet_bn_apply_conv1x1_fused(lib, c, seed, res_bn):
    """icamd_bn_apply_conv1x1_fused at a layer1 / layer2 shape: out = relu(bn3(y3) + shortcut) with mask bits, y1 = conv1(out)
    of the next block with its statistics."""
    hip = _harness.hip()
    N, h, K, Nout = c
    d = hip.conv_desc(N, h, h, K, Nout, 1, 1, 1, 0)
    assert lib.icamd_bn_apply_conv1x1_fused_supported(ctypes.byref(d)) == 1
    M = N * h * h
    y = rnd((N, h, h, K), seed, scale=1.3)
    res = rnd((N, h, h, K), seed + 1, relu=not res_bn)
    scale, shift = urand(K, seed + 2, 0.5, 1.5), urand(K, seed + 3, -0.5, 0.5)
    rsc, rsh = urand(K, seed + 4, 0.5, 1.5), urand(K, seed + 5, -0.5, 0.5)
    w = rnd((Nout, 1, 1, K), seed + 6, scale=(2.0 / K) ** 0.5)
    rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
    out = torch.empty(N, h, h, K, dtype=torch.bfloat16, device=DEV)
    bits = torch.full((M * K // 8,), 0xAA, dtype=torch.uint8, device=DEV)
    y1 = torch.empty(N, h, h, Nout, dtype=torch.bfloat16, device=DEV)
    stats = torch.full((rows, 2, Nout), float("nan"), device=DEV)
    ok(lib.icamd_bn_apply_conv1x1_fused(ctypes.byref(d), y.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(),
                                        rsc.data_ptr() if res_bn else None, rsh.data_ptr() if res_bn else None, out.data_ptr(),
                                        bits.data_ptr(), w.data_ptr(), y1.data_ptr(), stats.data_ptr(), hip.stream_ptr()), "fused")
    sync()
    # the shortcut's BatchNorm is rounded to bf16 before the add (R.bn_apply's residual operand), as in the kernels
    residual = R.bn_apply(res, rsc, rsh, None, relu=False, acc=F64) if res_bn else res
    out_ref = R.bn_apply(y, scale, shift, residual, relu=True, acc=F64)
    require(check_bf16(f2(out), f2(out_ref)), "bn apply (fused)")
    assert torch.equal(bits, pack_bits(out.reshape(-1) > 0)), "mask bits (fused)"
    del out_ref, residual
    # conv1 is computed on the activation the kernel itself stored
    require(check_bf16(f2(y1), f2(R.conv2d_fwd(out, w, 1, 0, acc=F64))), "conv1 (fused)")
    require(check_stats(stats, y1), "conv1 statistics (fused)")


def _gy_partials(g, y, C):
    """[ceil(M/128)][2][C] = (sum g, sum g*y) per 128 rows, fp64 summed, as icamd_conv2d_dgrad_bnred leaves them."""
    M = g.numel() // C
    rows = (M + 127) // 128
    pad = rows * 128 - M
    g2 = torch.nn.functional.pad(g.double().reshape(-1, C), (0, 0, 0, pad)).reshape(rows, 128, C)
    y2 = torch.nn.functional.pad(y.double().reshape(-1, C), (0, 0, 0, pad)).reshape(rows, 128, C)
    return torch.stack([g2.sum(1), (g2 * y2).sum(1)], 1).float().contiguous(), rows


def _bn_coeffs(y, C, gamma):
    yy = y.double().reshape(-1, C)
    mean, var = yy.mean(0), yy.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    return mean.float(), invstd.float(), (gamma * invstd.float()).contiguous()


def resnet_conv1x1_bn_bwd_fused(lib, c, seed):
    """icamd_conv1x1_bn_bwd_fused (conv3 + bn3 backward of a bottleneck) at a layer1 / layer2 shape."""
    hip = _harness.hip()
    N, h, Cin, Cout = c
    d = hip.conv_desc(N, h, h, Cin, Cout, 1, 1, 1, 0)
    assert lib.icamd_conv1x1_bn_bwd_fused_supported(ctypes.byref(d)) == 1
    gen = torch.Generator(device=DEV).manual_seed(seed)
    g = rnd((N, h, h, Cout), seed + 1) * (torch.rand(N, h, h, Cout, generator=gen, device=DEV) > 0.45)
    y = rnd((N, h, h, Cout), seed + 2, scale=1.5, shift=0.3)
    x = rnd((N, h, h, Cin), seed + 3, relu=True)
    w = rnd((Cout, 1, 1, Cin), seed + 4, scale=(1.0 / Cin) ** 0.5)
    w_t = w.permute(3, 1, 2, 0).contiguous()
    mean, invstd, scale = _bn_coeffs(y, Cout, urand(Cout, seed + 5, 0.5, 1.5))
    part, rows = _gy_partials(g, y, Cout)
    s = hip.stream_ptr()
    bwsb = lib.icamd_bn_bwd_apply_workspace_bytes(Cout)
    bws = torch.zeros(bwsb, dtype=torch.uint8, device=DEV)
    wsb = lib.icamd_conv1x1_bn_bwd_fused_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dx = torch.empty(N, h, h, Cin, dtype=torch.bfloat16, device=DEV)
    dw = torch.full((Cout, Cin), float("nan"), device=DEV)
    dgam, dbet = torch.full((Cout,), float("nan"), device=DEV), torch.full((Cout,), float("nan"), device=DEV)
    ok(lib.icamd_conv1x1_bn_bwd_fused(ctypes.byref(d), part.data_ptr(), rows, g.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                      invstd.data_ptr(), scale.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), x.data_ptr(),
                                      w_t.data_ptr(), dx.data_ptr(), dw.data_ptr(), 0, bws.data_ptr(), bwsb, ws.data_ptr(), wsb, s),
       "fused bwd")
    sync()
    rdy, rdg, rdb, _ = R.bn_bwd(g, torch.ones_like(g), y, mean, invstd, scale, acc=F64)
    # dy is formed in fp32 and rounded to bf16 inside the kernel; where that rounding lands on the other side of a bf16
    # boundary than the fp64 reference's, the whole row of dx moves by one dy ulp times the filter -- above the elementwise
    # bound where dx cancels.  dx has 51 M (layer1) / 26 M (layer2) elements: the > 1e7-element rule of
    # test_kernels_gpu.py (the 600-head attention case) applies.  rel L2 and every 64 x 64 block keep their bounds.  Measured on
    # the MI355X: 3 of 51.4 M (layer1) and 2 of 25.7 M (layer2) elements outside the elementwise bound (allowed: 51 / 25).
    require(check_bf16(f2(dx), f2(R.conv2d_dgrad(rdy, w, (h, h), 1, 0, acc=F64)), max_frac=1e-6), "dx (fused)")
    # dw: the bound test_kernels_gpu.py applies to this entry -- dy is formed and rounded inside the kernel, so a few of its
    # bf16 roundings differ from the fp64 reference's
    require(check_fp32(dw, R.conv2d_wgrad(x, rdy, (1, 1), 1, 0, acc=F64).reshape(Cout, Cin), rel=1e-3), "dw (fused)")
    assert R.rel_l2(dgam, rdg) <= 1e-4 and R.rel_l2(dbet, rdb) <= 1e-4, "dgamma / dbeta (fused)"


def resnet_dgrad_bnred(lib, c, seed):
    """icamd_conv2d_dgrad_bnred (conv1 residual data gradient + the sums of the previous block's last BatchNorm backward),
    then icamd_bn_bwd_from_gy_partials on those sums."""
    hip = _harness.hip()
    N, h, Cin, Cout = c
    d = hip.conv_desc(N, h, h, Cin, Cout, 1, 1, 1, 0)
    assert lib.icamd_conv2d_dgrad_bnred_supported(ctypes.byref(d)) == 1
    M = N * h * h
    gen = torch.Generator(device=DEV).manual_seed(seed)
    dy = rnd((N, h, h, Cout), seed + 1)
    w = rnd((Cout, 1, 1, Cin), seed + 2, scale=(1.0 / Cout) ** 0.5)
    w_t = w.permute(3, 1, 2, 0).contiguous()
    addend = rnd((N, h, h, Cin), seed + 3)
    y = rnd((N, h, h, Cin), seed + 4, scale=1.5, shift=0.3)
    amask = torch.rand(N, h, h, Cin, generator=gen, device=DEV) > 0.4
    pmask = torch.rand(N, h, h, Cin, generator=gen, device=DEV) > 0.45
    abits, pbits = pack_bits(amask), pack_bits(pmask)     # held: a freed temporary's block would be handed to the next one
    rows = lib.icamd_conv2d_dgrad_stats_rows(ctypes.byref(d))
    part = torch.full((rows, 2, Cin), float("nan"), device=DEV)
    g = torch.empty(N, h, h, Cin, dtype=torch.bfloat16, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_conv2d_dgrad_bnred(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), g.data_ptr(), addend.data_ptr(),
                                    abits.data_ptr(), 0, y.data_ptr(), pbits.data_ptr(), part.data_ptr(), s),
       "dgrad_bnred")
    sync()
    g_ref = R.conv2d_dgrad(dy, w, (h, h), 1, 0, addend * amask, acc=F64) * pmask
    require(check_bf16(f2(g), f2(g_ref)), "g (dgrad_bnred)")
    del g_ref
    require(check_stats(part, g, weight=y), "(sum g, sum g*y) partials")
    mean, invstd, scale = _bn_coeffs(y, Cin, urand(Cin, seed + 5, 0.5, 1.5))
    dgam, dbet = torch.zeros(Cin, device=DEV), torch.zeros(Cin, device=DEV)
    dyo = torch.empty_like(g)
    wsb = lib.icamd_bn_bwd_apply_workspace_bytes(Cin)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    ok(lib.icamd_bn_bwd_from_gy_partials(part.data_ptr(), rows, g.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                         scale.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dyo.data_ptr(), M, Cin, 0,
                                         ws.data_ptr(), wsb, s), "bn_bwd_from_gy_partials")
    sync()
    rdy, rdg, rdb, _ = R.bn_bwd(g, torch.ones_like(g), y, mean, invstd, scale, acc=F64)
    require(check_bf16(f2(dyo), f2(rdy)), "BatchNorm backward from the partials")
    assert R.rel_l2(dgam, rdg) <= 1e-4 and R.rel_l2(dbet, rdb) <= 1e-4, "dgamma / dbeta"


def _bn_fake_coeffs(C, seed):
    """BatchNorm (mean, invstd, scale, shift) of a layer, as contiguous device vectors."""
    return (urand(C, seed, -0.1, 0.1), urand(C, seed + 1, 0.5, 1.5), urand(C, seed + 2, 0.5, 1.5), urand(C, seed + 3, -0.3, 0.3))


def resnet_stem_bn_pool(lib, seed):
    """The stem's tail: icamd_bn_relu_maxpool3x3s2_fwd on the 256 x 112 x 112 x 64 conv output, then the backward through
    the pool and the BatchNorm, both as nets.py runs them (icamd_maxpool3x3s2_bwd + icamd_bn_bwd) and folded
    (icamd_bn_bwd_maxpool3x3s2)."""
    hip = _harness.hip()
    N, H, C = TRAIN_N, 112, 64
    OH = 56
    y = rnd((N, H, H, C), seed, scale=1.5)
    mean, invstd, scale, shift = _bn_fake_coeffs(C, seed + 1)
    pooled = torch.empty(N, OH, OH, C, dtype=torch.bfloat16, device=DEV)
    idx = torch.empty(N, OH, OH, C, dtype=torch.uint8, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_bn_relu_maxpool3x3s2_fwd(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), pooled.data_ptr(), idx.data_ptr(), N, H, H,
                                          C, s), "bn relu maxpool")
    act_k = torch.empty_like(y)
    ok(lib.icamd_bn_apply(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, act_k.data_ptr(), None, y.numel(), C, 1, s), "bn apply")
    sync()
    act = R.bn_apply(y, scale, shift, None, relu=True, acc=F64)
    require(check_bf16(f2(act_k), f2(act)), "bn + relu")
    # the pool is a max of bf16 values: exact, on the activation the device rounds (fp32 fma) -- which also decides the
    # window position a tie or a one-ulp rounding difference routes the gradient to
    pref, _ = R.maxpool3x3s2_fwd(act_k)
    assert torch.equal(pooled.float(), pref), "bn + relu + max-pool"
    act = act_k
    dout = rnd((N, OH, OH, C), seed + 5)
    da = torch.empty(N, H, H, C, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_maxpool3x3s2_bwd(dout.data_ptr(), idx.data_ptr(), da.data_ptr(), N, H, H, C, s), "maxpool bwd")
    sync()
    # the recorded window position is the first maximum in scan order, as torch's: ties (zeros after the ReLU) route alike
    da_ref = R.bf16_round(R.maxpool3x3s2_bwd(dout, act, acc=F64))
    require(check_bf16(f2(da), f2(da_ref)), "max-pool backward")
    M = N * H * H
    wsb = lib.icamd_bn_bwd_workspace_bytes(M, C)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    rdy, rdg, rdb, _ = R.bn_bwd(da_ref, act, y, mean, invstd, scale, relu=True, acc=F64)
    for folded in (False, True):
        dy = torch.empty_like(y)
        dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        if folded:
            ok(lib.icamd_bn_bwd_maxpool3x3s2(dout.data_ptr(), idx.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                             scale.data_ptr(), shift.data_ptr(), dg.data_ptr(), db.data_ptr(), dy.data_ptr(), N, H, H, C,
                                             0, ws.data_ptr(), wsb, s), "bn bwd + maxpool")
        else:
            ok(lib.icamd_bn_bwd(da.data_ptr(), None, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                dg.data_ptr(), db.data_ptr(), dy.data_ptr(), None, None, M, C, 1, 0, ws.data_ptr(), wsb, s), "bn bwd")
        sync()
        what = "BatchNorm backward through the pool" + (" (folded)" if folded else "")
        require(check_bf16(f2(dy), f2(rdy)), what)
        assert R.rel_l2(dg, rdg) <= 1e-4 and R.rel_l2(db, rdb) <= 1e-4, what + ": dgamma / dbeta"


def resnet_bn_apply_res_bn(lib, c, seed):
    """icamd_bn_apply_res_bn: the block output of a projection block, relu(bn3(y3) + bn_d(y_d)), with its mask bits."""
    hip = _harness.hip()
    N, h, C = c
    y, yd = rnd((N, h, h, C), seed, scale=1.3), rnd((N, h, h, C), seed + 1, scale=1.3)
    sc, sh = urand(C, seed + 2, 0.5, 1.5), urand(C, seed + 3, -0.3, 0.3)
    scd, shd = urand(C, seed + 4, 0.5, 1.5), urand(C, seed + 5, -0.3, 0.3)
    out = torch.empty_like(y)
    bits = torch.empty(y.numel() // 8, dtype=torch.uint8, device=DEV)
    ok(lib.icamd_bn_apply_res_bn(y.data_ptr(), sc.data_ptr(), sh.data_ptr(), yd.data_ptr(), scd.data_ptr(), shd.data_ptr(), out.data_ptr(),
                                 bits.data_ptr(), y.numel(), C, 1, hip.stream_ptr()), "bn_apply_res_bn")
    sync()
    # the shortcut's BatchNorm is rounded to bf16 before the add (bit-identical to icamd_bn_apply twice)
    ref = R.bn_apply(y, sc, sh, R.bn_apply(yd, scd, shd, None, relu=False, acc=F64), relu=True, acc=F64)
    require(check_bf16(f2(out), f2(ref)), "bn apply with shortcut BatchNorm")
    assert torch.equal(bits, pack_bits(out.reshape(-1) > 0)), "mask bits"


def resnet_bn_bwd_dual(lib, c, seed):
    """icamd_bn_bwd_dual: the block-output BatchNorm and the shortcut BatchNorm backward of a projection block, one mask."""
    hip = _harness.hip()
    N, h, C = c
    M = N * h * h
    gen = torch.Generator(device=DEV).manual_seed(seed)
    mask = torch.rand(N, h, h, C, generator=gen, device=DEV) > 0.45
    bits = pack_bits(mask)
    dout = rnd((N, h, h, C), seed + 1)
    yA, yB = rnd((N, h, h, C), seed + 2, shift=0.2), rnd((N, h, h, C), seed + 3, shift=-0.2)
    A, B = _bn_fake_coeffs(C, seed + 4), _bn_fake_coeffs(C, seed + 8)
    wsb = lib.icamd_bn_bwd_workspace_bytes(M, C)
    wsA, wsB = torch.zeros(wsb, dtype=torch.uint8, device=DEV), torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    out = {k: (torch.empty_like(dout), torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV))
           for k in "AB"}
    ok(lib.icamd_bn_bwd_dual(dout.data_ptr(), bits.data_ptr(), yA.data_ptr(), A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(),
                             out["A"][1].data_ptr(), out["A"][2].data_ptr(), out["A"][0].data_ptr(), yB.data_ptr(), B[0].data_ptr(),
                             B[1].data_ptr(), B[2].data_ptr(), out["B"][1].data_ptr(), out["B"][2].data_ptr(), out["B"][0].data_ptr(),
                             M, C, 0, wsA.data_ptr(), wsB.data_ptr(), wsb, hip.stream_ptr()), "bn_bwd_dual")
    sync()
    act = mask.to(torch.bfloat16)        # > 0 exactly where the mask bit is set
    for k, y, (m, i, sc, _) in (("A", yA, A), ("B", yB, B)):
        rdy, rdg, rdb, _ = R.bn_bwd(dout, act, y, m, i, sc, relu=True, acc=F64)
        require(check_bf16(f2(out[k][0]), f2(rdy)), f"dual BatchNorm backward {k}")
        assert R.rel_l2(out[k][1], rdg) <= 1e-4 and R.rel_l2(out[k][2], rdb) <= 1e-4, f"dual {k}: dgamma / dbeta"


def resnet_dgrad_sub2(lib, c, seed):
    """icamd_conv2d_dgrad_sub2 (first block of stages 2-4, nets.py default): conv1's data gradient plus the 1x1 / stride-2
    shortcut's gradient, which lives on the even pixels only ([N][H/2][W/2][Cin] addend)."""
    hip = _harness.hip()
    N, h, Cin, Cout = c
    d = hip.conv_desc(N, h, h, Cin, Cout, 1, 1, 1, 0)
    dy = rnd((N, h, h, Cout), seed)
    w = rnd((Cout, 1, 1, Cin), seed + 1, scale=(1.0 / Cout) ** 0.5)
    w_t = w.permute(3, 1, 2, 0).contiguous()
    compact = rnd((N, (h + 1) // 2, (h + 1) // 2, Cin), seed + 2)
    dx = torch.empty(N, h, h, Cin, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_conv2d_dgrad_sub2(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), compact.data_ptr(), hip.stream_ptr()),
       "dgrad_sub2")
    sync()
    full = torch.zeros(N, h, h, Cin, dtype=torch.bfloat16, device=DEV)
    full[:, ::2, ::2, :] = compact
    require(check_bf16(f2(dx), f2(R.conv2d_dgrad(dy, w, (h, h), 1, 0, full, acc=F64))), "dgrad + even-grid shortcut gradient")


def resnet_dgrad_bnred_even(lib, c, seed):
    """icamd_conv2d_dgrad_bnred in its even-grid addend form (mode 1: the 1x1 / stride-2 shortcut's gradient of the next
    stage's first block, nets.py default where the pair is supported)."""
    hip = _harness.hip()
    N, h, Cin, Cout = c
    d = hip.conv_desc(N, h, h, Cin, Cout, 1, 1, 1, 0)
    assert lib.icamd_conv2d_dgrad_bnred_supported(ctypes.byref(d)) == 1
    gen = torch.Generator(device=DEV).manual_seed(seed)
    dy = rnd((N, h, h, Cout), seed + 1)
    w = rnd((Cout, 1, 1, Cin), seed + 2, scale=(1.0 / Cout) ** 0.5)
    w_t = w.permute(3, 1, 2, 0).contiguous()
    compact = rnd((N, (h + 1) // 2, (h + 1) // 2, Cin), seed + 3)
    y = rnd((N, h, h, Cin), seed + 4, scale=1.5, shift=0.3)
    pmask = torch.rand(N, h, h, Cin, generator=gen, device=DEV) > 0.45
    pbits = pack_bits(pmask)
    rows = lib.icamd_conv2d_dgrad_stats_rows(ctypes.byref(d))
    part = torch.full((rows, 2, Cin), float("nan"), device=DEV)
    g = torch.empty(N, h, h, Cin, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_conv2d_dgrad_bnred(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), g.data_ptr(), compact.data_ptr(), None, 1,
                                    y.data_ptr(), pbits.data_ptr(), part.data_ptr(), hip.stream_ptr()), "dgrad_bnred even grid")
    sync()
    full = torch.zeros(N, h, h, Cin, dtype=torch.bfloat16, device=DEV)
    full[:, ::2, ::2, :] = compact
    require(check_bf16(f2(g), f2(R.conv2d_dgrad(dy, w, (h, h), 1, 0, full, acc=F64) * pmask)), "g (even-grid addend)")
    require(check_stats(part, g, weight=y), "(sum g, sum g*y) partials (even-grid addend)")


def resnet_avgpool(lib, N, seed):
    """icamd_avgpool_fwd / _bwd over the 7 x 7 x 2048 features."""
    hip = _harness.hip()
    HW, C = 49, 2048
    x = rnd((N, 7, 7, C), seed, relu=True)
    out = torch.empty(N, C, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_avgpool_fwd(x.data_ptr(), out.data_ptr(), N, HW, C, hip.stream_ptr()), "avgpool fwd")
    dout = rnd((N, C), seed + 1)
    dx = torch.empty(N, HW, C, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_avgpool_bwd(dout.data_ptr(), dx.data_ptr(), N, HW, C, hip.stream_ptr()), "avgpool bwd")
    sync()
    require(check_bf16(out.float(), R.avgpool_fwd(x, acc=F64)), "avgpool forward")
    rdx = R.bf16_round((dout.double() / HW).reshape(N, 1, C).expand(N, HW, C)).reshape(-1, C)
    require(check_bf16(f2(dx), rdx), "avgpool backward")


TRAIN_CASES = ([(f"resnet50-train-256-{_conv_id(c)}-fwd_stats_bn", resnet_conv_fwd_bn, c) for c in RESNET_CONVS]
               + [(f"resnet50-train-256-{_conv_id(c)}-dgrad", resnet_conv_dgrad, c) for c in RESNET_CONVS]
               + [(f"resnet50-train-256-{_conv_id(c)}-wgrad", resnet_conv_wgrad, c) for c in RESNET_CONVS]
               + [("resnet50-train-256-stem7x7s2-224-fwd_wgrad", lambda lib, c, seed: resnet_stem(lib, seed), None)]
               + [(f"resnet50-train-256-{c[2]}to{c[3]}-1x1-{c[1]}-bn_apply_conv1x1_fused{'-res_bn' if rb else ''}",
                   lambda lib, c, seed, rb=rb: resnet_bn_apply_conv1x1_fused(lib, c, seed, rb), c)
                  for c, rb in (((256, 56, 256, 64), False), ((256, 56, 256, 64), True), ((256, 56, 256, 128), False),
                                ((256, 28, 512, 128), False))]
               + [(f"resnet50-train-256-{c[2]}to{c[3]}-1x1-{c[1]}-conv1x1_bn_bwd_fused", resnet_conv1x1_bn_bwd_fused, c)
                  for c in ((256, 56, 64, 256), (256, 28, 128, 512))]
               + [(f"resnet50-train-256-{c[3]}to{c[2]}-1x1-{c[1]}-dgrad_bnred", resnet_dgrad_bnred, c)
                  for c in ((256, 56, 256, 64), (256, 28, 512, 128), (256, 14, 1024, 256))]
               + [(f"resnet50-train-256-{c[3]}to{c[2]}-1x1-{c[1]}-dgrad_bnred_even_grid", resnet_dgrad_bnred_even, c)
                  for c in ((256, 28, 512, 128), (256, 14, 1024, 256))]
               + [(f"resnet50-train-256-{c[3]}to{c[2]}-1x1-{c[1]}-dgrad_sub2", resnet_dgrad_sub2, c)
                  for c in ((256, 56, 256, 128), (256, 28, 512, 256), (256, 14, 1024, 512))]
               + [("resnet50-train-256-stem-112-bn_relu_maxpool_fwd_bwd", lambda lib, c, seed: resnet_stem_bn_pool(lib, seed), None)]
               + [(f"resnet50-train-256-{c[1]}-{c[2]}-bn_apply_res_bn", resnet_bn_apply_res_bn, c)
                  for c in ((256, 56, 256), (256, 28, 512), (256, 14, 1024), (256, 7, 2048))]
               + [(f"resnet50-train-256-{c[1]}-{c[2]}-bn_bwd_dual", resnet_bn_bwd_dual, c)
                  for c in ((256, 56, 256), (256, 28, 512), (256, 14, 1024), (256, 7, 2048))]
               + [("resnet50-train-256-avgpool-7-2048-fwd_bwd", lambda lib, c, seed: resnet_avgpool(lib, TRAIN_N, seed), None)])


@pytest.mark.parametrize("case", range(len(TRAIN_CASES)), ids=[c[0] for c in TRAIN_CASES])
def test_resnet50_train(lib, case):
    _, fn, c = TRAIN_CASES[case]
    fn(lib, c, 1000 + 17 * case)


# ============================================ ResNet-50, eval, batch 384 ============================================
def resnet_eval_fold_act(lib, c, seed):
    """icamd_bn_fold_filters + icamd_conv2d_fwd_act (folded shift, optional residual and ReLU) at batch 384."""
    hip = _harness.hip()
    cin, cout, k, st, h = c
    pad = k // 2
    N = EVAL_N
    d = hip.conv_desc(N, h, h, cin, cout, k, k, st, pad)
    x = rnd((N, h, h, cin), seed, relu=True)
    w = torch.randn(cout, k, k, cin, generator=torch.Generator(device=DEV).manual_seed(seed + 1), device=DEV) * (2.0 / (k * k * cin)) ** 0.5
    gamma, beta = urand(cout, seed + 2, 0.5, 1.5), urand(cout, seed + 3, -0.1, 0.1)
    rm, rv = urand(cout, seed + 4, -0.2, 0.2), urand(cout, seed + 5, 0.5, 1.5)
    wf = torch.empty(cout, k, k, cin, dtype=torch.bfloat16, device=DEV)
    shift = torch.empty(cout, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_bn_fold_filters(w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, cout,
                                 k * k * cin, wf.data_ptr(), shift.data_ptr(), s), "fold")
    sync()
    sc = gamma / torch.sqrt(rv + 1e-5)
    wf_ref = R.bf16_round(w * sc.view(-1, 1, 1, 1))
    assert R.max_bf16_ulp(wf.float(), wf_ref) <= 1.0 and float((wf.float() != wf_ref).float().mean()) <= 1e-4, "folded filters"
    res = rnd((N, d.OH, d.OW, cout), seed + 6)
    y = torch.empty(N, d.OH, d.OW, cout, dtype=torch.bfloat16, device=DEV)
    # the three epilogues of the folded network: conv1 / conv2 (+ ReLU), conv3 (+ residual + ReLU), the shortcut (neither)
    for use_res, relu in ((False, True), (True, True), (False, False)):
        r = res if use_res else None
        ok(lib.icamd_conv2d_fwd_act(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), y.data_ptr(), shift.data_ptr(), hip.ptr(r), int(relu),
                                    s), "fwd_act")
        sync()
        ref = R.conv2d_fwd(x, wf, st, pad, shift, r, acc=F64)
        if relu:
            ref = ref.clamp_min(0)
        require(check_bf16(f2(y), f2(ref)), f"conv + folded BatchNorm (residual {use_res}, ReLU {relu})")
        del ref


def resnet_eval_stem_pool(lib, seed):
    """Eval stem at batch 384: icamd_stem7x7s2_fwd with the folded bias + ReLU in its epilogue, then icamd_maxpool3x3s2_fwd."""
    hip = _harness.hip()
    N, H, Cout, OH = EVAL_N, 224, 64, 112
    x = rnd((N, 3, H, H), seed).float()
    w = rnd((Cout, 7, 7, 3), seed + 1, scale=(2.0 / 147) ** 0.5).float()
    bias = urand(Cout, seed + 2, -0.3, 0.3)
    x4 = torch.empty(N, H, H + 8, 4, dtype=torch.bfloat16, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_pack_input_rgb4(x.data_ptr(), x4.data_ptr(), N, 3, H, H, 0, 1.0, 0, 0, 0, 0, s), "pack")
    wp = torch.zeros(Cout, 8, 8, 4, device=DEV)
    wp[:, :7, :7, :3] = w
    wd = wp.to(torch.bfloat16)
    y = torch.empty(N, OH, OH, Cout, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_stem7x7s2_fwd(x4.data_ptr(), wd.data_ptr(), y.data_ptr(), bias.data_ptr(), None, 1, N, H, H, Cout, s), "stem fwd")
    sync()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous()
    del x, x4
    require(check_bf16(f2(y), f2(R.conv2d_fwd(x_nhwc, w, 2, 3, bias, acc=F64).clamp_min(0))), "stem + bias + ReLU")
    del x_nhwc
    pooled = torch.empty(N, 56, 56, Cout, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_maxpool3x3s2_fwd(y.data_ptr(), pooled.data_ptr(), None, N, OH, OH, Cout, s), "maxpool fwd")
    sync()
    assert torch.equal(pooled.float(), R.maxpool3x3s2_fwd(y)[0]), "max-pool (exact)"


EVAL_CASES = ([(f"resnet50-eval-384-{_conv_id(c)}-fold_fwd_act", resnet_eval_fold_act, c) for c in RESNET_CONVS]
              + [("resnet50-eval-384-stem7x7s2-224-act_maxpool", lambda lib, c, seed: resnet_eval_stem_pool(lib, seed), None),
                 ("resnet50-eval-384-avgpool-7-2048", lambda lib, c, seed: resnet_avgpool(lib, EVAL_N, seed), None)])


@pytest.mark.parametrize("case", range(len(EVAL_CASES)), ids=[c[0] for c in EVAL_CASES])
def test_resnet50_eval(lib, case):
    _, fn, c = EVAL_CASES[case]
    fn(lib, c, 5000 + 13 * case)


# ============================================ ViT-B/16, batch 256 ============================================
def linear_layer(lib, rows, cin, cout, seed, gelu_fwd=False, gelu_bwd=False, addend=False):
    """One Linear layer as the model runs it (a 1x1 convolution over `rows` pixels): forward (+bias, + residual addend, or
    GELU in the store pass), data gradient (GELU' in the store pass where the layer's input is a GELU output), weight
    gradient with the bias gradient."""
    hip = _harness.hip()
    d = hip.conv_desc(rows, 1, 1, cin, cout, 1, 1, 1, 0)
    x = rnd((rows, 1, 1, cin), seed)
    if gelu_bwd:     # the layer's input is a GELU output
        x = R.gelu_fwd(x).to(torch.bfloat16)
    w = rnd((cout, 1, 1, cin), seed + 1, scale=(1.0 / cin) ** 0.5)
    b = urand(cout, seed + 2, -0.5, 0.5)
    s = hip.stream_ptr()
    y = torch.empty(rows, 1, 1, cout, dtype=torch.bfloat16, device=DEV)
    if gelu_fwd:
        a = torch.empty_like(y)
        ok(lib.icamd_conv2d_fwd_gelu(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), s), "fwd_gelu")
        sync()
        require(check_bf16(f2(y), f2(R.conv2d_fwd(x, w, 1, 0, b, acc=F64))), "forward (z)")
        require(check_bf16(f2(a), f2(R.gelu_fwd(y, acc=F64))), "GELU of the stored z")
        del a
    else:
        res = rnd((rows, 1, 1, cout), seed + 3) if addend else None
        ok(lib.icamd_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), b.data_ptr(), hip.ptr(res), None, s), "fwd")
        sync()
        require(check_bf16(f2(y), f2(R.conv2d_fwd(x, w, 1, 0, b, res, acc=F64))), "forward")
        del res
    del y
    dy = rnd((rows, 1, 1, cout), seed + 4)
    w_t = w.permute(3, 1, 2, 0).contiguous()
    dx = torch.empty(rows, 1, 1, cin, dtype=torch.bfloat16, device=DEV)
    if gelu_bwd:
        z = rnd((rows, 1, 1, cin), seed + 5)
        ok(lib.icamd_conv2d_dgrad_gelu(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), z.data_ptr(), dx.data_ptr(), s), "dgrad_gelu")
        sync()
        # the kernel rounds dgrad to bf16 and applies GELU' to that (bit-identical to icamd_conv2d_dgrad + icamd_gelu_bwd)
        require(check_bf16(f2(dx), f2(R.gelu_bwd(R.conv2d_dgrad(dy, w, (1, 1), 1, 0, acc=F64), z, acc=F64))), "dgrad * GELU'")
        del z
    else:
        ok(lib.icamd_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), None, None, s), "dgrad")
        sync()
        require(check_bf16(f2(dx), f2(R.conv2d_dgrad(dy, w, (1, 1), 1, 0, acc=F64))), "dgrad")
    del dx
    ws, wsb = wgrad_ws(lib, d)
    dw = torch.full((cout, cin), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    ok(lib.icamd_conv2d_wgrad_bias(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), wsb, s),
       "wgrad_bias")
    sync()
    require(check_fp32(dw, R.conv2d_wgrad(x, dy, (1, 1), 1, 0, acc=F64).reshape(cout, cin)), "wgrad")
    bref = dy.double().reshape(-1, cout).sum(0)
    require(check_close(db, bref, 1e-4, 1e-3 * (float(bref.abs().max()) + 1), "bias gradient"), "wgrad (bias)")


def patch_conv(lib, N, H, cin_true, cout, k, seed, relu=False):
    """A k x k / stride-k patchifying convolution on the 8-channel packed input (ViT patch embedding, ConvNeXt stem) or on a
    feature map (ConvNeXt downsample): forward + bias, data gradient (feature-map inputs), weight gradient + bias."""
    hip = _harness.hip()
    cin = 8 if cin_true == 3 else cin_true
    d = hip.conv_desc(N, H, H, cin, cout, k, k, k, 0)
    x = rnd((N, H, H, cin), seed, relu=relu)
    if cin_true == 3:
        x[..., 3:] = 0
    w = rnd((cout, k, k, cin), seed + 1, scale=(1.0 / (k * k * cin_true)) ** 0.5)
    if cin_true == 3:
        w[..., 3:] = 0
    b = urand(cout, seed + 2, -0.5, 0.5)
    s = hip.stream_ptr()
    y = torch.empty(N, d.OH, d.OW, cout, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), b.data_ptr(), None, None, s), "fwd")
    sync()
    require(check_bf16(f2(y), f2(R.conv2d_fwd(x, w, k, 0, b, acc=F64))), "forward")
    del y
    dy = rnd((N, d.OH, d.OW, cout), seed + 3)
    if cin_true != 3:
        w_t = w.permute(3, 1, 2, 0).contiguous()
        dx = torch.empty_like(x)
        ok(lib.icamd_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), w_t.data_ptr(), dx.data_ptr(), None, None, s), "dgrad")
        sync()
        require(check_bf16(f2(dx), f2(R.conv2d_dgrad(dy, w, (H, H), k, 0, acc=F64))), "dgrad")
        del dx
    ws, wsb = wgrad_ws(lib, d)
    dw = torch.full((cout, k, k, cin), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    ok(lib.icamd_conv2d_wgrad_bias(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), wsb, s),
       "wgrad_bias")
    sync()
    ref = R.conv2d_wgrad(x, dy, (k, k), k, 0, acc=F64)
    if cin_true == 3:   # the padding channels' gradient is that of zero inputs: exactly zero
        assert float(dw[..., 3:].abs().max()) == 0.0
        dw, ref = dw[..., :3], ref[..., :3]
    require(check_fp32(dw.reshape(cout, -1), ref.reshape(cout, -1)), "wgrad")
    bref = dy.double().reshape(-1, cout).sum(0)
    require(check_close(db, bref, 1e-4, 1e-3 * (float(bref.abs().max()) + 1), "bias gradient"), "wgrad (bias)")


def layernorm(lib, rows, C, seed, eps):
    hip = _harness.hip()
    x = rnd((rows, C), seed, scale=2.0, shift=0.5)
    gamma, beta = urand(C, seed + 1, 0.5, 1.5), urand(C, seed + 2, -0.2, 0.2)
    y = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C,
                               eps, s), "ln fwd")
    sync()
    ry, rmean, rrstd = R.layernorm_fwd(x, gamma, beta, eps, acc=F64)
    require(check_close(mean, rmean, 1e-5, 1e-6, "mean") + check_close(rstd, rrstd, 1e-5, 0, "rstd"), "layernorm fwd")
    require(check_bf16(y.float(), ry), "layernorm fwd")
    del y, ry
    dy = rnd((rows, C), seed + 3)
    wsb = lib.icamd_layernorm_bwd_workspace_bytes(rows, C)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    dx = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    ok(lib.icamd_layernorm_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), None, dx.data_ptr(),
                               dg.data_ptr(), db.data_ptr(), rows, C, 0, ws.data_ptr(), wsb, s), "ln bwd")
    sync()
    rdx, rdg, rdb = R.layernorm_bwd(dy, x, gamma, eps, acc=F64)
    require(check_bf16(dx.float(), rdx), "layernorm bwd dx")
    assert R.rel_l2(dg, rdg) <= 1e-4 and R.rel_l2(db, rdb) <= 1e-4, "layernorm dgamma / dbeta"


def vit_attention(lib, seed):
    """icamd_attention_fwd / _bwd at B = 256 (3072 (image, head) pairs over one persistent workgroup per CU: pair p runs in
    round p // #CUs of workgroup p % #CUs).  The reference covers images 0, 21, 128 and 234-255: heads 0, 255, 256 and 3071,
    and every pair from 234 * 12 = 2808 on -- the last round of every workgroup on a 256-CU device (pairs 2816-3071)."""
    hip = _harness.hip()
    B, T, H, D = VIT_B, VIT_T, VIT_H, VIT_D
    scale = D ** -0.5
    qkv = rnd((B * T, 3 * H * D), seed)
    out = torch.full((B * T, H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, H, T, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, T, H, D, scale, s), "attention fwd")
    dout = rnd((B * T, H * D), seed + 1)
    delta = torch.empty(B, H, T, device=DEV)
    dqkv = torch.full((B * T, 3 * H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_attention_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, T,
                               H, D, scale, s), "attention bwd")
    sync()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    imgs = torch.tensor([0, 21, 128] + list(range(234, 256)), device=DEV)
    nb = len(imgs)
    sub = lambda t: t.reshape(B, T, -1)[imgs].reshape(nb * T, -1)   # noqa: E731
    ro, rlse = R.attention_fwd(sub(qkv), nb, T, H, D, scale, acc=F64)
    require(check_close(lse[imgs], rlse, 1e-4, 1e-4, "lse"), "attention lse")
    # the bounds test_kernels_gpu.py applies to this entry (P and dS pass through bf16 MFMA operands, the oracle keeps them
    # wide); the per-block bound is the global one -- the same rounding model holds in every 64 x 64 (token x head) block.
    # max_frac: test_kernels_gpu.py's rule for this entry (1e-6 wherever B * H > 256; here 3072 pairs)
    require(check_bf16(sub(out).float(), ro, rel=3e-3, block_rel=3e-3, atol_rms=8e-3, max_frac=1e-6), "attention fwd")
    rd = R.attention_bwd(sub(qkv), sub(dout), nb, T, H, D, scale, acc=F64)
    got = sub(dqkv).float()
    for name, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, 2 * H * D)), ("dv", slice(2 * H * D, 3 * H * D))):
        fails = [f for f in check_bf16(got[:, sl].contiguous(), rd[:, sl].contiguous(), rel=6e-3, block_rel=6e-3)
                 if "elementwise" not in f]    # test_kernels_gpu.py bounds the gradient by rel L2 only
        require(fails, f"attention bwd {name}")


def cnx_layerscale_tail(lib, C, h, seed):
    """The ConvNeXt block tail with the layer scale folded into fc2 and a drop-path keep mask, at a stage's real size:
    fc2 on the folded filter with the residual addend, icamd_rows_fix (dropped samples: out = x, their fc2 input zeroed);
    backward icamd_dropped_colsum, the weight gradient + bias, icamd_layerscale_param_grads, and the data gradient on the
    folded filter with its dropped rows zeroed."""
    hip = _harness.hip()
    N, HW, K = CNX_N, h * h, 4 * C
    M = N * HW
    gen = torch.Generator(device=DEV).manual_seed(seed)
    a = R.gelu_fwd(rnd((M, K), seed + 1)).to(torch.bfloat16)
    x = rnd((M, C), seed + 2)
    W2 = torch.randn(C, K, generator=gen, device=DEV) * K ** -0.5
    b2 = urand(C, seed + 3, -0.2, 0.2)
    gamma = urand(C, seed + 4, 0.3, 1.3)
    cb = 1.0 / 0.9
    keep = (torch.rand(N, generator=gen, device=DEV) > 0.1).float() * cb
    keep[1], keep[N - 1] = 0.0, 0.0                  # the second and the last sample dropped
    wf = (cb * gamma[:, None] * W2).to(torch.bfloat16)   # the fold (a filter fold: icamd_layerscale_fold, tested elsewhere)
    fold_bias = (cb * gamma * b2).contiguous()
    d = hip.conv_desc(N, h, h, K, C, 1, 1, 1, 0)
    s = hip.stream_ptr()
    a_in = a.clone()
    out = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_conv2d_fwd(ctypes.byref(d), a.data_ptr(), wf.data_ptr(), out.data_ptr(), fold_bias.data_ptr(), x.data_ptr(), None, s),
       "fc2 folded")
    ok(lib.icamd_rows_fix(keep.data_ptr(), N, out.data_ptr(), x.data_ptr(), HW * C * 2, a.data_ptr(), HW * K * 2, s), "rows_fix")
    sync()
    kept = (keep != 0).repeat_interleave(HW)
    ref = R.conv2d_fwd(a_in.reshape(M, 1, 1, K), wf.reshape(C, 1, 1, K), 1, 0, fold_bias, x.reshape(M, 1, 1, C), acc=F64).reshape(M, C)
    ref[~kept] = x[~kept].float()
    require(check_bf16(out.float(), ref), "folded fc2 + layer scale + drop path")
    assert torch.equal(out[~kept], x[~kept]) and bool((a[~kept] == 0).all()) and torch.equal(a[kept], a_in[kept]), "dropped rows"
    del ref, a_in
    dout = rnd((M, C), seed + 5)
    part = torch.full((N, C), float("nan"), device=DEV)
    ok(lib.icamd_dropped_colsum(dout.data_ptr(), keep.data_ptr(), N, HW, C, part.data_ptr(), s), "dropped_colsum")
    wsb = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.zeros(max(wsb, 256), dtype=torch.uint8, device=DEV)
    G, S = torch.empty(C, K, device=DEV), torch.empty(C, device=DEV)
    ok(lib.icamd_conv2d_wgrad_bias(ctypes.byref(d), a.data_ptr(), dout.data_ptr(), G.data_ptr(), S.data_ptr(), 0, ws.data_ptr(), wsb, s),
       "wgrad_bias")
    grads = torch.full((C * K + 2 * C,), float("nan"), device=DEV)
    ok(lib.icamd_layerscale_param_grads(G.data_ptr(), W2.data_ptr(), b2.data_ptr(), gamma.data_ptr(), S.data_ptr(), part.data_ptr(), N,
                                        cb, C, K, grads.data_ptr(), grads.data_ptr() + 4 * C * K, grads.data_ptr() + 4 * (C * K + C), 0,
                                        s), "layerscale_param_grads")
    da = torch.empty(M, K, dtype=torch.bfloat16, device=DEV)
    w_t = wf.t().contiguous()
    ok(lib.icamd_conv2d_dgrad(ctypes.byref(d), dout.data_ptr(), w_t.data_ptr(), da.data_ptr(), None, None, s), "dgrad folded")
    ok(lib.icamd_rows_fix(keep.data_ptr(), N, da.data_ptr(), None, HW * K * 2, None, 0, s), "rows_fix (gradient)")
    sync()
    d64 = dout.double().reshape(N, HW, C)
    rp = d64.sum(1) * (keep == 0).double()[:, None]
    require(check_close(part, rp, 1e-5, 1e-4 * (float(rp.abs().max()) + 1), "dropped column sums"), "dropped_colsum")
    require(check_fp32(G, dout.double().t() @ a.double()), "weight gradient of the folded fc2")
    # the layer's parameter gradients by the three-step definition fc2 -> layer scale -> drop path (the oracle's
    # R.layerscale_bwd on the fp32 Linear layer), in fp64: the folded path rounds the filter once where that one rounds z2 --
    # the bound test_kernels_gpu.py applies (2e-3), also per 64 x 64 block of dW
    kk = keep.double().repeat_interleave(HW)[:, None]
    a_ref = R.gelu_fwd(rnd((M, K), seed + 1)).double() * (keep != 0).double().repeat_interleave(HW)[:, None]
    dz2 = d64.reshape(M, C) * kk * gamma.double()
    z2 = a_ref @ W2.to(torch.bfloat16).double().t() + b2.double()
    r_dw, r_db = dz2.t() @ a_ref, dz2.sum(0)
    r_dg = (d64.reshape(M, C) * kk * z2).sum(0)
    require(check_fp32(grads[:C * K].reshape(C, K), r_dw, rel=2e-3), "layer-scale dW")
    assert R.rel_l2(grads[C * K:C * K + C], r_db) <= 2e-3 and R.rel_l2(grads[C * K + C:], r_dg) <= 2e-3, "layer-scale db / dgamma"
    del a_ref, z2, dz2
    rda = R.conv2d_dgrad(dout.reshape(M, 1, 1, C), wf.reshape(C, 1, 1, K), (1, 1), 1, 0, acc=F64).reshape(M, K)
    rda[~kept] = 0
    require(check_bf16(da.float(), rda), "data gradient on the folded filter, dropped rows zeroed")


def vit_tokens(lib, seed):
    """Token plumbing at B = 256: icamd_vit_tokens_fwd (class token + position embedding), icamd_batch_sum (their
    gradients), icamd_strided_rows_copy (class-token gather / scatter, patch gradients)."""
    hip = _harness.hip()
    B, T, D = VIT_B, VIT_T, VIT_DIM
    patches = rnd((B, T - 1, D), seed)
    cls, pos = urand(D, seed + 1, -1, 1), urand(T * D, seed + 2, -1, 1).reshape(T, D)
    tok = torch.empty(B, T, D, dtype=torch.bfloat16, device=DEV)
    s = hip.stream_ptr()
    ok(lib.icamd_vit_tokens_fwd(patches.data_ptr(), cls.data_ptr(), pos.data_ptr(), tok.data_ptr(), B, T, D, s), "tokens")
    sync()
    ref = R.bf16_round(torch.cat([cls.double().expand(B, 1, D), patches.double()], 1) + pos.double())
    require(check_bf16(f2(tok), f2(ref)), "tokens")
    dx = rnd((B, T, D), seed + 3)
    gpos, gcls = torch.full((T * D,), float("nan"), device=DEV), torch.full((D,), float("nan"), device=DEV)
    ok(lib.icamd_batch_sum(dx.data_ptr(), T * D, B, T * D, gpos.data_ptr(), 0, s), "pos grad")
    ok(lib.icamd_batch_sum(dx.data_ptr(), T * D, B, D, gcls.data_ptr(), 0, s), "cls grad")
    cls_rows = torch.empty(B, D, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_strided_rows_copy(tok.data_ptr(), T * D, cls_rows.data_ptr(), D, B, D, s), "cls gather")
    dpatch = torch.empty(B, T - 1, D, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_strided_rows_copy(dx.data_ptr() + 2 * D, T * D, dpatch.data_ptr(), (T - 1) * D, B, (T - 1) * D, s), "patch grads")
    sync()
    rpos = dx.double().sum(0).reshape(T, D)
    require(check_fp32(gpos.reshape(T, D), rpos, rel=1e-5), "position-embedding gradient")
    require(check_close(gcls, rpos[0], 1e-5, 1e-5 * float(rpos[0].abs().max()), "class-token gradient"), "class-token gradient")
    assert torch.equal(cls_rows, tok[:, 0]) and torch.equal(dpatch, dx[:, 1:]), "strided row copies"


def head_bias_colsum(lib, N, seed):
    """icamd_colsum: the classifier's bias gradient from dlogits [N][1024] (1000 classes padded)."""
    hip = _harness.hip()
    dl = rnd((N, 1024), seed)
    out = torch.full((1024,), float("nan"), device=DEV)
    ok(lib.icamd_colsum(dl.data_ptr(), N, 1024, 1024, out.data_ptr(), 0, hip.stream_ptr()), "colsum")
    sync()
    ref = dl.double().sum(0)
    require(check_close(out, ref, 1e-5, 1e-5 * float(ref.abs().max()), "column sums"), "head bias gradient")


VIT_CASES = [
    ("vit_b16-256-patch16x16s16-fwd_wgrad", lambda lib, seed: patch_conv(lib, VIT_B, 224, 3, VIT_DIM, 16, seed)),
    ("vit_b16-256-qkv-768to2304", lambda lib, seed: linear_layer(lib, VIT_M, VIT_DIM, 3 * VIT_DIM, seed)),
    ("vit_b16-256-proj-768to768", lambda lib, seed: linear_layer(lib, VIT_M, VIT_DIM, VIT_DIM, seed, addend=True)),
    ("vit_b16-256-fc1-768to3072-gelu", lambda lib, seed: linear_layer(lib, VIT_M, VIT_DIM, 4 * VIT_DIM, seed, gelu_fwd=True)),
    ("vit_b16-256-fc2-3072to768-gelu_bwd", lambda lib, seed: linear_layer(lib, VIT_M, 4 * VIT_DIM, VIT_DIM, seed, addend=True,
                                                                          gelu_bwd=True)),
    ("vit_b16-256-layernorm-768", lambda lib, seed: layernorm(lib, VIT_M, VIT_DIM, seed, 1e-6)),
    ("vit_b16-256-attention-3072heads", vit_attention),
    ("vit_b16-256-head-768to1024", lambda lib, seed: linear_layer(lib, VIT_B, VIT_DIM, 1024, seed)),
    ("vit_b16-256-tokens-pos_cls_grads-row_copies", vit_tokens),
    ("vit_b16-256-head-bias_colsum", lambda lib, seed: head_bias_colsum(lib, VIT_B, seed)),
]


@pytest.mark.parametrize("case", range(len(VIT_CASES)), ids=[c[0] for c in VIT_CASES])
def test_vit_b16(lib, case):
    VIT_CASES[case][1](lib, 7000 + 11 * case)


# ============================================ ConvNeXt-T, batch 256 ============================================
def dwconv7(lib, C, h, seed):
    """icamd_dwconv7_fwd / _dgrad (+ residual addend) / _wgrad_bias (or _wgrad where the one-pass form is refused)."""
    hip = _harness.hip()
    N = CNX_N
    x = rnd((N, h, h, C), seed)
    w = rnd((C, 7, 7), seed + 1, scale=0.15)
    b = urand(C, seed + 2, -0.1, 0.1)
    wd = w.permute(1, 2, 0).contiguous()          # kernel layout [7][7][C]
    s = hip.stream_ptr()
    y = torch.empty(N, h, h, C, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_dwconv7_fwd(x.data_ptr(), wd.data_ptr(), b.data_ptr(), y.data_ptr(), N, h, h, C, s), "dw fwd")
    sync()
    require(check_bf16(f2(y), f2(R.dwconv7_fwd(x, w, b, acc=F64))), "dwconv fwd")
    del y
    dy, addend = rnd((N, h, h, C), seed + 3), rnd((N, h, h, C), seed + 4)
    dx = torch.empty(N, h, h, C, dtype=torch.bfloat16, device=DEV)
    ok(lib.icamd_dwconv7_dgrad(dy.data_ptr(), wd.data_ptr(), addend.data_ptr(), dx.data_ptr(), N, h, h, C, s), "dw dgrad")
    wsb = lib.icamd_dwconv7_wgrad_workspace_bytes(N, h, h, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw = torch.full((7, 7, C), float("nan"), device=DEV)
    db = torch.full((C,), float("nan"), device=DEV)
    one_pass = bool(lib.icamd_dwconv7_wgrad_bias_supported(N, h, h, C))
    if one_pass:
        ok(lib.icamd_dwconv7_wgrad_bias(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), wsb, N, h, h, C, s),
           "dw wgrad_bias")
    else:
        ok(lib.icamd_dwconv7_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), wsb, N, h, h, C, s), "dw wgrad")
    sync()
    rdx, rdw = R.dwconv7_bwd(x, w, dy, addend, acc=F64)
    require(check_bf16(f2(dx), f2(rdx)), "dwconv dgrad")
    # filters as [C, 49]: the per-block bound runs over (channel x tap) blocks
    require(check_fp32(dw.reshape(49, C).t(), rdw.reshape(C, 49)), "dwconv wgrad")
    if one_pass:
        bref = dy.double().reshape(-1, C).sum(0)
        require(check_close(db, bref, 1e-5, 1e-4 * max(1.0, float(bref.abs().max())), "bias gradient"), "dwconv bias")


CNX_CASES = [("convnext_t-256-stem4x4s4-224", lambda lib, seed: patch_conv(lib, CNX_N, 224, 3, 96, 4, seed))]
for _si, (_C, _h) in enumerate(CNX_STAGES):
    _M = CNX_N * _h * _h
    CNX_CASES += [
        (f"convnext_t-256-s{_si}-{_h}-dwconv7-{_C}", lambda lib, seed, C=_C, h=_h: dwconv7(lib, C, h, seed)),
        (f"convnext_t-256-s{_si}-{_h}-layernorm-{_C}", lambda lib, seed, C=_C, M=_M: layernorm(lib, M, C, seed, 1e-6)),
        (f"convnext_t-256-s{_si}-{_h}-pw1-{_C}to{4 * _C}-gelu",
         lambda lib, seed, C=_C, M=_M: linear_layer(lib, M, C, 4 * C, seed, gelu_fwd=True)),
        (f"convnext_t-256-s{_si}-{_h}-pw2-{4 * _C}to{_C}-gelu_bwd",
         lambda lib, seed, C=_C, M=_M: linear_layer(lib, M, 4 * C, C, seed, addend=True, gelu_bwd=True)),
        (f"convnext_t-256-s{_si}-{_h}-pw2-folded_layerscale_droppath-{4 * _C}to{_C}",
         lambda lib, seed, C=_C, h=_h: cnx_layerscale_tail(lib, C, h, seed)),
    ]
    if _si < 3:
        CNX_CASES.append((f"convnext_t-256-s{_si}-{_h}-downsample2x2s2-{_C}to{2 * _C}",
                          lambda lib, seed, C=_C, h=_h: patch_conv(lib, CNX_N, h, C, 2 * C, 2, seed)))
CNX_CASES += [("convnext_t-256-head-768to1024", lambda lib, seed: linear_layer(lib, CNX_N, 768, 1024, seed)),
              ("convnext_t-256-head-bias_colsum", lambda lib, seed: head_bias_colsum(lib, CNX_N, seed))]


@pytest.mark.parametrize("case", range(len(CNX_CASES)), ids=[c[0] for c in CNX_CASES])
def test_convnext_t(lib, case):
    CNX_CASES[case][1](lib, 9000 + 7 * case)


# ============================================ the checkers reject a corrupted real output ============================================
def test_checkers_reject_a_corrupted_copy_of_real_outputs(lib):
    """One case per checker kind on a real kernel output at a benchmark shape (ResNet-50 64 -> 256 1x1 at 56 x 56): the
    kernel's own output passes, a copy with one wrong 64 x 64 block / ragged-tile row / in-tile row position does not.
    Only the copy is changed."""
    hip = _harness.hip()
    N, h, cin, cout = TRAIN_N, 56, 64, 256
    d = hip.conv_desc(N, h, h, cin, cout, 1, 1, 1, 0)
    x = rnd((N, h, h, cin), 11, relu=True)
    w = rnd((cout, 1, 1, cin), 12, scale=(2.0 / cin) ** 0.5)
    y = torch.empty(N, h, h, cout, dtype=torch.bfloat16, device=DEV)
    rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
    stats = torch.empty(rows, 2, cout, device=DEV)
    ok(lib.icamd_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None, stats.data_ptr(),
                            hip.stream_ptr()), "fwd")
    dy = rnd((N, h, h, cout), 13)
    ws, wsb = wgrad_ws(lib, d)
    dw = torch.empty(cout, cin, device=DEV)
    ok(lib.icamd_conv2d_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), wsb,
                              hip.stream_ptr()), "wgrad")
    sync()
    got, ref = f2(y), f2(R.conv2d_fwd(x, w, 1, 0, acc=F64))
    assert check_bf16(got, ref) == []
    M = got.shape[0]
    a = got.clone(); a[64 * 5000:64 * 5001, 128:192] *= 1.01
    assert check_bf16(a, ref) != []
    a = got.clone(); a[64 * 77:64 * 78, 0:64] *= -1
    assert check_bf16(a, ref) != []
    a = got.clone(); a[M - 1] = 0
    assert check_bf16(a, ref) != []
    a = got.clone(); pos = torch.arange(17, M, 64, device=DEV); a[pos] = got[pos - 1]
    assert check_bf16(a, ref) != []
    del a
    # sampled form of the same comparison
    from _fullsize_check import sample_rows
    rs = sample_rows(M, h * h, r=5, device=DEV)
    assert check_bf16(got, ref, rows=rs) == []
    a = got.clone(); a[M - 1] = 0
    assert check_bf16(a, ref, rows=rs) != []
    a = got.clone(); pos = torch.arange(17, M, 64, device=DEV); a[pos] = got[pos - 1]
    assert check_bf16(a, ref, rows=rs) != []
    del a, got, ref
    # fp32 filter gradient
    rw = R.conv2d_wgrad(x, dy, (1, 1), 1, 0, acc=F64).reshape(cout, cin)
    assert check_fp32(dw, rw) == []
    b = dw.clone(); b[64:128, 0:64] *= 1.01
    assert check_fp32(b, rw) != []
    b = dw.clone(); b[192:256, 0:64] *= -1
    assert check_fp32(b, rw) != []
    # BatchNorm statistics partials
    assert check_stats(stats, y) == []
    busiest = int(stats[:, 0].abs().sum(-1).argmax())      # (partial rows no workgroup owns are zero)
    st = stats.clone(); st[busiest] = 0
    assert check_stats(st, y) != []
    st = stats.clone(); st[:, 1, 100] *= 1.0001
    assert check_stats(st, y) != []
