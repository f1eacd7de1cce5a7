"""Parity at BASELINE.json's FULL sizes (batch 256, 3x224x224, 1000 classes), where the CPU oracle would take minutes per
step: size-independent properties of the step instead of element-wise comparison.

* reproducibility: the same step from the same state twice gives bit-identical loss rows and gradients (the build's
  claim of fixed-order reductions, incl. the weight-gradient stream running beside the main stream);
* softmax-cross-entropy: every row of dlogits sums to zero (sum_c (p_c - t_c) = 0 for smoothed / mixed targets);
* eval forward: a sample's logits do not depend on which batch it sits in (ResNet-50 with BatchNorm folded, batch 256 vs
  its first 32 images) -- different tile decompositions and kernel routings, same numbers to bf16 rounding;
* ViT-B/16 (no batch statistics): the gradient of the 256-image batch is the mean of the gradients of its two halves
  (1/B is a power of two, so the only difference is fp32 summation order) -- the identity data parallelism rests on;
* BatchNorm in train mode: the batch statistics written by the step are those of the stored conv output (fp64 check on
  the stem: 256 x 112 x 112 x 64 values);
* BASELINE configs[4] at its own size -- ConvNeXt-T, batch 256, mixup / cutmix soft targets, stochastic depth, AdamW + EMA:
  the mixed step twice is bit-identical, every dlogits row sums to zero for the soft targets, a cutmix step equals the step
  on the explicitly pasted images, and the EMA recursion holds on the trajectory train_one_epoch produces.
"""
import pytest
import torch

from _parity import xent_backward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, HW, C = 256, 224, 1000


def _step(net, x, y, smoothing=0.1):
    ws = net.pack(x)
    net.forward_packed(ws)
    xent_backward(net, ws, y, C, smoothing)
    return ws


def _data(n=B, seed=88):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, HW, HW, generator=g).to(DEV), torch.randint(0, C, (n,), generator=g).to(DEV)


def test_resnet50_full_batch_step_is_reproducible_and_consistent():
    from imageclassification_amd.nets import ResNet
    net = ResNet("resnet50", C, seed=3, zero_init_last=False)
    x, y = _data()
    buf0 = net.buffer_arena.clone()
    ws = _step(net, x, y)
    loss1, grad1, dl1 = ws["loss_rows"].clone(), net.grad_arena.clone(), ws["dlogits"].clone()
    assert torch.isfinite(loss1).all() and torch.isfinite(grad1).all()
    # (1) every row of dlogits sums to zero (over the real classes; the 24 padding columns are zero)
    rows = dl1.float()[:, :C].double().sum(1)
    assert float(rows.abs().max()) <= 2e-3 * float(dl1.float().abs().max()) * 8     # bf16 rounding of 1000 terms
    assert float(dl1.float()[:, C:].abs().max()) == 0.0
    # (2) BatchNorm statistics of the stem equal those of the stored conv output (fp64)
    y0 = ws["y0"].double().reshape(-1, 64)
    st = net.stat_arena[net.stem_bn.stat_offset: net.stem_bn.stat_offset + 4 * 64].double()
    mean, var = y0.mean(0), y0.var(0, unbiased=False)
    assert torch.allclose(st[:64], mean.to(DEV), rtol=1e-5, atol=1e-6)
    assert torch.allclose(st[64:128], 1.0 / torch.sqrt(var + 1e-5).to(DEV), rtol=1e-5)
    # (3) same state, same batch again: bit-identical
    net.buffer_arena.copy_(buf0)
    ws = _step(net, x, y)
    assert torch.equal(ws["loss_rows"], loss1) and torch.equal(ws["dlogits"], dl1)
    assert torch.equal(net.grad_arena, grad1)
    # (4) eval forward: sample i's logits are the same in a batch of 256 and in a batch of 32
    net.eval()
    full = net(x).float().clone()
    part = net(x[:32]).float()
    err = (full[:32] - part).abs().max().item()
    assert err <= 2.0 ** -7 * full.abs().max().item(), err      # 1 bf16 ulp of the largest logit
    # and folded vs unfolded eval paths agree at the full size
    net.fold_eval = False
    plain = net(x).float()
    rel = ((plain - full).norm() / full.norm()).item()
    assert rel <= 2e-2, rel


def test_vit_base_full_batch_gradient_is_the_mean_of_its_halves():
    from imageclassification_amd.vit import VisionTransformer
    net = VisionTransformer("vit_base_patch16_224", C, seed=4)
    x, y = _data(seed=89)
    _step(net, x, y)
    g_full = net.grad_arena.double().clone()
    _step(net, x[:128].contiguous(), y[:128].contiguous())
    g_a = net.grad_arena.double().clone()
    _step(net, x[128:].contiguous(), y[128:].contiguous())
    g_b = net.grad_arena.double().clone()
    mean = 0.5 * (g_a + g_b)
    rel = ((g_full - mean).norm() / mean.norm()).item()
    assert rel <= 1e-5, rel
    # twice the same step: bit-identical
    _step(net, x, y)
    assert torch.equal(net.grad_arena.double(), g_full)


def _mixed_step(net, x, y, mix, smoothing=0.1, seed=7):
    """One ConvNeXt step on a mixed batch: (mode, lam, box) applied inside the packing kernel, soft targets
    lam*onehot_s(y) + (1-lam)*onehot_s(y.flip(0)) inside the loss kernel; stochastic-depth masks drawn from torch's CPU RNG."""
    from imageclassification_amd import hip
    lib = hip.load()
    torch.manual_seed(seed)                      # the per-sample stochastic-depth masks of this step
    ws = net.pack(x, mix)
    logits = net.forward_packed(ws)
    n = x.shape[0]
    flipped = y.flip(0).contiguous()
    hip.check(lib.icamd_softmax_xent(logits.data_ptr(), net.ncls_p, n, C, y.data_ptr(), flipped.data_ptr(), float(mix[1]),
                                     smoothing, 1.0 / n, ws["loss_rows"].data_ptr(), ws["pred"].data_ptr(),
                                     ws["dlogits"].data_ptr(), hip.stream_ptr()), "xent")
    net.backward_packed(ws)
    torch.cuda.synchronize()
    return ws


def test_convnext_tiny_config4_full_batch_properties():
    """BASELINE configs[4] at full size: ConvNeXt-T, batch 256 x 224^2, mixup 0.8 / cutmix 1.0 / label smoothing 0.1 soft
    targets, drop-path 0.05, AdamW + ModelEmaV3(0.9995) (reference recipe train.py:172-201, loop engine.py:44-77)."""
    import numpy as np
    from imageclassification_amd.convnext import ConvNeXt
    from imageclassification_amd.ema import ModelEmaV3
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import Mixup, SoftTargetCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    net = ConvNeXt("convnext_tiny", C, drop_path_rate=0.05, seed=3)
    x, y = _data(seed=90)
    # (1) a mixup step and a cutmix step: finite, rows of dlogits sum to zero for the soft targets, bit-reproducible
    box = (40, 150, 64, 200)                                           # yl, yh, xl, xh
    lam_cut = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(HW * HW)
    for mix in ((1, 0.37, (0, 0, 0, 0)), (2, lam_cut, box)):
        ws = _mixed_step(net, x, y, mix)
        loss1, grad1, dl1 = ws["loss_rows"].clone(), net.grad_arena.clone(), ws["dlogits"].clone()
        assert torch.isfinite(loss1).all() and torch.isfinite(grad1).all() and float(grad1.abs().max()) > 0
        rows = dl1.float()[:, :C].double().sum(1)
        assert float(rows.abs().max()) <= 2e-3 * float(dl1.float().abs().max()) * 8, mix
        assert float(dl1.float()[:, C:].abs().max()) == 0.0
        ws = _mixed_step(net, x, y, mix)
        assert torch.equal(ws["loss_rows"], loss1) and torch.equal(ws["dlogits"], dl1) and torch.equal(net.grad_arena, grad1)
        if mix[0] == 2:
            # the fused cutmix equals an un-mixed step on explicitly pasted images with the same soft targets
            pasted = x.clone()
            pasted[:, :, box[0]:box[1], box[2]:box[3]] = x.flip(0)[:, :, box[0]:box[1], box[2]:box[3]]
            ws = _mixed_step(net, pasted, y, (0, lam_cut, (0, 0, 0, 0)))
            assert torch.equal(ws["loss_rows"], loss1) and torch.equal(net.grad_arena, grad1)
    # (2) the composition through the drop-in boundary: 3 steps of train_one_epoch with mixup_fn + EMA; the EMA recursion
    # ema <- ema + (1 - decay) * (p - ema) holds on the trajectory (parameters AND the lerp are the fused kernel's)
    decay = 0.9995
    ema = ModelEmaV3(net, decay=decay)
    opt = create_optimizer("adamw", 1e-3, 5e-2, net)
    np.random.seed(5)
    mixer = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    expect = net.param_arena.clone()
    xc, yc = x.cpu(), y.cpu()
    moved = 0.0
    for i in range(3):
        before = net.param_arena.clone()
        st = train_one_epoch(net, SoftTargetCrossEntropy(), [(xc, yc)], opt, DEV, 0, NativeScalerWithGradNormCount(), None, ema,
                             mixer, start_steps=i, lr_schedule_values=[1e-3] * 3, wd_schedule_values=[5e-2] * 3,
                             num_training_steps_per_epoch=1, update_freq=1, use_amp=True, num_classes=C)
        # ~ln(1000) at init; the same 256 images again at lr 1e-3 are memorised fast (4.3 at the third step, measured)
        assert np.isfinite(st["loss"]) and (6.0 if i == 0 else 1.0) < st["loss"] < 8.0 and 0.0 <= st["class_acc"] <= 1.0
        expect = expect + (1.0 - decay) * (net.param_arena - expect)
        moved += float((net.param_arena - before).abs().max())
    assert moved > 0 and opt.steps_taken == 3
    assert torch.allclose(ema.param_arena, expect, rtol=1e-6, atol=1e-9)
    assert float((ema.param_arena - net.param_arena).abs().max()) > 0      # the EMA lags the model: it is not a copy
