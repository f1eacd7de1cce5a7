"""MobileNetV2 on the HIP kernels against oracle/mobilenet_ref.py::MobileNetV2Ref with the rounding points of the HIP path, under the
yardstick protocol of tests/_resnet_parity.py: the reference's own fp64 copy sets the noise every bound is a multiple of.
The gradients are held a second time under teacher forcing (tests/_parity.py::forced_check), where that noise is capped at 8e-3 /
2.5e-2.

mobilenetv2_test: stem 16; ds -> 8; ir (r2, s2) -> 16; ir (r1, s2) -> 24; ir (r2, s1) -> 32; head 64 -- a stride-2 block, stride-1
blocks with and without residual, the depthwise-separable block.  Input 64 x 64, batch 8, 10 classes: the feature maps are 32, 32, 16,
8, 8, so the last BatchNorms (blocks.3.*, the head) see 8 x 8 x 8 = 512 values per channel and none sees fewer."""
import copy
import pickle

import numpy as np
import pytest
import torch

from _parity import forced_check, mobilenet_pair, xent_backward
from _resnet_parity import assert_hip_within_yardstick, hip_rows, parity_batch, yardstick
from oracle import ops_ref as R
from oracle.mobilenet_ref import MobileNetV2Ref, param_count

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ARCH, C, B, HW = "mobilenetv2_test", 10, 8, 64
SMOOTHING = 0.1


def _net(arch=ARCH, num_classes=C):
    from imageclassification_amd.mobilenet import MobileNetV2
    return MobileNetV2(arch, num_classes)


def _pair(perturbed, seed=0):
    return mobilenet_pair(ARCH, C, perturbed, seed)


@pytest.mark.parametrize("perturbed", [False, True], ids=["timm_default_init", "perturbed_batchnorm"])
def test_one_training_step_and_eval_logits(perturbed):
    ref, net = _pair(perturbed)
    sd = net.state_dict()
    assert list(sd) == list(ref.state_dict()) and all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    x, y = parity_batch(C, B, HW)
    twin = copy.deepcopy(ref).double()           # for the eval pass below: takes the same training forward, in fp64
    trace = []
    ref.set_trace(trace)
    yard = yardstick(ref, x, y, SMOOTHING)
    ref.set_trace(None)
    at6 = float((torch.cat([t.flatten() for t in trace]) == 6).float().mean())
    print(f"{at6:.2%} of the expanded activations clamped at 6; yardstick: logits noise {yard.noise_logits:.2e}, mean gradient noise "
          f"{yard.mean_noise:.2e}, worst {yard.worst_noise[1]:.2e} at {yard.worst_noise[0]}")
    if perturbed:
        assert at6 >= 0.01
    got = hip_rows(net, x, y, C, SMOOTHING, yard)
    print(f"HIP: logits err {got.err_logits:.2e}, loss {got.loss:.5f} vs {yard.loss:.5f}, mean gradient err {got.mean_err:.2e}, worst "
          f"{got.worst[1]:.2e} (noise {got.worst[2]:.2e}) at {got.worst[0]}; {got.zero_branch} zero-gradient tensors")
    assert len(got.rows) + got.zero_branch == len(list(ref.named_parameters()))
    assert_hip_within_yardstick(yard, got)
    # What that yardstick is worth here: every stored tensor is a bf16 rounding point, a difference d in front of one leaves about
    # sqrt(4e-3 d) behind it, so two runs that sum in different orders drift apart layer by layer until they differ at bf16's own level
    # and ReLU6 masks flip: the reference and its fp64 copy agree to 10-20 % on most gradients, and the protocol above is that wide.
    # So the gradients are held a second time under TEACHER FORCING (oracle/mobilenet_ref.py::Tape, tests/_parity.py): the reference runs on the HIP
    # path's own stored tensors -- input, every convolution output, a2, block outputs, head, pooled, logits --, so masks and batch
    # statistics are those of the same numbers and nothing drifts.  Its yardstick is the same construction between the reference and
    # its fp64 copy; that one is capped, and so is what it admits.
    forced_check(ref, net, MobileNetV2Ref(ARCH, C, bf16_points=False).double(), x, y, SMOOTHING, negligible=6 if perturbed else 12,
                 n_params=59)
    assert net.num_batches_tracked == 1
    # eval-mode logits after that step, every side on its own running statistics; the yardstick is again the fp64 twin, which took
    # the same training forward
    twin.train()
    with torch.no_grad():
        twin(x.double())
    ref.eval()
    twin.eval()
    with torch.no_grad():
        ev, ev64 = ref(x), twin(x.double()).float()
    net.eval()
    hv = net(x.cuda()).float().cpu()
    torch.cuda.synchronize()
    net.train()
    err, noise = R.rel_l2(hv, ev), R.rel_l2(ev64, ev)
    print(f"eval logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 1e-3)
    # ... and those running statistics themselves, tensor by tensor, by the per-tensor rule of assert_hip_within_yardstick (three times
    # the fp64 copy's distance) with the 1e-3 floor of its logits rule: a running statistic is a tenth of a batch statistic, which is a
    # mean over the tensors whose drift the logits bound already allows.  A mean is measured in
    # units of its channel's standard deviation: the head's BatchNorm sees zero-mean inputs, its running mean is rounding noise.
    tsd, nsd, rsd = twin.state_dict(), net.state_dict(), ref.state_dict()
    for k, v in rsd.items():
        if k.endswith(("running_mean", "running_var")):
            unit = torch.linalg.vector_norm(rsd[k.replace("running_mean", "running_var")].double().sqrt() if k.endswith("mean") else v.double())
            e, n = float(torch.linalg.vector_norm(nsd[k].double() - v) / unit), float(torch.linalg.vector_norm(tsd[k] - v) / unit)
            assert e <= 3.0 * max(n, 1e-3), (k, e, n)


def test_on_load_and_plain_routes_give_the_same_bits(monkeypatch):
    """mobilenet.DW_ONLOAD, all four settings: the logits and the whole gradient arena of one training step are the same bits"""
    from imageclassification_amd import mobilenet
    _, net = _pair(True, seed=6)
    x, y = parity_batch(C, B, HW)
    seen = []
    for fwd, wgrad in ((True, True), (False, False), (True, False), (False, True)):
        monkeypatch.setattr(mobilenet, "DW_ONLOAD", {"fwd": fwd, "wgrad": wgrad})
        net.train()
        ws = net.pack(x.cuda())
        logits = net.forward_packed(ws).clone()
        xent_backward(net, ws, y.cuda(), C, SMOOTHING)
        seen.append((logits, net.grad_arena.clone()))
    assert float(seen[0][1].abs().max()) > 0
    for logits, grads in seen[1:]:
        assert torch.equal(logits, seen[0][0]) and torch.equal(grads, seen[0][1])


def _loader(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 3, HW, HW, generator=g), torch.randint(0, C, (B,), generator=g)) for _ in range(n)]


def _train(net, opt, loader, crit=None, mixup_fn=None, update_freq=1, lr=1e-6):
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    steps = len(loader) // update_freq
    return train_one_epoch(net, crit or LabelSmoothingCrossEntropy(0.1), loader, opt, DEV, 0, NativeScalerWithGradNormCount(), None,
                           None, mixup_fn, start_steps=0, lr_schedule_values=[lr] * steps, wd_schedule_values=[5e-4] * steps,
                           num_training_steps_per_epoch=steps, update_freq=update_freq, use_amp=True, num_classes=C)


def test_engine_two_steps_mixup_and_evaluate():
    from imageclassification_amd.engine import evaluate
    from imageclassification_amd.mixup import Mixup, SoftTargetCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    _, net = _pair(True, seed=2)
    opt = create_optimizer("adamw", 1e-6, 5e-4, net)
    np.random.seed(3)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    before = net.param_arena.clone()
    stats = _train(net, opt, _loader(2, 24), crit=SoftTargetCrossEntropy(), mixup_fn=mix)
    assert set(stats) == {"loss", "class_acc"} and np.isfinite(stats["loss"]) and stats["loss"] > 0.5
    assert net.num_batches_tracked == 4          # the accuracy-only second forward of every step is a training forward
    assert opt.step_count == 2 and not torch.equal(net.param_arena, before) and bool(torch.isfinite(net.param_arena).all())
    ev = evaluate(_loader(2, 25), net, DEV, C)
    assert np.isfinite(ev["loss"]) and 0.0 <= ev["acc1"] <= 100.0
    assert net.num_batches_tracked == 4          # evaluate ran in eval mode


def test_engine_update_freq_accumulates_two_single_steps():
    from imageclassification_amd import hip
    from imageclassification_amd.optim_factory import create_optimizer
    _, net = _pair(True, seed=4)
    opt = create_optimizer("adamw", 0.0, 0.0, net)
    data = _loader(4, 26)                        # two optimizer steps of two micro-batches each
    # expected in the arena at the end: the LAST window's two micro-batch gradients, each scaled 1 / (B * 2), summed on the host
    net.train()
    expect = torch.zeros_like(net.grad_arena)
    for x, y in data[2:]:
        ws = net.pack(x.cuda())
        net.forward_packed(ws)
        hip.check(net.lib.icamd_softmax_xent(ws["logits"].data_ptr(), net.ncls_p, B, C, y.cuda().data_ptr(), None, 1.0, 0.1, 1.0 / (B * 2),
                                             ws["loss_rows"].data_ptr(), ws["pred"].data_ptr(), ws["dlogits"].data_ptr(),
                                             hip.stream_ptr()), "xent")
        net.backward_packed(ws, accumulate=False)
        torch.cuda.synchronize()
        expect += net.grad_arena
    before = net.param_arena.clone()
    stats = _train(net, opt, data, update_freq=2, lr=0.0)
    got = net.grad_arena.clone()
    assert np.isfinite(stats["loss"]) and opt.step_count == 2
    assert torch.equal(net.param_arena, before)                                  # lr = 0, weight decay 0
    assert float(expect.abs().max()) > 0 and bool(torch.isfinite(got).all())
    print(f"accumulated gradient against the two single steps: rel_l2 {R.rel_l2(got.cpu(), expect.cpu()):.2e}")
    assert R.rel_l2(got.cpu(), expect.cpu()) <= 1e-5                             # the same kernels on the same weights: fp32 sums


def test_checkpoint_round_trip(tmp_path):
    from imageclassification_amd.checkpoint import DeferredModel
    _, net = _pair(True, seed=5)
    x, y = parity_batch(C, B, HW)
    net.train()
    ws = net.pack(x.cuda())
    net.forward_packed(ws)                       # moves the running statistics and the batch counter
    torch.cuda.synchronize()
    sd = net.state_dict()
    net.eval()
    want = net(x.cuda()).float().cpu()
    path = tmp_path / "mobilenetv2.pth"
    torch.save({"model": net}, path)
    back = torch.load(path, map_location="cpu", weights_only=False)["model"]
    assert isinstance(back, DeferredModel)
    assert list(back.state_dict()) == list(sd) and all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())
    live = pickle.loads(pickle.dumps(back)).materialise()
    assert live.arch == ARCH and live.num_classes == C and live.num_batches_tracked == 1
    live.eval()
    assert torch.equal(live(x.cuda()).float().cpu(), want)
    # the depthwise filter survives the arena layout [3][3][C] both ways
    k = "blocks.1.0.conv_dw.weight"
    assert sd[k].shape == (48, 1, 3, 3)
    other = _net()
    other.load_state_dict(sd)
    assert torch.equal(other.state_dict()[k], sd[k])


@pytest.mark.parametrize("arch", ["mobilenetv2_035", "mobilenetv2_140"])
def test_width_multiplier_paths(arch):
    net = _net(arch, 1000)
    assert sum(v.numel() for k, v in net.state_dict().items() if k in net.params) == param_count(arch)
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(2, 3, 32, 32, generator=g), torch.randint(0, 1000, (2,), generator=g)
    net.train()
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    assert logits.shape == (2, net.ncls_p) and net.feat_dim == (1792 if arch.endswith("140") else 1280)
    loss = xent_backward(net, ws, y.cuda(), 1000, 0.1)
    assert np.isfinite(loss) and bool(torch.isfinite(logits.float()).all())
    assert bool(torch.isfinite(net.grad_arena).all()) and float(net.grad_arena.abs().max()) > 0
    for name in ("conv_stem.weight", "blocks.1.0.conv_pw.weight", "blocks.1.0.conv_dw.weight", "blocks.6.0.bn3.weight", "classifier.bias"):
        assert float(net.grad_of(name).abs().max()) > 0, name
