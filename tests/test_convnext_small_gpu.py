"""The small ConvNeXt models (widths 40 / 80 / 160 / 320: no multiple of 32 in the first two stages) on the HIP kernels vs the CPU
oracles (oracle/convnext_ref.py and tests/_convnextv2_ref.py: bf16 rounding points, injected stochastic-depth masks, and their fp64
twins).  The bounds are those of tests/test_convnextv2_gpu.py: the oracle's own fp64 re-association noise is the yardstick.

convnext_test_narrow / convnextv2_test_narrow (depths 1, 1, 2, 1) at batch 6, 64 x 64, 10 classes: the depthwise kernels see
6 x 16 x 16 x 40, 6 x 8 x 8 x 80, 6 x 4 x 4 x 160 and 6 x 2 x 2 x 320, GRN sees C = 160 (and 320, 640, 1280).

The V2 names of narrow widths (convnextv2_test_narrow, convnextv2_nano here) are not in convnext.CONFIGS: tests/test_convnextv2_cpu.py
pins GRN_ARCHS to the oracle's five names and convnextv2_atto as a name train.py rejects.  The class and the kernels run them, so
these tests register them for the length of a constructor (tests/_convnext_narrow.py::narrow_registered) and take them out again."""
import copy

import numpy as np
import pytest
import torch

from _convnext_narrow import narrow_registered
from _convnextv2_ref import ConvNeXtV2Ref
from oracle import ops_ref as R
from oracle.convnext_ref import ConvNeXtRef

pytestmark = pytest.mark.gpu

C, B, HW = 10, 6, 64
ARCHS = ["convnext_test_narrow", "convnextv2_test_narrow"]


def _pair(arch, seed=0, drop_path=0.2):
    from imageclassification_amd.convnext import ConvNeXt
    torch.manual_seed(seed)
    ref = (ConvNeXtV2Ref if arch.startswith("convnextv2_") else ConvNeXtRef)(arch, C, bf16_points=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if ".mlp.grn.weight" in n:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))             # GRN away from its zero init
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("gamma"):
                p.copy_(0.3 + 0.4 * torch.rand(p.shape, generator=g))       # layer scale far from its 1e-6 init
            elif "norm" in n or n.startswith("stem.1") or "downsample.0" in n:
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif n.endswith("weight"):
                p.mul_(4.0)                                                  # std 0.08: activations of O(1)
    net = ConvNeXt(arch, C, drop_path_rate=drop_path)
    net.load_state_dict(ref.state_dict())
    return ref, net


@pytest.fixture(scope="module", params=ARCHS)
def case(request):
    """One oracle evaluation (fp32 with rounding points, and its fp64 twin) per model, shared by the tests; nothing here is modified
    later."""
    arch = request.param
    with narrow_registered():
        ref, net = _pair(arch)
    g = torch.Generator().manual_seed(5)
    keeps = [((torch.rand(B, generator=g) < 0.8).float() / 0.8) for _ in ref.all_blocks()]
    keeps[0] = None                                           # first block: rate 0
    for blk, k in zip(ref.all_blocks(), keeps):
        blk.keep = k
    ref64 = copy.deepcopy(ref).double()
    x = torch.randn(B, 3, HW, HW, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    out = ref(x)
    loss = torch.nn.functional.cross_entropy(out, y, label_smoothing=0.1)
    loss.backward()
    out64 = ref64(x.double())
    torch.nn.functional.cross_entropy(out64, y, label_smoothing=0.1).backward()
    for blk in ref.all_blocks() + ref64.all_blocks():        # eval: no masks
        blk.keep = None
    with torch.no_grad():
        ev, ev64 = ref(x), ref64(x.double())
    return {"arch": arch, "ref": ref, "ref64": ref64, "net": net, "keeps": keeps, "x": x, "y": y, "out": out.detach(),
            "out64": out64.detach(), "loss": float(loss), "eval": ev, "eval64": ev64}


def _step(case):
    from imageclassification_amd import hip
    net, x, y = case["net"], case["x"], case["y"]
    net.train()
    net.injected_keep = [torch.ones(B) if k is None else k for k in case["keeps"]]
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    yd = y.cuda()
    hip.check(net.lib.icamd_softmax_xent(ws["logits"].data_ptr(), net.ncls_p, B, C, yd.data_ptr(), None, 1.0, 0.1, 1.0 / B,
                                         ws["loss_rows"].data_ptr(), ws["pred"].data_ptr(), ws["dlogits"].data_ptr(),
                                         hip.stream_ptr()), "xent")
    net.backward_packed(ws)
    torch.cuda.synchronize()
    return ws, logits


def test_forward_backward_matches_oracle(case):
    arch, ref, ref64, net, out, out64 = case["arch"], case["ref"], case["ref64"], case["net"], case["out"], case["out64"]
    assert net.dims == (40, 80, 160, 320)
    ws, logits = _step(case)
    got = logits[:, :C].float().cpu()
    noise = R.rel_l2(out64.float(), out)
    err = R.rel_l2(got, out)
    print(f"{arch}: logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert abs(float(ws["loss_rows"].mean()) - case["loss"]) <= 5e-3 * case["loss"]
    p64 = dict(ref64.named_parameters())
    worst, checked = ("", 0.0), []
    for name, p in ref.named_parameters():
        e = R.rel_l2(net.grad_of(name), p.grad)
        n = R.rel_l2(p64[name].grad.float(), p.grad)
        if ".conv_dw." in name:
            print(f"  {name}: err {e:.2e} (self-noise {n:.2e})")
        if e > worst[1]:
            worst = (name, e)
        assert e <= 3.0 * max(n, 1e-2), (name, e, n)
        checked.append(name)
    print(f"{arch}: worst grad err {worst[1]:.2e} at {worst[0]}")
    assert set(checked) == set(net.params)
    # A second backward with accumulate doubles every gradient.  The accumulating launches fold their partial sums onto the prior
    # contents, another association of the same fp32 terms than the first pass's, so the double is exact only up to fp32
    # re-association: a few dozen partials at 2^-24 each, 1e-5 in rel-L2 with room to spare.  A lost or repeated accumulate is an
    # error of 0.5.  (The GRN vectors, one add per element, meet the rule of tests/test_convnextv2_gpu.py.)
    first = {n: net.grad_of(n).clone() for n in checked}
    net.backward_packed(ws, accumulate=True)
    torch.cuda.synchronize()
    worst2 = max((R.rel_l2(net.grad_of(n), 2 * g1), n) for n, g1 in first.items())
    print(f"{arch}: accumulate, worst distance from the double {worst2[0]:.2e} at {worst2[1]}")
    for n, g1 in first.items():
        assert float(g1.abs().max()) > 0 and R.rel_l2(net.grad_of(n), 2 * g1) <= 1e-5, n
        if ".mlp.grn." in n:
            assert torch.allclose(net.grad_of(n), 2 * g1, rtol=1e-6, atol=0), n


def test_eval_forward_equals_the_oracles(case):
    net = case["net"]
    net.eval()
    got = net(case["x"].cuda()).float().cpu()
    torch.cuda.synchronize()
    net.train()
    noise = R.rel_l2(case["eval64"].float(), case["eval"])
    err = R.rel_l2(got, case["eval"])
    print(f"{case['arch']} eval: logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert R.rel_l2(case["eval"], case["out"]) > 1e-2        # the masks mattered: eval is another function than the training pass


def test_adamw_step_moves_the_depthwise_weights_and_an_epoch_is_finite():
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import Mixup, SoftTargetCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    with narrow_registered():
        _, net = _pair("convnext_test_narrow", seed=3, drop_path=0.1)
    net.injected_keep = None
    before = net.state_dict()
    opt = create_optimizer("adamw", 1e-3, 5e-2, net)
    np.random.seed(0)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    g = torch.Generator().manual_seed(1)
    data = [(torch.randn(8, 3, HW, HW, generator=g), torch.randint(0, C, (8,), generator=g)) for _ in range(2)]
    stats = train_one_epoch(net, SoftTargetCrossEntropy(), data[:1], opt, torch.device("cuda"), 0, NativeScalerWithGradNormCount(),
                            None, None, mix, start_steps=0, lr_schedule_values=[1e-3, 1e-3], wd_schedule_values=[5e-2, 5e-2],
                            num_training_steps_per_epoch=1, update_freq=1, use_amp=False, num_classes=C)
    assert np.isfinite(stats["loss"]) and opt.step_count == 1
    after = net.state_dict()
    for name in ("stages.0.blocks.0.conv_dw.weight", "stages.1.blocks.0.conv_dw.weight", "stages.2.blocks.1.conv_dw.bias"):
        moved = (after[name] - before[name]).abs()
        assert float(moved.max()) > 1e-4 and bool(torch.isfinite(after[name]).all()), name      # one AdamW step is about lr
    stats = train_one_epoch(net, SoftTargetCrossEntropy(), data, opt, torch.device("cuda"), 1, NativeScalerWithGradNormCount(),
                            None, None, mix, start_steps=1, lr_schedule_values=[1e-3] * 3, wd_schedule_values=[5e-2] * 3,
                            num_training_steps_per_epoch=2, update_freq=1, use_amp=False, num_classes=C)
    assert np.isfinite(stats["loss"])
    assert all(bool(torch.isfinite(v).all()) for v in net.state_dict().values())


@pytest.mark.parametrize("arch", ["convnext_atto", "convnextv2_nano"])
def test_published_models_construct_and_run(arch):
    """convnext_atto through train.create_model; convnextv2_nano is not a registered name (module docstring), so the class is
    constructed with the name registered for the length of the constructor, and train.py rejects it."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train
    from imageclassification_amd import hip
    from imageclassification_amd.convnext import ConvNeXt
    if arch.startswith("convnextv2_"):
        with pytest.raises(ValueError):
            train.create_model(arch, 10)
        with narrow_registered():
            net = ConvNeXt(arch, 10)
        assert net.grn and net.dims == (80, 160, 320, 640)
    else:
        net = train.create_model(arch, 10)
    net.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    y = torch.randint(0, 10, (2,), generator=g).cuda()
    ws = net.pack(x)
    logits = net.forward_packed(ws)
    hip.check(net.lib.icamd_softmax_xent(ws["logits"].data_ptr(), net.ncls_p, 2, 10, y.data_ptr(), None, 1.0, 0.1, 0.5,
                                         ws["loss_rows"].data_ptr(), ws["pred"].data_ptr(), ws["dlogits"].data_ptr(),
                                         hip.stream_ptr()), "xent")
    net.backward_packed(ws)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits[:, :10].float()).all()) and bool(torch.isfinite(ws["loss_rows"]).all())
    for name in net.params:
        assert bool(torch.isfinite(net.grad_of(name)).all()), name
    assert float(net.grad_of("stages.0.blocks.0.conv_dw.weight").abs().max()) > 0
