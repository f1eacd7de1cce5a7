"""ConvNeXt V2 on the HIP kernels vs the CPU oracle (tests/_convnextv2_ref.py: bf16 rounding points, injected stochastic-depth
masks).  The yardsticks are those of tests/test_convnext_gpu.py: the oracle's own fp64 re-association noise."""
import copy

import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from _convnextv2_ref import ConvNeXtV2Ref

pytestmark = pytest.mark.gpu

C, B, HW = 10, 6, 64


def _pair(seed=0, drop_path=0.2):
    from imageclassification_amd.convnext import ConvNeXt
    torch.manual_seed(seed)
    ref = ConvNeXtV2Ref("convnextv2_test", C, bf16_points=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if ".mlp.grn.weight" in n:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))             # GRN away from its zero init
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))             # (mlp.grn.bias among them)
            elif "norm" in n or n.startswith("stem.1") or "downsample.0" in n:
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif n.endswith("weight"):
                p.mul_(4.0)                                                  # std 0.08: activations of O(1)
    net = ConvNeXt("convnextv2_test", C, drop_path_rate=drop_path)
    net.load_state_dict(ref.state_dict())
    return ref, net


@pytest.fixture(scope="module")
def case():
    """One oracle evaluation (fp32 with rounding points, and its fp64 twin) shared by the tests; nothing here is modified later."""
    ref, net = _pair()
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
    # eval: no masks
    for blk in ref.all_blocks() + ref64.all_blocks():
        blk.keep = None
    with torch.no_grad():
        ev, ev64 = ref(x), ref64(x.double())
    return {"ref": ref, "ref64": ref64, "net": net, "keeps": keeps, "x": x, "y": y, "out": out.detach(), "out64": out64.detach(),
            "loss": float(loss), "eval": ev, "eval64": ev64}


def _step(case, accumulate=False, forward=True):
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
    net.backward_packed(ws, accumulate=accumulate)
    torch.cuda.synchronize()
    return ws, logits


def test_forward_backward_matches_oracle(case):
    ref, ref64, net, out, out64 = case["ref"], case["ref64"], case["net"], case["out"], case["out64"]
    ws, logits = _step(case)
    got = logits[:, :C].float().cpu()
    noise = R.rel_l2(out64.float(), out)
    err = R.rel_l2(got, out)
    print(f"convnextv2_test: logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert abs(float(ws["loss_rows"].mean()) - case["loss"]) <= 5e-3 * case["loss"]
    p64 = dict(ref64.named_parameters())
    worst, checked = ("", 0.0), []
    for name, p in ref.named_parameters():
        e = R.rel_l2(net.grad_of(name), p.grad)
        n = R.rel_l2(p64[name].grad.float(), p.grad)
        if ".mlp.grn." in name:
            print(f"  {name}: err {e:.2e} (self-noise {n:.2e})")
        if e > worst[1]:
            worst = (name, e)
        assert e <= 3.0 * max(n, 1e-2), (name, e, n)
        checked.append(name)
    print(f"convnextv2_test: worst grad err {worst[1]:.2e} at {worst[0]}")
    assert sum(".mlp.grn.weight" in n for n in checked) == 5 and sum(".mlp.grn.bias" in n for n in checked) == 5
    assert set(checked) == set(net.params)
    # a second backward with accumulate doubles the GRN gradients (and every other one)
    first = {n: net.grad_of(n).clone() for n in checked if ".mlp.grn." in n}
    net.backward_packed(ws, accumulate=True)
    torch.cuda.synchronize()
    for n, g1 in first.items():
        assert float(g1.abs().max()) > 0 and torch.allclose(net.grad_of(n), 2 * g1, rtol=1e-6, atol=0), n


def test_eval_forward_equals_the_oracles(case):
    net = case["net"]
    net.eval()
    got = net(case["x"].cuda()).float().cpu()
    torch.cuda.synchronize()
    net.train()
    noise = R.rel_l2(case["eval64"].float(), case["eval"])
    err = R.rel_l2(got, case["eval"])
    print(f"convnextv2_test eval: logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert R.rel_l2(case["eval"], case["out"]) > 1e-2        # the masks mattered: eval is another function than the training pass


def test_adamw_step_moves_the_grn_weights_and_an_epoch_is_finite():
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import Mixup, SoftTargetCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    _, net = _pair(seed=3, drop_path=0.1)
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
    for name in ("stages.0.blocks.0.mlp.grn.weight", "stages.2.blocks.1.mlp.grn.weight", "stages.3.blocks.0.mlp.grn.bias"):
        moved = (after[name] - before[name]).abs()
        assert float(moved.max()) > 1e-4 and bool(torch.isfinite(after[name]).all()), name      # one AdamW step is about lr
    stats = train_one_epoch(net, SoftTargetCrossEntropy(), data, opt, torch.device("cuda"), 1, NativeScalerWithGradNormCount(),
                            None, None, mix, start_steps=1, lr_schedule_values=[1e-3] * 3, wd_schedule_values=[5e-2] * 3,
                            num_training_steps_per_epoch=2, update_freq=1, use_amp=False, num_classes=C)
    assert np.isfinite(stats["loss"])
    assert all(bool(torch.isfinite(v).all()) for v in net.state_dict().values())
