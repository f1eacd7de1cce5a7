"""ConvNeXt V2 on the HIP kernels vs the CPU oracle (oracle/convnext_ref.py: bf16 rounding points, injected stochastic-depth
masks).  The yardsticks are those of tests/test_convnext_gpu.py: the oracle's own fp64 re-association noise."""
import numpy as np
import pytest
import torch

from _parity import assert_within, convnext_case, convnext_case_eval, convnext_case_step, convnext_pair, worst
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

C, B, HW = 10, 6, 64


@pytest.fixture(scope="module")
def case():
    """One oracle evaluation (fp32 with rounding points, and its fp64 twin) shared by the tests; nothing here is modified later."""
    return convnext_case("convnextv2_test", C, B, HW)


def test_forward_backward_matches_oracle(case):
    net = case["net"]
    s = convnext_case_step(case)
    print(f"convnextv2_test: logits err {s.err:.2e} (self-noise {s.noise:.2e})")
    for name, e, n in s.rows:
        if ".mlp.grn." in name:
            print(f"  {name}: err {e:.2e} (self-noise {n:.2e})")
    w = worst(s.rows)
    print(f"convnextv2_test: worst grad err {w[1]:.2e} at {w[0]}")
    assert_within(s)
    checked = [r[0] for r in s.rows]
    assert sum(".mlp.grn.weight" in n for n in checked) == 5 and sum(".mlp.grn.bias" in n for n in checked) == 5
    assert set(checked) == set(net.params)
    # a second backward with accumulate doubles the GRN gradients (and every other one)
    first = {n: net.grad_of(n).clone() for n in checked if ".mlp.grn." in n}
    net.backward_packed(s.ws, accumulate=True)
    torch.cuda.synchronize()
    for n, g1 in first.items():
        assert float(g1.abs().max()) > 0 and torch.allclose(net.grad_of(n), 2 * g1, rtol=1e-6, atol=0), n


def test_eval_forward_equals_the_oracles(case):
    err, noise = convnext_case_eval(case)
    print(f"convnextv2_test eval: logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert R.rel_l2(case["eval"], case["oracle"].out) > 1e-2  # the masks mattered: eval is another function than the training pass


def test_adamw_step_moves_the_grn_weights_and_an_epoch_is_finite():
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import Mixup, SoftTargetCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    _, net = convnext_pair("convnextv2_test", C, seed=3, drop_path=0.1)
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
