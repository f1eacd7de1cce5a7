"""The small ConvNeXt models (widths 40 / 80 / 160 / 320: no multiple of 32 in the first two stages) on the HIP kernels vs the CPU
oracle of both versions (oracle/convnext_ref.py: bf16 rounding points, injected stochastic-depth masks, and its fp64 twin).  The
bounds are those of tests/test_convnextv2_gpu.py: the oracle's own fp64 re-association noise is the yardstick.

convnext_test_narrow / convnextv2_test_narrow (depths 1, 1, 2, 1) at batch 6, 64 x 64, 10 classes: the depthwise kernels see
6 x 16 x 16 x 40, 6 x 8 x 8 x 80, 6 x 4 x 4 x 160 and 6 x 2 x 2 x 320, GRN sees C = 160 (and 320, 640, 1280).

The V2 names of narrow widths (convnextv2_test_narrow, convnextv2_nano here) are not in convnext.CONFIGS: tests/test_convnextv2_cpu.py
pins GRN_ARCHS to the oracle's five names and convnextv2_atto as a name train.py rejects.  The class and the kernels run them, so
these tests register them for the length of a constructor (tests/_convnext_narrow.py::narrow_registered) and take them out again.
The oracle is built from the (depths, dims) pair itself."""
import numpy as np
import pytest
import torch

from _convnext_narrow import NARROW, narrow_registered
from _parity import (assert_within, convnext_case, convnext_case_eval, convnext_case_step, convnext_pair, worst,
                     xent_backward)
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

C, B, HW = 10, 6, 64
ARCHS = ["convnext_test_narrow", "convnextv2_test_narrow"]


@pytest.fixture(scope="module", params=ARCHS)
def case(request):
    """One oracle evaluation (fp32 with rounding points, and its fp64 twin) per model, shared by the tests; nothing here is modified
    later."""
    with narrow_registered():
        return convnext_case(request.param, C, B, HW, cfg=NARROW)


def test_forward_backward_matches_oracle(case):
    arch, net = case["arch"], case["net"]
    assert net.dims == (40, 80, 160, 320)
    s = convnext_case_step(case)
    ws = s.ws
    print(f"{arch}: logits err {s.err:.2e} (self-noise {s.noise:.2e})")
    for name, e, n in s.rows:
        if ".conv_dw." in name:
            print(f"  {name}: err {e:.2e} (self-noise {n:.2e})")
    w = worst(s.rows)
    print(f"{arch}: worst grad err {w[1]:.2e} at {w[0]}")
    assert_within(s)
    checked = [r[0] for r in s.rows]
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
    err, noise = convnext_case_eval(case)
    print(f"{case['arch']} eval: logits err {err:.2e} (self-noise {noise:.2e})")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert R.rel_l2(case["eval"], case["oracle"].out) > 1e-2  # the masks mattered: eval is another function than the training pass


def test_adamw_step_moves_the_depthwise_weights_and_an_epoch_is_finite():
    from imageclassification_amd.engine import train_one_epoch
    from imageclassification_amd.mixup import Mixup, SoftTargetCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    with narrow_registered():
        _, net = convnext_pair("convnext_test_narrow", C, seed=3, drop_path=0.1, cfg=NARROW)
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
    xent_backward(net, ws, y, 10, smoothing=0.1)
    assert bool(torch.isfinite(logits[:, :10].float()).all()) and bool(torch.isfinite(ws["loss_rows"]).all())
    for name in net.params:
        assert bool(torch.isfinite(net.grad_of(name)).all()), name
    assert float(net.grad_of("stages.0.blocks.0.conv_dw.weight").abs().max()) > 0
