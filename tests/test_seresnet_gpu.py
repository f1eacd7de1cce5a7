"""SE-ResNet / SE-ResNeXt on the GPU: whole-network parity of seresnet50 and seresnext50_32x4d against the oracle
(oracle/resnet_ref.py) by the protocol of tests/test_resnet_family_gpu.py; the deepest members take one finite step; eval (folded
and unfolded), state_dict, engine, reproducibility and the command line for seresnet50."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from oracle import ops_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _resnet_parity import (assert_hip_within_yardstick, hip_rows, parity_batch, perturbed_bn_pair, timm_default_pair,  # noqa: E402
                            xent_backward, yardstick)
from oracle.resnet_ref import ResNetRef  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


# arch, gamma_last, yardstick caps (logits, gradient mean, gradient worst)
PARITY = [
    ("seresnet50", 0.0, (5e-3, 4.5e-2, 7e-2)),
    ("seresnet50", 0.02, (8e-3, 0.13, 0.22)),
    ("seresnext50_32x4d", 0.02, (8e-3, 0.13, 0.22)),
]


@pytest.mark.parametrize("arch,gamma_last,caps", PARITY)
def test_whole_network_parity_well_conditioned(arch, gamma_last, caps):
    """Batch 32 at 128 x 128, 100 classes, label smoothing 0.1, timm-default init; the last BatchNorm weight of every block at 0
    (49 tensors compared; the 11 tensors of every block's main branch, its four SE tensors included, exactly zero on both sides)
    or at 0.02 (all 225 compared).  The yardstick -- the reference against its own fp64 copy -- is asserted first under the family
    test's caps, which are conditions (measured on a CPU for seresnet50: logits 2.9e-3 / mean 2.4e-2 / worst 3.5e-2 at gamma 0
    and 4.3e-3 / 7.6e-2 / 0.135 at 0.02; seresnext50_32x4d 3.6e-3 / 7.0e-2 / 0.131); an all-zero gradient scores 1.0.  Then the HIP path: logits <= 2 max(noise, 1e-3), loss to
    1e-3, mean gradient error <= 2 max(mean noise, 1e-3), per tensor <= 3 max(its noise, 5e-3)."""
    C, B, HW = 100, 32, 128
    ref, net = timm_default_pair(arch, C, gamma_last=gamma_last)
    x, y = parity_batch(C, B, HW)
    yard = yardstick(ref, x, y, 0.1)
    got = hip_rows(net, x, y, C, 0.1, yard)
    rows, zero_branch, worst, worst_n = got.rows, got.zero_branch, got.worst, yard.worst_noise
    print(f"{arch} B={B} {HW}x{HW} gamma_last={gamma_last}: logits err {got.err_logits:.2e} (self-noise {yard.noise_logits:.2e}); "
          f"loss {got.loss:.6f} vs {yard.loss:.6f}; {len(rows)} gradient tensors: mean err {got.mean_err:.2e} (self-noise "
          f"{yard.mean_noise:.2e}), worst {worst[0]} {worst[1]:.2e} (its self-noise {worst[2]:.2e}), yardstick worst "
          f"{worst_n[0]} {worst_n[1]:.2e}; {zero_branch} zero-gradient branch tensors exact")
    for name, e, n in rows:
        if ".se." in name:
            print(f"    {name:28s} HIP {e:.2e} yardstick {n:.2e}")
    # the yardstick itself
    cap_logits, cap_mean, cap_worst = caps
    assert yard.noise_logits <= cap_logits and yard.mean_noise <= cap_mean and worst_n[1] <= cap_worst, \
        (yard.noise_logits, yard.mean_noise, worst_n)
    if gamma_last:
        assert zero_branch == 0 and len(rows) == 225                 # every parameter tensor has a non-zero gradient
    else:
        assert zero_branch == 176 and len(rows) == 49                # 11 per block
    # the HIP path against it
    assert_hip_within_yardstick(yard, got)


@pytest.mark.parametrize("arch", ["seresnet152", "seresnext101_32x4d"])
def test_deeper_members_take_one_finite_step(arch):
    from imageclassification_amd.nets import ResNet
    C, B, HW = 10, 4, 64
    net = ResNet(arch, C, seed=3, zero_init_last=False)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 3, HW, HW, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    net.train()
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    loss = xent_backward(net, ws, y.cuda(), C, smoothing=0.1)
    assert torch.isfinite(logits[:, :C].float()).all() and loss == loss and abs(loss) < 1e3
    assert torch.isfinite(net.grad_arena).all()
    for name in ("conv1.weight", "layer3.20.se.fc2.weight", "layer4.2.se.fc1.bias", "layer4.2.conv3.weight", "fc.weight"):
        assert float(net.grad_of(name).abs().max()) > 0.0, name


def test_seresnet50_eval_folded_and_state_dict_round_trip():
    """Batch 4 at 64 x 64, timm-default affine parameters, random running statistics; folded and unfolded eval logits against the
    reference's fp32 arithmetic, <= 1e-2 each (the family test's bound).  The reference with the bf16 rounding points is itself
    6.7e-3 .. 8.8e-3 from its fp32 arithmetic at this setting (measured on a CPU, three inputs; the gate halves every branch, so
    the rounding of the shortcut chain weighs more than in ResNet-50: 5.7e-3 .. 6.7e-3 there); with the BatchNorm weights
    also drawn from U(0.5, 1.5), as the ResNeXt test does, it is at 1.1e-2 .. 1.4e-2, above the bound, so that setting cannot
    be held to it.  The distance to the bf16-points reference is printed.  Over weight draws that distance swings between 5.0e-3
    and 1.1e-2 (seeds 4 .. 12).  The folded path rounds at other points than the reference, so its distance d' from the fp32
    arithmetic is a second sample of the same noise, up to sqrt(2) d for two independent errors of size d: the bound holds only
    where d <= 1e-2 / 1.5, asserted first as <= 6.5e-3.  Seed 10 (5.0e-3) is the first seed from 4 up that meets it.  Seed 4 did
    while the oracle still constructed layers it threw away; dropping them moved the seeded draw (7.4e-3, folded HIP path
    1.05e-2)."""
    from imageclassification_amd.nets import ResNet
    C = 10
    ref, net, sd = perturbed_bn_pair("seresnet50", C, seed=10, affine=False)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(10))
    exact = ResNetRef("seresnet50", C, bf16_points=False, zero_init_last=False)   # the reference's fp32 arithmetic
    exact.load_state_dict(sd)
    exact.eval()
    net.eval()
    ref.eval()
    with torch.no_grad():
        want = exact(x)
        rounded = ref(x)
    assert R.rel_l2(rounded, want) <= 6.5e-3          # the condition under which the bound below can be held
    assert net.fold_eval
    folded = net(x.cuda()).float().cpu()
    net.fold_eval = False
    unfolded = net(x.cuda()).float().cpu()
    net.fold_eval = True
    e_fold, e_plain = R.rel_l2(folded, want), R.rel_l2(unfolded, want)
    print(f"seresnet50 eval logits vs fp32 reference: folded {e_fold:.2e}, separate BatchNorm pass {e_plain:.2e}; the bf16-points "
          f"reference {R.rel_l2(rounded, want):.2e}; against it: folded {R.rel_l2(folded, rounded):.2e}, separate "
          f"{R.rel_l2(unfolded, rounded):.2e}")
    assert e_fold <= 1e-2 and e_plain <= 1e-2
    # state_dict -> load_state_dict: bit-exact, the key order included
    out = net.state_dict()
    assert list(out) == list(sd)
    assert tuple(out["layer1.0.se.fc1.weight"].shape) == (16, 256, 1, 1)
    assert tuple(out["layer4.2.se.fc2.weight"].shape) == (2048, 128, 1, 1)
    for k in sd:
        assert torch.equal(out[k].float(), sd[k].float()), k
    net2 = ResNet("seresnet50", C, seed=99)
    net2.load_state_dict(out)
    assert torch.equal(net2.param_arena, net.param_arena) and torch.equal(net2.buffer_arena, net.buffer_arena)
    assert torch.equal(net2.shadow, net.shadow)
    # timm's init: Kaiming-normal (fan_out) SE weights, nn.Conv2d's default bias range, the last BatchNorm weight zeroed
    fresh = ResNet("seresnet50", C, seed=1).state_dict()
    assert abs(float(fresh["layer3.0.se.fc2.weight"].std()) / (2.0 / 1024) ** 0.5 - 1.0) <= 0.05
    assert abs(float(fresh["layer3.0.se.fc1.weight"].std()) / (2.0 / 64) ** 0.5 - 1.0) <= 0.05
    b = fresh["layer3.0.se.fc2.bias"]
    assert 0.5 / 64 ** 0.5 < float(b.abs().max()) <= 1.0 / 64 ** 0.5 and abs(float(b.mean())) < 0.3 / 64 ** 0.5
    assert float(fresh["layer3.0.bn3.weight"].abs().max()) == 0.0


def test_seresnet50_engine_step_evaluate_and_bitwise_repeat():
    """As the ResNeXt test: the loss is compared at a well-conditioned setting (every block's last BatchNorm weight at 0.02); the
    yardstick (reference against its fp64 copy) is asserted <= 1e-3 on the loss before the HIP path is held to 5e-3."""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.nets import ResNet
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    from oracle import engine_ref as E
    C, B = 10, 8
    torch.manual_seed(0)
    ref = ResNetRef("seresnet50", C, bf16_points=True, zero_init_last=False)
    for n, m in ref.named_modules():
        if n.endswith("bn3"):
            m.weight.data.fill_(0.02)
    net = ResNet("seresnet50", C)
    net.load_state_dict(ref.state_dict())
    start = copy.deepcopy(ref.state_dict())
    g = torch.Generator().manual_seed(21)
    data = [(torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, C, (B,), generator=g))]
    # the step twice from the same state: loss, logits and the whole gradient arena bit-identical
    net.train()
    runs = []
    for _ in range(2):
        ws = net.pack(data[0][0].cuda())
        net.forward_packed(ws)
        loss = xent_backward(net, ws, data[0][1].cuda(), C, smoothing=0.1)
        runs.append((loss, net.grad_arena.clone(), ws["logits"].clone()))
        net.load_state_dict(ref.state_dict())      # running statistics back to the start
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().max()) > 0.0
    ref64 = copy.deepcopy(ref).double()
    ref.train(); ref64.train()
    with torch.no_grad():
        ref_loss = float(torch.nn.functional.cross_entropy(ref(data[0][0]), data[0][1], label_smoothing=0.1))
        loss64 = float(torch.nn.functional.cross_entropy(ref64(data[0][0].double()).float(), data[0][1], label_smoothing=0.1))
    ref.load_state_dict(start)                         # the reference's running statistics back to the start as well
    print(f"seresnet50 B={B} 64x64: loss HIP {runs[0][0]:.6f}, reference {ref_loss:.6f}, its fp64 copy {loss64:.6f}")
    assert abs(loss64 - ref_loss) <= 1e-3 * abs(ref_loss)          # the yardstick itself
    assert abs(runs[0][0] - ref_loss) <= 5e-3 * abs(ref_loss)
    # one engine step + evaluate: the reference's keys
    opt = create_optimizer("adamw", 1e-6, 5e-4, net)
    stats = train_one_epoch(net, LabelSmoothingCrossEntropy(0.1), data, opt, DEV, 0, NativeScalerWithGradNormCount(), None, None,
                            None, start_steps=0, lr_schedule_values=[1e-6], wd_schedule_values=[5e-4],
                            num_training_steps_per_epoch=1, update_freq=1, use_amp=True, num_classes=C)
    assert abs(stats["loss"] - ref_loss) <= 5e-3 * abs(ref_loss)
    ref.eval()
    rev = E.evaluate_ref(data, ref, C)
    ev = evaluate(data, net, DEV, C)
    assert list(ev) == list(rev)
    assert all(v == v for v in ev.values())


def test_train_cli_seresnet50_synthetic_and_resume(tmp_path):
    work = tmp_path / "work"
    os.makedirs(work / "train_cls" / "output")
    base = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "seresnet50", "--input_size", "64", "--synthetic", "16",
            "--num_classes", "10", "--batch_size", "8", "--num_workers", "0", "--mixup", "0", "--warmup_epochs", "0", "--lr", "1e-4",
            "--use_amp", "true"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(base + ["--epochs", "1"], cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    from imageclassification_amd.checkpoint import DeferredModel
    ck = torch.load(work / "train_cls" / "output" / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    model = ck["model"]
    assert isinstance(model, DeferredModel) and model.arch == "seresnet50"
    assert tuple(model.state_dict()["layer2.0.se.fc1.weight"].shape) == (32, 512, 1, 1)
    # a second epoch resumes from checkpoint-0
    out2 = subprocess.run(base + ["--epochs", "2"], cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out2.returncode == 0, out2.stdout[-3000:] + out2.stderr[-3000:]
    assert os.path.exists(work / "train_cls" / "output" / "checkpoint-1.pth")
    assert "checkpoint-0" in out2.stdout + out2.stderr
    import json
    lines = [json.loads(l) for l in open(work / "train_cls" / "log.txt")]
    assert [l["epoch"] for l in lines] == [0, 1]
