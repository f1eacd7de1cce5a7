"""The ResNet family beyond ResNet-18/34/50 on the GPU: whole-network parity of resnext50_32x4d (grouped conv2 through
icamd_gconv3x3_*), wide_resnet50_2 and resnet101 against the oracle (oracle/resnet_ref.py) by the protocol of
tests/test_model_gpu.py::test_resnet50_whole_network_parity_well_conditioned (tests/_resnet_parity.py); the two largest members
take one finite step; eval, state_dict, engine, command line and reproducibility for resnext50_32x4d."""
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


# arch, gamma_last, yardstick caps (logits, gradient mean, gradient worst), tensors with a gradient (None: at least 40)
PARITY = [
    ("resnext50_32x4d", 0.0, (5e-3, 4.5e-2, 7e-2), None),
    ("resnext50_32x4d", 0.02, (8e-3, 0.13, 0.22), 161),
    ("wide_resnet50_2", 0.02, (8e-3, 0.13, 0.22), 161),
    ("resnet101", 0.02, (8e-3, 0.13, 0.22), 314),
]


@pytest.mark.parametrize("arch,gamma_last,caps,ntensors", PARITY)
def test_whole_network_parity_well_conditioned(arch, gamma_last, caps, ntensors):
    """Batch 32 at 128 x 128, 100 classes, label smoothing 0.1, timm-default init; the last BatchNorm weight of every block at 0
    (49 tensors compared, the zero-gamma branches exactly zero on both sides) or at 0.02 (every tensor compared).  The yardstick
    -- the reference against its own fp64 copy -- is asserted first under caps that are conditions (measured on a CPU for
    resnext50_32x4d: logits 2.5e-3 / mean 2.1e-2 / worst 3.0e-2 at gamma 0 and 3.9e-3 / 8.3e-2 / 0.140 at 0.02;
    wide_resnet50_2 4.3e-3 / 9.0e-2 / 0.150; resnet101 5.0e-3 / 0.107 / 0.156); an all-zero gradient scores 1.0.  Then the HIP
    path: logits <= 2 max(noise, 1e-3), loss to 1e-3, mean gradient error <= 2 max(mean noise, 1e-3), per tensor <= 3 max(its
    noise, 5e-3)."""
    C, B, HW = 100, 32, 128
    ref, net = timm_default_pair(arch, C, gamma_last=gamma_last)
    x, y = parity_batch(C, B, HW)
    yard = yardstick(ref, x, y, 0.1)
    got = hip_rows(net, x, y, C, 0.1, yard)
    rows, zero_branch, worst = got.rows, got.zero_branch, got.worst
    print(f"{arch} B={B} {HW}x{HW} gamma_last={gamma_last}: logits err {got.err_logits:.2e} (self-noise {yard.noise_logits:.2e}); "
          f"loss {got.loss:.6f} vs {yard.loss:.6f}; {len(rows)} gradient tensors: mean err {got.mean_err:.2e} (self-noise "
          f"{yard.mean_noise:.2e}), worst {worst[0]} {worst[1]:.2e} (its self-noise {worst[2]:.2e}), yardstick worst "
          f"{yard.worst_noise[1]:.2e}; {zero_branch} zero-gradient branch tensors exact")
    if gamma_last:
        for kind in ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn2.weight", "bn3.weight"):
            sel = [r for r in rows if r[0].endswith(kind)]
            print(f"  {kind:14s} {len(sel):3d} tensors: HIP mean {sum(r[1] for r in sel) / len(sel):.2e} worst "
                  f"{max(r[1] for r in sel):.2e} | yardstick mean {sum(r[2] for r in sel) / len(sel):.2e} worst "
                  f"{max(r[2] for r in sel):.2e}")
        if arch.startswith("resnext"):
            for name, e, n in rows:
                if name.endswith("conv2.weight"):
                    print(f"    {name:28s} HIP {e:.2e} yardstick {n:.2e}")
    # the yardstick itself
    cap_logits, cap_mean, cap_worst = caps
    assert yard.noise_logits <= cap_logits and yard.mean_noise <= cap_mean and yard.worst_noise[1] <= cap_worst, \
        (yard.noise_logits, yard.mean_noise)
    if gamma_last:
        assert zero_branch == 0 and len(rows) == ntensors            # every parameter tensor has a non-zero gradient
    else:
        assert zero_branch == 112 and len(rows) == 49
    # the HIP path against it
    assert_hip_within_yardstick(yard, got)


@pytest.mark.parametrize("arch", ["resnet152", "wide_resnet101_2"])
def test_largest_members_take_one_finite_step(arch):
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
    for name in ("conv1.weight", "layer3.20.conv2.weight", "layer4.2.conv3.weight", "fc.weight"):
        assert float(net.grad_of(name).abs().max()) > 0.0, name


def test_resnext50_eval_folded_and_state_dict_round_trip():
    from imageclassification_amd.nets import ResNet
    C = 10
    ref, net, sd = perturbed_bn_pair("resnext50_32x4d", C, seed=4)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(10))
    exact = ResNetRef("resnext50_32x4d", C, bf16_points=False, zero_init_last=False)   # the reference's fp32 arithmetic
    exact.load_state_dict(sd)
    exact.eval()
    net.eval()
    with torch.no_grad():
        want = exact(x)
    assert net.fold_eval
    folded = net(x.cuda()).float().cpu()
    net.fold_eval = False
    unfolded = net(x.cuda()).float().cpu()
    net.fold_eval = True
    e_fold, e_plain = R.rel_l2(folded, want), R.rel_l2(unfolded, want)
    print(f"resnext50_32x4d eval logits vs fp32 reference: folded {e_fold:.2e}, separate BatchNorm pass {e_plain:.2e}")
    assert e_fold <= 1e-2 and e_plain <= 1e-2
    # state_dict -> load_state_dict: bit-exact, the (C, Cg, 3, 3) tensors included
    out = net.state_dict()
    assert list(out) == list(sd)
    assert tuple(out["layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
    assert tuple(out["layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)
    for k in sd:
        assert torch.equal(out[k].float(), sd[k].float()), k
    net2 = ResNet("resnext50_32x4d", C, seed=99)
    net2.load_state_dict(out)
    assert torch.equal(net2.param_arena, net.param_arena) and torch.equal(net2.buffer_arena, net.buffer_arena)
    assert torch.equal(net2.shadow, net.shadow)
    # timm's init on a grouped filter: kaiming_normal_(mode="fan_out") takes fan_out = Cout * k * k from the weight's shape
    w = ResNet("resnext50_32x4d", C, seed=1).state_dict()["layer3.0.conv2.weight"]
    assert abs(float(w.std()) / (2.0 / (512 * 9)) ** 0.5 - 1.0) <= 0.05


def test_resnext50_engine_step_evaluate_and_bitwise_repeat():
    """The loss is compared with the reference at a WELL-CONDITIONED setting: every block's last BatchNorm weight at 0.02, as in the
    whole-network protocol.  With those weights at 1 this batch of 8 at 64 x 64 (layer4 normalises over 32 values) is chaotic for
    any two correct implementations: the reference against its own fp64 copy differs by 3.1e-2 in the loss and 0.19 in the logits
    (ResNet-50, same setting: 2.5e-3 / 0.17), a yardstick that can tell nothing.  At 0.02 it measures 1.4e-4 / 7.6e-3 on a CPU;
    it is asserted <= 1e-3 on the loss before the HIP path is held to the engine tests' 5e-3."""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.nets import ResNet
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    from oracle import engine_ref as E
    import copy
    C, B = 10, 8
    torch.manual_seed(0)
    ref = ResNetRef("resnext50_32x4d", C, bf16_points=True, zero_init_last=False)
    for n, m in ref.named_modules():
        if n.endswith("bn3"):
            m.weight.data.fill_(0.02)
    net = ResNet("resnext50_32x4d", C)
    net.load_state_dict(ref.state_dict())
    start = copy.deepcopy(ref.state_dict())
    g = torch.Generator().manual_seed(21)
    data = [(torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, C, (B,), generator=g))]
    # the step twice from the same state: loss and the whole gradient arena bit-identical
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
    print(f"resnext50_32x4d B={B} 64x64: loss HIP {runs[0][0]:.6f}, reference {ref_loss:.6f}, its fp64 copy {loss64:.6f}")
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


def test_train_cli_resnext50_synthetic_and_resume(tmp_path):
    work = tmp_path / "work"
    os.makedirs(work / "train_cls" / "output")
    base = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "resnext50_32x4d", "--input_size", "64", "--synthetic", "16",
            "--num_classes", "10", "--batch_size", "8", "--num_workers", "0", "--mixup", "0", "--warmup_epochs", "0", "--lr", "1e-4",
            "--use_amp", "true"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(base + ["--epochs", "1"], cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    from imageclassification_amd.checkpoint import DeferredModel
    ck = torch.load(work / "train_cls" / "output" / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    model = ck["model"]
    assert isinstance(model, DeferredModel) and model.arch == "resnext50_32x4d"
    assert tuple(model.state_dict()["layer2.0.conv2.weight"].shape) == (256, 8, 3, 3)
    # a second epoch resumes from checkpoint-0
    out2 = subprocess.run(base + ["--epochs", "2"], cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out2.returncode == 0, out2.stdout[-3000:] + out2.stderr[-3000:]
    assert os.path.exists(work / "train_cls" / "output" / "checkpoint-1.pth")
    assert "checkpoint-0" in out2.stdout + out2.stderr
    import json
    lines = [json.loads(l) for l in open(work / "train_cls" / "log.txt")]
    assert [l["epoch"] for l in lines] == [0, 1]
