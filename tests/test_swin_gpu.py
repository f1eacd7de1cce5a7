"""Swin Transformer on the HIP kernels vs the CPU oracle (oracle/swin_ref.py, same bf16 rounding points), on the pattern of
tests/test_vit_gpu.py and with its bounds (tests/_parity.py): whole-network tolerances use the oracle's own re-association noise
(fp64 vs fp32 accumulation) as the yardstick."""
import os
import pickle
import subprocess
import sys

import pytest
import torch

from _parity import ROOT, check, swin_pair, xent_backward
from oracle.swin_ref import SwinRef

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("arch,img,B", [("swin_test", 56, 6), ("swin_test", 112, 2), ("swin_tiny_patch4_window7_224", 224, 2)])
def test_swin_forward_backward_matches_oracle(arch, img, B):
    C = 10
    ref, net = swin_pair(arch, C, img)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    check(f"{arch} img{img}", ref, net, x, y, C)


def test_swin_stochastic_depth_with_injected_masks():
    """drop_path_rate 0.5: the same per-sample masks on both sides (a seam on each: `injected_keep` / `_Block.keep`), at least one
    dropped and one kept sample in every branch that has a rate"""
    C, B, img = 10, 6, 56
    ref, net = swin_pair("swin_test", C, img, drop_path_rate=0.5)
    rates = [blk["rate"] for st in net.stages for blk in st["blocks"]]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.5) < 1e-6 and all(a < b for a, b in zip(rates, rates[1:]))
    g = torch.Generator().manual_seed(11)
    keeps = []
    for bi, (rate, blk) in enumerate(zip(rates, ref.blocks())):
        pair = []
        for branch in (0, 1):
            m = (torch.rand(B, generator=g) < 1.0 - rate).float()
            if rate > 0.0:
                m[(2 * bi + branch) % B] = 0.0            # one dropped,
                m[(2 * bi + branch + 1) % B] = 1.0        # one kept
            pair.append(m / (1.0 - rate))
        keeps += pair
        blk.keep = (pair[0], pair[1]) if rate > 0.0 else (None, None)
    net.injected_keep = keeps
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    check("swin_test drop_path 0.5", ref, net, x, y, C)


def test_swin_accumulation_state_and_pickling(tmp_path):
    from imageclassification_amd.checkpoint import DeferredModel
    C, B, img = 10, 4, 56
    ref, net = swin_pair("swin_test", C, img)
    # state_dict round trip, bit for bit; parameters only
    sd = net.state_dict()
    assert list(sd) == [n for n, _ in ref.named_parameters()]
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g).cuda()
    net.train()
    ws = net.pack(x.cuda())
    net.forward_packed(ws)
    xent_backward(net, ws, y, C, smoothing=0.1)
    once = net.grad_arena.clone()
    net.backward_packed(ws, accumulate=True)
    torch.cuda.synchronize()
    twice = net.grad_arena
    assert float(once.abs().max()) > 0
    assert torch.allclose(twice, 2 * once, rtol=1e-5, atol=1e-6 * float(once.abs().max()))
    # a pickled model reloads through checkpoint.py
    path = tmp_path / "swin.pth"
    torch.save({"model": net}, path)
    back = torch.load(path, map_location="cpu", weights_only=False)["model"]
    assert isinstance(back, DeferredModel)
    assert all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())
    back2 = pickle.loads(pickle.dumps(back))
    live = back2.materialise()
    assert live.arch == "swin_test" and live.img_size == img and live.drop_path_rate == 0.0
    live.eval()
    net.eval()
    with torch.no_grad():
        assert torch.equal(live(x), net(x))


def test_swin_tiny_engine_step_and_evaluate():
    """Swin-T at 1000 classes through the engine for one step (loss vs the oracle on the same weights, no stochastic depth in
    either); evaluate returns acc1."""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.swin import SwinTransformer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    C, B = 1000, 4
    torch.manual_seed(0)
    ref = SwinRef("swin_tiny_patch4_window7_224", C, bf16_points=True)
    assert sum(p.numel() for p in ref.parameters()) == 28288354
    net = SwinTransformer("swin_tiny_patch4_window7_224", C, drop_path_rate=0.0)
    net.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 224, 224, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    with torch.no_grad():
        rl = float(torch.nn.functional.cross_entropy(ref(x), y, label_smoothing=0.1))
    opt = create_optimizer("adamw", 1e-3, 5e-2, net)
    stats = train_one_epoch(net, LabelSmoothingCrossEntropy(0.1), [(x, y)], opt, torch.device("cuda"), 0,
                            NativeScalerWithGradNormCount(), None, None, None, start_steps=0, lr_schedule_values=[1e-4],
                            wd_schedule_values=[5e-2], num_training_steps_per_epoch=1, update_freq=1, use_amp=True,
                            num_classes=C)
    assert abs(stats["loss"] - rl) <= 5e-3 * rl, (stats, rl)
    assert opt.step_count == 1 and float(opt.norm_clip[0]) > 0
    # the optimizer step moved the bias tables, and the gathered bias the kernels read was refreshed behind it: bias = table[index]
    # of the UPDATED tables, bit for bit, for every block
    from imageclassification_amd.swin import relative_position_index
    torch.cuda.synchronize()
    after, before = net.state_dict(), ref.state_dict()
    idx = relative_position_index(7).view(-1)
    bias_host = net.bias_arena.cpu()
    moved = 0
    for st in net.stages:
        for blk in st["blocks"]:
            name, H = blk["table"].name, st["heads"]
            moved += int(not torch.equal(after[name], before[name]))
            want = after[name][idx].view(49, 49, H).permute(2, 0, 1).contiguous()
            got = bias_host[blk["bias_off"]:blk["bias_off"] + H * 49 * 49].view(H, 49, 49)
            assert torch.equal(got, want), name
    assert moved == sum(net.depths)
    ev = evaluate([(x, y)], net, torch.device("cuda"), C)
    assert "acc1" in ev and ev["loss"] > 0


def test_swin_default_drop_path_draws_masks_and_stays_finite():
    """the constructor default (0.1): masks are drawn on the host, a training step runs and every gradient is finite"""
    from imageclassification_amd.swin import SwinTransformer
    C, B = 10, 8
    torch.manual_seed(2)
    net = SwinTransformer("swin_test", C, img_size=56)
    assert net.drop_path_rate == 0.1
    x = torch.randn(B, 3, 56, 56)
    y = torch.randint(0, C, (B,)).cuda()
    net.train()
    ws = net.pack(x.cuda())
    net.forward_packed(ws)
    xent_backward(net, ws, y, C, smoothing=0.1)
    assert ws["keep_dev"].shape == (8, B)
    assert bool(torch.isfinite(net.grad_arena).all()) and float(net.grad_arena.abs().max()) > 0


def test_train_cli_swin_tiny_synthetic(tmp_path):
    """the command line in a fresh child process: one epoch of Swin-T on synthetic data, a checkpoint at the end.
    --warmup_epochs 0: the default (5 epochs) is longer than the one epoch asked for, which the learning-rate schedule refuses for
    every model (utils.cosine_scheduler's length assertion, as in the reference's utils.py)."""
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "swin_tiny_patch4_window7_224", "--synthetic", "64",
           "--num_classes", "10", "--epochs", "1", "--batch_size", "8", "--warmup_epochs", "0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ck = tmp_path / "train_cls" / "output" / "checkpoint-0.pth"
    assert ck.exists(), out.stdout[-2000:]
    c = torch.load(ck, map_location="cpu", weights_only=False)
    sd = c["model"].state_dict()
    assert sd["layers.0.blocks.1.attn.relative_position_bias_table"].shape == (169, 3)
    assert sd["head.fc.weight"].shape == (10, 768)
