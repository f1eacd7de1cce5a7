"""The window-12 Swin models on the HIP kernels vs the CPU oracle (oracle/swin_ref.py, same bf16 rounding points), with the
construction and the bounds of tests/test_swin_gpu.py (tests/_parity.py): logits <= 2 max(fp64 self-noise, 2e-3), loss within 5e-3
relative, every parameter gradient <= 3 max(yardstick, 1e-2).

swin_test_w12 at 96^2 has a shifted window-12 stage (24^2 tokens) and a one-window stage (12^2); at 192^2 both stages are shifted
window-12 stages (48^2, 24^2).  swin_base_patch4_window12_384 itself, at batch 1: its parameters (loaded from the reference's
state_dict, bit for bit), its logits and loss against the reference's forward under the bounds above (fp32 and fp64 forward: about a
second on the host), and finite, non-zero gradients -- the reference's two backward passes at 384^2 would take the test past the
few seconds it may use, and the gradient paths are the ones the swin_test_w12 cases compare."""
import os
import pickle
import subprocess
import sys

import pytest
import torch

from _parity import ROOT, check, swin_pair, swin_ref, xent_backward

pytestmark = pytest.mark.gpu
ARCH = "swin_test_w12"


@pytest.mark.parametrize("img,B", [(96, 4), (192, 2)])
def test_swin_w12_forward_backward_matches_oracle(img, B):
    C = 10
    ref, net = swin_pair(ARCH, C, img)
    assert [(st["res"], st["ws"]) for st in net.stages] == ([(24, 12), (12, 12)] if img == 96 else [(48, 12), (24, 12)])
    assert [blk["shift"] for st in net.stages for blk in st["blocks"]] == ([0, 6, 0, 0] if img == 96 else [0, 6, 0, 6])
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    check(f"{ARCH} img{img}", ref, net, x, y, C)


def test_swin_w12_stochastic_depth_with_injected_masks():
    """drop_path_rate 0.5 with the same per-sample masks on both sides, as tests/test_swin_gpu.py does for swin_test"""
    C, B, img = 10, 4, 96
    ref, net = swin_pair(ARCH, C, img, drop_path_rate=0.5)
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
    check(f"{ARCH} drop_path 0.5", ref, net, x, y, C)


def test_swin_w12_engine_step_and_evaluate():
    """one optimizer step through the engine (loss vs the oracle on the same weights, no stochastic depth in either); the gathered
    bias the kernels read follows the updated [529][heads] tables bit for bit; evaluate returns acc1"""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.swin import relative_position_index
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    C, B, img = 10, 4, 96
    ref, net = swin_pair(ARCH, C, img)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    with torch.no_grad():
        rl = float(torch.nn.functional.cross_entropy(ref(x), y, label_smoothing=0.1))
    opt = create_optimizer("adamw", 1e-3, 5e-2, net)
    stats = train_one_epoch(net, LabelSmoothingCrossEntropy(0.1), [(x, y)], opt, torch.device("cuda"), 0,
                            NativeScalerWithGradNormCount(), None, None, None, start_steps=0, lr_schedule_values=[1e-4],
                            wd_schedule_values=[5e-2], num_training_steps_per_epoch=1, update_freq=1, use_amp=True,
                            num_classes=C)
    assert abs(stats["loss"] - rl) <= 5e-3 * rl, (stats, rl)
    assert opt.step_count == 1
    torch.cuda.synchronize()
    after, before = net.state_dict(), ref.state_dict()
    idx = relative_position_index(12).view(-1)
    bias_host = net.bias_arena.cpu()
    moved = 0
    for st in net.stages:
        for blk in st["blocks"]:
            name, H = blk["table"].name, st["heads"]
            assert after[name].shape == (529, H)
            moved += int(not torch.equal(after[name], before[name]))
            want = after[name][idx].view(144, 144, H).permute(2, 0, 1).contiguous()
            got = bias_host[blk["bias_off"]:blk["bias_off"] + H * 144 * 144].view(H, 144, 144)
            assert torch.equal(got, want), name
    assert moved == sum(net.depths)
    ev = evaluate([(x, y)], net, torch.device("cuda"), C)
    assert "acc1" in ev and ev["loss"] > 0


def test_swin_w12_state_and_pickling(tmp_path):
    from imageclassification_amd.checkpoint import DeferredModel
    C, img = 10, 96
    ref, net = swin_pair(ARCH, C, img)
    sd = net.state_dict()
    assert list(sd) == [n for n, _ in ref.named_parameters()]                      # parameters only, timm's names and order
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    path = tmp_path / "swin_w12.pth"
    torch.save({"model": net}, path)
    back = torch.load(path, map_location="cpu", weights_only=False)["model"]
    assert isinstance(back, DeferredModel)
    assert all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())
    live = pickle.loads(pickle.dumps(back)).materialise()
    assert live.arch == ARCH and live.img_size == img and live.drop_path_rate == 0.0
    assert all(torch.equal(live.state_dict()[k], v) for k, v in sd.items())
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(3))
    live.eval()
    net.eval()
    with torch.no_grad():
        assert torch.equal(live(x), net(x))


def test_swin_base_window12_384_loads_and_steps():
    """the model the family was added for, at its own size: parameters from the reference's state_dict bit for bit (timm's names,
    [529][heads] tables), then one training step at batch 1: logits <= 2 max(fp64 self-noise, 2e-3) and loss within 5e-3 relative of
    the reference's forward (the bounds of the parity cases), finite and non-zero gradients"""
    import copy
    from oracle import ops_ref as R
    from imageclassification_amd.swin import SwinTransformer
    arch, C = "swin_base_patch4_window12_384", 1000
    ref = swin_ref(arch, C, 384)
    net = SwinTransformer(arch, C, drop_path_rate=0.0)                             # no size given: the name's own
    assert net.img_size == 384 and net.plan == [(96, 12, 6), (48, 12, 6), (24, 12, 6), (12, 12, 0)]
    want = ref.state_dict()
    net.load_state_dict(want)
    sd = net.state_dict()
    assert sum(v.numel() for v in sd.values()) == 87903584
    assert list(sd) == list(want) and all(torch.equal(sd[k], v) for k, v in want.items())
    assert sd["layers.2.blocks.17.attn.relative_position_bias_table"].shape == (529, 16)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 3, 384, 384, generator=g)
    y = torch.randint(0, C, (1,), generator=g)
    with torch.no_grad():
        out = ref(x)
        out64 = copy.deepcopy(ref).double()(x.double()).float()
        rl = float(torch.nn.functional.cross_entropy(out, y, label_smoothing=0.1))
    y = y.cuda()
    net.train()
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    xent_backward(net, ws, y, C, smoothing=0.1)
    got = logits[:, :C].float().cpu()
    assert bool(torch.isfinite(got).all())
    noise, err, loss = R.rel_l2(out64, out), R.rel_l2(got, out), float(ws["loss_rows"].mean())
    print(f"{arch}: logits err {err:.2e} (self-noise {noise:.2e}); loss {loss:.5f} vs {rl:.5f}")
    assert err <= 2.0 * max(noise, 2e-3), (err, noise)
    assert abs(loss - rl) <= 5e-3 * rl, (loss, rl)
    assert bool(torch.isfinite(net.grad_arena).all()) and float(net.grad_arena.abs().max()) > 0
    for name in ("layers.0.blocks.1.attn.relative_position_bias_table", "layers.3.blocks.1.attn.relative_position_bias_table",
                 "patch_embed.proj.weight"):
        assert float(net.grad_of(name).abs().max()) > 0, name


def test_train_cli_swin_test_w12_synthetic(tmp_path):
    """the command line in a fresh child process: one epoch of swin_test_w12 at 96 x 96 on synthetic data, a checkpoint at the end"""
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--model", ARCH, "--input_size", "96", "--synthetic", "32",
           "--num_classes", "10", "--epochs", "1", "--batch_size", "8", "--warmup_epochs", "0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ck = tmp_path / "train_cls" / "output" / "checkpoint-0.pth"
    assert ck.exists(), out.stdout[-2000:]
    c = torch.load(ck, map_location="cpu", weights_only=False)
    sd = c["model"].state_dict()
    assert sd["layers.0.blocks.1.attn.relative_position_bias_table"].shape == (529, 1)
    assert sd["head.fc.weight"].shape == (10, 64)
