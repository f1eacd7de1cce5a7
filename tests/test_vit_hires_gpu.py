"""ViT above 224^2 (T > 208 tokens: the tiled attention route of csrc/attention_long.hip) against the CPU oracle: whole-model
forward / backward parity, one engine step, and the command line with the `_384` model names.  Tolerances are those of
tests/test_vit_gpu.py (the oracle's own fp64-vs-fp32 re-association noise as the yardstick)."""
import os
import subprocess
import sys

import pytest
import torch

from _parity import ROOT, assert_within, step, vit_pair, worst
from oracle.vit_ref import ViTRef

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arch,img,B", [("vit_tiny_test", 256, 3),            # T = 257
                                        ("vit_tiny_test", 384, 2),            # T = 577
                                        ("vit_base_patch16_384", 384, 2)])    # ViT-B/16 at its true width and depth, T = 577
def test_vit_hires_forward_backward_matches_oracle(arch, img, B):
    C = 10
    ref, net = vit_pair(arch, C, img)
    assert net.T == (img // 16) ** 2 + 1 and net.T > 208
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    s = step(ref, net, x, y, C)
    w = worst(s.rows)
    print(f"{arch} img{img}: logits err {s.err:.2e} (self-noise {s.noise:.2e})")
    print(f"    worst grad err {w[1]:.2e} at {w[0]}")
    assert_within(s)


def test_vit_small_384_engine_step():
    """vit_small_patch16_384 through the engine for one training step and one evaluate batch (loss vs the fp32 oracle on the same
    weights)."""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    from imageclassification_amd.vit import VisionTransformer
    C, B = 1000, 4
    torch.manual_seed(0)
    ref = ViTRef("vit_small_patch16_384", C, img_size=384, bf16_points=True)
    net = VisionTransformer("vit_small_patch16_384", C)      # no img_size: the name carries it
    assert net.img_size == 384 and net.T == 577
    net.load_state_dict(ref.state_dict())
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 384, 384, generator=g)
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
    ev = evaluate([(x, y)], net, torch.device("cuda"), C)
    assert "acc1" in ev and ev["loss"] > 0


def test_create_model_with_a_384_name():
    sys.path.insert(0, ROOT)
    import train as T
    net = T.create_model("vit_base_patch16_384", 10)
    assert net.img_size == 384 and net.T == 577
    del net
    torch.cuda.empty_cache()
    assert T.create_model("vit_small_patch16_384", 10, input_size=384).T == 577
    with pytest.raises(ValueError, match="384"):
        T.create_model("vit_base_patch16_384", 10, input_size=224)
    # the _224 names keep taking any multiple of the patch size
    assert T.create_model("vit_small_patch16_224", 10, input_size=384).T == 577


def test_train_cli_vit_small_384_synthetic(tmp_path):
    """train.py --model vit_small_patch16_384 --input_size 384 on synthetic images: one short epoch in a child process, and the
    saved checkpoint's "model" reloads as the recipe of a 384^2 model."""
    work = tmp_path / "work"
    os.makedirs(work / "train_cls" / "output")
    argv = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "vit_small_patch16_384", "--input_size", "384",
            "--synthetic", "16", "--num_classes", "10", "--batch_size", "8", "--epochs", "1", "--num_workers", "0", "--mixup", "0",
            "--warmup_epochs", "0", "--lr", "1e-4", "--use_amp", "true"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(argv, cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    from imageclassification_amd.checkpoint import DeferredModel
    ck = torch.load(work / "train_cls" / "output" / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    model = ck["model"]
    assert isinstance(model, DeferredModel) and model.img_size == 384 and model.arch == "vit_small_patch16_384"
    assert tuple(model.state_dict()["pos_embed"].shape) == (1, 577, 384)
    assert ck["input_shape"] == [1, 3, 384, 384]
