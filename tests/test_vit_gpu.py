"""ViT on the HIP kernels vs the CPU oracle (oracle/vit_ref.py, same bf16 rounding points; the step: tests/_parity.py).
Whole-network tolerances use the oracle's own re-association noise (fp64 vs fp32 accumulation) as the yardstick, as in
tests/test_model_gpu.py; transformers have no ReLU masks, so the noise is an order of magnitude smaller than for ResNets."""
import pytest
import torch

from _parity import assert_within, step, vit_pair, worst
from oracle import ops_ref as R
from oracle.vit_ref import ViTRef

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_token_plumbing_kernels():
    from imageclassification_amd import hip
    lib = hip.load()
    B, T, C = 3, 5, 16
    g = torch.Generator().manual_seed(3)
    patches = R.bf16_round(torch.randn(B, T - 1, C, generator=g))
    cls, pos = torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    pd, cd, posd = patches.to(torch.bfloat16).to(DEV), cls.to(DEV), pos.to(DEV)
    tok = torch.empty(B, T, C, dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_vit_tokens_fwd(hip.ptr(pd), hip.ptr(cd), hip.ptr(posd), hip.ptr(tok), B, T, C, hip.stream_ptr()) == 0
    ref = torch.cat([cls.expand(B, 1, C), patches], 1) + pos
    torch.cuda.synchronize()
    assert R.max_bf16_ulp(tok.float().cpu(), R.bf16_round(ref)) <= 1.0
    out = torch.ones(T * C, device=DEV)
    assert lib.icamd_batch_sum(hip.ptr(tok), T * C, B, T * C, hip.ptr(out), 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.allclose(out.cpu(), 1 + tok.float().cpu().sum(0).flatten(), rtol=1e-5, atol=1e-5)
    dst = torch.zeros(B, C, dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_strided_rows_copy(hip.ptr(tok), T * C, hip.ptr(dst), C, B, C, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), tok[:, 0].cpu())


@pytest.mark.parametrize("arch,img,B", [("vit_tiny_test", 64, 6), ("vit_tiny_test", 224, 2),
                                        # ViT-B/16 at its true width and depth (D 768, 12 heads, MLP 3072, 12 blocks, T 197):
                                        # every gradient tensor against the oracle's, not only the loss
                                        ("vit_base_patch16_224", 224, 2)])
def test_vit_forward_backward_matches_oracle(arch, img, B):
    C = 10
    ref, net = vit_pair(arch, C, img)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, img, img, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    s = step(ref, net, x, y, C)
    w = worst(s.rows)
    print(f"{arch} img{img}: logits err {s.err:.2e} (self-noise {s.noise:.2e}); worst grad err {w[1]:.2e} at {w[0]}")
    assert_within(s)


def test_vit_base_parameter_layout_and_engine_step():
    """Full ViT-B/16 shapes through the engine for one step (loss vs the fp32 oracle on the same weights)."""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    from imageclassification_amd.vit import VisionTransformer
    C, B = 1000, 4
    torch.manual_seed(0)
    ref = ViTRef("vit_base_patch16_224", C, bf16_points=True)
    assert sum(p.numel() for p in ref.parameters()) == 86567656
    net = VisionTransformer("vit_base_patch16_224", C)
    net.load_state_dict(ref.state_dict())
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
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
    ev = evaluate([(x, y)], net, torch.device("cuda"), C)
    assert "acc1" in ev and ev["loss"] > 0
