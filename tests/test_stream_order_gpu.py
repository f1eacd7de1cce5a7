"""One stream against two, bit for bit, for the backward passes tests/test_resnet_routes_gpu.py does not cover: a ResNet with
squeeze-and-excitation, deep stem, average-pool shortcut and grouped convolutions; ConvNeXt V1 under stochastic depth with the layer
scale folded and unfolded; ConvNeXt V2 under stochastic depth; ViT with its opt-in lane.

On one saved forward state (batch 8 at the model's test input size) the gradient arena is taken after a backward into the zeroed
arena and again after an accumulating backward, with `wgrad_side_stream` True and False.  The kernels are deterministic and the
one-stream pass is the reference, so equality is exact and no tolerance is involved.  A difference is a cross-stream race that the
timing happened to expose: tests/test_stream_order_cpu.py finds the pair of launches from the call trace.
"""
import pytest
import torch

from _harness import free_after_each  # noqa: F401
from _parity import convnext_pair, hip_step, vit_pair
from _resnet_parity import perturbed_bn_pair

pytestmark = pytest.mark.gpu

C, B = 10, 8


def _masks(net):
    """Per block one [B] mask of {0, 1 / keep_prob} with two samples dropped, other samples from block to block; ones for the
    first block, whose rate is 0 (never read)."""
    out = []
    for k, blk in enumerate(net.blocks):
        m = torch.full((B,), 1.0 / (1.0 - blk["rate"]))
        m[k % B] = m[(k + 3) % B] = 0.0
        out.append(m if blk["rate"] > 0.0 else torch.ones(B))
    return out


def _seresnext(monkeypatch):
    _, net, _ = perturbed_bn_pair("seresnext26d_32x4d", C, seed=3)
    return net, 64


def _convnext(arch, fused_ls):
    def build(monkeypatch):
        from imageclassification_amd import convnext
        monkeypatch.setattr(convnext, "_FUSED_LS", fused_ls)          # read when the model is constructed
        _, net = convnext_pair(arch, C, drop_path=0.2)
        assert net.fused_ls == (fused_ls and not net.grn)
        net.injected_keep = _masks(net)
        assert sum(float(m.min()) == 0.0 for m in net.injected_keep) == len(net.blocks) - 1
        return net, 64
    return build


def _vit(monkeypatch):
    monkeypatch.setenv("ICAMD_WGRAD_STREAM_VIT", "1")                 # read when the first backward makes the lane
    _, net = vit_pair("vit_tiny_test", C, 224)
    return net, 224


MODELS = {
    "seresnext26d_32x4d": _seresnext,
    "convnext_test/folded": _convnext("convnext_test", True),
    "convnext_test/unfolded": _convnext("convnext_test", False),
    "convnextv2_test": _convnext("convnextv2_test", True),
    "vit_tiny_test/lane_on": _vit,
}


def _arenas(net, ws, side):
    """-> (the gradient arena after one backward into zeros, after an accumulating backward on top, did the pass use two streams)"""
    net.wgrad_side_stream = side
    net.grad_arena.zero_()
    net.backward_packed(ws)
    torch.cuda.synchronize()
    first = net.grad_arena.clone()
    two_streams = net._lane.enabled
    net.backward_packed(ws, accumulate=True)
    torch.cuda.synchronize()
    return first, net.grad_arena.clone(), two_streams and net._lane.enabled


@pytest.mark.parametrize("model", list(MODELS))
def test_one_stream_and_two_give_the_same_bits(monkeypatch, model):
    net, hw = MODELS[model](monkeypatch)
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(B, 3, hw, hw, generator=g), torch.randint(0, C, (B,), generator=g)
    ws, _, loss = hip_step(net, x, y, C)                              # train(), pack, forward, loss gradient (and one backward)
    assert loss == loss and net._lane.side is not None
    two, two_acc, used_two = _arenas(net, ws, True)
    one, one_acc, used_one = _arenas(net, ws, False)
    assert used_two and not used_one
    host, host_acc = one.cpu(), one_acc.cpu()
    assert bool(torch.isfinite(host).all()) and bool(torch.isfinite(host_acc).all())
    for name, p in net.params.items():
        assert float(host[p.offset:p.offset + p.numel].abs().max()) > 0.0, name
        assert not torch.equal(host_acc[p.offset:p.offset + p.numel], host[p.offset:p.offset + p.numel]), name
    differing = [n for n, p in net.params.items() if not torch.equal(two[p.offset:p.offset + p.numel], one[p.offset:p.offset + p.numel])]
    differing_acc = [n for n, p in net.params.items()
                     if not torch.equal(two_acc[p.offset:p.offset + p.numel], one_acc[p.offset:p.offset + p.numel])]
    print(f"{model}: {len(net.params)} parameters, loss {loss:.4f}; differing after one backward {differing}, after two {differing_acc}")
    assert differing == [] and differing_acc == []
    assert torch.equal(two, one) and torch.equal(two_acc, one_acc)    # the padding between the parameters as well
