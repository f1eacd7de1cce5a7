"""The ResNet family beyond ResNet-18/34/50 (resnet101/152, wide_resnet50_2/101_2, resnext50/101_32x4d), the parts that need no GPU:
the oracle has the published parameter counts and torchvision / timm names, the product's ARCHS rows describe
the same graph, the three existing names are unchanged, and the host-only entries of the grouped-convolution ABI answer."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _resnet_parity import named_shapes  # noqa: E402
from oracle.resnet_ref import ARCHS, ResNetRef  # noqa: E402

PUBLISHED = {
    "resnet101": 44549160,
    "resnet152": 60192808,
    "wide_resnet50_2": 68883240,
    "wide_resnet101_2": 126886696,
    "resnext50_32x4d": 25028904,
    "resnext101_32x4d": 44177704,
}
# ResNeXt-50 conv2 at batch 256, 224 x 224 input: (C, input grid, stride)
RESNEXT50_CONV2 = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


@pytest.mark.parametrize("arch", sorted(PUBLISHED))
def test_reference_parameter_counts_and_names(arch):
    ref = ResNetRef(arch, 1000)
    assert sum(p.numel() for p in ref.parameters()) == PUBLISHED[arch]
    sd = ref.state_dict()
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7)
    assert "layer1.0.downsample.0.weight" in sd and "layer1.0.downsample.1.running_var" in sd
    assert "layer4.2.bn3.num_batches_tracked" in sd and tuple(sd["fc.weight"].shape) == (1000, 2048)
    if arch == "resnext50_32x4d":
        assert tuple(sd["layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
        assert tuple(sd["layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)
        assert tuple(sd["layer1.0.conv1.weight"].shape) == (128, 64, 1, 1)
        assert tuple(sd["layer1.0.conv3.weight"].shape) == (256, 128, 1, 1)
    if arch == "wide_resnet50_2":
        assert tuple(sd["layer1.0.conv2.weight"].shape) == (128, 128, 3, 3)
        assert tuple(sd["layer4.0.conv3.weight"].shape) == (2048, 1024, 1, 1)


@pytest.mark.parametrize("arch", sorted(PUBLISHED))
def test_product_archs_describe_the_same_graph(arch):
    from imageclassification_amd import nets
    assert arch in nets.ARCHS
    assert nets.param_shapes(arch, 1000) == named_shapes(ResNetRef(arch, 1000))
    assert nets.param_shapes(arch, 10)[-2:] == [("fc.weight", (10, 2048)), ("fc.bias", (10,))]
    groups = {c[0]: c[6] for blk in nets.block_specs(arch) for c in blk["convs"]}
    want = ARCHS[arch][2]
    assert all(g == (want if n.endswith(".conv2") else 1) for n, g in groups.items())


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnet50"])
def test_existing_names_unchanged(arch):
    from imageclassification_amd import nets
    ref = ResNetRef(arch, 1000)
    assert nets.param_shapes(arch, 1000) == named_shapes(ref)
    assert tuple(nets.ARCHS[arch][:4]) == tuple(ARCHS[arch][:4])
    assert all(c[6] == 1 for blk in nets.block_specs(arch) for c in blk["convs"])


def test_train_cli_lists_the_new_names():
    import train
    with pytest.raises(ValueError) as e:
        train.create_model("resnext9000", 10)
    for arch in PUBLISHED:
        assert arch in str(e.value)


def test_grouped_abi_host_side():
    from imageclassification_amd import hip
    lib = hip.load()
    for name in ("icamd_gconv3x3_supported", "icamd_gconv3x3_fwd", "icamd_gconv3x3_fwd_act", "icamd_gconv3x3_dgrad",
                 "icamd_gconv3x3_wgrad_workspace_bytes", "icamd_gconv3x3_wgrad"):
        assert name in hip.EXPORTED_SYMBOLS
    assert lib.icamd_abi_version() == 6
    sizes = []
    for C, hw, st in RESNEXT50_CONV2:
        d = hip.conv_desc(256, hw, hw, C, C, 3, 3, st, 1)
        assert lib.icamd_gconv3x3_supported(ctypes.byref(d), 32) == 1, (C, hw, st)
        nbytes = lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), 32)
        assert nbytes > 0 and nbytes % (C * 9 * (C // 32) * 4) == 0       # whole fp32 slabs [C][3][3][Cg]
        sizes.append((C, nbytes))
    by_c = {}
    for C, nbytes in sizes:
        by_c[C] = max(by_c.get(C, 0), nbytes)
    assert by_c[128] < by_c[256] < by_c[512] < by_c[1024]
    # all four group widths, odd sizes
    for C, groups in ((64, 16), (128, 16), (128, 8), (128, 4), (96, 3)):
        d = hip.conv_desc(3, 9, 7, C, C, 3, 3, 1, 1)
        assert lib.icamd_gconv3x3_supported(ctypes.byref(d), groups) == 1
    refused = [
        (hip.conv_desc(2, 8, 8, 256, 256, 3, 3, 1, 1), 4),      # Cg = 64
        (hip.conv_desc(2, 8, 8, 128, 128, 1, 1, 1, 0), 32),     # 1x1
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 1, 0), 32),     # pad 0
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 3, 1), 32),     # stride 3
        (hip.conv_desc(2, 8, 8, 128, 256, 3, 3, 1, 1), 32),     # Cin != Cout
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 1, 1), 24),     # groups does not divide C
        (hip.conv_desc(2, 8, 8, 128, 128, 3, 3, 1, 1), 0),
    ]
    for d, groups in refused:
        assert lib.icamd_gconv3x3_supported(ctypes.byref(d), groups) == 0
        assert lib.icamd_gconv3x3_wgrad_workspace_bytes(ctypes.byref(d), groups) == 0
    assert lib.icamd_gconv3x3_supported(None, 32) == 0
