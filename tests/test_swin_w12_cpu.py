"""The window-12 Swin models (swin_base_patch4_window12_384 and swin_test_w12), the parts that need no GPU: parameter counts, the
product's shape listing against the oracle (oracle/swin_ref.py), the stage plans, the host-side window geometry and relative-position
index at 12 x 12 against the way timm builds them, the kernels' host-side queries for ws = 12 and their neighbours, and the
command-line surface.  Patterned on tests/test_swin_cpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _swin_w12 as W12  # noqa: E402
from oracle.swin_ref import CONFIGS as ORACLE_CONFIGS, SwinRef, relative_position_index as ref_index  # noqa: E402
from oracle.swin_ref import shifted_window_mask, window_partition  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (classes, input size, parameters): counted from SwinRef (oracle/swin_ref.py); timm lists 87.90 M
COUNTS = {
    "swin_base_patch4_window12_384": (1000, 384, 87903584),
    "swin_test_w12": (10, 96, 139408),
}
WINDOW7 = {"swin_tiny_patch4_window7_224", "swin_small_patch4_window7_224", "swin_base_patch4_window7_224", "swin_test"}
GEOMETRIES = [(24, 24, 12, 6), (24, 36, 12, 6), (12, 12, 12, 0)]


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@pytest.mark.parametrize("arch", sorted(COUNTS))
def test_parameter_counts_and_shapes_equal_the_reference(arch):
    from imageclassification_amd import swin
    C, img, count = COUNTS[arch]
    shapes = swin.param_shapes(arch, C, img)
    assert sum(_numel(s) for s in shapes.values()) == count
    ref = SwinRef(arch, C, img_size=img)
    assert sum(p.numel() for p in ref.parameters()) == count
    assert list(shapes.items()) == [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    assert list(ref.state_dict()) == list(shapes)                      # parameters only: no index, no mask
    assert shapes["layers.0.blocks.1.attn.relative_position_bias_table"] == (529, swin.config(arch)[2][0])


def test_the_tables_stay_apart():
    from imageclassification_amd import swin
    assert set(swin.CONFIGS) == WINDOW7
    assert set(swin.CONFIGS_W12) == set(COUNTS)
    assert swin.CONFIGS_W12["swin_base_patch4_window12_384"] == (128, (2, 2, 18, 2), (4, 8, 16, 32), 12)
    assert swin.CONFIGS_W12["swin_test_w12"] == (32, (2, 2), (1, 2), 12)
    for arch, cfg in swin.CONFIGS_W12.items():
        assert ORACLE_CONFIGS[arch] == cfg


def test_stage_plans():
    from imageclassification_amd import swin
    base = [(96, 12, 6), (48, 12, 6), (24, 12, 6), (12, 12, 0)]
    assert swin.stage_plan("swin_base_patch4_window12_384", 384) == base
    assert swin.stage_plan("swin_base_patch4_window12_384") == base             # the name's own size
    assert swin.param_shapes("swin_base_patch4_window12_384") == swin.param_shapes("swin_base_patch4_window12_384", 1000, 384)
    assert swin.stage_plan("swin_test_w12", 96) == [(24, 12, 6), (12, 12, 0)]
    assert swin.stage_plan("swin_test_w12", 192) == [(48, 12, 6), (24, 12, 6)]
    with pytest.raises(ValueError, match="multiple of the window, or <= the window"):
        swin.stage_plan("swin_test_w12", 224)
    with pytest.raises(ValueError, match="multiple of the window, or <= the window"):
        swin.SwinTransformer("swin_base_patch4_window12_384", 10, img_size=224)   # raised before the GPU is asked for
    # the window-7 names keep their plan, their default size and their message
    assert swin.stage_plan("swin_tiny_patch4_window7_224") == [(56, 7, 3), (28, 7, 3), (14, 7, 3), (7, 7, 0)]
    with pytest.raises(ValueError, match=r"the window is 7 \(224 and 448 work, 384 does not\)"):
        swin.stage_plan("swin_tiny_patch4_window7_224", 384)


@pytest.mark.parametrize("Hs,Ws,ws,shift", GEOMETRIES)
def test_window_geometry_matches_roll_and_partition(Hs, Ws, ws, shift):
    from imageclassification_amd import swin
    win, slot, region = swin.window_geometry(Hs, Ws, ws, shift)
    g = torch.Generator().manual_seed(Hs * 100 + Ws)
    B, C = 2, 5
    x = torch.randn(B, Hs, Ws, C, generator=g)
    sh = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift else x
    want = window_partition(sh, ws).view(B, -1, ws * ws, C)                      # [B, nW, T, C]
    nW = (Hs // ws) * (Ws // ws)
    got = torch.zeros(B, nW, ws * ws, C)
    got[:, win, slot] = x.view(B, Hs * Ws, C)
    assert torch.equal(got, want)
    assert sorted((win * ws * ws + slot).tolist()) == list(range(Hs * Ws))
    mask = shifted_window_mask(Hs, Ws, ws, shift)                                # region ids against timm's mask
    rw = torch.zeros(nW, ws * ws, dtype=torch.int64)
    rw[win, slot] = region
    differ = rw.unsqueeze(1) != rw.unsqueeze(2)
    if mask is None:
        assert not bool(differ.any())
    else:
        assert torch.equal(differ, mask != 0)
        assert torch.equal(mask[differ], torch.full_like(mask[differ], -100.0))


def test_relative_position_index_12():
    from imageclassification_amd import swin
    idx = swin.relative_position_index(12)
    assert idx.shape == (144, 144) and idx.dtype == torch.int64 and torch.equal(idx, ref_index(12))
    assert int(idx.min()) == 0 and int(idx.max()) == 528


def test_supported_and_workspace_queries_host_side():
    from imageclassification_amd import hip
    lib = hip.load()
    assert lib.icamd_window_attention_supported(24, 24, 12, 32) == 1
    assert lib.icamd_window_attention_supported(12, 36, 12, 32) == 1
    for ws in (9, 10, 11, 13, 16):
        assert lib.icamd_window_attention_supported(2 * ws, 2 * ws, ws, 32) == 0
        assert lib.icamd_window_attention_bwd_workspace_bytes(1, 2 * ws, 2 * ws, 2, ws) == 0
    assert lib.icamd_window_attention_supported(30, 24, 12, 32) == 0
    assert lib.icamd_window_attention_supported(24, 30, 12, 32) == 0
    assert lib.icamd_window_attention_supported(24, 24, 12, 64) == 0
    # one fp32 [heads][144][144] partial per workgroup: the planner mirror of tests/_swin_w12.py, rounded up to 256 bytes
    for B, Hs, Ws, H, chunks in ((2, 24, 24, 2, 8), (3, 12, 12, 2, 3), (1, 24, 36, 3, 6), (17, 24, 24, 32, 16), (64, 96, 96, 4, 128),
                                 (64, 48, 48, 8, 64), (64, 24, 24, 16, 32), (64, 12, 12, 32, 16), (1, 12, 12, 1024, 1)):
        nwin = B * (Hs // 12) * (Ws // 12)
        assert W12.bwd_grid(nwin, H) == chunks
        got = lib.icamd_window_attention_bwd_workspace_bytes(B, Hs, Ws, H, 12)
        assert got > 0 and got == W12.bwd_workspace_bytes(B, Hs, Ws, H) == (chunks * H * 144 * 144 * 4 + 255) // 256 * 256
    # Swin-B at 384 x 384, batch 64: 512 workgroups at every stage, 40.5 MiB
    assert lib.icamd_window_attention_bwd_workspace_bytes(64, 96, 96, 4, 12) == 512 * 144 * 144 * 4
    assert lib.icamd_window_attention_bwd_workspace_bytes(2, 30, 24, 2, 12) == 0
    # the window-7 planner is untouched
    assert 341 * 3 * 2401 * 4 <= lib.icamd_window_attention_bwd_workspace_bytes(256, 56, 56, 3, 7) < 341 * 3 * 2401 * 4 + 256


def test_unit_is_built_linted_and_free_of_atomics():
    from imageclassification_amd import hip
    assert hip.ABI_VERSION == 6
    unit = open(os.path.join(ROOT, "imageclassification_amd", "csrc", "window_attention_w12.hip")).read()
    assert "atomicAdd" not in unit and "atomic_" not in unit
    build = open(os.path.join(ROOT, "imageclassification_amd", "csrc", "build.sh")).read()
    units = build.split('UNITS="')[1].split('"')[0].split()
    assert "window_attention_w12" in units and "window_attention" in units


def test_create_model_surface(monkeypatch):
    sys.path.insert(0, ROOT)
    import train as T
    from imageclassification_amd import swin
    built = []

    class Recorder:
        def __init__(self, name, num_classes, **kw):
            built.append((name, num_classes, kw))

    monkeypatch.setattr(T, "SwinTransformer", Recorder)            # no model is constructed on a GPU-less host
    assert isinstance(T.create_model("swin_base_patch4_window12_384", 1000, 384, 0.05), Recorder)
    assert isinstance(T.create_model("swin_base_patch4_window12_384", 1000, None, 0.05), Recorder)
    assert isinstance(T.create_model("swin_test_w12", 10, 96, 0.05), Recorder)
    assert isinstance(T.create_model("swin_test_w12", 10, 192, 0.05), Recorder)
    assert built == [("swin_base_patch4_window12_384", 1000, {"img_size": 384}), ("swin_base_patch4_window12_384", 1000, {"img_size": None}),
                     ("swin_test_w12", 10, {"img_size": 96}), ("swin_test_w12", 10, {"img_size": 192})]
    # the name carries its size, as vit_*_384 does: another one is refused before anything is built
    for size in (224, 192, 448):
        with pytest.raises(ValueError, match="built for 384x384 inputs"):
            T.create_model("swin_base_patch4_window12_384", 1000, size, 0.05)
    assert len(built) == 4
    monkeypatch.undo()                                             # the real class: its size check comes before any GPU use
    with pytest.raises(ValueError, match="multiple of the window, or <= the window"):
        T.create_model("swin_test_w12", 10, 224, 0.05)
    with pytest.raises(ValueError, match="multiple of the window, or <= the window"):
        T.create_model("swin_tiny_patch4_window7_224", 1000, 384, 0.05)
    with pytest.raises(ValueError) as e:
        T.create_model("swin_giant_nothing", 1000, 224, 0.05)
    for name in sorted(WINDOW7 - {"swin_test"}) + ["swin_base_patch4_window12_384", "resnet50"]:
        assert name in str(e.value)
    assert set(swin.CONFIGS) == WINDOW7
    from imageclassification_amd.nets import ARCHS
    assert len(ARCHS) == 23


def test_multitrip_case_of_the_gpu_test_is_multitrip():
    """tests/test_window_attention_w12_gpu.py MULTITRIP by the planner mirrors: 68 windows x 32 heads walk the forward loop twice and
    the backward loop five times, both with a ragged last trip; one image fewer is a single forward trip"""
    B, Hs, Ws, H = 17, 24, 24, 32
    nwin = B * (Hs // 12) * (Ws // 12)
    assert nwin == 68
    assert (W12.fwd_grid(nwin, H), W12.trips(nwin, W12.fwd_grid(nwin, H)), nwin % W12.fwd_grid(nwin, H)) == (64, 2, 4)
    assert (W12.bwd_grid(nwin, H), W12.trips(nwin, W12.bwd_grid(nwin, H)), nwin % W12.bwd_grid(nwin, H)) == (16, 5, 4)
    assert W12.trips(64, W12.fwd_grid(64, H)) == 1
