"""MobileNetV2 without a GPU: timm's names, shapes and order, the five published parameter counts, the command-line surface, state-dict
round trips (the depthwise filter's [3][3][C] arena layout included), the reference module against a plain nn.Sequential in fp64, the
new entries in header, library and ctypes table, their host-side answers, and the loop counts of csrc/dwconv3x3.hip at the shapes
tests/test_dwconv3_gpu.py runs.

The models construct on the CPU under the replacements of tests/golden/make_arena_layouts.py (install_stubs)."""
import importlib.util
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

import _dwconv as D
from oracle.mobilenet_ref import MobileNetV2Ref, WIDTHS, layer_list, param_count, plain_sequential

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLISHED = {"mobilenetv2_035": 1677128, "mobilenetv2_050": 1968680, "mobilenetv2_075": 2636424, "mobilenetv2_100": 3504872,
             "mobilenetv2_140": 6108776}
NEW_ENTRIES = {"icamd_dwconv3_supported": 5, "icamd_dwconv3_stats_rows": 5, "icamd_dwconv3_fwd": 12, "icamd_dwconv3_dgrad": 9,
               "icamd_dwconv3_wgrad_workspace_bytes": 5, "icamd_dwconv3_wgrad": 14, "icamd_bn_apply_relu6": 7,
               "icamd_bn_bwd_relu6_workspace_bytes": 2, "icamd_bn_bwd_relu6": 15}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


L = _load("make_arena_layouts")


@pytest.fixture()
def stubs(monkeypatch):
    L.install_stubs(monkeypatch.setattr)


def _build(arch, num_classes=10):
    from imageclassification_amd.mobilenet import MobileNetV2
    return MobileNetV2(arch, num_classes, device="cpu", seed=0)


@pytest.mark.parametrize("arch", list(PUBLISHED) + ["mobilenetv2_test"])
def test_names_shapes_order_and_count(stubs, arch):
    from imageclassification_amd import mobilenet
    net = _build(arch, 1000)
    ref = MobileNetV2Ref(arch, 1000)
    sd, rsd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    assert [(n, tuple(p.shape)) for n, p in ref.named_parameters()] == mobilenet.param_shapes(arch, 1000)
    count = sum(p.numel() for p in ref.parameters())
    assert count == param_count(arch) == sum(v.numel() for k, v in sd.items() if k in net.params)
    if arch in PUBLISHED:
        assert count == PUBLISHED[arch]
    stem, stages, head = layer_list(arch)
    assert net.feat_dim == head and len(net.blocks) == sum(len(s) for s in stages)
    assert all(b.c % 8 == 0 for b in net.bns) and all(c.cin_p % 8 == 0 and c.cout_p % 8 == 0 for c in net.convs)


def test_widths_of_the_issue():
    """the depthwise widths and the narrowest pointwise layer across the five models"""
    dw, pw = set(), set()
    for arch in WIDTHS:
        stem, stages, _ = layer_list(arch)
        for stage in stages:
            for kind, cin, mid, cout, _ in stage:
                dw.add(mid)
                pw |= {(cin, mid), (mid, cout)} if kind == "ir" else {(cin, cout)}
    assert sorted(dw) == [16, 24, 32, 48, 96, 144, 192, 288, 336, 384, 432, 480, 528, 576, 720, 816, 960, 1344]
    assert min(min(p) for p in pw) == 8 and (8, 48) in pw
    assert layer_list("mobilenetv2_140")[2] == 1792 and layer_list("mobilenetv2_035")[2] == 1280


def test_create_model_accepts_the_family(stubs, monkeypatch):
    sys.path.insert(0, ROOT)
    import train as TR
    from imageclassification_amd.mobilenet import MobileNetV2

    class OnCpu(MobileNetV2):
        def __init__(self, arch, num_classes, **kw):
            super().__init__(arch, num_classes, device="cpu", seed=0, **kw)

    monkeypatch.setattr(TR, "MobileNetV2", OnCpu)
    for arch in list(PUBLISHED) + ["mobilenetv2_test"]:
        net = TR.create_model(arch, 10, 224, 0.3)                 # --drop_path does not reach the family
        assert isinstance(net, MobileNetV2) and net.arch == arch and net.num_classes == 10 and not hasattr(net, "drop_path_rate")
    with pytest.raises(ValueError, match="mobilenetv2_100"):       # the names are in the "available" list
        TR.create_model("mobilenetv2_110d", 10, 224, 0.0)


def test_state_dict_round_trip_is_exact(stubs):
    torch.manual_seed(3)
    ref = MobileNetV2Ref("mobilenetv2_test", 10)
    g = torch.Generator().manual_seed(4)
    sd = {k: (torch.randn(v.shape, generator=g) if v.dtype.is_floating_point else torch.tensor(7)) for k, v in ref.state_dict().items()}
    net = _build("mobilenetv2_test")
    assert net.load_state_dict(sd) == []
    back = net.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], v) for k, v in sd.items())
    assert net.num_batches_tracked == 7
    # the depthwise filter sits tap-major in the arena
    p = net.params["blocks.1.0.conv_dw.weight"]
    assert p.kind == "dw" and p.torch_shape == (48, 1, 3, 3) and p.padded_shape == (3, 3, 48)
    flat = net.param_arena[p.offset:p.offset + p.numel].reshape(3, 3, 48)
    assert torch.equal(flat, sd["blocks.1.0.conv_dw.weight"][:, 0].permute(1, 2, 0))
    with pytest.raises(KeyError):
        net.load_state_dict({k: v for k, v in sd.items() if k != "bn2.running_var"})
    with pytest.raises(ValueError):
        net.load_state_dict({**sd, "blocks.1.0.conv_dw.weight": torch.zeros(48, 1, 5, 5)})


def test_reference_equals_plain_sequential_in_fp64():
    torch.manual_seed(0)
    ref = MobileNetV2Ref("mobilenetv2_test", 10, bf16_points=False).double()
    seq = plain_sequential("mobilenetv2_test", 10).double()
    with torch.no_grad():
        for p, q in zip(seq.parameters(), ref.parameters()):
            assert p.shape == q.shape
            p.copy_(q)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 64, 64, generator=g, dtype=torch.float64)
    y = torch.randint(0, 10, (4,), generator=g)
    outs = []
    for m in (ref, seq):
        m.train()
        o = m(x)
        F.cross_entropy(o, y).backward()
        outs.append(o.detach())
    assert torch.allclose(outs[0], outs[1], rtol=1e-12, atol=1e-12)
    for p, q in zip(seq.parameters(), ref.parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-9, atol=1e-12)
    for (kb, b), (kr, r) in zip(seq.named_buffers(), ref.named_buffers()):
        assert torch.allclose(b.double(), r.double(), rtol=1e-12, atol=1e-12), (kb, kr)


def test_new_entries_in_header_library_and_ctypes_table():
    from imageclassification_amd import hip
    header = open(os.path.join(ROOT, "include", "icamd.h")).read()
    for name, nargs in NEW_ENTRIES.items():
        assert name in hip._SIGNATURES_ADDED and name not in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS
        res, args = hip._SIGNATURES_ADDED[name]
        assert len(args) == nargs, name
        m = re.search(r"(int|size_t) " + name + r"\(([^;]*?)\);", header, re.S)
        assert m is not None, name
        assert len(m.group(2).split(",")) == nargs, name
        assert (m.group(1) == "size_t") == (res is hip.c_size_t), name
    lib = hip.load()                                      # binds both tables: a missing symbol raises here
    assert hip.ABI_VERSION == 6 and lib.icamd_abi_version() == 6
    internal = open(os.path.join(ROOT, "imageclassification_amd", "csrc", "icamd_internal.h")).read()
    for launcher in ("icamd_dwconv3_fwd_launch(", "icamd_dwconv3_dgrad_launch(", "icamd_dwconv3_wgrad_launch(",
                     "icamd_bn_apply_relu6_launch(", "icamd_bn_bwd_relu6_launch("):
        assert launcher in internal
    units = open(os.path.join(ROOT, "imageclassification_amd", "csrc", "build.sh")).read().split('UNITS="')[1].split('"')[0].split()
    assert "dwconv3x3" in units


def test_host_side_answers():
    from imageclassification_amd import hip
    lib = hip.load()
    ok = (2, 7, 7, 24, 2)
    assert lib.icamd_dwconv3_supported(*ok) == 1 and lib.icamd_dwconv3_stats_rows(*ok) > 0
    assert lib.icamd_dwconv3_wgrad_workspace_bytes(*ok) > 0 and lib.icamd_bn_bwd_relu6_workspace_bytes(98, 24) > 0
    for bad in ((2, 7, 7, 20, 2), (2, 7, 7, 24, 3), (2, 7, 7, 24, 0), (0, 7, 7, 24, 1), (2, 0, 7, 24, 1), (2, 7, 7, 0, 1)):
        assert lib.icamd_dwconv3_supported(*bad) == 0 and lib.icamd_dwconv3_stats_rows(*bad) == 0
        assert lib.icamd_dwconv3_wgrad_workspace_bytes(*bad) == 0
    assert lib.icamd_bn_bwd_relu6_workspace_bytes(0, 24) == 0 and lib.icamd_bn_bwd_relu6_workspace_bytes(98, 0) == 0
    # the geometry the tests name their loops by is the library's
    for shape in D.SHAPES + [(256, 112, 112, 32), (256, 56, 56, 144), (256, 7, 7, 960)]:
        for stride in (1, 2):
            assert lib.icamd_dwconv3_stats_rows(*shape, stride) == D.fwd_geometry(*shape, stride)["rows"]
            assert lib.icamd_dwconv3_wgrad_workspace_bytes(*shape, stride) == D.wgrad_geometry(*shape, stride)["rows"] * 9 * shape[3] * 4
    # every launching entry refuses all-zero arguments (before any launch: this runs without a GPU)
    assert lib.icamd_dwconv3_fwd(None, None, None, None, None, None, 0, 0, 0, 0, 0, None) != 0
    assert lib.icamd_dwconv3_dgrad(None, None, None, 0, 0, 0, 0, 0, None) != 0
    assert lib.icamd_dwconv3_wgrad(None, None, None, None, None, 0, None, 0, 0, 0, 0, 0, 0, None) != 0
    assert lib.icamd_bn_apply_relu6(None, None, None, None, 0, 0, None) != 0
    assert lib.icamd_bn_bwd_relu6(None, None, None, None, None, None, None, None, None, 0, 0, 0, None, 0, None) != 0


def test_loop_counts_at_the_gpu_test_shapes():
    """what the docstring of tests/test_dwconv3_gpu.py says each shape drives through more than one trip"""
    t = {(shape, s): D.trips(*shape, s) for shape in D.SHAPES for s in (1, 2)}
    big = t[((3, 57, 57, 96), 1)]
    assert big["rows of a segment"] == 16 and big["row segments"] == 4 and big["column groups"] == 3
    assert big["LDS outputs of a kernel row of taps (o += 256)"] == 2
    assert all(v["column lanes folded per output"] >= 3 for v in t.values())
    assert t[((2, 8, 8, 528), 1)]["LDS outputs of the statistics fold (o += 256)"] == 5
    assert t[((2, 14, 14, 144), 2)]["LDS outputs of the statistics fold (o += 256)"] == 2
    assert t[((2, 8, 8, 528), 2)]["LDS outputs of a kernel row of taps (o += 256)"] == 7
    items = [(t[((2100, 3, 5, 16), s)]["items of a workgroup, forward"], t[((2100, 3, 5, 16), s)]["items of a workgroup, weight gradient"])
             for s in (1, 2)]
    assert items == [(2, 5), (3, 11)]
    assert all(v["items of a workgroup, forward"] == 1 for (shape, _), v in t.items() if shape != (2100, 3, 5, 16))
    assert t[((2, 5, 5, 1344), 1)]["channel slices per pixel"] == 2
    assert sum(v["partial rows, forward"] > 1 for v in t.values()) >= 12


def test_route_constants_are_not_environment_switches():
    src = open(os.path.join(ROOT, "imageclassification_amd", "mobilenet.py")).read()
    assert "os.environ" not in src and "getenv" not in src and "import os" not in src
    from imageclassification_amd import mobilenet
    assert set(mobilenet.DW_ONLOAD) == {"fwd", "wgrad"} and all(isinstance(v, bool) for v in mobilenet.DW_ONLOAD.values())
    kernels = open(os.path.join(ROOT, "imageclassification_amd", "csrc", "dwconv3x3.hip")).read()
    assert "getenv" not in kernels and "icamd_env_int" not in kernels and "atomic" not in kernels.lower().replace("no atomics", "")
