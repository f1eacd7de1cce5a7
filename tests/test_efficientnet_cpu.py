"""EfficientNet-B0 / B1 without a GPU: timm's names, shapes and order, the two published parameter counts, the squeeze-and-excitation
widths, the command-line surface, state-dict round trips (the 4-D squeeze-and-excitation shapes and the [5][5][C] arena layout included),
the new entries in header, library and ctypes table and their host-side answers, the two-pass reference of the BatchNorm + SiLU + SE
backward against fp64 autograd, and the loop counts of csrc/dwconv5x5.hip at the shapes tests/test_dwconv5_gpu.py runs.

The models construct on the CPU under the replacements of tests/golden/make_arena_layouts.py (install_stubs)."""
import importlib.util
import os
import re
import sys

import pytest
import torch

import _dwconv as D
from oracle import efficientnet_ref as E
from oracle import ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"icamd_dwconv5_supported": 5, "icamd_dwconv5_stats_rows": 5, "icamd_dwconv5_fwd": 10, "icamd_dwconv5_dgrad": 9,
               "icamd_dwconv5_wgrad_workspace_bytes": 5, "icamd_dwconv5_wgrad": 12, "icamd_bn_apply_silu": 9,
               "icamd_bn_silu_squeeze_workspace_bytes": 3, "icamd_bn_silu_squeeze": 10, "icamd_se_excite_silu_fwd": 13,
               "icamd_se_silu_bwd_reduce_workspace_bytes": 3, "icamd_se_silu_bwd_reduce": 11, "icamd_se_excite_silu_bwd": 17,
               "icamd_bn_bwd_silu_workspace_bytes": 3, "icamd_bn_bwd_silu": 18}
ARCHS = ["efficientnet_b0", "efficientnet_b1", "efficientnet_test"]


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
    from imageclassification_amd.efficientnet import EfficientNet
    return EfficientNet(arch, num_classes, device="cpu", seed=0)


@pytest.mark.parametrize("arch", ARCHS)
def test_names_shapes_order_and_count(stubs, arch):
    from imageclassification_amd import efficientnet
    net = _build(arch, 1000)
    ref = E.EfficientNetRef(arch, 1000)
    sd, rsd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    assert [(n, tuple(p.shape)) for n, p in ref.named_parameters()] == efficientnet.param_shapes(arch, 1000)
    count = sum(p.numel() for p in ref.parameters())
    assert count == E.param_count(arch) == sum(v.numel() for k, v in sd.items() if k in net.params)
    if arch in E.PUBLISHED:
        assert count == E.PUBLISHED[arch]
    # each BatchNorm's buffers sit right behind its bias
    keys = list(sd)
    for i, k in enumerate(keys):
        if k.endswith(".running_mean"):
            stem = k[:-len("running_mean")]
            assert keys[i - 1] == stem + "bias" and keys[i + 1] == stem + "running_var" and keys[i + 2] == stem + "num_batches_tracked"
    # the squeeze-and-excitation parameters are 4-D and sit between the depthwise BatchNorm and the projection convolution
    i = keys.index("blocks.1.0.se.conv_reduce.weight")
    assert keys[i - 1] == "blocks.1.0.bn2.num_batches_tracked" and keys[i + 4] == "blocks.1.0.conv_pwl.weight"
    assert sd[keys[i]].dim() == 4 and sd[keys[i + 2]].dim() == 4 and sd[keys[i + 1]].dim() == 1
    stem, stages, head = E.layer_list(arch)
    assert net.feat_dim == head and len(net.blocks) == sum(len(s) for s in stages)
    assert all(b.c % 8 == 0 for b in net.bns) and all(c.cin_p % 8 == 0 and c.cout_p % 8 == 0 for c in net.convs)


def test_se_widths_repeats_and_kernels(stubs):
    """The reduced widths are a quarter of each block's INPUT width: 32 | 16, 24 | 24, 40 | 40, 80, 80 | 80, 112, 112 | 112, 192, 192,
    192 | 192.  (The issue listed 8, 4, 4, 6, 6, 10, 10, 20, 20, 20, 28, 28, 28, 48, 48, 48 -- one 4 too many and one 48 too few for
    that rule; only the list below gives the published 5 288 548 parameters, which test_names_shapes_order_and_count holds.)"""
    b0, b1 = _build("efficientnet_b0"), _build("efficientnet_b1")
    assert [blk.se.rd for blk in b0.blocks] == [8, 4, 6, 6, 10, 10, 20, 20, 20, 28, 28, 28, 48, 48, 48, 48]
    assert [blk.se.rd for blk in b0.blocks] == [blk.cin // 4 for blk in b0.blocks]
    assert sum(blk.dw.k == 5 for blk in b0.blocks) == 9 and len(b0.blocks) == 16
    per_stage = {}
    for blk in b1.blocks:
        per_stage[blk.name.split(".")[1]] = per_stage.get(blk.name.split(".")[1], 0) + 1
    assert list(per_stage.values()) == [2, 3, 3, 4, 4, 5, 2]
    assert b1.blocks[1].kind == "ds" and b1.blocks[1].residual and not b1.blocks[0].residual
    # the widths the 5x5 kernels and the gate kernels meet, as (C, rd)
    assert sorted({(blk.dw.c, blk.se.rd) for blk in b0.blocks if blk.dw.k == 5}) == [(144, 6), (240, 10), (480, 20), (672, 28), (1152, 48)]
    test = _build("efficientnet_test")
    assert [(blk.kind, blk.dw.k, blk.stride, blk.residual) for blk in test.blocks] == [
        ("ds", 3, 1, False), ("ir", 3, 2, False), ("ir", 3, 1, True), ("ir", 5, 2, False), ("ir", 5, 1, False), ("ir", 5, 1, True)]


def test_create_model_accepts_the_family(stubs, monkeypatch):
    sys.path.insert(0, ROOT)
    import train as TR
    from imageclassification_amd.efficientnet import EfficientNet

    class OnCpu(EfficientNet):
        def __init__(self, arch, num_classes, **kw):
            super().__init__(arch, num_classes, device="cpu", seed=0, **kw)

    monkeypatch.setattr(TR, "EfficientNet", OnCpu)
    for arch in ARCHS:
        args = TR.get_args_parser().parse_args(["--model", arch])
        net = TR.create_model(args.model, 10, 224, 0.3)                 # --drop_path does not reach the family
        assert isinstance(net, EfficientNet) and net.arch == arch and net.num_classes == 10 and not hasattr(net, "drop_path_rate")
    with pytest.raises(ValueError, match="efficientnet_b1"):            # the names are in the "available" list
        TR.create_model("efficientnet_b2", 10, 224, 0.0)


def test_state_dict_round_trip_is_exact(stubs):
    torch.manual_seed(3)
    ref = E.EfficientNetRef("efficientnet_test", 10)
    g = torch.Generator().manual_seed(4)
    sd = {k: (torch.randn(v.shape, generator=g) if v.dtype.is_floating_point else torch.tensor(7)) for k, v in ref.state_dict().items()}
    net = _build("efficientnet_test")
    assert net.load_state_dict(sd) == []
    back = net.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], v) for k, v in sd.items())
    assert net.num_batches_tracked == 7
    # the 5x5 depthwise filter sits tap-major in the arena, the squeeze-and-excitation filters in torch layout
    p = net.params["blocks.2.0.conv_dw.weight"]
    assert p.kind == "dw" and p.torch_shape == (96, 1, 5, 5) and p.padded_shape == (5, 5, 96)
    flat = net.param_arena[p.offset:p.offset + p.numel].reshape(5, 5, 96)
    assert torch.equal(flat, sd["blocks.2.0.conv_dw.weight"][:, 0].permute(1, 2, 0))
    q = net.params["blocks.2.0.se.conv_reduce.weight"]
    assert q.torch_shape == (4, 96, 1, 1) and torch.equal(net.param_arena[q.offset:q.offset + q.numel].reshape(4, 96),
                                                          sd["blocks.2.0.se.conv_reduce.weight"][:, :, 0, 0])
    with pytest.raises(ValueError):
        net.load_state_dict({**sd, "blocks.2.0.se.conv_expand.weight": torch.zeros(96, 4)})


def test_init_is_goog(stubs):
    net = _build("efficientnet_b0", 1000)
    sd = net.state_dict()
    for k, want in (("blocks.2.0.conv_dw.weight", (2 / 25) ** 0.5), ("blocks.5.0.se.conv_expand.weight", (2 / 672) ** 0.5),
                    ("blocks.5.0.se.conv_reduce.weight", (2 / 28) ** 0.5), ("conv_head.weight", (2 / 1280) ** 0.5)):
        assert abs(float(sd[k].std()) / want - 1) < 0.1, k
    assert all(float(v.abs().max()) == 0 for k, v in sd.items() if ".se." in k and k.endswith(".bias"))


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
    for launcher in ("icamd_dwconv5_fwd_launch(", "icamd_dwconv5_dgrad_launch(", "icamd_dwconv5_wgrad_launch(", "icamd_bn_apply_silu_launch(",
                     "icamd_silu_rowsum_launch(", "icamd_se_excite_silu_fwd_launch(", "icamd_se_excite_silu_bwd_launch(",
                     "icamd_bn_bwd_silu_launch("):
        assert launcher in internal
    assert "dwconv5x5" in open(os.path.join(ROOT, "imageclassification_amd", "csrc", "build.sh")).read()
    kernels = open(os.path.join(ROOT, "imageclassification_amd", "csrc", "dwconv5x5.hip")).read()
    assert "getenv" not in kernels and "icamd_env_int" not in kernels and "atomic" not in kernels.lower().replace("no atomics", "")
    src = open(os.path.join(ROOT, "imageclassification_amd", "efficientnet.py")).read()
    assert "os.environ" not in src and "getenv" not in src and "import os" not in src


def test_host_side_answers():
    from imageclassification_amd import hip
    lib = hip.load()
    ok = (2, 7, 7, 24, 2)
    assert lib.icamd_dwconv5_supported(*ok) == 1 and lib.icamd_dwconv5_stats_rows(*ok) > 0 and lib.icamd_dwconv5_wgrad_workspace_bytes(*ok) > 0
    assert lib.icamd_dwconv5_supported(2, 2, 3, 8, 1) == 1                # an image smaller than the filter
    for bad in ((2, 7, 7, 20, 2), (2, 7, 7, 24, 3), (2, 7, 7, 24, 0), (0, 7, 7, 24, 1), (2, 0, 7, 24, 1), (2, 7, 7, 0, 1)):
        assert lib.icamd_dwconv5_supported(*bad) == 0 and lib.icamd_dwconv5_stats_rows(*bad) == 0
        assert lib.icamd_dwconv5_wgrad_workspace_bytes(*bad) == 0
    # the geometry the tests name their loops by is the library's
    for shape in D.SHAPES5 + [(256, 56, 56, 144), (256, 28, 28, 240), (256, 14, 14, 672), (256, 7, 7, 1152)]:
        for stride in (1, 2):
            assert lib.icamd_dwconv5_stats_rows(*shape, stride) == D.fwd_geometry(*shape, stride)["rows"]
            assert lib.icamd_dwconv5_wgrad_workspace_bytes(*shape, stride) == D.wgrad_geometry(*shape, stride)["rows"] * 25 * shape[3] * 4
    queries = (lib.icamd_bn_silu_squeeze_workspace_bytes, lib.icamd_se_silu_bwd_reduce_workspace_bytes, lib.icamd_bn_bwd_silu_workspace_bytes)
    assert all(q(2, 49, 144) > 0 for q in queries)
    assert lib.icamd_bn_bwd_silu_workspace_bytes(2, 49, 144) == lib.icamd_bn_bwd_workspace_bytes(98, 144)
    for bad in ((2, 49, 20), (2, 49, 4104), (0, 49, 144), (2, 0, 144)):
        assert all(q(*bad) == 0 for q in queries)
    # every launching entry refuses all-zero arguments (before any launch: this runs without a GPU)
    assert lib.icamd_dwconv5_fwd(None, None, None, None, 0, 0, 0, 0, 0, None) != 0
    assert lib.icamd_dwconv5_dgrad(None, None, None, 0, 0, 0, 0, 0, None) != 0
    assert lib.icamd_dwconv5_wgrad(None, None, None, 0, None, 0, 0, 0, 0, 0, 0, None) != 0
    assert lib.icamd_bn_apply_silu(None, None, None, None, None, 0, 0, 0, None) != 0
    assert lib.icamd_bn_silu_squeeze(None, None, None, None, 0, 0, 0, None, 0, None) != 0
    assert lib.icamd_se_excite_silu_fwd(None, 0.0, None, None, None, None, None, None, None, 0, 0, 0, None) != 0
    assert lib.icamd_se_silu_bwd_reduce(None, None, None, None, None, 0, 0, 0, None, 0, None) != 0
    assert lib.icamd_se_excite_silu_bwd(*([None] * 11), 0, 0, 0, 0.0, 0, None) != 0
    assert lib.icamd_bn_bwd_silu(*([None] * 11), 0, 0, 0, 0, None, 0, None) != 0


@pytest.mark.parametrize("N,HW,C,rd", [(3, 7, 16, 4), (2, 1, 8, 1), (4, 12, 24, 6)])
def test_two_pass_reference_equals_fp64_autograd(N, HW, C, rd):
    """the kernels' form (squeeze pass, excite, apply pass; gate-gradient pass, excite backward, reduce pass, apply pass) is the
    derivative of out = silu(bn(y)) * sigmoid(W2 silu(W1 mean(silu(bn(y))) + b1) + b2)"""
    g = torch.Generator().manual_seed(10 * N + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)     # noqa: E731
    args = (r(N, HW, C) * 1.5 + r(C), r(C) + 2, r(C), r(rd, C), r(rd), r(C, rd), r(C), r(N, HW, C))
    out, grads = R.se_block_two_pass(*args)
    out64, grads64 = R.se_block_autograd(*args)
    assert torch.allclose(out, out64, rtol=1e-10, atol=1e-10)
    for k in grads64:
        assert torch.allclose(grads[k], grads64[k], rtol=1e-10, atol=1e-10), k


def test_reference_without_rounding_points_is_the_plain_network():
    """EfficientNetRef(bf16_points=False) in fp64 == the same layers applied by hand from its state_dict (one block of every kind)"""
    import torch.nn.functional as F
    torch.manual_seed(0)
    ref = E.EfficientNetRef("efficientnet_test", 10).double().eval()
    E.perturb(ref, 1)
    sd = ref.state_dict()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 32, 32, generator=g, dtype=torch.float64)

    def bn(t, n):
        return F.batch_norm(t, sd[n + ".running_mean"], sd[n + ".running_var"], sd[n + ".weight"], sd[n + ".bias"], False, 0.0, 1e-5)

    def se(t, n):
        s = t.mean((2, 3), keepdim=True)
        h = F.silu(F.conv2d(s, sd[n + ".conv_reduce.weight"], sd[n + ".conv_reduce.bias"]))
        return t * torch.sigmoid(F.conv2d(h, sd[n + ".conv_expand.weight"], sd[n + ".conv_expand.bias"]))

    t = F.silu(bn(F.conv2d(x, sd["conv_stem.weight"], None, 2, 1), "bn1"))
    for si, stage in enumerate(E.layer_list("efficientnet_test")[1]):
        for bi, (kind, k, cin, mid, cout, s, rd) in enumerate(stage):
            n, inp = f"blocks.{si}.{bi}", t
            if kind == "ir":
                t = F.silu(bn(F.conv2d(t, sd[n + ".conv_pw.weight"]), n + ".bn1"))
            dwbn = ".bn2" if kind == "ir" else ".bn1"
            t = se(F.silu(bn(F.conv2d(t, sd[n + ".conv_dw.weight"], None, s, k // 2, 1, t.shape[1]), n + dwbn)), n + ".se")
            assert sd[n + ".se.conv_reduce.weight"].shape[0] == rd
            t = bn(F.conv2d(t, sd[n + (".conv_pwl.weight" if kind == "ir" else ".conv_pw.weight")]), n + (".bn3" if kind == "ir" else ".bn2"))
            if s == 1 and cin == cout:
                t = t + inp
    t = F.silu(bn(F.conv2d(t, sd["conv_head.weight"]), "bn2")).mean((2, 3))
    want = F.linear(t, sd["classifier.weight"], sd["classifier.bias"])
    with torch.no_grad():
        assert torch.allclose(ref(x), want, rtol=1e-12, atol=1e-12)


def test_loop_counts_at_the_gpu_test_shapes():
    """what the docstring of tests/test_dwconv5_gpu.py says each shape drives through more than one trip: the issue's list runs every
    loop whose length depends on the problem more than once"""
    t = {(shape, s): D.trips(*shape, s, k=5) for shape in D.SHAPES5 for s in (1, 2)}
    for name in next(iter(t.values())):
        assert any(v[name] > 1 for v in t.values()), name
    big = t[((3, 37, 41, 40), 1)]
    assert big["rows of a segment"] == 16 and big["row segments"] == 3 and t[((3, 37, 41, 40), 2)]["row segments"] == 2
    assert t[((2, 5, 5, 1152), 1)]["column groups"] == 2 and t[((2, 5, 5, 1152), 1)]["channel slices per pixel"] == 2
    assert min(v["column lanes folded per output"] for v in t.values()) == 3
    assert max(v["column lanes folded per output"] for v in t.values()) == 256
    assert t[((2, 14, 14, 144), 1)]["LDS outputs of the statistics fold (o += 256)"] == 2
    assert t[((2, 5, 5, 1152), 2)]["LDS outputs of the statistics fold (o += 256)"] == 5
    assert t[((2, 14, 14, 144), 2)]["LDS outputs of a kernel row of taps (o += 256)"] == 3
    assert t[((2, 5, 5, 1152), 1)]["LDS outputs of a kernel row of taps (o += 256)"] == 12
    items = [(t[((2100, 3, 5, 16), s)]["items of a workgroup, forward"], t[((2100, 3, 5, 16), s)]["items of a workgroup, weight gradient"])
             for s in (1, 2)]
    assert items == [(2, 5), (3, 11)]
    assert all(v["items of a workgroup, forward"] == 1 for (shape, _), v in t.items() if shape != (2100, 3, 5, 16))
    assert sum(v["partial rows, forward"] > 1 for v in t.values()) >= 12
