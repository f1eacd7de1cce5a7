"""imageclassification_amd/arena.py without a GPU: the arena layout of every model family is bit-for-bit the recorded one
(tests/golden/arena_layouts.json, written by tests/golden/make_arena_layouts.py), state dicts round-trip exactly, and the torch <->
arena conversions keep their padding zero and refuse a tensor of the wrong shape.

The models construct on the CPU once hip.require_gpu, hip.load and hip.stream_ptr are replaced (the generator's `install_stubs`,
applied here through a MonkeyPatch that is undone when the module is done)."""
import importlib.util
import json
import os
import re

import pytest
import torch

from imageclassification_amd import arena
from imageclassification_amd.arena import Param, from_arena, to_arena

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_arena_layouts", os.path.join(GOLDEN, "make_arena_layouts.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(os.path.join(GOLDEN, "arena_layouts.json")) as f:
    FIXTURE = json.load(f)
# one small model of each of the four classes
SMALL = ["resnet18", "convnext_test", "vit_tiny_test", "swin_test"]


@pytest.fixture(scope="module")
def build():
    """build(model_id) -> the model, constructed once per module with device="cpu" under the three replacements."""
    mp = pytest.MonkeyPatch()
    G.install_stubs(mp.setattr)
    cache = {}

    def get(model_id):
        if model_id not in cache:
            cache[model_id] = G.build_model(model_id)
        return cache[model_id]

    yield get
    mp.undo()


def test_fixture_lists_the_models():
    assert FIXTURE["num_classes"] == G.NUM_CLASSES == 10 and list(FIXTURE["models"]) == list(G.MODELS)


@pytest.mark.parametrize("model_id", list(G.MODELS))
def test_layout_is_the_recorded_one(build, model_id):
    m = build(model_id)
    want = FIXTURE["models"][model_id]
    assert (m.n_params, m.shadow_t.numel(), len(m.params)) == (want["n_params"], want["shadow_t"], want["parameters"])
    assert G.layout_hash(m) == want["sha256"]
    # the placeholder rows of an empty job table (the kernels are handed a valid pointer and a count of 0)
    assert m._tr_tjobs.dtype == m._tr_jobs.dtype == torch.int32 and m._tr_descs.dtype == torch.int64
    assert tuple(m._tr_tjobs.shape) == (max(m._tr_ntjobs, 1), 4) and tuple(m._tr_jobs.shape) == (max(m._tr_njobs, 1), 2)
    for p in m.params.values():
        assert p.offset % 64 == 0


@pytest.mark.parametrize("model_id", list(G.MODELS))
def test_state_dict_round_trip(build, model_id):
    m = build(model_id)
    first = m.state_dict()
    # other values than the ones the model holds, so that what comes back is what was loaded
    sd = {k: (torch.tensor(7) if k.endswith("num_batches_tracked") else v * 2 + 1) for k, v in first.items()}
    assert m.load_state_dict(sd) == []
    out = m.state_dict()
    assert list(out) == list(first)
    for k, v in sd.items():
        assert out[k].dtype == first[k].dtype and out[k].shape == first[k].shape and torch.equal(out[k], v), k
    padded = [n for n, p in m.params.items() if p.numel != out[n].numel()]
    assert padded                                    # at least the 10-class head
    views = dict(m.named_parameters())
    for name in padded:                              # the arena holds the tensor and, around it, zeros
        assert torch.equal(views[name], to_arena(m.params[name], out[name])), name
    assert torch.equal(m.grad_of(next(iter(m.params))), torch.zeros_like(out[next(iter(m.params))]))


def _param(name, torch_shape, kind, padded_shape):
    n = 1
    for s in padded_shape:
        n *= s
    return Param(name, 0, n, tuple(torch_shape), kind, tuple(padded_shape))


def test_head_of_ten_classes_is_padded_with_zero_rows():
    g = torch.Generator().manual_seed(0)
    t = torch.randn(10, 32, generator=g)
    for padded in ((64, 32), (64, 1, 1, 32)):          # the transformers' [out_p][in], ResNet's 1x1 filter
        p = _param("fc.weight", (10, 32), "lin", padded)
        flat = to_arena(p, t)
        assert flat.shape == (64 * 32,) and torch.equal(flat.view(64, 32)[:10], t) and not flat.view(64, 32)[10:].any()
        assert torch.equal(to_arena(p, t.view(10, 32, 1, 1)), flat)      # a 1x1 convolution's weight loads as well
        back = from_arena(p, flat)
        assert back.shape == (10, 32) and torch.equal(back, t)
    b = torch.randn(10, generator=g)
    pb = _param("fc.bias", (10,), "vec", (64,))
    assert torch.equal(to_arena(pb, b)[:10], b) and not to_arena(pb, b)[10:].any() and torch.equal(from_arena(pb, to_arena(pb, b)), b)


def test_stem_7x7_in_its_8x8x4_layout():
    t = torch.randn(64, 3, 7, 7, generator=torch.Generator().manual_seed(1))
    p = _param("conv1.weight", (64, 3, 7, 7), "conv", (64, 8, 8, 4))
    full = to_arena(p, t).view(64, 8, 8, 4)
    assert torch.equal(full[:, :7, :7, :3], t.permute(0, 2, 3, 1))
    assert not full[:, 7].any() and not full[:, :, 7].any() and not full[..., 3].any()
    assert torch.equal(from_arena(p, full.flatten()), t)
    # the squeeze-and-excitation convolutions: (rd, C, 1, 1) is [rd][1][1][C] in memory
    se = torch.randn(4, 64, 1, 1, generator=torch.Generator().manual_seed(2))
    ps = _param("layer1.0.se.fc1.weight", (4, 64, 1, 1), "conv", (4, 1, 1, 64))
    assert torch.equal(to_arena(ps, se), se.flatten()) and torch.equal(from_arena(ps, se.flatten()), se)


def test_depthwise_filter_is_stored_taps_first():
    t = torch.randn(6, 1, 7, 7, generator=torch.Generator().manual_seed(3))
    p = _param("stages.0.blocks.0.conv_dw.weight", (6, 1, 7, 7), "dw", (7, 7, 6))
    full = to_arena(p, t).view(7, 7, 6)
    assert all(torch.equal(full[:, :, c], t[c, 0]) for c in range(6))
    assert torch.equal(from_arena(p, full.flatten()), t)


def test_vectors_of_any_rank():
    g = torch.Generator().manual_seed(4)
    for name, shape, padded in (("pos_embed", (1, 5, 8), (40,)), ("cls_token", (1, 1, 8), (8,)),
                                ("attn.relative_position_bias_table", (169, 3), (169, 3))):
        t = torch.randn(shape, generator=g)
        p = _param(name, shape, "vec", padded)
        flat = to_arena(p, t)
        assert torch.equal(flat, t.flatten())
        back = from_arena(p, flat)
        assert back.shape == shape and torch.equal(back, t)


def test_transpose_plan_order_and_alignment():
    class Layer:
        def __init__(self, offset, numel):
            self.w, self.wt_offset = Param("w", offset, numel, (), "conv", ()), None

    a, b, c = Layer(0, 128 * 2 * 64), Layer(16384, 96 * 32), Layer(19456, 64 * 64)
    descs, tjobs, jobs, size = arena.plan_transposes([(a, 128, 2, 64), (b, 96, 1, 32), (c, 64, 1, 64)])
    assert (a.wt_offset, b.wt_offset, c.wt_offset, size) == (0, 16384, 16384 + 3072, 16384 + 3072 + 4096)
    assert descs == [[0, 0, 128, 2, 64, 0, 0, 0], [16384, 16384, 96, 1, 32, 0, 0, 0], [19456, 19456, 64, 1, 64, 0, 0, 0]]
    assert tjobs == [[0, 0, 0, 0], [0, 0, 64, 0], [0, 1, 0, 0], [0, 1, 64, 0], [2, 0, 0, 0]]     # taps outermost, then co0 (, ci0)
    assert jobs == [[1, 0]]                                   # 96 x 32 is no multiple of the tile: runs of 4096 elements
    wide = Layer(0, 64 * 192)
    assert arena.plan_transposes([(wide, 64, 1, 192)])[1] == [[0, 0, 0, 0], [0, 0, 0, 64], [0, 0, 0, 128]]      # ci0 innermost
    odd = Layer(64, 100 * 100)
    _, tj, j, size = arena.plan_transposes([(odd, 100, 1, 100)])
    assert tj == [] and j == [[0, 0], [0, 4096], [0, 8192]] and size == 10112          # 10000 rounded up to 128


def _wrong_shapes(m):
    """One parameter of each kind the model has, with a tensor that is not its shape (shorter, so that padding it would 'work')."""
    seen = {}
    for name, p in m.params.items():
        if p.kind not in seen and p.torch_shape[0] > 1:
            seen[p.kind] = (name, torch.zeros((p.torch_shape[0] - 1,) + tuple(p.torch_shape[1:])))
    return list(seen.values())


@pytest.mark.parametrize("model_id", SMALL)
def test_wrong_shape_is_refused_by_name(build, model_id):
    m = build(model_id)
    good = m.state_dict()
    cases = _wrong_shapes(m)
    assert {m.params[n].kind for n, _ in cases} >= {"vec", "lin", "conv"}
    for name, bad in cases + [(next(iter(m.params)), torch.zeros(3))]:
        sd = dict(good)
        sd[name] = bad
        with pytest.raises(ValueError, match=re.escape(f"size mismatch for {name}: {tuple(bad.shape)}")):
            m.load_state_dict(sd)
    m.load_state_dict(good)


@pytest.mark.parametrize("model_id", SMALL)
def test_missing_key(build, model_id):
    m = build(model_id)
    good = m.state_dict()
    gone = [list(m.params)[3]]
    if model_id == "resnet18":
        gone.append("layer1.0.bn1.running_var")        # buffers are expected too
    sd = {k: v for k, v in good.items() if k not in gone}
    with pytest.raises(KeyError, match="missing keys in state_dict"):
        m.load_state_dict(sd)
    with pytest.raises(KeyError):
        m.load_state_dict(sd, strict=True)
    assert m.load_state_dict(sd, strict=False) == gone
    after = m.state_dict()
    assert all(torch.equal(after[k], good[k]) for k in good)       # what was not given keeps its value
