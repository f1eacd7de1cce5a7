"""The library calls of a ViT, Swin and ConvNeXt training step, without a GPU: every launch of construct / pack / forward / backward /
accumulating backward / eval forward / reload -- entry, arguments, buffers, stream, order, side-lane waits and gradient-hook calls --
is the recorded one (tests/golden/call_traces.json, written by tests/golden/make_call_traces.py, whose docstring states what a
record holds), and a seed still gives the weights it gave.

The replacements (the generator's `install_recorders`) go through a MonkeyPatch that is undone when the module is done."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_call_traces", os.path.join(GOLDEN, "make_call_traces.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(os.path.join(GOLDEN, "call_traces.json")) as f:
    FIXTURE = json.load(f)


@pytest.fixture(scope="module")
def recorders():
    mp = pytest.MonkeyPatch()
    G.install_recorders(mp.setattr)
    yield mp
    mp.undo()


def test_fixture_lists_the_cases():
    assert FIXTURE["num_classes"] == G.L.NUM_CLASSES == 10 and FIXTURE["batch"] == G.BATCH == 2
    assert list(FIXTURE["cases"]) == list(G.CASES) and list(FIXTURE["state_dict_seed0"]) == list(G.MODELS)
    assert {G.CASES[c][0] for c in G.CASES} == set(G.MODELS)


@pytest.mark.parametrize("case_id", list(G.CASES))
def test_calls_are_the_recorded_ones(recorders, case_id):
    def setenv(name, value):
        recorders.delenv(name, raising=False) if value is None else recorders.setenv(name, value)

    got = G.run_case(case_id, setenv)
    want = FIXTURE["cases"][case_id]
    assert got["calls"] == want["calls"]
    assert got["stream_queries"] == want["stream_queries"]
    assert got["sha256"] == want["sha256"]


def test_the_cases_take_the_paths_they_are_there_for(recorders):
    """The side lane's launches carry stream 1 and make the main stream wait; the drop-path detour adds its kernels."""
    def launches(case_id):
        """(entry, its last argument: the stream of a launch) of every record but the size and support queries"""
        G.run_case(case_id, lambda k, v: recorders.delenv(k, raising=False) if v is None else recorders.setenv(k, v))
        return [(r[0], r[2][-1]) for r in G.TRACE if not r[0].endswith(("_bytes", "_supported"))]

    for on, off in (("vit_tiny_test/lane_on", "vit_tiny_test/lane_off"), ("convnext_test/lane_on", "convnext_test/lane_off")):
        a, b = launches(on), launches(off)
        assert ("icamd_conv2d_wgrad_bias", 1) in a and ("lane.before_write", None) in a
        assert all(s == 0 for n, s in b if n.startswith("icamd_")) and not any(n == "lane.before_write" for n, _ in b)
    for model in ("swin_test", "swin_test_w12"):
        drop, plain = launches(model + "/drop"), launches(model + "/no_drop")
        # blocks 1..3 have a rate above 0: two branches each, one training forward and two backward passes
        assert [n for n, _ in drop].count("icamd_layerscale_fwd") == 6 and [n for n, _ in drop].count("icamd_layerscale_bwd") == 12
        assert not any(n.startswith("icamd_layerscale") for n, _ in plain)
        assert all(s == 0 for n, s in drop + plain if n.startswith("icamd_"))      # Swin has no side lane


@pytest.mark.parametrize("model_id", list(G.MODELS))
def test_seed_0_gives_the_recorded_weights(recorders, model_id):
    """Names and shapes exactly; sums and sampled elements to the generator's state_tol (last-bit differences between CPUs)."""
    model = G.build_model(model_id)
    got, want = G.state_record(model), FIXTURE["state_dict_seed0"][model_id]
    assert got["names_and_shapes_sha256"] == want["names_and_shapes_sha256"]
    assert len(got["values"]) == len(want["values"]) == len(model.params)
    worst = [0.0, 0.0]
    for (name, t), g, w in zip(model.state_dict().items(), got["values"], want["values"]):
        assert float(t.abs().max()) < 0.25 or bool((t == 1).all()), name          # what state_tol assumes
        tol_sum, tol_el = G.state_tol(t.numel())
        worst = [max(worst[0], abs(g[0] - w[0]) / tol_sum), max(worst[1], max(abs(a - b) for a, b in zip(g[1:], w[1:])) / tol_el)]
        assert abs(g[0] - w[0]) <= tol_sum, name
        assert all(abs(a - b) <= tol_el for a, b in zip(g[1:], w[1:])), name
    print(f"{model_id}: largest deviation / tolerance: sums {worst[0]:.3g}, elements {worst[1]:.3g}")


def test_a_pointer_into_no_tensor_fails():
    x = torch.zeros(4)
    buf = torch.zeros(8)
    held = {buf.untyped_storage().data_ptr(): (buf.untyped_storage().nbytes(), buf),
            x.untyped_storage().data_ptr(): (x.untyped_storage().nbytes(), x)}
    P = ctypes.c_void_p
    ok = [("icamd_f32_to_bf16", (P, P, ctypes.c_longlong, P), (x.data_ptr(), buf.data_ptr() + 4, 8, 0))]
    assert G.canonical(ok, held, x) == [["icamd_f32_to_bf16", "input", [0, 4, 32], 8, "stream 0"]]
    past = [("icamd_f32_to_bf16", (P, P, ctypes.c_longlong, P), (x.data_ptr(), buf.data_ptr() + 32, 8, 0))]
    with pytest.raises(LookupError, match="is in no tensor of the model"):
        G.canonical(past, held, x)
