"""The library calls of a ViT, Swin, ConvNeXt (V1 folded and unfolded, V2), ResNet (nets.py), MobileNetV2 and EfficientNet training step,
without a GPU: every launch of construct / pack / forward / backward /
accumulating backward / eval forward (ResNet: twice) / reload -- entry, arguments, buffers, stream, order, side-lane waits and gradient-hook calls --
is the recorded one (tests/golden/call_traces.json, written by tests/golden/make_call_traces.py, whose docstring states what a
record holds), and a seed still gives the weights it gave.

The replacements (the generator's `install_recorders`) go through a MonkeyPatch that is undone when the module is done."""
import ctypes
import importlib.util
import json
import os
import re

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
    assert list(FIXTURE["cases"]) == list(G.CASES) and list(FIXTURE["state_dict_seed0"]) == list(G.STATE_MODELS)
    assert {G.CASES[c][0] for c in G.CASES} == set(G.MODELS)


@pytest.mark.parametrize("case_id", list(G.CASES))
def test_calls_are_the_recorded_ones(recorders, case_id):
    def setenv(name, value):
        recorders.delenv(name, raising=False) if value is None else recorders.setenv(name, value)

    got = G.run_case(case_id, setenv, setattr_fn=recorders.setattr)
    want = FIXTURE["cases"][case_id]
    assert got["calls"] == want["calls"]
    assert got["stream_queries"] == want["stream_queries"]
    assert got["sha256"] == want["sha256"]


def _run(recorders, case_id):
    return G.run_case(case_id, lambda k, v: recorders.delenv(k, raising=False) if v is None else recorders.setenv(k, v),
                      setattr_fn=recorders.setattr)


def test_the_cases_take_the_paths_they_are_there_for(recorders):
    """The side lane's launches carry stream 1 and make the main stream wait; the drop-path detour adds its kernels."""
    def launches(case_id):
        """(entry, its last argument: the stream of a launch) of every record but the size and support queries"""
        _run(recorders, case_id)
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


FUSED = ["icamd_bn_apply_conv1x1_fused", "icamd_conv2d_dgrad_bnred", "icamd_conv1x1_bn_bwd_fused"]
THIN = ["icamd_conv3x3_thin_fwd", "icamd_conv3x3_thin_dgrad", "icamd_conv3x3_thin_wgrad"]
# ResNet case -> (entries it must call, entries it must not call)
RESNET_PATHS = {
    "resnet50/routed": (FUSED + ["icamd_bn_bwd_maxpool3x3s2", "icamd_stem7x7s2_fwd", "icamd_stem7x7s2_wgrad"], ["icamd_bn_bwd_dual"]),
    "resnet50/plain_odd_width": (["icamd_bn_bwd_dual", "icamd_conv2d_dgrad_sub2", "icamd_pack_input_rgb4"], FUSED),
    "resnet50/gy_partials": (["icamd_bn_bwd_from_gy_partials", "icamd_conv2d_dgrad_bnred", "icamd_bn_bwd_dual"],
                             ["icamd_conv1x1_bn_bwd_fused"]),
    "resnet50/switches_off": (["icamd_maxpool3x3s2_bwd"], ["icamd_bn_bwd_dual", "icamd_conv2d_dgrad_sub2", "icamd_bn_bwd_maxpool3x3s2"]),
    "resnet50/fused_bnbwd": (["icamd_conv2d_dgrad_bnbwd", "icamd_bn_bwd_from_partials"], []),
    "resnet50/one_stream_unfolded": (["icamd_bn_eval_coeffs"], ["icamd_conv2d_fwd_act", "icamd_bn_fold_filters", "lane.before_write"]),
    "resnet18/basic": (["icamd_bn_bwd_dual", "icamd_conv2d_dgrad_sub2"], []),
    "resnext50_32x4d/routed": (["icamd_gconv3x3_fwd", "icamd_gconv3x3_fwd_act", "icamd_gconv3x3_dgrad", "icamd_gconv3x3_wgrad"], []),
    "seresnet50/routed": (["icamd_se_squeeze", "icamd_se_excite_fwd", "icamd_se_bn_apply", "icamd_se_bn_bwd"],
                          ["icamd_bn_apply_conv1x1_fused"]),
    "resnet50d/thin_default": (["icamd_conv3x3_thin_fwd", "icamd_conv3x3_thin_dgrad", "icamd_avgpool2x2_fwd", "icamd_avgpool2x2_bwd"],
                               ["icamd_conv3x3_thin_wgrad"]),
    "resnet50d/thin_all": (["icamd_conv3x3_thin_wgrad"], []),
    "resnet50d/thin_none_unfolded": (["icamd_avgpool2x2_fwd"], THIN),
    "resnet18d/basic": (["icamd_avgpool2x2_bwd"], []),
    "seresnext26d_32x4d/folded": (["icamd_gconv3x3_fwd_act", "icamd_se_bn_apply"], []),
    "seresnext26d_32x4d/unfolded": (["icamd_se_bn_apply"], ["icamd_gconv3x3_fwd_act"]),
}


@pytest.fixture(scope="module")
def resnet_calls(recorders):
    """ResNet case -> (the entries it calls, the records of its second eval forward, the streams of its launches)"""
    out = {}
    for case_id in RESNET_PATHS:
        _run(recorders, case_id)
        streams = {r[2][-1] for r in G.TRACE if r[0].startswith("icamd_") and not r[0].endswith(("_bytes", "_supported", "_rows"))}
        out[case_id] = ({r[0] for r in G.TRACE}, [r[0] for r in G.phase_records("eval_forward_again")], streams)
    return out


def test_resnet_cases_are_the_listed_ones():
    assert set(RESNET_PATHS) == {c for c in G.CASES if G.MODELS[G.CASES[c].model][0] == "nets"}


@pytest.mark.parametrize("case_id", list(RESNET_PATHS))
def test_the_resnet_cases_take_the_paths_they_are_there_for(resnet_calls, case_id):
    called, again, streams = resnet_calls[case_id]
    must, must_not = RESNET_PATHS[case_id]
    assert [n for n in must if n not in called] == [] and [n for n in must_not if n in called] == []
    # the second eval forward finds the BatchNorm fold done (or, unfolded, never folds), and still runs every layer
    assert "icamd_bn_fold_filters" not in again and "icamd_avgpool_fwd" in again
    if case_id == "resnet50/one_stream_unfolded":
        assert streams == {0}


def test_the_resnet_cases_call_every_entry_nets_names(resnet_calls):
    from imageclassification_amd import hip, nets
    with open(nets.__file__) as f:
        named = {n for n in re.findall(r"\bicamd_\w+", f.read()) if n in hip._SIGNATURES}
    called = set().union(*(c for c, _, _ in resnet_calls.values()))
    assert len(named) > 50 and sorted(named - called) == []


MOBILENET_CASES = ("mobilenetv2_test/default", "mobilenetv2_test/onload")
DW_ENTRIES = ("icamd_dwconv3_fwd", "icamd_dwconv3_wgrad")        # (x, scale, shift, ...): the input and what activates it on load


def test_mobilenet_cases_are_the_listed_ones():
    assert set(MOBILENET_CASES) == {c for c in G.CASES if G.MODELS[G.CASES[c].model][0] == "mobilenet"}


@pytest.mark.parametrize("case_id", MOBILENET_CASES)
def test_the_mobilenet_cases_take_the_paths_they_are_there_for(recorders, case_id):
    """default: icamd_bn_apply_relu6 writes the model's one scratch right in front of every depthwise forward and weight gradient,
    which read it with null scale / shift.  onload: nothing is applied into a scratch, the depthwise entries read the raw tensor with
    the BatchNorm's scale / shift.  One stream either way."""
    seen = []
    G.run_case(case_id, lambda k, v: recorders.delenv(k, raising=False) if v is None else recorders.setenv(k, v),
               setattr_fn=recorders.setattr, observer=lambda model, held, x: seen.append(model))
    ws, depthwise = seen[0]._ws[(G.BATCH, 64, 64)], len(seen[0].blocks)
    launches = [r for r in G.TRACE if r[0].startswith("icamd_") and not r[0].endswith(("_bytes", "_supported", "_rows"))]
    assert {r[2][-1] for r in launches} == {0} and not any(r[0].startswith("lane.") for r in G.TRACE)
    dw = [k for k, r in enumerate(launches) if r[0] in DW_ENTRIES]
    # one depthwise layer per block: one training and one eval forward, two backward passes
    assert depthwise == 6 and [launches[k][0] for k in dw].count("icamd_dwconv3_fwd") == 2 * depthwise and len(dw) == 4 * depthwise
    applies = [r for r in launches if r[0] == "icamd_bn_apply_relu6"]
    if case_id.endswith("/default"):
        a1 = ws["a1"].data_ptr()
        for k in dw:
            before, (x, scale, shift) = launches[k - 1], launches[k][2][:3]
            assert before[0] == "icamd_bn_apply_relu6" and before[2][3] == a1
            assert x == a1 and scale is None and shift is None
        assert sum(r[2][3] == a1 for r in applies) == len(dw)
    else:
        assert "a1" not in ws
        inputs = {launches[k][2][0] for k in dw}
        assert not any(r[2][3] in inputs for r in applies)
        stored = {t.data_ptr() for b in ws["blocks"] for t in (b["a2"],)} | {ws["ah"].data_ptr()}
        assert {r[2][3] for r in applies} == stored          # every apply left is one whose output the step stores
        assert all(launches[k][2][1] and launches[k][2][2] for k in dw)


EFFICIENTNET_CASES = ("efficientnet_test/default", "efficientnet_b1/ds_skip")
SE_SILU_ENTRIES = {"forward": ("icamd_bn_silu_squeeze", "icamd_se_excite_silu_fwd"),
                   "backward": ("icamd_se_silu_bwd_reduce", "icamd_se_excite_silu_bwd")}


def test_efficientnet_cases_are_the_listed_ones():
    assert set(EFFICIENTNET_CASES) == {c for c in G.CASES if G.MODELS[G.CASES[c].model][0] == "efficientnet"}


@pytest.mark.parametrize("case_id", EFFICIENTNET_CASES)
def test_the_efficientnet_cases_take_the_paths_they_are_there_for(recorders, case_id):
    """One stream.  The squeeze and the excitation run once per block in each of the two forwards, the gate-gradient reduce and the
    excitation backward once per block in each of the two backwards; nothing is activated by ReLU6.  efficientnet_test has depthwise
    layers of both filter sizes.  efficientnet_b1's blocks.0.1 is a depthwise-separable block with a skip: each backward adds its
    data gradient to the skip's with the one icamd_bn_apply a backward makes, the only one whose addend is not NULL."""
    seen = []
    G.run_case(case_id, lambda k, v: recorders.delenv(k, raising=False) if v is None else recorders.setenv(k, v),
               setattr_fn=recorders.setattr, observer=lambda model, held, x: seen.append(model))
    blocks = len(seen[0].blocks)
    launches = [r for r in G.TRACE if r[0].startswith("icamd_") and not r[0].endswith(("_bytes", "_supported", "_rows"))]
    assert {r[2][-1] for r in launches} == {0} and not any(r[0].startswith("lane.") for r in G.TRACE)
    names = [r[0] for r in launches]
    assert "icamd_bn_apply_relu6" not in names and "icamd_bn_bwd_relu6" not in names
    for phases, entries in ((("forward", "eval_forward"), SE_SILU_ENTRIES["forward"]),
                            (("backward", "backward_accumulate"), SE_SILU_ENTRIES["backward"])):
        for entry in entries:
            assert names.count(entry) == 2 * blocks
            assert all([r[0] for r in G.phase_records(ph)].count(entry) == blocks for ph in phases)
    skips = [[r for r in G.phase_records(ph) if r[0] == "icamd_bn_apply"] for ph in ("backward", "backward_accumulate")]
    if case_id == "efficientnet_test/default":
        assert blocks == 6 and skips == [[], []]
        for op in ("fwd", "dgrad", "wgrad"):
            assert names.count(f"icamd_dwconv3_{op}") > 0 and names.count(f"icamd_dwconv5_{op}") > 0
            assert names.count(f"icamd_dwconv3_{op}") + names.count(f"icamd_dwconv5_{op}") == 2 * blocks
    else:
        assert blocks == 23 and seen[0].blocks[1].kind == "ds" and seen[0].blocks[1].residual
        assert [len(s) for s in skips] == [1, 1] and all(s[0][2][3] is not None for s in skips)      # (y, scale, shift, addend, ...)
        # the forward's applies: one per block, the addend there exactly for the blocks with a skip
        fwd = [r[2][3] is not None for r in G.phase_records("forward") if r[0] == "icamd_bn_apply"]
        assert fwd == [b.residual for b in seen[0].blocks]


FOLDED = ["icamd_layerscale_fold", "icamd_layerscale_param_grads", "icamd_conv2d_dgrad_gelu"]
UNFOLDED = ["icamd_layerscale_fwd", "icamd_layerscale_bwd", "icamd_dwconv7_wgrad", "icamd_colsum_rows", "icamd_conv2d_dgrad_gelu"]
V2 = ["icamd_grn_fwd", "icamd_grn_bwd", "icamd_conv2d_dgrad"]
NOT_V2 = ["icamd_layerscale_fold", "icamd_layerscale_param_grads", "icamd_rows_fix", "icamd_dropped_colsum", "icamd_conv2d_dgrad_gelu"]
# ConvNeXt case -> (entries it must call, entries it must not call)
CONVNEXT_PATHS = {
    "convnext_test/lane_on": (FOLDED + ["icamd_dwconv7_wgrad", "icamd_colsum_rows", "icamd_rows_fix", "icamd_dropped_colsum"],
                              ["icamd_dwconv7_wgrad_bias", "icamd_layerscale_fwd", "icamd_layerscale_bwd", "icamd_grn_fwd"]),
    "convnext_test/lane_off": (FOLDED + ["icamd_dwconv7_wgrad", "icamd_colsum_rows"], ["icamd_dwconv7_wgrad_bias", "lane.before_write"]),
    "convnext_test/routed": (FOLDED + ["icamd_dwconv7_wgrad_bias", "icamd_dropped_colsum", "icamd_rows_fix", "lane.before_write"],
                             ["icamd_dwconv7_wgrad", "icamd_colsum_rows", "icamd_layerscale_fwd", "icamd_layerscale_bwd", "icamd_grn_fwd"]),
    "convnext_test/routed_no_drop": (FOLDED + ["icamd_dwconv7_wgrad_bias"],
                                     ["icamd_rows_fix", "icamd_dropped_colsum", "icamd_dwconv7_wgrad", "icamd_colsum_rows"]),
    "convnext_test/unfolded": (UNFOLDED + ["lane.before_write"],
                               ["icamd_dwconv7_wgrad_bias", "icamd_layerscale_fold", "icamd_layerscale_param_grads", "icamd_rows_fix",
                                "icamd_dropped_colsum"]),
    "convnext_test/unfolded_lane_off": (UNFOLDED, ["icamd_dwconv7_wgrad_bias", "icamd_layerscale_fold", "lane.before_write"]),
    "convnextv2_test/drop": (V2 + ["icamd_dwconv7_wgrad_bias", "icamd_layerscale_fwd", "icamd_layerscale_bwd", "lane.before_write"],
                             NOT_V2 + ["icamd_dwconv7_wgrad", "icamd_colsum_rows"]),
    "convnextv2_test/no_drop_lane_off": (V2 + ["icamd_dwconv7_wgrad", "icamd_colsum_rows"],
                                         NOT_V2 + ["icamd_dwconv7_wgrad_bias", "icamd_layerscale_fwd", "icamd_layerscale_bwd",
                                                   "lane.before_write"]),
}
HEAD_DESC = (G.BATCH, 1, 1, 192, 1, 1, 64, 1, 1, 1, 0)     # head.fc of both test models: 192 features, 10 classes padded to 64


@pytest.fixture(scope="module")
def convnext_calls(recorders):
    """ConvNeXt case -> (the entries it calls, the streams of its launches, {phase: its records})"""
    out = {}
    for case_id in CONVNEXT_PATHS:
        _run(recorders, case_id)
        streams = {r[2][-1] for r in G.TRACE if r[0].startswith("icamd_") and not r[0].endswith(("_bytes", "_supported"))}
        phases = {n: G.phase_records(n) for n, _ in G.PHASES if n.startswith("backward")}
        out[case_id] = ({r[0] for r in G.TRACE}, streams, phases)
    return out


def test_convnext_cases_are_the_listed_ones():
    assert set(CONVNEXT_PATHS) == {c for c in G.CASES if G.MODELS[G.CASES[c].model][0] == "convnext"}


@pytest.mark.parametrize("case_id", list(CONVNEXT_PATHS))
def test_the_convnext_cases_take_the_paths_they_are_there_for(convnext_calls, case_id):
    called, streams, _ = convnext_calls[case_id]
    must, must_not = CONVNEXT_PATHS[case_id]
    assert [n for n in must if n not in called] == [] and [n for n in must_not if n in called] == []
    assert streams == ({0} if case_id.endswith("lane_off") else {0, 1})


def test_the_convnext_cases_call_every_entry_convnext_names(convnext_calls):
    from imageclassification_amd import convnext, hip
    with open(convnext.__file__) as f:
        named = {n for n in re.findall(r"\bicamd_\w+", f.read()) if n in hip._SIGNATURES or n in hip._SIGNATURES_ADDED}
    called = set().union(*(c for c, _, _ in convnext_calls.values()))
    assert len(named) >= 20 and sorted(named - called) == []


@pytest.mark.parametrize("case_id", [c for c in CONVNEXT_PATHS if G.CASES[c].dfeat])
def test_a_backward_from_dfeat_skips_the_head_only(convnext_calls, case_id):
    """No pooling backward and no weight gradient of head.fc; every block's depthwise data gradient, as in the backward from the
    logits."""
    _, _, phases = convnext_calls[case_id]
    full, dfeat = phases["backward"], phases["backward_dfeat"]

    def names(records):
        return [r[0] for r in records]

    def wgrad_descs(records):
        return [r[2][0] for r in records if r[0] == "icamd_conv2d_wgrad_bias"]

    assert "icamd_avgpool_bwd" in names(full) and "icamd_avgpool_bwd" not in names(dfeat)
    assert wgrad_descs(full)[0] == HEAD_DESC and HEAD_DESC not in wgrad_descs(dfeat)
    assert wgrad_descs(dfeat) == wgrad_descs(full)[1:]
    dw = [r[2][4:8] for r in dfeat if r[0] == "icamd_dwconv7_dgrad"]          # (N, h, w, dim) of each, last block first
    assert dw == [(G.BATCH, 2, 2, 192), (G.BATCH, 4, 4, 128), (G.BATCH, 4, 4, 128), (G.BATCH, 8, 8, 64), (G.BATCH, 16, 16, 32)]
    assert dw == [r[2][4:8] for r in full if r[0] == "icamd_dwconv7_dgrad"]
    assert names(dfeat)[-1] == "hook" and names(dfeat).count("lane.join") == 1


@pytest.mark.parametrize("model_id", list(G.STATE_MODELS))
def test_seed_0_gives_the_recorded_weights(recorders, model_id):
    """Names and shapes exactly; sums and sampled elements to the generator's state_tol (last-bit differences between CPUs)."""
    model = G.build_model(model_id)
    got, want = G.state_record(model), FIXTURE["state_dict_seed0"][model_id]
    assert got["names_and_shapes_sha256"] == want["names_and_shapes_sha256"]
    assert len(got["values"]) == len(want["values"]) == len(model.state_dict()) >= len(model.params)
    worst = [0.0, 0.0]
    for (name, t), g, w in zip(model.state_dict().items(), got["values"], want["values"]):
        bound = G.STATE_BOUND.get(model_id, 0.25)
        assert float(t.abs().max()) < bound or bool((t == 1).all()), name          # what state_tol assumes
        tol_sum, tol_el = G.state_tol(t.numel(), bound)
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
