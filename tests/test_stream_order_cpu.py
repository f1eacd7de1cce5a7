"""The weight-gradient side stream of every backward pass is ordered against the main stream, proved from the call trace without a
GPU (tests/_stream_order.py states the access model, the extents and how happens-before is derived from the real streams.SideLane):

  - per case of the call-trace generator: no two launches on different streams touch overlapping bytes, one of
    them writing, without a happens-before path (`hazards`); the main stream has waited for every side launch when a backward ends
    (`unjoined`); after grad_ready_hook(lo, hi, events) nothing writes a gradient at or above `lo`, and every side-stream write
    there is covered by the main stream or by `events` (`late_writes`);
  - the checker reports each of these when the lane's bookkeeping is broken on purpose (monkeypatched, undone after the test),
    down to one `writes(p)` written as `p` at each of its call sites in turn; the three checks come first in the per-case test, so
    such a change is named by its launches and its buffer even where it also moves the recorded trace (compared in a test of its own);
  - hand-written traces of a few records pin what counts as a conflict and as an ordering.

MobileNetV2 (`mobilenetv2_test`, two cases of the generator's table) and EfficientNet (`efficientnet_test`, `efficientnet_b1`, one
case each) have no side lane, so their hazards and unjoined launches are empty by construction and the hook check is the one that
bears on them.
"""
import json
import os

import pytest

import _stream_order as S
from imageclassification_amd import hip

G = S.G
with open(os.path.join(S.HERE, "golden", "call_traces.json")) as f:
    FIXTURE = json.load(f)

# the cases whose backward stays on one stream: the lane's switch is off, the model has no lane, or the route keeps it off
LANE_OFF = {"vit_tiny_test/lane_off", "swin_test/no_drop", "swin_test/drop", "swin_test_w12/no_drop", "swin_test_w12/drop",
            "convnext_test/lane_off", "convnext_test/unfolded_lane_off", "convnextv2_test/no_drop_lane_off", "resnet50/fused_bnbwd",
            "resnet50/one_stream_unfolded", "mobilenetv2_test/default", "mobilenetv2_test/onload", "efficientnet_test/default",
            "efficientnet_b1/ds_skip"}
CASE_IDS = list(G.CASES)
LANE_ON = [c for c in CASE_IDS if c not in LANE_OFF]
MOBILENET = "mobilenetv2_test/default"
EFFICIENTNET = "efficientnet_test/default"
ONE_STREAM_MBCONV = (MOBILENET, EFFICIENTNET, "efficientnet_b1/ds_skip")


@pytest.fixture(scope="module")
def recorders():
    mp = pytest.MonkeyPatch()
    S.install(mp.setattr)
    yield mp
    mp.undo()


def _observe(mp, case_id):
    return S.observe(case_id, lambda k, v: mp.delenv(k, raising=False) if v is None else mp.setenv(k, v), setattr_fn=mp.setattr)


@pytest.fixture(scope="module")
def runs(recorders):
    """case -> its Run at HEAD, made on first use and shared"""
    class Runs(dict):
        def __missing__(self, case_id):
            self[case_id] = _observe(recorders, case_id)
            return self[case_id]
    return Runs()


# ------------------------------------------------------------------------------------------------------------------ access model
def test_every_exported_entry_is_parsed_from_the_header():
    assert [n for n in hip.EXPORTED_SYMBOLS if n not in S.DECLS] == []
    for name in hip.EXPORTED_SYMBOLS:
        argtypes = (hip._SIGNATURES.get(name) or hip._SIGNATURES_ADDED[name])[1]
        decl = S.DECLS[name]
        assert len(decl.args) == len(argtypes), name
        for a, t in zip(decl.args, argtypes):
            assert a.pointer == (t is hip.c_void_p or hasattr(t, "contents")), (name, a.name)
        assert all(a.pointer for a in decl.args if a.const), name
        assert decl.stream == (bool(decl.args) and decl.args[-1].name == "stream"), name


def test_roles_of_a_few_arguments():
    d = S.DECLS["icamd_conv2d_wgrad_bias"]
    assert [(a.name, a.pointer, a.const) for a in d.args] == [
        ("d", True, True), ("x", True, True), ("dy", True, True), ("dw", True, False), ("dbias", True, False), ("accumulate", False, False),
        ("workspace", True, False), ("workspace_bytes", False, False), ("stream", True, False)]
    assert d.stream and not S.DECLS["icamd_conv2d_wgrad_workspace_bytes"].stream and not S.DECLS["icamd_abi_version"].args
    assert [(f.name, f.pointer, f.const) for f in S.FUSE_FIELDS] == [
        ("y", True, True), ("mask_src", True, True), ("mean", True, True), ("invstd", True, True), ("scale", True, True),
        ("shift", True, True), ("partials", True, False), ("relu", False, False)]
    assert [n for n, _ in hip.BnBwdFuse._fields_] == [f.name for f in S.FUSE_FIELDS]
    assert all(e in S.DECLS and a in [x.name for x in S.DECLS[e].args] for e, a in list(S.EXACT) + list(S.WHOLE))


def test_extents_follow_the_tables(runs):
    run = runs["resnet50/routed"]
    m = run.model
    base = {a: getattr(m, a).untyped_storage().data_ptr() for a in ("param_arena", "grad_arena", "shadow", "shadow_t", "buffer_arena")}
    spans = {(p.offset, p.offset + p.numel) for p in m.params.values()}
    seen = {k: set() for k in base}
    for a in run.accesses:
        for k, b in base.items():
            if a.base == b:
                seen[k].add((a.entry, a.arg, a.start, a.end))
    for k, width in (("param_arena", 4), ("grad_arena", 4), ("shadow", 2)):
        whole = {s for s in seen[k] if (s[0], s[1]) in S.EXACT or (s[0], s[1]) in S.WHOLE}
        assert seen[k] - whole and all((lo // width, hi // width) in spans for _, _, lo, hi in seen[k] - whole), k
    assert ("icamd_f32_to_bf16", "src", 0, 4 * m.n_params) in seen["param_arena"]
    assert ("icamd_f32_to_bf16", "dst", 0, 2 * m.n_params) in seen["shadow"]
    assert ("icamd_filter_transpose_tiled", "dst_base", 0, 2 * m.shadow_t.numel()) in seen["shadow_t"]
    # every BatchNorm's gradient pair is written, each as its own parameter; every transposed filter is read as its table entry
    assert {(lo // 4, hi // 4) for e, _, lo, hi in seen["grad_arena"]} == spans
    entries = {(d[1], d[1] + d[2] * d[3] * d[4]) for d in m._tr_descs.tolist()}
    assert {(lo // 2, hi // 2) for e, a, lo, hi in seen["shadow_t"] if a == "w_t"} == entries and len(entries) == 53
    # running statistics: 2 c floats per BatchNorm, 53 of them
    stats = {(lo, hi) for _, _, lo, hi in seen["buffer_arena"]}
    assert len(stats) == 53 and len(run.arenas[base["buffer_arena"]][1]) == 53
    # any other tensor: from the pointer to the end of its storage
    gbuf = m._ws[next(iter(m._ws))]["gbuf"][0]
    ends = {a.end for a in run.accesses if a.base == gbuf.untyped_storage().data_ptr()}
    assert ends == {gbuf.untyped_storage().nbytes()}
    assert run.describe(gbuf.untyped_storage().data_ptr(), 0).endswith("['gbuf'][0] + 0")
    assert run.describe(base["grad_arena"], 4 * m.params["fc.bias"].offset) == "grad_arena[fc.bias]"


# ------------------------------------------------------------------------------------------------------------------ HEAD
def _told(found):
    return "".join(f"\n  {a[0]}({a[1]}) on stream {a[2]} at TRACE[{a[3]}]  /  {b[0]}({b[1]}) on stream {b[2]} at TRACE[{b[3]}]  in  {buffer}"
                   for a, b, buffer in found)


def _assert_ordered(run):
    """The three checks of one case, first of all: a change of the model code that breaks the ordering is named by its two launches
    and the buffer, whatever else it does to the trace.  -> the number of conflicting pairs examined"""
    counts = {}
    found = S.hazards(run, counts)
    assert not found, f"{run.case_id}: {len(found)} unordered conflicting pairs:" + _told(found)
    left = S.unjoined(run)
    assert not left, f"{run.case_id}: side launches the main stream never waited for (phase, entry, TRACE index): {left}"
    late = S.late_writes(run)
    assert not late, f"{run.case_id}: gradient writes a hook does not cover (phase, hook, lo, launch, buffer): {late}"
    return counts["pairs"]


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_the_backward_is_ordered(runs, case_id):
    run = runs[case_id]
    pairs = _assert_ordered(run)
    counts = {"pairs": pairs}
    side = run.side_launches()
    print(f"{case_id}: {len(side)} side launches, {pairs} conflicting pairs examined, {len(S.hooks(run))} hooks")
    assert [n for n, _, _ in run.backward] == [n for n in S.BACKWARD_PHASES if n != "backward_dfeat" or G.CASES[case_id].dfeat]
    assert sorted(side) == sorted(run.side_launches_anywhere())    # no other phase uses the second stream
    if case_id in LANE_ON:
        assert len(side) > 0 and counts["pairs"] > 0
        assert any(k == "wait" and s == S.MAIN for k, _, _, s in (e for e in run.log if e[0] != "events"))
    else:
        assert side == [] and counts["pairs"] == 0 and [e for e in run.log if e[0] != "events"] == []
    assert len(S.hooks(run)) >= 3 * len(run.backward)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_observing_leaves_the_trace_as_recorded(runs, case_id):
    """The real lane, the stand-ins and the observer beside it: TRACE, the number of calls and of stream queries are the fixture's."""
    assert runs[case_id].result == FIXTURE["cases"][case_id]


def test_nineteen_cases_run_the_lane():
    assert len(LANE_ON) == 19 and LANE_OFF < set(CASE_IDS) and len(CASE_IDS) == 33 and CASE_IDS == list(FIXTURE["cases"])


@pytest.mark.parametrize("case_id", ONE_STREAM_MBCONV)
def test_mobilenetv2_is_ordered(runs, case_id):
    run = runs[case_id]
    assert [n for n, _, _ in run.backward] == ["backward", "backward_accumulate"]
    writes = [a for a in run.accesses if a.base == run.grad_base and a.write and any(lo <= a.index < hi for _, lo, hi in run.backward)]
    written = {run.describe(a.base, a.start) for a in writes}
    assert written == {f"grad_arena[{n}]" for n in run.model.params}       # the trace sees every parameter's gradient
    assert S.hazards(run) == [] and S.unjoined(run) == [] and S.late_writes(run) == []
    assert run.side_launches_anywhere() == [] and len(S.hooks(run)) == 2 * (len(run.model.blocks) + 2)


# ------------------------------------------------------------------------------------------------------------------ broken on purpose
def _drop_reads(mp):
    launch = S.RealSideLane.launch
    mp.setattr(S.RealSideLane, "launch", lambda self, fn, reads=(): launch(self, fn, ()))


@pytest.mark.parametrize("case_id", LANE_ON)
def test_a_launch_that_forgets_its_reads_is_reported(recorders, runs, monkeypatch, case_id):
    _drop_reads(monkeypatch)
    run = _observe(recorders, case_id)
    found = S.hazards(run)
    assert found and run.result == runs[case_id].result            # TRACE does not depend on the real lane
    for a, b, buffer in found:                                     # the side launch still reads what the main stream overwrites
        side, main = (a, b) if a[2] != S.MAIN else (b, a)
        assert side[2] == S.SIDE and main[2] == S.MAIN and main[3] > side[3] and isinstance(buffer, str)
    assert S.unjoined(run) == []


@pytest.mark.parametrize("case_id", LANE_ON)
def test_a_before_write_that_does_not_wait_is_reported(recorders, runs, monkeypatch, case_id):
    assert any(r[0] == "lane.before_write" for r in runs[case_id].trace)       # every lane-on case meets a pending read
    monkeypatch.setattr(S.RealSideLane, "before_write", lambda self, *ptrs: None)
    assert S.hazards(_observe(recorders, case_id))


def _names_two_launches_and_a_buffer(found):
    for a, b, buffer in found:
        assert {a[2], b[2]} == {S.MAIN, S.SIDE} and a[0] in S.DECLS and b[0] in S.DECLS and a[3] != b[3]
        assert any(x.name == a[1].split(".")[0] for x in S.DECLS[a[0]].args) and buffer.startswith("model.")
    return len(found)


@pytest.mark.parametrize("case_id", [c for c in LANE_ON if G.MODELS[G.CASES[c].model][0] == "nets"])
def test_a_resnet_weight_gradient_launched_without_reads_is_reported(recorders, monkeypatch, case_id):
    """nets._side_wgrad with its `reads=(dy,)` left out: the output-gradient pool rotates under the pending weight gradients"""
    from imageclassification_amd import nets
    monkeypatch.setattr(nets.ResNet, "_side_wgrad", lambda self, run, conv, d, x, dy: run.lane.launch(
        lambda st: self._wgrad(conv, d, x, dy, run.acc, run.wsp, run.wsb, st)))
    run = _observe(recorders, case_id)
    with pytest.raises(AssertionError, match="unordered conflicting pairs"):
        _assert_ordered(run)
    found = S.hazards(run)
    assert _names_two_launches_and_a_buffer(found) > 0
    assert all("gbuf" in buffer for _, _, buffer in found)


def _writes_sites(module, function):
    """The source lines of `function` (a method of blocks.Backward or convnext.ConvNeXt) that call writes()"""
    import inspect
    lines, first = inspect.getsourcelines(function)
    return [first + k for k, text in enumerate(lines) if ".writes(" in text]


# One `writes(p)` written as `p`: (module, class, method, which of the method's writes() calls) -> the case that runs it with a read
# pending, or None where no side launch reads that buffer at that point (the wait is there for safety and its loss changes nothing)
WRITES_SITES = {
    ("blocks", "Backward", "gemm", 0): "convnext_test/unfolded",             # the plain data gradient's dx (d z2 -> G[1] read by fc2)
    ("blocks", "Backward", "gemm", 1): "vit_tiny_test/lane_on",              # dz of the data gradient with GELU's backward
    ("blocks", "Backward", "layernorm", 0): "vit_tiny_test/lane_on",
    ("blocks", "Backward", "drop_path", 0): "convnextv2_test/drop",
    ("blocks", "Backward", "block", 0): "vit_tiny_test/lane_on",             # d(qkv) of the attention's backward
    ("convnext", "ConvNeXt", "_v2_bwd", 0): "convnextv2_test/drop",
    ("convnext", "ConvNeXt", "_folded_bwd", 0): "convnext_test/routed",
    ("convnext", "ConvNeXt", "_dw_bwd", 0): "convnext_test/routed",
    ("convnext", "ConvNeXt", "_head_bwd", 0): None,
    ("convnext", "ConvNeXt", "_unfolded_bwd", 0): None,
}


def test_the_sites_are_all_of_them():
    import importlib
    import re
    for module in ("blocks", "convnext", "vit"):
        mod = importlib.import_module("imageclassification_amd." + module)
        with open(mod.__file__) as f:
            calls = len(re.findall(r"\.writes\(", f.read()))
        assert calls == sum(1 for m, *_ in WRITES_SITES if m == module), module


@pytest.mark.parametrize("site", list(WRITES_SITES), ids=lambda s: f"{s[0]}.{s[2]}.{s[3]}")
def test_one_writes_written_as_a_bare_pointer(recorders, runs, monkeypatch, site):
    """Exactly one call of Backward.writes hands its pointer on without waiting; every other one waits as before.  The per-case check
    then fails and names the main-stream launch that overwrites, the side launch that still reads, and the buffer."""
    import importlib
    import sys
    from imageclassification_amd import blocks
    module, cls, method, which = site
    expected = WRITES_SITES[site]
    unbroken = runs[expected] if expected else None       # made (on first use) before anything is broken
    function = getattr(getattr(importlib.import_module("imageclassification_amd." + module), cls), method)
    where = (function.__code__.co_name, _writes_sites(module, function)[which])
    writes, bare = blocks.Backward.writes, []

    def one_bare(self, ptr):
        frame = sys._getframe(1)
        if (frame.f_code.co_name, frame.f_lineno) == where:
            bare.append(ptr)
            return ptr
        return writes(self, ptr)
    monkeypatch.setattr(blocks.Backward, "writes", one_bare)
    if expected is None:
        for case_id in [c for c in LANE_ON if G.CASES[c].model.startswith("convnext")]:
            _assert_ordered(_observe(recorders, case_id))
        assert bare                                  # the site ran, and no read of its buffer was pending
        return
    run = _observe(recorders, expected)
    assert bare
    with pytest.raises(AssertionError, match="unordered conflicting pairs") as failure:
        _assert_ordered(run)
    found = S.hazards(run)
    assert _names_two_launches_and_a_buffer(found) > 0
    for a, b, buffer in found:
        assert f"{a[0]}({a[1]}) on stream {a[2]} at TRACE[{a[3]}]" in str(failure.value) and buffer in str(failure.value)
        main, side = (a, b) if a[2] == S.MAIN else (b, a)
        assert S.DECLS[main[0]].args[[x.name for x in S.DECLS[main[0]].args].index(main[1])].const is False      # the main stream writes
    assert S.hazards(unbroken) == []


@pytest.mark.parametrize("case_id", [c for c in LANE_ON if G.MODELS[G.CASES[c].model][0] == "nets"])
def test_a_resnet_pool_buffer_taken_without_waiting_is_reported(recorders, monkeypatch, case_id):
    """nets._next_y without its before_write"""
    from imageclassification_amd import nets
    monkeypatch.setattr(nets.ResNet, "_next_y", lambda self, run: next(run.ypool))
    run = _observe(recorders, case_id)
    with pytest.raises(AssertionError, match="unordered conflicting pairs"):
        _assert_ordered(run)
    assert _names_two_launches_and_a_buffer(S.hazards(run)) > 0


@pytest.mark.parametrize("case_id", LANE_ON)
def test_a_join_that_does_not_wait_is_reported(recorders, monkeypatch, case_id):
    monkeypatch.setattr(S.RealSideLane, "join", lambda self: None)
    run = _observe(recorders, case_id)
    left = S.unjoined(run)
    assert left and {p for p, _, _ in left} == {n for n, _, _ in run.backward}
    assert S.hazards(run)          # the next pass's main stream then overwrites what the last side launches still read


@pytest.mark.parametrize("case_id", LANE_ON)
def test_a_hook_without_the_lanes_events_is_reported(recorders, monkeypatch, case_id):
    monkeypatch.setattr(S.RealSideLane, "events", lambda self: ())
    late = S.late_writes(_observe(recorders, case_id))
    assert late and all(w[2] == S.SIDE for _, _, _, w, _ in late)


@pytest.mark.parametrize("case_id, module, cls", [("convnext_test/routed", "convnext", "ConvNeXt"), ("resnet50/routed", "nets", "ResNet"),
                                                  (MOBILENET, "mobilenet", "MobileNetV2"),
                                                  (EFFICIENTNET, "efficientnet", "EfficientNet")])
def test_a_hook_called_one_block_early_is_reported(recorders, runs, monkeypatch, case_id, module, cls):
    """Every hook announces the range the NEXT hook of the unbroken pass announces: the block in between has not run yet."""
    import importlib
    los = sorted({lo for _, _, lo, _ in S.hooks(runs[case_id])})
    earlier = {lo: los[max(k - 1, 0)] for k, lo in enumerate(los)}
    model_cls = getattr(importlib.import_module("imageclassification_amd." + module), cls)
    backward = model_cls.backward_packed

    def early(self, *a, **k):
        hook = self.grad_ready_hook
        self.grad_ready_hook = lambda lo, hi=None, events=(): hook(earlier[lo], hi, events)
        try:
            return backward(self, *a, **k)
        finally:
            self.grad_ready_hook = hook
    monkeypatch.setattr(model_cls, "backward_packed", early)
    run = _observe(recorders, case_id)
    late = S.late_writes(run)
    assert late and any(w[3] > i for _, i, _, w, _ in late)
    assert S.hazards(run) == []


# ------------------------------------------------------------------------------------------------------------------ by hand
BUFFERS = {"X": 1024, "Y": 1024, "Z": 1024}


def _gelu(src, dst, stream):
    """icamd_gelu_fwd(const void* z, void* a, ...): reads `src`, writes `dst` (each a (buffer, byte offset))"""
    return ("icamd_gelu_fwd", {"z": src, "a": dst}, stream)


def _pair(records, log):
    run = S.from_records(records, log, BUFFERS)
    counts = {}
    return S.hazards(run, counts), counts["pairs"]


def test_read_after_write():
    records = [_gelu(("Y", 0), ("X", 0), 0), _gelu(("X", 0), ("Z", 0), 1)]
    found, pairs = _pair(records, [])
    assert pairs == 1 and found == [(("icamd_gelu_fwd", "a", 0, 0), ("icamd_gelu_fwd", "z", 1, 1), "X + 0")]
    assert _pair(records, [("record", 1, 7, 0), ("wait", 1, 7, 1)]) == ([], 1)
    assert len(_pair(records, [("record", 0, 7, 0), ("wait", 1, 7, 1)])[0]) == 1        # recorded before the write was enqueued


def test_write_after_read():
    records = [_gelu(("X", 0), ("Z", 0), 1), _gelu(("Y", 0), ("X", 0), 0)]
    found, pairs = _pair(records, [])
    assert pairs == 1 and found == [(("icamd_gelu_fwd", "a", 0, 1), ("icamd_gelu_fwd", "z", 1, 0), "X + 0")]
    assert _pair(records, [("record", 1, 7, 1), ("wait", 1, 7, 0)]) == ([], 1)
    assert len(_pair(records, [("record", 1, 7, 1), ("wait", 2, 7, 0)])[0]) == 1        # the wait comes after the write


def test_write_after_write():
    records = [_gelu(("Y", 0), ("X", 0), 0), _gelu(("Z", 0), ("X", 512), 1)]
    found, pairs = _pair(records, [])
    # the first write runs to the end of X (conservative), so it covers the second one's half
    assert pairs == 1 and found == [(("icamd_gelu_fwd", "a", 0, 0), ("icamd_gelu_fwd", "a", 1, 1), "X + 512")]
    assert _pair(records, [("record", 1, 7, 0), ("wait", 1, 7, 1)]) == ([], 1)


def test_a_chain_of_two_events_orders():
    """Stream 0 writes X, stream 2 waits for it and writes Z, stream 1 waits for stream 2 and reads X: ordered through both events."""
    records = [_gelu(("Y", 0), ("X", 0), 0), _gelu(("Y", 0), ("Z", 0), 2), _gelu(("X", 0), ("Z", 512), 1)]
    chain = [("record", 1, 7, 0), ("wait", 1, 7, 2), ("record", 2, 8, 2), ("wait", 2, 8, 1)]
    assert _pair(records, chain) == ([], 2)                       # the pair on X, and streams 2 and 1 on Z
    found, pairs = _pair(records, chain[:1] + chain[2:])          # stream 2 never waited for stream 0
    assert pairs == 2 and [(a[3], b[3]) for a, b, _ in found] == [(0, 2)]
    found, pairs = _pair(records, chain[:3])                      # stream 1 never waited for stream 2
    assert pairs == 2 and sorted((a[3], b[3]) for a, b, _ in found) == [(0, 2), (2, 1)]


def test_two_reads_are_no_conflict():
    assert _pair([_gelu(("X", 0), ("Y", 0), 0), _gelu(("X", 0), ("Z", 0), 1)], []) == ([], 0)


def test_same_stream_needs_no_event():
    assert _pair([_gelu(("Y", 0), ("X", 0), 1), _gelu(("X", 0), ("Z", 0), 1)], []) == ([], 0)


def test_a_wait_for_an_unrecorded_event_is_an_error():
    with pytest.raises(KeyError):
        S.from_records([_gelu(("Y", 0), ("X", 0), 0)], [("wait", 0, 7, 1)], BUFFERS)
