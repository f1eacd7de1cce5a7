"""Generates tests/golden/call_traces.json: one SHA-256 per case over every library call a ViT, Swin, ConvNeXt, ResNet, MobileNetV2 or
EfficientNet step makes.

Run at the commit whose launches are to be pinned (no GPU needed):
    python tests/golden/make_call_traces.py
To see what moved when the test fails, write the records themselves at both commits and compare them (the fixture is untouched):
    python tests/golden/make_call_traces.py --dump DIR

The models run on the CPU under make_arena_layouts.install_stubs plus three more replacements (`install_recorders`): the library
records (entry, arguments) and returns 0 (a ResNet, MobileNetV2, EfficientNet or routed ConvNeXt case carries a table of other answers for the queries, `Case.answers`),
torch.cuda.current_stream is a stand-in whose stream is 0, and streams.SideLane is a
lane of the same interface that runs a launch with stream 1 when it is enabled (0 otherwise) and leaves a record for every
before_write that meets a pending read and for every join.  grad_ready_hook records (lo, hi, events).  A case is: construct at
seed 0, train(), pack, forward_packed, backward_packed, backward_packed(accumulate=True), eval(), forward_packed(logits_only=True)
(a ResNet case: twice, the second one with the BatchNorm fold already done), load_state_dict(state_dict()); a case with `dfeat`
(the ConvNeXt ones added with the block walk) also runs backward_packed(dfeat=zeros) after the accumulating backward.  PHASES keeps where each
phase starts in TRACE.

Arguments are written by their type in hip._SIGNATURES / _SIGNATURES_ADDED: a descriptor as its key(), a float as its repr, the last pointer as the
stream id, any other pointer as [number of its buffer in order of first use, byte offset, bytes of the buffer] -- looked up
among all tensors reachable from the model (collected after every phase and kept alive, so that an address is never used twice),
"input" for the image batch, None for NULL; a byref(BnBwdFuse) as the list of its fields, pointers in the same form.  No attribute or dictionary name enters the record; a pointer into no buffer is an
error.  Besides the trace the file keeps, per case, the number of stream queries (hip.stream_ptr, torch.cuda.current_stream) and,
per model, what state_dict() holds at seed 0 (`state_record`).  tests/test_call_trace_cpu.py reruns every case and compares.
"""
import bisect
import collections
import ctypes
import hashlib
import importlib
import importlib.util
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_arena_layouts", os.path.join(HERE, "make_arena_layouts.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)

BATCH = 2
DROP_PATH = 0.2
VIT_ENV, CNX_ENV = "ICAMD_WGRAD_STREAM_VIT", "ICAMD_WGRAD_STREAM"
# model id -> (module, class, constructor arguments, input size)
MODELS = {
    "vit_tiny_test": ("vit", "VisionTransformer", {"arch": "vit_tiny_test"}, 224),
    "swin_test": ("swin", "SwinTransformer", {"arch": "swin_test", "img_size": 56}, 56),
    "swin_test_w12": ("swin", "SwinTransformer", {"arch": "swin_test_w12", "img_size": 96}, 96),
    "convnext_test": ("convnext", "ConvNeXt", {"arch": "convnext_test"}, 64),
    "convnextv2_test": ("convnext", "ConvNeXt", {"arch": "convnextv2_test"}, 64),
}
RESNETS = ("resnet50", "resnet18", "resnext50_32x4d", "seresnet50", "resnet50d", "resnet18d", "seresnext26d_32x4d")
MODELS.update({arch: ("nets", "ResNet", {"arch": arch}, 64) for arch in RESNETS})
MODELS["mobilenetv2_test"] = ("mobilenet", "MobileNetV2", {"arch": "mobilenetv2_test"}, 64)
MODELS.update({arch: ("efficientnet", "EfficientNet", {"arch": arch}, 64) for arch in ("efficientnet_test", "efficientnet_b1")})
# the models whose seed-0 weights the fixture keeps
STATE_MODELS = ("vit_tiny_test", "swin_test", "swin_test_w12", "convnext_test", "resnet50", "seresnext26d_32x4d", "mobilenetv2_test",
                "efficientnet_test")

# One case.  more: further constructor arguments; masks: drop-path masks per block (None: none injected); env: environment
# (None: unset).  A ResNet or routed ConvNeXt case also has answers = (what a *_supported query returns, {entry: another answer})
# -- with a table every *_stats_rows query returns 4 and every *_bytes query 256, so that the statistics and workspace buffers are
# real tensors; None: every entry returns 0 --, switches: import-time switches of the module `switch_module` (read when the model is
# constructed or run), attrs: attributes set on the model, hw: the input's height and width where it is not the model's square
# size, dfeat: one more phase after the accumulating backward, a backward from a gradient of the last stage's output.
Case = collections.namedtuple("Case", "model more masks env answers switches attrs hw switch_module dfeat",
                              defaults=({}, None, {}, None, {}, {}, None, "nets", False))
RESNET_ENV = {"ICAMD_WGRAD_STREAM": None, "ICAMD_EVAL_FOLD": None}


# every ResNet case sets every switch (a test's setter undoes itself only when the module is done)
SWITCHES = {"_FUSED_BNBWD": False, "_DUAL_BNBWD": True, "_SUB2_SHORTCUT": True, "_FUSED_POOL_BWD": True,
            "_STEM_THIN": {"fwd": True, "dgrad": True, "wgrad": False}}


def _resnet(arch, supported=1, by_entry=None, switches=None, **kw):
    return Case(arch, env=RESNET_ENV, answers=(supported, by_entry or {}), switches={**SWITCHES, **(switches or {})}, **kw)


# every ConvNeXt case sets convnext.py's one switch, for the same reason; the model reads it when it is constructed
def _convnext(model, drop, lane, supported=None, fused_ls=True):
    """supported: what icamd_dwconv7_wgrad_bias_supported answers (None: the two cases recorded first, without an answers table
    and without the dfeat phase)"""
    return Case(model, {"drop_path_rate": drop}, 1 if drop > 0.0 else None, {CNX_ENV: None if lane else "0"},
                answers=None if supported is None else (supported, {}), dfeat=supported is not None,
                switches={"_FUSED_LS": fused_ls}, switch_module="convnext")


# every MobileNetV2 case sets both routes of mobilenet.py's one switch, for the same reason; every query answers as for a ResNet case
def _mobilenet(onload):
    return Case("mobilenetv2_test", answers=(1, {}), switches={"DW_ONLOAD": {"fwd": onload, "wgrad": onload}},
                switch_module="mobilenet")


CASES = {
    "vit_tiny_test/lane_off": Case("vit_tiny_test", env={VIT_ENV: None}),
    "vit_tiny_test/lane_on": Case("vit_tiny_test", env={VIT_ENV: "1"}),
    "swin_test/no_drop": Case("swin_test", {"drop_path_rate": 0.0}),
    "swin_test/drop": Case("swin_test", {"drop_path_rate": DROP_PATH}, 2),
    "swin_test_w12/no_drop": Case("swin_test_w12", {"drop_path_rate": 0.0}),
    "swin_test_w12/drop": Case("swin_test_w12", {"drop_path_rate": DROP_PATH}, 2),
    "convnext_test/lane_on": _convnext("convnext_test", DROP_PATH, True),
    "convnext_test/lane_off": _convnext("convnext_test", DROP_PATH, False),
    "convnext_test/routed": _convnext("convnext_test", DROP_PATH, True, 1),
    "convnext_test/routed_no_drop": _convnext("convnext_test", 0.0, True, 1),
    "convnext_test/unfolded": _convnext("convnext_test", DROP_PATH, True, 0, fused_ls=False),
    "convnext_test/unfolded_lane_off": _convnext("convnext_test", DROP_PATH, False, 0, fused_ls=False),
    "convnextv2_test/drop": _convnext("convnextv2_test", DROP_PATH, True, 1),
    "convnextv2_test/no_drop_lane_off": _convnext("convnextv2_test", 0.0, False, 0),
    "resnet50/routed": _resnet("resnet50"),
    "resnet50/plain_odd_width": _resnet("resnet50", 0, hw=(64, 63)),
    "resnet50/gy_partials": _resnet("resnet50", 0, {"icamd_conv2d_dgrad_bnred_supported": 1}),
    "resnet50/switches_off": _resnet("resnet50", 0, switches={"_DUAL_BNBWD": False, "_SUB2_SHORTCUT": False,
                                                                "_FUSED_POOL_BWD": False}),
    "resnet50/fused_bnbwd": _resnet("resnet50", switches={"_FUSED_BNBWD": True}),
    "resnet50/one_stream_unfolded": _resnet("resnet50", attrs={"wgrad_side_stream": False, "fold_eval": False}),
    "resnet18/basic": _resnet("resnet18", 0),
    "resnext50_32x4d/routed": _resnet("resnext50_32x4d"),
    "seresnet50/routed": _resnet("seresnet50"),
    "resnet50d/thin_default": _resnet("resnet50d"),
    "resnet50d/thin_all": _resnet("resnet50d", switches={"_STEM_THIN": {"fwd": True, "dgrad": True, "wgrad": True}}),
    "resnet50d/thin_none_unfolded": _resnet("resnet50d", switches={"_STEM_THIN": {"fwd": False, "dgrad": False, "wgrad": False}},
                                            attrs={"fold_eval": False}),
    "resnet18d/basic": _resnet("resnet18d"),
    "seresnext26d_32x4d/folded": _resnet("seresnext26d_32x4d"),
    "seresnext26d_32x4d/unfolded": _resnet("seresnext26d_32x4d", attrs={"fold_eval": False}),
    "mobilenetv2_test/default": _mobilenet(False),
    "mobilenetv2_test/onload": _mobilenet(True),
    # EfficientNet has no switch; every query answers as for a ResNet case.  b1 is the one configuration whose blocks.0.1 is a
    # depthwise-separable block with a skip (its data gradient is added to the skip's by icamd_bn_apply)
    "efficientnet_test/default": Case("efficientnet_test", answers=(1, {})),
    "efficientnet_b1/ds_skip": Case("efficientnet_b1", answers=(1, {})),
}

TRACE = []          # the records of the case that is running
PHASES = []         # (phase, index into TRACE of its first record)
QUERIES = [0]       # its stream queries


class FuseFields(list):
    """The fields of a BnBwdFuse argument, taken when the call was made: seven pointers and the relu flag."""


class RecordingLib:
    """Stands in for libicamd.so: every entry of hip._SIGNATURES and hip._SIGNATURES_ADDED records its call and returns 0 -- or, for a query, what the
    running case's `answers` say (Case); any other name is an error."""
    answers = None

    def __getattr__(self, name):
        from imageclassification_amd import hip
        argtypes = (hip._SIGNATURES.get(name) or hip._SIGNATURES_ADDED[name])[1]

        def by_value(a):      # byref(ConvDesc) -> the descriptor's fields, byref(BnBwdFuse) -> its fields, taken now
            d = getattr(a, "_obj", None)
            if isinstance(d, hip.BnBwdFuse):
                return FuseFields(getattr(d, n) for n, _ in d._fields_)
            return d.key() if isinstance(d, hip.ConvDesc) else a

        def entry(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            TRACE.append((name, argtypes, tuple(by_value(a) for a in args)))
            if self.answers is None:
                return 0
            if name.endswith("_supported"):
                return self.answers[1].get(name, self.answers[0])
            return 4 if name.endswith("_stats_rows") else 256 if name.endswith("_bytes") else 0
        return entry


class _Stream:
    cuda_stream = 0


class RecordingLane:
    """streams.SideLane without streams or events: same interface, same bookkeeping, and a record of every wait it would make."""
    main = _Stream()

    def __init__(self, device, enabled=True):
        self.enabled = bool(enabled)
        self.side = 1 if self.enabled else None
        self._pending = set()
        self._launched = self._joined = 0

    def begin(self, enabled=True):
        self.enabled = self.side is not None and bool(enabled)
        self._pending.clear()
        self._launched = 0
        self._joined = 0

    @property
    def stream_ptr(self):
        return 1 if self.enabled else 0

    def launch(self, fn, reads=()):
        fn(self.stream_ptr)
        if self.enabled:
            self._launched += 1
            self._pending.update(reads)

    def before_write(self, *ptrs):
        for p in ptrs:
            if p in self._pending:
                self._pending.discard(p)
                TRACE.append(("lane.before_write", (ctypes.c_void_p, None), (p, None)))

    def events(self):
        return (self._launched,) if self._launched > self._joined else ()

    def join(self):
        TRACE.append(("lane.join", (ctypes.c_int,), (self._launched - self._joined,)))
        self._joined = self._launched
        self._pending.clear()


def _query(value):
    def f(*a, **k):
        QUERIES[0] += 1
        return value
    return f


def install_recorders(setattr_fn=setattr):
    """install_stubs plus the recording library, stream stand-in and lane; a test passes monkeypatch.setattr."""
    from imageclassification_amd import hip, streams
    L.install_stubs(setattr_fn)
    lib = RecordingLib()
    setattr_fn(hip, "load", lambda: lib)
    setattr_fn(hip, "stream_ptr", _query(0))
    setattr_fn(torch.cuda, "current_stream", _query(_Stream()))
    setattr_fn(streams, "SideLane", RecordingLane)


def build_model(model_id, **more):
    module, cls, kwargs, _ = MODELS[model_id]
    mod = importlib.import_module("imageclassification_amd." + module)
    return getattr(mod, cls)(num_classes=L.NUM_CLASSES, device="cpu", seed=0, **kwargs, **more)


def state_record(model):
    """What pins the weights a seed gives: a SHA-256 over the names and shapes of state_dict(), and per parameter its sum (in
    float64) and its first, middle and last element.  The values themselves are not hashed: the draws are the generator's, the same
    everywhere, but trunc_normal_ evaluates erfinv, which differs in the last bits from one CPU to another; a draw that moved changes
    every figure here by far more (STATE_TOL)."""
    sd = model.state_dict()
    h = hashlib.sha256(json.dumps([[n, list(t.shape)] for n, t in sd.items()]).encode()).hexdigest()
    flat = [t.double().flatten() for t in sd.values()]
    return {"names_and_shapes_sha256": h,
            "values": [[float(f.sum()), float(f[0]), float(f[f.numel() // 2]), float(f[-1])] for f in flat]}


# |weight| stays below this (0.25 where a model is not listed).  A ResNet's filters are Kaiming-normal with std sqrt(2 / (cout k k)),
# at most 0.354 (the 16-row first SE convolution): 4.0 is more than 11 standard deviations.  MobileNetV2's depthwise filters are
# N(0, sqrt(2 / 9)) = 0.471: 4.0 is 8.5 of them.  EfficientNet's widest draw is the conv_reduce of a squeeze-and-excitation whose
# reduced width is 2 (blocks.1.0 of efficientnet_test: fan_out = 2, std 1.0): 8.0 is 8 of them
STATE_BOUND = {"resnet50": 4.0, "seresnext26d_32x4d": 4.0, "mobilenetv2_test": 4.0, "efficientnet_test": 8.0}


def state_tol(numel, bound=0.25):
    """(tolerance of a parameter's sum, of one element): the weights are below `bound` = 0.25 in magnitude except the LayerNorm ones,
    which are exact, so one float32 ulp is at most 1.5e-8 and a few ulps of evaluation difference stay below 1e-7 per element --
    summed over the parameter in the worst case.  A larger bound scales the ulp, and both tolerances, with it.  A parameter drawn
    from other random numbers moves its sum by about 0.02 * sqrt(numel)."""
    return 1e-7 * (bound / 0.25) * numel, 1e-7 * (bound / 0.25)


def _masks(model, per_block):
    """Per residual branch one [BATCH] mask of {0, 1 / keep_prob}, the zero alternating between the two samples; ones for a
    block whose rate is 0 (never read)."""
    out = []
    for st in model.stages:
        for blk in st["blocks"]:
            for _ in range(per_block):
                c = 1.0 / (1.0 - blk["rate"])
                m = [c, 0.0] if len(out) % 2 else [0.0, c]
                out.append(torch.tensor(m if blk["rate"] > 0.0 else [1.0, 1.0], dtype=torch.float32))
    return out


def _collect(obj, held, seen):
    """Every tensor reachable from `obj` through dicts, sequences and attributes: storage address -> (bytes, the tensor)."""
    if id(obj) in seen or obj is None or isinstance(obj, (int, float, str, bytes, bool, type)):
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        st = obj.untyped_storage()
        if st.nbytes():
            held.setdefault(st.data_ptr(), (st.nbytes(), obj))
    elif isinstance(obj, dict):
        for v in obj.values():
            _collect(v, held, seen)
    elif isinstance(obj, (list, tuple, set)):
        for v in obj:
            _collect(v, held, seen)
    elif hasattr(obj, "__dict__") and not callable(obj):
        _collect(vars(obj), held, seen)


def canonical(trace, held, x):
    """The trace with every argument in its canonical form (module docstring); LookupError for a pointer into no buffer."""
    bases = sorted(held)
    order = {}

    def pointer(p, where):
        if not p:
            return None
        i = bisect.bisect_right(bases, p) - 1
        if i < 0 or p >= bases[i] + held[bases[i]][0]:
            raise LookupError(f"{where}: pointer {p:#x} is in no tensor of the model")
        base = bases[i]
        if base == x.untyped_storage().data_ptr():
            return "input" if p == base else ["input", p - base]
        return [order.setdefault(base, len(order)), p - base, held[base][0]]

    out = []
    for name, argtypes, args in trace:
        row = [name]
        for k, (t, a) in enumerate(zip(argtypes, args)):
            if isinstance(a, FuseFields):
                row.append([pointer(v, f"{name} argument {k}") for v in a[:-1]] + [int(a[-1])])
            elif isinstance(a, tuple):
                row.append(list(a))
            elif t is ctypes.c_void_p:
                row.append(f"stream {a}" if k == len(args) - 1 else pointer(a, f"{name} argument {k}"))
            elif t is ctypes.c_float or isinstance(a, float):
                row.append(repr(float(a)))
            else:
                row.append(None if a is None else int(a))
        out.append(row)
    return out


def run_case(case_id, setenv=None, dump=None, setattr_fn=None, observer=None):
    """-> {"sha256", "calls", "stream_queries"} of one case, under install_recorders; dump: a file for the records, one per line.
    setenv(name, value or None) changes the environment and setattr_fn(module, switch, value) a switch of the case's module (a test passes
    functions that undo themselves); by default os.environ and setattr, restored at the end.  observer(model, held, x) is called once
    every phase has run, with the model, the buffers TRACE's pointers lie in and the image batch (tests/_stream_order.py)."""
    from imageclassification_amd import hip
    case = CASES[case_id]
    saved = {k: os.environ.get(k) for k in case.env}
    saved_switches = {}

    def default_setenv(k, v):
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    for k, v in case.env.items():
        (setenv or default_setenv)(k, v)
    try:
        if case.switches:
            nets = importlib.import_module("imageclassification_amd." + case.switch_module)
            for k, v in case.switches.items():
                saved_switches[k] = getattr(nets, k)
                (setattr_fn or setattr)(nets, k, v)
        hip.load().answers = case.answers
        del TRACE[:], PHASES[:]
        QUERIES[0] = 0
        held = {}
        model = build_model(case.model, **case.more)
        for k, v in case.attrs.items():
            assert hasattr(model, k), k
            setattr(model, k, v)

        def phase(name, run):
            PHASES.append((name, len(TRACE)))
            result = run()
            _collect(vars(model), held, set())
            return result

        model.grad_ready_hook = lambda lo, hi, events=(): TRACE.append(
            ("hook", (ctypes.c_int, ctypes.c_int, None), (lo, hi, tuple(events))))
        if case.masks:
            model.injected_keep = _masks(model, case.masks)
        h, w = case.hw or (MODELS[case.model][3],) * 2
        x = torch.randn(BATCH, 3, h, w, generator=torch.Generator().manual_seed(1))
        held[x.untyped_storage().data_ptr()] = (x.untyped_storage().nbytes(), x)
        PHASES.append(("construct", 0))
        phase("train", model.train)
        ws = phase("pack", lambda: model.pack(x))
        phase("forward", lambda: model.forward_packed(ws))
        phase("backward", lambda: model.backward_packed(ws))
        phase("backward_accumulate", lambda: model.backward_packed(ws, accumulate=True))
        if case.dfeat:
            dfeat = torch.zeros(BATCH, *ws["final_hw"], model.dims[-1], dtype=torch.bfloat16)
            phase("backward_dfeat", lambda: model.backward_packed(ws, dfeat=dfeat))
        phase("eval", model.eval)
        phase("eval_forward", lambda: model.forward_packed(ws, logits_only=True))
        if MODELS[case.model][0] == "nets":
            phase("eval_forward_again", lambda: model.forward_packed(ws, logits_only=True))
        phase("reload", lambda: model.load_state_dict(model.state_dict()))
        if observer is not None:
            observer(model, held, x)
        rows = canonical(TRACE, held, x)
    finally:
        hip.load().answers = None
        if setenv is None:
            for k, v in saved.items():
                default_setenv(k, v)
        if setattr_fn is None:
            for k, v in saved_switches.items():
                setattr(nets, k, v)
    blob = json.dumps(rows, separators=(",", ":"))
    if dump:
        with open(dump, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    return {"sha256": hashlib.sha256(blob.encode()).hexdigest(), "calls": len(rows), "stream_queries": QUERIES[0]}


def phase_records(name):
    """The records of TRACE that phase `name` of the case just run made."""
    starts = [i for _, i in PHASES] + [len(TRACE)]
    k = [n for n, _ in PHASES].index(name)
    return TRACE[starts[k]:starts[k + 1]]


def main():
    install_recorders()
    if sys.argv[1:2] == ["--dump"]:
        os.makedirs(sys.argv[2], exist_ok=True)
        for case_id in CASES:
            print(case_id, run_case(case_id, dump=os.path.join(sys.argv[2], case_id.replace("/", "__") + ".jsonl")))
        return
    out = {"generator": "tests/golden/make_call_traces.py", "num_classes": L.NUM_CLASSES, "batch": BATCH, "cases": {},
           "state_dict_seed0": {}}
    for case_id in CASES:
        out["cases"][case_id] = run_case(case_id)
        print(case_id, out["cases"][case_id])
    for model_id in STATE_MODELS:
        out["state_dict_seed0"][model_id] = state_record(build_model(model_id))
        print(model_id, out["state_dict_seed0"][model_id]["names_and_shapes_sha256"])
    with open(os.path.join(HERE, "call_traces.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
