"""Is the side stream of a backward pass ordered against the main stream wherever the two touch the same bytes?  Answered from the
call trace of tests/golden/make_call_traces.py, without a GPU.

Access model   include/icamd.h is parsed (`DECLS`): of every exported entry a `const T*` argument is read, any other pointer is
               written (and conflicts with reads as well), the trailing `void* stream` is the launch's stream; the fields of
               icamd_bn_bwd_fuse the same way (`FUSE_FIELDS`).  An entry without a stream argument is a host query and launches nothing.
Extent         a pointer into param_arena / grad_arena / shadow covers the padded range of the Param it lies in, one into shadow_t the
               transpose-table entry, one into buffer_arena the running statistics of its BatchNorm; a pointer into any other tensor
               covers everything from itself to the end of the storage (conservative).  `EXACT` and `WHOLE` hold the arguments whose
               contract in the header says otherwise.
Ordering       the case runs with the real streams.SideLane driven over stand-ins for torch.cuda.Stream (side stream 1, main stream 0)
               and torch.cuda.Event that log every record(stream) and wait_event(event) with the position in TRACE (`LOG`); happens-before
               is program order per stream plus record -> wait, kept as one vector clock per launch.  `ObservingLane` derives from the
               generator's RecordingLane and forwards every call to both, so TRACE stays what RecordingLane alone produces.

`observe(case_id, ...)` runs a case and returns a `Run`; hazards / unjoined / late_writes take that Run.
"""
import bisect
import collections
import ctypes
import importlib.util
import os
import re

import torch

from imageclassification_amd import hip, streams

RealSideLane = streams.SideLane          # taken at import, before any test replaces the module's attribute

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_call_traces_for_stream_order", os.path.join(HERE, "golden", "make_call_traces.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

HEADER = os.path.join(os.path.dirname(HERE), "include", "icamd.h")
BACKWARD_PHASES = ("backward", "backward_accumulate", "backward_dfeat")
MAIN, SIDE = 0, 1

# ---------------------------------------------------------------------------------------------------------------- access model
Arg = collections.namedtuple("Arg", "name pointer const")
Decl = collections.namedtuple("Decl", "args stream")        # stream: the entry's last argument is `void* stream`


def _declarators(statement):
    """`const float *mean, *invstd` -> [Arg(mean, True, True), Arg(invstd, True, True)]; `int relu` -> [Arg(relu, False, False)]"""
    statement = statement.strip()
    const = statement.startswith("const ")
    out = []
    for piece in statement.split(","):
        name = re.findall(r"[A-Za-z_]\w*", piece)[-1]
        out.append(Arg(name, "*" in piece, const and "*" in piece))
    return out


def parse_header(path=HEADER):
    """-> ({entry: Decl}, [Arg of every field of icamd_bn_bwd_fuse])"""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decls = {}
    for name, body in re.findall(r"\b(?:int|size_t)\s+(icamd_\w+)\s*\(([^)]*)\)\s*;", text):
        args = [] if body.strip() in ("", "void") else [_declarators(a)[0] for a in body.split(",")]
        stream = bool(args) and args[-1] == Arg("stream", True, False)
        decls[name] = Decl(tuple(args), stream)
    struct = re.search(r"typedef\s+struct\s+icamd_bn_bwd_fuse\s*\{(.*?)\}", text, flags=re.S).group(1)
    fields = [a for st in struct.split(";") if st.strip() for a in _declarators(st)]
    return decls, fields


DECLS, FUSE_FIELDS = parse_header()


def _bytes(count, width):
    return lambda a: width * a[count]


# (entry, argument) -> bytes it covers from its pointer on, as a function of the call's arguments by name: arguments the conservative
# rule (or, in an arena, the one-parameter rule) gets wrong.  Each with the line of include/icamd.h that states it.
EXACT = {
    # "int icamd_f32_to_bf16(const float* src, void* dst, long long n, void* stream);" -- n elements each way, whatever the pointers'
    # arenas hold there (refresh_shadow converts the whole parameter arena in one call)
    ("icamd_f32_to_bf16", "src"): _bytes("n", 4),
    ("icamd_f32_to_bf16", "dst"): _bytes("n", 2),
}
# (entry, argument): the base of an arena, addressed through a table of offsets -- the whole storage.
WHOLE = {
    # "descs: int64[nlayers][8] = {src_off, dst_off, Cout, T, Cin, 0,0,0} (element offsets)"
    ("icamd_filter_transpose", "src_base"), ("icamd_filter_transpose", "dst_base"),
    ("icamd_filter_transpose_tiled", "src_base"), ("icamd_filter_transpose_tiled", "dst_base"),
    # "jobs = device array of njobs rows of 8 x int64 {filter offset (elements: the same in the fp32 arena `params` and in its bf16
    # `shadow`), gamma offset, bias offset (both in `params`), folded-bias offset (in fold_bias), ..."
    ("icamd_layerscale_fold", "params"), ("icamd_layerscale_fold", "shadow"), ("icamd_layerscale_fold", "fold_bias"),
}

# ---------------------------------------------------------------------------------------------------------------- the stand-ins
LOG = []        # ("record" | "wait", position in TRACE, event, stream) and ("events", position, the lane's events) of the running case


class FakeStream:
    def __init__(self, device=None, cuda_stream=SIDE):
        self.cuda_stream = cuda_stream

    def wait_event(self, event):
        LOG.append(("wait", len(G.TRACE), event.id, self.cuda_stream))


MAIN_STREAM = FakeStream(cuda_stream=MAIN)


class FakeEvent:
    count = 0

    def __init__(self, *a, **k):
        FakeEvent.count += 1
        self.id = FakeEvent.count

    def record(self, stream=None):
        LOG.append(("record", len(G.TRACE), self.id, (stream or MAIN_STREAM).cuda_stream))

    def synchronize(self):
        pass


class ObservingLane(G.RecordingLane):
    """RecordingLane (what TRACE keeps) and, beside it, the real SideLane on the stand-ins (what LOG keeps); a launch runs once."""

    def __init__(self, device, enabled=True):
        super().__init__(device, enabled)
        self.real = RealSideLane(device, enabled)

    def begin(self, enabled=True):
        super().begin(enabled)
        queries = G.QUERIES[0]
        self.real.begin(enabled)            # asks for the current stream, which RecordingLane does not
        G.QUERIES[0] = queries

    def launch(self, fn, reads=()):
        assert self.real.stream_ptr == self.stream_ptr
        self.real.launch(fn, reads)
        super().launch(lambda stream: None, reads)

    def before_write(self, *ptrs):
        super().before_write(*ptrs)
        self.real.before_write(*ptrs)

    def events(self):
        # hooks() pairs a hook with these events by the position in TRACE: it assumes what every caller writes today,
        # `hook(lo, hi, lane.events())`, with no library call between the two.  A caller that kept the events and called the hook after
        # another launch would be read as passing none, and late_writes would then report side writes that the kept events do cover.
        LOG.append(("events", len(G.TRACE), tuple(e.id for e in self.real.events())))
        return super().events()

    def join(self):
        super().join()
        self.real.join()


def install(setattr_fn=setattr):
    """The generator's install_recorders, then the stand-ins and the observing lane; a test passes monkeypatch.setattr."""
    G.install_recorders(setattr_fn)
    setattr_fn(torch.cuda, "Stream", FakeStream)
    setattr_fn(torch.cuda, "Event", FakeEvent)
    setattr_fn(torch.cuda, "current_stream", G._query(MAIN_STREAM))
    setattr_fn(streams, "SideLane", ObservingLane)


# ---------------------------------------------------------------------------------------------------------------- one run
Access = collections.namedtuple("Access", "index entry arg stream write base start end")


def _walk(obj, path, seen, visit):
    """visit(path, obj) for every tensor and every plain object reachable from `obj` (the generator's _collect, with the way there)"""
    if id(obj) in seen or obj is None or isinstance(obj, (int, float, str, bytes, bool, type)):
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        visit(path, obj)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _walk(v, f"{path}[{k!r}]", seen, visit)
    elif isinstance(obj, (list, tuple, set)):
        for k, v in enumerate(obj):
            _walk(v, f"{path}[{k}]", seen, visit)
    elif hasattr(obj, "__dict__") and not callable(obj):
        visit(path, obj)
        for k, v in vars(obj).items():
            _walk(v, f"{path}.{k}", seen, visit)


class Run:
    """What one case left: the trace, its phases, the lane's log, and from them the accesses and the vector clocks."""

    def __init__(self, trace, phases, log, held, model=None, names=None, case_id=None, result=None):
        """trace, phases [(name, index of its first record)] and log as the generator's TRACE and PHASES and this module's LOG; held:
        {storage address: (bytes, anything)}.  With a model the arenas take their extents from its tables and the buffers their names
        from its attributes; without one (a hand-written trace) there are no arenas and `names` {storage address: name} names the
        buffers."""
        self.case_id, self.trace, self.log, self.model, self.held, self.result = case_id, trace, log, model, held, result
        starts = [i for _, i in phases] + [len(trace)]
        self.phases = [(n, starts[k], starts[k + 1]) for k, (n, _) in enumerate(phases)]
        self.backward = [(n, a, b) for n, a, b in self.phases if n in BACKWARD_PHASES]
        self._bases = sorted(held)
        self.names, self.arenas, self.grad_base = dict(names or {}), {}, None
        if model is not None:
            self._layout(model)
        self.accesses = [a for i, r in enumerate(trace) for a in self._accesses_of(i, r)]
        self._clocks()

    # -- buffers
    def _layout(self, model):
        bns, seen = [], set()

        def visit(path, obj):
            if isinstance(obj, torch.Tensor):
                if obj.untyped_storage().nbytes():
                    self.names.setdefault(obj.untyped_storage().data_ptr(), path)
            elif {"buf_offset", "c", "name"} <= set(vars(obj)):
                bns.append(obj)
        for k, v in vars(model).items():           # (the model itself is callable, which _walk takes for a function)
            _walk(v, f"model.{k}", seen, visit)
        params = [(p.offset, p.offset + p.numel, p.name) for p in model.params.values()]
        for attr, width in (("param_arena", 4), ("grad_arena", 4), ("shadow", 2)):
            self._arena(getattr(model, attr), attr, width, params)
        by_offset = {p.offset: p.name for p in model.params.values()}
        self._arena(model.shadow_t, "shadow_t", 2, [(dst, dst + cout * taps * cin, by_offset[src])
                                                    for src, dst, cout, taps, cin, *_ in model._tr_descs.tolist()])
        self._arena(model.buffer_arena, "buffer_arena", 4, [(b.buf_offset, b.buf_offset + 2 * b.c, b.name) for b in bns])
        self.grad_base = model.grad_arena.untyped_storage().data_ptr()

    def _arena(self, tensor, attr, width, ranges):
        ranges = sorted((lo * width, hi * width, name) for lo, hi, name in ranges)
        assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), attr
        self.arenas[tensor.untyped_storage().data_ptr()] = (attr, ranges, [r[0] for r in ranges])

    def _buffer(self, ptr, where):
        i = bisect.bisect_right(self._bases, ptr) - 1
        if i < 0 or ptr >= self._bases[i] + self.held[self._bases[i]][0]:
            raise LookupError(f"{where}: pointer {ptr:#x} is in no tensor of the model")
        return self._bases[i], self.held[self._bases[i]][0]

    def _extent(self, ptr, entry, arg, by_name):
        where = f"{entry} argument {arg}"
        base, nbytes = self._buffer(ptr, where)
        off = ptr - base
        if (entry, arg) in EXACT:
            end = off + EXACT[entry, arg](by_name)
            assert end <= nbytes, where
            return base, off, end
        if base in self.arenas and (entry, arg) not in WHOLE:
            attr, ranges, starts = self.arenas[base]
            k = bisect.bisect_right(starts, off) - 1
            if k >= 0 and off < ranges[k][1]:
                return base, ranges[k][0], ranges[k][1]
            if ranges:
                raise LookupError(f"{where}: byte {off} of {attr} is in no entry of its table")
        return base, off, nbytes

    def describe(self, base, start):
        if base in self.arenas and self.arenas[base][1]:
            attr, ranges, starts = self.arenas[base]
            k = bisect.bisect_right(starts, start) - 1
            return f"{attr}[{ranges[k][2]}]" if k >= 0 and start < ranges[k][1] else attr
        return f"{self.names.get(base, hex(base))} + {start}"

    def _accesses_of(self, index, record):
        entry, _, args = record
        decl = DECLS.get(entry)
        if decl is None or not decl.stream:
            return
        stream = int(args[-1] or 0)
        by_name = {a.name: v for a, v in zip(decl.args, args)}
        for a, v in zip(decl.args[:-1], args):
            if not a.pointer or isinstance(v, tuple):      # a tuple: the key() of a ConvDesc, recorded by value -- host memory
                continue
            fields = [(f"{a.name}.{f.name}", f, x) for f, x in zip(FUSE_FIELDS, v)] if isinstance(v, G.FuseFields) else [(a.name, a, v)]
            for name, role, ptr in fields:
                if role.pointer and ptr:
                    yield Access(index, entry, name, stream, not role.const, *self._extent(int(ptr), entry, name, by_name))

    # -- happens-before
    def _clocks(self):
        """Per launch its (stream, number on that stream) and vector clock; per event the clock of its record; per position in TRACE
        the main stream's clock before that record."""
        clock = collections.defaultdict(dict)
        count = collections.Counter()
        self.position, self.clock, self.event_clock, self.events_at, self.main_before = {}, {}, {}, {}, []
        log, k = self.log, 0

        def flush(upto):
            nonlocal k
            while k < len(log) and log[k][1] <= upto:
                kind, pos, *rest = log[k]
                k += 1
                if kind == "record":
                    self.event_clock[rest[0]] = dict(clock[rest[1]])
                elif kind == "wait":
                    seen = self.event_clock[rest[0]]       # KeyError: a wait for an event that was never recorded
                    mine = clock[rest[1]]
                    for s, n in seen.items():
                        mine[s] = max(mine.get(s, 0), n)
                else:
                    self.events_at[pos] = rest[0]

        for i, (entry, _, args) in enumerate(self.trace):
            flush(i)
            self.main_before.append(dict(clock[MAIN]))
            decl = DECLS.get(entry)
            if decl is not None and decl.stream:
                s = int(args[-1] or 0)
                count[s] += 1
                clock[s][s] = count[s]
                self.position[i], self.clock[i] = (s, count[s]), dict(clock[s])
        flush(len(self.trace))
        self.main_before.append(dict(clock[MAIN]))

    def ordered(self, i, j):
        """Is there a happens-before path between the launches at TRACE[i] and TRACE[j], either way?"""
        (si, ni), (sj, nj) = self.position[i], self.position[j]
        return self.clock[j].get(si, 0) >= ni or self.clock[i].get(sj, 0) >= nj

    def side_launches(self):
        return [i for _, a, b in self.backward for i in range(a, b) if self.position.get(i, (MAIN,))[0] != MAIN]

    def side_launches_anywhere(self):
        return [i for i, (s, _) in self.position.items() if s != MAIN]

    @staticmethod
    def tell(a):
        return (a.entry, a.arg, a.stream, a.index)

    @classmethod
    def from_records(cls, records, log, buffers):
        """A hand-written trace: records (entry, {argument: (buffer, byte offset)}, stream), log as LOG, buffers {name: bytes}.  The
        arguments not named are NULL / 0; the whole trace is one phase, "backward"."""
        bases, at = {}, 1 << 20
        for name, nbytes in buffers.items():
            bases[name] = at
            at += nbytes + 4096
        trace = []
        for entry, ptrs, stream in records:
            args = [bases[ptrs[a.name][0]] + ptrs[a.name][1] if a.name in ptrs else (None if a.pointer else 0)
                    for a in DECLS[entry].args[:-1]]
            trace.append((entry, None, tuple(args) + (stream,)))
        return cls(trace, [("backward", 0)], list(log), {bases[n]: (nbytes, None) for n, nbytes in buffers.items()},
                   names={bases[n]: n for n in buffers})


def observe(case_id, setenv=None, setattr_fn=None):
    """Run a case of G.CASES under `install` -> Run."""
    del LOG[:]
    got = {}
    result = G.run_case(case_id, setenv, setattr_fn=setattr_fn, observer=lambda model, held, x: got.update(model=model, held=dict(held)))
    return Run(list(G.TRACE), list(G.PHASES), list(LOG), got["held"], got["model"], case_id=case_id, result=result)


from_records = Run.from_records


# ---------------------------------------------------------------------------------------------------------------- the three checks
def conflicting_pairs(run):
    """Every pair of accesses on different streams whose extents overlap and of which one writes (ordered or not)."""
    by_base = collections.defaultdict(lambda: collections.defaultdict(list))
    for a in run.accesses:
        by_base[a.base][a.stream].append(a)
    for per_stream in by_base.values():
        ids = sorted(per_stream)
        for x, s in enumerate(ids):
            for t in ids[x + 1:]:
                for a in per_stream[s]:
                    for b in per_stream[t]:
                        if (a.write or b.write) and a.start < b.end and b.start < a.end:
                            yield a, b


def hazards(run, counts=None):
    """The conflicting pairs with no happens-before path between them: ((entry, argument, stream, trace index) twice, the buffer).
    counts: a dict that receives "pairs", the number of conflicting pairs examined."""
    out, n = [], 0
    for a, b in conflicting_pairs(run):
        n += 1
        if not run.ordered(a.index, b.index):
            out.append((run.tell(a), run.tell(b), run.describe(a.base, max(a.start, b.start))))
    if counts is not None:
        counts["pairs"] = n
    return out


def unjoined(run):
    """Side launches the main stream has not waited for when their backward phase ends: (phase, entry, trace index)."""
    out = []
    for name, a, b in run.backward:
        seen = run.main_before[b]
        for i in range(a, b):
            s, n = run.position.get(i, (MAIN, 0))
            if s != MAIN and seen.get(s, 0) < n:
                out.append((name, run.trace[i][0], i))
    return out


def hooks(run):
    """(phase, trace index, lo, the lane's events when the hook was called) of every grad_ready_hook call of the backward phases"""
    return [(name, i, run.trace[i][2][0], run.events_at.get(i, ())) for name, a, b in run.backward for i in range(a, b)
            if run.trace[i][0] == "hook"]


def late_writes(run):
    """Per hook(lo, hi, events): a write into grad_arena at or above element `lo` that comes later in the same backward, or that a
    side stream made earlier and neither the main stream nor `events` covers: (phase, hook's trace index, lo, the write, the buffer)."""
    out = []
    ends = {name: (a, b) for name, a, b in run.backward}
    grads = [a for a in run.accesses if a.base == run.grad_base and a.write]
    for name, i, lo, events in hooks(run):
        first, last = ends[name]
        main = run.main_before[i]
        for a in grads:
            if not first <= a.index < last or a.end <= 4 * lo:
                continue
            s, n = run.position[a.index]
            if a.index > i:
                late = True
            else:
                late = s != MAIN and main.get(s, 0) < n and not any(run.event_clock[e].get(s, 0) >= n for e in events)
            if late:
                out.append((name, i, lo, run.tell(a), run.describe(a.base, a.start)))
    return out
