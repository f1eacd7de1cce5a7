"""The flat-arena protocol every model of the package is written against, defined once.

A model keeps all its parameters in one fp32 tensor (`param_arena`), their gradients in a second of the same layout (`grad_arena`),
a bf16 copy the kernels read (`shadow`), the transposed bf16 filters of the data-gradient kernels (`shadow_t`) and its fp32 buffers
(`buffer_arena`).  `params` maps every state_dict name to a `Param`: a slice of the arenas (offsets are multiples of 64 elements,
256 B of fp32) plus the torch shape and the padded arena shape.  engine.py, ema.py, ddp.py, optim_factory.py, checkpoint.py and
bench.py address parameters by these offsets and names, so the layout rules live here and nowhere else:

  Layout            assigns the offsets as the model names its parameters
  to_arena / from_arena   torch layout <-> arena layout of one parameter, by kind ("conv", "lin", "dw", "vec")
  plan_transposes   lays out `shadow_t` and the job tables of icamd_filter_transpose_tiled / icamd_filter_transpose
  ArenaModel        the arenas, state_dict / load_state_dict, the bf16 refresh and the nn.Module surface the rest of the package uses

A model derives from ArenaModel, describes its parameters to a Layout, calls `_allocate`, and supplies `_ctor_kwargs`,
`init_weights`, `pack`, `forward_packed` and `backward_packed`; what differs between models goes into overrides (`refresh_transposed`
for work around the transposes, `_buffer_keys` / `_load_buffers` / `state_dict` for buffers, `train` for mode-dependent state).
`Lin` and `ArenaModel._draw_keep` are kept here; the steps and the transformer block the token models share are blocks.py's, what
the BatchNorm families share is bnmodel.py's.
"""
from collections import OrderedDict

import torch

from . import hip
from .checkpoint import PicklableModel


def align(n, a):
    return (n + a - 1) // a * a


class Param:
    """One logical parameter: a slice of the flat arenas plus its torch-layout shape."""
    __slots__ = ("name", "offset", "numel", "torch_shape", "kind", "padded_shape")

    def __init__(self, name, offset, numel, torch_shape, kind, padded_shape):
        self.name, self.offset, self.numel = name, offset, numel
        self.torch_shape, self.kind, self.padded_shape = torch_shape, kind, padded_shape


class Layout:
    """Assigns arena offsets in the order parameters are added: every slice starts at a multiple of 64 elements."""

    def __init__(self):
        self.params = OrderedDict()
        self.size = 0

    def add(self, name, torch_shape, kind, padded_shape=None):
        padded_shape = tuple(torch_shape if padded_shape is None else padded_shape)
        numel = 1
        for s in padded_shape:
            numel *= s
        p = self.params[name] = Param(name, self.size, numel, tuple(torch_shape), kind, padded_shape)
        self.size = align(self.size + numel, 64)
        return p


def to_arena(p, t):
    """Tensor `t` in torch layout -> the flat fp32 arena slice of `p` (zero where the arena shape is padded).
    conv: (cout, cin, kh, kw) -> [cout_p][kh_p][kw_p][cin_p];  lin: (out, in) or (out, in, 1, 1) -> [out_p][in];
    dw: (C, 1, kh, kw) -> [kh][kw][C];  vec: any rank, flattened."""
    t = t.detach().to(torch.float32).cpu()
    if p.kind == "lin" and t.dim() == 4 and tuple(t.shape[2:]) == (1, 1):
        t = t[:, :, 0, 0]
    if tuple(t.shape) != p.torch_shape:
        raise ValueError(f"size mismatch for {p.name}: {tuple(t.shape)} vs {p.torch_shape}")
    full = torch.zeros(p.padded_shape)
    if p.kind == "conv":
        cout, cin, kh, kw = t.shape
        full[:cout, :kh, :kw, :cin] = t.permute(0, 2, 3, 1)
    elif p.kind == "lin":
        full.view(p.padded_shape[0], -1)[: t.shape[0]] = t
    elif p.kind == "dw":
        full[:] = t[:, 0].permute(1, 2, 0)
    else:
        full.view(-1)[: t.numel()] = t.flatten()
    return full.flatten()


def from_arena(p, flat):
    """The inverse of to_arena: the arena slice `flat` of `p` -> a tensor of p.torch_shape."""
    t = flat.reshape(p.padded_shape)
    if p.kind == "conv":
        cout, cin, kh, kw = p.torch_shape
        return t[:cout, :kh, :kw, :cin].permute(0, 3, 1, 2).contiguous()
    if p.kind == "lin":
        return t.reshape(p.padded_shape[0], -1)[: p.torch_shape[0]].clone()
    if p.kind == "dw":
        return t.permute(2, 0, 1).reshape(p.torch_shape).contiguous()
    n = 1
    for s in p.torch_shape:
        n *= s
    return t.flatten()[:n].reshape(p.torch_shape).clone()


def plan_transposes(layers):
    """`layers`: [(layer, cout_p, taps, cin_p)] of the filters [cout_p][taps][cin_p] that need a transposed copy; sets each
    layer.wt_offset (128-element aligned) and returns (descriptors, tiled jobs, linear jobs, elements of shadow_t).  A filter whose
    cout_p and cin_p are multiples of 64 is moved in 64 x 64 tiles (taps outermost, then co0, then ci0), any other one in runs of
    4096 elements."""
    toff, descs, tjobs, jobs = 0, [], [], []
    for layer, cout_p, taps, cin_p in layers:
        layer.wt_offset = toff
        descs.append([layer.w.offset, toff, cout_p, taps, cin_p, 0, 0, 0])
        i = len(descs) - 1
        if cout_p % 64 == 0 and cin_p % 64 == 0:
            tjobs += [[i, t, co0, ci0] for t in range(taps) for co0 in range(0, cout_p, 64) for ci0 in range(0, cin_p, 64)]
        else:
            jobs += [[i, s] for s in range(0, layer.w.numel, 4096)]
        toff = align(toff + layer.w.numel, 128)
    return descs, tjobs, jobs, toff


class Lin:
    """Linear layer = 1x1 convolution record (weight [out_p][in] in the arena; `b` is None for a bias-free layer)."""

    def __init__(self, name, cin, cout, cout_p=None):
        self.name, self.cin, self.cout = name, cin, cout
        self.cout_p = cout_p or cout
        self.w = self.b = None
        self.wt_offset = None
        self.descs = {}

    def desc(self, rows):
        d = self.descs.get(rows)
        if d is None:
            d = hip.conv_desc(rows, 1, 1, self.cin, self.cout_p, 1, 1, 1, 0)
            self.descs[rows] = d
        return d


class ArenaModel(PicklableModel):
    def __init__(self, arch, num_classes, device):
        hip.require_gpu()
        self.lib = hip.load()
        self.arch, self.num_classes = arch, num_classes
        self.device = torch.device(device)
        self.training = True
        self.ncls_p = align(num_classes, 64)     # the classifier's rows in the arena
        self.num_batches_tracked = 0
        # called as gradients complete with (param_offset_lo, param_offset_hi or None, events): `events` are side-stream events a
        # consumer on another stream must wait for besides the main stream
        self.grad_ready_hook = None
        self._ws = {}

    def _allocate(self, layout, transposed, buffer_elems=0):
        """The arenas of `layout` and the transpose tables of `transposed` (plan_transposes' argument)."""
        dev = self.device
        self.params = layout.params
        self.n_params = layout.size
        self.param_arena = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.grad_arena = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.shadow = torch.zeros(self.n_params, dtype=torch.bfloat16, device=dev)
        # a model without buffers keeps 64 elements for the EMA / DDP protocol
        self.buffer_arena = torch.zeros(max(buffer_elems, 64), dtype=torch.float32, device=dev)
        descs, tjobs, jobs, toff = plan_transposes(transposed)
        self.shadow_t = torch.zeros(toff, dtype=torch.bfloat16, device=dev)
        self._tr_descs = torch.tensor(descs, dtype=torch.int64, device=dev)
        self._tr_tjobs = torch.tensor(tjobs if tjobs else [[0, 0, 0, 0]], dtype=torch.int32, device=dev)
        self._tr_ntjobs = len(tjobs)
        self._tr_jobs = torch.tensor(jobs if jobs else [[0, 0]], dtype=torch.int32, device=dev)
        self._tr_njobs = len(jobs)

    # ------------------------------------------------------------------ parameters / state_dict
    def _buffer_keys(self):
        """state_dict keys besides the parameters that load_state_dict expects (BatchNorm running statistics)."""
        return []

    def _load_buffers(self, sd):
        pass

    def load_state_dict(self, sd, strict=True):
        missing = [n for n in self.params if n not in sd] + [k for k in self._buffer_keys() if k not in sd]
        if strict and missing:
            raise KeyError(f"missing keys in state_dict: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        host = self.param_arena.cpu()
        for name, p in self.params.items():
            if name in sd:
                host[p.offset:p.offset + p.numel] = to_arena(p, sd[name])
        self.param_arena.copy_(host)
        self._load_buffers(sd)
        self.refresh_shadow()
        return missing

    def state_dict(self):
        host = self.param_arena.cpu()
        return OrderedDict((n, from_arena(p, host[p.offset:p.offset + p.numel])) for n, p in self.params.items())

    def named_parameters(self):
        """(name, fp32 arena view) pairs; the views alias the flat parameter arena."""
        for name, p in self.params.items():
            yield name, self.param_arena[p.offset:p.offset + p.numel]

    def parameters(self):
        for _, v in self.named_parameters():
            yield v

    def grad_of(self, name):
        """Gradient of a parameter in torch layout (host copy), for tests and checkpoint tools."""
        p = self.params[name]
        return from_arena(p, self.grad_arena[p.offset:p.offset + p.numel].cpu())

    def refresh_shadow(self):
        """Re-derive the bf16 filters (and their transposes) from the fp32 master parameters."""
        hip.check(self.lib.icamd_f32_to_bf16(self.param_arena.data_ptr(), self.shadow.data_ptr(), self.n_params,
                                             hip.stream_ptr()), "f32_to_bf16")
        self.refresh_transposed()

    def refresh_transposed(self):
        """What follows every change of the parameters (load, optimizer step): the transposed bf16 filters."""
        s = hip.stream_ptr()
        if self._tr_ntjobs:
            hip.check(self.lib.icamd_filter_transpose_tiled(self.shadow.data_ptr(), self.shadow_t.data_ptr(),
                                                            self._tr_descs.data_ptr(), self._tr_tjobs.data_ptr(),
                                                            self._tr_ntjobs, s), "filter_transpose_tiled")
        if self._tr_njobs:
            hip.check(self.lib.icamd_filter_transpose(self.shadow.data_ptr(), self.shadow_t.data_ptr(),
                                                      self._tr_descs.data_ptr(), self._tr_jobs.data_ptr(), self._tr_njobs, s),
                      "filter_transpose")

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    # ------------------------------------------------------------------ pointers
    def _pf(self, p):  # fp32 parameter
        return self.param_arena.data_ptr() + 4 * p.offset

    def _gf(self, p):  # fp32 gradient
        return self.grad_arena.data_ptr() + 4 * p.offset

    def _w(self, layer):  # bf16 filter
        return self.shadow.data_ptr() + 2 * layer.w.offset

    def _wt(self, layer):  # transposed bf16 filter
        return self.shadow_t.data_ptr() + 2 * layer.wt_offset

    # ------------------------------------------------------------------ input / forward
    def _pack_input(self, ws, x_nchw, mix, rgb4=False):
        """fp32 NCHW device tensor -> ws["x8"]: NHWC bf16 with the channels zero-padded to 8 (rgb4: the 7x7 stem's
        [N][H][W + 8][4] layout), with optional mixup / cutmix `mix` = (mode, lambda, box)."""
        N, C, H, W = x_nchw.shape
        mode, lam, box = (0, 1.0, (0, 0, 0, 0)) if mix is None else mix
        fn = self.lib.icamd_pack_input_rgb4 if rgb4 else self.lib.icamd_pack_input
        hip.check(fn(x_nchw.data_ptr(), ws["x8"].data_ptr(), N, C, H, W, mode, float(lam), int(box[0]), int(box[1]), int(box[2]),
                     int(box[3]), hip.stream_ptr()), "pack")
        return ws

    def __call__(self, x_nchw):
        """bf16 logits [B, num_classes] (a view of the workspace)."""
        ws = self.pack(x_nchw.to(self.device, dtype=torch.float32).contiguous())
        return self.forward_packed(ws)[:, : self.num_classes]

    def _draw_keep(self, ws, rates, batch):
        """Stochastic depth (timm drop_path: per sample, keep / keep_prob): one mask row per entry of `rates` for this step, drawn
        in ONE host call and uploaded ONCE from pinned memory without blocking, so the host keeps running ahead of the device.
        Returns the device tensor [len(rates)][batch], or None (and draws nothing) when no rate is above 0.

        The staging memory is a ring of 4 pinned rows: the upload of step i is enqueued behind step i's first kernels, so waiting
        for it before the NEXT draw (one buffer) tied the host to within one step of the device (12 ms of the host's step spent in
        Event.synchronize); with four rows the wait is for the upload issued 4 steps ago."""
        if not any(r > 0.0 for r in rates):
            return None
        kp = 1.0 - torch.tensor(rates, dtype=torch.float32).view(-1, 1)
        ring = ws.get("keep_host")
        if ring is None:
            ring = ws["keep_host"] = torch.empty(4, len(rates), batch, dtype=torch.float32).pin_memory()
            ws["keep_dev"] = torch.empty(len(rates), batch, dtype=torch.float32, device=self.device)
            ws["keep_copied"] = [None] * 4
            ws["keep_slot"] = 0
        slot = ws["keep_slot"]
        ws["keep_slot"] = (slot + 1) % 4
        host = ring[slot]
        if ws["keep_copied"][slot] is not None:
            ws["keep_copied"][slot].synchronize()   # the upload that last used this row has left it
        torch.div((torch.rand(len(rates), batch) < kp).float(), kp, out=host)
        ws["keep_dev"].copy_(host, non_blocking=True)
        ws["keep_copied"][slot] = torch.cuda.Event()
        ws["keep_copied"][slot].record()
        return ws["keep_dev"]
