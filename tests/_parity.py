"""What the whole-network parity tests of every family share: the loss + backward call, one training step of a CPU oracle beside
its fp64 twin, the same step on the HIP kernels, the comparison of the two, one perturbed (oracle, HIP model) pair per family, and the teacher-forcing protocol.
The oracle's own re-association noise (fp64 against fp32 accumulation, same rounding points) is the yardstick of every bound.
Importing this module needs no GPU."""
import copy
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from oracle.mobilenet_ref import MobileNetV2Ref, Tape, perturb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def xent_backward(net, ws, targets, num_classes, smoothing=0.0):
    """label-smoothed loss of the packed logits (mean over the batch), then the backward pass; -> the loss"""
    from imageclassification_amd import hip
    lib = net.lib
    B = targets.shape[0]
    hip.check(lib.icamd_softmax_xent(ws["logits"].data_ptr(), net.ncls_p, B, num_classes, targets.data_ptr(), None, 1.0,
                                     smoothing, 1.0 / B, ws["loss_rows"].data_ptr(), ws["pred"].data_ptr(),
                                     ws["dlogits"].data_ptr(), hip.stream_ptr()), "xent")
    net.backward_packed(ws)
    torch.cuda.synchronize()
    return float(ws["loss_rows"].mean())


# ---------------------------------------------------------------------------------------------------------------- the step
# out / out64: logits of the reference and of its fp64 twin (as fp32); the gradients stay on ref / ref64
Oracle = namedtuple("Oracle", "ref ref64 out out64 loss")
# rows: (name, HIP error, yardstick noise) per parameter, in named_parameters order
Step = namedtuple("Step", "ws err noise hip_loss loss rows")


def oracle_step(ref, x, y, smoothing=0.1):
    """The reference and its fp64 twin take one forward + backward on the CPU.  The twin is a deep copy: stochastic-depth masks
    injected into the reference before the call are the twin's too."""
    ref64 = copy.deepcopy(ref).double()
    out = ref(x)
    loss = F.cross_entropy(out, y, label_smoothing=smoothing)
    loss.backward()
    out64 = ref64(x.double())
    F.cross_entropy(out64, y, label_smoothing=smoothing).backward()
    return Oracle(ref, ref64, out.detach(), out64.detach().float(), float(loss.detach()))


def hip_step(net, x, y, num_classes, smoothing=0.1):
    """The HIP path on the same batch; -> (workspace, logits on the host as fp32, loss)"""
    net.train()
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    hip_loss = xent_backward(net, ws, y.cuda(), num_classes, smoothing)
    return ws, logits[:, :num_classes].float().cpu(), hip_loss


def compare(oracle, net, ws, logits, hip_loss):
    p64 = dict(oracle.ref64.named_parameters())
    rows = [(name, R.rel_l2(net.grad_of(name), p.grad), R.rel_l2(p64[name].grad.float(), p.grad))
            for name, p in oracle.ref.named_parameters()]
    return Step(ws, R.rel_l2(logits, oracle.out), R.rel_l2(oracle.out64, oracle.out), hip_loss, oracle.loss, rows)


def step(ref, net, x, y, num_classes, smoothing=0.1):
    oracle = oracle_step(ref, x, y, smoothing)
    return compare(oracle, net, *hip_step(net, x, y, num_classes, smoothing))


def worst(rows):
    """the first row with the largest HIP error"""
    return max(rows, key=lambda r: r[1])


def assert_within(s, logits_cap=(2.0, 2e-3), loss_cap=5e-3, grad_cap=(3.0, 1e-2)):
    """logits <= 2 max(noise, 2e-3), loss to 5e-3 relative, every gradient <= 3 max(its noise, 1e-2)"""
    assert s.err <= logits_cap[0] * max(s.noise, logits_cap[1]), (s.err, s.noise)
    assert abs(s.hip_loss - s.loss) <= loss_cap * s.loss, (s.hip_loss, s.loss)
    for name, e, n in s.rows:
        assert e <= grad_cap[0] * max(n, grad_cap[1]), (name, e, n)


def check(tag, ref, net, x, y, num_classes, smoothing=0.1, **caps):
    s = step(ref, net, x, y, num_classes, smoothing)
    w = worst(s.rows)
    print(f"{tag}: logits err {s.err:.2e} (self-noise {s.noise:.2e}); loss {s.hip_loss:.5f} vs {s.loss:.5f}; "
          f"worst grad err {w[1]:.2e} (yardstick {w[2]:.2e}) at {w[0]}")
    assert_within(s, **caps)
    return s


# ---------------------------------------------------------------------------------------------------------------- the pairs
def _perturb(ref, seed, rule):
    """rule(name, parameter, generator) rewrites a parameter in place or leaves it; one generator, named_parameters order"""
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            rule(n, p, g)
    return g


def _convnext_rule(n, p, g):
    if ".mlp.grn.weight" in n:
        p.copy_(0.5 * torch.randn(p.shape, generator=g))             # GRN away from its zero init
    elif n.endswith("bias"):
        p.copy_(0.1 * torch.randn(p.shape, generator=g))             # (mlp.grn.bias among them)
    elif n.endswith("gamma"):
        p.copy_(0.3 + 0.4 * torch.rand(p.shape, generator=g))        # layer scale far from its 1e-6 init
    elif "norm" in n or n.startswith("stem.1") or "downsample.0" in n:
        p.copy_(0.5 + torch.rand(p.shape, generator=g))
    elif n.endswith("weight"):
        p.mul_(4.0)                                                  # std 0.08: activations of O(1)


def _transformer_rule(n, p, g):
    """non-trivial biases, LayerNorm affine and (Swin) bias tables, so that every gradient path is exercised"""
    if n.endswith("relative_position_bias_table"):
        p.copy_(0.5 * torch.randn(p.shape, generator=g))
    elif n.endswith("bias"):
        p.copy_(0.1 * torch.randn(p.shape, generator=g))
    elif "norm" in n and n.endswith("weight"):
        p.copy_(0.5 + torch.rand(p.shape, generator=g))


def convnext_ref(arch, C, seed=0, cfg=None):
    """The ConvNeXt oracle (V2 by the name) with the rounding points, perturbed.  `cfg`: the (depths, dims) of a name the oracle's
    table does not list."""
    from oracle.convnext_ref import ConvNeXtRef
    torch.manual_seed(seed)
    ref = ConvNeXtRef(cfg or arch, C, bf16_points=True, v2=arch.startswith("convnextv2_"))
    _perturb(ref, seed, _convnext_rule)
    return ref


def convnext_pair(arch, C, seed=0, drop_path=0.0, cfg=None):
    from imageclassification_amd.convnext import ConvNeXt
    ref = convnext_ref(arch, C, seed, cfg)
    net = ConvNeXt(arch, C, drop_path_rate=drop_path)
    net.load_state_dict(ref.state_dict())
    return ref, net


def vit_pair(arch, C, img, seed=0):
    from imageclassification_amd.vit import VisionTransformer
    from oracle.vit_ref import ViTRef
    torch.manual_seed(seed)
    ref = ViTRef(arch, C, img_size=img, bf16_points=True)
    g = _perturb(ref, seed, _transformer_rule)
    with torch.no_grad():
        ref.cls_token.copy_(0.02 * torch.randn(ref.cls_token.shape, generator=g))
    net = VisionTransformer(arch, C, img_size=img)
    net.load_state_dict(ref.state_dict())
    return ref, net


def swin_ref(arch, C, img, seed=0):
    from oracle.swin_ref import SwinRef
    torch.manual_seed(seed)
    ref = SwinRef(arch, C, img_size=img, bf16_points=True)
    _perturb(ref, seed, _transformer_rule)
    return ref


def swin_pair(arch, C, img, seed=0, drop_path_rate=0.0):
    from imageclassification_amd.swin import SwinTransformer
    ref = swin_ref(arch, C, img, seed)
    net = SwinTransformer(arch, C, img_size=img, drop_path_rate=drop_path_rate)
    net.load_state_dict(ref.state_dict())
    return ref, net


def efficientnet_pair(arch, C, perturbed, seed=0):
    """timm's default init, or (perturbed) oracle/efficientnet_ref.py::perturb: BatchNorm affine, running statistics and SE biases"""
    from imageclassification_amd.efficientnet import EfficientNet
    from oracle import efficientnet_ref as E
    torch.manual_seed(seed)
    ref = E.EfficientNetRef(arch, C, bf16_points=True)
    if perturbed:
        E.perturb(ref, seed + 1)
    net = EfficientNet(arch, C)
    net.load_state_dict(ref.state_dict())
    return ref, net


def mobilenet_pair(arch, C, perturbed, seed=0):
    """timm's default init, or (perturbed) BatchNorm affine and running statistics at which ReLU6 clamps at both ends"""
    from imageclassification_amd.mobilenet import MobileNetV2
    torch.manual_seed(seed)
    ref = MobileNetV2Ref(arch, C, bf16_points=True)
    if perturbed:
        perturb(ref, seed + 1)
    net = MobileNetV2(arch, C)
    net.load_state_dict(ref.state_dict())
    return ref, net


# ---------------------------------------------------------------------------------------------------------------- ConvNeXt cases
def convnext_case(arch, C, B, HW, cfg=None):
    """One oracle evaluation of a perturbed ConvNeXt under injected stochastic-depth masks (training pass with its fp64 twin, then
    the eval pass without masks), and the HIP model loaded from it.  Meant for a module-scoped fixture: nothing is modified later."""
    ref, net = convnext_pair(arch, C, drop_path=0.2, cfg=cfg)
    g = torch.Generator().manual_seed(5)
    keeps = [((torch.rand(B, generator=g) < 0.8).float() / 0.8) for _ in ref.all_blocks()]
    keeps[0] = None                                           # first block: rate 0
    for blk, k in zip(ref.all_blocks(), keeps):
        blk.keep = k
    x = torch.randn(B, 3, HW, HW, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    oracle = oracle_step(ref, x, y)
    for blk in ref.all_blocks() + oracle.ref64.all_blocks():  # eval: no masks
        blk.keep = None
    with torch.no_grad():
        ev, ev64 = ref(x), oracle.ref64(x.double())
    return {"arch": arch, "C": C, "oracle": oracle, "net": net, "keeps": keeps, "x": x, "y": y, "eval": ev, "eval64": ev64}


def convnext_case_step(case):
    """the HIP side of convnext_case under the same masks, compared"""
    net, B = case["net"], case["x"].shape[0]
    net.injected_keep = [torch.ones(B) if k is None else k for k in case["keeps"]]
    return compare(case["oracle"], net, *hip_step(net, case["x"], case["y"], case["C"]))


def convnext_case_eval(case):
    """eval-mode logits of the HIP model against the oracle's eval pass; -> (error, self-noise)"""
    net = case["net"]
    net.eval()
    got = net(case["x"].cuda()).float().cpu()
    torch.cuda.synchronize()
    net.train()
    return R.rel_l2(got, case["eval"]), R.rel_l2(case["eval64"].float(), case["eval"])


# ---------------------------------------------------------------------------------------------------------------- teacher forcing
# The whole-model gradient check that bf16 drift cannot blur, for an oracle with set_tape (oracle/mobilenet_ref.py::Tape)
def forced_gradients(ref, values, x, y, smoothing):
    """{name: gradient} of a copy of `ref` whose stored tensors are `values` (Tape order, NCHW, on the bf16 grid), and its loss"""
    m = copy.deepcopy(ref)
    for p in m.parameters():
        p.grad = None
    m.train()
    tape = Tape(values)
    m.set_tape(tape)
    loss = F.cross_entropy(m(x), y, label_smoothing=smoothing)
    loss.backward()
    assert tape.i == len(tape.values)
    return {n: p.grad for n, p in m.named_parameters()}, float(loss.detach())


def recorded_step(model, x, y, smoothing):
    """one training forward + backward of `model` (any dtype) with its stored tensors recorded: (values as fp32, {name: gradient})"""
    for p in model.parameters():
        p.grad = None
    model.train()
    tape = Tape()
    model.set_tape(tape)
    F.cross_entropy(model(x.to(next(model.parameters()).dtype)), y, label_smoothing=smoothing).backward()
    model.set_tape(None)
    return [v.float() for v in tape.rec], {n: p.grad for n, p in model.named_parameters()}


def negligible_gradients(exact, ref, x, y, smoothing, skip=()):
    """Names of the BatchNorm parameters whose TRUE gradient is below 1e-3 of the gradient of the convolution in front of them.
    `exact`: the caller's fp64 model of `ref`'s architecture without rounding points (it takes ref's weights here); a name that holds
    one of `skip` is neither such a convolution nor such a parameter (EfficientNet: ".se.").  They are the bias of a BatchNorm
    without activation in front of a convolution + BatchNorm (exactly zero: the next batch mean removes a per-channel shift) and,
    for MobileNetV2 while no channel clamps at 6 and the bias is 0, the weight of a BatchNorm in front of ReLU6 + depthwise
    convolution + BatchNorm (zero but for eps: the per-channel gain is normalised away).  bf16 cannot resolve them: what any bf16 run
    computes there is rounding residue."""
    exact.load_state_dict(ref.state_dict())
    exact.train()
    F.cross_entropy(exact(x.double()), y, label_smoothing=smoothing).backward()
    out, conv, params = {}, None, dict(exact.named_parameters())
    for n, p in params.items():
        if any(k in n for k in skip):
            continue
        if p.dim() == 4:
            conv = n
        elif p.dim() == 1 and conv is not None and float(p.grad.norm()) <= 1e-3 * float(params[conv].grad.norm()):
            out[n] = conv
    return out


def hip_stored_tensors(net, ws):
    """the stored tensors of the MobileNetV2 or EfficientNet step just run on the HIP path, in Tape order, NCHW fp32 on the host"""
    nchw = lambda t: t.float().cpu().permute(0, 3, 1, 2).contiguous()     # noqa: E731
    out = [nchw(ws["x8"][..., :3]), nchw(ws["y0"])]
    for blk, b in zip(net.blocks, ws["blocks"]):
        out += ([nchw(b["y1"])] if blk.kind == "ir" else []) + [nchw(b[k]) for k in ("y2", "a2", "y3", "out")]
    return out + [nchw(ws["yh"]), nchw(ws["ah"]), ws["pooled"].float().cpu(), ws["logits"][:, :net.num_classes].float().cpu()]


def forced_check(ref, net, exact, x, y, smoothing, negligible, n_params, skip=()):
    """Gradients of the MobileNetV2 or EfficientNet HIP step just run (its workspace still holds it) against the reference forced onto
    the HIP path's stored tensors.  Caps on the yardstick (reference forced onto its fp64 copy's tensors, against that copy's
    gradients): mean 8e-3 -- the tightest cap a family of this project puts on its yardstick (tests/test_resnet_family_gpu.py) --,
    worst 2.5e-2, three relative bf16 steps (2^-7): with masks and statistics pinned, what is left is the rounding of the stored
    gradient tensors (tests/test_efficientnet_gpu.py says what these caps ask of its reference pair).  The HIP path gets the
    per-tensor and mean rules of tests/_resnet_parity.py::assert_hip_within_yardstick on these rows.  The parameters whose true
    gradient is zero (negligible_gradients with `exact` and `skip`) are `negligible` -- their number, or the sorted list of their
    names --, are taken out of the rows and held on their own: on every side at most 1e-2 of the gradient of the convolution in front
    of them (rounding residue: a few bf16 steps of that gradient's terms).  The reference has n_params parameters and 35 stored
    tensors."""
    ws = net._workspace(x.shape[0], x.shape[2], x.shape[3])
    hip_vals = hip_stored_tensors(net, ws)
    zero = negligible_gradients(exact, ref, x, y, smoothing, skip)
    assert (len(zero) if isinstance(negligible, int) else sorted(zero)) == negligible, sorted(zero)
    twin = copy.deepcopy(ref).double()
    vals64, g64 = recorded_step(twin, x, y, smoothing)
    assert [tuple(v.shape) for v in vals64] == [tuple(v.shape) for v in hip_vals] and len(hip_vals) == 35
    gn, _ = forced_gradients(ref, vals64, x, y, smoothing)                 # the yardstick: forced onto the fp64 copy
    gh, loss = forced_gradients(ref, hip_vals, x, y, smoothing)           # forced onto the HIP path
    names = [n for n, _ in ref.named_parameters()]
    rows = [(n, R.rel_l2(net.grad_of(n), gh[n]), R.rel_l2(g64[n].float(), gn[n])) for n in names if n not in zero]
    assert len(rows) == len(names) - len(zero) == n_params - len(zero)
    mean_err, mean_noise = sum(r[1] for r in rows) / len(rows), sum(r[2] for r in rows) / len(rows)
    worst, worst_noise = max(rows, key=lambda r: r[1]), max(rows, key=lambda r: r[2])
    print(f"forced: {len(rows)} tensors, yardstick mean {mean_noise:.2e} worst {worst_noise[2]:.2e} at {worst_noise[0]}; HIP mean "
          f"{mean_err:.2e} worst {worst[1]:.2e} (noise {worst[2]:.2e}) at {worst[0]}; loss {loss:.5f}")
    for n, e, z in sorted(rows, key=lambda r: r[1] / max(r[2], 5e-3), reverse=True)[:8]:
        print(f"    {n}: HIP {e:.2e}, noise {z:.2e}")
    assert mean_noise <= 8e-3 and worst_noise[2] <= 2.5e-2
    assert mean_err <= 2.0 * max(mean_noise, 1e-3)
    for n, e, z in rows:
        assert e <= 3.0 * max(z, 5e-3), (n, e, z)
    for n, conv in zero.items():
        for side, g, gc in (("HIP", net.grad_of(n), net.grad_of(conv)), ("reference", gh[n], gh[conv]), ("fp64 copy", g64[n], g64[conv])):
            ratio = float(torch.linalg.vector_norm(g.double()) / torch.linalg.vector_norm(gc.double()))
            assert ratio <= 1e-2, (n, side, ratio)
