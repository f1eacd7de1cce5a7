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


def negligible_gradients(ref, x, y, smoothing, arch="mobilenetv2_test"):
    """Names of the BatchNorm parameters whose TRUE gradient (fp64, no rounding points) is below 1e-3 of the gradient of the
    convolution in front of them: the bias of a BatchNorm without activation in front of a convolution + BatchNorm (exactly zero: the
    next batch mean removes a per-channel shift) and, while no channel clamps at 6 and the bias is 0, the weight of a BatchNorm in
    front of ReLU6 + depthwise convolution + BatchNorm (zero but for eps: the per-channel gain is normalised away).  bf16 cannot
    resolve them: what any bf16 run computes there is rounding residue."""
    exact = MobileNetV2Ref(arch, ref.classifier.out_features, bf16_points=False).double()
    exact.load_state_dict(ref.state_dict())
    exact.train()
    F.cross_entropy(exact(x.double()), y, label_smoothing=smoothing).backward()
    out, conv = {}, None
    for n, p in exact.named_parameters():
        if p.dim() == 4:
            conv = n
        elif p.dim() == 1 and conv is not None and float(p.grad.norm()) <= 1e-3 * float(dict(exact.named_parameters())[conv].grad.norm()):
            out[n] = conv
    return out
