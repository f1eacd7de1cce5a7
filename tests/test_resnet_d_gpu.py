"""The ResNet-D variants on the GPU: whole-network parity of resnet50d, resnet18d and seresnext26d_32x4d against the oracle
(oracle/resnet_ref.py) by the protocol of tests/test_resnet_family_gpu.py; the deep stem and the pooled shortcut
checked op by op on the HIP path's own tensors; the ICAMD_STEM_THIN routes against each other; one finite step of the two
largest members; eval, state_dict, engine, command line and reproducibility for resnet50d."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _resnet_parity import (assert_hip_within_yardstick, hip_rows, parity_batch, perturbed_bn_pair, set_last_gamma,  # noqa: E402
                            timm_default_pair, xent_backward, yardstick)
from oracle.resnet_ref import ResNetRef  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
F64 = torch.float64


# arch, tensors with a gradient
PARITY = [("resnet50d", 167), ("resnet18d", 68), ("seresnext26d_32x4d", 127)]


@pytest.mark.parametrize("arch,ntensors", PARITY)
def test_whole_network_parity_well_conditioned(arch, ntensors):
    """Batch 32 at 128 x 128, 100 classes, label smoothing 0.1, timm-default init, the last BatchNorm weight of every block at
    0.02 (every tensor compared).  The yardstick -- the reference against its own fp64 copy -- is asserted first under the caps
    of tests/test_resnet_family_gpu.py (8e-3, 0.13, 0.22; measured on a CPU: resnet50d logits 5.3e-3 / mean 0.111 / worst 0.182,
    resnet18d 4.4e-3 / 0.072 / 0.174, seresnext26d_32x4d 4.9e-3 / 0.085 / 0.161).  Then the HIP path: logits <= 2 max(noise,
    1e-3), loss to 1e-3, mean gradient error <= 2 max(mean noise, 1e-3), per tensor <= 3 max(its noise, 5e-3)."""
    C, B, HW = 100, 32, 128
    ref, net = timm_default_pair(arch, C, gamma_last=0.02)
    x, y = parity_batch(C, B, HW)
    yard = yardstick(ref, x, y, 0.1)
    for name, grad in yard.grads.items():
        assert float(grad.abs().max()) > 0.0, name
    got = hip_rows(net, x, y, C, 0.1, yard)
    rows, worst = got.rows, got.worst
    print(f"{arch} B={B} {HW}x{HW}: logits err {got.err_logits:.2e} (self-noise {yard.noise_logits:.2e}); loss {got.loss:.6f} vs "
          f"{yard.loss:.6f}; {len(rows)} gradient tensors: mean err {got.mean_err:.2e} (self-noise {yard.mean_noise:.2e}), worst "
          f"{worst[0]} {worst[1]:.2e} (its self-noise {worst[2]:.2e}), yardstick worst {yard.worst_noise[1]:.2e}")
    for name, e, n in rows:
        if name.startswith(("conv1.", "bn1.")) or "downsample" in name:
            print(f"    {name:32s} HIP {e:.2e} yardstick {n:.2e}")
    # the yardstick itself
    assert yard.noise_logits <= 8e-3 and yard.mean_noise <= 0.13 and yard.worst_noise[1] <= 0.22, \
        (yard.noise_logits, yard.mean_noise)
    assert len(rows) == ntensors
    # the HIP path against it
    assert_hip_within_yardstick(yard, got)


# ------------------------------------------------------------------------------------------------ teacher-forced stem and shortcut
def _cpu(t):
    return t.float().cpu()


def _close_bf16(got, ref, what):
    e = R.rel_l2(got, ref)
    print(f"    {what}: rel_l2 {e:.2e}")
    assert torch.isfinite(got).all(), what
    assert e <= 1e-3, (what, e)
    assert R.bf16_close(got, ref), what


@pytest.mark.parametrize("HW", [72, 64])
def test_stem_and_pooled_shortcut_op_by_op(HW):
    """resnet26d, batch 4: every stem op and the pooled shortcut inputs of layer2.0 / layer3.0, each against its reference applied
    to the HIP path's OWN input of that op (and, backward, its own upstream gradient), under the kernel bounds of
    tests/test_resnet_d_kernels_gpu.py and tests/test_kernels_gpu.py (BatchNorm backward: dy as a bf16 output, dgamma / dbeta
    rel_l2 <= 1e-4).  72 x 72 gives odd sizes downstream (36 -> 18 -> 9 -> 5 -> 3)."""
    from imageclassification_amd.nets import ResNet
    C, B = 10, 4
    net = ResNet("resnet26d", C, seed=3, zero_init_last=False)
    sd = net.state_dict()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 3, HW, HW, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    net.train()
    ws = net.pack(x.cuda())
    net.forward_packed(ws)
    # The backward of a pooled block leaves the shortcut's data gradient on the pooled grid in scratch buffer 2 (run.T), the main
    # branch's data gradient in buffer 3 (run.DA) and the finished block-input gradient in buffer 0 or 1 (they alternate from the
    # last block down).  The gradient-ready hook fires right after the block: copy the three before the next block reuses them.
    names = [blk["name"] for blk in net.blocks]
    watch = {net.blocks[names.index(n)]["convs"][0].w.offset: names.index(n) for n in ("layer2.0", "layer3.0")}
    seen = {}

    def hook(lo, hi, events):
        if lo in watch and hi is None:
            bi = watch[lo]
            torch.cuda.synchronize()
            gb = ws["gbuf"]
            other = gb[1] if (len(net.blocks) - 1 - bi) % 2 == 0 else gb[0]
            seen[bi] = (gb[2].clone(), gb[3].clone(), other.clone())

    net.grad_ready_hook = hook
    xent_backward(net, ws, y.cuda(), C, smoothing=0.1)
    net.grad_ready_hook = None

    def stats_of(bn):
        st = net.stat_arena[bn.stat_offset:bn.stat_offset + 4 * bn.c].cpu()
        return st[:bn.c], st[bn.c:2 * bn.c], st[2 * bn.c:3 * bn.c], st[3 * bn.c:]

    def filt(conv):
        p = conv.w
        return net.shadow[p.offset:p.offset + p.numel].float().cpu().reshape(p.padded_shape)

    assert len(ws["stem_in"]) == 3 and len(ws["stem_y"]) == 3 and len(ws["stem_a"]) == 2
    assert ws["stem_in"][0] is ws["x8"] and ws["stem_y"][2] is ws["y0"]
    for i, (conv, bn) in enumerate(net.stem_pairs):
        xin, yy = _cpu(ws["stem_in"][i]), _cpu(ws["stem_y"][i])
        print(f"  {conv.name} {tuple(xin.shape)} -> {tuple(yy.shape)}")
        _close_bf16(yy, R.conv2d_fwd(xin, filt(conv), conv.stride, conv.pad, acc=F64).float(), conv.name + " fwd")
        mean, invstd, scale, shift = stats_of(bn)
        rmean, rinv, rscale, rshift, rrm, rrv = R.bn_train_coeffs(yy, sd[bn.name + ".weight"], sd[bn.name + ".bias"],
                                                                  torch.zeros(bn.c), torch.ones(bn.c), 0.1, 1e-5)
        for name, a, b, rtol, atol in (("mean", mean, rmean, 1e-5, 1e-6), ("invstd", invstd, rinv, 1e-5, 0.0),
                                       ("scale", scale, rscale, 1e-5, 0.0), ("shift", shift, rshift, 1e-4, 1e-6)):
            assert torch.allclose(a, b, rtol=rtol, atol=atol), (bn.name, name)
        if i < 2:
            want = R.bn_apply(yy, scale, shift, None, relu=True, acc=F64).float()
            _close_bf16(_cpu(ws["stem_a"][i]), want, bn.name + " apply")
    # bn1 + ReLU + max-pool on the third convolution's output
    mean, invstd, scale, shift = stats_of(net.stem_bn)
    a0 = R.bn_apply(_cpu(ws["y0"]), scale, shift, None, relu=True, acc=F64).float()
    assert torch.equal(_cpu(ws["p0"]), R.maxpool3x3s2_fwd(a0)[0])
    # pooled shortcut inputs
    for name in ("layer2.0", "layer3.0"):
        bi = [b["name"] for b in net.blocks].index(name)
        b = ws["blocks"][bi]
        xin = _cpu(b["in"]).double().permute(0, 3, 1, 2)
        want = F.avg_pool2d(xin, 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
        ulp = R.max_bf16_ulp(_cpu(b["xp"]), R.bf16_round(want.float()))
        print(f"  {name} pooled shortcut input {tuple(b['xp'].shape)}: max ulp {ulp}")
        assert ulp <= 1.0
    assert "xp" not in ws["blocks"][0]
    # ... and their backward in place: block-input gradient = main branch's data gradient + the pooled-grid gradient spread over
    # the 1, 2 or 4 pixels of each window, one rounding (odd sizes at 72 x 72: 9 -> 5 at layer3.0)
    assert sorted(seen) == sorted(watch.values())
    for bi, (T, DA, other) in seen.items():
        b = ws["blocks"][bi]
        xin, xp = b["in"], b["xp"]
        t = T[:xp.numel()].view(xp.shape).float().cpu().double().permute(0, 3, 1, 2)
        da = DA[:xin.numel()].view(xin.shape).float().cpu().double()
        got = other[:xin.numel()].view(xin.shape).float().cpu()
        probe = torch.zeros(xin.shape[0], xin.shape[3], xin.shape[1], xin.shape[2], dtype=F64, requires_grad=True)
        F.avg_pool2d(probe, 2, 2, ceil_mode=True, count_include_pad=False).backward(t)
        want = R.bf16_round((probe.grad.permute(0, 2, 3, 1) + da).float())
        ulp = R.max_bf16_ulp(got, want)
        print(f"  {names[bi]} block-input gradient {tuple(xin.shape)} from pooled {tuple(xp.shape)}: max ulp {ulp}")
        assert torch.isfinite(got).all() and ulp <= 1.0
    # backward, last stem op to first, each on the HIP path's own upstream gradient
    dy = [_cpu(t) for t in ws["stem_dy"]]
    dx = [None if t is None else _cpu(t) for t in ws["stem_dx"]]
    for i in (2, 1, 0):
        conv, bn = net.stem_pairs[i]
        xin = _cpu(ws["stem_in"][i])
        want_dw = R.conv2d_wgrad(xin, dy[i], (3, 3), conv.stride, conv.pad, acc=F64)
        got_dw = net.grad_of(conv.name + ".weight").permute(0, 2, 3, 1).double()
        e = R.rel_l2(got_dw, want_dw[..., :conv.cin])
        print(f"    {conv.name} wgrad: rel_l2 {e:.2e}")
        assert e <= 1e-4, (conv.name, e)
        if i == 0:
            break
        hw = (xin.shape[1], xin.shape[2])
        _close_bf16(dx[i], R.conv2d_dgrad(dy[i], filt(conv), hw, 1, 1, acc=F64).float(), conv.name + " dgrad")
        pbn = net.stem_pairs[i - 1][1]
        mean, invstd, scale, shift = stats_of(pbn)
        yy = _cpu(ws["stem_y"][i - 1])
        act = R.bn_apply(yy, scale, shift, None, relu=True, acc=F64).float()
        rdy, rdg, rdb, _ = R.bn_bwd(dx[i], act, yy, mean, invstd, scale, True)
        _close_bf16(dy[i - 1], rdy, pbn.name + " bwd")
        assert R.rel_l2(net.grad_of(pbn.name + ".weight"), rdg) <= 1e-4 and R.rel_l2(net.grad_of(pbn.name + ".bias"), rdb) <= 1e-4


# ------------------------------------------------------------------------------------------------ routes
_ROUTE_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import torch
import test_resnet_d_gpu as T
from imageclassification_amd.nets import ResNet
C, B, HW = 10, 8, 64
net = ResNet("resnet50d", C, seed=11, zero_init_last=False)
g = torch.Generator().manual_seed(12)
x = torch.randn(B, 3, HW, HW, generator=g)
y = torch.randint(0, C, (B,), generator=g)
runs = []
start = net.state_dict()
for _ in range(%(repeat)d):
    net.load_state_dict(start)
    net.train()
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    loss = T.xent_backward(net, ws, y.cuda(), C, smoothing=0.1)
    runs.append((logits[:, :C].float().cpu().clone(), net.grad_arena.cpu().clone()))
assert all(torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) for r in runs), "not bitwise repeatable"
grads = {name: net.grad_of(name) for name in net.params}
torch.save({"logits": runs[0][0], "grads": grads}, %(out)r)
print("child-ok")
"""


def _route(tmp_path, mode, repeat=1):
    out_file = str(tmp_path / f"route_{mode}.pt")
    code = _ROUTE_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "repeat": repeat, "out": out_file}
    env = dict(os.environ)
    env.pop("ICAMD_STEM_THIN", None)
    if mode != "default":
        env["ICAMD_STEM_THIN"] = mode
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "child-ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return torch.load(out_file, map_location="cpu", weights_only=False)


def test_stem_thin_routes_agree(tmp_path):
    """resnet50d, batch 8 at 64 x 64, one forward + backward per child process with ICAMD_STEM_THIN unset (twice: bitwise
    repeatable), 0 and 2: finite; logits of any two routes R.bf16_close; every gradient tensor rel_l2 <= 0.05, the bound of
    tests/test_resnet_routes_gpu.py between routes."""
    res = {"default": _route(tmp_path, "default", repeat=2)}      # nothing is started after a child that failed
    res["0"] = _route(tmp_path, "0")
    res["2"] = _route(tmp_path, "2")
    names = list(res)
    for r in res.values():
        assert torch.isfinite(r["logits"]).all()
        assert all(torch.isfinite(gr).all() for gr in r["grads"].values())
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            a, b = res[names[i]], res[names[j]]
            assert R.bf16_close(a["logits"], b["logits"]), (names[i], names[j])
            worst = max(((n, R.rel_l2(a["grads"][n], b["grads"][n])) for n in a["grads"]), key=lambda t: t[1])
            print(f"routes {names[i]} vs {names[j]}: worst gradient tensor {worst[0]} rel_l2 {worst[1]:.2e}")
            for n in a["grads"]:
                assert R.rel_l2(a["grads"][n], b["grads"][n]) <= 0.05, (names[i], names[j], n)


# ------------------------------------------------------------------------------------------------ the rest of the host side
@pytest.mark.parametrize("arch", ["resnet200d", "seresnet152d"])
def test_largest_members_take_one_finite_step(arch):
    from imageclassification_amd.nets import ResNet
    C, B, HW = 10, 4, 64
    net = ResNet(arch, C, seed=3, zero_init_last=False)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 3, HW, HW, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    net.train()
    ws = net.pack(x.cuda())
    logits = net.forward_packed(ws)
    loss = xent_backward(net, ws, y.cuda(), C, smoothing=0.1)
    assert torch.isfinite(logits[:, :C].float()).all() and loss == loss and abs(loss) < 1e3
    assert torch.isfinite(net.grad_arena).all()
    for name in ("conv1.0.weight", "conv1.3.weight", "conv1.6.weight", "layer2.0.downsample.1.weight", "layer3.20.conv2.weight",
                 "layer4.2.conv3.weight", "fc.weight"):
        assert float(net.grad_of(name).abs().max()) > 0.0, name


@pytest.mark.parametrize("HW", [64, 72])
def test_resnet50d_eval_folded_and_state_dict_round_trip(HW):
    """Folded and unfolded eval logits against the reference's fp32 arithmetic, <= 1e-2 each.  At batch 4 the bf16-points
    reference's own distance d from its fp32 arithmetic swings with the weight draw between 4e-3 and 1.0e-2 (measured on a CPU,
    seeds 4 .. 12).  The HIP paths round at other points or in another order, so their distance is a second sample of the same
    noise, up to sqrt(2) d for two independent errors of size d: the bound holds only where d <= 1e-2 / 1.5, asserted first as
    <= 6.5e-3 (as tests/test_seresnet_gpu.py).  Seed 10 (4.9e-3 at 64 x 64, 4.3e-3 at 72 x 72) is the first seed from 4 up that
    meets it at both sizes; seed 4 stopped meeting it (1.01e-2 at 64 x 64, the unfolded HIP path at 1.14e-2) when the oracle
    stopped constructing layers it threw away, which moved the seeded draw of every member but resnet18/34/50."""
    from imageclassification_amd.nets import ResNet
    C = 10
    ref, net, sd = perturbed_bn_pair("resnet50d", C, seed=10)
    x = torch.randn(4, 3, HW, HW, generator=torch.Generator().manual_seed(10))
    exact = ResNetRef("resnet50d", C, bf16_points=False, zero_init_last=False)   # the reference's fp32 arithmetic
    exact.load_state_dict(sd)
    exact.eval()
    net.eval()
    ref.eval()
    with torch.no_grad():
        want = exact(x)
        rounded = ref(x)
    print(f"resnet50d {HW}x{HW} eval: the bf16-points reference vs its fp32 arithmetic {R.rel_l2(rounded, want):.2e}")
    assert R.rel_l2(rounded, want) <= 6.5e-3          # the condition under which the bound below can be held
    assert net.fold_eval
    folded = net(x.cuda()).float().cpu()
    net.fold_eval = False
    unfolded = net(x.cuda()).float().cpu()
    net.fold_eval = True
    e_fold, e_plain = R.rel_l2(folded, want), R.rel_l2(unfolded, want)
    print(f"resnet50d {HW}x{HW} eval logits vs fp32 reference: folded {e_fold:.2e}, separate BatchNorm pass {e_plain:.2e}")
    assert e_fold <= 1e-2 and e_plain <= 1e-2
    # state_dict -> load_state_dict: bit-exact, key for key in the reference's order
    out = net.state_dict()
    assert list(out) == list(sd)
    assert tuple(out["conv1.0.weight"].shape) == (32, 3, 3, 3)
    assert tuple(out["layer2.0.downsample.1.weight"].shape) == (512, 256, 1, 1)
    for k in sd:
        assert torch.equal(out[k].float(), sd[k].float()), k
    net2 = ResNet("resnet50d", C, seed=99)
    net2.load_state_dict(out)
    assert torch.equal(net2.param_arena, net.param_arena) and torch.equal(net2.buffer_arena, net.buffer_arena)
    assert torch.equal(net2.shadow, net.shadow)


def test_resnet50d_eval_unfolded_by_environment(tmp_path):
    """ICAMD_EVAL_FOLD=0 is read by the constructor: a fresh process, the same bound."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch\n"
            "import test_resnet_d_gpu as T\n"
            "from oracle import ops_ref as R\n"
            "ref, net, sd = T.perturbed_bn_pair('resnet50d', 10, seed=4)\n"
            "assert not net.fold_eval\n"
            "x = torch.randn(4, 3, 72, 72, generator=torch.Generator().manual_seed(10))\n"
            "exact = T.ResNetRef('resnet50d', 10, bf16_points=False, zero_init_last=False)\n"
            "exact.load_state_dict(sd); exact.eval(); net.eval()\n"
            "with torch.no_grad():\n"
            "    want = exact(x)\n"
            "e = R.rel_l2(net(x.cuda()).float().cpu(), want)\n"
            "print('unfolded', e)\n"
            "assert e <= 1e-2\n"
            "print('child-ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ICAMD_EVAL_FOLD="0"), capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "child-ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_resnet50d_engine_step_evaluate_and_bitwise_repeat():
    """As tests/test_resnet_family_gpu.py::test_resnext50_engine_step_evaluate_and_bitwise_repeat: every block's last BatchNorm
    weight at 0.02, the yardstick (reference against its fp64 copy) asserted <= 1e-3 on the loss before the HIP path is held to
    the engine tests' 5e-3."""
    from imageclassification_amd.engine import evaluate, train_one_epoch
    from imageclassification_amd.mixup import LabelSmoothingCrossEntropy
    from imageclassification_amd.nets import ResNet
    from imageclassification_amd.optim_factory import create_optimizer
    from imageclassification_amd.utils import NativeScalerWithGradNormCount
    from oracle import engine_ref as E
    C, B = 10, 8
    torch.manual_seed(0)
    ref = ResNetRef("resnet50d", C, bf16_points=True, zero_init_last=False)
    set_last_gamma(ref, 0.02)
    net = ResNet("resnet50d", C)
    net.load_state_dict(ref.state_dict())
    start = copy.deepcopy(ref.state_dict())
    g = torch.Generator().manual_seed(21)
    data = [(torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, C, (B,), generator=g))]
    net.train()
    runs = []
    for _ in range(2):
        ws = net.pack(data[0][0].cuda())
        net.forward_packed(ws)
        loss = xent_backward(net, ws, data[0][1].cuda(), C, smoothing=0.1)
        runs.append((loss, net.grad_arena.clone(), ws["logits"].clone()))
        net.load_state_dict(ref.state_dict())      # running statistics back to the start
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().max()) > 0.0
    ref64 = copy.deepcopy(ref).double()
    ref.train(); ref64.train()
    with torch.no_grad():
        ref_loss = float(F.cross_entropy(ref(data[0][0]), data[0][1], label_smoothing=0.1))
        loss64 = float(F.cross_entropy(ref64(data[0][0].double()).float(), data[0][1], label_smoothing=0.1))
    ref.load_state_dict(start)
    print(f"resnet50d B={B} 64x64: loss HIP {runs[0][0]:.6f}, reference {ref_loss:.6f}, its fp64 copy {loss64:.6f}")
    assert abs(loss64 - ref_loss) <= 1e-3 * abs(ref_loss)          # the yardstick itself
    assert abs(runs[0][0] - ref_loss) <= 5e-3 * abs(ref_loss)
    opt = create_optimizer("adamw", 1e-6, 5e-4, net)
    stats = train_one_epoch(net, LabelSmoothingCrossEntropy(0.1), data, opt, DEV, 0, NativeScalerWithGradNormCount(), None, None,
                            None, start_steps=0, lr_schedule_values=[1e-6], wd_schedule_values=[5e-4],
                            num_training_steps_per_epoch=1, update_freq=1, use_amp=True, num_classes=C)
    assert abs(stats["loss"] - ref_loss) <= 5e-3 * abs(ref_loss)
    ref.eval()
    rev = E.evaluate_ref(data, ref, C)
    ev = evaluate(data, net, DEV, C)
    assert list(ev) == list(rev)
    assert all(v == v for v in ev.values())


def test_train_cli_resnet50d_synthetic_and_resume(tmp_path):
    work = tmp_path / "work"
    os.makedirs(work / "train_cls" / "output")
    base = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "resnet50d", "--input_size", "64", "--synthetic", "16",
            "--num_classes", "10", "--batch_size", "8", "--num_workers", "0", "--mixup", "0", "--warmup_epochs", "0", "--lr", "1e-4",
            "--use_amp", "true"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(base + ["--epochs", "1"], cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    from imageclassification_amd.checkpoint import DeferredModel
    ck = torch.load(work / "train_cls" / "output" / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    model = ck["model"]
    assert isinstance(model, DeferredModel) and model.arch == "resnet50d"
    sd = model.state_dict()
    assert tuple(sd["conv1.3.weight"].shape) == (32, 32, 3, 3) and "conv1.4.running_var" in sd
    assert tuple(sd["layer2.0.downsample.1.weight"].shape) == (512, 256, 1, 1)
    out2 = subprocess.run(base + ["--epochs", "2"], cwd=work, env=env, capture_output=True, text=True, timeout=900)
    assert out2.returncode == 0, out2.stdout[-3000:] + out2.stderr[-3000:]
    assert os.path.exists(work / "train_cls" / "output" / "checkpoint-1.pth")
    assert "checkpoint-0" in out2.stdout + out2.stderr
    import json
    lines = [json.loads(l) for l in open(work / "train_cls" / "log.txt")]
    assert [l["epoch"] for l in lines] == [0, 1]
