"""What the ResNet-family parity tests share: the reference / HIP pair builders and the whole-network protocol, split at the
CPU / GPU line.  yardstick() -- the reference against its own fp64 copy -- needs no GPU; hip_rows() runs the HIP path on the
same batch.  The caps on the yardstick, the tensor counts and what a family prints beyond this stay in that family's test."""
from collections import namedtuple

import torch
import torch.nn as nn

from _parity import hip_step, oracle_step, xent_backward  # noqa: F401  (xent_backward: for the family tests that import it here)
from oracle import ops_ref as R
from oracle.resnet_ref import ResNetRef, _Block


def named_shapes(model):
    return [(n, tuple(p.shape)) for n, p in model.named_parameters()]


def set_last_gamma(ref, value):
    for m in ref.modules():
        if isinstance(m, _Block):
            m.last_bn.weight.data.fill_(value)


def timm_default_ref(arch, num_classes, seed=0, gamma_last=0.0):
    """The configuration the reference really trains from: timm's ResNet init (Kaiming fan-out filters, BatchNorm weight 1 /
    bias 0, ZERO-initialised last BatchNorm weight of every residual block), or that weight at gamma_last."""
    torch.manual_seed(seed)
    ref = ResNetRef(arch, num_classes, bf16_points=True, zero_init_last=True)
    if gamma_last:
        set_last_gamma(ref, gamma_last)
    return ref


def timm_default_pair(arch, num_classes, seed=0, gamma_last=0.0):
    from imageclassification_amd.nets import ResNet
    ref = timm_default_ref(arch, num_classes, seed, gamma_last)
    net = ResNet(arch, num_classes)
    net.load_state_dict(ref.state_dict())
    return ref, net


def perturbed_bn_pair(arch, num_classes, seed, affine=True):
    """Kaiming filters, random running statistics and, with `affine`, BatchNorm weights from U(0.5, 1.5) and biases from
    N(0, 0.1): (reference with the rounding points, HIP network, the state_dict both were loaded from)."""
    from imageclassification_amd.nets import ResNet
    torch.manual_seed(seed)
    ref = ResNetRef(arch, num_classes, bf16_points=True, zero_init_last=False)
    g = torch.Generator().manual_seed(seed + 1)
    bns = {n for n, m in ref.named_modules() if isinstance(m, nn.BatchNorm2d)}
    sd = ref.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.2
        elif k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif affine and k.rpartition(".")[0] in bns and k.endswith(".weight"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif affine and k.rpartition(".")[0] in bns and k.endswith(".bias"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    ref.load_state_dict(sd)
    net = ResNet(arch, num_classes)
    net.load_state_dict(sd)
    return ref, net, sd


def parity_batch(num_classes, batch, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 3, hw, hw, generator=g), torch.randint(0, num_classes, (batch,), generator=g)


# noise: name -> relative L2 distance of the fp64 copy's gradient, for every tensor whose gradient is not all zero
Yardstick = namedtuple("Yardstick", "logits loss grads noise_logits noise mean_noise worst_noise")
# rows: (name, HIP error, yardstick noise) per tensor of Yardstick.noise; worst: the row with the largest HIP error
HipResult = namedtuple("HipResult", "err_logits loss rows zero_branch mean_err worst")


def yardstick(ref, x, y, smoothing):
    """The reference and its fp64 copy (same rounding points) take one training forward + backward on the CPU."""
    ref.train()                      # the twin is a copy: it trains too
    o = oracle_step(ref, x, y, smoothing)
    p64 = dict(o.ref64.named_parameters())
    grads = {n: p.grad for n, p in ref.named_parameters()}
    noise = {n: R.rel_l2(p64[n].grad.float(), g) for n, g in grads.items() if float(g.abs().max()) != 0.0}
    return Yardstick(o.out, o.loss, grads, R.rel_l2(o.out64, o.out), noise,
                     sum(noise.values()) / len(noise), max(noise.items(), key=lambda kv: kv[1]))


def hip_rows(net, x, y, num_classes, smoothing, yard):
    """The HIP path on the yardstick's batch.  Where the reference's gradient is all zero (zero-gamma branches) the HIP
    gradient is asserted exactly zero and counted; every other tensor gets a row."""
    _, logits, hip_loss = hip_step(net, x, y, num_classes, smoothing)
    err_logits = R.rel_l2(logits, yard.logits)
    rows, zero_branch = [], 0
    for name, grad in yard.grads.items():
        if name not in yard.noise:
            assert float(net.grad_of(name).abs().max()) == 0.0, name
            zero_branch += 1
            continue
        rows.append((name, R.rel_l2(net.grad_of(name), grad), yard.noise[name]))
    return HipResult(err_logits, hip_loss, rows, zero_branch, sum(r[1] for r in rows) / len(rows), max(rows, key=lambda r: r[1]))


def assert_hip_within_yardstick(yard, got):
    """logits <= 2 max(noise, 1e-3), loss to 1e-3, mean gradient error <= 2 max(mean noise, 1e-3), per tensor <= 3 max(its
    noise, 5e-3)."""
    assert got.err_logits <= 2.0 * max(yard.noise_logits, 1e-3)
    assert abs(got.loss - yard.loss) <= 1e-3 * abs(yard.loss)
    assert got.mean_err <= 2.0 * max(yard.mean_noise, 1e-3)
    for name, e, n in got.rows:
        assert e <= 3.0 * max(n, 5e-3), (name, e, n)
