"""The switches and routes of ResNet.backward_packed, HIP path against HIP path on one saved forward state (no CPU oracle).

ResNet-50, 100 classes, batch 32 at 256 x 256: by the thresholds in nets.py the smallest shape at which the default backward takes
every one of its branches (layer1/2 rows 131072 / 32768: fused conv3 + bn3 backward and the deferred apply + conv1; layer3 rows
8192: icamd_bn_bwd_from_gy_partials in its identity blocks; layer4 plain; layer3.0 / layer4.0 icamd_bn_bwd_dual; layer2.0 fused
conv3 + stride-2 shortcut on the even grid + bnred hand-over; layer1.0 fused stride-1 shortcut).  `zero_init_last=False` keeps
every one of the 161 gradient tensors non-zero.  One forward, then several backward_packed(ws) calls, each followed by a copy of
the gradient arena."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C, B, HW = 100, 32, 256

# Kernel launches per profiling class of ONE default forward + backward at the shape above (hip.prof_collect), recorded before the
# backward was split into named steps; classes not listed are 0.
PROF_CALLS = {"conv_fwd": 48, "conv_dgrad": 45, "conv_wgrad": 46, "bn_finalize": 53, "bn_apply": 43, "bn_bwd": 43, "pool": 2,
              "misc": 1, "conv_bn_bwd_fused": 8, "bn_apply_conv_fused": 6}

# switch -> (worst, mean) per-tensor relative L2 of the 161 gradient tensors against the default route, as measured on an MI355X
# before the backward was split into named steps.  They differ by reduction order and bf16 re-rounding of the gradient chain only;
# the kernels are deterministic, and each figure is asserted with a factor 2 for another compiler or driver.  A dropped term or
# stride class scores >= 0.5 on its tensor (tests/test_model_gpu.py), so no asserted bound may exceed 0.1: WORST_CAP holds where
# twice the measured worst would pass it.
WORST_CAP = 0.1
MEASURED = {
    "_SUB2_SHORTCUT": (False, 8.274e-2, 2.248e-3),
    "_DUAL_BNBWD": (False, 0.0, 0.0),
    "_FUSED_BNBWD": (True, 9.594e-2, 1.079e-2),
}


def _forward_state(arch, batch, hw, seed):
    from imageclassification_amd import hip
    from imageclassification_amd.nets import ResNet
    net = ResNet(arch, num_classes=C, zero_init_last=False, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, 3, hw, hw, generator=g).cuda()
    y = torch.randint(0, C, (batch,), generator=g).cuda()
    net.train()
    ws = net.pack(x)
    net.forward_packed(ws)
    hip.check(net.lib.icamd_softmax_xent(ws["logits"].data_ptr(), net.ncls_p, batch, C, y.data_ptr(), None, 1.0, 0.1, 1.0 / batch,
                                         ws["loss_rows"].data_ptr(), ws["pred"].data_ptr(), ws["dlogits"].data_ptr(),
                                         hip.stream_ptr()), "xent")
    torch.cuda.synchronize()
    return net, ws


def _backward(net, ws):
    """One backward_packed on the saved forward state -> a copy of the gradient arena (zeroed first: a tensor a route forgets to
    write scores 1.0, it does not inherit the previous run's values)."""
    net.grad_arena.zero_()
    net.backward_packed(ws)
    torch.cuda.synchronize()
    return net.grad_arena.clone()


@pytest.fixture(scope="module")
def r50():
    net, ws = _forward_state("resnet50", B, HW, seed=11)
    default = _backward(net, ws)
    assert bool(torch.isfinite(default).all())
    return net, ws, default


def test_default_route_is_deterministic(r50):
    net, ws, default = r50
    assert len(net.params) == 161
    again = _backward(net, ws)
    assert torch.equal(again, default)
    host = default.cpu()
    for name, p in net.params.items():
        assert float(host[p.offset:p.offset + p.numel].abs().max()) > 0.0, name


def _one_stream_against_two(net, ws, default):
    assert net.wgrad_side_stream
    net.wgrad_side_stream = False
    try:
        one = _backward(net, ws)
    finally:
        net.wgrad_side_stream = True
    assert torch.equal(one, default)


def test_weight_gradients_on_the_main_stream_are_bit_equal(r50):
    _one_stream_against_two(*r50)


@pytest.mark.parametrize("arch", ["resnet18", "resnext50_32x4d"])
def test_one_stream_bit_equal_basic_and_grouped(arch):
    """Basic blocks (3x3 conv1, no bottleneck routes) and ResNeXt's grouped weight / data gradients, batch 8 at 64 x 64."""
    net, ws = _forward_state(arch, 8, 64, seed=13)
    default = _backward(net, ws)
    assert float(default.abs().max()) > 0.0 and bool(torch.isfinite(default).all())
    _one_stream_against_two(net, ws, default)


def test_two_call_stem_pool_backward_is_bit_equal(r50, monkeypatch):
    import imageclassification_amd.nets as nets
    net, ws, default = r50
    monkeypatch.setattr(nets, "_FUSED_POOL_BWD", False)
    assert torch.equal(_backward(net, ws), default)


@pytest.mark.parametrize("switch", sorted(MEASURED))
def test_switched_route_against_default(r50, monkeypatch, switch):
    """Measured before the split (worst tensor / mean over the 161 tensors / tensors that are bit-equal):
    _SUB2_SHORTCUT=False  worst bn1.bias 8.274e-2, mean 2.248e-3, 89 bit-equal
    _DUAL_BNBWD=False     bit-equal in all 161 (so asserted bit-equal: twice zero)
    _FUSED_BNBWD=True     worst bn1.bias 9.594e-2, mean 1.079e-2, 5 bit-equal
    Both worst figures are above 0.05 and sit on the stem BatchNorm's bias, the sum of the gradient at the far end of the chain over
    32 x 128 x 128 signed values per channel; the second-worst tensors are bn1.weight at 1.24e-2 and layer1.0.bn1.weight at
    2.03e-2.  Twice either worst figure would pass 0.1, so the cap is what is asserted for them."""
    import imageclassification_amd.nets as nets
    from imageclassification_amd.arena import from_arena
    from oracle import ops_ref as R
    net, ws, default = r50
    value, worst_measured, mean_measured = MEASURED[switch]
    worst_bound = min(2.0 * worst_measured, WORST_CAP)
    assert getattr(nets, switch) != value
    monkeypatch.setattr(nets, switch, value)
    got = _backward(net, ws).cpu()
    want = default.cpu()
    errs = []
    for name, p in net.params.items():
        sl = slice(p.offset, p.offset + p.numel)
        errs.append((float(R.rel_l2(from_arena(p, got[sl]), from_arena(p, want[sl]))), name))
    worst, mean = max(errs), sum(e for e, _ in errs) / len(errs)
    print(f"{switch}={value} against the default route, {len(errs)} tensors: worst {worst[1]} {worst[0]:.3e}, mean {mean:.3e}, "
          f"bit-equal tensors {sum(e == 0.0 for e, _ in errs)}; five worst {sorted(errs, reverse=True)[:5]}")
    assert len(errs) == 161
    assert worst[0] <= worst_bound, worst
    assert mean <= 2.0 * mean_measured


def test_routing_did_not_move(r50):
    """Launch counts per profiling class of one default forward + backward."""
    from imageclassification_amd import hip
    net, ws, default = r50
    hip.prof_collect()
    net.lib.icamd_prof_enable(1)
    try:
        net.forward_packed(ws)
        net.backward_packed(ws)
        torch.cuda.synchronize()
    finally:
        net.lib.icamd_prof_enable(0)
    calls = {k: v[1] for k, v in hip.prof_collect().items() if v[1]}
    print("prof calls:", calls)
    assert calls == PROF_CALLS
    assert torch.equal(net.grad_arena, default)


def test_profiler_state_is_one_object_across_the_capi_units():
    """The C-ABI layer is five translation units (csrc/capi*.hip) around one profiler state, defined in capi.hip.  One tiny call
    into each unit while profiling is on: icamd_prof_collect (capi.hip) sees exactly one call in each of their five classes and none
    anywhere else -- a unit with a state of its own would never see the switch, or would keep its record to itself."""
    import ctypes
    from imageclassification_amd import hip
    lib = hip.load()
    dev, s = "cuda", hip.stream_ptr()
    bf = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16, device=dev)      # noqa: E731
    f32 = lambda *shape: torch.ones(*shape, dtype=torch.float32, device=dev)       # noqa: E731
    x, w, y = bf(1, 8, 8, 64), bf(64, 1, 1, 64), bf(1, 8, 8, 64)                   # capi.hip: 1x1 convolution, 64 -> 64 at 8 x 8
    d = hip.conv_desc(1, 8, 8, 64, 64, 1, 1, 1, 0)
    gamma, beta, rm, rv, scale, shift = (f32(64) for _ in range(6))                # capi_norm.hip: C = 64
    z, a = bf(1024), bf(1024)                                                      # capi_tokens.hip
    src, dst = f32(1024), bf(1024)                                                 # capi_step.hip
    px, pout = bf(1, 2, 2, 8), bf(1, 1, 1, 8)                                      # capi_conv_special.hip: 2x2 average pool, C = 8
    torch.cuda.synchronize()
    hip.prof_collect()
    lib.icamd_prof_enable(1)
    try:
        hip.check(lib.icamd_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None, None, s), "conv2d_fwd")
        hip.check(lib.icamd_bn_eval_coeffs(64, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5,
                                           scale.data_ptr(), shift.data_ptr(), s), "bn_eval_coeffs")
        hip.check(lib.icamd_gelu_fwd(z.data_ptr(), a.data_ptr(), 1024, s), "gelu_fwd")
        hip.check(lib.icamd_f32_to_bf16(src.data_ptr(), dst.data_ptr(), 1024, s), "f32_to_bf16")
        hip.check(lib.icamd_avgpool2x2_fwd(px.data_ptr(), pout.data_ptr(), 1, 2, 2, 8, s), "avgpool2x2_fwd")
        torch.cuda.synchronize()
    finally:
        lib.icamd_prof_enable(0)
    calls = {k: v[1] for k, v in hip.prof_collect().items()}
    print("prof calls:", {k: v for k, v in calls.items() if v})
    expected = {"conv_fwd": 1, "bn_finalize": 1, "elementwise": 1, "optimizer": 1, "pool": 1}
    assert calls == {k: expected.get(k, 0) for k in hip.PROF_CLASSES}
    assert bool((dst.float() == 1).all())                                          # the calls ran: f32 ones arrived as bf16 ones
    assert all(v[1] == 0 for v in hip.prof_collect().values())                     # collected once, the log is empty
