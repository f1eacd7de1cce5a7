"""MobileNetV2 on the HIP kernels: timm's `mobilenetv2_*` (inverted residuals, depthwise 3x3, ReLU6), restated.

    conv_stem 3x3/2 -> bn1 + ReLU6
    blocks.0.0   depthwise-separable: conv_dw 3x3 -> bn1 + ReLU6 -> conv_pw 1x1 -> bn2
    blocks.S.B   inverted residual:   conv_pw 1x1 (in -> 6 in) -> bn1 + ReLU6 -> conv_dw 3x3 / s -> bn2 + ReLU6 -> conv_pwl 1x1 -> bn3
                 (+ input when s = 1 and in = out)
    conv_head 1x1 -> bn2 + ReLU6 -> global average pool -> classifier

Every channel count is make_divisible(c * width multiplier, 8), so every pointwise layer runs on the general convolution entries
(Cin % 8 == 0, Cout % 8 == 0) and every depthwise one on icamd_dwconv3_* (C % 8 == 0).  No stochastic depth and no dropout.

What is stored per inverted-residual block: y1 (raw conv_pw output, six times the block's width), y2 (raw depthwise output), a2 =
relu6(bn2(y2)), y3 and the block output.  The activated a1 = relu6(bn1(y1)) is NEVER stored per block: the depthwise forward and weight
gradient either form it on load from y1 and bn1's scale / shift, or icamd_bn_apply_relu6 writes it into the model's one scratch buffer
right in front of them (DW_ONLOAD; the same bits either way), and the BatchNorm + ReLU6 backward recomputes its mask from y and the
same scale / shift.  The same holds for the stem's activation in
front of blocks.0.0.conv_dw.  One stream; eval walks the same graph with icamd_bn_eval_coeffs' scale / shift (no filter folding).
"""
from . import hip, mbconv

# Does a depthwise layer form relu6(bn(y)) on load ("fwd": icamd_dwconv3_fwd, "wgrad": icamd_dwconv3_wgrad), or read a tensor that
# icamd_bn_apply_relu6 wrote first (into ONE scratch buffer of the model: it is recomputed for the weight gradient, so the expanded
# activation is not stored per block either way)?  A module constant per operation, not an environment variable; both routes give
# the same bits (tests/test_dwconv3_gpu.py, tests/test_mobilenetv2_gpu.py).  Measured (profiles/mobilenetv2.txt, the ten shapes of
# mobilenetv2_100 at batch 256): apply + plain beats the on-load form beyond the spread at all ten shapes for the forward and at nine
# for the weight gradient -- a thread activates the three columns under its output, so the on-load kernels do that arithmetic three times and
# are VALU-bound on it -- so both default to the plain route.
DW_ONLOAD = {"fwd": False, "wgrad": False}

# (repeats, first stride, out channels) of stages 1..6; name -> (width multiplier, stem, stage 0 out, stages, head)
_STAGES = ((2, 2, 24), (3, 2, 32), (4, 2, 64), (3, 1, 96), (3, 2, 160), (1, 1, 320))
CONFIGS = {f"mobilenetv2_{tag}": (m, 32, 16, _STAGES, 1280) for tag, m in (("035", 0.35), ("050", 0.5), ("075", 0.75), ("100", 1.0),
                                                                           ("140", 1.4))}
# parity-test member: a stride-2 block, a stride-1 block with and without residual, the depthwise-separable block
CONFIGS["mobilenetv2_test"] = (1.0, 16, 8, ((2, 2, 16), (1, 2, 24), (2, 1, 32)), 64)


def make_divisible(v, divisor=8, round_limit=0.9):
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new < round_limit * v:
        new += divisor
    return new


def block_plan(arch):
    """(stem width, [(name, kind, kernel, in, mid, out, stride, rd)], head width), mbconv.py's plan; kind "ds" (mid = in) or "ir" (mid =
    make_divisible(6 in)); the kernel is 3 and rd None (no squeeze-and-excitation) throughout"""
    mult, stem, first, stages, head = CONFIGS[arch]
    r = lambda c: make_divisible(c * mult)     # noqa: E731
    cin = r(stem)
    blocks = [("blocks.0.0", "ds", 3, cin, cin, r(first), 1, None)]
    plan_stem, cin = cin, r(first)
    for si, (repeats, stride, out) in enumerate(stages, 1):
        for bi in range(repeats):
            blocks.append((f"blocks.{si}.{bi}", "ir", 3, cin, make_divisible(cin * 6), r(out), stride if bi == 0 else 1, None))
            cin = r(out)
    return plan_stem, blocks, (head if arch == "mobilenetv2_test" else max(head, r(head)))


def param_shapes(arch, num_classes=1000):
    """[(name, torch shape)] in timm's module order (parameters only)"""
    return mbconv.param_shapes(block_plan(arch), num_classes)


class MobileNetV2(mbconv.MBConvModel):
    """HIP MobileNetV2: mbconv.py's walks with ReLU6 and no gate."""
    block_plan = staticmethod(block_plan)

    def __init__(self, arch="mobilenetv2_100", num_classes=1000, device="cuda", seed=None):
        super().__init__(arch, num_classes, device, seed)

    def _residual(self, kind, cin, cout, stride):
        return kind == "ir" and stride == 1 and cin == cout

    def _apply_act(self, s, y, scale, shift, out, what):
        hip.check(self.lib.icamd_bn_apply_relu6(y.data_ptr(), scale, shift, out, y.numel(), y.shape[-1], s), what)

    def _dw_input(self, ws, op, src, coeffs, s):
        """(x, scale, shift) arguments of a depthwise entry whose input is relu6(bn(src)): on load, or applied into the scratch"""
        if DW_ONLOAD[op]:
            return src.data_ptr(), coeffs[0], coeffs[1]
        a1 = self._scratch(ws, "a1").data_ptr()
        self._apply_act(s, src, coeffs[0], coeffs[1], a1, "a1")
        return a1, None, None

    def _after_dw_fwd(self, fw, blk, b, scale, shift):
        self._apply_act(fw.s, b["y2"], scale, shift, b["a2"].data_ptr(), blk.bn_dw.name)

    def _bn_act_bwd(self, run, bn, dout, y, dy):
        """dy = BatchNorm backward of `bn` over y from dout, behind a ReLU6 (mask recomputed from y)"""
        mean, invstd, scale, shift = self._stats(bn)
        hip.check(self.lib.icamd_bn_bwd_relu6(dout, y.data_ptr(), mean, invstd, scale, shift, self._gf(bn.weight), self._gf(bn.bias),
                                              dy, y.numel() // bn.c, bn.c, run.acc, run.bws, run.bwb, run.s), bn.name + " bwd")

    def _after_dw_bwd(self, run, blk, b, da2, dy):
        self._bn_act_bwd(run, blk.bn_dw, da2, b["y2"], dy)

    def _dw_bwd(self, run, dw, src, src_bn, h, w, dy, dx):
        """data gradient, the input formed from src, weight gradient: in this order"""
        self._dw_dgrad(run, dw, h, w, dy, dx)
        _, _, scale, shift = self._stats(src_bn)
        self._dw_wgrad(run, dw, self._dw_input(run.ws, "wgrad", src, (scale, shift), run.s), h, w, dy)
