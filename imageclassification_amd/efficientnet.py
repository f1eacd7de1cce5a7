"""EfficientNet-B0 / B1 on the HIP kernels: timm's `efficientnet_b0` / `efficientnet_b1` (MBConv blocks with squeeze-and-excitation,
depthwise 3x3 and 5x5, SiLU; symmetric padding k // 2, BatchNorm eps 1e-5 / momentum 0.1 -- not the `tf_` variants), restated.

    conv_stem 3x3/2 -> bn1 + SiLU
    blocks.0.B   depthwise-separable: conv_dw 3x3 -> bn1 + SiLU -> se -> conv_pw 1x1 -> bn2 (+ input when in = out: B1's blocks.0.1)
    blocks.S.B   inverted residual:   conv_pw 1x1 (in -> 6 in) -> bn1 + SiLU -> conv_dw k x k / s -> bn2 + SiLU -> se -> conv_pwl 1x1
                 -> bn3 (+ input when s = 1 and in = out)
    se           gate = sigmoid(conv_expand(silu(conv_reduce(mean_hw(a))))), a the ACTIVATED depthwise output; the reduced width is a
                 quarter of the block's INPUT width; the projection convolution reads a * gate
    conv_head 1x1 -> bn2 + SiLU -> global average pool -> classifier

No dropout and no stochastic depth (timm's defaults for the family; the reference passes --drop_path elsewhere only).

What is stored per block: y1 (raw conv_pw output), y2 (raw depthwise output), the GATED projection input bf16(a2 * gate), y3 and the
block output, plus the [N, C]-sized fp32 arrays of the excitation (s, hpre, gate).  The ungated a2 = silu(bn2(y2)) is never stored:
icamd_bn_silu_squeeze sums it, icamd_bn_apply_silu writes it gated, and the backward recomputes it (and silu') from y2.  The expanded
a1 = silu(bn1(y1)) goes through the model's one scratch buffer in front of the depthwise call and is recomputed for the weight
gradient, as MobileNetV2's plain route does (profiles/mobilenetv2.txt measured the on-load form slower; it is not built for 5x5).

Launches of an inverted-residual block.  Forward: conv_pw, finalize, apply_silu (a1), depthwise, finalize, squeeze, excite, gated
apply, conv_pwl, finalize, apply (+ input).  Backward: bn3 backward, conv_pwl weight + data gradient, gate-gradient reduce, excite
backward, bn2 + SiLU backward (reduce, finalize, apply), apply_silu (a1 again), depthwise data gradient, depthwise weight gradient,
bn1 + SiLU backward, conv_pw weight + data gradient.  One stream; eval walks the same graph with icamd_bn_eval_coeffs' scale / shift.
"""
import math

import torch

from . import hip, mbconv

# (kernel, first stride, out channels, repeats) of stages 1..6; name -> (stem, (stage 0 out, repeats), stages, head)
_B0 = ((3, 2, 24, 2), (5, 2, 40, 2), (3, 2, 80, 3), (5, 1, 112, 3), (5, 2, 192, 4), (3, 1, 320, 1))


def _scaled(depth):
    return tuple((k, s, c, int(math.ceil(depth * n))) for k, s, c, n in _B0)


CONFIGS = {"efficientnet_b0": (32, (16, 1), _scaled(1.0), 1280), "efficientnet_b1": (32, (16, 2), _scaled(1.1), 1280)}
# parity-test member: one block of every kind -- the depthwise-separable one, 3x3 and 5x5 at stride 2, stride-1 blocks with the skip
CONFIGS["efficientnet_test"] = (16, (8, 1), ((3, 2, 16, 2), (5, 2, 24, 1), (5, 1, 32, 2)), 64)


def block_plan(arch):
    """(stem width, [(name, kind, kernel, in, mid, out, stride, rd)], head width), mbconv.py's plan; kind "ds" (mid = in) or "ir" (mid = 6 in); rd, the
    reduced width of the block's squeeze-and-excitation, is a quarter of the block INPUT width"""
    stem, (first, first_n), stages, head = CONFIGS[arch]
    blocks, cin = [], stem
    for bi in range(first_n):
        blocks.append((f"blocks.0.{bi}", "ds", 3, cin, cin, first, 1, max(1, cin // 4)))
        cin = first
    for si, (k, stride, out, repeats) in enumerate(stages, 1):
        for bi in range(repeats):
            blocks.append((f"blocks.{si}.{bi}", "ir", k, cin, cin * 6, out, stride if bi == 0 else 1, max(1, cin // 4)))
            cin = out
    return stem, blocks, head


def se_shapes(name, c, rd):
    return [(name + ".conv_reduce.weight", (rd, c, 1, 1)), (name + ".conv_reduce.bias", (rd,)),
            (name + ".conv_expand.weight", (c, rd, 1, 1)), (name + ".conv_expand.bias", (c,))]


def param_shapes(arch, num_classes=1000):
    """[(name, torch shape)] in timm's module order (parameters only)"""
    return mbconv.param_shapes(block_plan(arch), num_classes, se_shapes)


class _SE:
    """Squeeze-and-excitation record: conv_reduce [rd][C] + bias, conv_expand [C][rd] + bias, fp32 in the parameter arena in torch
    layout; the excite kernels read the fp32 masters (the bf16 shadow slice is written by the optimizer and read by nothing)."""

    def __init__(self, name, c, rd):
        self.name, self.c, self.rd = name, c, rd
        self.w1 = self.b1 = self.w2 = self.b2 = None


class EfficientNet(mbconv.MBConvModel):
    """HIP EfficientNet: mbconv.py's walks with SiLU and a squeeze-and-excitation behind every depthwise BatchNorm."""
    block_plan = staticmethod(block_plan)
    _se_record = _SE      # (name, c, rd) -> the record of a block's squeeze-and-excitation

    def __init__(self, arch="efficientnet_b0", num_classes=1000, device="cuda", seed=None):
        super().__init__(arch, num_classes, device, seed)

    def _residual(self, kind, cin, cout, stride):
        return stride == 1 and cin == cout

    def _add_record(self, add, m):
        """The second kind of record of its own: a squeeze-and-excitation module."""
        if not isinstance(m, _SE):
            return super()._add_record(add, m)
        (n1, s1), (nb1, sb1), (n2, s2), (nb2, sb2) = se_shapes(m.name, m.c, m.rd)
        m.w1 = add(n1, s1, "conv", (m.rd, 1, 1, m.c))     # [rd][1][1][C] is torch's (rd, C, 1, 1) memory
        m.b1 = add(nb1, sb1, "vec", sb1)
        m.w2 = add(n2, s2, "conv", (m.c, 1, 1, m.rd))
        m.b2 = add(nb2, sb2, "vec", sb2)

    # ------------------------------------------------------------------ workspaces
    def _block_workspace(self, blk, b, N, hw, sizes):
        """the [N, C]-sized fp32 arrays of the excitation; the largest workspace of the two reduce passes and the largest N C"""
        lib, se = self.lib, blk.se
        for key, width in (("se_asum", se.c), ("se_s", se.c), ("se_h", se.rd), ("se_e", se.c)):
            b[key] = torch.empty(N, width, dtype=torch.float32, device=self.device)
        sizes.se = max(getattr(sizes, "se", 0), lib.icamd_bn_silu_squeeze_workspace_bytes(N, hw, se.c),
                       lib.icamd_se_silu_bwd_reduce_workspace_bytes(N, hw, se.c))
        sizes.nc = max(getattr(sizes, "nc", 0), N * se.c)

    def _extra_workspaces(self, ws, sizes):
        dev = self.device
        ws["se_ws"] = torch.empty(max(sizes.se, 64), dtype=torch.uint8, device=dev)
        ws["se_ws_bytes"] = sizes.se
        ws["se_de"] = torch.empty(sizes.nc, dtype=torch.float32, device=dev)       # gate gradient and dsn of the block in hand
        ws["se_dsn"] = torch.empty(sizes.nc, dtype=torch.float32, device=dev)
        # scale 1 | shift 0: the data gradient of a depthwise-separable block with a skip is added to the skip's by icamd_bn_apply
        ws["ident"] = torch.cat([torch.ones(self.bn_width, device=dev), torch.zeros(self.bn_width, device=dev)])

    # ------------------------------------------------------------------ forward
    def _apply_act(self, s, y, scale, shift, out, what, gate=None):
        """out = silu(y * scale + shift), times gate[n][c] when given; y [N][h][w][C]"""
        N, C = y.shape[0], y.shape[-1]
        hip.check(self.lib.icamd_bn_apply_silu(y.data_ptr(), scale, shift, gate, out, N, y.numel() // (N * C), C, s), what)

    def _dw_input(self, ws, op, src, coeffs, s):
        """silu(bn(src)) in the model's one scratch buffer: the input of a depthwise call, never formed on load"""
        a1 = self._scratch(ws, "a1").data_ptr()
        self._apply_act(s, src, coeffs[0], coeffs[1], a1, "a1")
        return a1, None, None

    def _se_gate(self, fw, blk, b, scale, shift):
        """the squeeze pass over y2, the excitation, the gated apply pass: b["a2"] = bf16(silu(bn(y2)) * gate)"""
        lib, ws, N, s, se = self.lib, fw.ws, fw.N, fw.s, blk.se
        hw = b["y2"].shape[1] * b["y2"].shape[2]
        hip.check(lib.icamd_bn_silu_squeeze(b["y2"].data_ptr(), scale, shift, b["se_asum"].data_ptr(), N, hw, se.c,
                                            ws["se_ws"].data_ptr(), ws["se_ws_bytes"], s), se.name + " squeeze")
        hip.check(lib.icamd_se_excite_silu_fwd(b["se_asum"].data_ptr(), 1.0 / hw, self._pf(se.w1), self._pf(se.b1), self._pf(se.w2),
                                               self._pf(se.b2), b["se_s"].data_ptr(), b["se_h"].data_ptr(), b["se_e"].data_ptr(), N,
                                               se.c, se.rd, s), se.name + " excite")
        self._apply_act(s, b["y2"], scale, shift, b["a2"].data_ptr(), se.name + " apply", gate=b["se_e"].data_ptr())

    # ------------------------------------------------------------------ backward
    def _bn_act_bwd(self, run, bn, dout, y, dy, gate=None, dsn=None):
        """dy = BatchNorm backward of `bn` over y from dout, behind a SiLU (silu' recomputed from y); the upstream gradient is dout *
        gate + dsn when the two [N, C] arrays are given"""
        mean, invstd, scale, shift = self._stats(bn)
        c, N = bn.c, y.shape[0]
        hip.check(self.lib.icamd_bn_bwd_silu(dout, y.data_ptr(), mean, invstd, scale, shift, gate, dsn, self._gf(bn.weight),
                                             self._gf(bn.bias), dy, N, y.numel() // (c * N), c, run.acc, run.bws, run.bwb, run.s),
                  bn.name + " bwd")

    def _se_bn_bwd(self, run, blk, b, dgated, dy):
        """from the gradient of the gated tensor: the gate-gradient pass, the excitation backward (its parameter gradients and dsn),
        and the BatchNorm + SiLU backward of the depthwise BatchNorm under dout * gate + dsn -> dy = d y2"""
        lib, ws, N, se = self.lib, run.ws, run.N, blk.se
        y2 = b["y2"]
        hw = y2.shape[1] * y2.shape[2]
        _, _, scale, shift = self._stats(blk.bn_dw)
        de, dsn = ws["se_de"].data_ptr(), ws["se_dsn"].data_ptr()
        hip.check(lib.icamd_se_silu_bwd_reduce(dgated, y2.data_ptr(), scale, shift, de, N, hw, se.c, ws["se_ws"].data_ptr(),
                                               ws["se_ws_bytes"], run.s), se.name + " gate gradient")
        hip.check(lib.icamd_se_excite_silu_bwd(de, b["se_s"].data_ptr(), b["se_h"].data_ptr(), b["se_e"].data_ptr(), self._pf(se.w1),
                                               self._pf(se.w2), self._gf(se.w1), self._gf(se.b1), self._gf(se.w2), self._gf(se.b2), dsn,
                                               N, se.c, se.rd, 1.0 / hw, run.acc, run.s), se.name + " excite bwd")
        self._bn_act_bwd(run, blk.bn_dw, dgated, y2, dy, gate=b["se_e"].data_ptr(), dsn=dsn)

    _after_dw_fwd, _after_dw_bwd = _se_gate, _se_bn_bwd

    def _dw_bwd(self, run, dw, src, src_bn, h, w, dy, dx):
        """the input formed from src, data gradient, weight gradient: in this order"""
        _, _, scale, shift = self._stats(src_bn)
        dw_in = self._dw_input(run.ws, "wgrad", src, (scale, shift), run.s)
        self._dw_dgrad(run, dw, h, w, dy, dx)
        self._dw_wgrad(run, dw, dw_in, h, w, dy)
