"""icamd_attention_fwd / icamd_attention_bwd above T = 208: the tiled route of csrc/attention_long.hip, through the C ABI.

The resident kernels of csrc/attention.hip end at T = 208; longer sequences (ViT at 384^2 / 448^2 / 512^2: T = 577 / 785 / 1025)
stream K / V (or Q / dO) through LDS in 64-row tiles with an online softmax.  Bounds are those tests/test_kernels_gpu.py applies
to the same entries at T <= 208: the rounding points are the same (P and dS rounded to bf16 once as MFMA operands, fp32
accumulation, one final rounding), so the distance to the oracle does not grow with T.

Every output is allocated with a guard band behind it (one 64-row tile, or 64 fp32 values per (image, head) row vector) that
must come back untouched: the buffers hold exactly B * T rows, and a tile that reaches past T must store nothing there.

ICAMD_ATTN_LONG is read once per process, so the forced (2) and disabled (0) routes run in child processes.
"""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 64
SCALE = D ** -0.5
BAND = 64                      # guard rows behind every output (one tile)
SENT16 = 0x5A5B                # bf16 bit pattern of the band (a finite value no kernel produces by accident)
SENT32 = 0x4B5A5B5C            # fp32 bit pattern of the band
ICAMD_ERR_UNSUPPORTED = 2

LONG_CASES = [(1, 209, 2), (2, 257, 3), (2, 333, 2), (2, 577, 12), (1, 785, 4), (1, 1025, 2),
              # 288 pairs x 5 query blocks = 1440 workgroups: several rounds of every CU
              (24, 577, 12)]
SHORT_CASES = [(2, 17, 3), (3, 50, 4), (1, 64, 2), (2, 100, 3), (2, 192, 2), (2, 197, 12), (1, 208, 2)]


@pytest.fixture(scope="module")
def lib():
    from imageclassification_amd import hip
    hip.require_gpu()
    return hip.load()


def _hip():
    from imageclassification_amd import hip
    return hip


def rnd_bf16(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return R.bf16_round(torch.randn(*shape, generator=g) * scale)


def guarded_bf16(rows, cols, fill):
    """[rows][cols] bf16 filled with `fill`, with BAND sentinel rows behind it in the same allocation.  Returns (view, whole)."""
    whole = torch.full(((rows + BAND) * cols,), SENT16, dtype=torch.int16, device=DEV)
    view = whole[:rows * cols].view(torch.bfloat16).view(rows, cols)
    view.fill_(fill)
    return view, whole


def guarded_f32(n, fill):
    whole = torch.full((n + BAND,), SENT32, dtype=torch.int32, device=DEV)
    view = whole[:n].view(torch.float32)
    view.fill_(fill)
    return view, whole


def band_intact(whole, n, sentinel):
    return bool((whole[n:] == sentinel).all())


def run(lib, qkv, dout, B, T, H):
    """Forward + backward on guarded outputs.  Returns (rc_fwd, rc_bwd, out, lse, delta, dqkv) and asserts the bands."""
    hip = _hip()
    qd = qkv.to(torch.bfloat16).to(DEV).contiguous()
    dd = dout.to(torch.bfloat16).to(DEV).contiguous()
    nan = float("nan")
    out, out_w = guarded_bf16(B * T, H * D, nan)
    lse, lse_w = guarded_f32(B * H * T, nan)
    delta, delta_w = guarded_f32(B * H * T, nan)
    dqkv, dqkv_w = guarded_bf16(B * T, 3 * H * D, nan)
    rc_f = lib.icamd_attention_fwd(hip.ptr(qd), hip.ptr(out), hip.ptr(lse), B, T, H, D, SCALE, hip.stream_ptr())
    rc_b = lib.icamd_attention_bwd(hip.ptr(qd), hip.ptr(out), hip.ptr(dd), hip.ptr(lse), hip.ptr(delta), hip.ptr(dqkv), B, T, H, D,
                                   SCALE, hip.stream_ptr())
    torch.cuda.synchronize()
    assert band_intact(out_w, B * T * H * D, SENT16), "guard band behind out written"
    assert band_intact(lse_w, B * H * T, SENT32), "guard band behind lse written"
    assert band_intact(delta_w, B * H * T, SENT32), "guard band behind delta written"
    assert band_intact(dqkv_w, B * T * 3 * H * D, SENT16), "guard band behind dqkv written"
    return rc_f, rc_b, out, lse.view(B, H, T), delta.view(B, H, T), dqkv


def operands(B, T, H):
    return rnd_bf16(B * T, 3 * H * D, scale=1.0, seed=120), rnd_bf16(B * T, H * D, seed=121)


def check_case(lib, B, T, H):
    """Parity with the oracle under the bounds of test_kernels_gpu.test_attention_fwd_bwd, finiteness, guard bands."""
    qkv, dout = operands(B, T, H)
    rc_f, rc_b, out, lse, delta, dqkv = run(lib, qkv, dout, B, T, H)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    ro, rlse = R.attention_fwd(qkv, B, T, H, D, SCALE)
    got = out.float().cpu()
    assert torch.isfinite(got).all() and torch.isfinite(lse).all() and torch.isfinite(delta).all()
    lse_err = float((lse.cpu() - rlse).abs().max())
    fwd = R.rel_l2(got, ro)
    print(f"B {B} T {T} H {H}: lse max abs err {lse_err:.3g}, fwd rel_l2 {fwd:.3g}")
    assert torch.allclose(lse.cpu(), rlse, rtol=1e-4, atol=1e-4)
    assert fwd <= 3e-3
    assert R.bf16_close(got, ro, ulps=2.0, atol_rms=8e-3, max_frac=1e-6 if B * H > 256 else 0.0)
    # delta = rowsum(dout * out) of the values the forward stored
    rdelta = (dout.reshape(B, T, H, D).double() * got.reshape(B, T, H, D).double()).sum(-1).permute(0, 2, 1)
    assert torch.allclose(delta.cpu().double(), rdelta, rtol=1e-4, atol=1e-4)
    rd = R.attention_bwd(qkv, dout, B, T, H, D, SCALE)
    gd = dqkv.float().cpu()
    assert torch.isfinite(gd).all()
    for name, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, 2 * H * D)), ("dv", slice(2 * H * D, 3 * H * D))):
        e = R.rel_l2(gd[:, sl], rd[:, sl])
        print(f"    {name} rel_l2 {e:.3g}")
        assert e <= 6e-3, name


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def digest_case(lib, B, T, H):
    qkv, dout = operands(B, T, H)
    rc_f, rc_b, out, lse, delta, dqkv = run(lib, qkv, dout, B, T, H)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    return digest(out, lse, delta, dqkv)


def child(code, mode):
    """Run `code` (which has `T` = this module and `lib`) in a fresh process with ICAMD_ATTN_LONG = mode."""
    here = os.path.dirname(os.path.abspath(__file__))
    prelude = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import test_attention_long_gpu as T\n"
        "from imageclassification_amd import hip\n"
        "lib = hip.load()\n"
    ) % (here, os.path.dirname(here))
    env = dict(os.environ, ICAMD_ATTN_LONG=mode)
    out = subprocess.run([sys.executable, "-c", prelude + code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "child-ok" in out.stdout, out.stdout + out.stderr
    return out.stdout


@pytest.mark.parametrize("B,T,H", LONG_CASES)
def test_long_attention_matches_oracle(lib, B, T, H):
    check_case(lib, B, T, H)


def test_long_attention_is_bitwise_reproducible(lib):
    assert digest_case(lib, 2, 577, 12) == digest_case(lib, 2, 577, 12)


def test_forced_long_route_on_short_sequences():
    """ICAMD_ATTN_LONG=2: a single ragged tile (17, 50), exact multiples of the tile (64, 192), the one-tile-only loop, and the
    production T = 197 on the tiled kernels."""
    child("for B, T_, H in T.SHORT_CASES:\n"
          "    T.check_case(lib, B, T_, H)\n"
          "print('child-ok')\n", "2")


def test_disabled_long_route_refuses_and_writes_nothing(lib):
    child("import torch\n"
          "B, T_, H = 1, 577, 2\n"
          "qkv, dout = T.operands(B, T_, H)\n"
          "rc_f, rc_b, out, lse, delta, dqkv = T.run(lib, qkv, dout, B, T_, H)\n"
          "assert rc_f == T.ICAMD_ERR_UNSUPPORTED and rc_b == T.ICAMD_ERR_UNSUPPORTED, (rc_f, rc_b)\n"
          "for t in (out, lse, delta, dqkv):\n"
          "    assert bool(torch.isnan(t.float()).all()), 'a refused call wrote to an output'\n"
          "print('child-ok')\n", "0")


def test_default_route_below_209_is_the_resident_kernels(lib):
    """T = 197 must give the same bits with the tiled route disabled: the default rule did not move it."""
    assert "ICAMD_ATTN_LONG" not in os.environ, "this test compares the default routing; unset ICAMD_ATTN_LONG"
    here = digest_case(lib, 2, 197, 12)
    out = child("print('digest', T.digest_case(lib, 2, 197, 12))\nprint('child-ok')\n", "0")
    there = [ln.split()[1] for ln in out.splitlines() if ln.startswith("digest ")]
    assert there == [here]
