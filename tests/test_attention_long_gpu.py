"""icamd_attention_fwd / icamd_attention_bwd above T = 208: the tiled route of csrc/attention_long.hip, through the C ABI.

The resident kernels of csrc/attention.hip end at T = 208; longer sequences (ViT at 384^2 / 448^2 / 512^2: T = 577 / 785 / 1025)
stream K / V (or Q / dO) through LDS in 64-row tiles with an online softmax.  Bounds are those tests/test_kernels_gpu.py applies
to the same entries at T <= 208: the rounding points are the same (P and dS rounded to bf16 once as MFMA operands, fp32
accumulation, one final rounding), so the distance to the oracle does not grow with T.

Every output is allocated with a guard band behind it (tests/_harness.py guarded: at least one 64-row tile) that
must come back untouched: the buffers hold exactly B * T rows, and a tile that reaches past T must store nothing there.

ICAMD_ATTN_LONG is read once per process, so the forced (2) and disabled (0) routes run in child processes.
"""
import os
import subprocess
import sys

import pytest
import torch

from _attention_long import D, SCALE, digest_case, operands, run
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

LONG_CASES = [(1, 209, 2), (2, 257, 3), (2, 333, 2), (2, 577, 12), (1, 785, 4), (1, 1025, 2),
              # 288 pairs x 5 query blocks = 1440 workgroups: several rounds of every CU
              (24, 577, 12)]
SHORT_CASES = [(2, 17, 3), (3, 50, 4), (1, 64, 2), (2, 100, 3), (2, 192, 2), (2, 197, 12), (1, 208, 2)]


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


def child(code, mode):
    """Run `code` (which has `T` = this module, `AL` = tests/_attention_long.py, `UNSUPPORTED` and `lib`) in a fresh process with
    ICAMD_ATTN_LONG = mode."""
    here = os.path.dirname(os.path.abspath(__file__))
    prelude = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import test_attention_long_gpu as T\n"
        "import _attention_long as AL\n"
        "from _harness import UNSUPPORTED\n"
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
          "qkv, dout = AL.operands(B, T_, H)\n"
          "rc_f, rc_b, out, lse, delta, dqkv = AL.run(lib, qkv, dout, B, T_, H)\n"
          "assert rc_f == UNSUPPORTED and rc_b == UNSUPPORTED, (rc_f, rc_b)\n"
          "for t in (out, lse, delta, dqkv):\n"
          "    assert bool(torch.isnan(t.float()).all()), 'a refused call wrote to an output'\n"
          "print('child-ok')\n", "0")


def test_default_route_below_209_is_the_resident_kernels(lib):
    """T = 197 must give the same bits with the tiled route disabled: the default rule did not move it."""
    assert "ICAMD_ATTN_LONG" not in os.environ, "this test compares the default routing; unset ICAMD_ATTN_LONG"
    here = digest_case(lib, 2, 197, 12)
    out = child("print('digest', AL.digest_case(lib, 2, 197, 12))\nprint('child-ok')\n", "0")
    there = [ln.split()[1] for ln in out.splitlines() if ln.startswith("digest ")]
    assert there == [here]
