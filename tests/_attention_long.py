"""Shared by tests/test_attention_long_gpu.py and tests/test_attention_ranges_gpu.py: seeded operands of icamd_attention_fwd / _bwd,
the forward + backward launch on guarded, NaN-filled outputs, and the digest of a case.  Importing it needs no GPU."""
import torch

from _harness import DEV, digest, guarded, hip, intact, rnd_bf16

D = 64
SCALE = D ** -0.5


def run(lib, qkv, dout, B, T, H):
    """Forward + backward on guarded outputs.  Returns (rc_fwd, rc_bwd, out, lse, delta, dqkv) and asserts the bands."""
    h = hip()
    qd = qkv.to(torch.bfloat16).to(DEV).contiguous()
    dd = dout.to(torch.bfloat16).to(DEV).contiguous()
    nan = float("nan")
    out, out_g = guarded((B * T, H * D), torch.bfloat16, nan)
    lse, lse_g = guarded((B, H, T), torch.float32, nan)
    delta, delta_g = guarded((B, H, T), torch.float32, nan)
    dqkv, dqkv_g = guarded((B * T, 3 * H * D), torch.bfloat16, nan)
    rc_f = lib.icamd_attention_fwd(h.ptr(qd), h.ptr(out), h.ptr(lse), B, T, H, D, SCALE, h.stream_ptr())
    rc_b = lib.icamd_attention_bwd(h.ptr(qd), h.ptr(out), h.ptr(dd), h.ptr(lse), h.ptr(delta), h.ptr(dqkv), B, T, H, D,
                                   SCALE, h.stream_ptr())
    assert intact(out_g), "guard band behind out written"
    assert intact(lse_g), "guard band behind lse written"
    assert intact(delta_g), "guard band behind delta written"
    assert intact(dqkv_g), "guard band behind dqkv written"
    return rc_f, rc_b, out, lse, delta, dqkv


def operands(B, T, H):
    return rnd_bf16(B * T, 3 * H * D, scale=1.0, seed=120), rnd_bf16(B * T, H * D, seed=121)


def digest_case(lib, B, T, H):
    qkv, dout = operands(B, T, H)
    rc_f, rc_b, out, lse, delta, dqkv = run(lib, qkv, dout, B, T, H)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    return digest(out, lse, delta, dqkv)
