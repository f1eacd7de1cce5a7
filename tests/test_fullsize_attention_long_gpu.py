"""icamd_attention_fwd / _bwd at the size ViT-B/16 trains at above 224^2: B = 64 images of 384^2 (T = 577 tokens, 12 heads:
768 (image, head) pairs x 5 blocks of 128 rows = 3840 workgroups per kernel, several rounds of every CU, in the XCD-grouped order
of csrc/attention_long.hip), default routing.  A subset of the images is compared with oracle/ops_ref.py accumulated in fp64 on
the GPU, under the bounds tests/test_fullsize_layers_gpu.py applies to the same entries at T = 197 (vit_attention there)."""
import pytest
import torch

from _fullsize_check import check_bf16, check_close, require
from _harness import default_routing_lib as lib  # noqa: F401
from _harness import rnd_dev as rnd
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
B, T, H, D = 64, 577, 12, 64


def test_vit_b16_384_attention_768_pairs(lib):
    """The reference covers images 0, 21 and 32 and the last eight: the first and last pairs of the grid, pairs in its middle, and --
    pairs 672-767 -- the last workgroups every XCD runs."""
    from imageclassification_amd import hip
    scale = D ** -0.5
    seed = 7300
    qkv = rnd((B * T, 3 * H * D), seed)
    out = torch.full((B * T, H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, T), float("nan"), device=DEV)
    s = hip.stream_ptr()
    assert lib.icamd_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, T, H, D, scale, s) == 0, "attention fwd"
    dout = rnd((B * T, H * D), seed + 1)
    delta = torch.full((B, H, T), float("nan"), device=DEV)
    dqkv = torch.full((B * T, 3 * H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib.icamd_attention_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(),
                                   B, T, H, D, scale, s) == 0, "attention bwd"
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(delta).all())
    imgs = torch.tensor([0, 21, 32] + list(range(56, 64)), device=DEV)
    nb = len(imgs)
    sub = lambda t: t.reshape(B, T, -1)[imgs].reshape(nb * T, -1)   # noqa: E731
    ro, rlse = R.attention_fwd(sub(qkv), nb, T, H, D, scale, acc=F64)
    require(check_close(lse[imgs], rlse, 1e-4, 1e-4, "lse"), "attention lse")
    # max_frac: test_kernels_gpu.py's rule for these entries (1e-6 wherever B * H > 256; here 768 pairs)
    require(check_bf16(sub(out).float(), ro, rel=3e-3, block_rel=3e-3, atol_rms=8e-3, max_frac=1e-6), "attention fwd")
    rd = R.attention_bwd(sub(qkv), sub(dout), nb, T, H, D, scale, acc=F64)
    got = sub(dqkv).float()
    for name, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, 2 * H * D)), ("dv", slice(2 * H * D, 3 * H * D))):
        fails = [f for f in check_bf16(got[:, sl].contiguous(), rd[:, sl].contiguous(), rel=6e-3, block_rel=6e-3)
                 if "elementwise" not in f]    # test_kernels_gpu.py bounds the gradient by rel L2 only
        require(fails, f"attention bwd {name}")
