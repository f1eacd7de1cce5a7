"""tests/_harness.py on the CPU: the guard band catches a write behind the view and only that, digest() sees one bit, and the
seeded operands are the ones the kernel tests have always used."""
import pytest
import torch

import _window_attention as WA
from _harness import BAND, INT, SENT, digest, guarded, intact, rnd_bf16

NAN = float("nan")


@pytest.mark.parametrize("dtype,fill", [(torch.uint8, 0xA5), (torch.bfloat16, NAN), (torch.float32, NAN), (torch.float32, 1.5)])
@pytest.mark.parametrize("shape", [(5,), (3, 7), (2, 3, 100)])
def test_guard_band_sees_a_write_behind_the_view_and_only_that(dtype, fill, shape):
    view, guard = guarded(shape, dtype, fill, device="cpu")
    whole, n, sentinel = guard
    es = view.element_size()
    assert view.shape == shape and view.dtype == dtype and view.is_contiguous() and n == view.numel()
    assert bool(torch.isnan(view.float()).all()) if fill != fill else bool((view == fill).all())
    # one allocation: the band starts where the view ends
    assert whole.dtype == INT[es] and sentinel == SENT[es] and view.data_ptr() == whole.data_ptr()
    band = whole.numel() - n
    assert band == max(BAND, 64 * shape[-1]) == (4096 if shape[-1] <= 64 else 6400)
    assert intact(guard)
    view.view(-1)[0] = 2.0
    view.view(-1)[-1] = 3.0
    assert intact(guard), "a write inside the view is no write to the band"
    for pos in (n, n + band - 1):                      # directly behind the view; the last element of the band
        whole[pos] ^= 1
        assert not intact(guard), pos
        whole[pos] ^= 1
        assert intact(guard)


def test_digest_sees_one_bit_of_one_tensor():
    a, b = torch.arange(12, dtype=torch.float32).view(3, 4), torch.ones(5, dtype=torch.bfloat16)
    first = digest(a, b)
    assert digest(a.clone(), b.clone()) == first
    assert digest(a.t().contiguous().t(), b) == first          # equal bytes after .contiguous(), whatever the strides
    assert digest(b, a) != first
    flipped = b.clone()
    flipped.view(torch.int16)[3] ^= 1
    assert digest(a, flipped) != first


# Recorded with the helpers of commit 5e538c3 (rnd_bf16 and operands of its tests/test_window_attention_gpu.py) on the CPU: sha256 of
# the fp32 bytes.
PINNED = {
    "rnd_bf16(4, 8, seed=3)": "43c78c0a9d24d2290a7d386c11ee8acd8c486148411af91cfa2a6b4fb7f5a4e5",
    "rnd_bf16(3, 5, 7, scale=0.25, seed=120)": "286cc900e4559f41757d1dd6530365f17ce779c83944a1ad4c8212235cacfb4e",
    "qkv": "79407844496221f2304b283d74948de4fc5afcdab13818fbb22db564000ff640",
    "dout": "6d862cc8849d8a52c71c24cd3fbdca766caaf9b979846fff787e32c8f6152418",
    "bias": "82e31f9109a2a3bca28c501e5040b281a977452690f9a53d73473f89b5da3306",
}


def test_seeded_operands_are_the_ones_the_kernel_tests_have_always_used():
    qkv, dout, bias = WA.operands(2, 14, 14, 3, 7)
    got = {"rnd_bf16(4, 8, seed=3)": rnd_bf16(4, 8, seed=3),
           "rnd_bf16(3, 5, 7, scale=0.25, seed=120)": rnd_bf16(3, 5, 7, scale=0.25, seed=120),
           "qkv": qkv, "dout": dout, "bias": bias}
    for name, t in got.items():
        assert t.dtype == torch.float32 and t.device.type == "cpu"
        assert digest(t) == PINNED[name], name
    assert qkv.shape == (2 * 14 * 14, 3 * 3 * WA.D) and dout.shape == (2 * 14 * 14, 3 * WA.D) and bias.shape == (3, 49, 49)
