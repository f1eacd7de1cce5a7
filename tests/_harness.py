"""What the GPU kernel tests share: the library fixtures, seeded operands, guard bands, digests.  One definition of each, so that a
new kernel-family test module imports them and no test module is imported by another.

Importing this module needs no GPU and makes no CUDA call; imageclassification_amd.hip is imported on first use.  A test module
takes the fixture it wants under the name `lib`:

    from _harness import lib  # noqa: F401
    from _harness import default_routing_lib as lib  # noqa: F401      (modules that check the default routing)
"""
import hashlib
import os

import pytest
import torch

from oracle import ops_ref as R

DEV = "cuda"
UNSUPPORTED = 2                                    # ICAMD_ERR_UNSUPPORTED of include/icamd.h
BAND = 4096                                        # guard elements behind an output, at least; at least 64 rows of it
SENT = {1: 0x5A, 2: 0x5A5B, 4: 0x4B5A5B5C}         # band pattern by element size (finite values no kernel produces by accident)
INT = {1: torch.int8, 2: torch.int16, 4: torch.int32}


def hip():
    from imageclassification_amd import hip as module
    return module


def load_lib():
    hip().require_gpu()
    return hip().load()


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def default_routing_lib():
    routed = sorted(k for k in os.environ if k.startswith("ICAMD_"))
    # a routing switch in the environment would test some other route than the default: a failure, not a skip
    assert not routed, f"this module checks the default routing; unset {routed}"
    return load_lib()


@pytest.fixture(autouse=True)
def free_after_each():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def sync():
    torch.cuda.synchronize()


def rnd_bf16(*shape, scale=1.0, seed=0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return R.bf16_round(torch.randn(*shape, generator=g, device=device) * scale)


def rnd_dev(shape, seed, scale=1.0, relu=False, shift=0.0):
    """Seeded normal values on the GPU, rounded to bf16 (post-ReLU inputs: clamped at zero, so mask bits are non-trivial).
    scale = 1 and shift = 0 leave the draw untouched; otherwise one multiply and one add, in that order."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(shape, generator=g, device=DEV)
    if scale != 1.0 or shift != 0.0:
        t = t * scale + shift
    if relu:
        t = t.clamp_min(0)
    return t.to(torch.bfloat16)


def dev(t):
    return t.to(torch.bfloat16).to(DEV).contiguous()


def guarded(shape, dtype, fill=float("nan"), device=DEV):
    """a `fill`-ed tensor of `shape` with a band of sentinel elements behind it in the same allocation: max(BAND, 64 rows of
    shape[-1]) elements.  Returns (tensor, guard); intact(guard) says whether the band still holds the sentinel."""
    n = 1
    for s in shape:
        n *= s
    es = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((n + max(BAND, 64 * shape[-1]),), SENT[es], dtype=INT[es], device=device)
    view = whole[:n].view(dtype).view(*shape)
    view.fill_(fill)
    return view, (whole, n, SENT[es])


def intact(guard):
    whole, n, sentinel = guard
    if whole.is_cuda:
        torch.cuda.synchronize()
    return bool((whole[n:] == sentinel).all())


def digest(*tensors):
    """sha256 over the raw bytes of the tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()
