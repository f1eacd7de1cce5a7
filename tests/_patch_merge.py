"""Shared by tests/test_patch_merge_gpu.py and tests/test_multitrip_gpu.py: seeded operands of icamd_patch_merge_ln_fwd / _bwd and the
forward + backward launch on guarded, NaN-filled outputs.  Importing it needs no GPU."""
import torch

from _harness import DEV, guarded, hip, intact, rnd_bf16
from oracle import ops_ref as R

EPS = 1e-5


def operands(N, H, W, C):
    g = torch.Generator().manual_seed(100)
    x = R.bf16_round(rnd_bf16(N, H, W, C, scale=2.0, seed=101) + 0.5)
    gamma = torch.rand(4 * C, generator=g) + 0.5
    beta = torch.randn(4 * C, generator=g) * 0.2
    dy = rnd_bf16(N * (H // 2) * (W // 2), 4 * C, seed=102)
    return x, gamma, beta, dy


def run(lib, N, H, W, C, accs=(0,)):
    h = hip()
    x, gamma, beta, dy = operands(N, H, W, C)
    rows = N * (H // 2) * (W // 2)
    xd, gd, bd, dyd = x.to(torch.bfloat16).to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(torch.bfloat16).to(DEV)
    nan = float("nan")
    y, y_g = guarded((rows, 4 * C), torch.bfloat16, nan)
    y = y.view(-1)
    mean, rstd = torch.full((rows,), nan, device=DEV), torch.full((rows,), nan, device=DEV)
    rc_f = lib.icamd_patch_merge_ln_fwd(h.ptr(xd), h.ptr(gd), h.ptr(bd), h.ptr(y), h.ptr(mean), h.ptr(rstd), N, H, W, C,
                                        EPS, h.stream_ptr())
    wsb = max(int(lib.icamd_patch_merge_ln_bwd_workspace_bytes(N, H, W, C)), 256)
    wsp = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dx, dx_g = guarded((N * H * W, C), torch.bfloat16, nan)
    dx = dx.view(-1)
    dg, db = torch.ones(4 * C, device=DEV), torch.ones(4 * C, device=DEV)
    grads = []
    rc_b = 0
    for acc in accs:
        rc_b = lib.icamd_patch_merge_ln_bwd(h.ptr(dyd), h.ptr(xd), h.ptr(mean), h.ptr(rstd), h.ptr(gd), h.ptr(dx),
                                            h.ptr(dg), h.ptr(db), N, H, W, C, acc, h.ptr(wsp), wsb, h.stream_ptr())
        torch.cuda.synchronize()
        grads.append((dg.cpu().clone(), db.cpu().clone()))
    assert intact(y_g), "guard band behind y written"
    assert intact(dx_g), "guard band behind dx written"
    return rc_f, rc_b, y, mean, rstd, dx, grads
