"""icamd_conv2d_fwd (with statistics), _dgrad (with and without addend) and _wgrad on the 1x1 problems MobileNetV2 brings: widths
down to 8 and others that are no multiple of 16 or 32 (8 -> 48 is blocks.1.0.conv_pw at width 0.35 / 0.5, 88 -> 528 its widest
expansion at 1.4 ... 320 -> 1280 the head), at N H W = 2 x 7 x 7 (one m-tile) and 3 x 29 x 29 (2523 rows: twenty 128-row statistic
rows, a ragged last tile).  Against oracle.ops_ref with the bounds of tests/test_kernels_gpu.py's convolution tests.  The kernels
are the general entries' own: nothing here is new code, no model had driven them at these widths."""
import ctypes

import pytest
import torch

import _harness
from _harness import DEV, dev, guarded, intact, rnd_bf16, sync
from _harness import lib  # noqa: F401
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = [(8, 48), (48, 8), (16, 96), (144, 24), (24, 144), (88, 528), (320, 1280)]
PIXELS = [(2, 7, 7), (3, 29, 29)]
CASES = [(n, h, w, cin, cout) for n, h, w in PIXELS for cin, cout in WIDTHS]


@pytest.mark.parametrize("case", CASES)
def test_pointwise_fwd_dgrad_wgrad(lib, case):
    hip = _harness.hip()
    N, H, W, Cin, Cout = case
    d = hip.conv_desc(N, H, W, Cin, Cout, 1, 1, 1, 0)
    x = rnd_bf16(N, H, W, Cin, seed=1)
    w = rnd_bf16(Cout, 1, 1, Cin, scale=(1.0 / Cin) ** 0.5, seed=2)
    xd, wd = dev(x), dev(w)
    # forward with statistics
    ref = R.conv2d_fwd(x, w, 1, 0)
    y, gy = guarded((N, H, W, Cout), torch.bfloat16)
    rows = lib.icamd_conv2d_stats_rows(ctypes.byref(d))
    stats, gs = guarded((rows, 2, Cout), torch.float32)
    assert lib.icamd_conv2d_fwd(ctypes.byref(d), hip.ptr(xd), hip.ptr(wd), hip.ptr(y), None, None, hip.ptr(stats), hip.stream_ptr()) == 0
    assert intact(gy) and intact(gs)
    got = y.float().cpu()
    print(f"{case}: y rel_l2 {R.rel_l2(got, ref):.2e}")
    assert R.rel_l2(got, ref) <= 1e-3 and R.bf16_close(got, ref)
    s1, s2 = R.conv2d_stats(got)
    st_sum = stats.double().sum(0).cpu()
    assert torch.allclose(st_sum[0], s1, rtol=1e-5, atol=1e-3) and torch.allclose(st_sum[1], s2, rtol=1e-5, atol=1e-3)
    # data gradient without and with the residual addend
    dy = rnd_bf16(N, H, W, Cout, seed=5)
    wdg = rnd_bf16(Cout, 1, 1, Cin, scale=(1.0 / Cout) ** 0.5, seed=6)
    addend = rnd_bf16(N, H, W, Cin, seed=7)
    dyd, wtd = dev(dy), dev(wdg.permute(3, 1, 2, 0).contiguous())      # [Cin][1][1][Cout]
    for use_add in (False, True):
        rdx = R.conv2d_dgrad(dy, wdg, (H, W), 1, 0, addend if use_add else None)
        dx, gx = guarded((N, H, W, Cin), torch.bfloat16)
        ad = dev(addend) if use_add else None
        assert lib.icamd_conv2d_dgrad(ctypes.byref(d), hip.ptr(dyd), hip.ptr(wtd), hip.ptr(dx), hip.ptr(ad), None, hip.stream_ptr()) == 0
        assert intact(gx)
        gdx = dx.float().cpu()
        print(f"{case}: dx rel_l2 {R.rel_l2(gdx, rdx):.2e} (addend {use_add})")
        assert R.rel_l2(gdx, rdx) <= 1e-3 and R.bf16_close(gdx, rdx)
    # weight gradient, then accumulated on top
    rdw = R.conv2d_wgrad(x, dy, (1, 1), 1, 0)
    wsb = lib.icamd_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw, gw = guarded((Cout, 1, 1, Cin), torch.float32, fill=1.0)
    for acc, expect in ((0, rdw), (1, 2 * rdw)):
        assert lib.icamd_conv2d_wgrad(ctypes.byref(d), hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw), acc, hip.ptr(ws), wsb, hip.stream_ptr()) == 0
        sync()
        print(f"{case}: dw rel_l2 {R.rel_l2(dw.cpu(), expect):.2e} (accumulate {acc})")
        assert R.rel_l2(dw.cpu(), expect) <= 1e-4
    assert intact(gw)
