"""GPU box: the attention kernels, forward and backward, with a correctness check against torch's fp32 softmax attention on a
few images.  Default shape: ViT-B/16's (batch 256, T = 197, 12 heads of 64).

usage: python tools/bench_attn.py [batch] [reps] [heads] [--tokens T] [--sdpa] [--no-split]
  --tokens T   sequence length (197; T > 208 runs on the tiled kernels of csrc/attention_long.hip, ICAMD_ATTN_LONG=2 forces them)
  --sdpa       also time torch.nn.functional.scaled_dot_product_attention (bf16, same shape) forward and forward+backward: context
               only -- what it dispatches to depends on the torch build
  --no-split   skip the torch.profiler pass that splits the backward into its two kernels (dQ + delta, dK / dV)
FLOPs: 4 T^2 64 per head forward (two products), 10 T^2 64 backward (five products); the dQ kernel computes three products and the
dK / dV kernel four (S and dP are recomputed), so the per-kernel TFLOP/s are quoted on 6 T^2 64 and 8 T^2 64 EXECUTED flops."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from imageclassification_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=256)
ap.add_argument("reps", nargs="?", type=int, default=10)
ap.add_argument("heads", nargs="?", type=int, default=12)
ap.add_argument("--tokens", type=int, default=197)
ap.add_argument("--sdpa", action="store_true")
ap.add_argument("--no-split", action="store_true")
args = ap.parse_args()

hip.require_gpu()
lib = hip.load(); s = hip.stream_ptr()
B, reps, T, H, D = args.batch, args.reps, args.tokens, args.heads, 64
scale = D ** -0.5
g = torch.Generator(device="cuda").manual_seed(3)
qkv = (torch.randn(B * T, 3 * H * D, device="cuda", generator=g)).bfloat16()
dout = (torch.randn(B * T, H * D, device="cuda", generator=g) * 0.1).bfloat16()
out = torch.empty(B * T, H * D, dtype=torch.bfloat16, device="cuda")
lse = torch.empty(B, H, T, device="cuda"); delta = torch.empty_like(lse)
dqkv = torch.empty_like(qkv)
def fwd(): hip.check(lib.icamd_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, T, H, D, scale, s))
def bwd(): hip.check(lib.icamd_attention_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, T, H, D, scale, s))
def timeit(fn):
    """us per call: three warm-up calls, then the median of five windows of `reps` calls between device events"""
    for _ in range(3): fn()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(ts)[2], min(ts), max(ts)
(tf, tf_lo, tf_hi), (tb, tb_lo, tb_hi) = timeit(fwd), timeit(bwd)
# reference on the first images
nb = min(4, B)
x = qkv[: nb * T].float().reshape(nb, T, 3, H, D).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)   # [3][nb][H][T][D]
q, k, v = x[0], x[1], x[2]
p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
o = (p @ v).permute(0, 2, 1, 3).reshape(nb * T, H * D)
o.backward(dout[: nb * T].float())
ref_d = x.grad.permute(1, 3, 0, 2, 4).reshape(nb * T, 3 * H * D)
e_o = ((out[: nb * T].float() - o).norm() / o.norm()).item()
e_d = ((dqkv[: nb * T].float() - ref_d).norm() / ref_d.norm()).item()
gf_f = 4.0 * B * H * T * T * D / 1e9
route = os.environ.get("ICAMD_ATTN_LONG", "unset")
print(f"attention B {B} T {T} H {H} (ICAMD_ATTN_LONG {route}): fwd {tf:.1f} us [{tf_lo:.1f}-{tf_hi:.1f}] ({gf_f / tf * 1e3:.0f} TFLOP/s), "
      f"bwd {tb:.1f} us [{tb_lo:.1f}-{tb_hi:.1f}] ({2.5 * gf_f / tb * 1e3:.0f} TFLOP/s on 5 products); "
      f"rel err out {e_o:.1e}, dqkv {e_d:.1e}")

if not args.no_split:
    # the two kernels of the backward, from the profiler's kernel records (a pass of its own: tracing slows the host)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps): bwd()
        torch.cuda.synchronize()
    rows = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0), e.count)
            for e in prof.key_averages() if "attn" in e.key]
    if not rows:
        print("  backward kernels: not measured (the profiler returned no kernel records)")
    for key, total, count in sorted(rows):
        us = total / max(count, 1)
        executed = (1.5 if "dq" in key else 2.0) * gf_f        # 6 / 8 T^2 64 per head
        short = re.search(r"attn\w*", key).group(0)
        print(f"  {short}: {us:.1f} us per launch over {count} launches ({executed / us * 1e3:.0f} TFLOP/s executed)")

if args.sdpa:
    F = torch.nn.functional
    x5 = qkv.reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    qs, ks, vs = (t.contiguous().requires_grad_(True) for t in (x5[0], x5[1], x5[2]))      # [B][H][T][D] bf16
    do = dout.reshape(B, T, H, D).permute(0, 2, 1, 3).contiguous()
    def sd_f():
        with torch.no_grad(): F.scaled_dot_product_attention(qs, ks, vs)
    def sd_fb(): F.scaled_dot_product_attention(qs, ks, vs).backward(do)
    (sf, _, _), (sfb, _, _) = timeit(sd_f), timeit(sd_fb)
    print(f"  torch SDPA (context only; contiguous [B][H][T][D] operands): fwd {sf:.1f} us ({gf_f / sf * 1e3:.0f} TFLOP/s), "
          f"fwd+bwd {sfb:.1f} us ({3.5 * gf_f / sfb * 1e3:.0f} TFLOP/s on 7 products)")
