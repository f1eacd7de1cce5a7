// Token-wise kernels for the transformer / ConvNeXt branches of the step (gfx950): LayerNorm forward / backward over
// the channel dimension of [rows][C] bf16 tensors, exact (erf) GELU forward / backward, and a two-level column sum
// (bias gradients).  LayerNorm: 16 / 32 / 64 lanes per row by channel count, 16 B per lane, statistics by xor-shuffles
// in fp32 (two-pass variance, as torch.nn.functional.layer_norm), fp32 mean / rstd saved for backward.
// Replaces what ATen runs for timm's LayerNorm / GELU / Linear-bias layers under `model(samples)` and
// `loss.backward()` (/root/reference/engine.py:48,51,64,72; ConvNeXt block spec
// /root/reference/semantic_segmentation/backbone/convnext.py:43-56,158-182).
// once-read streams of this translation unit use non-temporal loads (round 5: ViT-B/16 34.9-35.0 -> 34.7 ms, ResNet-50 -0.03..-0.06 ms
// in two A/B pairs each; dwconv.hip measured worse with them and keeps the default)
#define ICAMD_STREAM_NT 1
#include "common.h"
#include "icamd_internal.h"

namespace {

constexpr int LN_MAX_C = 1024;   // two 16 B vectors per lane at 64 lanes per row

// LayerNorm rows are short (96 ... 768 channels): a whole wave per row leaves most lanes idle for ConvNeXt's 96 / 192
// channels.  LPR lanes (16, 32 or 64) share a row, 64 / LPR rows are in flight per wave, each lane holds up to two
// 8-channel vectors (16 B loads), statistics are reduced by xor-shuffles inside the lane group.
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
template <int LPR>
__device__ __forceinline__ float cross_group_sum(float v) {   // same lane position of every group in the wave
#pragma unroll
  for (int m = LPR; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = bf16_lo(v[e]); f[2 * e + 1] = bf16_hi(v[e]); }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
  return o;
}

// y = (x - mean) * rstd * gamma + beta (two-pass variance in registers, as torch.nn.functional.layer_norm)
// NV (round 4): 16 B vectors per lane, 1 when the row fits LPR vectors (C <= 8 * LPR: every ConvNeXt-T LayerNorm but the 768-wide
// ones) -- half the registers of the two-vector form, twice the waves in flight for kernels that live on loads in flight.
template <int LPR, int NV>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                            long long rows, int C, float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LPR, grp = lane / LPR;
  const int nvec = C >> 3;
  bool has[NV];
#pragma unroll
  for (int it = 0; it < NV; ++it) has[it] = sub + it * LPR < nvec;
  float g[NV][8], bt[NV][8];
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int c = (has[it] ? sub + it * LPR : 0) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { g[it][e] = gamma[c + e]; bt[it][e] = beta[c + e]; }
  }
  const float invC = 1.f / (float)C;
  const long long stride = (long long)gridDim.x * 4 * RPW;
  for (long long rbase = ((long long)blockIdx.x * 4 + wave) * RPW; rbase < rows; rbase += stride) {
    const long long row = rbase + grp;
    const bool live = row < rows;
    const bf16_t* xr = x + (live ? row : 0) * C;
    float v[NV][8];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it) {
      u32x4 raw = {0u, 0u, 0u, 0u};
      if (has[it] && live) raw = ld_stream((const u32x4*)(xr + (sub + it * LPR) * 8));
      unpack8(raw, v[it]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[it][e];
    }
    const float mean = group_sum<LPR>(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it)
      if (has[it]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[it][e] - mean; q += d * d; }
      }
    const float rstd = rsqrtf(group_sum<LPR>(q) * invC + eps);
    if (!live) continue;
    if (sub == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    bf16_t* yr = y + row * C;
#pragma unroll
    for (int it = 0; it < NV; ++it)
      if (has[it]) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[it][e] - mean) * rstd * g[it][e] + bt[it][e];
        *(u32x4*)(yr + (sub + it * LPR) * 8) = pack8(o);
      }
  }
}

// dx = rstd * (dy*gamma - mean_C(dy*gamma) - xhat * mean_C(dy*gamma*xhat)) (+ addend); per-workgroup partial column
// sums of dy (-> dbeta) and dy*xhat (-> dgamma) in part[blk][2][C].  Each wave walks `rows_per_wave` rows, 64/LPR at a time.
template <int LPR, int NV>
__global__ __launch_bounds__(256, NV == 1 ? 4 : (NV == 2 ? 3 : 2)) void layernorm_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const bf16_t* __restrict__ addend,
                                                            bf16_t* __restrict__ dx, float* __restrict__ part, long long rows,
                                                            int C, int rows_per_wave) {
  constexpr int RPW = 64 / LPR;
  __shared__ float red[4][2][LN_MAX_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LPR, grp = lane / LPR;
  const int nvec = C >> 3;
  bool has[NV];
#pragma unroll
  for (int it = 0; it < NV; ++it) has[it] = sub + it * LPR < nvec;
  // Column sums (d beta, d gamma) and gamma as PACKED pairs in the order the 16 B vectors hold them (element 2e in .x, 2e + 1
  // in .y): every pair the packed-fp32 instructions see is then a natural VGPR pair and no op_sel swizzle is needed.  That is
  // a correctness matter on this part, not a style one -- see the note at the accumulation below.
  f32x2 g2[NV][4], sb[NV][4], sg[NV][4];
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int c = (has[it] ? sub + it * LPR : 0) * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g2[it][e] = f32x2{gamma[c + 2 * e], gamma[c + 2 * e + 1]};
      sb[it][e] = f32x2{0.f, 0.f};
      sg[it][e] = f32x2{0.f, 0.f};
    }
  }
  const float invC = 1.f / (float)C;
  const long long r0 = ((long long)blockIdx.x * 4 + wave) * rows_per_wave;
  const long long r1 = (rows < r0 + rows_per_wave) ? rows : r0 + rows_per_wave;
  // Software-pipelined over rows: the raw vectors (dy, x, addend) and statistics of the NEXT row group are requested
  // before the current one is reduced, so every wave keeps two rows of loads in flight (the kernel is latency-bound at
  // the 12 waves per CU its registers allow).
  u32x4 nd[NV], nx[NV], na[NV];
  float nmu = 0.f, nrs = 0.f;
  auto fetch = [&](long long rbase) {
    const long long row = rbase + grp;
    const bool live = row < r1;
    const long long ro = (live ? row : 0) * C;
    nmu = live ? mean[row] : 0.f;
    nrs = live ? rstd[row] : 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it) {
      nd[it] = u32x4{0u, 0u, 0u, 0u}; nx[it] = nd[it]; na[it] = nd[it];
      if (has[it] && live) {
        nd[it] = ld_stream((const u32x4*)(dy + ro + (sub + it * LPR) * 8));
        nx[it] = ld_stream((const u32x4*)(x + ro + (sub + it * LPR) * 8));
        if (addend != nullptr) na[it] = ld_stream((const u32x4*)(addend + ro + (sub + it * LPR) * 8));
      }
    }
  };
  if (r0 < r1) fetch(r0);
  for (long long rbase = r0; rbase < r1; rbase += RPW) {
    const long long row = rbase + grp;
    const bool live = row < r1;
    const long long ro = (live ? row : 0) * C;
    const float mu = nmu, rs = nrs;
    u32x4 rd[NV], rx[NV], ra[NV];
#pragma unroll
    for (int it = 0; it < NV; ++it) { rd[it] = nd[it]; rx[it] = nx[it]; ra[it] = na[it]; }
    if (rbase + RPW < r1) fetch(rbase + RPW);
    f32x2 dyg[NV][4], xh[NV][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it) {
      const bool on = has[it] && live;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x2 d = {bf16_lo(rd[it][e]), bf16_hi(rd[it][e])};
        const f32x2 xv = {bf16_lo(rx[it][e]), bf16_hi(rx[it][e])};
        const f32x2 xn = (xv - mu) * rs;
        xh[it][e] = f32x2{on ? xn.x : 0.f, on ? xn.y : 0.f};
        dyg[it][e] = d * g2[it][e];
        const f32x2 p = dyg[it][e] * xh[it][e];
        s1 += dyg[it][e].x + dyg[it][e].y;
        s2 += p.x + p.y;
        // HARDWARE NOTE (round 4, tools/hazard_probe/, DESIGN 5 "round-4 finding 1"): written element by element
        // (sb[8] += d[e]), hipcc's SLP vectoriser paired the sums across vector boundaries and emitted
        // `v_pk_add_f32 vD, vD, vS op_sel:[0,1] op_sel_hi:[1,0]`.  On this MI355X a packed-fp32 instruction whose LOW result
        // takes the HIGH register of a source pair returns a wrong low result in lanes 48-63 while another wave of the SIMD
        // executes MFMAs with VGPR accumulators (the weight-gradient stream): a few rows of the 192-channel instance lost one
        // row's value.  Natural pairs need no op_sel; tools/isa_lint.py fails the build if one ever appears again.
        sb[it][e] += d;
        sg[it][e] += d * xh[it][e];
      }
    }
    const float c1 = group_sum<LPR>(s1) * invC, c2 = group_sum<LPR>(s2) * invC;
    if (!live) continue;
#pragma unroll
    for (int it = 0; it < NV; ++it)
      if (has[it]) {
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f32x2 o = (dyg[it][e] - c1 - xh[it][e] * c2) * rs;
          if (addend != nullptr) o += f32x2{bf16_lo(ra[it][e]), bf16_hi(ra[it][e])};   // the skip connection's gradient joins here
          ov[e] = pack_bf16x2(o.x, o.y);
        }
        *(u32x4*)(dx + ro + (sub + it * LPR) * 8) = ov;
      }
  }
  // fold: lane groups of the wave (fixed xor order), then the 4 waves in wave order; one partial row per workgroup
#pragma unroll
  for (int it = 0; it < NV; ++it)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float b = cross_group_sum<LPR>(sb[it][e >> 1][e & 1]), gg = cross_group_sum<LPR>(sg[it][e >> 1][e & 1]);
      if (grp == 0 && has[it]) {
        red[wave][0][(sub + it * LPR) * 8 + e] = b;
        red[wave][1][(sub + it * LPR) * 8 + e] = gg;
      }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int which = i / C, c = i - which * C;
    const float s = (red[0][which][c] + red[1][which][c]) + (red[2][which][c] + red[3][which][c]);
    part[((long long)blockIdx.x * 2 + which) * C + c] = s;
  }
}

__global__ __launch_bounds__(256) void gelu_fwd_kernel(const bf16_t* __restrict__ z, bf16_t* __restrict__ a, long long nvec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const u32x4 v = ld_stream((const u32x4*)z + i);
    ((u32x4*)a)[i] = gelu8(v);
  }
}

// dz = da * gelu'(z); optional per-workgroup column sums of dz (the preceding Linear's bias gradient):
// part[blk][2][C] (second row zero) -- the launcher makes the grid stride a multiple of C/8
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const bf16_t* __restrict__ da, const bf16_t* __restrict__ z,
                                                       bf16_t* __restrict__ dz, long long nvec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const u32x4 g = ld_stream((const u32x4*)da + i);
    const u32x4 v = ld_stream((const u32x4*)z + i);
    ((u32x4*)dz)[i] = gelu_bwd8(g, v);
  }
}

// column sums of x [rows][ld] (first `cols` columns, cols % 8 == 0): per-workgroup partial rows part[blk][2][cols]
// (second row zero so the BatchNorm reduce+finalize kernel can fold them)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const bf16_t* __restrict__ x, float* __restrict__ part,
                                                             long long rows, int ld, int cols, int rows_per_block) {
  __shared__ float red[256 * 8];
  const int cpr = cols >> 3;
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = (rows < r0 + rows_per_block) ? rows : r0 + rows_per_block;
  for (int cg0 = 0; cg0 < cpr; cg0 += 256) {
    const int tcols = (cpr - cg0 < 256) ? (cpr - cg0) : 256;
    const int rlanes = 256 / tcols;
    const int cgi = tid % tcols, rl = tid / tcols;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (rl < rlanes) {
      for (long long r = r0 + rl; r < r1; r += rlanes) {
        const u32x4 v = ld_stream((const u32x4*)(x + r * ld + (cg0 + cgi) * 8));
#pragma unroll
        for (int e = 0; e < 4; ++e) { s[2 * e] += bf16_lo(v[e]); s[2 * e + 1] += bf16_hi(v[e]); }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = s[e];
    __syncthreads();
    for (int o = tid; o < tcols * 8; o += 256) {
      const int cgo = o >> 3, e = o & 7;
      float t = 0.f;
      for (int l = 0; l < rlanes; ++l) t += red[(l * tcols + cgo) * 8 + e];
      part[((long long)blockIdx.x * 2 + 0) * cols + (cg0 + cgo) * 8 + e] = t;
      part[((long long)blockIdx.x * 2 + 1) * cols + (cg0 + cgo) * 8 + e] = 0.f;
    }
    __syncthreads();
  }
}

// ViT token assembly: tok[b][0] = cls + pos[0]; tok[b][1+i] = patch[b][i] + pos[1+i]   (C % 8 == 0)
__global__ __launch_bounds__(256) void vit_tokens_fwd_kernel(const bf16_t* __restrict__ patches, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, bf16_t* __restrict__ tok, int B,
                                                             int T, int C) {
  const int cpr = C >> 3;
  const long long total = (long long)B * T * cpr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int cg = (int)(i % cpr);
    const long long row = i / cpr;
    const int t = (int)(row % T);
    const int b = (int)(row / T);
    float v[8];
    if (t == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = cls[cg * 8 + e];
    } else {
      const u32x4 p = ((const u32x4*)patches)[((long long)b * (T - 1) + (t - 1)) * cpr + cg];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[2 * e] = bf16_lo(p[e]); v[2 * e + 1] = bf16_hi(p[e]); }
    }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = pack_bf16x2(v[2 * e] + pos[(long long)t * C + cg * 8 + 2 * e], v[2 * e + 1] + pos[(long long)t * C + cg * 8 + 2 * e + 1]);
    ((u32x4*)tok)[i] = o;
  }
}

// out[j] = (accumulate ? out[j] : 0) + sum_b x[b*stride + j], j < n (n % 8 == 0): gradients of cls_token / pos_embed
__global__ __launch_bounds__(256) void batch_sum_kernel(const bf16_t* __restrict__ x, long long stride, int B, long long n8,
                                                        float* __restrict__ out, int accumulate) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  for (int b = 0; b < B; ++b) {
    const u32x4 v = *(const u32x4*)(x + (long long)b * stride + i * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[2 * e] += bf16_lo(v[e]); s[2 * e + 1] += bf16_hi(v[e]); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) out[i * 8 + e] = accumulate ? out[i * 8 + e] + s[e] : s[e];
}

// dst[r][0..C) = src[r][0..C) for r < rows, with independent row strides (elements; C % 8 == 0)
__global__ __launch_bounds__(256) void strided_rows_copy_kernel(const bf16_t* __restrict__ src, long long sstride,
                                                                bf16_t* __restrict__ dst, long long dstride, long long rows,
                                                                long long c8) {
  const long long total = rows * c8;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long r = i / c8, c = i - r * c8;
    *(u32x4*)(dst + r * dstride + c * 8) = *(const u32x4*)(src + r * sstride + c * 8);
  }
}

inline unsigned int ew_grid(long long nvec) {
  long long blocks = (nvec + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  return (unsigned int)blocks;
}

}  // namespace

static inline int ln_lanes_per_row(int C) { return C <= 128 ? 16 : (C <= 256 ? 32 : 64); }
// round 5: rows of 3 * 2^k vectors (every ConvNeXt width and ViT-B's 768: 12 / 24 / 48 / 96 vectors) as THREE vectors per lane on
// 4 / 8 / 16 / 32 lanes -- no idle lanes (the one- and two-vector forms leave a quarter of them idle on these widths; the two-vector
// backward also spilled 3-4 registers at its three workgroups per CU).  Measured, two A/B pairs on one box: ViT-B/16 (C = 768)
// 35.93 / 36.02 -> 35.60 / 35.62 ms with both directions on the three-vector form, forward alone -0.1, backward alone -0.15;
// ConvNeXt-T (C = 96 ... 384, one vector per lane today) 26.8-27.0 either way -- so only the 768-wide rows take it by default.
// ICAMD_LN_NV3: bit 0 forward, bit 1 backward (default 3), bit 2 every eligible width.
static inline int ln_nv3_lanes(int C, int mode_bit) {
  static const int mode = icamd_env_int("ICAMD_LN_NV3", 3);
  const int nvec = C >> 3;
  if (!(mode & mode_bit) || nvec % 3 != 0) return 0;
  const int l = nvec / 3;
  if (l == 32) return l;
  return ((mode & 4) && (l == 4 || l == 8 || l == 16)) ? l : 0;
}

int icamd_layernorm_fwd_launch(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                               long long rows, int C, float eps, hipStream_t s) {
  if (C % 8 != 0 || C > LN_MAX_C || C <= 0) return ICAMD_ERR_UNSUPPORTED;
  const int lpr = ln_lanes_per_row(C);
  long long blocks = (rows + 4 * (64 / lpr) - 1) / (4 * (64 / lpr));
  if (blocks > 2048) blocks = 2048;   // grid-stride beyond: 8 workgroups per CU keep enough loads in flight
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks), block(256);
  const bool one = C <= 8 * lpr;   // one 16 B vector per lane
#define ICAMD_LN_FWD(L, V) hipLaunchKernelGGL((layernorm_fwd_kernel<L, V>), grid, block, 0, s, x, gamma, beta, y, mean, rstd, rows, C, eps)
  if (const int l3 = ln_nv3_lanes(C, 1)) {
    long long b3 = (rows + 4 * (64 / l3) - 1) / (4 * (64 / l3));
    if (b3 > 2048) b3 = 2048;
    const dim3 grid((unsigned)(b3 < 1 ? 1 : b3));
    if (l3 == 4) ICAMD_LN_FWD(4, 3); else if (l3 == 8) ICAMD_LN_FWD(8, 3); else if (l3 == 16) ICAMD_LN_FWD(16, 3); else ICAMD_LN_FWD(32, 3);
    return icamd_launch_status();
  }
  if (lpr == 16) { if (one) ICAMD_LN_FWD(16, 1); else ICAMD_LN_FWD(16, 2); }
  else if (lpr == 32) { if (one) ICAMD_LN_FWD(32, 1); else ICAMD_LN_FWD(32, 2); }
  else { if (one) ICAMD_LN_FWD(64, 1); else ICAMD_LN_FWD(64, 2); }
#undef ICAMD_LN_FWD
  return icamd_launch_status();
}

int icamd_layernorm_bwd_blocks(long long rows) {
  // ~1024 workgroups of 4 waves, at least one row per wave
  long long waves = (rows < 4096) ? rows : 4096;
  return (int)((waves + 3) / 4);
}

int icamd_layernorm_bwd_launch(const bf16_t* dy, const bf16_t* x, const float* mean, const float* rstd, const float* gamma,
                               const bf16_t* addend, bf16_t* dx, float* part, long long rows, int C, hipStream_t s) {
  if (C % 8 != 0 || C > LN_MAX_C || C <= 0) return ICAMD_ERR_UNSUPPORTED;
  const int nblk = icamd_layernorm_bwd_blocks(rows);
  const int rpw = (int)((rows + (long long)nblk * 4 - 1) / ((long long)nblk * 4));
  const int lpr = ln_lanes_per_row(C);
  const dim3 grid((unsigned)nblk), block(256);
  const bool one = C <= 8 * lpr;
#define ICAMD_LN_BWD(L, V) \
  hipLaunchKernelGGL((layernorm_bwd_kernel<L, V>), grid, block, 0, s, dy, x, mean, rstd, gamma, addend, dx, part, rows, C, rpw)
  if (const int l3 = ln_nv3_lanes(C, 2)) {
    if (l3 == 4) ICAMD_LN_BWD(4, 3); else if (l3 == 8) ICAMD_LN_BWD(8, 3); else if (l3 == 16) ICAMD_LN_BWD(16, 3); else ICAMD_LN_BWD(32, 3);
    return icamd_launch_status();
  }
  if (lpr == 16) { if (one) ICAMD_LN_BWD(16, 1); else ICAMD_LN_BWD(16, 2); }
  else if (lpr == 32) { if (one) ICAMD_LN_BWD(32, 1); else ICAMD_LN_BWD(32, 2); }
  else { if (one) ICAMD_LN_BWD(64, 1); else ICAMD_LN_BWD(64, 2); }
#undef ICAMD_LN_BWD
  return icamd_launch_status();
}

int icamd_gelu_fwd_launch(const bf16_t* z, bf16_t* a, long long numel, hipStream_t s) {
  if (numel % 8 != 0) return ICAMD_ERR_BAD_ARG;
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(ew_grid(numel / 8)), dim3(256), 0, s, z, a, numel / 8);
  return icamd_launch_status();
}

int icamd_gelu_bwd_launch(const bf16_t* da, const bf16_t* z, bf16_t* dz, long long numel, hipStream_t s) {
  if (numel % 8 != 0) return ICAMD_ERR_BAD_ARG;
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(ew_grid(numel / 8)), dim3(256), 0, s, da, z, dz, numel / 8);
  return icamd_launch_status();
}

int icamd_colsum_blocks(long long rows) {
  long long rpb = (rows + 1023) / 1024;
  if (rpb < 32) rpb = 32;
  return (int)((rows + rpb - 1) / rpb);
}

int icamd_colsum_partial_launch(const bf16_t* x, float* part, long long rows, int ld, int cols, hipStream_t s) {
  if (cols % 8 != 0 || ld % 8 != 0) return ICAMD_ERR_BAD_ARG;
  const int nblk = icamd_colsum_blocks(rows);
  const int rpb = (int)((rows + nblk - 1) / nblk);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, s, x, part, rows, ld, cols, rpb);
  return icamd_launch_status();
}

int icamd_vit_tokens_fwd_launch(const bf16_t* patches, const float* cls, const float* pos, bf16_t* tok, int B, int T, int C,
                                hipStream_t s) {
  if (C % 8 != 0) return ICAMD_ERR_BAD_ARG;
  hipLaunchKernelGGL(vit_tokens_fwd_kernel, dim3(ew_grid((long long)B * T * (C / 8))), dim3(256), 0, s, patches, cls, pos, tok, B,
                     T, C);
  return icamd_launch_status();
}

int icamd_batch_sum_launch(const bf16_t* x, long long stride, int B, long long n, float* out, int accumulate, hipStream_t s) {
  if (n % 8 != 0 || stride % 8 != 0) return ICAMD_ERR_BAD_ARG;
  const long long n8 = n / 8;
  hipLaunchKernelGGL(batch_sum_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, stride, B, n8, out, accumulate);
  return icamd_launch_status();
}

int icamd_strided_rows_copy_launch(const bf16_t* src, long long sstride, bf16_t* dst, long long dstride, long long rows,
                                   long long C, hipStream_t s) {
  if (C % 8 != 0 || sstride % 8 != 0 || dstride % 8 != 0) return ICAMD_ERR_BAD_ARG;
  hipLaunchKernelGGL(strided_rows_copy_kernel, dim3(ew_grid(rows * (C / 8))), dim3(256), 0, s, src, sstride, dst, dstride, rows,
                     C / 8);
  return icamd_launch_status();
}
