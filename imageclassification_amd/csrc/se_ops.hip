// Squeeze-and-excitation tail of a bottleneck block for gfx950 (timm Bottleneck with attn_layer='se': the gate sits on bn3's
// output, before the shortcut add):
//   z = y3*scale[c] + shift[c]      s = mean_hw(z)      h = relu(W1 s + b1)      e = sigmoid(W2 h + b2)
//   out = relu(z * e[n,c] + shortcut)
// z is never stored and never passed over: the pooled BatchNorm output is linear in the per-sample sums of the RAW convolution
// output, s = scale*(sum_hw y3)/HW + shift, and the gradient that reaches the excitation is linear in two per-sample sums,
// de = gamma * sum_hw(g*xhat) + beta * sum_hw(g).  So the tail costs the two passes over the block's widest tensor that the plain
// BatchNorm tail costs, forward (squeeze, gated apply) and backward (reduce, apply); everything else is [N,C]-sized.
//
// NHWC bf16 moved as 16 B (8-channel) vectors; a workgroup never straddles two samples; per-sample partial rows are folded in
// index order and every sum over samples is a serial loop in n: no float atomics, every output is bitwise repeatable.
#include "common.h"
#include "icamd_internal.h"
#include "workspace.h"
#include <stdlib.h>

namespace {

__device__ __forceinline__ u32x4 se_ld(const void* base, long long i) { return __builtin_nontemporal_load((const u32x4*)base + i); }

// ------------------------------------------------------------------------------------------------
// Per-sample column sums over one segment of a sample's HW rows.  blockIdx.x = n * S + seg.
//   NS = 1 (squeeze):  part[blk][C]    = sum y
//   NS = 2 (backward): part[blk][2][C] = sum g, sum g*xhat,   g = dout * maskbits
// thread -> (channel group, row lane) and the LDS fold over row lanes as bn_bwd_reduce_kernel (norm_pool.hip).
// ------------------------------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(256) void se_reduce_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ dout,
                                                        const unsigned char* __restrict__ maskbits,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        float* __restrict__ part, int HW, int C, int S, int rps) {
  constexpr int W = 8 * NS;
  __shared__ float red[256 * W];
  const int cpr = C >> 3;
  const int tid = threadIdx.x;
  const int n = blockIdx.x / S, seg = blockIdx.x - n * S;
  const int r0 = seg * rps;
  const int r1 = (HW < r0 + rps) ? HW : r0 + rps;
  const long long base = (long long)n * HW * cpr;
  for (int cg0 = 0; cg0 < cpr; cg0 += 256) {
    const int tcols = (cpr - cg0 < 256) ? (cpr - cg0) : 256;
    const int rlanes = 256 / tcols;
    const int cgi = tid % tcols, rl = tid / tcols;
    float acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.f;
    if (rl < rlanes) {
      const int c = (cg0 + cgi) * 8;
      float mu[8], is[8];
      if constexpr (NS == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { mu[e] = mean[c + e]; is[e] = invstd[c + e]; }
      }
#pragma unroll 4
      for (int r = r0 + rl; r < r1; r += rlanes) {
        const long long off = base + (long long)r * cpr + cg0 + cgi;
        const u32x4 yv = se_ld(y, off);
        float yy[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { yy[2 * e] = bf16_lo(yv[e]); yy[2 * e + 1] = bf16_hi(yv[e]); }
        if constexpr (NS == 1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += yy[e];
        } else {
          const u32x4 d = se_ld(dout, off);
          const unsigned int bits = maskbits != nullptr ? (unsigned int)maskbits[off] : 0xffu;
          float g[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { g[2 * e] = bf16_lo(d[e]); g[2 * e + 1] = bf16_hi(d[e]); }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (!((bits >> e) & 1u)) g[e] = 0.f;
            acc[e] += g[e];
            acc[8 + e] += g[e] * ((yy[e] - mu[e]) * is[e]);
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) red[tid * W + e] = acc[e];
    __syncthreads();
    for (int o = tid; o < tcols * W; o += 256) {
      const int cgo = o / W, e = o - cgo * W;
      float s = 0.f;
      for (int l = 0; l < rlanes; ++l) s += red[(l * tcols + cgo) * W + e];
      part[((long long)blockIdx.x * NS + (e >> 3)) * C + (cg0 + cgo) * 8 + (e & 7)] = s;
    }
    __syncthreads();
  }
}

// ysum[n][c] = sum over the S segment rows of sample n, in index order (fp64)
__global__ __launch_bounds__(256) void se_fold_kernel(const float* __restrict__ part, float* __restrict__ ysum, int N, int S, int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * C) return;
  const int n = (int)(i / C), c = (int)(i - (long long)n * C);
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += (double)part[((long long)n * S + k) * C + c];
  ysum[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------
// Excitation forward, one workgroup per sample: s = scale*ysum/HW + shift, h = relu(W1 s + b1), e = sigmoid(W2 h + b2).
// W1 [rd][C] rows are walked by a wave (16 B loads, wave_sum); W2 [C][rd] rows by groups of jw lanes (jw = the largest power of
// two <= min(rd, 64)) folded with xor shuffles.  Both folds have a fixed order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_excite_fwd_kernel(const float* __restrict__ ysum, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float inv_hw,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2,
                                                            float* __restrict__ s_out, float* __restrict__ h_out,
                                                            float* __restrict__ e_out, int C, int rd, int jw) {
  __shared__ __attribute__((aligned(16))) float s_l[4096];
  __shared__ float h_l[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) {
    const float v = fmaf(scale[c], ysum[(long long)n * C + c] * inv_hw, shift[c]);
    s_l[c] = v;
    s_out[(long long)n * C + c] = v;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < rd; j += 4) {
    const f32x4* row = (const f32x4*)(w1 + (long long)j * C);
    float acc = 0.f;
    for (int q = lane; q < (C >> 2); q += 64) {
      const f32x4 w = row[q];
      const f32x4 sv = *(const f32x4*)(s_l + 4 * q);
      acc += w[0] * sv[0] + w[1] * sv[1] + w[2] * sv[2] + w[3] * sv[3];
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      float v = acc + b1[j];
      v = v > 0.f ? v : 0.f;
      h_l[j] = v;
      h_out[(long long)n * rd + j] = v;
    }
  }
  __syncthreads();
  const int cper = 256 / jw;
  const int jl = tid % jw, cs = tid / jw;
  for (int c0 = 0; c0 < C; c0 += cper) {
    const int c = c0 + cs;
    float acc = 0.f;
    if (c < C)
      for (int j = jl; j < rd; j += jw) acc += w2[(long long)c * rd + j] * h_l[j];
    for (int o = jw >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (c < C && jl == 0) {
      const float v = acc + b2[c];
      e_out[(long long)n * C + c] = 1.f / (1.f + expf(-v));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// out = act((y*scale[c] + shift[c]) * e[n][c] (+ residual)); 8 channels per thread; grid (blocks per sample, N).  The residual,
// its on-the-fly BatchNorm and the mask bits are icamd_bn_apply's (norm_pool.hip); the gate multiplies the main branch only.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_bn_apply_kernel(const bf16_t* __restrict__ y, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ gate,
                                                          const bf16_t* __restrict__ residual, const float* __restrict__ res_scale,
                                                          const float* __restrict__ res_shift, bf16_t* __restrict__ out,
                                                          unsigned char* __restrict__ maskbits, int HW, int cpr, int relu) {
  const int n = blockIdx.y;
  const long long nvec = (long long)HW * cpr;
  const long long base = (long long)n * nvec;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // the launcher makes stride a multiple of cpr, so this thread's channel group never changes
  const int cg = (int)(i % cpr) * 8;
  const float* gn = gate + (long long)n * cpr * 8;
  float sc[8], sh[8], ge[8], rsc[8], rsh[8];
  const bool res_bn = res_scale != nullptr;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = scale[cg + e]; sh[e] = shift[cg + e]; ge[e] = gn[cg + e];
    rsc[e] = res_bn ? res_scale[cg + e] : 1.f; rsh[e] = res_bn ? res_shift[cg + e] : 0.f;
  }
  for (; i < nvec; i += stride) {
    const u32x4 v = se_ld(y, base + i);
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[2 * e] = fmaf(bf16_lo(v[e]), sc[2 * e], sh[2 * e]);
      f[2 * e + 1] = fmaf(bf16_hi(v[e]), sc[2 * e + 1], sh[2 * e + 1]);
    }
    if (residual != nullptr) {
      const u32x4 r = se_ld(residual, base + i);
      float rr[8];
      if (res_bn) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          rr[2 * e] = bf16_to_f32(f32_to_bf16(fmaf(bf16_lo(r[e]), rsc[2 * e], rsh[2 * e])));
          rr[2 * e + 1] = bf16_to_f32(f32_to_bf16(fmaf(bf16_hi(r[e]), rsc[2 * e + 1], rsh[2 * e + 1])));
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { rr[2 * e] = bf16_lo(r[e]); rr[2 * e + 1] = bf16_hi(r[e]); }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = fmaf(f[e], ge[e], rr[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] *= ge[e];
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = (f[e] < 0.f) ? 0.f : f[e];   // NaN stays NaN, as torch.relu
    }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
    ((u32x4*)out)[base + i] = o;
    if (maskbits != nullptr) {
      unsigned int bits = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) bits |= (f[e] > 0.f ? 1u : 0u) << e;
      maskbits[base + i] = (unsigned char)bits;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Backward, [N,C]-sized step 1, one workgroup per sample: fold the segment rows to A = sum_hw g and B = sum_hw g*xhat, then
//   de = gamma*B + beta*A    dp2 = de*e*(1-e)    dh = (dp2 W2) * [h > 0]    ds = dh W1
// (gamma = beta = 0 makes de, and with it every excitation gradient, an exact zero).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_bwd_sample_kernel(const float* __restrict__ part, int S, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ e,
                                                            const float* __restrict__ h, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, float* __restrict__ AB,
                                                            float* __restrict__ dp2, float* __restrict__ dh,
                                                            float* __restrict__ ds, int C, int rd) {
  __shared__ float dp2_l[4096];
  __shared__ float dh_l[256];
  __shared__ float red[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) {
    double Ad = 0.0, Bd = 0.0;
    for (int k = 0; k < S; ++k) {
      Ad += (double)part[(((long long)n * S + k) * 2 + 0) * C + c];
      Bd += (double)part[(((long long)n * S + k) * 2 + 1) * C + c];
    }
    const float A = (float)Ad, B = (float)Bd;
    AB[((long long)n * 2 + 0) * C + c] = A;
    AB[((long long)n * 2 + 1) * C + c] = B;
    const float de = gamma[c] * B + beta[c] * A;
    const float ev = e[(long long)n * C + c];
    const float p = de * ev * (1.f - ev);
    dp2_l[c] = p;
    dp2[(long long)n * C + c] = p;
  }
  __syncthreads();
  const int nl = 256 / rd;   // channel lanes per hidden unit (rd <= 256)
  {
    float acc = 0.f;
    if (tid < nl * rd) {
      const int j = tid % rd, cl = tid / rd;
      for (int c = cl; c < C; c += nl) acc += dp2_l[c] * w2[(long long)c * rd + j];
    }
    red[tid] = acc;
  }
  __syncthreads();
  if (tid < rd) {
    float v = 0.f;
    for (int l = 0; l < nl; ++l) v += red[l * rd + tid];
    v = h[(long long)n * rd + tid] > 0.f ? v : 0.f;
    dh_l[tid] = v;
    dh[(long long)n * rd + tid] = v;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < rd; ++j) acc += dh_l[j] * w1[(long long)j * C + c];
    ds[(long long)n * C + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// Backward, [N,C]-sized step 2: every sum over samples, serial in n.  Thread t -> (four channels c, hidden unit j):
//   dW2[c][j] = sum_n dp2[n][c] h[n][j]      dW1[j][c] = sum_n dh[n][j] s[n][c]
// the j == 0 threads also own their four channels' per-channel results (fp64 sums over n):
//   dbeta = sum_n (e A + ds)    dgamma = sum_n (e B + ds Shat/HW)    db2 = sum_n dp2
//   k2[c] = scale dgamma / M    k0[n][c] = scale (ds[n][c]/HW - dbeta/M)         Shat = (ysum - HW mean) invstd
// and the threads of the first four channels db1[j] = sum_n dh[n][j].
// ------------------------------------------------------------------------------------------------
struct SeBwdArgs {
  const float *AB, *dp2, *dh, *ds, *ysum, *s, *h, *e, *mean, *invstd, *gamma;
  float *dgamma, *dbeta, *dw1, *db1, *dw2, *db2, *k0, *k2;
  int N, HW, C, rd, accumulate;
};
__global__ __launch_bounds__(256) void se_bwd_params_kernel(const SeBwdArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = a.C, rd = a.rd, N = a.N;
  if (t >= (long long)(C >> 2) * rd) return;
  const int cq = (int)(t / rd), j = (int)(t - (long long)cq * rd);
  const int c = cq * 4;
  f32x4 aw2 = {0.f, 0.f, 0.f, 0.f}, aw1 = {0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < N; ++n) {
    const f32x4 p = *(const f32x4*)(a.dp2 + (long long)n * C + c);
    const f32x4 sv = *(const f32x4*)(a.s + (long long)n * C + c);
    const float hv = a.h[(long long)n * rd + j];
    const float dv = a.dh[(long long)n * rd + j];
    aw2 += p * hv;
    aw1 += sv * dv;
  }
  float* dw1p = a.dw1 + (long long)j * C + c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float* dw2p = a.dw2 + (long long)(c + k) * rd + j;
    *dw2p = a.accumulate ? *dw2p + aw2[k] : aw2[k];
    dw1p[k] = a.accumulate ? dw1p[k] + aw1[k] : aw1[k];
  }
  if (cq == 0) {
    double sum = 0.0;
    for (int n = 0; n < N; ++n) sum += (double)a.dh[(long long)n * rd + j];
    a.db1[j] = a.accumulate ? a.db1[j] + (float)sum : (float)sum;
  }
  if (j != 0) return;
  const double hw = (double)a.HW, M = (double)N * hw;
  double db[4] = {0, 0, 0, 0}, dg[4] = {0, 0, 0, 0}, d2[4] = {0, 0, 0, 0};
  float mu[4], is[4], sc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { mu[k] = a.mean[c + k]; is[k] = a.invstd[c + k]; sc[k] = a.gamma[c + k] * is[k]; }
  for (int n = 0; n < N; ++n) {
    const long long o = (long long)n * C + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double ev = a.e[o + k], dsv = a.ds[o + k];
      const double A = a.AB[((long long)n * 2 + 0) * C + c + k], B = a.AB[((long long)n * 2 + 1) * C + c + k];
      const double shat = ((double)a.ysum[o + k] - hw * (double)mu[k]) * (double)is[k];
      db[k] += ev * A + dsv;
      dg[k] += ev * B + dsv * shat / hw;
      d2[k] += (double)a.dp2[o + k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.dbeta[c + k] = a.accumulate ? a.dbeta[c + k] + (float)db[k] : (float)db[k];
    a.dgamma[c + k] = a.accumulate ? a.dgamma[c + k] + (float)dg[k] : (float)dg[k];
    a.db2[c + k] = a.accumulate ? a.db2[c + k] + (float)d2[k] : (float)d2[k];
    a.k2[c + k] = (float)((double)sc[k] * dg[k] / M);
  }
  for (int n = 0; n < N; ++n) {
    const long long o = (long long)n * C + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.k0[o + k] = (float)((double)sc[k] * ((double)a.ds[o + k] / hw - db[k] / M));
  }
}

// Backward, pass 2: dy3 = k1[n][c]*g + k0[n][c] - k2[c]*xhat, k1 = gamma*invstd*e[n][c]; grid (blocks per sample, N)
__global__ __launch_bounds__(256) void se_bwd_apply_kernel(const bf16_t* __restrict__ dout, const unsigned char* __restrict__ maskbits,
                                                           const bf16_t* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ gate, const float* __restrict__ k0,
                                                           const float* __restrict__ k2, bf16_t* __restrict__ dy, int HW, int cpr) {
  const int n = blockIdx.y;
  const long long nvec = (long long)HW * cpr;
  const long long base = (long long)n * nvec;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(i % cpr) * 8;
  const long long nc = (long long)n * cpr * 8 + cg;
  float mu[8], is[8], a1[8], a0[8], a2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mu[e] = mean[cg + e]; is[e] = invstd[cg + e];
    a1[e] = gamma[cg + e] * is[e] * gate[nc + e];
    a0[e] = k0[nc + e]; a2[e] = k2[cg + e];
  }
  for (; i < nvec; i += stride) {
    const u32x4 d = se_ld(dout, base + i);
    const u32x4 yv = se_ld(y, base + i);
    const unsigned int bits = maskbits != nullptr ? (unsigned int)maskbits[base + i] : 0xffu;
    float g[8], yy[8], o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g[2 * e] = bf16_lo(d[e]); g[2 * e + 1] = bf16_hi(d[e]);
      yy[2 * e] = bf16_lo(yv[e]); yy[2 * e + 1] = bf16_hi(yv[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (!((bits >> e) & 1u)) g[e] = 0.f;
      o[e] = fmaf(a1[e], g[e], a0[e]) - a2[e] * ((yy[e] - mu[e]) * is[e]);
    }
    u32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = pack_bf16x2(o[2 * e], o[2 * e + 1]);
    ((u32x4*)dy)[base + i] = ov;
  }
}

inline int gcd_i(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

// blocks per sample of the two elementwise passes: ~2048 workgroups in all, total threads per sample a multiple of C/8
unsigned int blocks_per_sample(int N, int HW, int cpr) {
  const long long nvec = (long long)HW * cpr;
  long long blocks = (nvec + 255) / 256;
  const long long cap = (2048 + N - 1) / N;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const int mult = cpr / gcd_i(cpr, 256);
  return (unsigned int)((blocks + mult - 1) / mult * mult);
}

}  // namespace

// ---------------- host launchers (called from the capi*.hip units) ----------------

bool icamd_se_shape_ok(int N, int HW, int C, int rd) {
  return N > 0 && N <= 65535 && HW > 0 && C > 0 && C % 8 == 0 && C <= 4096 && rd >= 1 && rd <= 256 &&
         (long long)N * HW * (C / 8) < (1ll << 40);
}

// Segments per sample of the reduce passes: HW is split where few samples leave the device idle (layer1 at a small batch: long
// columns), at least 32 rows per segment, ~2048 workgroups in all.
void icamd_se_plan(int N, int HW, int* S, int* rps) {
  long long s = (2048 + N - 1) / N;
  const long long smax = (HW + 31) / 32;
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  const int r = (int)((HW + s - 1) / s);
  *rps = r;
  *S = (HW + r - 1) / r;
}

size_t icamd_se_squeeze_bytes(int N, int HW, int C) {
  int S, rps;
  icamd_se_plan(N, HW, &S, &rps);
  return ws_round256((size_t)N * S * C * sizeof(float));
}

int icamd_se_squeeze_launch(const bf16_t* y, float* ysum, int N, int HW, int C, float* part, hipStream_t s) {
  int S, rps;
  icamd_se_plan(N, HW, &S, &rps);
  float* dst = S == 1 ? ysum : part;
  hipLaunchKernelGGL(se_reduce_kernel<1>, dim3((unsigned)(N * S)), dim3(256), 0, s, y, (const bf16_t*)nullptr,
                     (const unsigned char*)nullptr, (const float*)nullptr, (const float*)nullptr, dst, HW, C, S, rps);
  int rc = icamd_launch_status();
  if (rc || S == 1) return rc;
  hipLaunchKernelGGL(se_fold_kernel, dim3((unsigned)(((long long)N * C + 255) / 256)), dim3(256), 0, s, part, ysum, N, S, C);
  return icamd_launch_status();
}

int icamd_se_excite_fwd_launch(const float* ysum, const float* scale, const float* shift, float inv_hw, const float* w1,
                               const float* b1, const float* w2, const float* b2, float* s_out, float* h_out, float* e_out,
                               int N, int C, int rd, hipStream_t s) {
  int jw = 1;
  while (jw * 2 <= rd && jw * 2 <= 64) jw *= 2;
  hipLaunchKernelGGL(se_excite_fwd_kernel, dim3((unsigned)N), dim3(256), 0, s, ysum, scale, shift, inv_hw, w1, b1, w2, b2, s_out,
                     h_out, e_out, C, rd, jw);
  return icamd_launch_status();
}

int icamd_se_bn_apply_launch(const bf16_t* y, const float* scale, const float* shift, const float* gate, const bf16_t* residual,
                             const float* res_scale, const float* res_shift, bf16_t* out, unsigned char* maskbits, int N, int HW,
                             int C, int relu, hipStream_t s) {
  const int cpr = C / 8;
  hipLaunchKernelGGL(se_bn_apply_kernel, dim3(blocks_per_sample(N, HW, cpr), (unsigned)N), dim3(256), 0, s, y, scale, shift, gate,
                     residual, res_scale, res_shift, out, maskbits, HW, cpr, relu);
  return icamd_launch_status();
}

// workspace: the seven regions of se_bwd_ws (workspace.h)
size_t icamd_se_bn_bwd_bytes(int N, int HW, int C) {
  int S, rps;
  icamd_se_plan(N, HW, &S, &rps);
  return se_bwd_ws(nullptr, N, S, C).bytes;
}

int icamd_se_bn_bwd_launch(const bf16_t* dout, const unsigned char* maskbits, const bf16_t* y, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, const float* ysum, const float* sv,
                           const float* h, const float* e, const float* w1, const float* w2, float* dgamma, float* dbeta,
                           float* dw1, float* db1, float* dw2, float* db2, bf16_t* dy, int N, int HW, int C, int rd,
                           int accumulate, void* workspace, hipStream_t s) {
  int S, rps;
  icamd_se_plan(N, HW, &S, &rps);
  const SeBwdWs w = se_bwd_ws(workspace, N, S, C);
  float *part = w.part, *AB = w.AB, *dp2 = w.dp2, *ds = w.ds, *k0 = w.k0, *dh = w.dh, *k2 = w.k2;
  hipLaunchKernelGGL(se_reduce_kernel<2>, dim3((unsigned)(N * S)), dim3(256), 0, s, y, dout, maskbits, mean, invstd, part, HW, C,
                     S, rps);
  int rc = icamd_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(se_bwd_sample_kernel, dim3((unsigned)N), dim3(256), 0, s, (const float*)part, S, gamma, beta, e, h, w1, w2, AB,
                     dp2, dh, ds, C, rd);
  rc = icamd_launch_status();
  if (rc) return rc;
  SeBwdArgs a;
  a.AB = AB; a.dp2 = dp2; a.dh = dh; a.ds = ds; a.ysum = ysum; a.s = sv; a.h = h; a.e = e; a.mean = mean; a.invstd = invstd;
  a.gamma = gamma; a.dgamma = dgamma; a.dbeta = dbeta; a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.k0 = k0; a.k2 = k2;
  a.N = N; a.HW = HW; a.C = C; a.rd = rd; a.accumulate = accumulate;
  const long long nthr = (long long)(C / 4) * rd;
  hipLaunchKernelGGL(se_bwd_params_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, a);
  rc = icamd_launch_status();
  if (rc) return rc;
  const int cpr = C / 8;
  hipLaunchKernelGGL(se_bwd_apply_kernel, dim3(blocks_per_sample(N, HW, cpr), (unsigned)N), dim3(256), 0, s, dout, maskbits, y, mean,
                     invstd, gamma, e, (const float*)k0, (const float*)k2, dy, HW, cpr);
  return icamd_launch_status();
}
