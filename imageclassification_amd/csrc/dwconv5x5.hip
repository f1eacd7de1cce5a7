// EfficientNet-class kernels for gfx950: depthwise 5x5 convolution, pad 2, stride 1 or 2 (forward with BatchNorm statistics, data
// gradient, weight gradient), BatchNorm + SiLU (apply, per-sample sums, backward) and the squeeze-and-excitation of an MBConv block
// (it sits between the depthwise BatchNorm + SiLU and the projection convolution, pools the ACTIVATED tensor and has a SiLU inside).
// NHWC bf16 activations, filter bf16 [5][5][C] (tap-major shadow of the [C,1,5,5] parameter), fp32 accumulation, every stored tensor
// rounded to bf16 once.  No atomics: partial sums are folded in a fixed order, so every launch gives the same bits.  All addressing
// is 64-bit.
//
// Depthwise 5x5, the register split.  The 3x3 kernels (dwconv3x3.hip) keep a ring of input rows and the taps unpacked in fp32; at
// 5x5 that is 25 + 25 vectors of 8 floats (400 registers), and 25 more for the weight gradient.  Here
//   forward / stride-1 data gradient: a thread owns one 8-channel vector of one output column and walks down a segment of RS output
//     rows with the 25 taps PACKED (bf16 pairs, 100 registers) and NO ring: the 25 input vectors of an output are loaded as they are
//     used, one kernel row of taps at a time (5 + 5 unpacked vectors live), and the reuse between neighbouring outputs is the L1's;
//   weight gradient: one KERNEL ROW of taps per workgroup (blockIdx selects r): 5 accumulators of 8 floats, dy and the five input
//     vectors of row r loaded per output;
//   stride-2 data gradient: a gather, one thread per dx vector, 3 or 2 taps per axis.
// Workgroup shape, items and partial rows are those of the 3x3 kernels: `lanes` columns x `cv` channel vectors, an ITEM is (image,
// row segment, column group), a workgroup takes `ipb` consecutive items.
#include "common.h"
#include "icamd_internal.h"

namespace {

constexpr int RS = 16;   // output rows per item

struct Dw5Geom {
  int OH, OW, cpr, cv, lanes, nslices, colgroups, rowsegs, ipb;
  long long items, rows;   // rows: workgroup rows = partial rows
};

struct Vec8 { f32x2 v[4]; };
__device__ __forceinline__ Vec8 unpack8(const u32x4 p) {
  Vec8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r.v[e] = f32x2{bf16_lo(p[e]), bf16_hi(p[e])};
  return r;
}

struct Dw5Item { int n, oh0, oh1, ow; };
__device__ __forceinline__ Dw5Item dw5_item(long long it, int colgroups, int rowsegs, int lanes, int lane, int OH) {
  Dw5Item r;
  const int cgp = (int)(it % colgroups);
  const long long q = it / colgroups;
  const int seg = (int)(q % rowsegs);
  r.n = (int)(q / rowsegs);
  r.oh0 = seg * RS;
  r.oh1 = (OH < r.oh0 + RS) ? OH : r.oh0 + RS;
  r.ow = cgp * lanes + lane;
  return r;
}

// y[n,oh,ow,c] = sum_{r,t} x[n, oh*S-2+r, ow*S-2+t, c] * w[r][t][c]   (flip: taps mirrored = the stride-1 data gradient)
// stats[row][2][C]: partial sums of the ROUNDED y and of its square, one row per workgroup row
template <int STRIDE, bool STATS>
__global__ __launch_bounds__(256) void dwconv5_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                          bf16_t* __restrict__ y, float* __restrict__ stats, int H, int W, int C,
                                                          Dw5Geom g, int flip) {
  __shared__ float red[STATS ? 256 * 16 : 1];
  const int tid = threadIdx.x;
  const int cslice = (int)(blockIdx.x % (unsigned)g.nslices);
  const long long ib = blockIdx.x / (unsigned)g.nslices;
  const int cvi = tid % g.cv, lane = tid / g.cv;
  const int c = (cslice * g.cv + cvi) * 8;
  u32x4 wt[25];   // packed: unpacked where used
#pragma unroll
  for (int k = 0; k < 25; ++k) wt[k] = *(const u32x4*)(w + (long long)(flip ? 24 - k : k) * C + c);
  f32x2 s1[4], s2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { s1[e] = f32x2{0.f, 0.f}; s2[e] = f32x2{0.f, 0.f}; }
  const long long it1 = (g.items < (ib + 1) * g.ipb) ? g.items : (ib + 1) * g.ipb;
  for (long long it = ib * g.ipb; it < it1; ++it) {            // the items of this workgroup
    const Dw5Item q = dw5_item(it, g.colgroups, g.rowsegs, g.lanes, lane, g.OH);
    if (lane >= g.lanes || q.ow >= g.OW) continue;
    const long long nbase = (long long)q.n * H;
    const int iw0 = q.ow * STRIDE - 2;
    for (int oh = q.oh0; oh < q.oh1; ++oh) {                   // down the segment
      f32x2 acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = f32x2{0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 5; ++r) {                            // one kernel row of taps at a time
        const int ih = oh * STRIDE - 2 + r;
        if ((unsigned)ih >= (unsigned)H) continue;
        // an empty statement the compiler cannot see through: without it the 25 unpacks are hoisted out of the row loop and the
        // taps live unpacked after all (256 VGPRs + AGPR copies, one wave per SIMD)
#pragma unroll
        for (int t = 0; t < 5; ++t) asm volatile("" : "+v"(wt[r * 5 + t]));
        const bf16_t* row = x + ((nbase + ih) * W) * C + c;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
          const int iw = iw0 + t;
          if ((unsigned)iw >= (unsigned)W) continue;
          const Vec8 a = unpack8(ld_stream((const u32x4*)(row + (long long)iw * C)));
          const Vec8 wv = unpack8(wt[r * 5 + t]);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __builtin_elementwise_fma(a.v[e], wv.v[e], acc[e]);
        }
      }
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[e][0], acc[e][1]);
      *(u32x4*)(y + (((long long)q.n * g.OH + oh) * g.OW + q.ow) * C + c) = o;
      if constexpr (STATS) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x2 yr = f32x2{bf16_lo(o[e]), bf16_hi(o[e])};
          s1[e] = s1[e] + yr;
          s2[e] = __builtin_elementwise_fma(yr, yr, s2[e]);
        }
      }
    }
  }
  if constexpr (STATS) {
    // fold the column lanes that share a channel vector, lane 0 first: red[tid][16]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[tid * 16 + 2 * e] = s1[e][0]; red[tid * 16 + 2 * e + 1] = s1[e][1];
      red[tid * 16 + 8 + 2 * e] = s2[e][0]; red[tid * 16 + 8 + 2 * e + 1] = s2[e][1];
    }
    __syncthreads();
    for (int o = tid; o < g.cv * 16; o += 256) {
      const int cvo = o >> 4, e = o & 15;
      float s = 0.f;
      for (int l = 0; l < g.lanes; ++l) s += red[(l * g.cv + cvo) * 16 + e];
      stats[(ib * 2 + (e >> 3)) * C + (cslice * g.cv + cvo) * 8 + (e & 7)] = s;
    }
  }
}

// Stride-2 data gradient as a gather: dx[n,ih,iw,c] = sum over the taps (r,t) with ih+2-r and iw+2-t even of
// dy[n,(ih+2-r)/2,(iw+2-t)/2,c] * w[r][t][c] -- three or two taps per axis.  One thread per dx vector: every element of dx is
// written exactly once, in this one launch (no zero fill, no scatter).
__global__ __launch_bounds__(256) void dwconv5_dgrad_s2_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
                                                               bf16_t* __restrict__ dx, long long nvec, int H, int W, int C, int OH,
                                                               int OW) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const int cpr = C >> 3;
  const int c = (int)(i % cpr) * 8;
  long long pix = i / cpr;
  const int iw = (int)(pix % W); pix /= W;
  const int ih = (int)(pix % H);
  const long long n = pix / H;
  f32x2 acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = f32x2{0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int a = ih + 2 - r;
    if ((a & 1) || a < 0 || (a >> 1) >= OH) continue;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int b = iw + 2 - t;
      if ((b & 1) || b < 0 || (b >> 1) >= OW) continue;
      const Vec8 d = unpack8(ld_stream((const u32x4*)(dy + ((n * OH + (a >> 1)) * OW + (b >> 1)) * C + c)));
      const Vec8 wv = unpack8(*(const u32x4*)(w + (long long)(r * 5 + t) * C + c));
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_elementwise_fma(d.v[e], wv.v[e], acc[e]);
    }
  }
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[e][0], acc[e][1]);
  *(u32x4*)(dx + i * 8) = o;
}

// dw[r][t][c] = sum_{n,oh,ow} dy[n,oh,ow,c] * x[n, oh*S-2+r, ow*S-2+t, c], ONE kernel row r per workgroup (blockIdx.x % 5): the
// forward's walk with the five tap sums of that row in registers.  The column lanes of a workgroup are folded through LDS, lane 0
// first; part[row][25][C], folded over the rows by the slab reducer.
template <int STRIDE>
__global__ __launch_bounds__(256) void dwconv5_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                            float* __restrict__ part, int H, int W, int C, Dw5Geom g) {
  __shared__ float red[256 * 40];
  const int tid = threadIdx.x;
  const int r = (int)(blockIdx.x % 5u);
  const unsigned int rest = blockIdx.x / 5u;
  const int cslice = (int)(rest % (unsigned)g.nslices);
  const long long ib = rest / (unsigned)g.nslices;
  const int cvi = tid % g.cv, lane = tid / g.cv;
  const int c = (cslice * g.cv + cvi) * 8;
  Vec8 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[t].v[e] = f32x2{0.f, 0.f};
  const long long it1 = (g.items < (ib + 1) * g.ipb) ? g.items : (ib + 1) * g.ipb;
  for (long long it = ib * g.ipb; it < it1; ++it) {            // the items of this workgroup
    const Dw5Item q = dw5_item(it, g.colgroups, g.rowsegs, g.lanes, lane, g.OH);
    if (lane >= g.lanes || q.ow >= g.OW) continue;
    const long long nbase = (long long)q.n * H;
    const int iw0 = q.ow * STRIDE - 2;
    for (int oh = q.oh0; oh < q.oh1; ++oh) {                   // down the segment
      const int ih = oh * STRIDE - 2 + r;
      if ((unsigned)ih >= (unsigned)H) continue;
      const Vec8 d = unpack8(ld_stream((const u32x4*)(dy + (((long long)q.n * g.OH + oh) * g.OW + q.ow) * C + c)));
      const bf16_t* row = x + ((nbase + ih) * W) * C + c;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const int iw = iw0 + t;
        if ((unsigned)iw >= (unsigned)W) continue;
        const Vec8 a = unpack8(ld_stream((const u32x4*)(row + (long long)iw * C)));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t].v[e] = __builtin_elementwise_fma(a.v[e], d.v[e], acc[t].v[e]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[tid * 40 + t * 8 + 2 * e] = acc[t].v[e][0];
      red[tid * 40 + t * 8 + 2 * e + 1] = acc[t].v[e][1];
    }
  __syncthreads();
  for (int o = tid; o < g.cv * 40; o += 256) {
    const int cvo = o / 40, k = o - cvo * 40;                  // k = tap-in-row * 8 + channel of the vector
    float s = 0.f;
    for (int l = 0; l < g.lanes; ++l) s += red[(l * g.cv + cvo) * 40 + k];
    part[(ib * 25 + r * 5 + (k >> 3)) * C + (cslice * g.cv + cvo) * 8 + (k & 7)] = s;
  }
}

// ---- BatchNorm + SiLU -------------------------------------------------------------------------------------------------------------
// sigma(z) = 1 / (1 + exp(-z)) and silu(z) = z / (1 + exp(-z)), full-precision expf and IEEE division: exp(-z) overflows to +inf
// for z < -88.7, where sigma = 0 and silu = -0 (finite for every finite z); NaN stays NaN.
__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float silu_f(float z) { return z / (1.f + expf(-z)); }
// silu'(z) = sigma (1 + z (1 - sigma)): 0 * (1 - 2^20) = -0 at the far left, 1 at the far right
__device__ __forceinline__ float silu_grad_f(float z) {
  const float sg = sigmoid_f(z);
  return sg * fmaf(z, 1.f - sg, 1.f);
}
// the ONE definition of the activated, rounded value a = bf16(silu(fma(y, scale, shift))): icamd_bn_apply_silu stores it (gated or
// not), the per-sample sums and the backward form it in registers
__device__ __forceinline__ u32x4 bn_silu_8(const u32x4 v, const float (&sc)[8], const float (&sh)[8]) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    o[e] = pack_bf16x2(silu_f(fmaf(bf16_lo(v[e]), sc[2 * e], sh[2 * e])), silu_f(fmaf(bf16_hi(v[e]), sc[2 * e + 1], sh[2 * e + 1])));
  return o;
}

// out = a, or bf16(float(a) * gate[n][c]); 8 channels per thread, grid-stride with a loop-invariant channel group
template <bool GATED>
__global__ __launch_bounds__(256) void bn_apply_silu_kernel(const bf16_t* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ gate,
                                                            bf16_t* __restrict__ out, long long nvec, int cpr, long long vec_per_image) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(i % cpr) * 8;   // the launcher makes stride a multiple of cpr
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = scale[cg + e]; sh[e] = shift[cg + e]; }
  for (; i < nvec; i += stride) {
    u32x4 a = bn_silu_8(ld_stream((const u32x4*)y + i), sc, sh);
    if constexpr (GATED) {
      const float* gp = gate + (i / vec_per_image) * ((long long)cpr * 8) + cg;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = pack_bf16x2(bf16_lo(a[e]) * gp[2 * e], bf16_hi(a[e]) * gp[2 * e + 1]);
    }
    ((u32x4*)out)[i] = a;
  }
}

// part[n * S + seg][C] = sum over the segment's pixels of float(a) (squeeze) or of dout * float(a) (gate gradient); thread ->
// (channel group, row lane), the row lanes folded through LDS, lane 0 first
template <bool WITH_DOUT>
__global__ __launch_bounds__(256) void silu_rowsum_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          float* __restrict__ part, int HW, int C, int S, int rps) {
  __shared__ float red[256 * 8];
  const int cpr = C >> 3;
  const int tid = threadIdx.x;
  const long long n = blockIdx.x / (unsigned)S;
  const int seg = (int)(blockIdx.x % (unsigned)S);
  const int r0 = seg * rps;
  const int r1 = (HW < r0 + rps) ? HW : r0 + rps;
  for (int cg0 = 0; cg0 < cpr; cg0 += 256) {
    const int tcols = (cpr - cg0 < 256) ? (cpr - cg0) : 256;
    const int rlanes = 256 / tcols;
    const int cgi = tid % tcols, rl = tid / tcols;
    float sum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = 0.f;
    if (rl < rlanes) {
      const int c = (cg0 + cgi) * 8;
      float sc[8], sh[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { sc[e] = scale[c + e]; sh[e] = shift[c + e]; }
      for (int r = r0 + rl; r < r1; r += rlanes) {
        const long long off = (n * HW + r) * cpr + cg0 + cgi;
        const u32x4 a = bn_silu_8(ld_stream((const u32x4*)y + off), sc, sh);
        if constexpr (WITH_DOUT) {
          const u32x4 d = ld_stream((const u32x4*)dout + off);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            sum[2 * e] = fmaf(bf16_lo(d[e]), bf16_lo(a[e]), sum[2 * e]);
            sum[2 * e + 1] = fmaf(bf16_hi(d[e]), bf16_hi(a[e]), sum[2 * e + 1]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) { sum[2 * e] += bf16_lo(a[e]); sum[2 * e + 1] += bf16_hi(a[e]); }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = sum[e];
    __syncthreads();
    for (int o = tid; o < tcols * 8; o += 256) {
      const int cgo = o >> 3, e = o & 7;
      float s = 0.f;
      for (int l = 0; l < rlanes; ++l) s += red[(l * tcols + cgo) * 8 + e];
      part[(long long)blockIdx.x * C + (cg0 + cgo) * 8 + e] = s;
    }
    __syncthreads();
  }
}

// out[n][c] = sum over the S segments of part[n * S + seg][c], segment 0 first
__global__ __launch_bounds__(256) void seg_fold_kernel(const float* __restrict__ part, float* __restrict__ out, long long nc, int S,
                                                       int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc) return;
  const long long n = i / C;
  const int c = (int)(i - n * C);
  float s = 0.f;
  for (int seg = 0; seg < S; ++seg) s += part[(n * S + seg) * C + c];
  out[i] = s;
}

// ---- the excitation of an MBConv block: [N, C]-sized work, one workgroup per sample (forward, dsn) or per hidden unit (parameter
// gradients).  C <= 4096, rd <= 256.
// s = asum * inv_hw; hpre = W1 s + b1; e = sigmoid(W2 silu(hpre) + b2)
__global__ __launch_bounds__(256) void se_excite_silu_fwd_kernel(const float* __restrict__ asum, float inv_hw,
                                                                 const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, const float* __restrict__ b2,
                                                                 float* __restrict__ s_out, float* __restrict__ hpre_out,
                                                                 float* __restrict__ e_out, int C, int rd) {
  __shared__ float sS[4096];
  __shared__ float sH[256];
  const int tid = threadIdx.x, wave = tid >> 6, ln = tid & 63;
  const long long n = blockIdx.x;
  for (int c = tid; c < C; c += 256) {
    const float v = asum[n * C + c] * inv_hw;
    sS[c] = v;
    s_out[n * C + c] = v;
  }
  __syncthreads();
  for (int j = wave; j < rd; j += 4) {
    float acc = 0.f;
    for (int c = ln; c < C; c += 64) acc = fmaf(w1[(long long)j * C + c], sS[c], acc);
    acc = wave_sum(acc);
    if (ln == 0) {
      const float hp = acc + b1[j];
      hpre_out[n * rd + j] = hp;
      sH[j] = silu_f(hp);
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float acc = b2[c];
    for (int j = 0; j < rd; ++j) acc = fmaf(w2[(long long)c * rd + j], sH[j], acc);
    e_out[n * C + c] = sigmoid_f(acc);
  }
}

// dp2 = de e (1 - e); dh = (dp2 W2) silu'(hpre); dsn = (dh W1) inv_hw
__global__ __launch_bounds__(256) void se_excite_silu_bwd_dsn_kernel(const float* __restrict__ de, const float* __restrict__ hpre,
                                                                     const float* __restrict__ e, const float* __restrict__ w1,
                                                                     const float* __restrict__ w2, float* __restrict__ dsn, int C,
                                                                     int rd, float inv_hw) {
  __shared__ float sD[4096];
  __shared__ float sH[256];
  const int tid = threadIdx.x, wave = tid >> 6, ln = tid & 63;
  const long long n = blockIdx.x;
  for (int c = tid; c < C; c += 256) {
    const float ev = e[n * C + c];
    sD[c] = de[n * C + c] * ev * (1.f - ev);
  }
  __syncthreads();
  for (int j = wave; j < rd; j += 4) {
    float acc = 0.f;
    for (int c = ln; c < C; c += 64) acc = fmaf(sD[c], w2[(long long)c * rd + j], acc);
    acc = wave_sum(acc);
    if (ln == 0) sH[j] = acc * silu_grad_f(hpre[n * rd + j]);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < rd; ++j) acc = fmaf(sH[j], w1[(long long)j * C + c], acc);
    dsn[n * C + c] = acc * inv_hw;
  }
}

// Parameter gradients, workgroup j = one hidden unit: dh[n][j] for every sample (a wave per sample, in chunks of NCH samples kept in
// LDS), then dW1[j][:] = sum_n dh[n][j] s[n][:], db1[j] = sum_n dh[n][j], dW2[:][j] = sum_n dp2[n][:] silu(hpre[n][j]) and, in
// workgroup 0, db2 = sum_n dp2[n][:]; a thread owns the channels tid + 256 k and adds the samples in order.
constexpr int NCH = 1024;
__global__ __launch_bounds__(256) void se_excite_silu_bwd_params_kernel(const float* __restrict__ de, const float* __restrict__ sv,
                                                                        const float* __restrict__ hpre, const float* __restrict__ e,
                                                                        const float* __restrict__ w2, float* __restrict__ dw1,
                                                                        float* __restrict__ db1, float* __restrict__ dw2,
                                                                        float* __restrict__ db2, int N, int C, int rd, int accumulate) {
  __shared__ float sW2[4096];
  __shared__ float sDh[NCH];
  __shared__ float sHj[NCH];
  const int tid = threadIdx.x, wave = tid >> 6, ln = tid & 63;
  const int j = blockIdx.x;
  for (int c = tid; c < C; c += 256) sW2[c] = w2[(long long)c * rd + j];
  float a1[16], a2[16], ab2[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { a1[k] = 0.f; a2[k] = 0.f; ab2[k] = 0.f; }
  float ab1 = 0.f;
  __syncthreads();
  for (int n0 = 0; n0 < N; n0 += NCH) {
    const int nn = (N - n0 < NCH) ? (N - n0) : NCH;
    for (int i = wave; i < nn; i += 4) {
      const long long n = n0 + i;
      float acc = 0.f;
      for (int c = ln; c < C; c += 64) {
        const float ev = e[n * C + c];
        acc = fmaf(de[n * C + c] * ev * (1.f - ev), sW2[c], acc);
      }
      acc = wave_sum(acc);
      if (ln == 0) {
        const float hp = hpre[n * rd + j];
        sDh[i] = acc * silu_grad_f(hp);
        sHj[i] = silu_f(hp);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = tid + 256 * k;
      if (c < C) {
#pragma unroll 4
        for (int i = 0; i < nn; ++i) {
          const long long o = (long long)(n0 + i) * C + c;
          const float ev = e[o];
          const float dp2 = de[o] * ev * (1.f - ev);
          a1[k] = fmaf(sDh[i], sv[o], a1[k]);
          a2[k] = fmaf(dp2, sHj[i], a2[k]);
          ab2[k] += dp2;
        }
      }
    }
    if (tid == 0)
      for (int i = 0; i < nn; ++i) ab1 += sDh[i];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = tid + 256 * k;
    if (c < C) {
      const long long o1 = (long long)j * C + c, o2 = (long long)c * rd + j;
      dw1[o1] = (accumulate ? dw1[o1] : 0.f) + a1[k];
      dw2[o2] = (accumulate ? dw2[o2] : 0.f) + a2[k];
      if (j == 0) db2[c] = (accumulate ? db2[c] : 0.f) + ab2[k];
    }
  }
  if (tid == 0) db1[j] = (accumulate ? db1[j] : 0.f) + ab1;
}

// ---- BatchNorm backward behind a SiLU ---------------------------------------------------------------------------------------------
// g = upstream * silu'(z), z the forward's own fp32 expression fma(y, scale, shift); upstream = dout, or dout * gate[n][c] + dsn[n][c]
template <bool GATED>
__device__ __forceinline__ void silu_g(const u32x4 d, const u32x4 yv, const float (&sc)[8], const float (&sh)[8],
                                       const float* __restrict__ gate, const float* __restrict__ dsn, float (&g)[8], float (&yy)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    g[2 * e] = bf16_lo(d[e]); g[2 * e + 1] = bf16_hi(d[e]);
    yy[2 * e] = bf16_lo(yv[e]); yy[2 * e + 1] = bf16_hi(yv[e]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if constexpr (GATED) g[e] = fmaf(g[e], gate[e], dsn[e]);
    g[e] *= silu_grad_f(fmaf(yy[e], sc[e], sh[e]));
  }
}

// pass 1: part[blk][2][C] = (sum g, sum g * xhat) over the block's rows; a twin of bn_bwd_relu6_reduce_kernel (dwconv3x3.hip) and
// of bn_bwd_reduce_kernel (norm_pool.hip), whose finalize kernel folds these rows: the sums and the dy expression are the same
template <bool GATED>
__global__ __launch_bounds__(256) void bn_bwd_silu_reduce_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ gate, const float* __restrict__ dsn,
                                                                 float* __restrict__ part, long long rows, int HW, int C,
                                                                 int rows_per_block) {
  __shared__ float red[256 * 16];
  const int cpr = C >> 3;
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = (rows < r0 + rows_per_block) ? rows : r0 + rows_per_block;
  for (int cg0 = 0; cg0 < cpr; cg0 += 256) {
    const int tcols = (cpr - cg0 < 256) ? (cpr - cg0) : 256;
    const int rlanes = 256 / tcols;
    const int cgi = tid % tcols, rl = tid / tcols;
    float sg[8], sgx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sg[e] = 0.f; sgx[e] = 0.f; }
    if (rl < rlanes) {
      const int c = (cg0 + cgi) * 8;
      float mu[8], is[8], sc[8], sh[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { mu[e] = mean[c + e]; is[e] = invstd[c + e]; sc[e] = scale[c + e]; sh[e] = shift[c + e]; }
      for (long long r = r0 + rl; r < r1; r += rlanes) {
        const long long off = r * cpr + cg0 + cgi;
        const long long nc = GATED ? (r / HW) * C + c : 0;
        float g[8], yy[8];
        silu_g<GATED>(ld_stream((const u32x4*)dout + off), ld_stream((const u32x4*)y + off), sc, sh, gate + nc, dsn + nc, g, yy);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          sg[e] += g[e];
          sgx[e] += g[e] * ((yy[e] - mu[e]) * is[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[tid * 16 + e] = sg[e]; red[tid * 16 + 8 + e] = sgx[e]; }
    __syncthreads();
    for (int o = tid; o < tcols * 16; o += 256) {
      const int cgo = o >> 4, e = o & 15;
      float s = 0.f;
      for (int l = 0; l < rlanes; ++l) s += red[(l * tcols + cgo) * 16 + e];
      part[((long long)blockIdx.x * 2 + (e >> 3)) * C + (cg0 + cgo) * 8 + (e & 7)] = s;
    }
    __syncthreads();
  }
}

// pass 2: dy = scale * (g - c1 - xhat * c2)
template <bool GATED>
__global__ __launch_bounds__(256) void bn_bwd_silu_apply_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ gate, const float* __restrict__ dsn,
                                                                const float* __restrict__ c1, const float* __restrict__ c2,
                                                                bf16_t* __restrict__ dy, long long nvec, int cpr,
                                                                long long vec_per_image) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(i % cpr) * 8;   // the launcher makes stride a multiple of cpr
  float mu[8], is[8], sc[8], sh[8], k1[8], k2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mu[e] = mean[cg + e]; is[e] = invstd[cg + e]; sc[e] = scale[cg + e]; sh[e] = shift[cg + e];
    k1[e] = c1[cg + e]; k2[e] = c2[cg + e];
  }
  for (; i < nvec; i += stride) {
    const long long nc = GATED ? (i / vec_per_image) * ((long long)cpr * 8) + cg : 0;
    float g[8], yy[8], o[8];
    silu_g<GATED>(ld_stream((const u32x4*)dout + i), ld_stream((const u32x4*)y + i), sc, sh, gate + nc, dsn + nc, g, yy);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = sc[e] * (g[e] - k1[e] - ((yy[e] - mu[e]) * is[e]) * k2[e]);
    u32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = pack_bf16x2(o[2 * e], o[2 * e + 1]);
    ((u32x4*)dy)[i] = ov;
  }
}

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// grid of a grid-stride elementwise kernel: at most ~1024 workgroups, total threads a multiple of cpr
unsigned int elementwise_grid(long long nvec, int cpr) {
  const int mult = cpr / gcd_i(cpr, 256);
  long long blocks = (nvec + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  return (unsigned int)((blocks + mult - 1) / mult * mult);
}

// `cap`: the most partial rows wanted; `pixels_per_row`: at least this many output pixels behind every partial row; `fan`: the
// workgroups per (row, slice) pair (5 for the weight gradient: one per kernel row of taps)
bool dw5_geometry(int N, int H, int W, int C, int stride, long long cap, long long pixels_per_row, int fan, Dw5Geom* out) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (stride != 1 && stride != 2)) return false;
  Dw5Geom g;
  g.OH = (H - 1) / stride + 1;
  g.OW = (W - 1) / stride + 1;
  g.cpr = C / 8;
  // the widest divisor of cpr (whole channel runs per pixel) whose multiples fill 192 of the 256 threads at least
  int best = g.cpr < 256 ? g.cpr : 256;
  while (g.cpr % best != 0 || (256 / best) * best < 192) --best;
  g.cv = best;
  g.lanes = 256 / best;
  g.nslices = g.cpr / best;
  g.colgroups = (g.OW + g.lanes - 1) / g.lanes;
  g.rowsegs = (g.OH + RS - 1) / RS;
  g.items = (long long)N * g.rowsegs * g.colgroups;
  long long target = (long long)N * g.OH * g.OW / pixels_per_row;
  if (target < 32) target = 32;
  if (target > cap) target = cap;
  g.ipb = (int)((g.items + target - 1) / target);
  g.rows = (g.items + g.ipb - 1) / g.ipb;
  if (g.rows * g.nslices * fan >= (1ll << 31)) return false;
  if (((long long)N * H * W * g.cpr + 255) / 256 >= (1ll << 31)) return false;   // the gather's grid
  *out = g;
  return true;
}
bool dw5_fwd_geometry(int N, int H, int W, int C, int stride, Dw5Geom* g) { return dw5_geometry(N, H, W, C, stride, 2048, 16, 1, g); }
bool dw5_wgrad_geometry(int N, int H, int W, int C, int stride, Dw5Geom* g) { return dw5_geometry(N, H, W, C, stride, 1024, 64, 5, g); }

}  // namespace

bool icamd_dwconv5_ok(int N, int H, int W, int C, int stride) {
  Dw5Geom g;
  return dw5_fwd_geometry(N, H, W, C, stride, &g) && dw5_wgrad_geometry(N, H, W, C, stride, &g);
}

long long icamd_dwconv5_stats_rows_cxx(int N, int H, int W, int C, int stride) {
  Dw5Geom g;
  return icamd_dwconv5_ok(N, H, W, C, stride) && dw5_fwd_geometry(N, H, W, C, stride, &g) ? g.rows : 0;
}

long long icamd_dwconv5_wgrad_rows(int N, int H, int W, int C, int stride) {
  Dw5Geom g;
  return icamd_dwconv5_ok(N, H, W, C, stride) && dw5_wgrad_geometry(N, H, W, C, stride, &g) ? g.rows : 0;
}

int icamd_dwconv5_fwd_launch(const bf16_t* x, const bf16_t* w, bf16_t* y, float* stats, int N, int H, int W, int C, int stride,
                             int flip, hipStream_t s) {
  Dw5Geom g;
  if (!icamd_dwconv5_ok(N, H, W, C, stride) || !dw5_fwd_geometry(N, H, W, C, stride, &g)) return ICAMD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(g.rows * g.nslices)), block(256);
#define DW5_FWD(S, T) hipLaunchKernelGGL((dwconv5_fwd_kernel<S, T>), grid, block, 0, s, x, w, y, stats, H, W, C, g, flip)
  if (stride == 1) { if (stats) DW5_FWD(1, true); else DW5_FWD(1, false); }
  else { if (stats) DW5_FWD(2, true); else DW5_FWD(2, false); }
#undef DW5_FWD
  return icamd_launch_status();
}

// dy [N][OH][OW][C] -> dx [N][H][W][C]
int icamd_dwconv5_dgrad_launch(const bf16_t* dy, const bf16_t* w, bf16_t* dx, int N, int H, int W, int C, int stride, hipStream_t s) {
  if (!icamd_dwconv5_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  if (stride == 1) return icamd_dwconv5_fwd_launch(dy, w, dx, nullptr, N, H, W, C, 1, /*flip=*/1, s);
  const long long nvec = (long long)N * H * W * (C / 8);
  hipLaunchKernelGGL(dwconv5_dgrad_s2_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, dy, w, dx, nvec, H, W, C,
                     (H - 1) / 2 + 1, (W - 1) / 2 + 1);
  return icamd_launch_status();
}

int icamd_dwconv5_wgrad_launch(const bf16_t* x, const bf16_t* dy, float* part, float* dw, int N, int H, int W, int C, int stride,
                               int accumulate, hipStream_t s) {
  Dw5Geom g;
  if (!icamd_dwconv5_ok(N, H, W, C, stride) || !dw5_wgrad_geometry(N, H, W, C, stride, &g)) return ICAMD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(g.rows * g.nslices * 5)), block(256);
  if (stride == 1) hipLaunchKernelGGL((dwconv5_wgrad_kernel<1>), grid, block, 0, s, x, dy, part, H, W, C, g);
  else hipLaunchKernelGGL((dwconv5_wgrad_kernel<2>), grid, block, 0, s, x, dy, part, H, W, C, g);
  const int rc = icamd_launch_status();
  if (rc) return rc;
  return icamd_slab_reduce_launch(part, dw, 25ll * C, (int)g.rows, accumulate, s);
}

// ---- BatchNorm + SiLU, MBConv squeeze-and-excitation ----
bool icamd_silu_shape_ok(int N, int HW, int C, int rd) {
  return N > 0 && HW > 0 && C > 0 && C % 8 == 0 && C <= 4096 && rd >= 1 && rd <= 256;
}

// S row segments per sample: about 1024 workgroups, 32 pixels per segment at least
void icamd_silu_plan(int N, int HW, int* S, int* rps) {
  int want = 1024 / N;
  if (want < 1) want = 1;
  const int most = (HW + 31) / 32;
  if (want > most) want = most;
  *rps = (HW + want - 1) / want;
  *S = (HW + *rps - 1) / *rps;
}

size_t icamd_silu_rowsum_bytes(int N, int HW, int C) {
  int S, rps;
  icamd_silu_plan(N, HW, &S, &rps);
  return (size_t)N * S * C * sizeof(float);
}

int icamd_bn_apply_silu_launch(const bf16_t* y, const float* scale, const float* shift, const float* gate, bf16_t* out, int N, int HW,
                               int C, hipStream_t s) {
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  const int cpr = C / 8;
  const long long nvec = (long long)N * HW * cpr, vpi = (long long)HW * cpr;
  const dim3 grid(elementwise_grid(nvec, cpr)), block(256);
  if (gate) hipLaunchKernelGGL((bn_apply_silu_kernel<true>), grid, block, 0, s, y, scale, shift, gate, out, nvec, cpr, vpi);
  else hipLaunchKernelGGL((bn_apply_silu_kernel<false>), grid, block, 0, s, y, scale, shift, gate, out, nvec, cpr, vpi);
  return icamd_launch_status();
}

// dout == nullptr: out[n][c] = sum_hw float(a); else sum_hw dout * float(a).  part: icamd_silu_rowsum_bytes
int icamd_silu_rowsum_launch(const bf16_t* dout, const bf16_t* y, const float* scale, const float* shift, float* out, int N, int HW,
                             int C, float* part, hipStream_t s) {
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  int S, rps;
  icamd_silu_plan(N, HW, &S, &rps);
  if ((long long)N * S >= (1ll << 31)) return ICAMD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((long long)N * S)), block(256);
  if (dout) hipLaunchKernelGGL((silu_rowsum_kernel<true>), grid, block, 0, s, dout, y, scale, shift, part, HW, C, S, rps);
  else hipLaunchKernelGGL((silu_rowsum_kernel<false>), grid, block, 0, s, dout, y, scale, shift, part, HW, C, S, rps);
  const int rc = icamd_launch_status();
  if (rc) return rc;
  const long long nc = (long long)N * C;
  hipLaunchKernelGGL(seg_fold_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, part, out, nc, S, C);
  return icamd_launch_status();
}

int icamd_se_excite_silu_fwd_launch(const float* asum, float inv_hw, const float* w1, const float* b1, const float* w2, const float* b2,
                                    float* s_out, float* hpre, float* e, int N, int C, int rd, hipStream_t s) {
  if (!icamd_silu_shape_ok(N, 1, C, rd)) return ICAMD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(se_excite_silu_fwd_kernel, dim3((unsigned)N), dim3(256), 0, s, asum, inv_hw, w1, b1, w2, b2, s_out, hpre, e, C, rd);
  return icamd_launch_status();
}

int icamd_se_excite_silu_bwd_launch(const float* de, const float* sv, const float* hpre, const float* e, const float* w1,
                                    const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dsn, int N, int C, int rd,
                                    float inv_hw, int accumulate, hipStream_t s) {
  if (!icamd_silu_shape_ok(N, 1, C, rd)) return ICAMD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(se_excite_silu_bwd_dsn_kernel, dim3((unsigned)N), dim3(256), 0, s, de, hpre, e, w1, w2, dsn, C, rd, inv_hw);
  const int rc = icamd_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(se_excite_silu_bwd_params_kernel, dim3((unsigned)rd), dim3(256), 0, s, de, sv, hpre, e, w2, dw1, db1, dw2, db2, N,
                     C, rd, accumulate);
  return icamd_launch_status();
}

// part: [icamd_bn_bwd_rows_per_block blocks][2][C]; chunks / c1c2: the regions of icamd_bn_bwd's workspace
int icamd_bn_bwd_silu_launch(const bf16_t* dout, const bf16_t* y, const float* mean, const float* invstd, const float* scale,
                             const float* shift, const float* gate, const float* dsn, float* dgamma, float* dbeta, bf16_t* dy, int N,
                             int HW, int C, int accumulate, float* part, double* chunks, float* c1c2, hipStream_t s) {
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  const long long rows = (long long)N * HW;
  const int rpb = icamd_bn_bwd_rows_per_block(rows, C);
  const int nblk = (int)((rows + rpb - 1) / rpb);
  const int cpr = C / 8;
  if (gate) hipLaunchKernelGGL((bn_bwd_silu_reduce_kernel<true>), dim3((unsigned)nblk), dim3(256), 0, s, dout, y, mean, invstd, scale,
                               shift, gate, dsn, part, rows, HW, C, rpb);
  else hipLaunchKernelGGL((bn_bwd_silu_reduce_kernel<false>), dim3((unsigned)nblk), dim3(256), 0, s, dout, y, mean, invstd, scale,
                          shift, gate, dsn, part, rows, HW, C, rpb);
  int rc = icamd_launch_status();
  if (rc) return rc;
  rc = icamd_bn_bwd_finalize_launch(part, nblk, mean, invstd, dgamma, dbeta, rows, C, accumulate, chunks, c1c2, s, 0);
  if (rc) return rc;
  const long long nvec = rows * cpr, vpi = (long long)HW * cpr;
  const dim3 grid(elementwise_grid(nvec, cpr)), block(256);
  if (gate) hipLaunchKernelGGL((bn_bwd_silu_apply_kernel<true>), grid, block, 0, s, dout, y, mean, invstd, scale, shift, gate, dsn,
                               c1c2, c1c2 + C, dy, nvec, cpr, vpi);
  else hipLaunchKernelGGL((bn_bwd_silu_apply_kernel<false>), grid, block, 0, s, dout, y, mean, invstd, scale, shift, gate, dsn, c1c2,
                          c1c2 + C, dy, nvec, cpr, vpi);
  return icamd_launch_status();
}
