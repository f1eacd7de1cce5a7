// MobileNet-class kernels for gfx950: depthwise 3x3 convolution, pad 1, stride 1 or 2 (forward with BatchNorm statistics, data
// gradient, weight gradient) and BatchNorm + ReLU6 (apply, backward).  NHWC bf16 activations, filter bf16 [3][3][C] (tap-major shadow
// of the [C,1,3,3] parameter), fp32 accumulation, every stored tensor rounded to bf16 once.  No atomics: partial sums are folded in a
// fixed order, so every launch gives the same bits.
//
// The expanded activation of an inverted-residual block, a1 = relu6(bn1(y1)), is six times as wide as the block's input.  The
// forward and the weight gradient therefore take the RAW convolution output y1 with bn1's scale / shift and form
//   a = bf16(min(max(y1 * scale[c] + shift[c], 0), 6))
// on load (ONLOAD): bit for bit what icamd_bn_apply_relu6 would have stored, so a1 is never written or read.  The zero padding is
// zero in the ACTIVATED domain: a tap outside the image contributes 0, not relu6(shift[c]).
//
// Work split (forward, stride-1 data gradient, weight gradient).  A thread owns one 8-channel vector of one output column and walks
// DOWN a segment of RS output rows with a ring of the three input rows in reach (3 columns x 8 channels, unpacked fp32), so an input
// row is loaded once per segment, not once per kernel row; the lanes of a wave are consecutive (channel vector, column) pairs: whole
// pixels, contiguous in memory.  A workgroup is `lanes` columns x `cv` channel vectors (cv = the widest divisor of C/8 that fills
// three quarters of the 256 threads), an ITEM is (image, row segment, column group), and a workgroup takes `ipb` consecutive items, so that the number
// of partial rows (statistics: [2][C], filter gradient: [9][C]) stays a small fraction of the tensor.  All addressing is 64-bit:
// tensors of 4 GB and more are served.
#include "common.h"
#include "icamd_internal.h"

namespace {

constexpr int RS = 16;   // output rows per item

struct Dw3Geom {
  int OH, OW, cpr, cv, lanes, nslices, colgroups, rowsegs, ipb;
  long long items, rows;   // rows: workgroup rows = partial rows
};

__device__ __forceinline__ float relu6f(float f) {   // NaN stays NaN, as torch's hardtanh
  f = (f < 0.f) ? 0.f : f;
  return (f > 6.f) ? 6.f : f;
}
// the one definition of the activated, rounded value: icamd_bn_apply_relu6 stores it, the ONLOAD kernels form it in registers
__device__ __forceinline__ u32x4 bn_relu6_8(const u32x4 v, const float (&sc)[8], const float (&sh)[8]) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    o[e] = pack_bf16x2(relu6f(fmaf(bf16_lo(v[e]), sc[2 * e], sh[2 * e])), relu6f(fmaf(bf16_hi(v[e]), sc[2 * e + 1], sh[2 * e + 1])));
  return o;
}

struct Vec8 { f32x2 v[4]; };
__device__ __forceinline__ Vec8 unpack8(const u32x4 p) {
  Vec8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r.v[e] = f32x2{bf16_lo(p[e]), bf16_hi(p[e])};
  return r;
}

// the (activated) input vector at (n, ih, iw), zero outside the image
template <bool ONLOAD>
__device__ __forceinline__ Vec8 dw3_load(const bf16_t* __restrict__ x, long long nbase, int ih, int iw, int H, int W, int C, int c,
                                         const float (&sc)[8], const float (&sh)[8]) {
  u32x4 p = {0u, 0u, 0u, 0u};
  if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
    p = ld_stream((const u32x4*)(x + ((nbase + ih) * W + iw) * C + c));
    if constexpr (ONLOAD) p = bn_relu6_8(p, sc, sh);
  }
  return unpack8(p);
}

struct Dw3Item { int n, oh0, oh1, ow; };
__device__ __forceinline__ Dw3Item dw3_item(long long it, int colgroups, int rowsegs, int lanes, int lane, int OH) {
  Dw3Item r;
  const int cgp = (int)(it % colgroups);
  const long long q = it / colgroups;
  const int seg = (int)(q % rowsegs);
  r.n = (int)(q / rowsegs);
  r.oh0 = seg * RS;
  r.oh1 = (OH < r.oh0 + RS) ? OH : r.oh0 + RS;
  r.ow = cgp * lanes + lane;
  return r;
}

// Advance the ring to output row oh: ring[r][t] = input (oh * STRIDE - 1 + r, ow * STRIDE - 1 + t).  Stride 1 keeps two rows and
// loads one, stride 2 keeps one and loads two; `first` loads all three.
template <int STRIDE, bool ONLOAD>
__device__ __forceinline__ void dw3_advance(Vec8 (&ring)[3][3], bool first, const bf16_t* __restrict__ x, long long nbase, int oh,
                                            int iw0, int H, int W, int C, int c, const float (&sc)[8], const float (&sh)[8]) {
  const int ih0 = oh * STRIDE - 1;
  constexpr int KEEP = 3 - STRIDE;
  if (!first) {
#pragma unroll
    for (int r = 0; r < KEEP; ++r)
#pragma unroll
      for (int t = 0; t < 3; ++t) ring[r][t] = ring[r + STRIDE][t];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (r >= KEEP || first) {
#pragma unroll
      for (int t = 0; t < 3; ++t) ring[r][t] = dw3_load<ONLOAD>(x, nbase, ih0 + r, iw0 + t, H, W, C, c, sc, sh);
    }
  }
}

// y[n,oh,ow,c] = sum_{r,t} a[n, oh*S-1+r, ow*S-1+t, c] * w[r][t][c]   (flip: taps mirrored = the stride-1 data gradient)
// stats[row][2][C]: partial sums of the ROUNDED y and of its square, one row per workgroup row
template <int STRIDE, bool ONLOAD, bool STATS>
__global__ __launch_bounds__(256) void dwconv3_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ in_scale,
                                                          const float* __restrict__ in_shift, const bf16_t* __restrict__ w,
                                                          bf16_t* __restrict__ y, float* __restrict__ stats, int H, int W, int C,
                                                          Dw3Geom g, int flip) {
  __shared__ float red[STATS ? 256 * 16 : 1];
  const int tid = threadIdx.x;
  const int cslice = (int)(blockIdx.x % (unsigned)g.nslices);
  const long long ib = blockIdx.x / (unsigned)g.nslices;
  const int cvi = tid % g.cv, lane = tid / g.cv;
  const int c = (cslice * g.cv + cvi) * 8;
  Vec8 wt[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wt[k] = unpack8(*(const u32x4*)(w + (long long)(flip ? 8 - k : k) * C + c));
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = ONLOAD ? in_scale[c + e] : 1.f; sh[e] = ONLOAD ? in_shift[c + e] : 0.f; }
  f32x2 s1[4], s2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { s1[e] = f32x2{0.f, 0.f}; s2[e] = f32x2{0.f, 0.f}; }
  const long long it1 = (g.items < (ib + 1) * g.ipb) ? g.items : (ib + 1) * g.ipb;
  for (long long it = ib * g.ipb; it < it1; ++it) {            // the items of this workgroup
    const Dw3Item q = dw3_item(it, g.colgroups, g.rowsegs, g.lanes, lane, g.OH);
    if (lane >= g.lanes || q.ow >= g.OW) continue;
    const long long nbase = (long long)q.n * H;
    Vec8 ring[3][3];
    for (int oh = q.oh0; oh < q.oh1; ++oh) {                   // down the segment
      dw3_advance<STRIDE, ONLOAD>(ring, oh == q.oh0, x, nbase, oh, q.ow * STRIDE - 1, H, W, C, c, sc, sh);
      f32x2 acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = f32x2{0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __builtin_elementwise_fma(ring[r][t].v[e], wt[r * 3 + t].v[e], acc[e]);
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

// Stride-2 data gradient as a gather: dx[n,ih,iw,c] = sum over the taps (r,t) with ih+1-r and iw+1-t even of
// dy[n,(ih+1-r)/2,(iw+1-t)/2,c] * w[r][t][c] -- one or two taps per axis.  One thread per dx vector: every element of dx is written
// exactly once, in this one launch (no zero fill, no scatter).
__global__ __launch_bounds__(256) void dwconv3_dgrad_s2_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
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
  for (int r = 0; r < 3; ++r) {
    const int a = ih + 1 - r;
    if ((a & 1) || a < 0 || (a >> 1) >= OH) continue;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int b = iw + 1 - t;
      if ((b & 1) || b < 0 || (b >> 1) >= OW) continue;
      const Vec8 d = unpack8(ld_stream((const u32x4*)(dy + ((n * OH + (a >> 1)) * OW + (b >> 1)) * C + c)));
      const Vec8 wv = unpack8(*(const u32x4*)(w + (long long)(r * 3 + t) * C + c));
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_elementwise_fma(d.v[e], wv.v[e], acc[e]);
    }
  }
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[e][0], acc[e][1]);
  *(u32x4*)(dx + i * 8) = o;
}

// dw[r][t][c] = sum_{n,oh,ow} dy[n,oh,ow,c] * a[n, oh*S-1+r, ow*S-1+t, c]: the forward's walk with the nine tap sums in registers.
// The column lanes of a workgroup are folded through LDS one kernel row at a time, lane 0 first; part[row][9][C], folded over the
// rows by the slab reducer.
template <int STRIDE, bool ONLOAD>
__global__ __launch_bounds__(256) void dwconv3_wgrad_kernel(const bf16_t* __restrict__ x, const float* __restrict__ in_scale,
                                                            const float* __restrict__ in_shift, const bf16_t* __restrict__ dy,
                                                            float* __restrict__ part, int H, int W, int C, Dw3Geom g) {
  __shared__ float red[256 * 24];
  const int tid = threadIdx.x;
  const int cslice = (int)(blockIdx.x % (unsigned)g.nslices);
  const long long ib = blockIdx.x / (unsigned)g.nslices;
  const int cvi = tid % g.cv, lane = tid / g.cv;
  const int c = (cslice * g.cv + cvi) * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = ONLOAD ? in_scale[c + e] : 1.f; sh[e] = ONLOAD ? in_shift[c + e] : 0.f; }
  Vec8 acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[k].v[e] = f32x2{0.f, 0.f};
  const long long it1 = (g.items < (ib + 1) * g.ipb) ? g.items : (ib + 1) * g.ipb;
  for (long long it = ib * g.ipb; it < it1; ++it) {            // the items of this workgroup
    const Dw3Item q = dw3_item(it, g.colgroups, g.rowsegs, g.lanes, lane, g.OH);
    if (lane >= g.lanes || q.ow >= g.OW) continue;
    const long long nbase = (long long)q.n * H;
    Vec8 ring[3][3];
    for (int oh = q.oh0; oh < q.oh1; ++oh) {                   // down the segment
      const Vec8 d = unpack8(ld_stream((const u32x4*)(dy + (((long long)q.n * g.OH + oh) * g.OW + q.ow) * C + c)));
      dw3_advance<STRIDE, ONLOAD>(ring, oh == q.oh0, x, nbase, oh, q.ow * STRIDE - 1, H, W, C, c, sc, sh);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r * 3 + t].v[e] = __builtin_elementwise_fma(ring[r][t].v[e], d.v[e], acc[r * 3 + t].v[e]);
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        red[tid * 24 + t * 8 + 2 * e] = acc[r * 3 + t].v[e][0];
        red[tid * 24 + t * 8 + 2 * e + 1] = acc[r * 3 + t].v[e][1];
      }
    __syncthreads();
    for (int o = tid; o < g.cv * 24; o += 256) {
      const int cvo = o / 24, k = o - cvo * 24;                // k = tap-in-row * 8 + channel of the vector
      float s = 0.f;
      for (int l = 0; l < g.lanes; ++l) s += red[(l * g.cv + cvo) * 24 + k];
      part[(ib * 9 + r * 3 + (k >> 3)) * C + (cslice * g.cv + cvo) * 8 + (k & 7)] = s;
    }
  }
}

// ---- BatchNorm + ReLU6 ------------------------------------------------------------------------------------------------------------
// out = bf16(min(max(y * scale[c] + shift[c], 0), 6)); 8 channels per thread, grid-stride with a loop-invariant channel group
__global__ __launch_bounds__(256) void bn_apply_relu6_kernel(const bf16_t* __restrict__ y, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, bf16_t* __restrict__ out,
                                                             long long nvec, int cpr) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = (int)(i % cpr) * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = scale[cg + e]; sh[e] = shift[cg + e]; }
  for (; i < nvec; i += stride) ((u32x4*)out)[i] = bn_relu6_8(ld_stream((const u32x4*)y + i), sc, sh);
}

// g = dout where 0 < y * scale + shift < 6 (both strict, the forward's own fp32 expression), else 0
__device__ __forceinline__ void relu6_masked_g(const u32x4 d, const u32x4 yv, const float (&sc)[8], const float (&sh)[8], float (&g)[8],
                                               float (&yy)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    g[2 * e] = bf16_lo(d[e]); g[2 * e + 1] = bf16_hi(d[e]);
    yy[2 * e] = bf16_lo(yv[e]); yy[2 * e + 1] = bf16_hi(yv[e]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float z = fmaf(yy[e], sc[e], sh[e]);
    if (!(z > 0.f && z < 6.f)) g[e] = 0.f;
  }
}

// pass 1: part[blk][2][C] = (sum g, sum g * xhat) over the block's rows; thread -> (channel group, row lane), as the reduce pass of
// icamd_bn_bwd (norm_pool.hip), whose finalize kernel folds these rows.  This kernel and the apply pass below are twins of
// bn_bwd_reduce_kernel / bn_bwd_apply_kernel there (a template parameter on those would have rebuilt the existing instantiations):
// the sums and the dy expression must stay the same in both places
__global__ __launch_bounds__(256) void bn_bwd_relu6_reduce_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                                  const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  float* __restrict__ part, long long rows, int C, int rows_per_block) {
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
        float g[8], yy[8];
        relu6_masked_g(ld_stream((const u32x4*)dout + off), ld_stream((const u32x4*)y + off), sc, sh, g, yy);
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
__global__ __launch_bounds__(256) void bn_bwd_relu6_apply_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ c1, const float* __restrict__ c2,
                                                                 bf16_t* __restrict__ dy, long long nvec, int cpr) {
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
    float g[8], yy[8], o[8];
    relu6_masked_g(ld_stream((const u32x4*)dout + i), ld_stream((const u32x4*)y + i), sc, sh, g, yy);
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

// `cap`: the most partial rows wanted; `pixels_per_row`: at least this many output pixels behind every partial row, so that the
// rows stay a small fraction of the tensor ([2][C] fp32 per row against 2 C bytes per pixel)
bool dw3_geometry(int N, int H, int W, int C, int stride, long long cap, long long pixels_per_row, Dw3Geom* out) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (stride != 1 && stride != 2)) return false;
  Dw3Geom g;
  g.OH = (H - 1) / stride + 1;
  g.OW = (W - 1) / stride + 1;
  g.cpr = C / 8;
  // the widest divisor of cpr (whole channel runs per pixel) whose multiples fill 192 of the 256 threads at least: 66 -> 66 x 3,
  // 168 -> 84 x 3, 90 -> 45 x 5; d = 1 fills them all, so the search ends
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
  if (g.rows * g.nslices >= (1ll << 31)) return false;
  if (((long long)N * H * W * g.cpr + 255) / 256 >= (1ll << 31)) return false;   // the gather's grid
  *out = g;
  return true;
}
bool dw3_fwd_geometry(int N, int H, int W, int C, int stride, Dw3Geom* g) { return dw3_geometry(N, H, W, C, stride, 2048, 16, g); }
bool dw3_wgrad_geometry(int N, int H, int W, int C, int stride, Dw3Geom* g) { return dw3_geometry(N, H, W, C, stride, 1024, 64, g); }

}  // namespace

bool icamd_dwconv3_ok(int N, int H, int W, int C, int stride) {
  Dw3Geom g;
  return dw3_fwd_geometry(N, H, W, C, stride, &g) && dw3_wgrad_geometry(N, H, W, C, stride, &g);
}

long long icamd_dwconv3_stats_rows_cxx(int N, int H, int W, int C, int stride) {
  Dw3Geom g;
  return icamd_dwconv3_ok(N, H, W, C, stride) && dw3_fwd_geometry(N, H, W, C, stride, &g) ? g.rows : 0;
}

long long icamd_dwconv3_wgrad_rows(int N, int H, int W, int C, int stride) {
  Dw3Geom g;
  return icamd_dwconv3_ok(N, H, W, C, stride) && dw3_wgrad_geometry(N, H, W, C, stride, &g) ? g.rows : 0;
}

int icamd_dwconv3_fwd_launch(const bf16_t* x, const float* in_scale, const float* in_shift, const bf16_t* w, bf16_t* y, float* stats,
                             int N, int H, int W, int C, int stride, int flip, hipStream_t s) {
  Dw3Geom g;
  if (!icamd_dwconv3_ok(N, H, W, C, stride) || !dw3_fwd_geometry(N, H, W, C, stride, &g)) return ICAMD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(g.rows * g.nslices)), block(256);
  const bool on = in_scale != nullptr, st = stats != nullptr;
#define DW3_FWD(S, O, T) \
  hipLaunchKernelGGL((dwconv3_fwd_kernel<S, O, T>), grid, block, 0, s, x, in_scale, in_shift, w, y, stats, H, W, C, g, flip)
  if (stride == 1) {
    if (on) { if (st) DW3_FWD(1, true, true); else DW3_FWD(1, true, false); }
    else { if (st) DW3_FWD(1, false, true); else DW3_FWD(1, false, false); }
  } else {
    if (on) { if (st) DW3_FWD(2, true, true); else DW3_FWD(2, true, false); }
    else { if (st) DW3_FWD(2, false, true); else DW3_FWD(2, false, false); }
  }
#undef DW3_FWD
  return icamd_launch_status();
}

// dy [N][OH][OW][C] -> dx [N][H][W][C]
int icamd_dwconv3_dgrad_launch(const bf16_t* dy, const bf16_t* w, bf16_t* dx, int N, int H, int W, int C, int stride, hipStream_t s) {
  if (!icamd_dwconv3_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  if (stride == 1) return icamd_dwconv3_fwd_launch(dy, nullptr, nullptr, w, dx, nullptr, N, H, W, C, 1, /*flip=*/1, s);
  const long long nvec = (long long)N * H * W * (C / 8);
  hipLaunchKernelGGL(dwconv3_dgrad_s2_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, dy, w, dx, nvec, H, W, C,
                     (H - 1) / 2 + 1, (W - 1) / 2 + 1);
  return icamd_launch_status();
}

int icamd_dwconv3_wgrad_launch(const bf16_t* x, const float* in_scale, const float* in_shift, const bf16_t* dy, float* part, float* dw,
                               int N, int H, int W, int C, int stride, int accumulate, hipStream_t s) {
  Dw3Geom g;
  if (!icamd_dwconv3_ok(N, H, W, C, stride) || !dw3_wgrad_geometry(N, H, W, C, stride, &g)) return ICAMD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(g.rows * g.nslices)), block(256);
  const bool on = in_scale != nullptr;
#define DW3_WGRAD(S, O) hipLaunchKernelGGL((dwconv3_wgrad_kernel<S, O>), grid, block, 0, s, x, in_scale, in_shift, dy, part, H, W, C, g)
  if (stride == 1) { if (on) DW3_WGRAD(1, true); else DW3_WGRAD(1, false); }
  else { if (on) DW3_WGRAD(2, true); else DW3_WGRAD(2, false); }
#undef DW3_WGRAD
  const int rc = icamd_launch_status();
  if (rc) return rc;
  return icamd_slab_reduce_launch(part, dw, 9ll * C, (int)g.rows, accumulate, s);
}

int icamd_bn_apply_relu6_launch(const bf16_t* y, const float* scale, const float* shift, bf16_t* out, long long numel, int C,
                                hipStream_t s) {
  if (C % 8 != 0 || numel % C != 0) return ICAMD_ERR_BAD_ARG;
  const long long nvec = numel / 8;
  hipLaunchKernelGGL(bn_apply_relu6_kernel, dim3(elementwise_grid(nvec, C / 8)), dim3(256), 0, s, y, scale, shift, out, nvec, C / 8);
  return icamd_launch_status();
}

// part: [icamd_bn_bwd_rows_per_block blocks][2][C]; chunks / c1c2: the regions of icamd_bn_bwd's workspace
int icamd_bn_bwd_relu6_launch(const bf16_t* dout, const bf16_t* y, const float* mean, const float* invstd, const float* scale,
                              const float* shift, float* dgamma, float* dbeta, bf16_t* dy, long long rows, int C, int accumulate,
                              float* part, double* chunks, float* c1c2, hipStream_t s) {
  if (C % 8 != 0) return ICAMD_ERR_BAD_ARG;
  const int rpb = icamd_bn_bwd_rows_per_block(rows, C);
  const int nblk = (int)((rows + rpb - 1) / rpb);
  hipLaunchKernelGGL(bn_bwd_relu6_reduce_kernel, dim3((unsigned)nblk), dim3(256), 0, s, dout, y, mean, invstd, scale, shift, part, rows,
                     C, rpb);
  int rc = icamd_launch_status();
  if (rc) return rc;
  rc = icamd_bn_bwd_finalize_launch(part, nblk, mean, invstd, dgamma, dbeta, rows, C, accumulate, chunks, c1c2, s, 0);
  if (rc) return rc;
  const long long nvec = rows * (C / 8);
  hipLaunchKernelGGL(bn_bwd_relu6_apply_kernel, dim3(elementwise_grid(nvec, C / 8)), dim3(256), 0, s, dout, y, mean, invstd, scale,
                     shift, c1c2, c1c2 + C, dy, nvec, C / 8);
  return icamd_launch_status();
}
