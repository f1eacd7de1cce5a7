// Global Response Normalisation (ConvNeXt V2), channels-last, on a = gelu(z1) of shape [N][HW][C] bf16, C = 4 dim:
//   Gx[n,c] = sqrt(sum_hw a^2)     m_n = mean_c Gx[n,:] + eps     Nx = Gx / m_n     s = 1 + gamma Nx
//   g  = a s[n,c] + beta[c]
//   da = dg s[n,c] + a t[n,c],     t = Gx > 0 ? dG / Gx : 0,   dG = dN / m_n - (sum_c' dN Gx) / (C m_n^2),   dN = gamma P
//   P[n,c] = sum_hw dg a,  Q[n,c] = sum_hw dg,   dgamma[c] = sum_n P Nx,   dbeta[c] = sum_n Q
// Two launches each way, both HBM-bound passes over the wide tensors (16 B per lane on every bf16 stream):
//   reduce  grid (column tiles, S row segments, N): lanes run along the channels, a thread keeps the running sums of its 8 channels
//           in registers across the rows of its segment; the row lanes of a workgroup meet in LDS; ONE partial row per workgroup
//   apply   grid (B row blocks, N): the prologue folds the S partial rows of its sample in a fixed order and forms m_n, s (and t)
//           for all C channels in LDS -- at most 6144 floats per sample, so no launch of its own --, then one pass over the rows
// No float atomics anywhere: two launches on the same inputs give the same bits.  The backward's finishing launch sums the
// per-sample rows P Nx and Q over n in a fixed order into dgamma / dbeta (fp32, accumulate flag).
#include "icamd_internal.h"
#include "workspace.h"

namespace {

constexpr int GRN_THREADS = 256;
constexpr int GRN_MAX_C = 6144;

// sums over the rows [r0, r1) of sample blockIdx.z, columns of tile blockIdx.x: NSUM == 1: a^2;  NSUM == 2: dg a and dg
template <int NSUM>
__global__ __launch_bounds__(GRN_THREADS) void grn_reduce_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ dg,
                                                                 float* __restrict__ part, int HW, int C, int tcols, int rps,
                                                                 int S) {
  __shared__ float red[GRN_THREADS * 8 * NSUM];
  const int cpr = C >> 3;
  const int tid = threadIdx.x;
  const int n = blockIdx.z, seg = blockIdx.y, cg0 = blockIdx.x * tcols;
  const int rlanes = GRN_THREADS / tcols;
  const int cgi = tid % tcols, rl = tid / tcols;
  const int r0 = seg * rps;
  const int r1 = (HW < r0 + rps) ? HW : r0 + rps;
  const u32x4* av = (const u32x4*)a + (long long)n * HW * cpr + cg0 + cgi;
  const u32x4* dv = (const u32x4*)dg + (long long)n * HW * cpr + cg0 + cgi;
  float s0[8], s1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
  if (rl < rlanes) {
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += rlanes) {
      const u32x4 x = ld_stream(av + (long long)r * cpr);
      if constexpr (NSUM == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = bf16_lo(x[e]), hi = bf16_hi(x[e]);
          s0[2 * e] = fmaf(lo, lo, s0[2 * e]);
          s0[2 * e + 1] = fmaf(hi, hi, s0[2 * e + 1]);
        }
      } else {
        const u32x4 d = ld_stream(dv + (long long)r * cpr);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dl = bf16_lo(d[e]), dh = bf16_hi(d[e]);
          s0[2 * e] = fmaf(dl, bf16_lo(x[e]), s0[2 * e]);
          s0[2 * e + 1] = fmaf(dh, bf16_hi(x[e]), s0[2 * e + 1]);
          s1[2 * e] += dl;
          s1[2 * e + 1] += dh;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[tid * 8 + e] = s0[e];
    if constexpr (NSUM == 2) red[GRN_THREADS * 8 + tid * 8 + e] = s1[e];
  }
  __syncthreads();
  // part[n][seg][NSUM][C]: the row lanes summed in lane order
  float* prow = part + ((long long)n * S + seg) * NSUM * C + cg0 * 8;
  for (int o = tid; o < tcols * 8 * NSUM; o += GRN_THREADS) {
    const int which = o / (tcols * 8), oc = o - which * tcols * 8;
    const int cgo = oc >> 3, e = oc & 7;
    float t = 0.f;
    for (int l = 0; l < rlanes; ++l) t += red[which * GRN_THREADS * 8 + (l * tcols + cgo) * 8 + e];
    prow[which * C + oc] = t;
  }
}

// sum of v over the workgroup, the same bits in every thread and in every workgroup that sums the same values
__device__ __forceinline__ float block_sum(float v, float* wsum) {
  v = wave_sum(v);
  __syncthreads();   // wsum may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < GRN_THREADS / 64; ++w) t += wsum[w];
  return t;
}

// The per-sample finalisation, in every workgroup of the sample: lds_gx[c] = Gx, returns m_n.  gx != nullptr: the statistic is read
// (backward); otherwise it is folded from the S partial rows of sums of squares (forward).
// A thread takes four channels at a time (16 B loads of the fp32 rows, C / 1024 trips): the prologue is a chain of L2 latencies, not
// of bytes, and every workgroup of the sample pays it.
__device__ __forceinline__ float grn_stats(const float* __restrict__ part, const float* __restrict__ gx, float* lds_gx, float* wsum,
                                           int n, int C, int S, float eps) {
  const int C4 = C >> 2;
  float local = 0.f;
  for (int c4 = threadIdx.x; c4 < C4; c4 += GRN_THREADS) {
    f32x4 g;
    if (gx != nullptr) {
      g = *((const f32x4*)(gx + (long long)n * C) + c4);
    } else {
      const f32x4* row = (const f32x4*)(part + (long long)n * S * C) + c4;
      f32x4 ss = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int s = 0; s < S; ++s) ss += row[(long long)s * C4];
      g = f32x4{sqrtf(ss[0]), sqrtf(ss[1]), sqrtf(ss[2]), sqrtf(ss[3])};
    }
    *((f32x4*)lds_gx + c4) = g;
    local += (g[0] + g[1]) + (g[2] + g[3]);
  }
  return block_sum(local, wsum) / (float)C + eps;
}

// g = a s[n,c] + beta[c] over the rows [blockIdx.x * rpb, ...) of sample blockIdx.y; block 0 of a sample leaves Gx[n,:]
__global__ __launch_bounds__(GRN_THREADS) void grn_fwd_apply_kernel(const bf16_t* __restrict__ a, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, bf16_t* __restrict__ g,
                                                                    float* __restrict__ gx_out, const float* __restrict__ part,
                                                                    int HW, int C, int S, int rpb, float eps) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // s[C] | beta[C]
  __shared__ float wsum[GRN_THREADS / 64];
  float* ls = lds;
  float* lb = lds + C;
  const int n = blockIdx.y, tid = threadIdx.x;
  const float m = grn_stats(part, nullptr, ls, wsum, n, C, S, eps);
  const float inv_m = 1.f / m;
  for (int c4 = tid; c4 < (C >> 2); c4 += GRN_THREADS) {   // each thread revisits the channels it wrote
    const f32x4 gxv = *((const f32x4*)ls + c4);
    if (blockIdx.x == 0) *((f32x4*)(gx_out + (long long)n * C) + c4) = gxv;
    const f32x4 gm = *((const f32x4*)gamma + c4);
    f32x4 sv;
#pragma unroll
    for (int e = 0; e < 4; ++e) sv[e] = fmaf(gm[e], gxv[e] * inv_m, 1.f);
    *((f32x4*)ls + c4) = sv;
    *((f32x4*)lb + c4) = *((const f32x4*)beta + c4);
  }
  __syncthreads();
  const int cpr = C >> 3;
  const int r0 = blockIdx.x * rpb;
  const int r1 = (HW < r0 + rpb) ? HW : r0 + rpb;
  const int v1 = r1 * cpr;
  const int step = GRN_THREADS % cpr;
  const u32x4* av = (const u32x4*)a + (long long)n * HW * cpr;
  u32x4* gv = (u32x4*)g + (long long)n * HW * cpr;
  int cg = (r0 * cpr + tid) % cpr;
#pragma unroll 2
  for (int i = r0 * cpr + tid; i < v1; i += GRN_THREADS) {
    const u32x4 x = ld_stream(av + i);
    const f32x4 sa = *(const f32x4*)(ls + cg * 8), sb = *(const f32x4*)(ls + cg * 8 + 4);
    const f32x4 ba = *(const f32x4*)(lb + cg * 8), bb = *(const f32x4*)(lb + cg * 8 + 4);
    u32x4 o;
    o[0] = pack_bf16x2(fmaf(bf16_lo(x[0]), sa[0], ba[0]), fmaf(bf16_hi(x[0]), sa[1], ba[1]));
    o[1] = pack_bf16x2(fmaf(bf16_lo(x[1]), sa[2], ba[2]), fmaf(bf16_hi(x[1]), sa[3], ba[3]));
    o[2] = pack_bf16x2(fmaf(bf16_lo(x[2]), sb[0], bb[0]), fmaf(bf16_hi(x[2]), sb[1], bb[1]));
    o[3] = pack_bf16x2(fmaf(bf16_lo(x[3]), sb[2], bb[2]), fmaf(bf16_hi(x[3]), sb[3], bb[3]));
    gv[i] = o;
    cg += step;
    if (cg >= cpr) cg -= cpr;
  }
}

// dx = (dg s[n,c] + a t[n,c]) (* gelu'(z)); block 0 of a sample leaves fin[n][0][c] = P Nx and fin[n][1][c] = Q
template <bool GELU>
__global__ __launch_bounds__(GRN_THREADS) void grn_bwd_apply_kernel(const bf16_t* __restrict__ dg, const bf16_t* __restrict__ a,
                                                                    const float* __restrict__ gx, const float* __restrict__ gamma,
                                                                    const bf16_t* __restrict__ z, bf16_t* __restrict__ dx,
                                                                    const float* __restrict__ part, float* __restrict__ fin,
                                                                    int HW, int C, int S, int rpb, float eps) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // s[C] | t[C]
  __shared__ float wsum[GRN_THREADS / 64];
  float* ls = lds;
  float* lt = lds + C;
  const int n = blockIdx.y, tid = threadIdx.x;
  const float m = grn_stats(nullptr, gx, ls, wsum, n, C, S, eps);
  const float inv_m = 1.f / m;
  // P, Q folded from the S partial rows in segment order; dN = gamma P kept in lt until the dot product is known
  const int C4 = C >> 2;
  float dot = 0.f;
  for (int c4 = tid; c4 < C4; c4 += GRN_THREADS) {
    const f32x4* row = (const f32x4*)(part + (long long)n * S * 2 * C) + c4;
    f32x4 p = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    // block 0 owes the parameter gradients Q of every channel; the others need only P
    if (blockIdx.x == 0) {
#pragma unroll 2
      for (int s = 0; s < S; ++s) {
        p += row[(long long)s * 2 * C4];
        q += row[(long long)s * 2 * C4 + C4];
      }
    } else {
#pragma unroll 4
      for (int s = 0; s < S; ++s) p += row[(long long)s * 2 * C4];
    }
    const f32x4 gxv = *((const f32x4*)ls + c4);
    if (blockIdx.x == 0) {
      *((f32x4*)(fin + ((long long)n * 2 + 0) * C) + c4) = p * (gxv * inv_m);
      *((f32x4*)(fin + ((long long)n * 2 + 1) * C) + c4) = q;
    }
    const f32x4 dn = *((const f32x4*)gamma + c4) * p;
    *((f32x4*)lt + c4) = dn;
#pragma unroll
    for (int e = 0; e < 4; ++e) dot = fmaf(dn[e], gxv[e], dot);
  }
  dot = block_sum(dot, wsum);
  const float sub = dot * inv_m * inv_m / (float)C;
  for (int c4 = tid; c4 < C4; c4 += GRN_THREADS) {
    const f32x4 gxv = *((const f32x4*)ls + c4), dn = *((const f32x4*)lt + c4), gm = *((const f32x4*)gamma + c4);
    f32x4 tv, sv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float dG = dn[e] * inv_m - sub;
      tv[e] = gxv[e] > 0.f ? dG / gxv[e] : 0.f;
      sv[e] = fmaf(gm[e], gxv[e] * inv_m, 1.f);
    }
    *((f32x4*)lt + c4) = tv;
    *((f32x4*)ls + c4) = sv;
  }
  __syncthreads();
  const int cpr = C >> 3;
  const int r0 = blockIdx.x * rpb;
  const int r1 = (HW < r0 + rpb) ? HW : r0 + rpb;
  const int v1 = r1 * cpr;
  const int step = GRN_THREADS % cpr;
  const long long base = (long long)n * HW * cpr;
  const u32x4* av = (const u32x4*)a + base;
  const u32x4* dv = (const u32x4*)dg + base;
  const u32x4* zv = (const u32x4*)z + base;
  u32x4* ov = (u32x4*)dx + base;
  int cg = (r0 * cpr + tid) % cpr;
#pragma unroll 2
  for (int i = r0 * cpr + tid; i < v1; i += GRN_THREADS) {
    const u32x4 x = ld_stream(av + i);
    const u32x4 d = ld_stream(dv + i);
    float sv[8], tv[8];
    *(f32x4*)sv = *(const f32x4*)(ls + cg * 8);
    *(f32x4*)(sv + 4) = *(const f32x4*)(ls + cg * 8 + 4);
    *(f32x4*)tv = *(const f32x4*)(lt + cg * 8);
    *(f32x4*)(tv + 4) = *(const f32x4*)(lt + cg * 8 + 4);
    u32x4 zz = {0u, 0u, 0u, 0u};
    if constexpr (GELU) zz = ld_stream(zv + i);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f32x2 da = {fmaf(bf16_lo(d[e]), sv[2 * e], bf16_lo(x[e]) * tv[2 * e]),
                  fmaf(bf16_hi(d[e]), sv[2 * e + 1], bf16_hi(x[e]) * tv[2 * e + 1])};
      if constexpr (GELU) da = da * gelu_grad2(f32x2{bf16_lo(zz[e]), bf16_hi(zz[e])});
      o[e] = pack_bf16x2(da[0], da[1]);
    }
    ov[i] = o;
    cg += step;
    if (cg >= cpr) cg -= cpr;
  }
}

// dgamma[c] (+)= sum_n fin[n][0][c], dbeta[c] (+)= sum_n fin[n][1][c]: 64 channels (the last workgroup: what is left of C) x 4
// sample lanes per workgroup, the samples of a lane in order, the lanes in order
__global__ __launch_bounds__(GRN_THREADS) void grn_param_grads_kernel(const float* __restrict__ fin, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta, int N, int C, int accumulate) {
  __shared__ float red[2][4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), lane = threadIdx.x >> 6;
  const bool live = c < C;   // C % 64 == 32: the upper half of the last workgroup's channels does not exist
  float p = 0.f, q = 0.f;
#pragma unroll 4
  for (int n = live ? lane : N; n < N; n += 4) {
    p += fin[((long long)n * 2 + 0) * C + c];
    q += fin[((long long)n * 2 + 1) * C + c];
  }
  red[0][lane][threadIdx.x & 63] = p;
  red[1][lane][threadIdx.x & 63] = q;
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, cc = threadIdx.x & 63;
    const float t = ((red[which][0][cc] + red[which][1][cc]) + red[which][2][cc]) + red[which][3][cc];
    float* out = (which ? dbeta : dgamma) + blockIdx.x * 64 + cc;
    if (blockIdx.x * 64 + cc < C) *out = accumulate ? *out + t : t;
  }
}

// vector columns of a reduce workgroup: all of them up to 256, else the largest divisor of C / 8 that is a multiple of 8
// (C % 64 == 0) or of 4 (C % 64 == 32: C / 8 is a multiple of 4 only)
int reduce_tcols(int cpr) {
  if (cpr <= GRN_THREADS) return cpr;
  const int q = cpr % 8 == 0 ? 8 : 4;
  for (int t = GRN_THREADS; t >= q; t -= q)
    if (cpr % t == 0) return t;
  return q;
}

}  // namespace

bool icamd_grn_ok(int N, long long HW, int C) {
  return N >= 1 && N <= 65535 && HW >= 1 && C >= 128 && C <= GRN_MAX_C && C % 32 == 0 && HW * C < (1ll << 31);
}

// S row segments per sample for the reductions (about 2048 workgroups over the batch, 32 rows and more each, at most 64 partial
// rows for a prologue to fold), B row blocks per sample for the apply passes (four 16 B vectors per thread and 8 rows, or more)
void icamd_grn_plan(int N, int HW, int C, int* S, int* rps, int* B, int* rpb) {
  auto cdiv = [](long long x, long long y) { return (int)((x + y - 1) / y); };
  int s = cdiv(2048, N);
  if (s > cdiv(HW, 32)) s = cdiv(HW, 32);
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  *rps = cdiv(HW, s);
  *S = cdiv(HW, *rps);
  int b = cdiv((long long)HW * (C / 8), 4 * GRN_THREADS);
  if (b > cdiv(4096, N)) b = cdiv(4096, N);
  if (b > cdiv(HW, 8)) b = cdiv(HW, 8);   // 8 rows and more per block: its prologue is as long as about one row of every channel
  if (b < 1) b = 1;
  *rpb = cdiv(HW, b);
  *B = cdiv(HW, *rpb);
}

// workspace (grn_ws): partial rows [N][S][2][C] | per-sample rows of the parameter gradients [N][2][C]
size_t icamd_grn_bytes(int N, int HW, int C) {
  int S, rps, B, rpb;
  icamd_grn_plan(N, HW, C, &S, &rps, &B, &rpb);
  return grn_ws(nullptr, N, S, C).bytes;
}

int icamd_grn_fwd_launch(const bf16_t* a, const float* gamma, const float* beta, bf16_t* g, float* gx_out, int N, int HW, int C,
                         float eps, void* workspace, hipStream_t s) {
  int S, rps, B, rpb;
  icamd_grn_plan(N, HW, C, &S, &rps, &B, &rpb);
  float* part = grn_ws(workspace, N, S, C).part;
  const int cpr = C / 8, tcols = reduce_tcols(cpr);
  hipLaunchKernelGGL(grn_reduce_kernel<1>, dim3(cpr / tcols, S, N), dim3(GRN_THREADS), 0, s, a, nullptr, part, HW, C, tcols, rps, S);
  hipLaunchKernelGGL(grn_fwd_apply_kernel, dim3(B, N), dim3(GRN_THREADS), 2 * C * sizeof(float), s, a, gamma, beta, g, gx_out, part,
                     HW, C, S, rpb, eps);
  return icamd_launch_status();
}

int icamd_grn_bwd_launch(const bf16_t* dg, const bf16_t* a, const float* gx, const float* gamma, const bf16_t* z, bf16_t* dx,
                         float* dgamma, float* dbeta, int accumulate, int N, int HW, int C, float eps, void* workspace,
                         hipStream_t s) {
  int S, rps, B, rpb;
  icamd_grn_plan(N, HW, C, &S, &rps, &B, &rpb);
  const GrnWs w = grn_ws(workspace, N, S, C);
  float *part = w.part, *fin = w.fin;
  const int cpr = C / 8, tcols = reduce_tcols(cpr);
  hipLaunchKernelGGL(grn_reduce_kernel<2>, dim3(cpr / tcols, S, N), dim3(GRN_THREADS), 0, s, a, dg, part, HW, C, tcols, rps, S);
  if (z != nullptr)
    hipLaunchKernelGGL(grn_bwd_apply_kernel<true>, dim3(B, N), dim3(GRN_THREADS), 2 * C * sizeof(float), s, dg, a, gx, gamma, z, dx,
                       part, fin, HW, C, S, rpb, eps);
  else
    hipLaunchKernelGGL(grn_bwd_apply_kernel<false>, dim3(B, N), dim3(GRN_THREADS), 2 * C * sizeof(float), s, dg, a, gx, gamma, z, dx,
                       part, fin, HW, C, S, rpb, eps);
  hipLaunchKernelGGL(grn_param_grads_kernel, dim3((C + 63) / 64), dim3(GRN_THREADS), 0, s, fin, dgamma, dbeta, N, C, accumulate);
  return icamd_launch_status();
}
