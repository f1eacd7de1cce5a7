// Kernels of the ResNet-D variants ("Bag of Tricks": timm resnet50d and siblings, stem_type='deep', avg_down=True) for gfx950:
//
// 1. 2x2 / stride 2 average pool, ceil_mode, count_include_pad=False (the pool in front of a D block's projection shortcut),
//    NHWC bf16, C % 8 == 0: forward, and backward with the main branch's gradient as an optional addend.  Pure streaming kernels:
//    one lane = 16 B = 8 channels of one output window, consecutive lanes on consecutive channels; the full-resolution tensor is
//    touched once and goes past the caches (non-temporal), the quarter-size one is read / written normally.
//
// 2. "Thin" 3x3 / pad 1 / stride 1 convolution with 32 input channels and 32 or 64 output channels (the second and third
//    convolution of the deep stem, at 112 x 112 for a 224 x 224 image): forward, data gradient, weight gradient.
//    With 32 input channels one filter tap is exactly one v_mfma_f32_16x16x32_bf16 k-step: K = 9 steps per output fragment.
//
//    Forward / data gradient (one kernel, two modes): a workgroup walks over tiles of SB = 256 / 128 / 64 consecutive output
//    pixels in (n, h, w) raster order.  The input rows of a tile (first pixel - W - 1 .. last pixel + W + 1) are staged ONCE by
//    LDS-DMA, 16 B per lane, the 16 B chunks of a row rotated by the slot number (conflict-free ds_read_b128 of a 16-slot
//    fragment); a tap is an offset dh * W + dw on the slot, taps that leave the image read the tile's zero slot.  The WHOLE
//    filter stays resident in registers for all tiles of the workgroup (36 KB over the four waves' fragments: 144 VGPRs per lane
//    at 64 output channels): wave w takes the pixel fragments w, w + 4, ... of a tile and ALL output-channel blocks, so that an
//    input fragment is read from LDS once and multiplied by every filter block.  The data gradient reads the FORWARD filter
//    layout [Cout][3][3][32] and gathers its transposed, tap-mirrored fragments itself (once per workgroup), so these layers
//    need no slot in the transposed shadow; its reduction runs over Cout = 32 or 64 channels: one or two k-steps per tap.
//    The output tile goes through LDS (the staging area, after a barrier) and leaves as 16 B per lane; the forward adds the
//    per-channel sum / sum of squares of the ROUNDED outputs on the way, one partial row per tile (icamd_conv3x3_thin_stats_rows).
//
//    Weight gradient: workgroup = contiguous range of 128 / 64 / 32-pixel tiles; the reduction index is the pixel, both operands
//    are read with ds_read_b64_tr_b16 from the staged row images; wave = one 16-channel block of dy (Cout = 64: with both input
//    blocks; Cout = 32: one of the two), its D[ci][co] fragments of the nine taps stay in registers over the whole range and
//    leave as one fp32 slab [S][Cout][9][32], folded in fixed order by the shared slab reduction: bitwise reproducible.
//
//    Not done here: staging of tile i + 1 is not overlapped with the MFMAs of tile i inside a workgroup (two workgroups per CU
//    cover for each other), the tiles are raster-linear rather than square (the halo of a 256-pixel tile at W = 112 is 0.9 tiles:
//    the overlap comes from L2), and BatchNorm + ReLU of the previous stem layer is not applied while staging.
#define ICAMD_STREAM_NT 1
#include "common.h"
#include "icamd_internal.h"

namespace {

// =================================================================================================================================
// 2x2 average pool
// =================================================================================================================================
// the full-resolution tensor is read / written once: non-temporal under ICAMD_STREAM_NT (common.h), as the other streaming units
__device__ __forceinline__ u32x4 ld_nt(const bf16_t* p) { return ld_stream((const u32x4*)p); }
__device__ __forceinline__ void st_nt(bf16_t* p, u32x4 v) {
  if constexpr (ICAMD_STREAM_NT != 0) __builtin_nontemporal_store(v, (u32x4*)p);
  else *(u32x4*)p = v;
}

__device__ __forceinline__ void acc8(float* s, const u32x4 v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { s[2 * e] += bf16_lo(v[e]); s[2 * e + 1] += bf16_hi(v[e]); }
}

// lane -> (window, 8-channel chunk)
__device__ __forceinline__ void pool_coords(const Pool2x2Params& p, unsigned int idx, int& n, int& oh, int& ow, int& c) {
  const unsigned int pix = fdiv(idx, p.divC8);
  c = (int)(idx - pix * (unsigned)p.C8) * 8;
  const unsigned int t = fdiv(pix, p.divOW);
  ow = (int)(pix - t * (unsigned)p.OW);
  const unsigned int nn = fdiv(t, p.divOH);
  oh = (int)(t - nn * (unsigned)p.OH);
  n = (int)nn;
}

__global__ __launch_bounds__(256) void avgpool2x2_fwd_kernel(const Pool2x2Params p) {
  const unsigned int idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= p.total) return;
  int n, oh, ow, c;
  pool_coords(p, idx, n, oh, ow, c);
  const int C = p.C8 * 8;
  const int nh = (2 * oh + 1 < p.IH) ? 2 : 1, nw = (2 * ow + 1 < p.IW) ? 2 : 1;
  const bf16_t* src = p.in + (((long long)n * p.IH + 2 * oh) * p.IW + 2 * ow) * C + c;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  acc8(s, ld_nt(src));
  if (nw == 2) acc8(s, ld_nt(src + C));
  if (nh == 2) {
    acc8(s, ld_nt(src + (long long)p.IW * C));
    if (nw == 2) acc8(s, ld_nt(src + (long long)p.IW * C + C));
  }
  const float inv = 1.0f / (float)(nh * nw);      // 1, 0.5 or 0.25: the product is exact, the store is the only rounding
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(s[2 * e] * inv, s[2 * e + 1] * inv);
  *(u32x4*)(p.out + (long long)idx * 8) = o;
}

__global__ __launch_bounds__(256) void avgpool2x2_bwd_kernel(const Pool2x2Params p) {
  const unsigned int idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= p.total) return;
  int n, oh, ow, c;
  pool_coords(p, idx, n, oh, ow, c);
  const int C = p.C8 * 8;
  const int nh = (2 * oh + 1 < p.IH) ? 2 : 1, nw = (2 * ow + 1 < p.IW) ? 2 : 1;
  const float inv = 1.0f / (float)(nh * nw);
  const u32x4 g = *(const u32x4*)(p.in + (long long)idx * 8);
  float gs[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) { gs[2 * e] = bf16_lo(g[e]) * inv; gs[2 * e + 1] = bf16_hi(g[e]) * inv; }
  const long long off0 = (((long long)n * p.IH + 2 * oh) * p.IW + 2 * ow) * C + c;
  for (int a = 0; a < nh; ++a)
    for (int b = 0; b < nw; ++b) {
      const long long off = off0 + ((long long)a * p.IW + b) * C;
      u32x4 o;
      if (p.addend != nullptr) {
        const u32x4 ad = ld_nt(p.addend + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(bf16_lo(ad[e]) + gs[2 * e], bf16_hi(ad[e]) + gs[2 * e + 1]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(gs[2 * e], gs[2 * e + 1]);
      }
      st_nt(p.out + off, o);
    }
}

// =================================================================================================================================
// thin 3x3 convolution
// =================================================================================================================================
__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* p0, const unsigned char* p1) {
  bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)p0);
  bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)p1);
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// LDS rows of NCH * 16 B: slot j (0 <= j < nalloc, nalloc % 16 == 0) <- the row of pixel base + j of src; zeros where j >= nsl or
// the pixel is outside [0, npix).  Logical 16 B chunk c of slot j sits at position (c + j) & (NCH - 1).
template <int NCH>
__device__ __forceinline__ void stage_rows(unsigned char* dst, const bf16_t* __restrict__ src, int base, int nsl, int nalloc,
                                           int npix, int wave, int lane) {
  constexpr int SPI = 64 / NCH;                  // slots per LDS-DMA instruction (1 KB)
  const bf16_t* zero = (const bf16_t*)icamd_zero_page;
  const int nin = nalloc / SPI;
  for (int it = wave; it < nin; it += 4) {
    const int slot = it * SPI + lane / NCH;
    const int pix = base + slot;
    const int lc = (((lane % NCH) - slot) & (NCH - 1)) * 8;
    const bf16_t* s = (slot < nsl && pix >= 0 && pix < npix) ? src + ((long long)pix * (NCH * 8) + lc) : zero;
    __builtin_amdgcn_global_load_lds(GPTR(s), LPTR(dst + it * 1024), 16, 0, 0);
  }
}
// every LDS-DMA of this wave has landed (explicit, as in the other LDS-DMA kernels: the barrier that follows must not depend on
// the compiler's own bookkeeping of the DMA)
__device__ __forceinline__ void stage_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
template <int NCH>
__device__ __forceinline__ int row_addr(int slot, int chunk) { return slot * (NCH * 16) + (((chunk + slot) & (NCH - 1)) << 4); }

// bit t of the result: tap t = 3 r + s of pixel m reads inside the image
__device__ __forceinline__ unsigned int tap_mask(const ThinConvParams& p, int m) {
  const unsigned int n = fdiv((unsigned)m, p.divHW);
  const unsigned int rem = (unsigned)m - n * (unsigned)(p.H * p.W);
  const int h = (int)fdiv(rem, p.divW);
  const int w = (int)rem - h * p.W;
  unsigned int vm = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t)
    if ((unsigned)(h + t / 3 - 1) < (unsigned)p.H && (unsigned)(w + t % 3 - 1) < (unsigned)p.W) vm |= 1u << t;
  return vm;
}

// MODE 0: forward, in = x [M][32], out = y [M][16 NCB] (+ bias, ReLU, statistics).  MODE 1: data gradient, in = dy [M][32 KS],
// out = dx [M][32] (NCB = 2), taps mirrored and the filter fragment transposed.  FPW: pixel fragments per wave, SB = 64 FPW.
// (two waves per SIMD: 256 registers per lane, so that a second workgroup of the CU computes while this one stages)
template <int KS, int NCB, int MODE, int FPW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void thin3x3_tile_kernel(const ThinConvParams p) {
  constexpr int NCH = 4 * KS;                    // 16 B chunks of an input row
  constexpr int NCHO = 2 * NCB;                  // of an output row
  constexpr int SB = 64 * FPW;
  constexpr int RP = 256 / NCHO;                 // output rows per store pass
  constexpr int CO = 16 * NCB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int W = p.W, M = p.M;
  const int ZS = p.nalloc - 1;

  // the whole filter as A fragments (row = output channel of the launch = lane & 15, k = 8 * (lane >> 4) + j)
  bf16x8 wf[NCB][9][KS];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (MODE == 0) {
          wf[cb][t][ks] = *(const bf16x8*)(p.w + ((long long)(cb * 16 + fr) * 9 + t) * 32 + fq * 8);
        } else {
          bf16x8 v;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (short)p.w[((long long)(ks * 32 + fq * 8 + j) * 9 + (8 - t)) * 32 + cb * 16 + fr];
          wf[cb][t][ks] = v;
        }
      }
  f32x4 b4[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    b4[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (MODE == 0 && p.bias != nullptr) b4[cb] = *(const f32x4*)(p.bias + cb * 16 + 4 * fq);
  }
  const int cp = tid % NCHO, rg = tid / NCHO;

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int m0 = tile * SB;
    const int mend = m0 + SB < M ? m0 + SB : M;
    const int base = m0 - W - 1;
    __syncthreads();                             // the previous tile's LDS reads are over
    stage_rows<NCH>(smem, p.in, base, SB + 2 * W + 2, p.nalloc, M, wave, lane);
    stage_wait();
    __syncthreads();

    f32x4 acc[FPW][NCB];
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[i][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int ml = (wave + 4 * i) * 16 + fr;
      const int m = m0 + ml;
      const unsigned int vm = m < mend ? tap_mask(p, m) : 0u;
      const int cslot = ml + W + 1;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int sl = ((vm >> t) & 1u) ? cslot + (t / 3 - 1) * W + (t % 3 - 1) : ZS;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 xf = *(const bf16x8*)(smem + row_addr<NCH>(sl, ks * 4 + fq));
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
            acc[i][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb][t][ks], xf, acc[i][cb], 0, 0, 0);
        }
      }
    }
    __syncthreads();                             // all fragment reads done: LDS becomes the output tile [SB][CO] bf16
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
      const int ml = (wave + 4 * i) * 16 + fr;
      const int sw = NCHO == 8 ? ml : (ml >> 1);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        f32x4 v = acc[i][cb] + b4[cb];
        if (MODE == 0 && p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
        }
        u32x2 pk;
        pk[0] = pack_bf16x2(v[0], v[1]);
        pk[1] = pack_bf16x2(v[2], v[3]);
        const int chunk = cb * 2 + (fq >> 1);
        *(u32x2*)(smem + ml * (NCHO * 16) + (((chunk ^ sw) & (NCHO - 1)) << 4) + ((fq & 1) << 3)) = pk;
      }
    }
    __syncthreads();
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
#pragma unroll
    for (int ps = 0; ps < SB / RP; ++ps) {
      const int ml = ps * RP + rg;
      const int m = m0 + ml;
      const int sw = NCHO == 8 ? ml : (ml >> 1);
      const u32x4 o = *(const u32x4*)(smem + ml * (NCHO * 16) + (((cp ^ sw) & (NCHO - 1)) << 4));
      if (m < mend) {
        *(u32x4*)(p.out + (long long)m * CO + cp * 8) = o;
        if (MODE == 0 && p.stats != nullptr) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = bf16_lo(o[e]), hh = bf16_hi(o[e]);
            s1[2 * e] += lo; s2[2 * e] += lo * lo;
            s1[2 * e + 1] += hh; s2[2 * e + 1] += hh * hh;
          }
        }
      }
    }
    if (MODE == 0 && p.stats != nullptr) {
      // one partial row per tile; summation order fixed: rows of a lane in order, then the RP row groups in order
      __syncthreads();
      float* red = (float*)smem;                 // [RP][2][CO] = 16 KB
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[(rg * 2 + 0) * CO + cp * 8 + e] = s1[e];
        red[(rg * 2 + 1) * CO + cp * 8 + e] = s2[e];
      }
      __syncthreads();
      if (tid < 2 * CO) {
        const int which = tid / CO, c = tid - which * CO;
        float s = 0.f;
#pragma unroll 8
        for (int g = 0; g < RP; ++g) s += red[(g * 2 + which) * CO + c];
        p.stats[((long long)tile * 2 + which) * CO + c] = s;
      }
    }
  }
}

// weight gradient; NCB = Cout / 16 (2 or 4); KT: 32-pixel k-steps per tile (SB = 32 KT)
template <int NCB, int KT>
__global__ __launch_bounds__(256) void thin3x3_wgrad_kernel(const ThinConvParams p) {
  constexpr int NJ = NCB == 4 ? 2 : 1;           // input-channel blocks of a wave
  constexpr int NCHY = 2 * NCB;
  constexpr int SB = 32 * KT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;   // transposed-read roles: rows 8g + q (+ 4), 8 B at 8 * pq of a block
  const int cob = NCB == 4 ? wave : (wave & 1);
  const int cib0 = NCB == 4 ? 0 : (wave >> 1);
  const int W = p.W, M = p.M;
  const int ZS = p.nalloc - 1;
  unsigned char* const sX = smem;
  unsigned char* const sY = smem + p.nalloc * 64;
  const int ychunk = 2 * cob + (pq >> 1), sub = 8 * (pq & 1);
  int xchunk[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) xchunk[j] = 2 * (cib0 + j) + (pq >> 1);

  f32x4 acc[9][NJ];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int split = blockIdx.x;
  const int tile_end = (split + 1) * p.tiles_per_split < p.ntiles ? (split + 1) * p.tiles_per_split : p.ntiles;
  for (int tile = split * p.tiles_per_split; tile < tile_end; ++tile) {
    const int m0 = tile * SB;
    const int mend = m0 + SB < M ? m0 + SB : M;
    const int base = m0 - W - 1;
    stage_rows<4>(sX, p.in, base, SB + 2 * W + 2, p.nalloc, M, wave, lane);
    stage_rows<NCHY>(sY, p.dy, m0, mend - m0, SB, M, wave, lane);
    stage_wait();
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      int rrow[2];
      unsigned int vm[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        rrow[e] = ks * 32 + 8 * g + q + 4 * e;
        const int m = m0 + rrow[e];
        vm[e] = m < mend ? tap_mask(p, m) : 0u;
      }
      const bf16x8 yf = tr_pair(sY + row_addr<NCHY>(rrow[0], ychunk) + sub, sY + row_addr<NCHY>(rrow[1], ychunk) + sub);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = (t / 3 - 1) * W + (t % 3 - 1) + W + 1;
        const int sl0 = ((vm[0] >> t) & 1u) ? rrow[0] + d : ZS;
        const int sl1 = ((vm[1] >> t) & 1u) ? rrow[1] + d : ZS;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const bf16x8 xf = tr_pair(sX + row_addr<4>(sl0, xchunk[j]) + sub, sX + row_addr<4>(sl1, xchunk[j]) + sub);
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, yf, acc[t][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // D[ci][co]: lane holds co = fr of its block, ci = 4 * fq + reg of the input block
  float* slab = p.slab + (long long)split * (16 * NCB) * 9 * 32;
  const long long rowo = (long long)(cob * 16 + fr) * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j) *(f32x4*)(slab + (rowo + t) * 32 + (cib0 + j) * 16 + 4 * fq) = acc[t][j];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
constexpr size_t LDS_MAX = 65536;
inline int round16(int v) { return (v + 15) & ~15; }

struct Plan { int sb, nalloc; size_t lds; };
// forward / data gradient: the largest tile whose staged rows (in_row_bytes each) fit
bool plan_tile(int W, int in_row_bytes, int out_row_bytes, Plan* out) {
  for (int sb : {256, 128, 64}) {
    // 64 output channels: a 256-pixel tile would hold 64 accumulator registers per lane beside the 144 of the filter
    if (sb == 256 && in_row_bytes + out_row_bytes > 128) continue;
    const int na = round16(sb + 2 * W + 3);
    size_t lds = (size_t)na * in_row_bytes;
    if (lds < (size_t)sb * out_row_bytes) lds = (size_t)sb * out_row_bytes;
    if (lds < 16384) lds = 16384;
    if (lds <= LDS_MAX) { *out = {sb, na, lds}; return true; }
  }
  return false;
}
bool plan_wgrad(int W, int Cout, Plan* out) {
  for (int sb : {128, 64, 32}) {
    const int na = round16(sb + 2 * W + 3);
    const size_t lds = (size_t)na * 64 + (size_t)sb * Cout * 2;
    if (lds <= LDS_MAX) { *out = {sb, na, lds}; return true; }
  }
  return false;
}
void wgrad_split(int M, int sb, int* S, int* tps, int* ntiles) {
  const int nt = (M + sb - 1) / sb;
  int want = 256;                                // about one workgroup per CU; a constant: the summation order does not depend on the device
  if (want > nt) want = nt;
  if (want < 1) want = 1;
  *tps = (nt + want - 1) / want;
  *S = (nt + *tps - 1) / *tps;
  *ntiles = nt;
}

void fill_common(ThinConvParams& p) {
  p.M = p.N * p.H * p.W;
  p.divHW = make_fastdiv((unsigned)(p.H * p.W));
  p.divW = make_fastdiv((unsigned)p.W);
}

template <int KS, int NCB, int MODE>
int launch_tile(const ThinConvParams& p, const Plan& t, hipStream_t s) {
  int grid = 2 * icamd_num_cus();
  if (grid > p.ntiles) grid = p.ntiles;
  if (t.sb == 256) {
    if constexpr (KS * 2 + NCB <= 4) hipLaunchKernelGGL((thin3x3_tile_kernel<KS, NCB, MODE, 4>), dim3(grid), dim3(256), t.lds, s, p);
    else return ICAMD_ERR_UNSUPPORTED;           // (plan_tile never picks it)
  } else if (t.sb == 128) hipLaunchKernelGGL((thin3x3_tile_kernel<KS, NCB, MODE, 2>), dim3(grid), dim3(256), t.lds, s, p);
  else hipLaunchKernelGGL((thin3x3_tile_kernel<KS, NCB, MODE, 1>), dim3(grid), dim3(256), t.lds, s, p);
  return icamd_launch_status();
}

}  // namespace

// ---- 2x2 average pool --------------------------------------------------------------------------------------------------------------
bool icamd_avgpool2x2_ok(int N, int IH, int IW, int C) {
  if (N <= 0 || IH <= 0 || IW <= 0 || C <= 0 || C % 8 != 0) return false;
  return (long long)N * IH * IW * (C / 8) < (1ll << 31);
}

int icamd_avgpool2x2_launch(Pool2x2Params& p, int backward, hipStream_t stream) {
  if (!icamd_avgpool2x2_ok(p.N, p.IH, p.IW, p.C8 * 8)) return ICAMD_ERR_BAD_ARG;
  p.OH = (p.IH + 1) / 2;
  p.OW = (p.IW + 1) / 2;
  p.total = (unsigned int)((long long)p.N * p.OH * p.OW * p.C8);
  p.divC8 = make_fastdiv((unsigned)p.C8);
  p.divOW = make_fastdiv((unsigned)p.OW);
  p.divOH = make_fastdiv((unsigned)p.OH);
  const unsigned grid = (p.total + 255u) / 256u;
  if (backward) hipLaunchKernelGGL(avgpool2x2_bwd_kernel, dim3(grid), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(avgpool2x2_fwd_kernel, dim3(grid), dim3(256), 0, stream, p);
  return icamd_launch_status();
}

// ---- thin 3x3 convolution ----------------------------------------------------------------------------------------------------------
bool icamd_thin3x3_ok(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin != 32 || (Cout != 32 && Cout != 64)) return false;
  if ((long long)N * H * W >= (1ll << 30)) return false;
  Plan t;
  return plan_tile(W, 64, Cout * 2, &t) && plan_tile(W, Cout * 2, 64, &t) && plan_wgrad(W, Cout, &t);
}

int icamd_thin3x3_stats_rows(int N, int H, int W, int Cout) {
  Plan t;
  if (!icamd_thin3x3_ok(N, H, W, 32, Cout)) return 0;
  plan_tile(W, 64, Cout * 2, &t);
  return (N * H * W + t.sb - 1) / t.sb;
}

int icamd_thin3x3_fwd_launch(ThinConvParams& p, hipStream_t stream) {
  if (!icamd_thin3x3_ok(p.N, p.H, p.W, 32, p.Cout)) return ICAMD_ERR_UNSUPPORTED;
  fill_common(p);
  Plan t;
  plan_tile(p.W, 64, p.Cout * 2, &t);
  p.nalloc = t.nalloc;
  p.ntiles = (p.M + t.sb - 1) / t.sb;
  return p.Cout == 64 ? launch_tile<1, 4, 0>(p, t, stream) : launch_tile<1, 2, 0>(p, t, stream);
}

int icamd_thin3x3_dgrad_launch(ThinConvParams& p, hipStream_t stream) {
  if (!icamd_thin3x3_ok(p.N, p.H, p.W, 32, p.Cout)) return ICAMD_ERR_UNSUPPORTED;
  fill_common(p);
  Plan t;
  plan_tile(p.W, p.Cout * 2, 64, &t);
  p.nalloc = t.nalloc;
  p.ntiles = (p.M + t.sb - 1) / t.sb;
  p.bias = nullptr; p.stats = nullptr; p.relu = 0;
  return p.Cout == 64 ? launch_tile<2, 2, 1>(p, t, stream) : launch_tile<1, 2, 1>(p, t, stream);
}

size_t icamd_thin3x3_wgrad_bytes(int N, int H, int W, int Cout) {
  if (!icamd_thin3x3_ok(N, H, W, 32, Cout)) return 0;
  Plan t;
  plan_wgrad(W, Cout, &t);
  int S, tps, nt;
  wgrad_split(N * H * W, t.sb, &S, &tps, &nt);
  return (size_t)S * Cout * 9 * 32 * sizeof(float);
}

int icamd_thin3x3_wgrad_launch(ThinConvParams& p, hipStream_t stream) {
  if (!icamd_thin3x3_ok(p.N, p.H, p.W, 32, p.Cout)) return ICAMD_ERR_UNSUPPORTED;
  fill_common(p);
  Plan t;
  plan_wgrad(p.W, p.Cout, &t);
  p.nalloc = t.nalloc;
  wgrad_split(p.M, t.sb, &p.S, &p.tiles_per_split, &p.ntiles);
  const dim3 grid((unsigned)p.S), block(256);
  if (p.Cout == 64) {
    if (t.sb == 128) hipLaunchKernelGGL((thin3x3_wgrad_kernel<4, 4>), grid, block, t.lds, stream, p);
    else if (t.sb == 64) hipLaunchKernelGGL((thin3x3_wgrad_kernel<4, 2>), grid, block, t.lds, stream, p);
    else hipLaunchKernelGGL((thin3x3_wgrad_kernel<4, 1>), grid, block, t.lds, stream, p);
  } else {
    if (t.sb == 128) hipLaunchKernelGGL((thin3x3_wgrad_kernel<2, 4>), grid, block, t.lds, stream, p);
    else if (t.sb == 64) hipLaunchKernelGGL((thin3x3_wgrad_kernel<2, 2>), grid, block, t.lds, stream, p);
    else hipLaunchKernelGGL((thin3x3_wgrad_kernel<2, 1>), grid, block, t.lds, stream, p);
  }
  return icamd_launch_status();
}
