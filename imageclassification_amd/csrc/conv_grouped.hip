// Grouped 3x3 / pad 1 / stride 1 or 2 convolution for gfx950, Cin == Cout == C, Cg = C / groups in {4, 8, 16, 32}: forward,
// data gradient and weight gradient of ResNeXt's conv2 (timm Bottleneck.conv2 with cardinality 32 under model(samples) and
// loss.backward()).  A GENUINELY grouped computation: no dense [C][9][C] filter and no dense dW exists anywhere.
//
// Channel blocks.  A group never straddles an aligned 16-channel block (Cg <= 16) or an aligned 32-channel block (Cg = 32), so
// the channels are cut into 64-channel slices that are independent problems: workgroup = (pixel tile, 64-channel slice), wave
// w of the four = the slice's 16 output channels 16w .. 16w+15.  The slice of a pixel is one whole 128 B segment of its NHWC row.
//   Cg = 16: v_mfma_f32_16x16x32_bf16 with K = 2 taps x 16 input channels, five k-steps for the nine taps (the tenth is zero);
//   Cg = 8 / 4: the same five k-steps with a BLOCK-DIAGONAL filter fragment (2 / 4 groups inside the 16 x 16 block);
//   Cg = 32: K = the group's 32 input channels of one tap, nine k-steps; waves 2g and 2g+1 share the input fragment addresses.
// Executed / algorithmic MFMA work (2 M C 9 Cg), padding of 9 taps to 10 included:
//   forward, data gradient (stride 1), weight gradient:  Cg 4: 4.44x (weight gradient 4x)   Cg 8: 2.22x (2x)   Cg 16: 1.11x (1x)
//   Cg 32: 1x;  data gradient at stride 2: five k-steps per 4.5 algorithmic ones, the same 1.11x (Cg <= 16) and 1x (Cg 32).
//
// One read per activation.  The input of a tile (x, or dy for the data gradient) is staged ONCE by LDS-DMA as rows of 128 B:
// slot j of the tile holds the slice of input pixel base + j in (n, h, w) raster order, 16 B per lane, the 16 B chunks of a
// row rotated by the slot number (conflict-free ds_read_b128 of a 16-slot fragment at any alignment, as conv3x3_halo.hip).
// The output pixels of a tile are consecutive in raster order, so are their centre pixels' slots -- at stride 2 with gaps --
// and a tap is an offset dh * IW + dw on the slot; taps that leave the image read the tile's zero slot (staged from the zero
// page), never a neighbour row.  The overlap of neighbouring tiles' halos comes from L2.  The filter fragments of a wave (5 or
// 9 x 16 B per lane) are read once per workgroup into registers, re-indexed on the way: the data gradient takes the FORWARD
// filter layout [C][3][3][Cg] and gathers its transposed, tap-mirrored fragment itself, so a grouped convolution needs no slot
// in the transposed shadow.
//
// Data gradient at stride 2 in one launch: the 2x2 parity classes of dx pixels take 1, 2, 2 and 4 taps; a fragment is 16 dx
// pixels of ONE class (pixel (2 qh + a, 2 qw + b) for 16 consecutive "quads" q, and the quad grid IS the dy grid), so no MFMA
// multiplies by a tap that the parity rules out: five k-steps per quad fragment.
//
// Weight gradient: workgroup = (pixel split, slice); the reduction index is the pixel, so both operands are read with
// ds_read_b64_tr_b16 from the same row images; D[ci][co] per tap stays in registers over the whole split and leaves as one
// fp32 slab [S][C][9][Cg] (diagonal blocks only), folded in fixed order by slab_reduce_kernel: bitwise reproducible.
//
// Not done here: the workgroups are not persistent and a tile's staging is not overlapped with the previous tile's MFMAs inside a
// workgroup; several workgroups per CU (16-64 KB of LDS each) cover for each other instead.  tools/bench_gconv.py times every
// entry against the dense emulation on a block-diagonal filter.
#include "common.h"
#include "icamd_internal.h"
#include <map>
#include <mutex>
#include <tuple>

namespace {

__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* p0, const unsigned char* p1) {
  bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)p0);
  bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)p1);
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// raster index of the input pixel under the centre tap of output pixel m, and m's (oh, ow)
__device__ __forceinline__ int g_center(const GConvParams& p, int m, int& oh, int& ow) {
  const unsigned int n = fdiv((unsigned)m, p.divOHW);
  const unsigned int rem = (unsigned)m - n * (unsigned)(p.OH * p.OW);
  oh = (int)fdiv(rem, p.divOW);
  ow = (int)rem - oh * p.OW;
  return ((int)n * p.IH + oh * p.stride) * p.IW + ow * p.stride;
}

// LDS rows of 128 B: slot j (0 <= j < nalloc, nalloc % 8 == 0) <- channels [cs, cs + 64) of pixel base + j of src; zeros where
// j >= nsl, the pixel is outside [0, npix) or the channels are beyond C.  Logical 16 B chunk c of slot j sits at position (c + j) & 7.
__device__ __forceinline__ void stage_rows(unsigned char* dst, const bf16_t* __restrict__ src, int base, int nsl, int nalloc,
                                           int npix, int C, int cs, int wave, int lane) {
  const bf16_t* zero = (const bf16_t*)icamd_zero_page;
  const int nin = nalloc >> 3;
  for (int it = wave; it < nin; it += 4) {
    const int slot = it * 8 + (lane >> 3);
    const int pix = base + slot;
    const int lc = cs + (((lane & 7) - slot) & 7) * 8;
    const bf16_t* s = (slot < nsl && pix >= 0 && pix < npix && lc < C) ? src + ((long long)pix * C + lc) : zero;
    __builtin_amdgcn_global_load_lds(GPTR(s), LPTR(dst + it * 1024), 16, 0, 0);
  }
}
__device__ __forceinline__ int row_addr(int slot, int chunk) { return slot * 128 + (((chunk + slot) & 7) << 4); }

// ---- filter fragments (A operand: row = lane & 15, k = 8 * (lane >> 4) + j) from the forward layout [C][9][Cg] -------------------
// Cg <= 16: k = tap slot (fq >> 1) x 16 channels of the block; Cg = 32: k = the group's 32 channels.  wtap outside 0..8: zeros.
// forward: row = output channel c0 + fr, k = input channel
template <int CG>
__device__ __forceinline__ bf16x8 gfrag_fwd(const bf16_t* __restrict__ w, int c0, int C, int wtap, int fr, int fq) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c0 >= C || wtap < 0 || wtap > 8) return z;
  const long long row = (long long)(c0 + fr) * 9 + wtap;
  if constexpr (CG == 32) {
    return *(const bf16x8*)(w + row * 32 + fq * 8);
  } else if constexpr (CG == 16) {
    return *(const bf16x8*)(w + row * 16 + (fq & 1) * 8);
  } else if constexpr (CG == 8) {
    if ((fq & 1) != (fr >> 3)) return z;
    return *(const bf16x8*)(w + row * 8);
  } else {
    if ((fq & 1) != (fr >> 3)) return z;
    const bf16x4 v = *(const bf16x4*)(w + row * 4);
    if ((fr >> 2) & 1) return bf16x8{0, 0, 0, 0, v[0], v[1], v[2], v[3]};
    return bf16x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
  }
}
// data gradient: row = input channel cs + 16 * wave + fr, k = output channel (the transposed fragment, gathered element-wise)
template <int CG>
__device__ __forceinline__ bf16x8 gfrag_dgrad(const bf16_t* __restrict__ w, int cs, int wave, int C, int wtap, int fr, int fq) {
  bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  const int c0 = cs + wave * 16;
  if (c0 >= C || wtap < 0 || wtap > 8) return v;
  if constexpr (CG == 32) {
    const int cob = cs + 32 * (wave >> 1) + 8 * fq;
    const int cig = 16 * (wave & 1) + fr;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (short)w[((long long)(cob + j) * 9 + wtap) * 32 + cig];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = (fq & 1) * 8 + j;
      if (col / CG == fr / CG) v[j] = (short)w[((long long)(c0 + col) * 9 + wtap) * CG + (fr % CG)];
    }
  }
  return v;
}

// B-operand chunk (16 B = 8 channels) of the slice row this lane reads: Cg <= 16: the wave's block, half fq & 1; Cg = 32: the group's
template <int CG>
__device__ __forceinline__ int x_chunk(int wave, int fq) {
  return CG == 32 ? 4 * (wave >> 1) + fq : 2 * wave + (fq & 1);
}

// ---- epilogue pieces shared by the forward / data-gradient kernels ----------------------------------------------------------------
// accumulator fragment (lane: pixel row ml, channels 16 * wave + 4 * fq .. + 3) -> bf16 -> [rows][64] LDS tile (128 B rows)
__device__ __forceinline__ void put_tile(unsigned char* tile, int ml, int wave, int fq, f32x4 v) {
  u32x2 pk;
  pk[0] = pack_bf16x2(v[0], v[1]);
  pk[1] = pack_bf16x2(v[2], v[3]);
  const int slot = wave * 4 + fq;            // 8 B slot of the 128 B row; 16 B chunk = slot >> 1
  *(u32x2*)(tile + ml * 128 + ((((slot >> 1) ^ ml) & 7) << 4) + ((slot & 1) << 3)) = pk;
}
__device__ __forceinline__ u32x4 get_tile(const unsigned char* tile, int ml, int cp) {
  return *(const u32x4*)(tile + ml * 128 + (((cp ^ ml) & 7) << 4));
}

// MODE 0: forward (optional bias / ReLU / BatchNorm statistics); MODE 1: data gradient at stride 1 (taps mirrored, fragment transposed).
// A workgroup owns 128 consecutive output pixels (one statistics row) as 128 / (16 * MFR) sub-tiles staged one after the other.
template <int CG, int MODE, int MFR>
__global__ __launch_bounds__(256) void gconv3x3_tile_kernel(const GConvParams p) {
  constexpr int NK = CG == 32 ? 9 : 5;
  constexpr int SB = MFR * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, hi = fq >> 1;
  const int nslices = (p.C + 63) >> 6;
  const int tile = blockIdx.x / nslices, slice = blockIdx.x - tile * nslices;
  const int cs = slice * 64, c0 = cs + wave * 16;
  const int C = p.C, IW = p.IW, IH = p.IH, M = p.M;
  const int ZS = p.nalloc - 1;
  const int chunk = x_chunk<CG>(wave, fq);

  bf16x8 wf[NK];
  int doff[NK], tsel[NK];
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    const int t = CG == 32 ? s : 2 * s + hi;     // the tap this lane multiplies in k-step s (9: none)
    tsel[s] = t;
    const int tr = t / 3;
    doff[s] = (tr - 1) * IW + (t - 3 * tr - 1);
    const int wtap = MODE == 0 ? t : 8 - t;
    if constexpr (MODE == 0) wf[s] = gfrag_fwd<CG>(p.w, c0, C, wtap, fr, fq);
    else wf[s] = gfrag_dgrad<CG>(p.w, cs, wave, C, wtap, fr, fq);
  }
  f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && c0 < C) b4 = *(const f32x4*)(p.bias + c0 + 4 * fq);

  const int cp = tid & 7, rg = tid >> 3;
  const int co = cs + cp * 8;
  float s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }

  for (int sb = 0; sb < 128 / SB; ++sb) {
    const int m0 = tile * 128 + sb * SB;
    if (m0 >= M) break;
    const int mend = m0 + SB < M ? m0 + SB : M;
    int t0, t1;
    const int base = g_center(p, m0, t0, t1) - IW - 1;
    const int nsl = g_center(p, mend - 1, t0, t1) + IW + 2 - base;
    if (sb > 0) __syncthreads();                 // the previous sub-tile's output rows have been read
    stage_rows(smem, p.in, base, nsl, p.nalloc, p.npix_in, C, cs, wave, lane);
    __syncthreads();

    f32x4 acc[MFR];
#pragma unroll
    for (int i = 0; i < MFR; ++i) {
      acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int m = m0 + i * 16 + fr;
      int cslot = 0;
      unsigned int vm = 0;
      if (m < mend) {
        int oh, ow;
        cslot = g_center(p, m, oh, ow) - base;
        const int ih0 = oh * p.stride - 1, iw0 = ow * p.stride - 1;
#pragma unroll
        for (int t = 0; t < 9; ++t)
          if ((unsigned)(ih0 + t / 3) < (unsigned)IH && (unsigned)(iw0 + t % 3) < (unsigned)IW) vm |= 1u << t;
      }
#pragma unroll
      for (int s = 0; s < NK; ++s) {
        const int sl = ((vm >> tsel[s]) & 1u) ? cslot + doff[s] : ZS;
        const bf16x8 xf = *(const bf16x8*)(smem + row_addr(sl, chunk));
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], xf, acc[i], 0, 0, 0);
      }
    }
    __syncthreads();                             // all fragment reads done: LDS becomes the output tile
#pragma unroll
    for (int i = 0; i < MFR; ++i) {
      f32x4 v = acc[i] + b4;
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
      }
      put_tile(smem, i * 16 + fr, wave, fq, v);
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < SB / 32; ++ps) {
      const int ml = ps * 32 + rg;
      const int m = m0 + ml;
      const u32x4 o = get_tile(smem, ml, cp);
      if (m < mend && co < C) {
        *(u32x4*)(p.out + (long long)m * C + co) = o;
        if (p.stats != nullptr) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = bf16_lo(o[e]), hh = bf16_hi(o[e]);
            s1[2 * e] += lo; s2[2 * e] += lo * lo;
            s1[2 * e + 1] += hh; s2[2 * e + 1] += hh * hh;
          }
        }
      }
    }
  }
  if (p.stats != nullptr) {
    // one partial row per 128-pixel tile = per workgroup: exactly the ceil(M / 128) rows the consumer sums
    __syncthreads();
    float* red = (float*)smem;                   // [32][2][64]
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(rg * 2 + 0) * 64 + cp * 8 + e] = s1[e];
      red[(rg * 2 + 1) * 64 + cp * 8 + e] = s2[e];
    }
    __syncthreads();
    if (tid < 128) {
      const int which = tid >> 6, c = tid & 63;
      float s = 0.f;
#pragma unroll 8
      for (int g = 0; g < 32; ++g) s += red[(g * 2 + which) * 64 + c];
      if (cs + c < C) p.stats[((long long)tile * 2 + which) * C + cs + c] = s;
    }
  }
}

// ---- data gradient at stride 2: tile = 64 quads (dy pixels) x 4 parity classes = up to 256 dx pixels ------------------------------
// k-step order of the weight taps (r * 3 + s): class (a, b) = (r != 1, s != 1) of the dx pixel (2 qh + a, 2 qw + b) the tap feeds;
// tap (r, s) reads dy pixel (qh + (r == 0), qw + (s == 0)).
__device__ __forceinline__ constexpr int s2_tap(int idx) {
  constexpr int T[10] = {4, -1, 3, 5, 1, 7, 0, 2, 6, 8};
  return T[idx];
}
__device__ __forceinline__ constexpr int s2_tap32(int idx) { return idx == 0 ? 4 : s2_tap(idx + 1); }
__device__ __forceinline__ constexpr int s2_class(int tap) { return (tap / 3 != 1 ? 2 : 0) + (tap % 3 != 1 ? 1 : 0); }

template <int CG>
__global__ __launch_bounds__(256) void gconv3x3_dgrad_s2_kernel(const GConvParams p) {
  constexpr int NK = CG == 32 ? 9 : 5;
  constexpr int BQ = 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, hi = fq >> 1;
  const int nslices = (p.C + 63) >> 6;
  const int tile = blockIdx.x / nslices, slice = blockIdx.x - tile * nslices;
  const int cs = slice * 64;
  const int C = p.C, OW = p.OW, OH = p.OH, Mq = p.M;
  const int ZS = p.nalloc - 1;
  const int chunk = x_chunk<CG>(wave, fq);
  unsigned char* const sO = smem + p.nalloc * 128;   // [4][BQ] rows of 128 B
  const int q0 = tile * BQ;

  stage_rows(smem, p.in, q0, BQ + OW + 2, p.nalloc, Mq, C, cs, wave, lane);

  bf16x8 wf[NK];
  int doff[NK];
  unsigned int need[NK];      // bit 0: a tap exists, bit 1: it needs qh + 1 < OH, bit 2: it needs qw + 1 < OW
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    const int t = CG == 32 ? s2_tap32(s) : (hi ? s2_tap(2 * s + 1) : s2_tap(2 * s));
    const int tr = t < 0 ? 1 : t / 3, tc = t < 0 ? 1 : t - 3 * tr;
    doff[s] = (tr == 0 ? OW : 0) + (tc == 0 ? 1 : 0);
    need[s] = (t >= 0 ? 1u : 0u) | (tr == 0 ? 2u : 0u) | (tc == 0 ? 4u : 0u);
    wf[s] = gfrag_dgrad<CG>(p.w, cs, wave, C, t, fr, fq);
  }
  __syncthreads();

  f32x4 acc[4][BQ / 16];
#pragma unroll
  for (int i = 0; i < BQ / 16; ++i) {
    const int ql = i * 16 + fr, q = q0 + ql;
    unsigned int have = 0;    // bit 0: the quad exists, bit 1: qh + 1 < OH, bit 2: qw + 1 < OW
    if (q < Mq) {
      const unsigned int n = fdiv((unsigned)q, p.divOHW);
      const unsigned int rem = (unsigned)q - n * (unsigned)(OH * OW);
      const int qh = (int)fdiv(rem, p.divOW);
      const int qw = (int)rem - qh * OW;
      have = 1u | (qh + 1 < OH ? 2u : 0u) | (qw + 1 < OW ? 4u : 0u);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      const int k = s2_class(CG == 32 ? s2_tap32(s) : s2_tap(2 * s));   // both taps of a k-step feed the same class
      const int sl = ((have & need[s]) == need[s] && (need[s] & 1u)) ? ql + doff[s] : ZS;
      const bf16x8 xf = *(const bf16x8*)(smem + row_addr(sl, chunk));
      acc[k][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], xf, acc[k][i], 0, 0, 0);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int i = 0; i < BQ / 16; ++i) put_tile(sO + k * BQ * 128, i * 16 + fr, wave, fq, acc[k][i]);
  __syncthreads();
  const int cp = tid & 7, rg = tid >> 3;
  const int co = cs + cp * 8;
#pragma unroll
  for (int ps = 0; ps < 4 * BQ / 32; ++ps) {
    const int k = ps / (BQ / 32);
    const int ml = (ps % (BQ / 32)) * 32 + rg;
    const int q = q0 + ml;
    const u32x4 o = get_tile(sO + k * BQ * 128, ml, cp);
    if (q < Mq && co < C) {
      const unsigned int n = fdiv((unsigned)q, p.divOHW);
      const unsigned int rem = (unsigned)q - n * (unsigned)(OH * OW);
      const int qh = (int)fdiv(rem, p.divOW);
      const int qw = (int)rem - qh * OW;
      const int ih = 2 * qh + (k >> 1), iw = 2 * qw + (k & 1);
      if (ih < p.IH && iw < p.IW) *(u32x4*)(p.out + (((long long)n * p.IH + ih) * p.IW + iw) * C + co) = o;
    }
  }
}

// ---- weight gradient: workgroup = (pixel split, 64-channel slice); tile = 32 * KS output pixels -----------------------------------
template <int CG, int KS>
__global__ __launch_bounds__(256) void gconv3x3_wgrad_kernel(const GConvParams p) {
  constexpr int NJ = CG == 32 ? 2 : 1;
  constexpr int SB = 32 * KS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;   // transposed-read roles: rows 8g + q (+ 4), 8 B at 8 * pq of a block
  const int nslices = (p.C + 63) >> 6;
  const int split = blockIdx.x / nslices, slice = blockIdx.x - split * nslices;
  const int cs = slice * 64, c0 = cs + wave * 16;
  const int C = p.C, IW = p.IW, IH = p.IH, M = p.M;
  const int ZS = p.nalloc - 1;
  unsigned char* const sX = smem;
  unsigned char* const sY = smem + p.nalloc * 128;
  const int ychunk = 2 * wave + (pq >> 1), sub = 8 * (pq & 1);
  int xchunk[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) xchunk[j] = CG == 32 ? 2 * (2 * (wave >> 1) + j) + (pq >> 1) : ychunk;

  f32x4 acc[9][NJ];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tile_end = (split + 1) * p.tiles_per_split < p.ntiles ? (split + 1) * p.tiles_per_split : p.ntiles;
  for (int tile = split * p.tiles_per_split; tile < tile_end; ++tile) {
    const int m0 = tile * SB;
    const int mend = m0 + SB < M ? m0 + SB : M;
    int t0, t1;
    const int base = g_center(p, m0, t0, t1) - IW - 1;
    const int nsl = g_center(p, mend - 1, t0, t1) + IW + 2 - base;
    stage_rows(sX, p.in, base, nsl, p.nalloc, p.npix_in, C, cs, wave, lane);
    stage_rows(sY, p.dy, m0, mend - m0, SB, M, C, cs, wave, lane);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      int rrow[2], cslot[2];
      unsigned int vm[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        rrow[e] = ks * 32 + 8 * g + q + 4 * e;
        const int m = m0 + rrow[e];
        cslot[e] = 0;
        vm[e] = 0;
        if (m < mend) {
          int oh, ow;
          cslot[e] = g_center(p, m, oh, ow) - base;
          const int ih0 = oh * p.stride - 1, iw0 = ow * p.stride - 1;
#pragma unroll
          for (int t = 0; t < 9; ++t)
            if ((unsigned)(ih0 + t / 3) < (unsigned)IH && (unsigned)(iw0 + t % 3) < (unsigned)IW) vm[e] |= 1u << t;
        }
      }
      const bf16x8 yf = tr_pair(sY + row_addr(rrow[0], ychunk) + sub, sY + row_addr(rrow[1], ychunk) + sub);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = (t / 3 - 1) * IW + (t % 3 - 1);
        const int sl0 = ((vm[0] >> t) & 1u) ? cslot[0] + d : ZS;
        const int sl1 = ((vm[1] >> t) & 1u) ? cslot[1] + d : ZS;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const bf16x8 xf = tr_pair(sX + row_addr(sl0, xchunk[j]) + sub, sX + row_addr(sl1, xchunk[j]) + sub);
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, yf, acc[t][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // D[ci][co]: lane holds co = fr, ci = 4 * fq + reg of the 16 x 16 block; only the group's own columns leave
  if (c0 >= C) return;
  float* slab = p.slab + (long long)split * C * 9 * CG;
  const long long rowo = (long long)(c0 + fr) * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    if constexpr (CG == 32) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) *(f32x4*)(slab + (rowo + t) * 32 + j * 16 + 4 * fq) = acc[t][j];
    } else if constexpr (CG == 16) {
      *(f32x4*)(slab + (rowo + t) * 16 + 4 * fq) = acc[t][0];
    } else if constexpr (CG == 8) {
      if ((fq >> 1) == (fr >> 3)) *(f32x4*)(slab + (rowo + t) * 8 + 4 * (fq & 1)) = acc[t][0];
    } else {
      if (fq == (fr >> 2)) *(f32x4*)(slab + (rowo + t) * 4) = acc[t][0];
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
constexpr size_t LDS_MAX = 65536;

int center_host(int m, int IH, int IW, int OH, int OW, int stride) {
  const int n = m / (OH * OW), rem = m - n * (OH * OW), oh = rem / OW, ow = rem - oh * OW;
  return (n * IH + oh * stride) * IW + ow * stride;
}
// the most input slots any tile of SB consecutive output pixels needs (first centre - IW - 1 .. last centre + IW + 1)
int max_slots(int N, int IH, int IW, int OH, int OW, int stride, int SB) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, int, int, int, int>, int> cache;
  const auto key = std::make_tuple(N, IH, IW, OH, OW, stride, SB);
  std::lock_guard<std::mutex> lock(mu);
  const auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const int M = N * OH * OW;
  int best = 0;
  for (int m0 = 0; m0 < M; m0 += SB) {
    const int ml = (m0 + SB < M ? m0 + SB : M) - 1;
    const int span = center_host(ml, IH, IW, OH, OW, stride) - center_host(m0, IH, IW, OH, OW, stride) + 2 * IW + 3;
    if (span > best) best = span;
  }
  cache[key] = best;
  return best;
}
inline int round8(int v) { return (v + 7) & ~7; }

struct TilePlan { int sb, nalloc; size_t lds; };
// forward / stride-1 data gradient: the largest sub-tile whose staged rows fit
bool plan_tile(int N, int IH, int IW, int OH, int OW, int stride, TilePlan* out) {
  for (int sb : {128, 64, 32}) {
    const int na = round8(max_slots(N, IH, IW, OH, OW, stride, sb) + 1);
    size_t lds = (size_t)na * 128;
    if (lds < (size_t)sb * 128) lds = (size_t)sb * 128;
    if (lds < 16384) lds = 16384;
    if (lds <= LDS_MAX) { *out = {sb, na, lds}; return true; }
  }
  return false;
}
bool plan_wgrad(int N, int IH, int IW, int OH, int OW, int stride, TilePlan* out) {
  for (int sb : {64, 32}) {
    const int na = round8(max_slots(N, IH, IW, OH, OW, stride, sb) + 1);
    const size_t lds = (size_t)na * 128 + (size_t)sb * 128;
    if (lds <= LDS_MAX) { *out = {sb, na, lds}; return true; }
  }
  return false;
}
bool plan_dgrad_s2(int OW, TilePlan* out) {
  const int na = round8(64 + OW + 2 + 1);
  const size_t lds = (size_t)na * 128 + 4 * 64 * 128;
  if (lds > LDS_MAX) return false;
  *out = {64, na, lds};
  return true;
}
void wgrad_split(int M, int C, int sb, int* S, int* tps, int* ntiles) {
  const int nt = (M + sb - 1) / sb, nslices = (C + 63) / 64;
  int want = (512 + nslices - 1) / nslices;          // about two workgroups per CU
  if (want > nt) want = nt;
  if (want < 1) want = 1;
  *tps = (nt + want - 1) / want;
  *S = (nt + *tps - 1) / *tps;
  *ntiles = nt;
}

template <int CG, int MODE>
int launch_tile(const GConvParams& p, int sb, size_t lds, unsigned grid, hipStream_t s) {
  if (sb == 128) hipLaunchKernelGGL((gconv3x3_tile_kernel<CG, MODE, 8>), dim3(grid), dim3(256), lds, s, p);
  else if (sb == 64) hipLaunchKernelGGL((gconv3x3_tile_kernel<CG, MODE, 4>), dim3(grid), dim3(256), lds, s, p);
  else hipLaunchKernelGGL((gconv3x3_tile_kernel<CG, MODE, 2>), dim3(grid), dim3(256), lds, s, p);
  return icamd_launch_status();
}
template <int MODE>
int launch_tile_cg(const GConvParams& p, int sb, size_t lds, unsigned grid, hipStream_t s) {
  switch (p.Cg) {
    case 4: return launch_tile<4, MODE>(p, sb, lds, grid, s);
    case 8: return launch_tile<8, MODE>(p, sb, lds, grid, s);
    case 16: return launch_tile<16, MODE>(p, sb, lds, grid, s);
    case 32: return launch_tile<32, MODE>(p, sb, lds, grid, s);
  }
  return ICAMD_ERR_UNSUPPORTED;
}
template <int CG>
int launch_wgrad(const GConvParams& p, int sb, size_t lds, unsigned grid, hipStream_t s) {
  if (sb == 64) hipLaunchKernelGGL((gconv3x3_wgrad_kernel<CG, 2>), dim3(grid), dim3(256), lds, s, p);
  else hipLaunchKernelGGL((gconv3x3_wgrad_kernel<CG, 1>), dim3(grid), dim3(256), lds, s, p);
  return icamd_launch_status();
}

void fill_common(GConvParams& p) {
  p.Cg = p.C / p.groups;
  p.divOHW = make_fastdiv((unsigned)(p.OH * p.OW));
  p.divOW = make_fastdiv((unsigned)p.OW);
}

}  // namespace

bool icamd_gconv3x3_ok(int N, int IH, int IW, int OH, int OW, int C, int groups, int stride) {
  if (N <= 0 || IH <= 0 || IW <= 0 || C <= 0 || groups <= 0) return false;
  if (stride != 1 && stride != 2) return false;
  if (OH != (IH - 1) / stride + 1 || OW != (IW - 1) / stride + 1) return false;
  if (C % 32 != 0 || C % groups != 0) return false;
  const int cg = C / groups;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return false;
  if ((long long)N * IH * IW >= (1ll << 30)) return false;
  TilePlan t;
  if (!plan_tile(N, IH, IW, OH, OW, stride, &t)) return false;
  if (!plan_wgrad(N, IH, IW, OH, OW, stride, &t)) return false;
  if (stride == 2 && !plan_dgrad_s2(OW, &t)) return false;
  return true;
}

int icamd_gconv3x3_fwd_launch(GConvParams& p, hipStream_t stream) {
  if (!icamd_gconv3x3_ok(p.N, p.IH, p.IW, p.OH, p.OW, p.C, p.groups, p.stride)) return ICAMD_ERR_UNSUPPORTED;
  fill_common(p);
  TilePlan t;
  plan_tile(p.N, p.IH, p.IW, p.OH, p.OW, p.stride, &t);
  p.M = p.N * p.OH * p.OW;
  p.npix_in = p.N * p.IH * p.IW;
  p.nalloc = t.nalloc;
  const unsigned grid = (unsigned)(((p.M + 127) / 128) * ((p.C + 63) / 64));
  return launch_tile_cg<0>(p, t.sb, t.lds, grid, stream);
}

int icamd_gconv3x3_dgrad_launch(GConvParams& p, hipStream_t stream) {
  if (!icamd_gconv3x3_ok(p.N, p.IH, p.IW, p.OH, p.OW, p.C, p.groups, p.stride)) return ICAMD_ERR_UNSUPPORTED;
  fill_common(p);
  TilePlan t;
  if (p.stride == 1) {
    // the forward computation on dy (same grid) with mirrored taps
    plan_tile(p.N, p.IH, p.IW, p.OH, p.OW, 1, &t);
    p.M = p.N * p.IH * p.IW;
    p.npix_in = p.M;
    p.nalloc = t.nalloc;
    p.bias = nullptr; p.stats = nullptr; p.relu = 0;
    const unsigned grid = (unsigned)(((p.M + 127) / 128) * ((p.C + 63) / 64));
    return launch_tile_cg<1>(p, t.sb, t.lds, grid, stream);
  }
  plan_dgrad_s2(p.OW, &t);
  p.M = p.N * p.OH * p.OW;           // quads = dy pixels
  p.npix_in = p.M;
  p.nalloc = t.nalloc;
  const unsigned grid = (unsigned)(((p.M + 63) / 64) * ((p.C + 63) / 64));
  switch (p.Cg) {
    case 4: hipLaunchKernelGGL(gconv3x3_dgrad_s2_kernel<4>, dim3(grid), dim3(256), t.lds, stream, p); break;
    case 8: hipLaunchKernelGGL(gconv3x3_dgrad_s2_kernel<8>, dim3(grid), dim3(256), t.lds, stream, p); break;
    case 16: hipLaunchKernelGGL(gconv3x3_dgrad_s2_kernel<16>, dim3(grid), dim3(256), t.lds, stream, p); break;
    default: hipLaunchKernelGGL(gconv3x3_dgrad_s2_kernel<32>, dim3(grid), dim3(256), t.lds, stream, p); break;
  }
  return icamd_launch_status();
}

size_t icamd_gconv3x3_wgrad_bytes(int N, int IH, int IW, int OH, int OW, int C, int groups, int stride) {
  if (!icamd_gconv3x3_ok(N, IH, IW, OH, OW, C, groups, stride)) return 0;
  TilePlan t;
  plan_wgrad(N, IH, IW, OH, OW, stride, &t);
  int S, tps, nt;
  wgrad_split(N * OH * OW, C, t.sb, &S, &tps, &nt);
  return (size_t)S * C * 9 * (C / groups) * sizeof(float);
}

int icamd_gconv3x3_wgrad_launch(GConvParams& p, hipStream_t stream) {
  if (!icamd_gconv3x3_ok(p.N, p.IH, p.IW, p.OH, p.OW, p.C, p.groups, p.stride)) return ICAMD_ERR_UNSUPPORTED;
  fill_common(p);
  TilePlan t;
  plan_wgrad(p.N, p.IH, p.IW, p.OH, p.OW, p.stride, &t);
  p.M = p.N * p.OH * p.OW;
  p.npix_in = p.N * p.IH * p.IW;
  p.nalloc = t.nalloc;
  wgrad_split(p.M, p.C, t.sb, &p.S, &p.tiles_per_split, &p.ntiles);
  const unsigned grid = (unsigned)(p.S * ((p.C + 63) / 64));
  switch (p.Cg) {
    case 4: return launch_wgrad<4>(p, t.sb, t.lds, grid, stream);
    case 8: return launch_wgrad<8>(p, t.sb, t.lds, grid, stream);
    case 16: return launch_wgrad<16>(p, t.sb, t.lds, grid, stream);
    case 32: return launch_wgrad<32>(p, t.sb, t.lds, grid, stream);
  }
  return ICAMD_ERR_UNSUPPORTED;
}
