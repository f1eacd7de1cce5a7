// Multi-head self-attention for sequences of any length (ViT above 224^2: T = 577 / 785 / 1025, head dim 64) on gfx950: forward
// and backward with the second operand STREAMED through LDS in tiles of 64 rows.  attention.hip keeps a whole (image, head) pair
// resident in LDS and all of a query block's score tiles in registers, which ends at T = 208; here nothing scales with T but
// the trip count of the tile loop.
//
// Layouts and the division of work are those of attention.hip: qkv is [B*T][3*H*64] (q | k | v, each [head][64]), out / dout are
// [B*T][H*64], dqkv mirrors qkv, lse and delta are fp32 [B][H][T].  Three kernels, no atomics, every sum in a fixed order
// (bitwise reproducible):
//   forward         : a workgroup owns 128 queries of one pair (4 waves x 2 blocks of 16) and walks the key tiles: S^T = K Q^T
//                     (query on the lane) -> online softmax (running maximum and sum per query, O rescaled when the maximum
//                     moves) -> O += P V with P straight from the accumulators, rounded to bf16 once; O is normalised and
//                     rounded once at the end; lse = max + log(sum) of the scaled scores;
//   backward (dQ)   : the same ownership; S^T, dP^T = V dO^T -> dS^T -> dQ^T += K^T dS^T; writes delta = rowsum(dO * O);
//   backward (dK,dV): a workgroup owns 128 KEYS and walks the query tiles of Q and dO (and the lse / delta rows of the tile):
//                     S = Q K^T, dP = dO V^T (key on the lane) -> dV^T += dO^T P, dK^T += Q^T dS.  Launched behind the dQ
//                     kernel on the same stream, it reads the delta that one wrote.
// A wave holding two 16-row blocks reads every LDS fragment once for two MFMAs (the 16-row form of attention.hip reads K and V
// once per query block: 256 B / clock / CU asked of a 128 B / clock LDS).
//
// Tile ring: two buffers of [K | V] (or [Q | dO]) images, 64 rows x 128 B each, in the tr_img() layout, so one image serves
// ds_read_b128 (rows) and ds_read_b64_tr_b16 (columns).  Tile j + 1 is requested by LDS-DMA (four 1 KB pieces per wave) at the
// top of iteration j and waited for (vmcnt(0)) in front of the ONE barrier per tile at the top of iteration j + 1; that barrier
// also says that every wave is done reading the buffer about to be refilled.  All LDS reads of the loops are inline asm with a
// hand-placed s_waitcnt lgkmcnt(0) that names their destinations: in front of a C++ LDS read hipcc drains vmcnt(0) while an
// LDS-DMA is in flight (it cannot tell the buffers apart), which would make the ring a single buffer.
//
// Rows past T: tile rows >= T are filled from the zero page.  Forward: only the LAST key tile can hold them, and only there the
// scores are masked to -inf.  Backward: a key past T is a zero row of K and V (its dS meets a zero row of K^T; its own dK / dV are
// never stored), a query past T gets lse = +inf, i.e. p = 0.  The dQ kernel holds p to [0, 1] (clamp01()), so that such a key's
// dS = -e^-lse delta is finite whatever lse is: 0 * inf would be NaN in the whole dQ row.  Nothing is stored for a row >= T.
//
// Grid: one workgroup per (pair, block of 128 rows).  With 8 XCDs dispatched round-robin, workgroup w runs on XCD w % 8; the
// order below gives all blocks of a pair to ONE XCD, consecutively, so the pair's K / V (or Q / dO) tiles are fetched into one L2
// once.  It is a bijection onto (pair, block) for any XCD count; a device that does not report 8 gets the plain order.
//
// Measured (profiles/attention_long.txt; the resident kernels at B 256, T 197 in the same session: 323 / 330 TFLOP/s forward /
// backward): B 64, T 577, 12 heads: forward 140 us = 469 TFLOP/s, backward 335 us = 489 (dQ 166 us, dK / dV 244 us); B 32, T 1025:
// 195 us = 531, 447 us = 577.  The occupancy bounds of the three kernels are part of that: left alone hipcc took 224 / 208 / 320
// VGPRs (two / two / ONE wave per SIMD: the dK / dV kernel ran 378 us at T 577); bounded, 162 / 157 / 224 without spills.  With one
// lgkmcnt(0) per phase nothing overlaps inside a wave, so the other waves of the SIMD are what hides the LDS latency.
#include "common.h"
#include "icamd_internal.h"
#include "attention_common.h"

namespace {

constexpr int KT = 64;               // rows of a streamed tile
constexpr int TILE = KT * ROWB;      // bytes of one tile image
constexpr int LWAVES = 4, LTHREADS = LWAVES * 64;
constexpr int NQ = 2;                // 16-row blocks a wave owns
constexpr int WGROWS = LWAVES * NQ * 16;   // rows a workgroup owns
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)LPTR(p); }

// LDS reads hipcc's wait-count pass does not see (see the header): the result is valid after lds_wait() has named it
template <class V, int OFF>
__device__ __forceinline__ V lds_r128(unsigned addr) {
  V v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ bf16x4 lds_tr64(unsigned addr) {
  bf16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <class V>
__device__ __forceinline__ void lds_wait(V& a, V& b, V& c, V& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) :: "memory");
}
template <class V>
__device__ __forceinline__ void lds_wait(V& a, V& b, V& c, V& d, V& e, V& f, V& g, V& h) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) :: "memory");
}
__device__ __forceinline__ bf16x8 join(const bf16x4& a, const bf16x4& b) {
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// Lane offsets into a tile image.  Row reads: lane (c, g) takes row 16 kb + c, 16 B chunk 4 ks + g (kb as an immediate of 2048 B).
// Transposed reads: tr_pair()'s address for rows 4 g + (c >> 2) (+ 32 pp, + 16: immediates), column block db.
struct TileLanes {
  unsigned row[2];   // [ks]
  unsigned tr[4];    // [db]
};
__device__ __forceinline__ TileLanes tile_lanes(int lane) {
  const int g = lane >> 4, c = lane & 15;
  TileLanes t;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) t.row[ks] = (unsigned)tr_img(c, ks * 4 + g);
  const int r = 4 * g + (c >> 2), pq = c & 3;
#pragma unroll
  for (int db = 0; db < 4; ++db) t.tr[db] = (unsigned)(r * ROWB + ((db ^ ((r >> 1) & 3)) << 5) + 8 * pq);
  return t;
}

// Rows [row0, row0 + 64) of two [.][64] slices into two tile images by LDS-DMA: wave `wave` issues pieces wave and wave + 4 of
// each (a piece = 8 rows x 128 B, one wave-instruction; the chunk permutation of the image is applied on the source side, as in
// attention.hip's stage_two_dma).  Rows >= T read the zero page.  The caller waits vmcnt(0) in front of the hand-over barrier.
__device__ __forceinline__ void stage_tile_dma(const bf16_t* __restrict__ src0, long long ld0, unsigned char* img0,
                                               const bf16_t* __restrict__ src1, long long ld1, unsigned char* img1, int row0, int T,
                                               int wave, int lane) {
  const int lr = lane >> 3, cpos = lane & 7;
  const int ch = ((((cpos >> 1) ^ ((lr >> 1) & 3))) << 1) | (cpos & 1);
  const unsigned char* zero = (const unsigned char*)icamd_zero_page;
#pragma unroll
  for (int j = wave; j < KT / 8; j += LWAVES) {
    const int r = row0 + j * 8 + lr;
    const bool ok = r < T;
    const void* a0 = ok ? (const void*)(src0 + (long long)r * ld0 + ch * 8) : (const void*)zero;
    const void* a1 = ok ? (const void*)(src1 + (long long)r * ld1 + ch * 8) : (const void*)zero;
    __builtin_amdgcn_global_load_lds(GPTR(a0), LPTR(img0 + j * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(GPTR(a1), LPTR(img1 + j * 1024), 16, 0, 0);
  }
}

// workgroup -> (pair, block): see "Grid" in the header.  xcds = 1 is the plain order.
__device__ __forceinline__ bool decode_block(int nheads, int nblk, int xcds, int* pair, int* blk) {
  const int w = blockIdx.x;
  const int x = w % xcds, slot = w / xcds;
  *pair = (slot / nblk) * xcds + x;
  *blk = slot % nblk;
  return *pair < nheads;
}

// ----------------------------------------------------------------------------------------------------------------
// forward
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LTHREADS, 3) void attn_long_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                 float* __restrict__ lse, int T, int H, float scale, int nheads,
                                                                 int nblk, int xcds) {
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2][2][TILE];   // [buffer][K rows | V (read transposed)]
  int pair, blk;
  if (!decode_block(nheads, nblk, xcds, &pair, &blk)) return;
  const long long ld = 3ll * H * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const float c1 = scale * LOG2E;   // exp(scale * x) = 2^(c1 * x)
  const int b = pair / H, h = pair - b * H;
  const bf16_t* base = qkv + (long long)b * T * ld + h * HD;
  const bf16_t* Kg = base + (long long)H * HD;
  const bf16_t* Vg = base + 2ll * H * HD;
  const int ntiles = (T + KT - 1) / KT;
  const int q0 = blk * WGROWS + wave * (NQ * 16);
  const bool active = q0 < T;       // (wave-uniform) a wave wholly past T only stages
  const TileLanes tl = tile_lanes(lane);
  stage_tile_dma(Kg, ld, lds[0][0], Vg, ld, lds[0][1], 0, T, wave, lane);
  bf16x8 qf[NQ][2];
#pragma unroll
  for (int u = 0; u < NQ; ++u) load_rowfrag(base, ld, q0 + u * 16 + c, T, g, qf[u]);
  float m[NQ], l[NQ];
  f32x4 o[NQ][4];
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[u][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 1
  for (int j = 0; j < ntiles; ++j) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile j have landed
    __syncthreads();                                   // ... everybody's have, and buffer (j + 1) & 1 is no longer read
    if (j + 1 < ntiles)
      stage_tile_dma(Kg, ld, lds[(j + 1) & 1][0], Vg, ld, lds[(j + 1) & 1][1], (j + 1) * KT, T, wave, lane);
    if (!active) continue;
    const unsigned Ka = lds_addr(lds[j & 1][0]), Va = lds_addr(lds[j & 1][1]);
    // S^T[key][query] of the 4 key blocks x NQ query blocks: lane (c, g) holds, for query c, keys 16 kb + 4 g + r
    bf16x8 kf[4][2];
    static_for<0, 4>([&](auto kc) {
      constexpr int kb = decltype(kc)::value;
      kf[kb][0] = lds_r128<bf16x8, kb * 2048>(Ka + tl.row[0]);
      kf[kb][1] = lds_r128<bf16x8, kb * 2048>(Ka + tl.row[1]);
    });
    // V^T fragments of the tile are requested now and waited for behind the softmax
    bf16x4 vlo[2][4], vhi[2][4];
    static_for<0, 2>([&](auto pc) {
      constexpr int pp = decltype(pc)::value;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        vlo[pp][db] = lds_tr64<pp * 4096>(Va + tl.tr[db]);
        vhi[pp][db] = lds_tr64<pp * 4096 + 2048>(Va + tl.tr[db]);
      }
    });
    lds_wait(kf[0][0], kf[0][1], kf[1][0], kf[1][1], kf[2][0], kf[2][1], kf[3][0], kf[3][1]);
    f32x4 s[NQ][4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        s[u][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb][0], qf[u][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        s[u][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb][1], qf[u][1], s[u][kb], 0, 0, 0);
      }
    if (j == ntiles - 1) {   // the only tile that can reach past T
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = j * KT + kb * 16 + 4 * g + r < T;
#pragma unroll
          for (int u = 0; u < NQ; ++u) s[u][kb][r] = ok ? s[u][kb][r] : -INFINITY;
        }
    }
    bf16x8 pf[NQ][2];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      float mt = max3_raw(max3_raw(s[u][0][0], s[u][0][1], s[u][0][2]), s[u][0][3], s[u][1][0]);
      mt = max3_raw(max3_raw(mt, s[u][1][1], s[u][1][2]), s[u][1][3], s[u][2][0]);
      mt = max3_raw(max3_raw(mt, s[u][2][1], s[u][2][2]), s[u][2][3], s[u][3][0]);
      mt = max3_raw(max3_raw(mt, s[u][3][1], s[u][3][2]), s[u][3][3], m[u]);
      const float mnew = group_max(mt);                          // finite: every tile holds a key < T
      const float alpha = __builtin_amdgcn_exp2f((m[u] - mnew) * c1);   // first tile: 2^-inf = 0
      const float mc = mnew * c1;
      float lt = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[u][kb][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[u][kb][r], c1, -mc));   // masked keys: 2^-inf = 0
          lt += s[u][kb][r];
        }
      l[u] = __builtin_fmaf(l[u], alpha, lt);
      if (__builtin_amdgcn_ballot_w64(mnew != m[u]) != 0) {      // (wave-uniform) some query's maximum moved: rescale O
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a = __shfl(alpha, 4 * g + r, 64);          // factor of query 4g+r (held by the lanes with c == 4g+r)
#pragma unroll
          for (int db = 0; db < 4; ++db) o[u][db][r] *= a;
        }
      }
      m[u] = mnew;
      pf[u][0] = pack_acc2(s[u][0], s[u][1]);
      pf[u][1] = pack_acc2(s[u][2], s[u][3]);
    }
    static_for<0, 2>([&](auto pc) {
      constexpr int pp = decltype(pc)::value;
      lds_wait(vlo[pp][0], vlo[pp][1], vlo[pp][2], vlo[pp][3], vhi[pp][0], vhi[pp][1], vhi[pp][2], vhi[pp][3]);
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const bf16x8 vf = join(vlo[pp][db], vhi[pp][db]);
#pragma unroll
        for (int u = 0; u < NQ; ++u)
          o[u][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[u][pp], vf, o[u][db], 0, 0, 0);   // D[query 4g+r][d = db*16 + c]
      }
    });
  }
  if (!active) return;
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int qrow = q0 + u * 16 + c;
    const float lsum = group_sum(l[u]);
    if (g == 0 && qrow < T) lse[((long long)b * H + h) * T + qrow] = m[u] * scale + __logf(lsum);
    const float inv_l = 1.f / lsum;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float il = __shfl(inv_l, 4 * g + r, 64);
      const int qo = q0 + u * 16 + 4 * g + r;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const float v = o[u][db][r] * il;
        const float vn = __shfl_xor(v, 1, 64);
        if ((c & 1) == 0 && qo < T)
          *(unsigned int*)(out + ((long long)b * T + qo) * (H * HD) + h * HD + db * 16 + c) = pack_bf16x2(v, vn);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------
// backward, part 1: dQ (query on the lane) and delta = rowsum(dO * O).  No masks in the loop (see "Rows past T"); the softmax
// scale is applied once to the dQ accumulators (dS = p (dP - delta) here, without the factor).
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LTHREADS, 3) void attn_long_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out,
                                                                    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                    float* __restrict__ delta, bf16_t* __restrict__ dqkv, int T,
                                                                    int H, float scale, int nheads, int nblk, int xcds) {
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2][2][TILE];   // [buffer][K | V]; K read by rows and transposed
  int pair, blk;
  if (!decode_block(nheads, nblk, xcds, &pair, &blk)) return;
  const long long ld = 3ll * H * HD, ldo = (long long)H * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const float c1 = scale * LOG2E;
  const int b = pair / H, h = pair - b * H;
  const bf16_t* base = qkv + (long long)b * T * ld + h * HD;
  const bf16_t* Kg = base + (long long)H * HD;
  const bf16_t* Vg = base + 2ll * H * HD;
  const long long obase = (long long)b * T * ldo + h * HD;
  const int ntiles = (T + KT - 1) / KT;
  const int q0 = blk * WGROWS + wave * (NQ * 16);
  const bool active = q0 < T;
  const TileLanes tl = tile_lanes(lane);
  stage_tile_dma(Kg, ld, lds[0][0], Vg, ld, lds[0][1], 0, T, wave, lane);
  bf16x8 qf[NQ][2], dof[NQ][2];
  float lq2[NQ], dl[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int qrow = q0 + u * 16 + c;
    bf16x8 of[2];
    load_rowfrag(base, ld, qrow, T, g, qf[u]);
    load_rowfrag(dout + obase, ldo, qrow, T, g, dof[u]);
    load_rowfrag(out + obase, ldo, qrow, T, g, of);
    lq2[u] = qrow < T ? lse[(long long)pair * T + qrow] * LOG2E : INFINITY;   // a query past T: p = 2^-inf = 0
    float d = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 8; ++i) d += bf16_to_f32((bf16_t)dof[u][ks][i]) * bf16_to_f32((bf16_t)of[ks][i]);
    dl[u] = group_sum(d);
    if (g == 0 && qrow < T) delta[(long long)pair * T + qrow] = dl[u];
  }
  f32x4 dq[NQ][4];
#pragma unroll
  for (int u = 0; u < NQ; ++u)
#pragma unroll
    for (int db = 0; db < 4; ++db) dq[u][db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int j = 0; j < ntiles; ++j) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (j + 1 < ntiles)
      stage_tile_dma(Kg, ld, lds[(j + 1) & 1][0], Vg, ld, lds[(j + 1) & 1][1], (j + 1) * KT, T, wave, lane);
    if (!active) continue;
    const unsigned Ka = lds_addr(lds[j & 1][0]), Va = lds_addr(lds[j & 1][1]);
    // per pair of key blocks: S^T and dP^T (key on the accumulator rows, query on the lane) -> dS^T -> straight into
    // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
    static_for<0, 2>([&](auto pc) {
      constexpr int pp = decltype(pc)::value;
      bf16x8 kf[2][2], vf[2][2];
      bf16x4 tlo[4], thi[4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        kf[0][ks] = lds_r128<bf16x8, pp * 4096>(Ka + tl.row[ks]);
        vf[0][ks] = lds_r128<bf16x8, pp * 4096>(Va + tl.row[ks]);
        kf[1][ks] = lds_r128<bf16x8, pp * 4096 + 2048>(Ka + tl.row[ks]);
        vf[1][ks] = lds_r128<bf16x8, pp * 4096 + 2048>(Va + tl.row[ks]);
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        tlo[db] = lds_tr64<pp * 4096>(Ka + tl.tr[db]);
        thi[db] = lds_tr64<pp * 4096 + 2048>(Ka + tl.tr[db]);
      }
      lds_wait(kf[0][0], kf[0][1], kf[1][0], kf[1][1], vf[0][0], vf[0][1], vf[1][0], vf[1][1]);
      lds_wait(tlo[0], tlo[1], tlo[2], tlo[3], thi[0], thi[1], thi[2], thi[3]);
      bf16x8 dsf[NQ];
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        f32x4 ds2[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kk][ks], qf[u][ks], s, 0, 0, 0);      // S^T[key][query]
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[kk][ks], dof[u][ks], dp, 0, 0, 0);   // dP^T[key][query]
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = clamp01(__builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c1, -lq2[u])));
            ds2[kk][r] = p * (dp[r] - dl[u]);
          }
        }
        dsf[u] = pack_acc2(ds2[0], ds2[1]);
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const bf16x8 ktf = join(tlo[db], thi[db]);                                               // A[d = db*16 + c][keys]
#pragma unroll
        for (int u = 0; u < NQ; ++u)
          dq[u][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ktf, dsf[u], dq[u][db], 0, 0, 0);   // D[d 4g+r][query c]
      }
    });
  }
  if (!active) return;
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int qrow = q0 + u * 16 + c;
    if (qrow < T) {
      bf16_t* dst = dqkv + ((long long)b * T + qrow) * ld + h * HD;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        u32x2 pk;
        pk[0] = pack_bf16x2(dq[u][db][0] * scale, dq[u][db][1] * scale);
        pk[1] = pack_bf16x2(dq[u][db][2] * scale, dq[u][db][3] * scale);
        *(u32x2*)(dst + db * 16 + 4 * g) = pk;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------
// backward, part 2: dK and dV (key on the lane; a wave owns two key blocks and walks all query tiles).  Next to the Q and dO tile
// the ring carries the tile's lse (as log2, +inf past T: those queries get p = 0) and delta rows.  No masks in the loop (a key
// lane past T computes values nobody stores); the scale is applied once to dK.
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LTHREADS, 2) void attn_long_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                                     bf16_t* __restrict__ dqkv, int T, int H, float scale, int nheads,
                                                                     int nblk, int xcds) {
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2][2][TILE];   // [buffer][Q | dO]: each read by rows and transposed
  __shared__ __attribute__((aligned(16))) float s_row[2][2][KT];              // [buffer][lse * log2(e) | delta]
  int pair, blk;
  if (!decode_block(nheads, nblk, xcds, &pair, &blk)) return;
  const long long ld = 3ll * H * HD, ldo = (long long)H * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const float c1 = scale * LOG2E;
  const int b = pair / H, h = pair - b * H;
  const bf16_t* Qg = qkv + (long long)b * T * ld + h * HD;
  const bf16_t* Dg = dout + (long long)b * T * ldo + h * HD;
  const int ntiles = (T + KT - 1) / KT;
  const int k0 = blk * WGROWS + wave * (NQ * 16);
  const bool active = k0 < T;
  const TileLanes tl = tile_lanes(lane);
  // threads [0, 64) carry the lse row of a tile, threads [64, 128) its delta row
  auto load_row = [&](int row0) {
    const int r = row0 + (threadIdx.x & 63);
    if (threadIdx.x < 64) return r < T ? lse[(long long)pair * T + r] * LOG2E : INFINITY;
    return r < T ? delta[(long long)pair * T + r] : 0.f;
  };
  float rowv = threadIdx.x < 128 ? load_row(0) : 0.f;
  stage_tile_dma(Qg, ld, lds[0][0], Dg, ldo, lds[0][1], 0, T, wave, lane);
  if (threadIdx.x < 128) s_row[0][threadIdx.x >> 6][threadIdx.x & 63] = rowv;
  bf16x8 kf[NQ][2], vf[NQ][2];
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    load_rowfrag(Qg + (long long)H * HD, ld, k0 + u * 16 + c, T, g, kf[u]);
    load_rowfrag(Qg + 2ll * H * HD, ld, k0 + u * 16 + c, T, g, vf[u]);
  }
  f32x4 dk[NQ][4], dv[NQ][4];
#pragma unroll
  for (int u = 0; u < NQ; ++u)
#pragma unroll
    for (int db = 0; db < 4; ++db) { dk[u][db] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[u][db] = dk[u][db]; }
#pragma unroll 1
  for (int j = 0; j < ntiles; ++j) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (j + 1 < ntiles) {
      if (threadIdx.x < 128) rowv = load_row((j + 1) * KT);
      stage_tile_dma(Qg, ld, lds[(j + 1) & 1][0], Dg, ldo, lds[(j + 1) & 1][1], (j + 1) * KT, T, wave, lane);
    }
    if (active) {
      const unsigned Qa = lds_addr(lds[j & 1][0]), Da = lds_addr(lds[j & 1][1]);
      const unsigned La = lds_addr(&s_row[j & 1][0][4 * g]);
      static_for<0, 2>([&](auto pc) {
        constexpr int pp = decltype(pc)::value;   // queries 32 pp .. 32 pp + 31 of the tile
        bf16x8 qf[2][2], df[2][2];
        bf16x4 qlo[4], qhi[4], dlo[4], dhi[4];
        f32x4 l4[2], d4[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          qf[0][ks] = lds_r128<bf16x8, pp * 4096>(Qa + tl.row[ks]);
          df[0][ks] = lds_r128<bf16x8, pp * 4096>(Da + tl.row[ks]);
          qf[1][ks] = lds_r128<bf16x8, pp * 4096 + 2048>(Qa + tl.row[ks]);
          df[1][ks] = lds_r128<bf16x8, pp * 4096 + 2048>(Da + tl.row[ks]);
        }
        l4[0] = lds_r128<f32x4, pp * 128>(La);                 // queries 32 pp + 4 g + r
        l4[1] = lds_r128<f32x4, pp * 128 + 64>(La);            // queries 32 pp + 16 + 4 g + r
        d4[0] = lds_r128<f32x4, KT * 4 + pp * 128>(La);
        d4[1] = lds_r128<f32x4, KT * 4 + pp * 128 + 64>(La);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          qlo[db] = lds_tr64<pp * 4096>(Qa + tl.tr[db]);
          qhi[db] = lds_tr64<pp * 4096 + 2048>(Qa + tl.tr[db]);
          dlo[db] = lds_tr64<pp * 4096>(Da + tl.tr[db]);
          dhi[db] = lds_tr64<pp * 4096 + 2048>(Da + tl.tr[db]);
        }
        lds_wait(qf[0][0], qf[0][1], qf[1][0], qf[1][1], df[0][0], df[0][1], df[1][0], df[1][1]);
        lds_wait(l4[0], l4[1], d4[0], d4[1]);
        lds_wait(qlo[0], qlo[1], qlo[2], qlo[3], qhi[0], qhi[1], qhi[2], qhi[3]);
        lds_wait(dlo[0], dlo[1], dlo[2], dlo[3], dhi[0], dhi[1], dhi[2], dhi[3]);
        bf16x8 pf[NQ], dsf[NQ];
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          f32x4 p2[2], ds2[2];
#pragma unroll
          for (int qq = 0; qq < 2; ++qq) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[qq][ks], kf[u][ks], s, 0, 0, 0);     // S[query 4g+r][key c]
              dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[qq][ks], vf[u][ks], dp, 0, 0, 0);   // dP[query][key]
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c1, -l4[qq][r]));
              p2[qq][r] = p;
              ds2[qq][r] = p * (dp[r] - d4[qq][r]);
            }
          }
          pf[u] = pack_acc2(p2[0], p2[1]);     // B[k = queries 32pp + 4g + r | 32pp + 16 + 4g + r][col = key c]
          dsf[u] = pack_acc2(ds2[0], ds2[1]);
        }
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const bf16x8 dotf = join(dlo[db], dhi[db]);   // A[d][queries] = dO^T
          const bf16x8 qtf = join(qlo[db], qhi[db]);    // A[d][queries] = Q^T
#pragma unroll
          for (int u = 0; u < NQ; ++u) {
            dv[u][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dotf, pf[u], dv[u][db], 0, 0, 0);   // dV^T[d 4g+r][key c]
            dk[u][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qtf, dsf[u], dk[u][db], 0, 0, 0);   // dK^T[d 4g+r][key c]
          }
        }
      });
    }
    // the next tile's lse / delta rows: written behind this tile's work, seen by everybody after the next barrier
    if (j + 1 < ntiles && threadIdx.x < 128) s_row[(j + 1) & 1][threadIdx.x >> 6][threadIdx.x & 63] = rowv;
  }
  if (!active) return;
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int krow = k0 + u * 16 + c;
    if (krow < T) {
      bf16_t* dstk = dqkv + ((long long)b * T + krow) * ld + (long long)H * HD + h * HD;
      bf16_t* dstv = dqkv + ((long long)b * T + krow) * ld + 2ll * H * HD + h * HD;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        u32x2 pk;
        pk[0] = pack_bf16x2(dk[u][db][0] * scale, dk[u][db][1] * scale);
        pk[1] = pack_bf16x2(dk[u][db][2] * scale, dk[u][db][3] * scale);
        *(u32x2*)(dstk + db * 16 + 4 * g) = pk;
        pk[0] = pack_bf16x2(dv[u][db][0], dv[u][db][1]);
        pk[1] = pack_bf16x2(dv[u][db][2], dv[u][db][3]);
        *(u32x2*)(dstv + db * 16 + 4 * g) = pk;
      }
    }
  }
}

// blocks per pair, XCD count of the order, and the grid that covers every (pair, block) under it
struct LongGrid { int nblk, xcds; unsigned blocks; };
inline LongGrid long_grid(int nheads, int T) {
  LongGrid gr;
  gr.nblk = (T + WGROWS - 1) / WGROWS;
  gr.xcds = icamd_num_xccs() == 8 ? 8 : 1;
  const long long pairs = ((long long)nheads + gr.xcds - 1) / gr.xcds * gr.xcds;
  gr.blocks = (unsigned)(pairs * gr.nblk);
  return gr;
}

}  // namespace

int icamd_attention_long_fwd_launch(const bf16_t* qkv, bf16_t* out, float* lse, int B, int T, int H, float scale, hipStream_t s) {
  const int nheads = B * H;
  const LongGrid gr = long_grid(nheads, T);
  hipLaunchKernelGGL(attn_long_fwd_kernel, dim3(gr.blocks), dim3(LTHREADS), 0, s, qkv, out, lse, T, H, scale, nheads, gr.nblk,
                     gr.xcds);
  return icamd_launch_status();
}

int icamd_attention_long_bwd_launch(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, float* delta,
                                    bf16_t* dqkv, int B, int T, int H, float scale, hipStream_t s) {
  const int nheads = B * H;
  const LongGrid gr = long_grid(nheads, T);
  hipLaunchKernelGGL(attn_long_bwd_dq_kernel, dim3(gr.blocks), dim3(LTHREADS), 0, s, qkv, out, dout, lse, delta, dqkv, T, H, scale,
                     nheads, gr.nblk, gr.xcds);
  hipLaunchKernelGGL(attn_long_bwd_dkv_kernel, dim3(gr.blocks), dim3(LTHREADS), 0, s, qkv, dout, lse, delta, dqkv, T, H, scale,
                     nheads, gr.nblk, gr.xcds);
  return icamd_launch_status();
}
