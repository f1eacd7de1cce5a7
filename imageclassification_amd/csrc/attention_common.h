// Fragment helpers shared by the attention translation units (attention.hip: T <= 208 resident in LDS; attention_long.hip:
// K/V or Q/dO tiles streamed through an LDS ring).  Head dimension 64, bf16 operands, v_mfma_f32_16x16x32_bf16.
#pragma once
#include "common.h"

// the tiled route for any T (attention_long.hip); same contracts as icamd_attention_fwd_launch / _bwd_launch
int icamd_attention_long_fwd_launch(const bf16_t* qkv, bf16_t* out, float* lse, int B, int T, int H, float scale, hipStream_t s);
int icamd_attention_long_bwd_launch(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, float* delta,
                                    bf16_t* dqkv, int B, int T, int H, float scale, hipStream_t s);

namespace {

constexpr int HD = 64;          // head dimension
constexpr int ROWB = HD * 2;    // bytes per LDS row

// LDS image of a [rows][64] bf16 matrix (128 B rows): the 32 B column block is XOR-ed with (row>>1)&3.  ONE image
// serves both access patterns without bank conflicts: 4-row x 16-column blocks read transposed (ds_read_b64_tr_b16; a
// 32-lane half touches 8 rows x 32 B = 2 row parities x 4 block keys) and 16 B chunks of one row per lane
// (ds_read_b128; its 16-lane groups {0-3, 12-15, 20-27}, ... hold rows of four different keys for the even chunk and
// of four for the odd one).  Keeping a single image per matrix is what lets two workgroups share a CU's 160 KB.
__device__ __forceinline__ int tr_img(int row, int chunk) {
  return row * ROWB + ((((chunk >> 1) ^ ((row >> 1) & 3))) << 5) + ((chunk & 1) << 4);
}
__device__ __forceinline__ int row_img(int row, int chunk) { return tr_img(row, chunk); }

__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* img, int row0, int row1, int dblk, int lane) {
  const int c = lane & 15, q = c >> 2, pq = c & 3;
  const int ra = row0 + q, rb = row1 + q;
  bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (bf16x4 __attribute__((address_space(3)))*)(img + ra * ROWB + ((dblk ^ ((ra >> 1) & 3)) << 5) + 8 * pq));
  bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (bf16x4 __attribute__((address_space(3)))*)(img + rb * ROWB + ((dblk ^ ((rb >> 1) & 3)) << 5) + 8 * pq));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

__device__ __forceinline__ bf16x8 pack_acc2(const f32x4& lo, const f32x4& hi) {   // four v_cvt_pk_bf16_f32
  u32x4 r;
  r[0] = pack_bf16x2(lo[0], lo[1]);
  r[1] = pack_bf16x2(lo[2], lo[3]);
  r[2] = pack_bf16x2(hi[0], hi[1]);
  r[3] = pack_bf16x2(hi[2], hi[3]);
  return __builtin_bit_cast(bf16x8, r);
}

// B-operand fragments of a row-major [row][64] matrix straight from global memory: lane (c, g) takes row `row`,
// columns 8g..8g+7 (+32 for the second k-step)
__device__ __forceinline__ void load_rowfrag(const bf16_t* __restrict__ base, long long ld, int row, int T, int g,
                                             bf16x8* f) {
  // rows past T read the zero page: a select AFTER the loads (round 1-4: `if (row >= T) f = 0`) made every caller wait for the
  // loads on the spot -- the "prefetch" of the next head's fragments at the top of a head was followed by s_waitcnt vmcnt(0)
  // before the first MFMA (round 5, found in the ISA)
  const bf16_t* p = row < T ? base + (long long)row * ld + 8 * g : (const bf16_t*)icamd_zero_page;
  f[0] = *(const bf16x8*)p;
  f[1] = *(const bf16x8*)(p + (row < T ? 32 : 0));
}

// The same two loads issued behind hipcc's back (round 5): its s_waitcnt pass put vmcnt(3..0) in front of the first MFMAs of a head
// for loads whose results are only read after the head (the next head's fragments) -- seen in the ISA of all three kernels,
// whatever the source did about selects and stores.  The results must not be touched before prefetch_wait() has named them.
__device__ __forceinline__ void load_rowfrag_async(const bf16_t* __restrict__ base, long long ld, int row, int T, int g,
                                                   bf16x8* f) {
  const bf16_t* p = row < T ? base + (long long)row * ld + 8 * g : (const bf16_t*)icamd_zero_page;
  const bf16_t* p1 = p + (row < T ? 32 : 0);
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(f[0]) : "v"(p) : "memory");
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(f[1]) : "v"(p1) : "memory");
}

// v_max3_f32 as is (fmaxf adds a canonicalising v_max per operand that comes out of an MFMA)
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// A probability recomputed from a stored log-sum-exp, p = 2^(s c1 - lse log2 e), held to [0, 1]: it is <= 1 for every key the lse was
// taken over (an fp32 rounding above 1 becomes 1), so this changes nothing there, and for a zero-filled key row past T (s = 0, p = e^-lse) of a query whose lse is below
// -88.7 it is 1 instead of +inf.  med3(p, 0, 1) folds into the clamp bit of v_exp_f32: no instruction, no register.
__device__ __forceinline__ float clamp01(float p) { return __builtin_amdgcn_fmed3f(p, 0.f, 1.f); }
__device__ __forceinline__ float group_max(float v) {   // across the 4 lane groups that share a column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

}  // namespace
