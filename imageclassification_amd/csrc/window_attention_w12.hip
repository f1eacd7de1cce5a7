// Shifted-window attention for 12 x 12 windows (T = 144 tokens, D = 32) on gfx950: what swin_base_patch4_window12_384 runs in every
// block whose stage has 12 or more tokens per side.  Same C-ABI entries and the same contract as window_attention.hip (natural token
// order in and out, roll / partition / reverse / region mask as address arithmetic by the rule of win_token, scale before bias and
// mask, fp32 softmax / dS / accumulation, P and dS rounded to bf16 once as MFMA operands, dbias from the fp32 dS, no atomics);
// window_attention.hip's launch functions hand every ws == 12 call to the two launchers at the bottom.
//
// Execution: ONE WORKGROUP of three waves owns one (window, head) pair at a time -- 9 x 9 MFMA tiles of v_mfma_f32_16x16x32_bf16,
// and with D = 32 one k-step covers q k^T.  blockIdx.y is the head, blockIdx.x a chunk of windows (window wi = blockIdx.x + trip *
// gridDim.x, the same for the whole workgroup, so every barrier is uniform).  Wave w takes query blocks 3w..3w+2 (forward, and the
// dQ / dbias half of the backward) and key blocks 3w..3w+2 (the dK / dV half): three blocks each, no tail.  The window's matrices are
// staged once per pair as LDS images ([160][32] bf16, rows 80 B apart as in window_attention.hip; rows 144..159 are zero and pad the
// fifth 32-wide k-step of the products over keys / queries): V and K forward (25 KB), K, V, Q and dO backward (50 KB).  Row fragments (MFMA operands, 16 B per lane) are read from the images with ds_read_b128, transposed operands with
// ds_read_b64_tr_b16; the forward keeps its nine K fragments in registers for the whole pair.  As in window_attention.hip the score
// tile is computed transposed relative to its consumer, so an accumulator tile is the next product's operand.
//
// Bias: read from global memory (L2), not staged.  bias[h] is [144][144] fp32 = 81 KB; in LDS it would leave one workgroup of three
// waves per CU, and its reads would still be one per score tile.  All heads of a layer are at most 2.6 MB and are read by every
// workgroup of the launch, so they stay in L2; in the query-on-lane layout a lane's four keys are one 16 B load (taken when the
// bias pointer is 16 B aligned, four 4 B loads otherwise), in the key-on-lane layout sixteen lanes read 64 contiguous bytes.
//
// dbias: wave w owns the query rows 48w..48w+47 of the pair, so its fp32 sum of dS^T over the windows the workgroup walks lives in
// 3 x 9 accumulator tiles (108 registers) and is written straight to the workgroup's partial [144][144] -- no fold across waves.
// A second launch folds the partials in workgroup order.  The backward runs at most 512 workgroups (all heads together), so the
// workspace is at most 512 * 81 KB = 40.5 MB; that cap is reached by every stage of Swin-B at 384^2, batch 64 (4096 / 1024 / 256 /
// 64 windows of 4 / 8 / 16 / 32 heads), whose activations of one block are several times that.  The chunking depends on the problem
// shape only, so every output is bitwise repeatable.
//
// Registers (build/window_attention_w12-*.s): forward 172 VGPRs, backward 446 (256 + 190 accumulation registers), no spills and no
// private segment in either.  The backward therefore runs one wave per SIMD -- one workgroup per CU; the sched_barrier after
// every 32-wide step is what keeps the scheduler from hoisting all later steps' loads to the top and spilling.  Bringing it under 256
// registers (two workgroups per CU) is left for a later change.
#include "common.h"
#include "icamd_internal.h"
#include "attention_common.h"   // pack_acc2, group_max, group_sum

namespace {

constexpr int WS = 12, T = WS * WS;    // window side, tokens per window
constexpr int NB = T / 16;             // 16-row blocks per side: 9
constexpr int WD = 32;                 // head dimension
constexpr int WROW = 80;               // bytes between rows of an LDS image (64 B of data)
constexpr int IMG_ROWS = 160;          // 144 tokens + 16 zero rows: the second half of the fifth 32-wide k-step
constexpr int WIMG = IMG_ROWS * WROW;  // 12800 B
constexpr int WAVES = 3, THREADS = 64 * WAVES, BPW = NB / WAVES;   // three blocks per wave
constexpr int FWD_CAP = 2048, BWD_CAP = 512;                       // workgroups of a launch, all heads together
constexpr float LOG2E = 1.4426950408889634f;

struct Geom12 {
  int Hs, Ws, shift;
  int nWc, nW, H;       // windows per row, windows per image, heads
};

// slot -> token row of the [B*Hs*Ws] activation matrices and mask region id: win_token of window_attention.hip with ws = 12 (every
// slot of a 144-token window exists)
__device__ __forceinline__ void win_token12(const Geom12& G, int wi, int slot, int& tok, int& rid) {
  const int b = wi / G.nW, w = wi - b * G.nW;
  const int wr = w / G.nWc, wc = w - wr * G.nWc;
  const int ir = slot / WS, ic = slot - ir * WS;
  const int rr = wr * WS + ir, rc = wc * WS + ic;           // coordinates on the rolled grid
  int sr = rr + G.shift, sc = rc + G.shift;                 // where that token lives in the natural order
  if (sr >= G.Hs) sr -= G.Hs;
  if (sc >= G.Ws) sc -= G.Ws;
  tok = (b * G.Hs + sr) * G.Ws + sc;
  rid = 0;
  if (G.shift > 0) {
    const int a = rr < G.Hs - WS ? 0 : (rr < G.Hs - G.shift ? 1 : 2);
    const int c = rc < G.Ws - WS ? 0 : (rc < G.Ws - G.shift ? 1 : 2);
    rid = 3 * a + c;
  }
}

// rows 144..159 of `nimg` consecutive images are zeroed once per kernel; nothing writes them afterwards
__device__ __forceinline__ void zero_pad_rows(unsigned char* imgs, int nimg) {
  constexpr int CH = (IMG_ROWS - T) * WROW / 16;            // 16 B chunks of the pad rows of one image
  for (int i = threadIdx.x; i < nimg * CH; i += THREADS) {
    const int im = i / CH, ch = i - im * CH;
    *(u32x4*)(imgs + im * WIMG + T * WROW + ch * 16) = u32x4{0u, 0u, 0u, 0u};
  }
}

// the 16 B chunk (row, ch) of the [144][32] matrix `base` of this window; row -> token through s_tok
__device__ __forceinline__ u32x4 load_chunk(const bf16_t* __restrict__ base, long long ld, int tok, int ch) {
  return *(const u32x4*)(base + (long long)tok * ld + 8 * ch);
}

// row fragment: lane (c, g) takes row `row`, columns 8g..8g+7
__device__ __forceinline__ bf16x8 frag(const unsigned char* img, int row, int g) {
  return *(const bf16x8*)(img + row * WROW + 16 * g);
}

// transposed operand, as tr_pair32 of window_attention.hip
__device__ __forceinline__ bf16x8 tr_pair32(const unsigned char* img, int row0, int row1, int dblk, int lane) {
  const int c = lane & 15, q = c >> 2, pq = c & 3;
  bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (bf16x4 __attribute__((address_space(3)))*)(img + (row0 + q) * WROW + dblk * 32 + 8 * pq));
  bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (bf16x4 __attribute__((address_space(3)))*)(img + (row1 + q) * WROW + dblk * 32 + 8 * pq));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <bool AL>
__device__ __forceinline__ f32x4 load_bias4(const float* __restrict__ p) {
  if (AL) return *(const f32x4*)p;
  return f32x4{p[0], p[1], p[2], p[3]};
}

// ----------------------------------------------------------------------------------------------------------------
// forward
// ----------------------------------------------------------------------------------------------------------------
template <bool AL>
__global__ __launch_bounds__(THREADS) void winattn12_fwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                                bf16_t* __restrict__ out, float* __restrict__ lse, Geom12 G,
                                                                int nwin, float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char imgs[2][WIMG];   // K | V
  __shared__ int s_tok[T], s_rid[T];
  const int h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const long long ld = 3ll * G.H * WD, ldo = (long long)G.H * WD;
  const bf16_t* qbase = qkv + h * WD;
  const bf16_t* kbase = qbase + G.H * WD;
  const bf16_t* vbase = qbase + 2 * G.H * WD;
  const float* bh = bias + (long long)h * T * T;
  unsigned char* Kimg = imgs[0];
  unsigned char* Vimg = imgs[1];
  zero_pad_rows(&imgs[0][0], 2);
  for (int wi = blockIdx.x; wi < nwin; wi += gridDim.x) {
    if (threadIdx.x < T) {
      int tok, rid;
      win_token12(G, wi, threadIdx.x, tok, rid);
      s_tok[threadIdx.x] = tok;
      s_rid[threadIdx.x] = rid;
    }
    __syncthreads();
    {
      u32x4 kv[3], vv[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {                     // 576 chunks of 16 B per matrix, three per thread
        const int i = threadIdx.x + THREADS * k, row = i >> 2, ch = i & 3;
        const int tok = s_tok[row];
        kv[k] = load_chunk(kbase, ld, tok, ch);
        vv[k] = load_chunk(vbase, ld, tok, ch);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int i = threadIdx.x + THREADS * k, row = i >> 2, ch = i & 3;
        *(u32x4*)(Kimg + row * WROW + ch * 16) = kv[k];
        *(u32x4*)(Vimg + row * WROW + ch * 16) = vv[k];
      }
    }
    __syncthreads();
    bf16x8 kf[NB];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) kf[kb] = frag(Kimg, kb * 16 + c, g);
#pragma unroll 1
    for (int qi = 0; qi < BPW; ++qi) {
      const int qb = wave * BPW + qi;
      const int q = qb * 16 + c;                         // this lane's query slot
      const int ridq = s_rid[q];
      const bf16x8 qf = *(const bf16x8*)(qbase + (long long)s_tok[q] * ld + 8 * g);
      // S^T[key][query]: lane (c, g) holds, for query c, the keys kb*16 + 4g + r of tile kb
      f32x4 sv[NB];
      float m = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        const f32x4 bv = load_bias4<AL>(bh + q * T + kb * 16 + 4 * g);
        sv[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb], qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb * 16 + 4 * g + r;
          const float mk = s_rid[key] != ridq ? -100.f : 0.f;
          sv[kb][r] = __builtin_fmaf(sv[kb][r], scale, bv[r] + mk);
          m = fmaxf(m, sv[kb][r]);
        }
      }
      m = group_max(m);
      float l = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sv[kb][r] = __builtin_amdgcn_exp2f((sv[kb][r] - m) * LOG2E);
          l += sv[kb][r];
        }
      l = group_sum(l);
      if (g == 0) lse[((long long)wi * G.H + h) * T + q] = m + __logf(l);
      f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int pp = 0; pp < 5; ++pp) {                   // keys 32pp.. ; the last step's second half is the zero rows
        const f32x4 hi = 2 * pp + 1 < NB ? sv[(2 * pp + 1) % NB] : f32x4{0.f, 0.f, 0.f, 0.f};
        const bf16x8 pf = pack_acc2(sv[2 * pp], hi);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const bf16x8 vf = tr_pair32(Vimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);
          o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o[db], 0, 0, 0);       // D[query 4g+r][d = db*16 + c]
        }
      }
      const float inv_l = 1.f / l;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float il = __shfl(inv_l, 4 * g + r, 64);             // 1/l of query 4g+r (held by the lanes with c == 4g+r)
        const int tq = s_tok[qb * 16 + 4 * g + r];
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const float v = o[db][r] * il;
          const float vn = __shfl_xor(v, 1, 64);
          if ((c & 1) == 0) *(unsigned int*)(out + (long long)tq * ldo + h * WD + db * 16 + c) = pack_bf16x2(v, vn);
        }
      }
    }
    __syncthreads();                                     // the images and s_tok are rewritten by the next window
  }
}

// ----------------------------------------------------------------------------------------------------------------
// backward: dQ, dK, dV of every (window, head) pair and one dbias partial per workgroup
// ----------------------------------------------------------------------------------------------------------------
template <bool AL>
__global__ __launch_bounds__(THREADS) void winattn12_bwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                                const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                                const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                                                                float* __restrict__ part, Geom12 G, int nwin, float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char imgs[4][WIMG];   // K | V | Q | dO
  __shared__ __attribute__((aligned(16))) float s_lq[T], s_dl[T];        // lse * log2(e), delta = rowsum(dO * O)
  __shared__ int s_tok[T], s_rid[T];
  const int h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const long long ld = 3ll * G.H * WD, ldo = (long long)G.H * WD;
  const bf16_t* qbase = qkv + h * WD;
  const bf16_t* kbase = qbase + G.H * WD;
  const bf16_t* vbase = qbase + 2 * G.H * WD;
  const bf16_t* obase = out + h * WD;
  const bf16_t* dobase = dout + h * WD;
  const float* bh = bias + (long long)h * T * T;
  unsigned char* Kimg = imgs[0];
  unsigned char* Vimg = imgs[1];
  unsigned char* Qimg = imgs[2];
  unsigned char* Dimg = imgs[3];
  zero_pad_rows(&imgs[0][0], 4);
  f32x4 acc[BPW][NB];                                    // sum of dS^T over this workgroup's windows: [own query block][key block]
#pragma unroll
  for (int a = 0; a < BPW; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int wi = blockIdx.x; wi < nwin; wi += gridDim.x) {
    if (threadIdx.x < T) {
      int tok, rid;
      win_token12(G, wi, threadIdx.x, tok, rid);
      s_tok[threadIdx.x] = tok;
      s_rid[threadIdx.x] = rid;
      s_lq[threadIdx.x] = lse[((long long)wi * G.H + h) * T + threadIdx.x] * LOG2E;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {                         // 576 chunks of 16 B per matrix, three per thread; four lanes share a row
      const int i = threadIdx.x + THREADS * k, row = i >> 2, ch = i & 3;
      const int tok = s_tok[row];
      const u32x4 kv = load_chunk(kbase, ld, tok, ch);
      const u32x4 vv = load_chunk(vbase, ld, tok, ch);
      const u32x4 qv = load_chunk(qbase, ld, tok, ch);
      const u32x4 dv = load_chunk(dobase, ldo, tok, ch);
      const u32x4 ov = load_chunk(obase, ldo, tok, ch);
      *(u32x4*)(Kimg + row * WROW + ch * 16) = kv;
      *(u32x4*)(Vimg + row * WROW + ch * 16) = vv;
      *(u32x4*)(Qimg + row * WROW + ch * 16) = qv;
      *(u32x4*)(Dimg + row * WROW + ch * 16) = dv;
      float dl = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) dl += bf16_lo(dv[e]) * bf16_lo(ov[e]) + bf16_hi(dv[e]) * bf16_hi(ov[e]);
      dl += __shfl_xor(dl, 1, 64);
      dl += __shfl_xor(dl, 2, 64);
      if (ch == 0) s_dl[row] = dl;
    }
    __syncthreads();
    // ---- query on the lane: dS^T -> dbias and dQ
#pragma unroll
    for (int qi = 0; qi < BPW; ++qi) {
      const int qb = wave * BPW + qi;
      const int q = qb * 16 + c;
      const float lq = s_lq[q], dl = s_dl[q];
      const int ridq = s_rid[q];
      const bf16x8 qf = frag(Qimg, q, g), dof = frag(Dimg, q, g);
      f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int pp = 0; pp < 5; ++pp) {
        f32x4 ds[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int kb = 2 * pp + u;
          if (kb < NB) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 bv = load_bias4<AL>(bh + q * T + kb * 16 + 4 * g);
            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(Kimg, kb * 16 + c, g), qf, z, 0, 0, 0);    // S^T[key 4g+r][query c]
            const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(Vimg, kb * 16 + c, g), dof, z, 0, 0, 0);  // dP^T
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kb * 16 + 4 * g + r;
              const float mk = s_rid[key] != ridq ? -100.f : 0.f;
              const float sc = __builtin_fmaf(s[r], scale, bv[r] + mk);
              const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc, LOG2E, -lq));
              ds[u][r] = p * (dp[r] - dl);
              acc[qi][kb][r] += ds[u][r];
            }
          }
        }
        const bf16x8 dsf = pack_acc2(ds[0], ds[1]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const bf16x8 ktf = tr_pair32(Kimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);   // A[d = db*16 + c][keys]
          dq[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ktf, dsf, dq[db], 0, 0, 0);           // D[d 4g+r][query c]
        }
        __builtin_amdgcn_sched_barrier(0);             // keep the scheduler from hoisting every later step's loads up here
      }
      bf16_t* dst = dqkv + (long long)s_tok[q] * ld + h * WD;
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        u32x2 pk;
        pk[0] = pack_bf16x2(dq[db][0] * scale, dq[db][1] * scale);
        pk[1] = pack_bf16x2(dq[db][2] * scale, dq[db][3] * scale);
        *(u32x2*)(dst + db * 16 + 4 * g) = pk;
      }
    }
    // ---- key on the lane: dK and dV
#pragma unroll 1
    for (int ki = 0; ki < BPW; ++ki) {
      const int kb = wave * BPW + ki;
      const int key = kb * 16 + c;
      const int ridk = s_rid[key];
      const bf16x8 kf = frag(Kimg, key, g), vf = frag(Vimg, key, g);
      f32x4 dk[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      f32x4 dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int pp = 0; pp < 5; ++pp) {
        f32x4 p2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        f32x4 ds2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int qb = 2 * pp + u;
          if (qb < NB) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(Qimg, qb * 16 + c, g), kf, z, 0, 0, 0);    // S[query 4g+r][key c]
            const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(Dimg, qb * 16 + c, g), vf, z, 0, 0, 0);   // dP
            const f32x4 l4 = *(const f32x4*)&s_lq[qb * 16 + 4 * g];
            const f32x4 d4 = *(const f32x4*)&s_dl[qb * 16 + 4 * g];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int q = qb * 16 + 4 * g + r;
              const float bv = bh[q * T + key];
              const float mk = s_rid[q] != ridk ? -100.f : 0.f;
              const float sc = __builtin_fmaf(s[r], scale, bv + mk);
              const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc, LOG2E, -l4[r]));
              p2[u][r] = p;
              ds2[u][r] = p * (dp[r] - d4[r]);
            }
          }
        }
        const bf16x8 pf = pack_acc2(p2[0], p2[1]);       // B[k = queries 32pp + 4g + r | 32pp + 16 + 4g + r][col = key c]
        const bf16x8 dsf = pack_acc2(ds2[0], ds2[1]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const bf16x8 dotf = tr_pair32(Dimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);   // A[d][queries] = dO^T
          const bf16x8 qtf = tr_pair32(Qimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);    // A[d][queries] = Q^T
          dv[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dotf, pf, dv[db], 0, 0, 0);            // dV^T[d 4g+r][key c]
          dk[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qtf, dsf, dk[db], 0, 0, 0);            // dK^T[d 4g+r][key c]
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      const long long tk = s_tok[key];
      bf16_t* dstk = dqkv + tk * ld + (long long)G.H * WD + h * WD;
      bf16_t* dstv = dqkv + tk * ld + 2ll * G.H * WD + h * WD;
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        u32x2 pk;
        pk[0] = pack_bf16x2(dk[db][0] * scale, dk[db][1] * scale);
        pk[1] = pack_bf16x2(dk[db][2] * scale, dk[db][3] * scale);
        *(u32x2*)(dstk + db * 16 + 4 * g) = pk;
        pk[0] = pack_bf16x2(dv[db][0], dv[db][1]);
        pk[1] = pack_bf16x2(dv[db][2], dv[db][3]);
        *(u32x2*)(dstv + db * 16 + 4 * g) = pk;
      }
    }
    __syncthreads();                                     // the images and row vectors are rewritten by the next window
  }
  // this wave's 48 query rows of the workgroup's partial: lane (c, g) holds query qb*16 + c, keys kb*16 + 4g..+3
  float* dst = part + ((long long)blockIdx.x * G.H + h) * T * T;
#pragma unroll
  for (int qi = 0; qi < BPW; ++qi)
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
      *(f32x4*)(dst + ((wave * BPW + qi) * 16 + c) * T + kb * 16 + 4 * g) = acc[qi][kb];
}

// dbias[i] (+)= sum over the P partials, in order
__global__ __launch_bounds__(256) void winattn12_dbias_fold_kernel(const float* __restrict__ part, float* __restrict__ dbias, int n,
                                                                   int P, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[(long long)p * n + i];
  dbias[i] = accumulate ? dbias[i] + s : s;
}

Geom12 make_geom12(int Hs, int Ws, int H, int shift) {
  Geom12 G;
  G.Hs = Hs; G.Ws = Ws; G.shift = shift;
  G.nWc = Ws / WS; G.nW = (Hs / WS) * G.nWc; G.H = H;
  return G;
}

// workgroups per head: one per window until the launch would pass `cap` workgroups over all heads
int chunks12(long long nwin, int H, int cap) {
  const long long per_head = cap / H > 1 ? cap / H : 1;
  return (int)(nwin < per_head ? nwin : per_head);
}

}  // namespace

// workgroups per head of the backward (= dbias partials per head): a function of the problem shape only
int icamd_window_attention_w12_bwd_chunks(long long nwin, int H) { return chunks12(nwin, H, BWD_CAP); }

int icamd_window_attention_w12_fwd_launch(const bf16_t* qkv, const float* bias, bf16_t* out, float* lse, int B, int Hs, int Ws, int H,
                                          int shift, float scale, hipStream_t s) {
  const Geom12 G = make_geom12(Hs, Ws, H, shift);
  const long long nwin = (long long)B * G.nW;
  const dim3 grid((unsigned)chunks12(nwin, H, FWD_CAP), (unsigned)H);
  if (((uintptr_t)bias & 15) == 0)
    hipLaunchKernelGGL(winattn12_fwd_kernel<true>, grid, dim3(THREADS), 0, s, qkv, bias, out, lse, G, (int)nwin, scale);
  else
    hipLaunchKernelGGL(winattn12_fwd_kernel<false>, grid, dim3(THREADS), 0, s, qkv, bias, out, lse, G, (int)nwin, scale);
  return icamd_launch_status();
}

int icamd_window_attention_w12_bwd_launch(const bf16_t* qkv, const float* bias, const bf16_t* out, const bf16_t* dout,
                                          const float* lse, bf16_t* dqkv, float* dbias, int accumulate, float* part, int B, int Hs,
                                          int Ws, int H, int shift, float scale, hipStream_t s) {
  const Geom12 G = make_geom12(Hs, Ws, H, shift);
  const long long nwin = (long long)B * G.nW;
  const int P = icamd_window_attention_w12_bwd_chunks(nwin, H);
  const dim3 grid((unsigned)P, (unsigned)H);
  if (((uintptr_t)bias & 15) == 0)
    hipLaunchKernelGGL(winattn12_bwd_kernel<true>, grid, dim3(THREADS), 0, s, qkv, bias, out, dout, lse, dqkv, part, G, (int)nwin,
                       scale);
  else
    hipLaunchKernelGGL(winattn12_bwd_kernel<false>, grid, dim3(THREADS), 0, s, qkv, bias, out, dout, lse, dqkv, part, G, (int)nwin,
                       scale);
  const int n = H * T * T;
  hipLaunchKernelGGL(winattn12_dbias_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, dbias, n, P, accumulate);
  return icamd_launch_status();
}
