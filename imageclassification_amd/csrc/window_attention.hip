// Swin Transformer device work on gfx950: shifted-window attention (forward, backward with the relative-position-bias gradient),
// the relative-position table <-> bias gather / scatter, and patch merging fused with its LayerNorm.
//
// Replaces what ATen runs for timm's WindowAttention / SwinTransformerBlock._attn / PatchMerging under `model(samples)` and
// `loss.backward()` of the reference step (/root/reference/engine.py:48,51,64,72) for swin_*_patch4_window7_224.
//
// Window attention.  qkv is the [B][Hs][Ws][3*H*32] output of the fused QKV projection in the NATURAL token order (columns
// q | k | v, each [head][32]); out / dout are [B][Hs][Ws][H*32], dqkv mirrors qkv.  The roll by (-shift, -shift), the window
// partition, the window reverse and the roll back are address arithmetic: slot i of window (wr, wc) of image b is the token at
// ((wr*ws + i/ws + shift) mod Hs, (wc*ws + i%ws + shift) mod Ws), and its mask region is that of timm's img_mask on the rolled
// grid (win_token below; imageclassification_amd/swin.py window_geometry is the host-side statement of the same rule and the tests
// compare the two).  No permuted copy of an activation and no mask tensor exists.
//
// Windows of side 2..8; 12 x 12 windows are window_attention_w12.hip's, reached through the launch functions below.
//
// Execution: ONE WAVE owns one (window, head) pair at a time -- T = ws^2 <= 64 tokens is a single 64 x 64 score tile, i.e. 4 x 4
// MFMA tiles of v_mfma_f32_16x16x32_bf16, and with D = 32 one k-step covers q k^T.  A workgroup is four such waves with the SAME
// head: blockIdx.y is the head, blockIdx.x a chunk of windows, and bias[h] ([T][T] fp32, at most 16 KB) is staged into LDS once per
// workgroup and read from there by every window the workgroup walks (from registers it would cost 64 VGPRs per layout, and the
// backward needs it in two layouts).  Row fragments (a token's 32 values of q, k, v, dO: 16 B per lane) come straight from global
// memory as MFMA operands; only the matrices that are read TRANSPOSED (V forward; K, Q, dO backward) pass through a per-wave LDS image
// ([64][32] bf16, rows 80 B apart so that the 16 B stores stay aligned and the transposed 8 B reads spread over the banks), read
// with ds_read_b64_tr_b16.  As in attention.hip the score tile is computed transposed relative to its consumer, so an accumulator
// tile is directly the next product's operand: forward S^T = K Q^T -> P^T -> O = P V; backward, query on the lane: S^T, dP^T = V dO^T
// -> dS^T -> dQ^T = K^T dS^T, and key on the lane: S = Q K^T, dP = dO V^T -> dV^T = dO^T P, dK^T = Q^T dS.  Both backward
// layouts run in the same wave on the same resident fragments (16 + 16 extra MFMAs per pair instead of a second kernel that reloads
// everything).  P and dS are rounded to bf16 once, as MFMA operands; softmax, dS and every accumulation are fp32.
//
// dbias: every wave keeps the fp32 dS of the pairs it walks in 64 accumulator registers (query-on-lane layout), the four waves of a
// workgroup are folded through LDS in wave order, each workgroup writes ONE partial [T][T] of its head to the workspace, and a second
// launch folds the partials in workgroup order.  No atomics; the chunking depends on the problem shape only, so every output is
// bitwise repeatable.
#include "common.h"
#include "icamd_internal.h"
#include "attention_common.h"   // pack_acc2, group_max, group_sum: the helpers that do not depend on the head dimension

namespace {

constexpr int WD = 32;             // head dimension
constexpr int WROW = 80;           // bytes between rows of an LDS image (64 B of data)
constexpr int WIMG = 64 * WROW;    // one [64][32] bf16 image
constexpr int WTHREADS = 256, WWAVES = WTHREADS / 64;
constexpr float LOG2E = 1.4426950408889634f;

struct WinGeom {
  int Hs, Ws, ws, shift;   // token grid, window side, cyclic shift
  int nWc, nW, T, H;       // windows per row, windows per image, tokens per window, heads
};

// slot -> token row of the [B*Hs*Ws] activation matrices (-1: the slot does not exist) and mask region id
__device__ __forceinline__ void win_token(const WinGeom& G, int wi, int slot, int& tok, int& rid) {
  tok = -1;
  rid = 0;
  if (slot < G.T) {
    const int b = wi / G.nW, w = wi - b * G.nW;
    const int wr = w / G.nWc, wc = w - wr * G.nWc;
    const int ir = slot / G.ws, ic = slot - ir * G.ws;
    const int rr = wr * G.ws + ir, rc = wc * G.ws + ic;       // coordinates on the rolled grid
    int sr = rr + G.shift, sc = rc + G.shift;                 // where that token lives in the natural order
    if (sr >= G.Hs) sr -= G.Hs;
    if (sc >= G.Ws) sc -= G.Ws;
    tok = (b * G.Hs + sr) * G.Ws + sc;
    if (G.shift > 0) {
      const int a = rr < G.Hs - G.ws ? 0 : (rr < G.Hs - G.shift ? 1 : 2);
      const int c = rc < G.Ws - G.ws ? 0 : (rc < G.Ws - G.shift ? 1 : 2);
      rid = 3 * a + c;
    }
  }
}

// 16 B of a token's row: lane (c, g) takes columns 8g..8g+7; a missing token reads the zero page
__device__ __forceinline__ bf16x8 load_frag(const bf16_t* __restrict__ base, long long ld, int tok, int g) {
  const bf16_t* p = tok >= 0 ? base + (long long)tok * ld + 8 * g : (const bf16_t*)icamd_zero_page;
  return *(const bf16x8*)p;
}

// this wave's [64][32] image of one matrix: lane l stages chunk l & 3 of rows (l >> 2) + 16k; missing rows are zeros
__device__ __forceinline__ void stage_image(unsigned char* img, const bf16_t* __restrict__ base, long long ld, int tok, int lane) {
  u32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int trow = __shfl(tok, (lane >> 2) + 16 * k, 64);
    const bf16_t* p = trow >= 0 ? base + (long long)trow * ld + 8 * (lane & 3) : (const bf16_t*)icamd_zero_page;
    v[k] = *(const u32x4*)p;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) *(u32x4*)(img + ((lane >> 2) + 16 * k) * WROW + (lane & 3) * 16) = v[k];
}

// B / A operand [k = rows row0 + 4g'.., row1 + 4g'..][16 columns of block dblk] read transposed: within a group of 16 lanes, lane i
// names row (i >> 2), columns 4 (i & 3)..+3 of a 4 x 16 block and receives column i of its four rows (attention_common.h tr_pair)
__device__ __forceinline__ bf16x8 tr_pair32(const unsigned char* img, int row0, int row1, int dblk, int lane) {
  const int c = lane & 15, q = c >> 2, pq = c & 3;
  bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (bf16x4 __attribute__((address_space(3)))*)(img + (row0 + q) * WROW + dblk * 32 + 8 * pq));
  bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (bf16x4 __attribute__((address_space(3)))*)(img + (row1 + q) * WROW + dblk * 32 + 8 * pq));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// ----------------------------------------------------------------------------------------------------------------
// forward
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WTHREADS) void winattn_fwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                               bf16_t* __restrict__ out, float* __restrict__ lse, WinGeom G,
                                                               int nwin, float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char vimg[WWAVES][WIMG];
  __shared__ float sb[64 * 64];          // bias[h]: [T][T]
  __shared__ int s_rid[WWAVES][64];
  const int h = blockIdx.y, T = G.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  for (int i = threadIdx.x; i < T * T; i += WTHREADS) sb[i] = bias[(long long)h * T * T + i];
  const long long ld = 3ll * G.H * WD, ldo = (long long)G.H * WD;
  const bf16_t* qbase = qkv + h * WD;
  const bf16_t* kbase = qbase + G.H * WD;
  const bf16_t* vbase = qbase + 2 * G.H * WD;
  const int stride = gridDim.x * WWAVES;
  const int iters = (nwin + stride - 1) / stride;     // the same for every wave: the barriers below are uniform
  const int nqb = (T + 15) >> 4;
  unsigned char* img = vimg[wave];
  for (int it = 0; it < iters; ++it) {
    const int wi = (it * gridDim.x + blockIdx.x) * WWAVES + wave;
    const bool live = wi < nwin;
    int tok = -1, rid = 0;
    if (live) win_token(G, wi, lane, tok, rid);
    stage_image(img, vbase, ld, tok, lane);
    s_rid[wave][lane] = rid;
    bf16x8 kf[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) kf[kb] = load_frag(kbase, ld, __shfl(tok, kb * 16 + c, 64), g);
    __syncthreads();
#pragma unroll 1
    for (int qb = 0; qb < nqb; ++qb) {
      const int q = qb * 16 + c;                       // this lane's query slot
      const int tokq = __shfl(tok, q, 64);
      const int ridq = s_rid[wave][q];
      const bf16x8 qf = load_frag(qbase, ld, tokq, g);
      // S^T[key][query]: lane (c, g) holds, for query c, the keys kb*16 + 4g + r of tile kb
      f32x4 sv[4];
      float m = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        sv[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb], qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb * 16 + 4 * g + r;
          const bool pair = key < T && q < T;
          const float bv = pair ? sb[q * T + key] : 0.f;
          const float mk = s_rid[wave][key] != ridq ? -100.f : 0.f;
          sv[kb][r] = key < T ? __builtin_fmaf(sv[kb][r], scale, bv + mk) : -INFINITY;   // key columns >= T take no part
          m = fmaxf(m, sv[kb][r]);
        }
      }
      m = group_max(m);                                // finite: key 0 exists
      float l = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sv[kb][r] = __builtin_amdgcn_exp2f((sv[kb][r] - m) * LOG2E);
          l += sv[kb][r];
        }
      l = group_sum(l);
      if (g == 0 && live && q < T) lse[((long long)wi * G.H + h) * T + q] = m + __logf(l);
      f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        const bf16x8 pf = pack_acc2(sv[2 * pp], sv[2 * pp + 1]);   // A[query c][k = keys 32pp + 4g + r | 32pp + 16 + 4g + r]
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const bf16x8 vf = tr_pair32(img, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);
          o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o[db], 0, 0, 0);       // D[query 4g+r][d = db*16 + c]
        }
      }
      const float inv_l = 1.f / l;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float il = __shfl(inv_l, 4 * g + r, 64);             // 1/l of query 4g+r (held by the lanes with c == 4g+r)
        const int tq = __shfl(tok, qb * 16 + 4 * g + r, 64);       // rows >= T (tok < 0) store nothing
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const float v = o[db][r] * il;
          const float vn = __shfl_xor(v, 1, 64);
          if ((c & 1) == 0 && tq >= 0) *(unsigned int*)(out + (long long)tq * ldo + h * WD + db * 16 + c) = pack_bf16x2(v, vn);
        }
      }
    }
    __syncthreads();                                   // the images are rewritten by the next window
  }
}

// ----------------------------------------------------------------------------------------------------------------
// backward: dQ, dK, dV of every (window, head) pair and one dbias partial per workgroup
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WTHREADS) void winattn_bwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                               const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                               const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                                                               float* __restrict__ part, WinGeom G, int nwin, float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char imgs[WWAVES][3][WIMG];   // per wave: K | Q | dO (each read transposed)
  __shared__ float sb[64 * 64];
  __shared__ __attribute__((aligned(16))) float s_lq[WWAVES][64], s_dl[WWAVES][64];   // lse * log2(e) (+inf: no such query), delta
  __shared__ __attribute__((aligned(16))) int s_rid[WWAVES][64];
  const int h = blockIdx.y, T = G.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  for (int i = threadIdx.x; i < T * T; i += WTHREADS) sb[i] = bias[(long long)h * T * T + i];
  const long long ld = 3ll * G.H * WD, ldo = (long long)G.H * WD;
  const bf16_t* qbase = qkv + h * WD;
  const bf16_t* kbase = qbase + G.H * WD;
  const bf16_t* vbase = qbase + 2 * G.H * WD;
  const bf16_t* obase = out + h * WD;
  const bf16_t* dobase = dout + h * WD;
  const int stride = gridDim.x * WWAVES;
  const int iters = (nwin + stride - 1) / stride;
  unsigned char* Kimg = imgs[wave][0];
  unsigned char* Qimg = imgs[wave][1];
  unsigned char* Dimg = imgs[wave][2];
  f32x4 acc[4][4];                                     // sum of dS^T over this wave's windows: [query block][key block]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; ++it) {
    const int wi = (it * gridDim.x + blockIdx.x) * WWAVES + wave;
    const bool live = wi < nwin;
    int tok = -1, rid = 0;
    if (live) win_token(G, wi, lane, tok, rid);
    stage_image(Kimg, kbase, ld, tok, lane);
    stage_image(Qimg, qbase, ld, tok, lane);
    stage_image(Dimg, dobase, ldo, tok, lane);
    s_rid[wave][lane] = rid;
    s_lq[wave][lane] = (live && lane < T) ? lse[((long long)wi * G.H + h) * T + lane] * LOG2E : INFINITY;
    bf16x8 kf[4], vf[4], qf[4], dof[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int tk = __shfl(tok, b * 16 + c, 64);      // the token of slot b*16 + c, as key and as query
      kf[b] = load_frag(kbase, ld, tk, g);
      vf[b] = load_frag(vbase, ld, tk, g);
      qf[b] = load_frag(qbase, ld, tk, g);
      dof[b] = load_frag(dobase, ldo, tk, g);
      const bf16x8 of = load_frag(obase, ldo, tk, g);
      float dl = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) dl += bf16_to_f32((bf16_t)dof[b][j]) * bf16_to_f32((bf16_t)of[j]);
      dl = group_sum(dl);                              // delta = rowsum(dO * O)
      if (g == 0) s_dl[wave][b * 16 + c] = dl;
    }
    __syncthreads();
    // ---- query on the lane: dS^T -> dbias and dQ
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      if (qb * 16 < T) {
        const int q = qb * 16 + c;
        const float lq = s_lq[wave][q], dl = s_dl[wave][q];
        const int ridq = s_rid[wave][q];
        f32x4 ds[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb], qf[qb], z, 0, 0, 0);     // S^T[key 4g+r][query c]
          const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[kb], dof[qb], z, 0, 0, 0);   // dP^T
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kb * 16 + 4 * g + r;
            const bool pair = key < T && q < T;
            const float bv = pair ? sb[q * T + key] : 0.f;
            const float mk = s_rid[wave][key] != ridq ? -100.f : 0.f;
            const float sc = __builtin_fmaf(s[r], scale, bv + mk);
            const float p = key < T ? __builtin_amdgcn_exp2f(__builtin_fmaf(sc, LOG2E, -lq)) : 0.f;
            ds[kb][r] = p * (dp[r] - dl);
            acc[qb][kb][r] += ds[kb][r];
          }
        }
        f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          const bf16x8 dsf = pack_acc2(ds[2 * pp], ds[2 * pp + 1]);
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const bf16x8 ktf = tr_pair32(Kimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);   // A[d = db*16 + c][keys]
            dq[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ktf, dsf, dq[db], 0, 0, 0);           // D[d 4g+r][query c]
          }
        }
        const int tq = __shfl(tok, q, 64);
        if (tq >= 0) {
          bf16_t* dst = dqkv + (long long)tq * ld + h * WD;
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            u32x2 pk;
            pk[0] = pack_bf16x2(dq[db][0] * scale, dq[db][1] * scale);
            pk[1] = pack_bf16x2(dq[db][2] * scale, dq[db][3] * scale);
            *(u32x2*)(dst + db * 16 + 4 * g) = pk;
          }
        }
      }
    }
    // ---- key on the lane: dK and dV
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb * 16 < T) {
        const int key = kb * 16 + c;
        const int ridk = s_rid[wave][key];
        f32x4 dk[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        f32x4 dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          f32x4 p2[2], ds2[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int qb = 2 * pp + u;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[qb], kf[kb], z, 0, 0, 0);     // S[query 4g+r][key c]
            const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof[qb], vf[kb], z, 0, 0, 0);   // dP
            const f32x4 l4 = *(const f32x4*)&s_lq[wave][qb * 16 + 4 * g];
            const f32x4 d4 = *(const f32x4*)&s_dl[wave][qb * 16 + 4 * g];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int q = qb * 16 + 4 * g + r;
              const bool pair = key < T && q < T;
              const float bv = pair ? sb[q * T + key] : 0.f;
              const float mk = s_rid[wave][q] != ridk ? -100.f : 0.f;
              const float sc = __builtin_fmaf(s[r], scale, bv + mk);
              const float p = key < T ? __builtin_amdgcn_exp2f(__builtin_fmaf(sc, LOG2E, -l4[r])) : 0.f;
              p2[u][r] = p;
              ds2[u][r] = p * (dp[r] - d4[r]);
            }
          }
          const bf16x8 pf = pack_acc2(p2[0], p2[1]);     // B[k = queries 32pp + 4g + r | 32pp + 16 + 4g + r][col = key c]
          const bf16x8 dsf = pack_acc2(ds2[0], ds2[1]);
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const bf16x8 dotf = tr_pair32(Dimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);   // A[d][queries] = dO^T
            const bf16x8 qtf = tr_pair32(Qimg, 32 * pp + 4 * g, 32 * pp + 16 + 4 * g, db, lane);    // A[d][queries] = Q^T
            dv[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dotf, pf, dv[db], 0, 0, 0);            // dV^T[d 4g+r][key c]
            dk[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qtf, dsf, dk[db], 0, 0, 0);            // dK^T[d 4g+r][key c]
          }
        }
        const int tk = __shfl(tok, key, 64);
        if (tk >= 0) {
          bf16_t* dstk = dqkv + (long long)tk * ld + (long long)G.H * WD + h * WD;
          bf16_t* dstv = dqkv + (long long)tk * ld + 2ll * G.H * WD + h * WD;
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
      }
    }
    __syncthreads();                                   // the images and row vectors are rewritten by the next window
  }
  // fold the four waves in wave order (the images are dead: the fold buffer takes their place), one partial per workgroup
  float* red = (float*)&imgs[0][0][0];                 // [64][64]
#pragma unroll 1
  for (int w = 0; w < WWAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int qb = 0; qb < 4; ++qb)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          float* p = red + (qb * 16 + c) * 64 + kb * 16 + 4 * g;
          f32x4 v = acc[qb][kb];
          if (w > 0) {
            const f32x4 o = *(const f32x4*)p;
            v = o + v;
          }
          *(f32x4*)p = v;
        }
    }
    __syncthreads();
  }
  float* dst = part + ((long long)blockIdx.x * G.H + h) * T * T;
  for (int i = threadIdx.x; i < T * T; i += WTHREADS) {
    const int q = i / T, key = i - q * T;
    dst[i] = red[q * 64 + key];
  }
}

// dbias[i] (+)= sum over the P partials, in order
__global__ __launch_bounds__(256) void winattn_dbias_fold_kernel(const float* __restrict__ part, float* __restrict__ dbias, int n,
                                                                 int P, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[(long long)p * n + i];
  dbias[i] = accumulate ? dbias[i] + s : s;
}

// ----------------------------------------------------------------------------------------------------------------
// relative-position bias: bias[h][i][j] = table[index(i, j)][h], index = (dr + ws - 1) (2 ws - 1) + (dc + ws - 1) with
// (dr, dc) = coordinates of i minus coordinates of j (timm's relative_position_index)
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relpos_gather_kernel(const float* __restrict__ table, float* __restrict__ bias, int H, int ws) {
  const int T = ws * ws, n = H * T * T;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int h = idx / (T * T), ij = idx - h * T * T;
  const int i = ij / T, j = ij - i * T;
  const int dr = i / ws - j / ws, dc = i % ws - j % ws;
  const int e = (dr + ws - 1) * (2 * ws - 1) + dc + ws - 1;
  bias[idx] = table[e * H + h];
}

// the transpose of the gather: entry (e, h) sums the pairs (i, j) that map to it; each i has at most one such j, so walking i
// upwards is the increasing (i, j) order
__global__ __launch_bounds__(256) void relpos_scatter_kernel(const float* __restrict__ dbias, float* __restrict__ dtable, int H, int ws,
                                                             int accumulate) {
  const int T = ws * ws, L = 2 * ws - 1, n = L * L * H;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int e = idx / H, h = idx - e * H;
  const int dr = e / L - (ws - 1), dc = e % L - (ws - 1);
  float s = 0.f;
  for (int i = 0; i < T; ++i) {
    const int jr = i / ws - dr, jc = i % ws - dc;
    if (jr >= 0 && jr < ws && jc >= 0 && jc < ws) s += dbias[((long long)h * T + i) * T + jr * ws + jc];
  }
  dtable[idx] = accumulate ? dtable[idx] + s : s;
}

// ----------------------------------------------------------------------------------------------------------------
// patch merging + LayerNorm(4C): one wave per output row; the row's 4C values (at most 2048: four 16 B vectors per lane) live in
// registers between the gather and the store, so the gathered tensor is never stored un-normalised.  Channel block
// j = 2 (w parity) + (h parity) of output pixel (r, c) is x[n][2r + hpar][2c + wpar][:]  (timm: x0 | x1 | x2 | x3).
// ----------------------------------------------------------------------------------------------------------------
constexpr int PM_MAX_C4 = 2048;

struct PmRow { long long base; int W, C; };   // x offset of pixel (2r, 2c) of the row's image
__device__ __forceinline__ PmRow pm_row(long long row, int H, int W, int C) {
  const int W2 = W >> 1, H2 = H >> 1;
  const long long n = row / ((long long)H2 * W2);
  const int rem = (int)(row - n * H2 * W2);
  const int r = rem / W2, c = rem - r * W2;
  return PmRow{((n * H + 2 * r) * W + 2 * c) * C, W, C};
}
// element offset in x of 16 B vector q of the gathered row
__device__ __forceinline__ long long pm_src(const PmRow& R, int q, int cpb) {
  const int j = q / cpb, ci = q - j * cpb;
  return R.base + ((long long)(j & 1) * R.W + (j >> 1)) * R.C + ci * 8;
}
__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = bf16_lo(v[e]); f[2 * e + 1] = bf16_hi(v[e]); }
}

__global__ __launch_bounds__(256) void patch_merge_ln_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                                 float* __restrict__ mean, float* __restrict__ rstd, int H, int W,
                                                                 int C, float eps, long long rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpb = C >> 3, nvec = 4 * cpb, C4 = 4 * C;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
    const PmRow R = pm_row(row, H, W, C);
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = lane + 64 * k;
      if (q < nvec) {
        unpack8(*(const u32x4*)(x + pm_src(R, q, cpb)), v[k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[k][e];
      }
    }
    const float mu = wave_sum(s) / (float)C4;
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (lane + 64 * k < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[k][e] - mu; s2 += d * d; }
      }
    const float rs = 1.0f / sqrtf(wave_sum(s2) / (float)C4 + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = lane + 64 * k;
      if (q < nvec) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ch = q * 8 + 2 * e;
          o[e] = pack_bf16x2((v[k][2 * e] - mu) * rs * gamma[ch] + beta[ch], (v[k][2 * e + 1] - mu) * rs * gamma[ch + 1] + beta[ch + 1]);
        }
        *(u32x4*)(y + row * C4 + q * 8) = o;
      }
    }
  }
}

// backward: xhat is recomputed from x, mean and rstd; dx goes back to its pixel of [N][H][W][C] (every element exactly once); each
// wave keeps its share of dgamma / dbeta in registers over its rows, the four waves are folded in wave order through LDS and the
// workgroup writes one partial [2][4C]
__global__ __launch_bounds__(256) void patch_merge_ln_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, bf16_t* __restrict__ dx,
                                                                 float* __restrict__ part, int H, int W, int C, long long rows) {
  __shared__ float red[2 * PM_MAX_C4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpb = C >> 3, nvec = 4 * cpb, C4 = 4 * C;
  float gam[4][8], dg[4][8], db[4][8];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int q = lane + 64 * k;
      gam[k][e] = q < nvec ? gamma[q * 8 + e] : 0.f;
      dg[k][e] = 0.f;
      db[k][e] = 0.f;
    }
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
    const PmRow R = pm_row(row, H, W, C);
    const float mu = mean[row], rs = rstd[row];
    float xh[4][8], gy[4][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = lane + 64 * k;
      if (q < nvec) {
        float d[8];
        unpack8(*(const u32x4*)(x + pm_src(R, q, cpb)), xh[k]);
        unpack8(*(const u32x4*)(dy + row * C4 + q * 8), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[k][e] = (xh[k][e] - mu) * rs;
          dg[k][e] += d[e] * xh[k][e];
          db[k][e] += d[e];
          gy[k][e] = d[e] * gam[k][e];
          s1 += gy[k][e];
          s2 += gy[k][e] * xh[k][e];
        }
      }
    }
    const float m1 = wave_sum(s1) / (float)C4, m2 = wave_sum(s2) / (float)C4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = lane + 64 * k;
      if (q < nvec) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = pack_bf16x2(rs * (gy[k][2 * e] - m1 - xh[k][2 * e] * m2), rs * (gy[k][2 * e + 1] - m1 - xh[k][2 * e + 1] * m2));
        *(u32x4*)(dx + pm_src(R, q, cpb)) = o;
      }
    }
  }
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = lane + 64 * k;
        if (q < nvec) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ch = q * 8 + e;
            red[ch] = w > 0 ? red[ch] + dg[k][e] : dg[k][e];
            red[C4 + ch] = w > 0 ? red[C4 + ch] + db[k][e] : db[k][e];
          }
        }
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 2 * C4; i += 256) part[(long long)blockIdx.x * 2 * C4 + i] = red[i];
}

// dgamma | dbeta (+)= sum over the P partial rows [2][C4], in order
__global__ __launch_bounds__(256) void patch_merge_ln_fold_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, int C4, int P, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * C4) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[(long long)p * 2 * C4 + i];
  float* dst = i < C4 ? dgamma + i : dbeta + (i - C4);
  *dst = accumulate ? *dst + s : s;
}

WinGeom make_geom(int Hs, int Ws, int H, int ws, int shift) {
  WinGeom G;
  G.Hs = Hs; G.Ws = Ws; G.ws = ws; G.shift = shift;
  G.nWc = Ws / ws; G.nW = (Hs / ws) * G.nWc; G.T = ws * ws; G.H = H;
  return G;
}

int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

// 12 x 12 windows (T = 144: nine MFMA blocks per side) run on the kernels of window_attention_w12.hip
constexpr int WS12 = 12;

bool icamd_window_attention_ok(int Hs, int Ws, int ws, int D) {
  return D == WD && ((ws >= 2 && ws <= 8) || ws == WS12) && Hs > 0 && Ws > 0 && Hs % ws == 0 && Ws % ws == 0;
}

// workgroups per head of the backward (= dbias partials per head): a function of the problem shape only
int icamd_window_attention_bwd_chunks(long long nwin, int H, int ws) {
  if (ws == WS12) return icamd_window_attention_w12_bwd_chunks(nwin, H);
  const long long by_windows = (nwin + WWAVES - 1) / WWAVES;
  const long long cap = 1024 / H > 1 ? 1024 / H : 1;
  return (int)(by_windows < cap ? by_windows : cap);
}

int icamd_window_attention_fwd_launch(const bf16_t* qkv, const float* bias, bf16_t* out, float* lse, int B, int Hs, int Ws, int H,
                                      int ws, int shift, float scale, hipStream_t s) {
  if (ws == WS12) return icamd_window_attention_w12_fwd_launch(qkv, bias, out, lse, B, Hs, Ws, H, shift, scale, s);
  const WinGeom G = make_geom(Hs, Ws, H, ws, shift);
  const long long nwin = (long long)B * G.nW;
  const long long by_windows = (nwin + WWAVES - 1) / WWAVES;
  const long long cap = 2048 / H > 1 ? 2048 / H : 1;
  const dim3 grid((unsigned)(by_windows < cap ? by_windows : cap), (unsigned)H);
  hipLaunchKernelGGL(winattn_fwd_kernel, grid, dim3(WTHREADS), 0, s, qkv, bias, out, lse, G, (int)nwin, scale);
  return icamd_launch_status();
}

int icamd_window_attention_bwd_launch(const bf16_t* qkv, const float* bias, const bf16_t* out, const bf16_t* dout, const float* lse,
                                      bf16_t* dqkv, float* dbias, int accumulate, float* part, int B, int Hs, int Ws, int H, int ws,
                                      int shift, float scale, hipStream_t s) {
  if (ws == WS12)
    return icamd_window_attention_w12_bwd_launch(qkv, bias, out, dout, lse, dqkv, dbias, accumulate, part, B, Hs, Ws, H, shift, scale, s);
  const WinGeom G = make_geom(Hs, Ws, H, ws, shift);
  const long long nwin = (long long)B * G.nW;
  const int P = icamd_window_attention_bwd_chunks(nwin, H, ws);
  hipLaunchKernelGGL(winattn_bwd_kernel, dim3((unsigned)P, (unsigned)H), dim3(WTHREADS), 0, s, qkv, bias, out, dout, lse, dqkv, part, G,
                     (int)nwin, scale);
  const int n = H * G.T * G.T;
  hipLaunchKernelGGL(winattn_dbias_fold_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, part, dbias, n, P, accumulate);
  return icamd_launch_status();
}

int icamd_relpos_bias_gather_launch(const float* table, float* bias, int H, int ws, hipStream_t s) {
  const int n = H * ws * ws * ws * ws;
  hipLaunchKernelGGL(relpos_gather_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, table, bias, H, ws);
  return icamd_launch_status();
}

int icamd_relpos_bias_scatter_launch(const float* dbias, float* dtable, int H, int ws, int accumulate, hipStream_t s) {
  const int n = (2 * ws - 1) * (2 * ws - 1) * H;
  hipLaunchKernelGGL(relpos_scatter_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, dbias, dtable, H, ws, accumulate);
  return icamd_launch_status();
}

bool icamd_patch_merge_ln_ok(int N, int H, int W, int C) {
  return N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0 && 4 * C <= PM_MAX_C4;
}

int icamd_patch_merge_ln_bwd_blocks(long long rows) {
  const long long b = (rows + 3) / 4;
  return (int)(b < 512 ? b : 512);
}

int icamd_patch_merge_ln_fwd_launch(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                                    int N, int H, int W, int C, float eps, hipStream_t s) {
  const long long rows = (long long)N * (H / 2) * (W / 2);
  long long blocks = (rows + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(patch_merge_ln_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, gamma, beta, y, mean, rstd, H, W, C, eps,
                     rows);
  return icamd_launch_status();
}

int icamd_patch_merge_ln_bwd_launch(const bf16_t* dy, const bf16_t* x, const float* mean, const float* rstd, const float* gamma,
                                    bf16_t* dx, float* dgamma, float* dbeta, int N, int H, int W, int C, int accumulate, float* part,
                                    hipStream_t s) {
  const long long rows = (long long)N * (H / 2) * (W / 2);
  const int P = icamd_patch_merge_ln_bwd_blocks(rows);
  hipLaunchKernelGGL(patch_merge_ln_bwd_kernel, dim3((unsigned)P), dim3(256), 0, s, dy, x, mean, rstd, gamma, dx, part, H, W, C, rows);
  hipLaunchKernelGGL(patch_merge_ln_fold_kernel, dim3((unsigned)ceil_div(8 * C, 256)), dim3(256), 0, s, part, dgamma, dbeta, 4 * C, P,
                     accumulate);
  return icamd_launch_status();
}
