// Internal launch-parameter blocks and launcher prototypes shared between the C-ABI layer (the capi*.hip units) and the kernels.
// Every launcher is declared here and nowhere else; the defining unit includes this header, and the library is linked with
// -z defs, so a declaration that drifts from its definition fails the build.
#pragma once
#include "common.h"

#define ICAMD_MAX_TAPS 56

// One implicit-GEMM problem: out[n, p*ostr+ooff_h, q*ostr+ooff_w, :] = sum over active taps t, ci of
//   in[n, p*istr+dh[t], q*istr+dw[t], ci] * wt[co][wtap[t]][ci]        (+ bias[co] + addend[same pixel])
struct IgemmParams {
  const bf16_t* in;
  const bf16_t* wt;
  bf16_t* out;
  const bf16_t* addend;  // optional, laid out like out
  const unsigned char* addend_bits;  // optional 1 bit per addend element: the addend counts only where its bit is set
  int addend_sub2;       // 1: addend is [N][ceil(OH/2)][ceil(OW/2)][Cout], added at even (oh, ow) only; others get none
  const float* bias;     // optional [Cout]
  float* stats;          // optional [ceil(M/128)][2][Cout] partial sum / sum-of-squares of rounded outputs
  // fused BatchNorm-backward pass 1 (data-gradient launches only; enabled by bnb_y != nullptr)
  const bf16_t* bnb_y;     // BN input (conv output) of the layer whose output gradient this launch produces
  const bf16_t* bnb_mask;  // post-activation tensor for the ReLU mask, or nullptr: mask = bnb_y*scale+shift > 0
  const float *bnb_mean, *bnb_invstd, *bnb_scale, *bnb_shift;
  int bnb_relu;
  int relu;              // EPI 0 only: clamp the sum at zero before rounding (inference epilogue)
  bf16_t* gelu_out;      // EPI 0, optional second output laid out like out: gelu(rounded out)   (Mlp fc1 forward)
  int gelu_inplace;      // EPI 0: out itself receives gelu(rounded result) (forward passes that keep nothing for backward)
  const bf16_t* gelu_z;  // EPI 0, optional, laid out like out: out = rounded result * gelu'(gelu_z)  (Mlp fc2 data gradient)
  int N, IH, IW, Cin;
  int OH, OW, Cout;
  int P, Q, M;           // output sub-grid and row count N*P*Q
  int ostr, ooff_h, ooff_w, istr;
  int ntaps, Ktot;       // active taps; filter row length (elements)
  int KW, pad;           // regular-tap rule of the general (Cin % 64 != 0) path: dh = tap_sign*(r - pad)
  int tap_sign, regular_taps;
  int stem7;             // ResNet stem on the rgb4 layout (conv_igemm.hip KMODE 3)
  int ksteps, ntiles_n;  // filled by the launcher
  FastDiv divPQ, divQ, divCin, divKW;   // filled by the launcher
  short dh[ICAMD_MAX_TAPS], dw[ICAMD_MAX_TAPS], wtap[ICAMD_MAX_TAPS];
};
int icamd_igemm_launch(IgemmParams& p, hipStream_t stream);
int icamd_igemm_pick_bn(int Cout);

// 3x3 / stride 1 / pad 1 convolution, input tile staged once per 64-channel slice (conv3x3_halo.hip)
struct Halo3x3Params {
  const bf16_t* in;      // [N][H][W][C]
  const bf16_t* wt;      // [Cout][3][3][C]
  bf16_t* out;           // [N][H][W][Cout]
  const float* bias;     // optional [Cout]
  float* stats;          // optional [ceil(M/128)][2][Cout]
  int relu;
  int flip;              // 1: mirrored taps (data gradient with the transposed filter)
  int N, H, W, C, Cout;
  int M, ntiles_n;       // filled by the launcher
  FastDiv divHW, divW;
};
bool icamd_halo3x3_wanted(int N, int H, int W, int C, int Cout);
int icamd_halo3x3_launch(Halo3x3Params& p, hipStream_t stream);

// Grouped 3x3 / pad 1 / stride 1 or 2 convolution, Cin == Cout == C, C / groups in {4, 8, 16, 32} (conv_grouped.hip)
struct GConvParams {
  const bf16_t* in;      // forward / weight gradient: x [N][IH][IW][C]; data gradient: dy [N][OH][OW][C]
  const bf16_t* w;       // [C][3][3][Cg], the forward layout for every launch
  bf16_t* out;           // forward: y; data gradient: dx
  const bf16_t* dy;      // weight gradient only
  float* slab;           // weight gradient: [S][C][3][3][Cg] partial sums
  const float* bias;     // optional [C] (forward)
  float* stats;          // optional [ceil(M/128)][2][C] (forward)
  int relu;
  int N, IH, IW, OH, OW, C, groups, stride;
  int Cg, M, npix_in, nalloc;          // filled by the launcher
  int S, tiles_per_split, ntiles;      // filled by the launcher (weight gradient)
  FastDiv divOHW, divOW;
};
bool icamd_gconv3x3_ok(int N, int IH, int IW, int OH, int OW, int C, int groups, int stride);
int icamd_gconv3x3_fwd_launch(GConvParams& p, hipStream_t stream);
int icamd_gconv3x3_dgrad_launch(GConvParams& p, hipStream_t stream);
size_t icamd_gconv3x3_wgrad_bytes(int N, int IH, int IW, int OH, int OW, int C, int groups, int stride);
int icamd_gconv3x3_wgrad_launch(GConvParams& p, hipStream_t stream);   // fills p.S; the caller folds the slabs

// 2x2 / stride 2 average pool, ceil_mode, count_include_pad=False, and the thin 3x3 convolution of the deep stem (conv_stem_deep.hip)
struct Pool2x2Params {
  const bf16_t* in;      // forward: x [N][IH][IW][C]; backward: dout [N][OH][OW][C]
  const bf16_t* addend;  // backward, optional: [N][IH][IW][C]
  bf16_t* out;           // forward: [N][OH][OW][C]; backward: dx [N][IH][IW][C]
  int N, IH, IW, C8;     // C8 = C / 8
  int OH, OW;            // filled by the launcher
  unsigned int total;
  FastDiv divC8, divOW, divOH;
};
bool icamd_avgpool2x2_ok(int N, int IH, int IW, int C);
int icamd_avgpool2x2_launch(Pool2x2Params& p, int backward, hipStream_t stream);

struct ThinConvParams {
  const bf16_t* in;      // forward / weight gradient: x [N][H][W][32]; data gradient: dy [N][H][W][Cout]
  const bf16_t* w;       // [Cout][3][3][32], the forward layout for every launch
  bf16_t* out;           // forward: y [N][H][W][Cout]; data gradient: dx [N][H][W][32]
  const bf16_t* dy;      // weight gradient only
  float* slab;           // weight gradient: [S][Cout][3][3][32] partial sums
  const float* bias;     // optional [Cout] (forward)
  float* stats;          // optional [icamd_thin3x3_stats_rows][2][Cout] (forward)
  int relu;
  int N, H, W, Cout;
  int M, nalloc, ntiles;               // filled by the launcher
  int S, tiles_per_split;              // filled by the launcher (weight gradient)
  FastDiv divHW, divW;
};
bool icamd_thin3x3_ok(int N, int H, int W, int Cin, int Cout);
int icamd_thin3x3_stats_rows(int N, int H, int W, int Cout);
int icamd_thin3x3_fwd_launch(ThinConvParams& p, hipStream_t stream);
int icamd_thin3x3_dgrad_launch(ThinConvParams& p, hipStream_t stream);
size_t icamd_thin3x3_wgrad_bytes(int N, int H, int W, int Cout);
int icamd_thin3x3_wgrad_launch(ThinConvParams& p, hipStream_t stream);   // fills p.S; the caller folds the slabs

// Dense NT GEMM for big pointwise problems: out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]) (+ addend[m][n])
struct GemmNtParams {
  const bf16_t* A;       // [M][K]
  const bf16_t* B;       // [N][K]
  bf16_t* out;           // [M][N]
  const bf16_t* addend;  // optional [M][N]
  const unsigned char* addend_bits;   // optional, 1 bit per addend element (full-size addend only): counted where set
  const float* bias;     // optional [N]
  float* stats;          // optional [ceil(M/128)][2][N]: per-channel sum / sum of squares of the rounded outputs, one row
                         // per 256-row tile at row tile_m, zeros in the rows no tile owns
  int M, N, K;
  int sub2_h, sub2_w;    // > 0: rows are pixels of [.][sub2_h][sub2_w]; addend is [.][ceil(h/2)][ceil(w/2)][N], added at even (h, w)
  FastDiv divHW, divW;   // filled by the launcher when sub2_h > 0
  int relu;              // clamp at zero before rounding
  bf16_t* gelu_out;      // optional second output [M][N]: gelu(rounded out)
  int gelu_inplace;      // out itself receives gelu(rounded result)
  const bf16_t* gelu_z;  // optional [M][N]: out = rounded result * gelu'(gelu_z)
  int ntiles_n;          // filled by the launcher
  int group_n;           // 8-phase kernel: n-tiles per group of its tile order (filled by the launcher)
  int out_policy;        // cache policy of the output stores: 0 plain, 1 sc1 (the line leaves the XCD's L2), 2 nt (filled by the launcher)
};
int icamd_gemm_nt_launch(GemmNtParams& p, hipStream_t stream);
// true when the 256x256-tile kernel is expected to beat the 128x128 implicit-GEMM kernel for this problem
bool icamd_gemm_nt_wanted(long long M, int N, int K);

// Pointwise convolution with the filter resident in registers (conv1x1_resident.hip): out[m][n] = sum_k A[m][k] * B[n][k]
struct PwResidentParams {
  const bf16_t* A;       // [M][K]
  const bf16_t* B;       // [N][K]
  bf16_t* out;           // [M][N]
  const bf16_t* addend;  // optional [M][N] (or the even-grid form, see sub2_h)
  const unsigned char* addend_bits;   // optional 1 bit per addend element
  float* stats;          // optional [ceil(M/128)][2][N]; one partial row per workgroup, the other rows zero
  int M, N, K;
  int sub2_h, sub2_w;    // > 0: addend is [.][ceil(h/2)][ceil(w/2)][N], added at even (h, w)
  FastDiv divHW, divW;   // filled by the launcher
  int rows_per_split, ntiles_n;   // filled by the launcher
  int xcd_groups;                 // filled by the launcher: XCD-aware workgroup -> (row range, channel tile) order
  int nt_loads;                   // filled by the launcher: non-temporal LDS-DMA for the activation streams
  // "ext" launches (ConvNeXt's dim-96 Linear layers: K = 96 runs as four 32-wide k-steps, the last one against zero filter
  // columns): A rows are lda elements apart and only Ktrue of the K = 128 staged columns are real
  // "bnred" launches (residual data gradient whose output is the output gradient of the PREVIOUS block's last BatchNorm):
  // the epilogue gates the result with that block's ReLU mask bits, stores g and accumulates sum g and sum g * bn_y per
  // channel into one partial row per workgroup of bn_part[ceil(M/128)][2][N] (other rows zero); the finalize forms
  // sum g * xhat = invstd * (sum g*y - mean * sum g) in fp64
  const bf16_t* bn_y;             // [M][N] raw conv output the BatchNorm normalised
  const unsigned char* bn_bits;   // 1 bit per element: the block output was > 0
  float* bn_part;
  int lda, Ktrue;                 // 0: K
  const float* bias;              // optional [N]
  int relu;                       // inference epilogue (EPI instantiations): out = relu(acc + bias + addend)
  bf16_t* gelu_out;               // optional second output: gelu(rounded out)
  int gelu_inplace;               // out itself receives gelu(rounded result)
  const bf16_t* gelu_z;           // optional [M][N]: out = rounded result * gelu'(gelu_z)
  // round 5, stride-2 pointwise forward (ResNet's projection shortcuts): output row m = (n, oh, ow) of [.][gat_oh][gat_ow] reads
  // input row (n, 2 oh, 2 ow) of [.][gat_ih][gat_iw]; 0: rows are read in order
  int gat_oh, gat_ow, gat_ih, gat_iw;
  FastDiv gdivHW, gdivW;          // filled by the launcher when gat_ow > 0
};
bool icamd_pw_resident_wanted(long long M, int N, int K, bool with_addend = false);
int icamd_pw_resident_mode();   // ICAMD_PW_RESIDENT, read once: 0 = off, 1 = size floors, 2 = no floor, 5 = addend data gradients off
// the ext form: plain pointwise problems with K = 96 (bias / GELU epilogues allowed, no addend / statistics)
bool icamd_pw_resident_ext_wanted(long long M, int N, int K);
int icamd_pw_resident_launch(PwResidentParams& p, hipStream_t stream);
int icamd_pw_resident_ext_launch(PwResidentParams& p, hipStream_t stream);
// the bnred form: full-size addend (optionally gated by its own mask bits), (K, N) in {(64, 256), (128, 512), (256, 1024)}
bool icamd_pw_resident_bnred_wanted(long long M, int N, int K);
int icamd_pw_resident_bnred_launch(PwResidentParams& p, hipStream_t stream);

// ResNet stem forward with the filter resident in registers (conv_stem.hip)
struct StemParams {
  const bf16_t* x;   // [N][H][W+8][4]
  const bf16_t* w;   // [64][8][8][4]
  bf16_t* y;         // [N][OH][OW][64]
  float* stats;      // optional [ceil(M/128)][2][64]
  int N, H, W, OH, OW;
  const float* bias; // optional [64]: inference epilogue (folded BatchNorm shift)
  int relu;
};
struct StemWgradParams {
  const bf16_t* x;   // [N][H][W+8][4]
  const bf16_t* dy;  // [N][OH][OW][64]
  float* slab;       // [S][64][256]
  int N, H, W, OH, OW;
};
bool icamd_stem_resident_wanted(int N, int H, int W, int Cout);
int icamd_stem_wgrad_resident_splits(int N, int H);
int icamd_stem_wgrad_resident_launch(StemWgradParams& p, int S, hipStream_t stream);
int icamd_stem_resident_launch(StemParams& p, hipStream_t stream);

// Fused backward of "pointwise convolution -> BatchNorm" (conv_fused_bwd.hip): BatchNorm-backward apply + data gradient + weight
// gradient of the convolution in one pass over g and y
struct FusedBwdParams {
  const bf16_t* g;      // [M][CO] masked output gradient of the BatchNorm
  const bf16_t* y;      // [M][CO] BatchNorm input (raw convolution output)
  const bf16_t* x;      // [M][CI] convolution input
  const bf16_t* wt;     // [CI][CO] transposed filter
  bf16_t* dx;           // [M][CI]
  float* slab;          // [S][CO][CI] partial filter gradients
  const float *mean, *invstd, *scale, *c1, *c2;   // [CO]: batch statistics, gamma * invstd, mean g, mean g * xhat
  int M, CI, CO;
  int S, rows_per_split, nslices, xcd_pairs, nt;  // filled by the launcher
};
bool icamd_conv1x1_bn_bwd_fused_wanted(long long M, int Cin, int Cout);
void icamd_conv1x1_bn_bwd_fused_plan(int M, int Cin, int* S, int* rows_per_split);
int icamd_conv1x1_bn_bwd_fused_launch(FusedBwdParams& p, hipStream_t stream);

// Fused forward across a bottleneck boundary (conv_fused_fwd.hip): out = relu(y * scale + shift + residual) with its mask bits, and
// y1 = out * w^T (the next block's 1x1 convolution) with that layer's BatchNorm statistics, in one pass
struct FusedFwdParams {
  const bf16_t* y;        // [M][K] raw convolution output the BatchNorm normalises
  const bf16_t* res;      // [M][K] residual: an activation, or (res_scale != nullptr) the raw shortcut convolution output
  const float *scale, *shift, *res_scale, *res_shift;   // [K]
  bf16_t* out;            // [M][K]
  unsigned char* maskbits;   // [M * K / 8]: bit = [out > 0]
  const bf16_t* w;        // [N][K] filter of the next block's conv1
  bf16_t* y1;             // [M][N]
  float* stats;           // optional [ceil(M / 128)][2][N]
  int M, K, N;
  int S, rows_per_split, nt;  // filled by the launcher
};
bool icamd_bn_apply_conv1x1_fused_wanted(long long M, int K, int N);
int icamd_bn_apply_conv1x1_fused_launch(FusedFwdParams& p, hipStream_t stream);

// Weight-gradient problem: dw[co][t][ci] = sum_m dy[m][co] * x[n, p*stride+r-pad, q*stride+s-pad, ci]
struct WgradParams {
  const bf16_t* x;    // [N, IH, IW, Cin]
  const bf16_t* dy;   // [N, OH, OW, Cout]
  float* slab;        // [S][Cout][Ktot] partial sums
  float* bias_slab;   // optional [S][Cout] partial column sums of dy (bias gradient)
  int N, IH, IW, Cin, OH, OW, Cout;
  int KH, KW, stride, pad;
  int M, Ktot;        // N*OH*OW ; KH*KW*Cin
  int S, rows_per_split;  // split of the m reduction
  int ntiles_k, ntiles_c;
  int pointwise;      // 1x1, stride 1, pad 0: the gather is the identity
  int xcd_chunk;      // workgroup order: 1 = contiguous chunks of the split-major list per XCD (conv_wgrad.hip wgrad_block_order)
  int stem7;          // ResNet stem on the rgb4 layout: k = row*32 + pixel*4 + channel, IW = padded pitch, Cin = 4
  FastDiv divHW, divW, divCin, divKW;
};
int icamd_wgrad_launch(WgradParams& p, hipStream_t stream);
void icamd_wgrad_plan(int M, int Cout, int Ktot, int* S, int* rows_per_split);
void icamd_wgrad_tile(long long M, int Ktot, int Cout, int* bmk, int* bnc);
// halo-staged 3x3 / stride 1 weight gradient (conv_wgrad.hip): own pixel split; slab layout as the other kernels
bool icamd_wgrad_halo_wanted(int KH, int KW, int stride, int pad, int H, int W, int Cin, int Cout, long long M);
void icamd_wgrad_halo_plan(int M, int Cin, int Cout, int* S, int* rows_per_split);
int icamd_wgrad_halo_launch(WgradParams& p, hipStream_t stream);   // output-tile sides the launcher will use
// out[i] = (accumulate ? out[i] : 0) + sum over S slabs of slab[s][i], fixed order; n % 4 == 0
int icamd_slab_reduce_launch(const float* slab, float* out, long long n, int S, int accumulate, hipStream_t stream,
                             int stem7_mask = 0);

// BatchNorm, pooling, input packing, BatchNorm folding, partial-row sums (norm_pool.hip)
int icamd_bn_finalize_launch(const float* part, int nrows, int C, double count, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps, float* mean,
                             float* invstd, float* scale, float* shift, double* chunks, hipStream_t s);
int icamd_bn_eval_coeffs_launch(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                float* scale, float* shift, hipStream_t s);
int icamd_bn_apply_launch(const bf16_t* y, const float* scale, const float* shift, const bf16_t* residual, bf16_t* out,
                          unsigned char* maskbits, long long numel, int C, int relu, hipStream_t s,
                          const float* res_scale = nullptr, const float* res_shift = nullptr);
int icamd_bn_bwd_rows_per_block(long long rows, int C);
int icamd_bn_bwd_launch(const bf16_t* dout, const bf16_t* act, const bf16_t* y, const float* mean, const float* invstd,
                        const float* scale, const float* shift, float* dgamma, float* dbeta, bf16_t* dy, bf16_t* gout,
                        const unsigned char* maskbits, long long rows, int C, int relu, int accumulate, float* part,
                        double* chunks, float* c1c2, hipStream_t s, const unsigned char* pool_idx = nullptr,
                        int pool_ih = 0, int pool_iw = 0);
int icamd_bn_bwd_dual_launch(const bf16_t* dout, const unsigned char* maskbits, const bf16_t* yA, const float* meanA,
                             const float* invstdA, const float* scaleA, float* dgammaA, float* dbetaA, bf16_t* dyA,
                             const bf16_t* yB, const float* meanB, const float* invstdB, const float* scaleB, float* dgammaB,
                             float* dbetaB, bf16_t* dyB, long long rows, int C, int accumulate, float* partA, double* chunksA,
                             float* cA, float* partB, double* chunksB, float* cB, hipStream_t s);
int icamd_bn_bwd_apply_launch(const float* part, int nrows, const bf16_t* g, const bf16_t* y, const float* mean,
                              const float* invstd, const float* scale, float* dgamma, float* dbeta, bf16_t* dy,
                              long long rows, int C, int accumulate, double* chunks, float* c1c2, hipStream_t s, int sums_are_gy = 0);
int icamd_bn_bwd_finalize_launch(const float* part, int nrows, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                 long long rows, int C, int accumulate, double* chunks, float* c1c2, hipStream_t s, int sums_are_gy);
int icamd_bn_bwd_reduce_launch(const bf16_t* g, const bf16_t* y, const float* mean, const float* invstd, float* part, long long rows,
                               int C, int* nblk_out, hipStream_t s);
int icamd_maxpool_fwd_launch(const bf16_t* x, bf16_t* out, unsigned char* idx, int N, int IH, int IW, int C, int OH, int OW,
                             hipStream_t s);
int icamd_bn_relu_maxpool_fwd_launch(const bf16_t* y, const float* scale, const float* shift, bf16_t* out, unsigned char* idx,
                                     int N, int IH, int IW, int C, int OH, int OW, hipStream_t s);
int icamd_maxpool_bwd_launch(const bf16_t* dout, const unsigned char* idx, bf16_t* dx, int N, int IH, int IW, int C, int OH,
                             int OW, hipStream_t s);
int icamd_avgpool_fwd_launch(const bf16_t* x, bf16_t* out, int N, int HW, int C, hipStream_t s);
int icamd_avgpool_bwd_launch(const bf16_t* dout, bf16_t* dx, int N, int HW, int C, hipStream_t s);
int icamd_pack_input_launch(const float* x, bf16_t* out, int B, int Cin, int H, int W, int mode, float lam, int yl, int yh,
                            int xl, int xh, hipStream_t s);
int icamd_pack_input_rgb4_launch(const float* x, bf16_t* out, int B, int Cin, int H, int W, int mode, float lam, int yl,
                                 int yh, int xl, int xh, hipStream_t s);
int icamd_bn_fold_launch(const float* w, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                         int Cout, int K, bf16_t* w_folded, float* shift, hipStream_t s);
int icamd_sum_partials_launch(const float* part, int nrows, int C, float* out1, float* out2, int accumulate, double* chunks,
                              float* c1c2, hipStream_t s);

// squeeze-and-excitation tail (se_ops.hip)
bool icamd_se_shape_ok(int N, int HW, int C, int rd);
size_t icamd_se_squeeze_bytes(int N, int HW, int C);
int icamd_se_squeeze_launch(const bf16_t* y, float* ysum, int N, int HW, int C, float* part, hipStream_t s);
int icamd_se_excite_fwd_launch(const float* ysum, const float* scale, const float* shift, float inv_hw, const float* w1,
                               const float* b1, const float* w2, const float* b2, float* s_out, float* h_out, float* e_out,
                               int N, int C, int rd, hipStream_t s);
int icamd_se_bn_apply_launch(const bf16_t* y, const float* scale, const float* shift, const float* gate, const bf16_t* residual,
                             const float* res_scale, const float* res_shift, bf16_t* out, unsigned char* maskbits, int N, int HW,
                             int C, int relu, hipStream_t s);
size_t icamd_se_bn_bwd_bytes(int N, int HW, int C);
int icamd_se_bn_bwd_launch(const bf16_t* dout, const unsigned char* maskbits, const bf16_t* y, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, const float* ysum, const float* sv,
                           const float* h, const float* e, const float* w1, const float* w2, float* dgamma, float* dbeta,
                           float* dw1, float* db1, float* dw2, float* db2, bf16_t* dy, int N, int HW, int C, int rd,
                           int accumulate, void* workspace, hipStream_t s);

// loss, step metrics, optimizers, filter preparation, column sums (loss_optim.hip)
int icamd_softmax_xent_launch(const bf16_t* logits, int ld, int B, int C, const long long* y1, const long long* y2,
                              float lam, float smoothing, float gscale, float* loss_rows, int* pred, bf16_t* dlogits,
                              hipStream_t s);
int icamd_step_metrics_launch(const float* loss_rows, const int* pred, const long long* target, int B, int C,
                              float* loss_out, int* finite_out, double* acc_f64, int* counts, float* loss_log,
                              int log_slot, int log_stride, int respect_skip, hipStream_t s);
int icamd_grad_norm_launch(const float* g, long long n, float inv_scale, float max_norm, double* partial, float* out,
                           hipStream_t s);
int icamd_adamw_ema_launch(float* p, float* g, float* m, float* v, float* ema, bf16_t* shadow, long long n, float lr,
                           float wd, float beta1, float beta2, float eps, int step, float gscale, float ema_decay,
                           const float* clip, const int* finite_flag, int* skipped, int zero_grad, hipStream_t s);
int icamd_optim_ema_launch(int kind, float* p, float* g, float* m, float* v, float* ema, bf16_t* shadow, long long n,
                           float lr, float wd, float beta1, float beta2, float eps, int step, float gscale,
                           float ema_decay, const float* clip, const int* finite_flag, int* skipped, int zero_grad,
                           hipStream_t s);
int icamd_grad_guard_launch(float* g, long long n, const int* finite_flag, hipStream_t s);
int icamd_lerp_launch(float* dst, const float* src, long long n, float w, const int* finite_flag, hipStream_t s);
int icamd_f32_to_bf16_launch(const float* src, bf16_t* dst, long long n, hipStream_t s);
int icamd_filter_transpose_launch(const bf16_t* src_base, bf16_t* dst_base, const long long* descs, const int* jobs,
                                  int njobs, hipStream_t s);
int icamd_filter_transpose_tiled_launch(const bf16_t* src_base, bf16_t* dst_base, const long long* descs, const int* jobs,
                                        int njobs, hipStream_t s);
int icamd_colsum_launch(const bf16_t* x, int rows, int ld, int cols, float* out, int accumulate, hipStream_t s);

// LayerNorm, GELU, ViT tokens, row / batch reductions and copies (token_ops.hip)
int icamd_layernorm_fwd_launch(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                               long long rows, int C, float eps, hipStream_t s);
int icamd_layernorm_bwd_blocks(long long rows);
int icamd_layernorm_bwd_launch(const bf16_t* dy, const bf16_t* x, const float* mean, const float* rstd, const float* gamma,
                               const bf16_t* addend, bf16_t* dx, float* part, long long rows, int C, hipStream_t s);
int icamd_vit_tokens_fwd_launch(const bf16_t* patches, const float* cls, const float* pos, bf16_t* tok, int B, int T, int C,
                                hipStream_t s);
int icamd_batch_sum_launch(const bf16_t* x, long long stride, int B, long long n, float* out, int accumulate, hipStream_t s);
int icamd_strided_rows_copy_launch(const bf16_t* src, long long sstride, bf16_t* dst, long long dstride, long long rows,
                                   long long C, hipStream_t s);
int icamd_gelu_fwd_launch(const bf16_t* z, bf16_t* a, long long numel, hipStream_t s);
int icamd_gelu_bwd_launch(const bf16_t* da, const bf16_t* z, bf16_t* dz, long long numel, hipStream_t s);
int icamd_colsum_blocks(long long rows);
int icamd_colsum_partial_launch(const bf16_t* x, float* part, long long rows, int ld, int cols, hipStream_t s);

// ViT attention (attention.hip; sequences past its limit go on to attention_long.hip, see attention_common.h)
int icamd_attention_fwd_launch(const bf16_t* qkv, bf16_t* out, float* lse, int B, int T, int H, float scale, hipStream_t s);
int icamd_attention_bwd_launch(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, float* delta,
                               bf16_t* dqkv, int B, int T, int H, float scale, hipStream_t s);

// Swin: window attention, relative-position bias, patch merging (window_attention.hip)
bool icamd_window_attention_ok(int Hs, int Ws, int ws, int D);
int icamd_window_attention_bwd_chunks(long long nwin, int H, int ws);
int icamd_window_attention_fwd_launch(const bf16_t* qkv, const float* bias, bf16_t* out, float* lse, int B, int Hs, int Ws, int H,
                                      int ws, int shift, float scale, hipStream_t s);
int icamd_window_attention_bwd_launch(const bf16_t* qkv, const float* bias, const bf16_t* out, const bf16_t* dout, const float* lse,
                                      bf16_t* dqkv, float* dbias, int accumulate, float* part, int B, int Hs, int Ws, int H, int ws,
                                      int shift, float scale, hipStream_t s);
int icamd_relpos_bias_gather_launch(const float* table, float* bias, int H, int ws, hipStream_t s);
int icamd_relpos_bias_scatter_launch(const float* dbias, float* dtable, int H, int ws, int accumulate, hipStream_t s);
bool icamd_patch_merge_ln_ok(int N, int H, int W, int C);
int icamd_patch_merge_ln_bwd_blocks(long long rows);
int icamd_patch_merge_ln_fwd_launch(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                                    int N, int H, int W, int C, float eps, hipStream_t s);
int icamd_patch_merge_ln_bwd_launch(const bf16_t* dy, const bf16_t* x, const float* mean, const float* rstd, const float* gamma,
                                    bf16_t* dx, float* dgamma, float* dbeta, int N, int H, int W, int C, int accumulate, float* part,
                                    hipStream_t s);

// 12 x 12 windows (window_attention_w12.hip), reached through the launchers above
int icamd_window_attention_w12_bwd_chunks(long long nwin, int H);
int icamd_window_attention_w12_fwd_launch(const bf16_t* qkv, const float* bias, bf16_t* out, float* lse, int B, int Hs, int Ws, int H,
                                          int shift, float scale, hipStream_t s);
int icamd_window_attention_w12_bwd_launch(const bf16_t* qkv, const float* bias, const bf16_t* out, const bf16_t* dout,
                                          const float* lse, bf16_t* dqkv, float* dbias, int accumulate, float* part, int B, int Hs,
                                          int Ws, int H, int shift, float scale, hipStream_t s);

// ConvNeXt: depthwise 7x7, layer scale / stochastic depth (dwconv.hip)
int icamd_dwconv7_launch(const bf16_t* x, const bf16_t* w, const float* bias, const bf16_t* addend, bf16_t* y, int N, int H,
                         int W, int C, int flip, hipStream_t s);
bool icamd_dwconv7_ok(int N, int H, int W, int C);   // C % 32 == 0, or C % 8 == 0 where the register-window kernels run
int icamd_dwconv7_wgrad_blocks(int N, int H, int W, int C);
int icamd_dwconv7_wgrad_launch(const bf16_t* x, const bf16_t* dy, float* part, float* dw, float* dbias, int N, int H, int W, int C,
                               int accumulate, hipStream_t s);
bool icamd_dwconv7_wgrad_bias_supported_cxx(int N, int H, int W, int C);
int icamd_layerscale_fwd_launch(const bf16_t* z, const bf16_t* inp, const float* gamma, const float* keep, bf16_t* out,
                                long long rows, int C, long long rows_per_image, hipStream_t s);
int icamd_layerscale_bwd_blocks(long long rows);
int icamd_layerscale_fold_launch(const float* params, bf16_t* shadow, float* fold_bias, const long long* jobs, int njobs,
                                 int total_rows, hipStream_t s);
int icamd_rows_fix_launch(const float* keep, int n_images, void* dst1, const void* src1, long long bytes1, void* dst2,
                          long long bytes2, hipStream_t s);
int icamd_dropped_colsum_launch(const bf16_t* dy, const float* keep, int n_images, long long rows_per_image, int C, float* partial,
                                hipStream_t s);
int icamd_layerscale_param_grads_launch(const float* G, const float* w, const float* bias, const float* gamma,
                                        const float* colsum_all, const float* dropped, int n_images, float cb, int C, int K,
                                        float* dw, float* dbias, float* dgamma, int accumulate, hipStream_t s);
int icamd_layerscale_bwd_launch(const bf16_t* dout, const bf16_t* z, const float* gamma, const float* keep, bf16_t* dz,
                                float* part, long long rows, int C, long long rows_per_image, hipStream_t s);

// MobileNet class: depthwise 3x3 (pad 1, stride 1 / 2) and BatchNorm + ReLU6 (dwconv3x3.hip)
bool icamd_dwconv3_ok(int N, int H, int W, int C, int stride);   // C % 8 == 0, stride 1 or 2, grids below 2^31 workgroups
long long icamd_dwconv3_stats_rows_cxx(int N, int H, int W, int C, int stride);
long long icamd_dwconv3_wgrad_rows(int N, int H, int W, int C, int stride);
int icamd_dwconv3_fwd_launch(const bf16_t* x, const float* in_scale, const float* in_shift, const bf16_t* w, bf16_t* y, float* stats,
                             int N, int H, int W, int C, int stride, int flip, hipStream_t s);
int icamd_dwconv3_dgrad_launch(const bf16_t* dy, const bf16_t* w, bf16_t* dx, int N, int H, int W, int C, int stride, hipStream_t s);
int icamd_dwconv3_wgrad_launch(const bf16_t* x, const float* in_scale, const float* in_shift, const bf16_t* dy, float* part, float* dw,
                               int N, int H, int W, int C, int stride, int accumulate, hipStream_t s);
int icamd_bn_apply_relu6_launch(const bf16_t* y, const float* scale, const float* shift, bf16_t* out, long long numel, int C,
                                hipStream_t s);
int icamd_bn_bwd_relu6_launch(const bf16_t* dout, const bf16_t* y, const float* mean, const float* invstd, const float* scale,
                              const float* shift, float* dgamma, float* dbeta, bf16_t* dy, long long rows, int C, int accumulate,
                              float* part, double* chunks, float* c1c2, hipStream_t s);

// EfficientNet class: depthwise 5x5 (pad 2, stride 1 / 2), BatchNorm + SiLU and the MBConv squeeze-and-excitation (dwconv5x5.hip)
bool icamd_dwconv5_ok(int N, int H, int W, int C, int stride);   // C % 8 == 0, stride 1 or 2, grids below 2^31 workgroups
long long icamd_dwconv5_stats_rows_cxx(int N, int H, int W, int C, int stride);
long long icamd_dwconv5_wgrad_rows(int N, int H, int W, int C, int stride);
int icamd_dwconv5_fwd_launch(const bf16_t* x, const bf16_t* w, bf16_t* y, float* stats, int N, int H, int W, int C, int stride,
                             int flip, hipStream_t s);
int icamd_dwconv5_dgrad_launch(const bf16_t* dy, const bf16_t* w, bf16_t* dx, int N, int H, int W, int C, int stride, hipStream_t s);
int icamd_dwconv5_wgrad_launch(const bf16_t* x, const bf16_t* dy, float* part, float* dw, int N, int H, int W, int C, int stride,
                               int accumulate, hipStream_t s);
bool icamd_silu_shape_ok(int N, int HW, int C, int rd);          // C % 8 == 0, C <= 4096, 1 <= rd <= 256
void icamd_silu_plan(int N, int HW, int* S, int* rps);
size_t icamd_silu_rowsum_bytes(int N, int HW, int C);
int icamd_bn_apply_silu_launch(const bf16_t* y, const float* scale, const float* shift, const float* gate, bf16_t* out, int N, int HW,
                               int C, hipStream_t s);
int icamd_silu_rowsum_launch(const bf16_t* dout, const bf16_t* y, const float* scale, const float* shift, float* out, int N, int HW,
                             int C, float* part, hipStream_t s);
int icamd_se_excite_silu_fwd_launch(const float* asum, float inv_hw, const float* w1, const float* b1, const float* w2, const float* b2,
                                    float* s_out, float* hpre, float* e, int N, int C, int rd, hipStream_t s);
int icamd_se_excite_silu_bwd_launch(const float* de, const float* sv, const float* hpre, const float* e, const float* w1,
                                    const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dsn, int N, int C, int rd,
                                    float inv_hw, int accumulate, hipStream_t s);
int icamd_bn_bwd_silu_launch(const bf16_t* dout, const bf16_t* y, const float* mean, const float* invstd, const float* scale,
                             const float* shift, const float* gate, const float* dsn, float* dgamma, float* dbeta, bf16_t* dy, int N,
                             int HW, int C, int accumulate, float* part, double* chunks, float* c1c2, hipStream_t s);

// ConvNeXt V2: global response normalisation (grn.hip)
bool icamd_grn_ok(int N, long long HW, int C);
void icamd_grn_plan(int N, int HW, int C, int* S, int* rps, int* B, int* rpb);
size_t icamd_grn_bytes(int N, int HW, int C);
int icamd_grn_fwd_launch(const bf16_t* a, const float* gamma, const float* beta, bf16_t* g, float* gx_out, int N, int HW, int C,
                         float eps, void* workspace, hipStream_t s);
int icamd_grn_bwd_launch(const bf16_t* dg, const bf16_t* a, const float* gx, const float* gamma, const bf16_t* z, bf16_t* dx,
                         float* dgamma, float* dbeta, int accumulate, int N, int HW, int C, float eps, void* workspace,
                         hipStream_t s);
