// C-ABI entry points of the token models (ViT, Swin, ConvNeXt): LayerNorm, GELU, token assembly and reductions, depthwise 7x7,
// layer scale, global response normalisation, attention, window attention, relative-position bias and patch merging.
#include "capi_common.h"

extern "C" {

// ---- LayerNorm / GELU / column sums (ViT, ConvNeXt) -------------------------------------------------------------
int icamd_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                        long long rows, int C, float eps, void* stream) {
  ProfScope _prof(PC_LN_FWD, stream);
  _prof.work((double)rows * C * 4 + 8.0 * rows);
  if (x == nullptr || gamma == nullptr || beta == nullptr || y == nullptr || mean == nullptr || rstd == nullptr || rows <= 0 ||
      C <= 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_layernorm_fwd_launch((const bf16_t*)x, gamma, beta, (bf16_t*)y, mean, rstd, rows, C, eps, (hipStream_t)stream);
}

// workspace (reduce_ws): [counters|chunks] | partial rows [blocks][2][C] | scratch [2][C]
size_t icamd_layernorm_bwd_workspace_bytes(long long rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return reduce_ws(nullptr, C, icamd_layernorm_bwd_blocks(rows), 2).bytes;
}

int icamd_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                        const void* addend, void* dx, float* dgamma, float* dbeta, long long rows, int C, int accumulate,
                        void* workspace, size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_LN_BWD, stream);
  _prof.work((double)rows * C * (6 + (addend ? 2 : 0)) + 8.0 * rows);
  if (dy == nullptr || x == nullptr || mean == nullptr || rstd == nullptr || gamma == nullptr || dx == nullptr ||
      dgamma == nullptr || dbeta == nullptr || workspace == nullptr || rows <= 0 || C <= 0 || C > 4096)
    return ICAMD_ERR_BAD_ARG;
  if (workspace_bytes < icamd_layernorm_bwd_workspace_bytes(rows, C)) return ICAMD_ERR_WORKSPACE;
  const int nblk = icamd_layernorm_bwd_blocks(rows);
  const ReduceWs w = reduce_ws(workspace, C, nblk, 2);
  int rc = icamd_layernorm_bwd_launch((const bf16_t*)dy, (const bf16_t*)x, mean, rstd, gamma, (const bf16_t*)addend,
                                      (bf16_t*)dx, w.part, rows, C, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_sum_partials_launch(w.part, nblk, C, dbeta, dgamma, accumulate, w.chunks, w.scratch, (hipStream_t)stream);
}

int icamd_gelu_fwd(const void* z, void* a, long long numel, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(4.0 * numel);
  if (z == nullptr || a == nullptr || numel <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_gelu_fwd_launch((const bf16_t*)z, (bf16_t*)a, numel, (hipStream_t)stream);
}

int icamd_gelu_bwd(const void* da, const void* z, void* dz, long long numel, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(6.0 * numel);
  if (da == nullptr || z == nullptr || dz == nullptr || numel <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_gelu_bwd_launch((const bf16_t*)da, (const bf16_t*)z, (bf16_t*)dz, numel, (hipStream_t)stream);
}

size_t icamd_colsum_rows_workspace_bytes(long long rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return reduce_ws(nullptr, cols, icamd_colsum_blocks(rows), 3).bytes;
}

// out[c] = (accumulate ? out[c] : 0) + sum_r x[r][c], two-level, fixed order (bias gradients of long token matrices)
int icamd_colsum_rows(const void* x, long long rows, int ld, int cols, float* out, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_MISC, stream);
  _prof.work(2.0 * rows * cols);
  if (x == nullptr || out == nullptr || workspace == nullptr || rows <= 0 || cols <= 0 || cols > 4096 || ld < cols)
    return ICAMD_ERR_BAD_ARG;
  if (workspace_bytes < icamd_colsum_rows_workspace_bytes(rows, cols)) return ICAMD_ERR_WORKSPACE;
  const int nblk = icamd_colsum_blocks(rows);
  const ReduceWs w = reduce_ws(workspace, cols, nblk, 3);   // scratch [3][cols]: discarded second sum + c1/c2
  int rc = icamd_colsum_partial_launch((const bf16_t*)x, w.part, rows, ld, cols, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_sum_partials_launch(w.part, nblk, cols, out, w.scratch, accumulate, w.chunks, w.scratch + cols,
                                   (hipStream_t)stream);
}

int icamd_vit_tokens_fwd(const void* patches, const float* cls_token, const float* pos_embed, void* tokens, int B, int T, int C,
                         void* stream) {
  ProfScope _prof(PC_MISC, stream);
  _prof.work(4.0 * B * T * C);
  if (patches == nullptr || cls_token == nullptr || pos_embed == nullptr || tokens == nullptr || B <= 0 || T <= 1 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_vit_tokens_fwd_launch((const bf16_t*)patches, cls_token, pos_embed, (bf16_t*)tokens, B, T, C, (hipStream_t)stream);
}

int icamd_batch_sum(const void* x, long long stride, int B, long long n, float* out, int accumulate, void* stream) {
  ProfScope _prof(PC_MISC, stream);
  _prof.work(2.0 * B * n);
  if (x == nullptr || out == nullptr || B <= 0 || n <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_batch_sum_launch((const bf16_t*)x, stride, B, n, out, accumulate, (hipStream_t)stream);
}

int icamd_strided_rows_copy(const void* src, long long src_stride, void* dst, long long dst_stride, long long rows, long long C,
                            void* stream) {
  ProfScope _prof(PC_MISC, stream);
  _prof.work(4.0 * rows * C);
  if (src == nullptr || dst == nullptr || rows <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_strided_rows_copy_launch((const bf16_t*)src, src_stride, (bf16_t*)dst, dst_stride, rows, C, (hipStream_t)stream);
}

// ---- ConvNeXt: depthwise 7x7 + layer scale / stochastic depth / residual ------------------------------------------
int icamd_dwconv7_fwd(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int C, void* stream) {
  ProfScope _prof(PC_DWCONV, stream);
  _prof.work(4.0 * N * H * W * C, 98.0 * N * H * W * C);
  if (x == nullptr || w == nullptr || y == nullptr || N <= 0 || H <= 0 || W <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_dwconv7_launch((const bf16_t*)x, (const bf16_t*)w, bias, nullptr, (bf16_t*)y, N, H, W, C, 0, (hipStream_t)stream);
}

int icamd_dwconv7_dgrad(const void* dy, const void* w, const void* addend, void* dx, int N, int H, int W, int C, void* stream) {
  ProfScope _prof(PC_DWCONV, stream);
  _prof.work((4.0 + (addend ? 2 : 0)) * N * H * W * C, 98.0 * N * H * W * C);
  if (dy == nullptr || w == nullptr || dx == nullptr || N <= 0 || H <= 0 || W <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_dwconv7_launch((const bf16_t*)dy, (const bf16_t*)w, nullptr, (const bf16_t*)addend, (bf16_t*)dx, N, H, W, C, 1,
                              (hipStream_t)stream);
}

size_t icamd_dwconv7_wgrad_workspace_bytes(int N, int H, int W, int C) {
  if (!icamd_dwconv7_ok(N, H, W, C)) return 0;
  return dw_wgrad_ws(nullptr, icamd_dwconv7_wgrad_blocks(N, H, W, C), C).bytes;   // [blocks][49][C] + the bias rows [blocks][C]
}

int icamd_dwconv7_wgrad(const void* x, const void* dy, float* dw, int accumulate, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int C, void* stream) {
  ProfScope _prof(PC_DWCONV, stream);
  _prof.work(4.0 * N * H * W * C, 98.0 * N * H * W * C);
  if (x == nullptr || dy == nullptr || dw == nullptr || workspace == nullptr) return ICAMD_ERR_BAD_ARG;
  const size_t need = icamd_dwconv7_wgrad_workspace_bytes(N, H, W, C);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  return icamd_dwconv7_wgrad_launch((const bf16_t*)x, (const bf16_t*)dy, (float*)workspace, dw, nullptr, N, H, W, C, accumulate,
                                    (hipStream_t)stream);
}

int icamd_dwconv7_wgrad_bias_supported(int N, int H, int W, int C) {
  return ::icamd_dwconv7_wgrad_bias_supported_cxx(N, H, W, C) ? 1 : 0;
}

int icamd_dwconv7_wgrad_bias(const void* x, const void* dy, float* dw, float* dbias, int accumulate, void* workspace,
                             size_t workspace_bytes, int N, int H, int W, int C, void* stream) {
  ProfScope _prof(PC_DWCONV, stream);
  _prof.work(4.0 * N * H * W * C, 100.0 * N * H * W * C);
  if (x == nullptr || dy == nullptr || dw == nullptr || dbias == nullptr || workspace == nullptr) return ICAMD_ERR_BAD_ARG;
  const size_t need = icamd_dwconv7_wgrad_workspace_bytes(N, H, W, C);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  return icamd_dwconv7_wgrad_launch((const bf16_t*)x, (const bf16_t*)dy, (float*)workspace, dw, dbias, N, H, W, C, accumulate,
                                    (hipStream_t)stream);
}

int icamd_layerscale_fwd(const void* z, const void* inp, const float* gamma, const float* keep, void* out, long long rows, int C,
                         long long rows_per_image, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(6.0 * rows * C);
  if (z == nullptr || inp == nullptr || gamma == nullptr || out == nullptr || rows <= 0 || C <= 0 || rows_per_image <= 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_layerscale_fwd_launch((const bf16_t*)z, (const bf16_t*)inp, gamma, keep, (bf16_t*)out, rows, C, rows_per_image,
                                     (hipStream_t)stream);
}

size_t icamd_layerscale_bwd_workspace_bytes(long long rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return reduce_ws(nullptr, C, icamd_layerscale_bwd_blocks(rows), 3).bytes;
}

int icamd_layerscale_bwd(const void* dout, const void* z, const float* gamma, const float* keep, void* dz, float* dgamma,
                         long long rows, int C, long long rows_per_image, int accumulate, void* workspace,
                         size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(6.0 * rows * C);
  if (dout == nullptr || z == nullptr || gamma == nullptr || dz == nullptr || dgamma == nullptr || workspace == nullptr ||
      rows <= 0 || C <= 0 || C > 4096 || rows_per_image <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (workspace_bytes < icamd_layerscale_bwd_workspace_bytes(rows, C)) return ICAMD_ERR_WORKSPACE;
  const int nblk = icamd_layerscale_bwd_blocks(rows);
  const ReduceWs w = reduce_ws(workspace, C, nblk, 3);
  int rc = icamd_layerscale_bwd_launch((const bf16_t*)dout, (const bf16_t*)z, gamma, keep, (bf16_t*)dz, w.part, rows, C,
                                       rows_per_image, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_sum_partials_launch(w.part, nblk, C, dgamma, w.scratch, accumulate, w.chunks, w.scratch + C, (hipStream_t)stream);
}

// Layer scale folded into the Mlp's second Linear layer (round 5): see include/icamd.h
int icamd_layerscale_fold(const float* params, void* shadow, float* fold_bias, const long long* jobs, int njobs, int total_rows,
                          long long total_elements, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(6.0 * (double)total_elements);
  if (params == nullptr || shadow == nullptr || fold_bias == nullptr || jobs == nullptr || njobs <= 0 || total_rows <= 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_layerscale_fold_launch(params, (bf16_t*)shadow, fold_bias, jobs, njobs, total_rows, (hipStream_t)stream);
}

int icamd_rows_fix(const float* keep, int n_images, void* dst1, const void* src1, long long bytes1, void* dst2, long long bytes2,
                   void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(4.0 * n_images);   // (the bytes of the dropped samples are data-dependent: not booked)
  if (keep == nullptr || n_images <= 0 || n_images > 65535 || (dst1 == nullptr && dst2 == nullptr) || bytes1 < 0 || bytes2 < 0 ||
      bytes1 % 16 != 0 || bytes2 % 16 != 0 || (dst1 == nullptr && src1 != nullptr))
    return ICAMD_ERR_BAD_ARG;
  return icamd_rows_fix_launch(keep, n_images, dst1, src1, bytes1, dst2, bytes2, (hipStream_t)stream);
}

int icamd_dropped_colsum(const void* dy, const float* keep, int n_images, long long rows_per_image, int C, float* partial,
                         void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(4.0 * n_images * C);
  if (dy == nullptr || keep == nullptr || partial == nullptr || n_images <= 0 || rows_per_image <= 0 || C <= 0 || C % 8 != 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_dropped_colsum_launch((const bf16_t*)dy, keep, n_images, rows_per_image, C, partial, (hipStream_t)stream);
}

int icamd_layerscale_param_grads(const float* G, const float* w, const float* bias, const float* gamma, const float* colsum_all,
                                 const float* dropped, int n_images, float cb, int C, int K, float* dw, float* dbias,
                                 float* dgamma, int accumulate, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work((accumulate ? 16.0 : 12.0) * C * K);
  if (G == nullptr || w == nullptr || bias == nullptr || gamma == nullptr || colsum_all == nullptr || dw == nullptr ||
      dbias == nullptr || dgamma == nullptr || C <= 0 || K <= 0 || K % 4 != 0 || (dropped != nullptr && n_images <= 0))
    return ICAMD_ERR_BAD_ARG;
  return icamd_layerscale_param_grads_launch(G, w, bias, gamma, colsum_all, dropped, n_images, cb, C, K, dw, dbias, dgamma,
                                             accumulate, (hipStream_t)stream);
}

// ---- ConvNeXt V2: global response normalisation (grn.hip) ----------------------------------------------------------
int icamd_grn_supported(int N, long long rows_per_image, int C) { return icamd_grn_ok(N, rows_per_image, C) ? 1 : 0; }

size_t icamd_grn_workspace_bytes(int N, long long rows_per_image, int C) {
  return icamd_grn_ok(N, rows_per_image, C) ? icamd_grn_bytes(N, (int)rows_per_image, C) : 0;
}

int icamd_grn_fwd(const void* a, const float* gamma, const float* beta, void* g, float* gx_out, int N, long long rows_per_image,
                  int C, float eps, void* workspace, size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work(6.0 * N * rows_per_image * C);   // a twice, g once
  if (a == nullptr || gamma == nullptr || beta == nullptr || g == nullptr || gx_out == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!icamd_grn_ok(N, rows_per_image, C)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < icamd_grn_workspace_bytes(N, rows_per_image, C)) return ICAMD_ERR_WORKSPACE;
  return icamd_grn_fwd_launch((const bf16_t*)a, gamma, beta, (bf16_t*)g, gx_out, N, (int)rows_per_image, C, eps, workspace,
                              (hipStream_t)stream);
}

int icamd_grn_bwd(const void* dg, const void* a, const float* gx, const float* gamma, const void* z, void* dx, float* dgamma,
                  float* dbeta, int accumulate, int N, long long rows_per_image, int C, float eps, void* workspace,
                  size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_ELEMWISE, stream);
  _prof.work((z ? 12.0 : 10.0) * N * rows_per_image * C);   // dg and a twice, z once, dx once
  if (dg == nullptr || a == nullptr || gx == nullptr || gamma == nullptr || dx == nullptr || dgamma == nullptr || dbeta == nullptr)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_grn_ok(N, rows_per_image, C)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < icamd_grn_workspace_bytes(N, rows_per_image, C)) return ICAMD_ERR_WORKSPACE;
  return icamd_grn_bwd_launch((const bf16_t*)dg, (const bf16_t*)a, gx, gamma, (const bf16_t*)z, (bf16_t*)dx, dgamma, dbeta,
                              accumulate, N, (int)rows_per_image, C, eps, workspace, (hipStream_t)stream);
}

// ---- attention (ViT) --------------------------------------------------------------------------------------------
int icamd_attention_fwd(const void* qkv, void* out, float* lse, int B, int T, int H, int D, float scale, void* stream) {
  ProfScope _prof(PC_ATTN_FWD, stream);
  _prof.work(8.0 * B * T * H * D, 4.0 * B * H * (double)T * T * D);
  if (qkv == nullptr || out == nullptr || lse == nullptr || B <= 0 || T <= 0 || H <= 0) return ICAMD_ERR_BAD_ARG;
  if (D != 64) return ICAMD_ERR_UNSUPPORTED;
  return icamd_attention_fwd_launch((const bf16_t*)qkv, (bf16_t*)out, lse, B, T, H, scale, (hipStream_t)stream);
}

int icamd_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                        int B, int T, int H, int D, float scale, void* stream) {
  ProfScope _prof(PC_ATTN_BWD, stream);
  _prof.work(16.0 * B * T * H * D, 10.0 * B * H * (double)T * T * D);
  if (qkv == nullptr || out == nullptr || dout == nullptr || lse == nullptr || delta == nullptr || dqkv == nullptr || B <= 0 ||
      T <= 0 || H <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (D != 64) return ICAMD_ERR_UNSUPPORTED;
  return icamd_attention_bwd_launch((const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, B,
                                    T, H, scale, (hipStream_t)stream);
}

// ---- Swin: window attention, relative-position bias, patch merging (window_attention.hip) ---------------------------
int icamd_window_attention_supported(int Hs, int Ws, int ws, int D) { return icamd_window_attention_ok(Hs, Ws, ws, D) ? 1 : 0; }

int icamd_window_attention_fwd(const void* qkv, const float* bias, void* out, float* lse, int B, int Hs, int Ws, int H, int D,
                               int ws, int shift, float scale, void* stream) {
  ProfScope _prof(PC_ATTN_FWD, stream);
  _prof.work(8.0 * B * Hs * Ws * H * D, 4.0 * B * Hs * Ws * H * (double)ws * ws * D);
  if (qkv == nullptr || bias == nullptr || out == nullptr || lse == nullptr || B <= 0 || H <= 0) return ICAMD_ERR_BAD_ARG;
  if (!icamd_window_attention_ok(Hs, Ws, ws, D) || shift < 0 || shift >= ws || (long long)B * Hs * Ws >= (1ll << 31))
    return ICAMD_ERR_UNSUPPORTED;
  return icamd_window_attention_fwd_launch((const bf16_t*)qkv, bias, (bf16_t*)out, lse, B, Hs, Ws, H, ws, shift, scale,
                                           (hipStream_t)stream);
}

size_t icamd_window_attention_bwd_workspace_bytes(int B, int Hs, int Ws, int H, int ws) {
  if (B <= 0 || H <= 0 || !icamd_window_attention_ok(Hs, Ws, ws, 32)) return 0;
  const long long nwin = (long long)B * (Hs / ws) * (Ws / ws);
  return ws_round256((size_t)icamd_window_attention_bwd_chunks(nwin, H, ws) * H * ws * ws * ws * ws * sizeof(float));
}

int icamd_window_attention_bwd(const void* qkv, const float* bias, const void* out, const void* dout, const float* lse,
                               void* dqkv, float* dbias, int accumulate, void* workspace, size_t workspace_bytes, int B, int Hs,
                               int Ws, int H, int D, int ws, int shift, float scale, void* stream) {
  ProfScope _prof(PC_ATTN_BWD, stream);
  _prof.work(18.0 * B * Hs * Ws * H * D, 14.0 * B * Hs * Ws * H * (double)ws * ws * D);
  if (qkv == nullptr || bias == nullptr || out == nullptr || dout == nullptr || lse == nullptr || dqkv == nullptr ||
      dbias == nullptr || B <= 0 || H <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_window_attention_ok(Hs, Ws, ws, D) || shift < 0 || shift >= ws || (long long)B * Hs * Ws >= (1ll << 31))
    return ICAMD_ERR_UNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < icamd_window_attention_bwd_workspace_bytes(B, Hs, Ws, H, ws))
    return ICAMD_ERR_WORKSPACE;
  return icamd_window_attention_bwd_launch((const bf16_t*)qkv, bias, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv,
                                           dbias, accumulate, (float*)workspace, B, Hs, Ws, H, ws, shift, scale,
                                           (hipStream_t)stream);
}

int icamd_relpos_bias_gather(const float* table, float* bias, int H, int ws, void* stream) {
  ProfScope _prof(PC_MISC, stream);
  if (table == nullptr || bias == nullptr || H <= 0) return ICAMD_ERR_BAD_ARG;
  if ((ws < 2 || ws > 8) && ws != 12) return ICAMD_ERR_UNSUPPORTED;
  return icamd_relpos_bias_gather_launch(table, bias, H, ws, (hipStream_t)stream);
}

int icamd_relpos_bias_scatter(const float* dbias, float* dtable, int H, int ws, int accumulate, void* stream) {
  ProfScope _prof(PC_MISC, stream);
  if (dbias == nullptr || dtable == nullptr || H <= 0) return ICAMD_ERR_BAD_ARG;
  if ((ws < 2 || ws > 8) && ws != 12) return ICAMD_ERR_UNSUPPORTED;
  return icamd_relpos_bias_scatter_launch(dbias, dtable, H, ws, accumulate, (hipStream_t)stream);
}

int icamd_patch_merge_ln_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int N, int H,
                             int W, int C, float eps, void* stream) {
  ProfScope _prof(PC_LN_FWD, stream);
  _prof.work(4.0 * N * H * W * C + 2.0 * N * H * W);
  if (x == nullptr || gamma == nullptr || beta == nullptr || y == nullptr || mean == nullptr || rstd == nullptr)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_patch_merge_ln_ok(N, H, W, C)) return ICAMD_ERR_UNSUPPORTED;
  return icamd_patch_merge_ln_fwd_launch((const bf16_t*)x, gamma, beta, (bf16_t*)y, mean, rstd, N, H, W, C, eps,
                                         (hipStream_t)stream);
}

size_t icamd_patch_merge_ln_bwd_workspace_bytes(int N, int H, int W, int C) {
  if (!icamd_patch_merge_ln_ok(N, H, W, C)) return 0;
  return ws_round256((size_t)icamd_patch_merge_ln_bwd_blocks((long long)N * (H / 2) * (W / 2)) * 8 * C * sizeof(float));
}

int icamd_patch_merge_ln_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, void* dx,
                             float* dgamma, float* dbeta, int N, int H, int W, int C, int accumulate, void* workspace,
                             size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_LN_BWD, stream);
  _prof.work(6.0 * N * H * W * C + 2.0 * N * H * W);
  if (dy == nullptr || x == nullptr || mean == nullptr || rstd == nullptr || gamma == nullptr || dx == nullptr ||
      dgamma == nullptr || dbeta == nullptr)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_patch_merge_ln_ok(N, H, W, C)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < icamd_patch_merge_ln_bwd_workspace_bytes(N, H, W, C)) return ICAMD_ERR_WORKSPACE;
  return icamd_patch_merge_ln_bwd_launch((const bf16_t*)dy, (const bf16_t*)x, mean, rstd, gamma, (bf16_t*)dx, dgamma, dbeta, N, H, W,
                                         C, accumulate, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
