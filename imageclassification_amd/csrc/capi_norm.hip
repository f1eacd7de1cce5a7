// C-ABI entry points of BatchNorm (finalize / apply / backward, the ReLU6 pair), the squeeze-and-excitation tail and max / average
// pooling.
#include "capi_common.h"

extern "C" {

size_t icamd_bn_workspace_bytes(int C) { return C > 0 ? reduce_ws(nullptr, C, 0, 0).bytes : 0; }

int icamd_bn_train_finalize(const float* partials, int nrows, int C, double count, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                            float* mean, float* invstd, float* scale, float* shift, void* workspace, void* stream) {
  ProfScope _prof(PC_BN_FINALIZE, stream);
  _prof.work(8.0 * nrows * C);
  if (partials == nullptr || nrows <= 0 || C <= 0 || count <= 0 || gamma == nullptr || beta == nullptr ||
      mean == nullptr || invstd == nullptr || scale == nullptr || shift == nullptr || workspace == nullptr || C > 4096)
    return ICAMD_ERR_BAD_ARG;
  return icamd_bn_finalize_launch(partials, nrows, C, count, gamma, beta, running_mean, running_var, momentum, eps, mean,
                                  invstd, scale, shift, reduce_ws(workspace, C, 0, 0).chunks, (hipStream_t)stream);
}

int icamd_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, float* scale, float* shift, void* stream) {
  ProfScope _prof(PC_BN_FINALIZE, stream);
  _prof.work(24.0 * C);
  if (C <= 0 || gamma == nullptr || beta == nullptr || running_mean == nullptr || running_var == nullptr ||
      scale == nullptr || shift == nullptr)
    return ICAMD_ERR_BAD_ARG;
  return icamd_bn_eval_coeffs_launch(C, gamma, beta, running_mean, running_var, eps, scale, shift, (hipStream_t)stream);
}

int icamd_bn_apply(const void* y, const float* scale, const float* shift, const void* residual, void* out,
                   uint8_t* maskbits, long long numel, int C, int relu, void* stream) {
  ProfScope _prof(PC_BN_APPLY, stream);
  _prof.work((double)numel * (4 + (residual ? 2 : 0)) + (maskbits ? numel / 8.0 : 0));
  if (y == nullptr || scale == nullptr || shift == nullptr || out == nullptr || numel <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_bn_apply_launch((const bf16_t*)y, scale, shift, (const bf16_t*)residual, (bf16_t*)out, maskbits, numel, C,
                               relu, (hipStream_t)stream);
}

int icamd_bn_apply_res_bn(const void* y, const float* scale, const float* shift, const void* res_y, const float* res_scale,
                          const float* res_shift, void* out, uint8_t* maskbits, long long numel, int C, int relu,
                          void* stream) {
  ProfScope _prof(PC_BN_APPLY, stream);
  _prof.work((double)numel * 6 + (maskbits ? numel / 8.0 : 0));
  if (y == nullptr || scale == nullptr || shift == nullptr || res_y == nullptr || res_scale == nullptr ||
      res_shift == nullptr || out == nullptr || numel <= 0 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_bn_apply_launch((const bf16_t*)y, scale, shift, (const bf16_t*)res_y, (bf16_t*)out, maskbits, numel, C, relu,
                               (hipStream_t)stream, res_scale, res_shift);
}

// ---- squeeze-and-excitation tail (se_ops.hip) ----
size_t icamd_se_squeeze_workspace_bytes(int N, int HW, int C) {
  if (!icamd_se_shape_ok(N, HW, C, 1)) return 0;
  return icamd_se_squeeze_bytes(N, HW, C);
}

int icamd_se_squeeze(const void* y, float* ysum, int N, int HW, int C, void* workspace, size_t workspace_bytes, void* stream) {
  if (y == nullptr || ysum == nullptr || workspace == nullptr || N <= 0 || HW <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  if (!icamd_se_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace_bytes < icamd_se_squeeze_bytes(N, HW, C)) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_POOL, stream);
  _prof.work(2.0 * N * HW * C + 4.0 * N * C);
  return icamd_se_squeeze_launch((const bf16_t*)y, ysum, N, HW, C, (float*)workspace, (hipStream_t)stream);
}

int icamd_se_excite_fwd(const float* ysum, const float* scale, const float* shift, float inv_hw, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* s, float* h, float* e, int N, int C, int rd, void* stream) {
  if (ysum == nullptr || scale == nullptr || shift == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || b2 == nullptr ||
      s == nullptr || h == nullptr || e == nullptr || N <= 0 || C <= 0 || rd <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_se_shape_ok(N, 1, C, rd)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_MISC, stream);
  _prof.work(4.0 * N * (3.0 * C + rd) + 4.0 * (2.0 * C * rd + C + rd), 4.0 * N * C * rd);
  return icamd_se_excite_fwd_launch(ysum, scale, shift, inv_hw, w1, b1, w2, b2, s, h, e, N, C, rd, (hipStream_t)stream);
}

int icamd_se_bn_apply(const void* y, const float* scale, const float* shift, const float* e, const void* residual,
                      const float* res_scale, const float* res_shift, void* out, uint8_t* maskbits, int N, int HW, int C, int relu,
                      void* stream) {
  if (y == nullptr || scale == nullptr || shift == nullptr || e == nullptr || out == nullptr || N <= 0 || HW <= 0 || C <= 0 ||
      (res_scale == nullptr) != (res_shift == nullptr) || (res_scale != nullptr && residual == nullptr))
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_se_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_BN_APPLY, stream);
  const double numel = (double)N * HW * C;
  _prof.work(numel * (4 + (residual ? 2 : 0)) + (maskbits ? numel / 8.0 : 0) + 4.0 * N * C);
  return icamd_se_bn_apply_launch((const bf16_t*)y, scale, shift, e, (const bf16_t*)residual, res_scale, res_shift, (bf16_t*)out,
                                  maskbits, N, HW, C, relu, (hipStream_t)stream);
}

size_t icamd_se_bn_bwd_workspace_bytes(int N, int HW, int C) {
  if (!icamd_se_shape_ok(N, HW, C, 1)) return 0;
  return icamd_se_bn_bwd_bytes(N, HW, C);
}

int icamd_se_bn_bwd(const void* dout, const uint8_t* maskbits, const void* y, const float* mean, const float* invstd,
                    const float* gamma, const float* beta, const float* ysum, const float* s, const float* h, const float* e,
                    const float* w1, const float* w2, float* dgamma, float* dbeta, float* dw1, float* db1, float* dw2, float* db2,
                    void* dy, int N, int HW, int C, int rd, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (dout == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || gamma == nullptr || beta == nullptr ||
      ysum == nullptr || s == nullptr || h == nullptr || e == nullptr || w1 == nullptr || w2 == nullptr || dgamma == nullptr ||
      dbeta == nullptr || dw1 == nullptr || db1 == nullptr || dw2 == nullptr || db2 == nullptr || dy == nullptr ||
      workspace == nullptr || N <= 0 || HW <= 0 || C <= 0 || rd <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_se_shape_ok(N, HW, C, rd)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace_bytes < icamd_se_bn_bwd_bytes(N, HW, C)) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_BN_BWD, stream);
  const double numel = (double)N * HW * C;
  _prof.work(numel * (2 * 4 + 2) + (maskbits ? numel / 4.0 : 0) + 4.0 * N * (8.0 * C + 2.0 * rd) + 16.0 * C * rd, 8.0 * N * C * rd);
  return icamd_se_bn_bwd_launch((const bf16_t*)dout, maskbits, (const bf16_t*)y, mean, invstd, gamma, beta, ysum, s, h, e, w1, w2,
                                dgamma, dbeta, dw1, db1, dw2, db2, (bf16_t*)dy, N, HW, C, rd, accumulate, workspace,
                                (hipStream_t)stream);
}

// bwd workspace (reduce_ws): counters | chunks [64][2][C] doubles | partial rows [nblk][2][C] floats | c1,c2 [2][C] floats
size_t icamd_bn_bwd_workspace_bytes(long long rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return reduce_ws(nullptr, C, bn_bwd_blocks(rows, C), 2).bytes;
}

// what icamd_bn_bwd and icamd_bn_bwd_maxpool3x3s2 share behind their argument checks
static int bn_bwd_impl(const void* dout, const void* act, const void* y, const float* mean, const float* invstd, const float* scale,
                       const float* shift, float* dgamma, float* dbeta, void* dy, void* gout, const uint8_t* maskbits,
                       long long rows, int C, int relu, int accumulate, void* workspace, size_t workspace_bytes, void* stream,
                       const uint8_t* pool_idx = nullptr, int IH = 0, int IW = 0) {
  if (workspace_bytes < icamd_bn_bwd_workspace_bytes(rows, C)) return ICAMD_ERR_WORKSPACE;
  if (C > 4096) return ICAMD_ERR_UNSUPPORTED;
  const ReduceWs w = reduce_ws(workspace, C, bn_bwd_blocks(rows, C), 2);
  return icamd_bn_bwd_launch((const bf16_t*)dout, (const bf16_t*)act, (const bf16_t*)y, mean, invstd, scale, shift, dgamma,
                             dbeta, (bf16_t*)dy, (bf16_t*)gout, maskbits, rows, C, relu, accumulate, w.part, w.chunks, w.scratch,
                             (hipStream_t)stream, pool_idx, IH, IW);
}

int icamd_bn_bwd(const void* dout, const void* act, const void* y, const float* mean, const float* invstd,
                 const float* scale, const float* shift, float* dgamma, float* dbeta, void* dy, void* gout,
                 const uint8_t* maskbits, long long rows, int C, int relu, int accumulate, void* workspace,
                 size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)rows * C * (2 * (4 + (act ? 2 : 0)) + 2 + (gout ? 2 : 0)) + (maskbits ? rows * C / 4.0 : 0));
  if (dout == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || scale == nullptr || shift == nullptr ||
      dgamma == nullptr || dbeta == nullptr || dy == nullptr || workspace == nullptr || rows <= 0 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  return bn_bwd_impl(dout, act, y, mean, invstd, scale, shift, dgamma, dbeta, dy, gout, maskbits, rows, C, relu, accumulate,
                     workspace, workspace_bytes, stream);
}

int icamd_bn_bwd_maxpool3x3s2(const void* dout_pooled, const uint8_t* idx, const void* y, const float* mean,
                              const float* invstd, const float* scale, const float* shift, float* dgamma, float* dbeta,
                              void* dy, int N, int IH, int IW, int C, int accumulate, void* workspace, size_t workspace_bytes,
                              void* stream) {
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)N * IH * IW * C * (2 * 2 + 2) + 2.0 * N * IH * IW * C / 4 * 3);
  if (dout_pooled == nullptr || idx == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || scale == nullptr ||
      shift == nullptr || dgamma == nullptr || dbeta == nullptr || dy == nullptr || workspace == nullptr || N <= 0 || IH <= 0 ||
      IW <= 0 || C <= 0 || C % 8 != 0)
    return ICAMD_ERR_BAD_ARG;
  return bn_bwd_impl(dout_pooled, nullptr, y, mean, invstd, scale, shift, dgamma, dbeta, dy, nullptr, nullptr,
                     (long long)N * IH * IW, C, /*relu=*/1, accumulate, workspace, workspace_bytes, stream, idx, IH, IW);
}

int icamd_bn_bwd_dual(const void* dout, const uint8_t* maskbits, const void* yA, const float* meanA, const float* invstdA,
                      const float* scaleA, float* dgammaA, float* dbetaA, void* dyA, const void* yB, const float* meanB,
                      const float* invstdB, const float* scaleB, float* dgammaB, float* dbetaB, void* dyB, long long rows, int C,
                      int accumulate, void* workspaceA, void* workspaceB, size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)rows * C * (2 * 6 + 4) + rows * C / 4.0);
  if (dout == nullptr || maskbits == nullptr || yA == nullptr || yB == nullptr || meanA == nullptr || meanB == nullptr ||
      invstdA == nullptr || invstdB == nullptr || scaleA == nullptr || scaleB == nullptr || dgammaA == nullptr ||
      dgammaB == nullptr || dbetaA == nullptr || dbetaB == nullptr || dyA == nullptr || dyB == nullptr ||
      workspaceA == nullptr || workspaceB == nullptr || workspaceA == workspaceB || rows <= 0 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (workspace_bytes < icamd_bn_bwd_workspace_bytes(rows, C)) return ICAMD_ERR_WORKSPACE;
  if (C > 4096) return ICAMD_ERR_UNSUPPORTED;
  const long long nblk = bn_bwd_blocks(rows, C);
  const ReduceWs a = reduce_ws(workspaceA, C, nblk, 2), b = reduce_ws(workspaceB, C, nblk, 2);
  return icamd_bn_bwd_dual_launch((const bf16_t*)dout, maskbits, (const bf16_t*)yA, meanA, invstdA, scaleA, dgammaA, dbetaA,
                                  (bf16_t*)dyA, (const bf16_t*)yB, meanB, invstdB, scaleB, dgammaB, dbetaB, (bf16_t*)dyB, rows,
                                  C, accumulate, a.part, a.chunks, a.scratch, b.part, b.chunks, b.scratch, (hipStream_t)stream);
}

// workspace (reduce_ws without partial rows): counters | chunks [64][2][C] doubles | c1,c2 [2][C] floats
size_t icamd_bn_bwd_apply_workspace_bytes(int C) { return C > 0 ? reduce_ws(nullptr, C, 0, 2).bytes : 0; }

// what icamd_bn_bwd_from_partials and icamd_bn_bwd_from_gy_partials share behind their argument checks
static int bn_bwd_from_partials_impl(const float* partials, int nrows, const void* g, const void* y, const float* mean,
                                     const float* invstd, const float* scale, float* dgamma, float* dbeta, void* dy,
                                     long long rows, int C, int accumulate, void* workspace, size_t workspace_bytes,
                                     void* stream, int sums_are_gy) {
  if (workspace_bytes < icamd_bn_bwd_apply_workspace_bytes(C)) return ICAMD_ERR_WORKSPACE;
  if (C > 4096) return ICAMD_ERR_UNSUPPORTED;
  const ReduceWs w = reduce_ws(workspace, C, 0, 2);
  return icamd_bn_bwd_apply_launch(partials, nrows, (const bf16_t*)g, (const bf16_t*)y, mean, invstd, scale, dgamma, dbeta,
                                   (bf16_t*)dy, rows, C, accumulate, w.chunks, w.scratch, (hipStream_t)stream, sums_are_gy);
}

int icamd_bn_bwd_from_partials(const float* partials, int nrows, const void* g, const void* y, const float* mean,
                               const float* invstd, const float* scale, float* dgamma, float* dbeta, void* dy,
                               long long rows, int C, int accumulate, void* workspace, size_t workspace_bytes,
                               void* stream) {
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)rows * C * 6 + 8.0 * nrows * C);
  if (partials == nullptr || nrows <= 0 || g == nullptr || y == nullptr || mean == nullptr || invstd == nullptr ||
      scale == nullptr || dgamma == nullptr || dbeta == nullptr || dy == nullptr || workspace == nullptr || rows <= 0 ||
      C <= 0 || C % 8 != 0)
    return ICAMD_ERR_BAD_ARG;
  return bn_bwd_from_partials_impl(partials, nrows, g, y, mean, invstd, scale, dgamma, dbeta, dy, rows, C, accumulate, workspace,
                                   workspace_bytes, stream, 0);
}

int icamd_bn_bwd_from_gy_partials(const float* partials, int nrows, const void* g, const void* y, const float* mean,
                                  const float* invstd, const float* scale, float* dgamma, float* dbeta, void* dy,
                                  long long rows, int C, int accumulate, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)rows * C * 6 + 8.0 * nrows * C);
  if (partials == nullptr || nrows <= 0 || g == nullptr || y == nullptr || mean == nullptr || invstd == nullptr ||
      scale == nullptr || dgamma == nullptr || dbeta == nullptr || dy == nullptr || workspace == nullptr || rows <= 0 ||
      C <= 0 || C % 8 != 0)
    return ICAMD_ERR_BAD_ARG;
  return bn_bwd_from_partials_impl(partials, nrows, g, y, mean, invstd, scale, dgamma, dbeta, dy, rows, C, accumulate, workspace,
                                   workspace_bytes, stream, 1);
}

// ---- BatchNorm + ReLU6 (dwconv3x3.hip) ----
int icamd_bn_apply_relu6(const void* y, const float* scale, const float* shift, void* out, long long numel, int C, void* stream) {
  if (y == nullptr || scale == nullptr || shift == nullptr || out == nullptr || numel <= 0 || C <= 0 || C % 8 != 0 || numel % C != 0)
    return ICAMD_ERR_BAD_ARG;
  ProfScope _prof(PC_BN_APPLY, stream);
  _prof.work((double)numel * 4);
  return icamd_bn_apply_relu6_launch((const bf16_t*)y, scale, shift, (bf16_t*)out, numel, C, (hipStream_t)stream);
}

// the workspace of icamd_bn_bwd: the same reduce pass geometry, the same finalize kernel
size_t icamd_bn_bwd_relu6_workspace_bytes(long long rows, int C) { return icamd_bn_bwd_workspace_bytes(rows, C); }

int icamd_bn_bwd_relu6(const void* dout, const void* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                       float* dgamma, float* dbeta, void* dy, long long rows, int C, int accumulate, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (dout == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || scale == nullptr || shift == nullptr ||
      dgamma == nullptr || dbeta == nullptr || dy == nullptr || workspace == nullptr || rows <= 0 || C <= 0 || C % 8 != 0)
    return ICAMD_ERR_BAD_ARG;
  if (workspace_bytes < icamd_bn_bwd_relu6_workspace_bytes(rows, C)) return ICAMD_ERR_WORKSPACE;
  if (C > 4096) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)rows * C * (2 * 4 + 2));
  const ReduceWs w = reduce_ws(workspace, C, bn_bwd_blocks(rows, C), 2);
  return icamd_bn_bwd_relu6_launch((const bf16_t*)dout, (const bf16_t*)y, mean, invstd, scale, shift, dgamma, dbeta, (bf16_t*)dy, rows,
                                   C, accumulate, w.part, w.chunks, w.scratch, (hipStream_t)stream);
}

// ---- BatchNorm + SiLU and the MBConv squeeze-and-excitation (dwconv5x5.hip) ----
int icamd_bn_apply_silu(const void* y, const float* scale, const float* shift, const float* e, void* out, int N, int HW, int C,
                        void* stream) {
  if (y == nullptr || scale == nullptr || shift == nullptr || out == nullptr || N <= 0 || HW <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_BN_APPLY, stream);
  _prof.work((double)N * HW * C * 4 + (e ? 4.0 * N * C : 0.0));
  return icamd_bn_apply_silu_launch((const bf16_t*)y, scale, shift, e, (bf16_t*)out, N, HW, C, (hipStream_t)stream);
}

size_t icamd_bn_silu_squeeze_workspace_bytes(int N, int HW, int C) {
  return icamd_silu_shape_ok(N, HW, C, 1) ? icamd_silu_rowsum_bytes(N, HW, C) : 0;
}

int icamd_bn_silu_squeeze(const void* y, const float* scale, const float* shift, float* asum, int N, int HW, int C, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (y == nullptr || scale == nullptr || shift == nullptr || asum == nullptr || workspace == nullptr || N <= 0 || HW <= 0 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace_bytes < icamd_silu_rowsum_bytes(N, HW, C)) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_POOL, stream);
  _prof.work(2.0 * N * HW * C + 4.0 * N * C);
  return icamd_silu_rowsum_launch(nullptr, (const bf16_t*)y, scale, shift, asum, N, HW, C, (float*)workspace, (hipStream_t)stream);
}

int icamd_se_excite_silu_fwd(const float* asum, float inv_hw, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* s, float* hpre, float* e, int N, int C, int rd, void* stream) {
  if (asum == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || b2 == nullptr || s == nullptr || hpre == nullptr ||
      e == nullptr || N <= 0 || C <= 0 || rd <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_silu_shape_ok(N, 1, C, rd)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_MISC, stream);
  _prof.work(4.0 * N * (3.0 * C + rd) + 4.0 * (2.0 * C * rd + C + rd), 4.0 * N * C * rd);
  return icamd_se_excite_silu_fwd_launch(asum, inv_hw, w1, b1, w2, b2, s, hpre, e, N, C, rd, (hipStream_t)stream);
}

size_t icamd_se_silu_bwd_reduce_workspace_bytes(int N, int HW, int C) { return icamd_bn_silu_squeeze_workspace_bytes(N, HW, C); }

int icamd_se_silu_bwd_reduce(const void* dout, const void* y, const float* scale, const float* shift, float* de, int N, int HW, int C,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (dout == nullptr || y == nullptr || scale == nullptr || shift == nullptr || de == nullptr || workspace == nullptr || N <= 0 ||
      HW <= 0 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  if (workspace_bytes < icamd_silu_rowsum_bytes(N, HW, C)) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work(4.0 * N * HW * C + 4.0 * N * C);
  return icamd_silu_rowsum_launch((const bf16_t*)dout, (const bf16_t*)y, scale, shift, de, N, HW, C, (float*)workspace,
                                  (hipStream_t)stream);
}

int icamd_se_excite_silu_bwd(const float* de, const float* s, const float* hpre, const float* e, const float* w1, const float* w2,
                             float* dw1, float* db1, float* dw2, float* db2, float* dsn, int N, int C, int rd, float inv_hw,
                             int accumulate, void* stream) {
  if (de == nullptr || s == nullptr || hpre == nullptr || e == nullptr || w1 == nullptr || w2 == nullptr || dw1 == nullptr ||
      db1 == nullptr || dw2 == nullptr || db2 == nullptr || dsn == nullptr || N <= 0 || C <= 0 || rd <= 0)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_silu_shape_ok(N, 1, C, rd)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_MISC, stream);
  _prof.work(4.0 * N * (5.0 * C + rd) + 16.0 * C * rd, 8.0 * N * C * rd);
  return icamd_se_excite_silu_bwd_launch(de, s, hpre, e, w1, w2, dw1, db1, dw2, db2, dsn, N, C, rd, inv_hw, accumulate,
                                         (hipStream_t)stream);
}

// the workspace of icamd_bn_bwd over N * HW rows: the same reduce pass geometry, the same finalize kernel
size_t icamd_bn_bwd_silu_workspace_bytes(int N, int HW, int C) {
  return icamd_silu_shape_ok(N, HW, C, 1) ? icamd_bn_bwd_workspace_bytes((long long)N * HW, C) : 0;
}

int icamd_bn_bwd_silu(const void* dout, const void* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                      const float* e, const float* dsn, float* dgamma, float* dbeta, void* dy, int N, int HW, int C, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (dout == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || scale == nullptr || shift == nullptr ||
      dgamma == nullptr || dbeta == nullptr || dy == nullptr || workspace == nullptr || N <= 0 || HW <= 0 || C <= 0 ||
      (e == nullptr) != (dsn == nullptr))
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_silu_shape_ok(N, HW, C, 1)) return ICAMD_ERR_UNSUPPORTED;
  const long long rows = (long long)N * HW;
  if (workspace_bytes < icamd_bn_bwd_workspace_bytes(rows, C)) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_BN_BWD, stream);
  _prof.work((double)rows * C * (2 * 4 + 2) + (e ? 16.0 * N * C : 0.0));
  const ReduceWs w = reduce_ws(workspace, C, bn_bwd_blocks(rows, C), 2);
  return icamd_bn_bwd_silu_launch((const bf16_t*)dout, (const bf16_t*)y, mean, invstd, scale, shift, e, dsn, dgamma, dbeta, (bf16_t*)dy,
                                  N, HW, C, accumulate, w.part, w.chunks, w.scratch, (hipStream_t)stream);
}

int icamd_maxpool3x3s2_fwd(const void* x, void* out, uint8_t* argmax, int N, int IH, int IW, int C, void* stream) {
  ProfScope _prof(PC_POOL, stream);
  _prof.work((double)N * IH * IW * C * (2 + 0.75));
  if (x == nullptr || out == nullptr || N <= 0 || IH <= 0 || IW <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  const int OH = (IH + 2 - 3) / 2 + 1, OW = (IW + 2 - 3) / 2 + 1;
  return icamd_maxpool_fwd_launch((const bf16_t*)x, (bf16_t*)out, argmax, N, IH, IW, C, OH, OW, (hipStream_t)stream);
}

int icamd_bn_relu_maxpool3x3s2_fwd(const void* y, const float* scale, const float* shift, void* out, uint8_t* argmax, int N,
                                   int IH, int IW, int C, void* stream) {
  ProfScope _prof(PC_BN_APPLY, stream);
  _prof.work((double)N * IH * IW * C * (2 + 0.75));
  if (y == nullptr || scale == nullptr || shift == nullptr || out == nullptr || N <= 0 || IH <= 0 || IW <= 0 || C <= 0)
    return ICAMD_ERR_BAD_ARG;
  const int OH = (IH + 2 - 3) / 2 + 1, OW = (IW + 2 - 3) / 2 + 1;
  return icamd_bn_relu_maxpool_fwd_launch((const bf16_t*)y, scale, shift, (bf16_t*)out, argmax, N, IH, IW, C, OH, OW,
                                          (hipStream_t)stream);
}

int icamd_maxpool3x3s2_bwd(const void* dout, const uint8_t* argmax, void* dx, int N, int IH, int IW, int C, void* stream) {
  ProfScope _prof(PC_POOL, stream);
  _prof.work((double)N * IH * IW * C * (2 + 0.75));
  if (dout == nullptr || argmax == nullptr || dx == nullptr || N <= 0 || IH <= 0 || IW <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  const int OH = (IH + 2 - 3) / 2 + 1, OW = (IW + 2 - 3) / 2 + 1;
  return icamd_maxpool_bwd_launch((const bf16_t*)dout, argmax, (bf16_t*)dx, N, IH, IW, C, OH, OW, (hipStream_t)stream);
}

int icamd_avgpool_fwd(const void* x, void* out, int N, int HW, int C, void* stream) {
  ProfScope _prof(PC_POOL, stream);
  _prof.work(2.0 * N * HW * C + 2.0 * N * C);
  if (x == nullptr || out == nullptr || N <= 0 || HW <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_avgpool_fwd_launch((const bf16_t*)x, (bf16_t*)out, N, HW, C, (hipStream_t)stream);
}

int icamd_avgpool_bwd(const void* dout, void* dx, int N, int HW, int C, void* stream) {
  ProfScope _prof(PC_POOL, stream);
  _prof.work(2.0 * N * HW * C + 2.0 * N * C);
  if (dout == nullptr || dx == nullptr || N <= 0 || HW <= 0 || C <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_avgpool_bwd_launch((const bf16_t*)dout, (bf16_t*)dx, N, HW, C, (hipStream_t)stream);
}

}  // extern "C"
