// C-ABI entry points of the training step around the network: input packing, loss, step metrics, gradient norm, optimizers,
// weight conversion and small utilities.
#include "capi_common.h"

extern "C" {

int icamd_pack_input(const float* x, void* out, int B, int Cin, int H, int W, int mode, float lam, int yl, int yh,
                     int xl, int xh, void* stream) {
  ProfScope _prof(PC_PACK, stream);
  _prof.work((mode ? 8.0 : 4.0) * B * Cin * H * W + 16.0 * B * H * W);
  if (x == nullptr || out == nullptr || B <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2) return ICAMD_ERR_BAD_ARG;
  if (mode != 0 && (B % 2) != 0) return ICAMD_ERR_BAD_ARG;  // timm Mixup asserts an even batch
  return icamd_pack_input_launch(x, (bf16_t*)out, B, Cin, H, W, mode, lam, yl, yh, xl, xh, (hipStream_t)stream);
}

int icamd_pack_input_rgb4(const float* x, void* out, int B, int Cin, int H, int W, int mode, float lam, int yl, int yh,
                          int xl, int xh, void* stream) {
  ProfScope _prof(PC_PACK, stream);
  _prof.work((mode ? 8.0 : 4.0) * B * Cin * H * W + 8.0 * B * H * (W + 8));
  if (x == nullptr || out == nullptr || B <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2) return ICAMD_ERR_BAD_ARG;
  return icamd_pack_input_rgb4_launch(x, (bf16_t*)out, B, Cin, H, W, mode, lam, yl, yh, xl, xh, (hipStream_t)stream);
}

int icamd_softmax_xent(const void* logits, int ld, int B, int C, const int64_t* y1, const int64_t* y2, float lam,
                       float smoothing, float gscale, float* loss_rows, int32_t* pred, void* dlogits, void* stream) {
  ProfScope _prof(PC_LOSS, stream);
  _prof.work(4.0 * B * ld);
  if (logits == nullptr || y1 == nullptr || loss_rows == nullptr) return ICAMD_ERR_BAD_ARG;
  return icamd_softmax_xent_launch((const bf16_t*)logits, ld, B, C, (const long long*)y1, (const long long*)y2, lam,
                                   smoothing, gscale, loss_rows, pred, (bf16_t*)dlogits, (hipStream_t)stream);
}

int icamd_step_metrics(const float* loss_rows, const int32_t* pred, const int64_t* target, int B, int C,
                       float* loss_out, int32_t* finite_out, double* acc_f64, int32_t* counts, float* loss_log,
                       int log_slot, int log_stride, int respect_skip, void* stream) {
  ProfScope _prof(PC_LOSS, stream);
  _prof.work(16.0 * B);
  if (loss_out == nullptr || finite_out == nullptr || acc_f64 == nullptr || B <= 0) return ICAMD_ERR_BAD_ARG;
  if (pred != nullptr && target == nullptr) return ICAMD_ERR_BAD_ARG;
  if (loss_rows == nullptr && pred == nullptr && !(respect_skip & 4)) return ICAMD_ERR_BAD_ARG;
  return icamd_step_metrics_launch(loss_rows, pred, (const long long*)target, B, C, loss_out, finite_out, acc_f64, counts,
                                   loss_log, log_slot, log_stride, respect_skip, (hipStream_t)stream);
}

size_t icamd_grad_norm_workspace_bytes(void) { return 512 * sizeof(double); }

int icamd_grad_norm(const float* g, long long n, float inv_scale, float max_norm, void* workspace, float* out,
                    void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work(4.0 * n);
  if (g == nullptr || n <= 0 || workspace == nullptr || out == nullptr) return ICAMD_ERR_BAD_ARG;
  return icamd_grad_norm_launch(g, n, inv_scale, max_norm, (double*)workspace, out, (hipStream_t)stream);
}

int icamd_adamw_ema(float* p, float* g, float* m, float* v, float* ema, void* shadow, long long n, float lr, float wd,
                    float beta1, float beta2, float eps, int step, float gscale, float ema_decay, const float* clip,
                    const int32_t* finite_flag, int32_t* skipped_steps, int zero_grad, void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work((30.0 + (ema ? 8 : 0)) * n);
  if (p == nullptr || g == nullptr || m == nullptr || v == nullptr || n <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_adamw_ema_launch(p, g, m, v, ema, (bf16_t*)shadow, n, lr, wd, beta1, beta2, eps, step, gscale, ema_decay,
                                clip, finite_flag, skipped_steps, zero_grad, (hipStream_t)stream);
}

int icamd_grad_guard(float* g, long long n, const int32_t* finite_flag, void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work(0.0);
  if (g == nullptr || finite_flag == nullptr || n <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_grad_guard_launch(g, n, finite_flag, (hipStream_t)stream);
}

int icamd_optim_ema(int kind, float* p, float* g, float* m, float* v, float* ema, void* shadow, long long n, float lr,
                    float wd, float beta1, float beta2, float eps, int step, float gscale, float ema_decay,
                    const float* clip, const int32_t* finite_flag, int32_t* skipped_steps, int zero_grad, void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work((22.0 + (v ? 8 : 0) + (ema ? 8 : 0)) * n);
  if (p == nullptr || g == nullptr || m == nullptr || n <= 0) return ICAMD_ERR_BAD_ARG;
  if ((kind == ICAMD_OPT_ADAMW || kind == ICAMD_OPT_ADAM) && v == nullptr) return ICAMD_ERR_BAD_ARG;
  return icamd_optim_ema_launch(kind, p, g, m, v, ema, (bf16_t*)shadow, n, lr, wd, beta1, beta2, eps, step, gscale,
                                ema_decay, clip, finite_flag, skipped_steps, zero_grad, (hipStream_t)stream);
}

int icamd_lerp(float* dst, const float* src, long long n, float w, const int32_t* finite_flag, void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work(12.0 * n);
  if (dst == nullptr || src == nullptr || n <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_lerp_launch(dst, src, n, w, finite_flag, (hipStream_t)stream);
}

int icamd_f32_to_bf16(const float* src, void* dst, long long n, void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work(6.0 * n);
  if (src == nullptr || dst == nullptr || n <= 0) return ICAMD_ERR_BAD_ARG;
  return icamd_f32_to_bf16_launch(src, (bf16_t*)dst, n, (hipStream_t)stream);
}

int icamd_colsum(const void* x, int rows, int ld, int cols, float* out, int accumulate, void* stream) {
  ProfScope _prof(PC_MISC, stream);
  _prof.work(2.0 * rows * cols);
  if (x == nullptr || out == nullptr || rows <= 0 || cols <= 0 || ld < cols) return ICAMD_ERR_BAD_ARG;
  return icamd_colsum_launch((const bf16_t*)x, rows, ld, cols, out, accumulate, (hipStream_t)stream);
}

int icamd_fill_zero(void* ptr, size_t bytes, void* stream) {
  if (ptr == nullptr) return ICAMD_ERR_BAD_ARG;
  return hipMemsetAsync(ptr, 0, bytes, (hipStream_t)stream) == hipSuccess ? ICAMD_OK : ICAMD_ERR_LAUNCH;
}

}  // extern "C"
