// C-ABI entry points of the special-purpose convolutions: grouped 3x3, the thin 3x3 and 2x2 average pool of ResNet-D, the 7x7
// stem, the two fused bottleneck entries, BatchNorm folding into filters, the filter transposes and the depthwise 3x3 of MobileNetV2.
#include "capi_common.h"

extern "C" {

// ---- grouped 3x3 convolution (conv_grouped.hip).  Algorithmic work: x + y + filter bytes, 2 M C 9 Cg flops.
static bool gconv_ok(const icamd_conv_desc* d, int groups) {
  if (!conv_desc_ok(d) || groups <= 0) return false;
  if (d->KH != 3 || d->KW != 3 || d->pad != 1 || d->Cin != d->Cout) return false;
  return icamd_gconv3x3_ok(d->N, d->IH, d->IW, d->OH, d->OW, d->Cin, groups, d->stride);
}
static GConvParams gconv_params(const icamd_conv_desc* d, int groups) {
  GConvParams p;
  memset(&p, 0, sizeof(p));
  p.N = d->N; p.IH = d->IH; p.IW = d->IW; p.OH = d->OH; p.OW = d->OW; p.C = d->Cin; p.groups = groups; p.stride = d->stride;
  return p;
}
static void gconv_work(ProfScope& prof, const icamd_conv_desc* d, int groups, double filter_bytes_per_element) {
  if (d == nullptr || groups <= 0) return;
  const double wel = 9.0 * d->Cout * (d->Cin / groups);
  prof.work(2.0 * d->N * d->IH * d->IW * d->Cin + 2.0 * d->N * d->OH * d->OW * d->Cout + filter_bytes_per_element * wel,
            2.0 * d->N * d->OH * d->OW * wel);
}

int icamd_gconv3x3_supported(const icamd_conv_desc* d, int groups) { return gconv_ok(d, groups) ? 1 : 0; }

int icamd_gconv3x3_fwd(const icamd_conv_desc* d, int groups, const void* x, const void* w, void* y, float* stats, void* stream) {
  ProfScope _prof(PC_IGEMM_FWD, stream);
  gconv_work(_prof, d, groups, 2.0);
  if (d == nullptr || x == nullptr || w == nullptr || y == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!gconv_ok(d, groups)) return ICAMD_ERR_UNSUPPORTED;
  GConvParams p = gconv_params(d, groups);
  p.in = (const bf16_t*)x; p.w = (const bf16_t*)w; p.out = (bf16_t*)y; p.stats = stats;
  return icamd_gconv3x3_fwd_launch(p, (hipStream_t)stream);
}

int icamd_gconv3x3_fwd_act(const icamd_conv_desc* d, int groups, const void* x, const void* w, void* y, const float* bias, int relu,
                           void* stream) {
  ProfScope _prof(PC_IGEMM_FWD, stream);
  gconv_work(_prof, d, groups, 2.0);
  if (d == nullptr || x == nullptr || w == nullptr || y == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!gconv_ok(d, groups)) return ICAMD_ERR_UNSUPPORTED;
  GConvParams p = gconv_params(d, groups);
  p.in = (const bf16_t*)x; p.w = (const bf16_t*)w; p.out = (bf16_t*)y; p.bias = bias; p.relu = relu ? 1 : 0;
  return icamd_gconv3x3_fwd_launch(p, (hipStream_t)stream);
}

int icamd_gconv3x3_dgrad(const icamd_conv_desc* d, int groups, const void* dy, const void* w, void* dx, void* stream) {
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  gconv_work(_prof, d, groups, 2.0);
  if (d == nullptr || dy == nullptr || w == nullptr || dx == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!gconv_ok(d, groups)) return ICAMD_ERR_UNSUPPORTED;
  GConvParams p = gconv_params(d, groups);
  p.in = (const bf16_t*)dy; p.w = (const bf16_t*)w; p.out = (bf16_t*)dx;
  return icamd_gconv3x3_dgrad_launch(p, (hipStream_t)stream);
}

size_t icamd_gconv3x3_wgrad_workspace_bytes(const icamd_conv_desc* d, int groups) {
  if (!gconv_ok(d, groups)) return 0;
  return icamd_gconv3x3_wgrad_bytes(d->N, d->IH, d->IW, d->OH, d->OW, d->Cin, groups, d->stride);
}

int icamd_gconv3x3_wgrad(const icamd_conv_desc* d, int groups, const void* x, const void* dy, float* dw, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_WGRAD, stream);
  gconv_work(_prof, d, groups, 4.0);
  if (d == nullptr || x == nullptr || dy == nullptr || dw == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!gconv_ok(d, groups)) return ICAMD_ERR_UNSUPPORTED;
  const size_t need = icamd_gconv3x3_wgrad_workspace_bytes(d, groups);
  if (workspace == nullptr || need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  GConvParams p = gconv_params(d, groups);
  p.in = (const bf16_t*)x; p.dy = (const bf16_t*)dy; p.slab = (float*)workspace;
  const int rc = icamd_gconv3x3_wgrad_launch(p, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_slab_reduce_launch(p.slab, dw, (long long)d->Cin * 9 * (d->Cin / groups), p.S, accumulate, (hipStream_t)stream);
}

// ---- ResNet-D: 2x2 average pool of the shortcut and the thin 3x3 convolutions of the deep stem (conv_stem_deep.hip).  Arguments are
// validated before any profiling work is booked.
int icamd_avgpool2x2_fwd(const void* x, void* out, int N, int IH, int IW, int C, void* stream) {
  if (x == nullptr || out == nullptr || !icamd_avgpool2x2_ok(N, IH, IW, C)) return ICAMD_ERR_BAD_ARG;
  ProfScope _prof(PC_POOL, stream);
  _prof.work(2.0 * N * IH * IW * C + 2.0 * N * ((IH + 1) / 2) * ((IW + 1) / 2) * C);
  Pool2x2Params p;
  memset(&p, 0, sizeof(p));
  p.in = (const bf16_t*)x; p.out = (bf16_t*)out; p.N = N; p.IH = IH; p.IW = IW; p.C8 = C / 8;
  return icamd_avgpool2x2_launch(p, 0, (hipStream_t)stream);
}

int icamd_avgpool2x2_bwd(const void* dout, const void* addend, void* dx, int N, int IH, int IW, int C, void* stream) {
  if (dout == nullptr || dx == nullptr || !icamd_avgpool2x2_ok(N, IH, IW, C)) return ICAMD_ERR_BAD_ARG;
  ProfScope _prof(PC_POOL, stream);
  _prof.work((addend ? 4.0 : 2.0) * N * IH * IW * C + 2.0 * N * ((IH + 1) / 2) * ((IW + 1) / 2) * C);
  Pool2x2Params p;
  memset(&p, 0, sizeof(p));
  p.in = (const bf16_t*)dout; p.addend = (const bf16_t*)addend; p.out = (bf16_t*)dx; p.N = N; p.IH = IH; p.IW = IW; p.C8 = C / 8;
  return icamd_avgpool2x2_launch(p, 1, (hipStream_t)stream);
}

static bool thin_ok(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d)) return false;
  if (d->KH != 3 || d->KW != 3 || d->pad != 1 || d->stride != 1) return false;
  return icamd_thin3x3_ok(d->N, d->IH, d->IW, d->Cin, d->Cout);
}
static ThinConvParams thin_params(const icamd_conv_desc* d) {
  ThinConvParams p;
  memset(&p, 0, sizeof(p));
  p.N = d->N; p.H = d->IH; p.W = d->IW; p.Cout = d->Cout;
  return p;
}
static void thin_work(ProfScope& prof, const icamd_conv_desc* d, double filter_bytes_per_element) {
  const ConvWork cw = conv_work(d);
  prof.work(cw.in + cw.out + filter_bytes_per_element * cw.w, cw.flops);
}

int icamd_conv3x3_thin_supported(const icamd_conv_desc* d) { return thin_ok(d) ? 1 : 0; }

int icamd_conv3x3_thin_stats_rows(const icamd_conv_desc* d) {
  return thin_ok(d) ? icamd_thin3x3_stats_rows(d->N, d->IH, d->IW, d->Cout) : 0;
}

int icamd_conv3x3_thin_fwd(const icamd_conv_desc* d, const void* x, const void* w, void* y, const float* bias, float* stats, int relu,
                           void* stream) {
  if (d == nullptr || x == nullptr || w == nullptr || y == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!thin_ok(d)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_IGEMM_FWD, stream);
  thin_work(_prof, d, 2.0);
  ThinConvParams p = thin_params(d);
  p.in = (const bf16_t*)x; p.w = (const bf16_t*)w; p.out = (bf16_t*)y; p.bias = bias; p.stats = stats; p.relu = relu ? 1 : 0;
  return icamd_thin3x3_fwd_launch(p, (hipStream_t)stream);
}

int icamd_conv3x3_thin_dgrad(const icamd_conv_desc* d, const void* dy, const void* w, void* dx, void* stream) {
  if (d == nullptr || dy == nullptr || w == nullptr || dx == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!thin_ok(d)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  thin_work(_prof, d, 2.0);
  ThinConvParams p = thin_params(d);
  p.in = (const bf16_t*)dy; p.w = (const bf16_t*)w; p.out = (bf16_t*)dx;
  return icamd_thin3x3_dgrad_launch(p, (hipStream_t)stream);
}

size_t icamd_conv3x3_thin_wgrad_workspace_bytes(const icamd_conv_desc* d) {
  return thin_ok(d) ? icamd_thin3x3_wgrad_bytes(d->N, d->IH, d->IW, d->Cout) : 0;
}

int icamd_conv3x3_thin_wgrad(const icamd_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (d == nullptr || x == nullptr || dy == nullptr || dw == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!thin_ok(d)) return ICAMD_ERR_UNSUPPORTED;
  const size_t need = icamd_conv3x3_thin_wgrad_workspace_bytes(d);
  if (workspace == nullptr || need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_WGRAD, stream);
  thin_work(_prof, d, 4.0);
  ThinConvParams p = thin_params(d);
  p.in = (const bf16_t*)x; p.dy = (const bf16_t*)dy; p.slab = (float*)workspace;
  const int rc = icamd_thin3x3_wgrad_launch(p, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_slab_reduce_launch(p.slab, dw, (long long)d->Cout * 9 * 32, p.S, accumulate, (hipStream_t)stream);
}

// ---- ResNet stem: 7x7 stride 2 pad 3 convolution on the rgb4 layout ------------------------------------------------
static bool stem_shape_ok(int N, int H, int W, int Cout) {
  return N > 0 && H >= 7 && W >= 8 && W % 2 == 0 && Cout > 0 && Cout % 8 == 0 && (long long)N * H * (W + 8) * 4 < (1ll << 31);
}

int icamd_stem7x7s2_stats_rows(int N, int H, int W) {
  const long long M = (long long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
  return (int)((M + 127) / 128);
}

int icamd_stem7x7s2_fwd(const void* x4, const void* w, void* y, const float* bias, float* stats, int relu, int N, int H,
                        int W, int Cout, void* stream) {
  ProfScope _prof(PC_IGEMM_FWD, stream);
  {   // rgb4 layout in, [N][OH][OW][Cout] out, [Cout][8][8][4] filters; 147 real taps per output
    const double oh = (H - 1) / 2 + 1, ow = (W - 1) / 2 + 1;
    _prof.work(8.0 * N * H * (W + 8) + 2.0 * N * oh * ow * Cout + 512.0 * Cout, 2.0 * N * oh * ow * Cout * 147);
  }
  if (x4 == nullptr || w == nullptr || y == nullptr || !stem_shape_ok(N, H, W, Cout)) return ICAMD_ERR_BAD_ARG;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;   // (H + 6 - 7) / 2 + 1
  if ((long long)N * OH * OW >= (1ll << 31)) return ICAMD_ERR_UNSUPPORTED;
  // conv_stem.hip: the training form (statistics) and, round 4, the inference form (bias + ReLU, no statistics)
  if ((stats == nullptr || (bias == nullptr && !relu)) && icamd_stem_resident_wanted(N, H, W, Cout)) {
    StemParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.x = (const bf16_t*)x4; sp.w = (const bf16_t*)w; sp.y = (bf16_t*)y; sp.stats = stats; sp.N = N; sp.H = H; sp.W = W;
    sp.bias = bias; sp.relu = relu;
    return icamd_stem_resident_launch(sp, (hipStream_t)stream);
  }
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.in = (const bf16_t*)x4; p.wt = (const bf16_t*)w; p.out = (bf16_t*)y; p.bias = bias; p.stats = stats; p.relu = relu;
  p.N = N; p.IH = H; p.IW = W + 8; p.Cin = 4;              // IW: padded row pitch in pixels; Cin: elements per pixel
  p.OH = OH; p.OW = OW; p.Cout = Cout;
  p.P = OH; p.Q = OW; p.M = N * OH * OW;
  p.ostr = 1; p.istr = 2;
  p.ntaps = 1; p.Ktot = 256; p.KW = 1; p.tap_sign = 1; p.regular_taps = 1;
  p.stem7 = 1;
  return icamd_igemm_launch(p, (hipStream_t)stream);
}

size_t icamd_stem7x7s2_wgrad_workspace_bytes(int N, int H, int W, int Cout) {
  if (!stem_shape_ok(N, H, W, Cout)) return 0;
  const long long M = (long long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
  if (M >= (1ll << 30)) return 0;
  int S = 1, rows = 0;
  icamd_wgrad_plan((int)M, Cout, 256, &S, &rows);
  if (icamd_stem_resident_wanted(N, H, W, Cout)) {
    const int S2 = icamd_stem_wgrad_resident_splits(N, H);
    if (S2 > S) S = S2;
  }
  return (size_t)S * Cout * (256 + 1) * sizeof(float);
}

int icamd_stem7x7s2_wgrad(const void* x4, const void* dy, float* dw, int accumulate, void* workspace, size_t workspace_bytes,
                          int N, int H, int W, int Cout, void* stream) {
  ProfScope _prof(PC_WGRAD, stream);
  {
    const double oh = (H - 1) / 2 + 1, ow = (W - 1) / 2 + 1;
    _prof.work(8.0 * N * H * (W + 8) + 2.0 * N * oh * ow * Cout + 1024.0 * Cout, 2.0 * N * oh * ow * Cout * 147);
  }
  if (x4 == nullptr || dy == nullptr || dw == nullptr || workspace == nullptr) return ICAMD_ERR_BAD_ARG;
  const size_t need = icamd_stem7x7s2_wgrad_workspace_bytes(N, H, W, Cout);
  if (need == 0) return ICAMD_ERR_BAD_ARG;
  if (workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  if (icamd_stem_resident_wanted(N, H, W, Cout)) {   // conv_stem.hip
    StemWgradParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.x = (const bf16_t*)x4; sp.dy = (const bf16_t*)dy; sp.slab = (float*)workspace; sp.N = N; sp.H = H; sp.W = W;
    const int S = icamd_stem_wgrad_resident_splits(N, H);
    const int rc = icamd_stem_wgrad_resident_launch(sp, S, (hipStream_t)stream);
    if (rc) return rc;
    return icamd_slab_reduce_launch(sp.slab, dw, (long long)Cout * 256, S, accumulate, (hipStream_t)stream, 1);
  }
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const bf16_t*)x4; p.dy = (const bf16_t*)dy; p.slab = (float*)workspace;
  p.N = N; p.IH = H; p.IW = W + 8; p.Cin = 4; p.OH = (H - 1) / 2 + 1; p.OW = (W - 1) / 2 + 1; p.Cout = Cout;
  p.KH = 8; p.KW = 8; p.stride = 2; p.pad = 3;
  p.M = N * p.OH * p.OW; p.Ktot = 256;
  p.stem7 = 1;
  icamd_wgrad_plan(p.M, p.Cout, p.Ktot, &p.S, &p.rows_per_split);
  int rc = icamd_wgrad_launch(p, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_slab_reduce_launch(p.slab, dw, (long long)p.Cout * p.Ktot, p.S, accumulate, (hipStream_t)stream, 1);
}

// ---- fused forward across a bottleneck boundary (conv_fused_fwd.hip) --------------------------------------------------
int icamd_bn_apply_conv1x1_fused_supported(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d) || d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0) return 0;
  return icamd_bn_apply_conv1x1_fused_wanted((long long)d->N * d->OH * d->OW, d->Cin, d->Cout) ? 1 : 0;
}

int icamd_bn_apply_conv1x1_fused(const icamd_conv_desc* d, const void* y, const float* scale, const float* shift,
                                 const void* residual, const float* res_scale, const float* res_shift, void* out,
                                 uint8_t* maskbits, const void* w, void* y1, float* stats, void* stream) {
  ProfScope _prof(PC_FUSED_FWD, stream);
  if (d != nullptr) {
    const ConvWork cw = conv_work(d);
    _prof.work(3.0 * cw.in + cw.in / 16 + cw.out + 2 * cw.w, cw.flops);   // y, residual read, out + mask written; y1 written
  }
  if (y == nullptr || scale == nullptr || shift == nullptr || residual == nullptr || out == nullptr || maskbits == nullptr ||
      w == nullptr || y1 == nullptr || (res_scale == nullptr) != (res_shift == nullptr))
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_bn_apply_conv1x1_fused_supported(d)) return ICAMD_ERR_UNSUPPORTED;
  FusedFwdParams p;
  memset(&p, 0, sizeof(p));
  p.y = (const bf16_t*)y; p.res = (const bf16_t*)residual; p.scale = scale; p.shift = shift; p.res_scale = res_scale;
  p.res_shift = res_shift; p.out = (bf16_t*)out; p.maskbits = maskbits; p.w = (const bf16_t*)w; p.y1 = (bf16_t*)y1; p.stats = stats;
  p.M = d->N * d->OH * d->OW; p.K = d->Cin; p.N = d->Cout;
  return icamd_bn_apply_conv1x1_fused_launch(p, (hipStream_t)stream);
}

// ---- fused backward of "pointwise convolution -> BatchNorm" (conv_fused_bwd.hip) -----------------------------------------
int icamd_conv1x1_bn_bwd_fused_supported(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d) || d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0) return 0;
  return icamd_conv1x1_bn_bwd_fused_wanted((long long)d->N * d->OH * d->OW, d->Cin, d->Cout) ? 1 : 0;
}

size_t icamd_conv1x1_bn_bwd_fused_workspace_bytes(const icamd_conv_desc* d) {
  if (!icamd_conv1x1_bn_bwd_fused_supported(d)) return 0;
  int S = 1, rows = 0;
  icamd_conv1x1_bn_bwd_fused_plan(d->N * d->OH * d->OW, d->Cin, &S, &rows);
  return (size_t)S * d->Cout * d->Cin * sizeof(float);
}

int icamd_conv1x1_bn_bwd_fused(const icamd_conv_desc* d, const float* partials, int nrows, const void* g, const void* y,
                               const float* mean, const float* invstd, const float* scale, float* dgamma, float* dbeta,
                               const void* x, const void* w_t, void* dx, float* dw, int accumulate, void* bn_workspace,
                               size_t bn_workspace_bytes, void* wgrad_workspace, size_t wgrad_workspace_bytes, void* stream) {
  ProfScope _prof(PC_FUSED_BWD, stream);
  if (d != nullptr) {
    const ConvWork cw = conv_work(d);
    // g, y read (twice when the sums are formed here); x read, dx written; dw
    _prof.work((partials ? 2.0 : 4.0) * cw.out + 2.0 * cw.in + 4.0 * cw.w + (partials ? 8.0 * nrows * d->Cout : 0.0), 2.0 * cw.flops);
  }
  if ((partials != nullptr && nrows <= 0) || g == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || scale == nullptr ||
      dgamma == nullptr || dbeta == nullptr || x == nullptr || w_t == nullptr || dx == nullptr || dw == nullptr ||
      bn_workspace == nullptr || wgrad_workspace == nullptr)
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_conv1x1_bn_bwd_fused_supported(d)) return ICAMD_ERR_UNSUPPORTED;
  const int C = d->Cout;
  const long long M = (long long)d->N * d->OH * d->OW;
  if (bn_workspace_bytes < (partials ? icamd_bn_bwd_apply_workspace_bytes(C) : icamd_bn_bwd_workspace_bytes(M, C)) ||
      wgrad_workspace_bytes < icamd_conv1x1_bn_bwd_fused_workspace_bytes(d))
    return ICAMD_ERR_WORKSPACE;
  // the workspace of icamd_bn_bwd_from_gy_partials, or (no sums yet) of icamd_bn_bwd
  const ReduceWs w = reduce_ws(bn_workspace, C, partials ? 0 : bn_bwd_blocks(M, C), 2);
  float* c1c2 = w.scratch;
  int rc;
  if (partials != nullptr) {
    // (sum g, sum g * y) rows left by icamd_conv2d_dgrad_bnred
    rc = icamd_bn_bwd_finalize_launch(partials, nrows, mean, invstd, dgamma, dbeta, M, C, accumulate, w.chunks, c1c2, (hipStream_t)stream, 1);
  } else {
    // the reduce pass of icamd_bn_bwd over the (already masked) g and y first
    int nb = 0;
    rc = icamd_bn_bwd_reduce_launch((const bf16_t*)g, (const bf16_t*)y, mean, invstd, w.part, M, C, &nb, (hipStream_t)stream);
    if (rc) return rc;
    rc = icamd_bn_bwd_finalize_launch(w.part, nb, mean, invstd, dgamma, dbeta, M, C, accumulate, w.chunks, c1c2, (hipStream_t)stream, 0);
  }
  if (rc) return rc;
  FusedBwdParams p;
  memset(&p, 0, sizeof(p));
  p.g = (const bf16_t*)g; p.y = (const bf16_t*)y; p.x = (const bf16_t*)x; p.wt = (const bf16_t*)w_t; p.dx = (bf16_t*)dx;
  p.slab = (float*)wgrad_workspace;
  p.mean = mean; p.invstd = invstd; p.scale = scale; p.c1 = c1c2; p.c2 = c1c2 + C;
  p.M = (int)M; p.CI = d->Cin; p.CO = C;
  rc = icamd_conv1x1_bn_bwd_fused_launch(p, (hipStream_t)stream);
  if (rc) return rc;
  return icamd_slab_reduce_launch(p.slab, dw, (long long)C * d->Cin, p.S, accumulate, (hipStream_t)stream);
}

int icamd_bn_fold_filters(const float* w, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, int Cout, int K, void* w_folded, float* shift,
                          void* stream) {
  ProfScope _prof(PC_BN_FINALIZE, stream);
  _prof.work(6.0 * Cout * K);
  if (w == nullptr || gamma == nullptr || beta == nullptr || running_mean == nullptr || running_var == nullptr ||
      w_folded == nullptr || shift == nullptr || Cout <= 0 || K <= 0)
    return ICAMD_ERR_BAD_ARG;
  return icamd_bn_fold_launch(w, gamma, beta, running_mean, running_var, eps, Cout, K, (bf16_t*)w_folded, shift,
                              (hipStream_t)stream);
}

int icamd_filter_transpose(const void* src_base, void* dst_base, const int64_t* descs, const int32_t* jobs, int njobs,
                           void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work(4.0 * 4096 * njobs);
  if (src_base == nullptr || dst_base == nullptr || descs == nullptr || jobs == nullptr || njobs < 0) return ICAMD_ERR_BAD_ARG;
  return icamd_filter_transpose_launch((const bf16_t*)src_base, (bf16_t*)dst_base, (const long long*)descs, jobs, njobs,
                                       (hipStream_t)stream);
}

int icamd_filter_transpose_tiled(const void* src_base, void* dst_base, const int64_t* descs, const int32_t* jobs, int njobs,
                                 void* stream) {
  ProfScope _prof(PC_OPTIM, stream);
  _prof.work(4.0 * 4096 * njobs);
  if (src_base == nullptr || dst_base == nullptr || descs == nullptr || jobs == nullptr || njobs < 0) return ICAMD_ERR_BAD_ARG;
  return icamd_filter_transpose_tiled_launch((const bf16_t*)src_base, (bf16_t*)dst_base, (const long long*)descs, jobs, njobs,
                                             (hipStream_t)stream);
}

// ---- depthwise 3x3, pad 1, stride 1 / 2 (dwconv3x3.hip).  Arguments are validated before any profiling work is booked.
int icamd_dwconv3_supported(int N, int H, int W, int C, int stride) { return icamd_dwconv3_ok(N, H, W, C, stride) ? 1 : 0; }

int icamd_dwconv3_stats_rows(int N, int H, int W, int C, int stride) { return (int)icamd_dwconv3_stats_rows_cxx(N, H, W, C, stride); }

static double dw3_out_elements(int N, int H, int W, int C, int stride) {
  return (double)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1) * C;
}

int icamd_dwconv3_fwd(const void* x, const float* in_scale, const float* in_shift, const void* w, void* y, float* stats, int N, int H,
                      int W, int C, int stride, void* stream) {
  if (x == nullptr || w == nullptr || y == nullptr || (in_scale == nullptr) != (in_shift == nullptr)) return ICAMD_ERR_BAD_ARG;
  if (!icamd_dwconv3_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_DWCONV, stream);
  const double out = dw3_out_elements(N, H, W, C, stride);
  _prof.work(2.0 * N * H * W * C + 2.0 * out + (stats ? 8.0 * icamd_dwconv3_stats_rows_cxx(N, H, W, C, stride) * C : 0.0), 18.0 * out);
  return icamd_dwconv3_fwd_launch((const bf16_t*)x, in_scale, in_shift, (const bf16_t*)w, (bf16_t*)y, stats, N, H, W, C, stride, 0,
                                  (hipStream_t)stream);
}

int icamd_dwconv3_dgrad(const void* dy, const void* w, void* dx, int N, int H, int W, int C, int stride, void* stream) {
  if (dy == nullptr || w == nullptr || dx == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!icamd_dwconv3_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_DWCONV, stream);
  const double out = dw3_out_elements(N, H, W, C, stride);
  _prof.work(2.0 * N * H * W * C + 2.0 * out, 18.0 * out);
  return icamd_dwconv3_dgrad_launch((const bf16_t*)dy, (const bf16_t*)w, (bf16_t*)dx, N, H, W, C, stride, (hipStream_t)stream);
}

size_t icamd_dwconv3_wgrad_workspace_bytes(int N, int H, int W, int C, int stride) {
  return (size_t)icamd_dwconv3_wgrad_rows(N, H, W, C, stride) * 9 * C * sizeof(float);   // one region: [rows][9][C]
}

int icamd_dwconv3_wgrad(const void* x, const float* in_scale, const float* in_shift, const void* dy, float* dw, int accumulate,
                        void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int stride, void* stream) {
  if (x == nullptr || dy == nullptr || dw == nullptr || workspace == nullptr || (in_scale == nullptr) != (in_shift == nullptr))
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_dwconv3_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  const size_t need = icamd_dwconv3_wgrad_workspace_bytes(N, H, W, C, stride);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_DWCONV, stream);
  const double out = dw3_out_elements(N, H, W, C, stride);
  _prof.work(2.0 * N * H * W * C + 2.0 * out + 2.0 * need, 18.0 * out);
  return icamd_dwconv3_wgrad_launch((const bf16_t*)x, in_scale, in_shift, (const bf16_t*)dy, (float*)workspace, dw, N, H, W, C, stride,
                                    accumulate, (hipStream_t)stream);
}

// ---- depthwise 5x5, pad 2, stride 1 / 2 (dwconv5x5.hip).  Arguments are validated before any profiling work is booked.
int icamd_dwconv5_supported(int N, int H, int W, int C, int stride) { return icamd_dwconv5_ok(N, H, W, C, stride) ? 1 : 0; }

int icamd_dwconv5_stats_rows(int N, int H, int W, int C, int stride) { return (int)icamd_dwconv5_stats_rows_cxx(N, H, W, C, stride); }

int icamd_dwconv5_fwd(const void* x, const void* w, void* y, float* stats, int N, int H, int W, int C, int stride, void* stream) {
  if (x == nullptr || w == nullptr || y == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!icamd_dwconv5_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_DWCONV, stream);
  const double out = dw3_out_elements(N, H, W, C, stride);
  _prof.work(2.0 * N * H * W * C + 2.0 * out + (stats ? 8.0 * icamd_dwconv5_stats_rows_cxx(N, H, W, C, stride) * C : 0.0), 50.0 * out);
  return icamd_dwconv5_fwd_launch((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, stats, N, H, W, C, stride, 0, (hipStream_t)stream);
}

int icamd_dwconv5_dgrad(const void* dy, const void* w, void* dx, int N, int H, int W, int C, int stride, void* stream) {
  if (dy == nullptr || w == nullptr || dx == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!icamd_dwconv5_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  ProfScope _prof(PC_DWCONV, stream);
  const double out = dw3_out_elements(N, H, W, C, stride);
  _prof.work(2.0 * N * H * W * C + 2.0 * out, 50.0 * out);
  return icamd_dwconv5_dgrad_launch((const bf16_t*)dy, (const bf16_t*)w, (bf16_t*)dx, N, H, W, C, stride, (hipStream_t)stream);
}

size_t icamd_dwconv5_wgrad_workspace_bytes(int N, int H, int W, int C, int stride) {
  return (size_t)icamd_dwconv5_wgrad_rows(N, H, W, C, stride) * 25 * C * sizeof(float);   // one region: [rows][25][C]
}

int icamd_dwconv5_wgrad(const void* x, const void* dy, float* dw, int accumulate, void* workspace, size_t workspace_bytes, int N, int H,
                        int W, int C, int stride, void* stream) {
  if (x == nullptr || dy == nullptr || dw == nullptr || workspace == nullptr) return ICAMD_ERR_BAD_ARG;
  if (!icamd_dwconv5_ok(N, H, W, C, stride)) return ICAMD_ERR_UNSUPPORTED;
  const size_t need = icamd_dwconv5_wgrad_workspace_bytes(N, H, W, C, stride);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  ProfScope _prof(PC_DWCONV, stream);
  const double out = dw3_out_elements(N, H, W, C, stride);
  _prof.work(2.0 * N * H * W * C + 2.0 * out + 2.0 * need, 50.0 * out);
  return icamd_dwconv5_wgrad_launch((const bf16_t*)x, (const bf16_t*)dy, (float*)workspace, dw, N, H, W, C, stride, accumulate,
                                    (hipStream_t)stream);
}

}  // extern "C"
