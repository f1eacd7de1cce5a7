// C-ABI entry points (include/icamd.h): argument checks + translation into kernel launch parameters.  This unit: ABI version,
// the profiler, and the dense convolution family with its forward / data-gradient / weight-gradient routing.  The other
// entries live in capi_conv_special.hip, capi_norm.hip, capi_tokens.hip and capi_step.hip.
#include "capi_common.h"

// the profiler state (declared in capi_common.h)
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e; (void)hipEventCreate(&e); return e;
}

extern "C" {

int icamd_abi_version(void) { return 6; }

int icamd_prof_enable(int on) { g_prof_on = on != 0; return ICAMD_OK; }
int icamd_prof_classes(void) { return PC_COUNT; }
// Synchronises the recorded events, adds per-class elapsed ms / call counts into the arrays, clears the log.
int icamd_prof_collect(double* ms, long long* calls, double* bytes, double* flops, int n) {
  if (ms == nullptr || calls == nullptr || n < PC_COUNT) return ICAMD_ERR_BAD_ARG;
  for (auto& r : g_prof_recs) {
    (void)hipEventSynchronize(r.b);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, r.a, r.b);
    ms[r.cls] += (double)t;
    calls[r.cls] += 1;
    if (bytes != nullptr) bytes[r.cls] += r.bytes;
    if (flops != nullptr) flops[r.cls] += r.flops;
    g_prof_pool.push_back(r.a);
    g_prof_pool.push_back(r.b);
  }
  g_prof_recs.clear();
  return ICAMD_OK;
}

int icamd_conv2d_stats_rows(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d)) return 0;
  const long long M = (long long)d->N * d->OH * d->OW;
  return (int)((M + 127) / 128);
}

static int conv_fwd_impl(const icamd_conv_desc* d, const void* x, const void* w, void* y, const float* bias,
                         const void* addend, float* stats, int relu, void* stream, void* gelu_out = nullptr,
                         int gelu_inplace = 0) {
  if (!conv_desc_ok(d) || x == nullptr || w == nullptr || y == nullptr) return ICAMD_ERR_BAD_ARG;
  if ((long long)d->N * d->OH * d->OW >= (1ll << 31)) return ICAMD_ERR_UNSUPPORTED;
  if (d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && addend == nullptr && gelu_out == nullptr &&
      !gelu_inplace && icamd_halo3x3_wanted(d->N, d->IH, d->IW, d->Cin, d->Cout)) {
    Halo3x3Params h;
    memset(&h, 0, sizeof(h));
    h.in = (const bf16_t*)x; h.wt = (const bf16_t*)w; h.out = (bf16_t*)y; h.bias = bias; h.stats = stats; h.relu = relu;
    h.N = d->N; h.H = d->IH; h.W = d->IW; h.C = d->Cin; h.Cout = d->Cout;
    return icamd_halo3x3_launch(h, (hipStream_t)stream);
  }
  // round 5: a 1x1 / stride-2 convolution (ResNet's projection shortcuts) is the same pointwise problem on the rows (n, 2 oh, 2 ow):
  // the register-resident kernel gathers them in its LDS-DMA staging
  const bool pw_gather = d->KH == 1 && d->KW == 1 && d->stride == 2 && d->pad == 0 && addend == nullptr;
  if (d->KH == 1 && d->KW == 1 && (d->stride == 1 || pw_gather) && d->pad == 0 && bias == nullptr && addend == nullptr && !relu &&
      gelu_out == nullptr && !gelu_inplace && icamd_pw_resident_wanted((long long)d->N * d->OH * d->OW, d->Cout, d->Cin)) {
    PwResidentParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)x; g.B = (const bf16_t*)w; g.out = (bf16_t*)y; g.stats = stats;
    g.M = d->N * d->OH * d->OW; g.N = d->Cout; g.K = d->Cin;
    if (pw_gather) { g.gat_oh = d->OH; g.gat_ow = d->OW; g.gat_ih = d->IH; g.gat_iw = d->IW; }
    return icamd_pw_resident_launch(g, (hipStream_t)stream);
  }
  // evaluate()'s BatchNorm-folded forward (bias = the folded shift, optional residual addend, ReLU): the same register-resident
  // kernel with the inference epilogue (round 4; these launches ran on conv_igemm's single-stage tiles before)
  if (d->KH == 1 && d->KW == 1 && (d->stride == 1 || pw_gather) && d->pad == 0 && (bias != nullptr || relu) && stats == nullptr &&
      gelu_out == nullptr && !gelu_inplace &&
      icamd_pw_resident_wanted((long long)d->N * d->OH * d->OW, d->Cout, d->Cin, addend != nullptr)) {
    PwResidentParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)x; g.B = (const bf16_t*)w; g.out = (bf16_t*)y; g.bias = bias; g.relu = relu;
    g.addend = (const bf16_t*)addend;
    g.M = d->N * d->OH * d->OW; g.N = d->Cout; g.K = d->Cin;
    if (pw_gather) { g.gat_oh = d->OH; g.gat_ow = d->OW; g.gat_ih = d->IH; g.gat_iw = d->IW; }
    return icamd_pw_resident_launch(g, (hipStream_t)stream);
  }
  if (d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && addend == nullptr && !relu && stats == nullptr &&
      icamd_pw_resident_ext_wanted((long long)d->N * d->OH * d->OW, d->Cout, d->Cin)) {
    PwResidentParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)x; g.B = (const bf16_t*)w; g.out = (bf16_t*)y; g.bias = bias;
    g.gelu_out = (bf16_t*)gelu_out; g.gelu_inplace = gelu_inplace;
    g.M = d->N * d->OH * d->OW; g.N = d->Cout; g.K = d->Cin;
    return icamd_pw_resident_ext_launch(g, (hipStream_t)stream);
  }
  if (d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 &&
      icamd_gemm_nt_wanted((long long)d->N * d->OH * d->OW, d->Cout, d->Cin)) {
    GemmNtParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)x; g.B = (const bf16_t*)w; g.out = (bf16_t*)y; g.addend = (const bf16_t*)addend; g.bias = bias;
    g.stats = stats;
    g.M = d->N * d->OH * d->OW; g.N = d->Cout; g.K = d->Cin; g.relu = relu; g.gelu_out = (bf16_t*)gelu_out; g.gelu_inplace = gelu_inplace;
    return icamd_gemm_nt_launch(g, (hipStream_t)stream);
  }
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.in = (const bf16_t*)x; p.wt = (const bf16_t*)w; p.out = (bf16_t*)y;
  p.addend = (const bf16_t*)addend; p.bias = bias; p.stats = stats; p.relu = relu; p.gelu_out = (bf16_t*)gelu_out; p.gelu_inplace = gelu_inplace;
  p.N = d->N; p.IH = d->IH; p.IW = d->IW; p.Cin = d->Cin;
  p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout;
  p.P = d->OH; p.Q = d->OW; p.M = d->N * d->OH * d->OW;
  p.ostr = 1; p.ooff_h = 0; p.ooff_w = 0; p.istr = d->stride;
  p.ntaps = d->KH * d->KW; p.Ktot = p.ntaps * d->Cin;
  p.KW = d->KW; p.pad = d->pad; p.tap_sign = 1; p.regular_taps = 1;
  if (p.ntaps <= ICAMD_MAX_TAPS)
    for (int r = 0; r < d->KH; ++r)
      for (int s = 0; s < d->KW; ++s) {
        const int t = r * d->KW + s;
        p.dh[t] = (short)(r - d->pad); p.dw[t] = (short)(s - d->pad); p.wtap[t] = (short)t;
      }
  return icamd_igemm_launch(p, (hipStream_t)stream);
}

int icamd_conv2d_fwd(const icamd_conv_desc* d, const void* x, const void* w, void* y, const float* bias,
                     const void* addend, float* stats, void* stream) {
  ProfScope _prof(PC_IGEMM_FWD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.in + cw.out + 2 * cw.w + (addend ? cw.out : 0), cw.flops);
  return conv_fwd_impl(d, x, w, y, bias, addend, stats, 0, stream);
}

int icamd_conv2d_fwd_act(const icamd_conv_desc* d, const void* x, const void* w, void* y, const float* bias,
                         const void* addend, int relu, void* stream) {
  ProfScope _prof(PC_IGEMM_FWD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.in + cw.out + 2 * cw.w + (addend ? cw.out : 0), cw.flops);
  return conv_fwd_impl(d, x, w, y, bias, addend, nullptr, relu ? 1 : 0, stream);
}

int icamd_conv2d_fwd_gelu(const icamd_conv_desc* d, const void* x, const void* w, void* z, void* a, const float* bias,
                          void* stream) {
  ProfScope _prof(PC_IGEMM_FWD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.in + (z ? cw.out : 0) + cw.out + 2 * cw.w, cw.flops);
  if (a == nullptr) return ICAMD_ERR_BAD_ARG;
  if (z == nullptr) return conv_fwd_impl(d, x, w, a, bias, nullptr, nullptr, 0, stream, nullptr, /*gelu_inplace=*/1);
  return conv_fwd_impl(d, x, w, z, bias, nullptr, nullptr, 0, stream, a);
}

static int dgrad_impl(const icamd_conv_desc* d, const void* dy, const void* w_t, void* dx, const void* addend,
                      const uint8_t* addend_bits, const icamd_bn_bwd_fuse* f, void* stream, const void* gelu_z = nullptr,
                      int addend_sub2 = 0) {
  if (!conv_desc_ok(d) || dy == nullptr || w_t == nullptr || dx == nullptr) return ICAMD_ERR_BAD_ARG;
  if (d->Cout % 8 != 0 || d->Cin % 8 != 0) return ICAMD_ERR_UNSUPPORTED;
  if ((long long)d->N * d->IH * d->IW >= (1ll << 31)) return ICAMD_ERR_UNSUPPORTED;
  const int st = d->stride;
  // (ICAMD_PW_RESIDENT=5: the residual / even-grid addend launches stay on conv_igemm -- the A/B switch for the
  // LDS-DMA-staged addend of conv1x1_resident.hip)
  const bool pw_addend = icamd_pw_resident_mode() != 5;
  if (d->KH == 1 && d->KW == 1 && st == 1 && d->pad == 0 && f == nullptr && gelu_z == nullptr &&
      (addend == nullptr || pw_addend) && !(addend_bits != nullptr && addend_sub2) &&
      icamd_pw_resident_wanted((long long)d->N * d->IH * d->IW, d->Cin, d->Cout, addend != nullptr)) {
    PwResidentParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)dy; g.B = (const bf16_t*)w_t; g.out = (bf16_t*)dx; g.addend = (const bf16_t*)addend;
    g.addend_bits = addend_bits;
    g.M = d->N * d->IH * d->IW; g.N = d->Cin; g.K = d->Cout;
    if (addend_sub2) { g.sub2_h = d->IH; g.sub2_w = d->IW; }
    return icamd_pw_resident_launch(g, (hipStream_t)stream);
  }
  if (d->KH == 1 && d->KW == 1 && st == 1 && d->pad == 0 && f == nullptr && addend == nullptr &&
      icamd_pw_resident_ext_wanted((long long)d->N * d->IH * d->IW, d->Cin, d->Cout)) {
    PwResidentParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)dy; g.B = (const bf16_t*)w_t; g.out = (bf16_t*)dx; g.gelu_z = (const bf16_t*)gelu_z;
    g.M = d->N * d->IH * d->IW; g.N = d->Cin; g.K = d->Cout;
    return icamd_pw_resident_ext_launch(g, (hipStream_t)stream);
  }
  if (d->KH == 1 && d->KW == 1 && st == 1 && d->pad == 0 && f == nullptr && !(addend_bits != nullptr && addend_sub2) &&
      icamd_gemm_nt_wanted((long long)d->N * d->IH * d->IW, d->Cin, d->Cout)) {
    GemmNtParams g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t*)dy; g.B = (const bf16_t*)w_t; g.out = (bf16_t*)dx; g.addend = (const bf16_t*)addend;
    g.addend_bits = addend_bits;
    g.M = d->N * d->IH * d->IW; g.N = d->Cin; g.K = d->Cout; g.gelu_z = (const bf16_t*)gelu_z;
    if (addend_sub2) { g.sub2_h = d->IH; g.sub2_w = d->IW; }
    return icamd_gemm_nt_launch(g, (hipStream_t)stream);
  }
  if (d->KH == 3 && d->KW == 3 && st == 1 && d->pad == 1 && addend == nullptr && addend_bits == nullptr && f == nullptr &&
      gelu_z == nullptr && icamd_halo3x3_wanted(d->N, d->IH, d->IW, d->Cout, d->Cin)) {
    // dX = conv(dY, transposed filter, mirrored taps): same spatial size in and out for stride 1 / pad 1
    Halo3x3Params h;
    memset(&h, 0, sizeof(h));
    h.in = (const bf16_t*)dy; h.wt = (const bf16_t*)w_t; h.out = (bf16_t*)dx; h.flip = 1;
    h.N = d->N; h.H = d->IH; h.W = d->IW; h.C = d->Cout; h.Cout = d->Cin;
    return icamd_halo3x3_launch(h, (hipStream_t)stream);
  }
  float* partials = f ? f->partials : nullptr;
  // one launch per output parity class (ph, pw): pixels h = st*p + ph, w = st*q + pw receive only the taps
  // r with (ph + pad - r) % st == 0, read at dy row p + (ph + pad - r)/st
  for (int ph = 0; ph < st; ++ph)
    for (int pw = 0; pw < st; ++pw) {
      const int P = (d->IH - ph + st - 1) / st, Q = (d->IW - pw + st - 1) / st;
      if (P <= 0 || Q <= 0) continue;
      IgemmParams p;
      memset(&p, 0, sizeof(p));
      p.in = (const bf16_t*)dy; p.wt = (const bf16_t*)w_t; p.out = (bf16_t*)dx;
      p.addend = (const bf16_t*)addend;
      p.addend_bits = addend_bits;
      p.addend_sub2 = addend_sub2;
      p.gelu_z = (const bf16_t*)gelu_z;
      p.N = d->N; p.IH = d->OH; p.IW = d->OW; p.Cin = d->Cout;
      p.OH = d->IH; p.OW = d->IW; p.Cout = d->Cin;
      p.P = P; p.Q = Q; p.M = d->N * P * Q;
      p.ostr = st; p.ooff_h = ph; p.ooff_w = pw; p.istr = 1;
      p.Ktot = d->KH * d->KW * d->Cout;
      p.KW = d->KW; p.pad = d->pad; p.tap_sign = -1; p.regular_taps = (st == 1) ? 1 : 0;
      if (f != nullptr) {
        p.bnb_y = (const bf16_t*)f->y; p.bnb_mask = (const bf16_t*)f->mask_src;
        p.bnb_mean = f->mean; p.bnb_invstd = f->invstd; p.bnb_scale = f->scale; p.bnb_shift = f->shift;
        p.bnb_relu = f->relu; p.stats = partials;
        partials += (size_t)((p.M + 127) / 128) * 2 * d->Cin;   // each parity class writes its own partial rows
      }
      int nt = 0;
      for (int r = 0; r < d->KH; ++r) {
        const int eh = ph + d->pad - r;
        if (((eh % st) + st) % st != 0) continue;
        for (int s = 0; s < d->KW; ++s) {
          const int ew = pw + d->pad - s;
          if (((ew % st) + st) % st != 0) continue;
          // exact division (eh, ew are multiples of st, possibly negative)
          if (nt < ICAMD_MAX_TAPS) { p.dh[nt] = (short)(eh / st); p.dw[nt] = (short)(ew / st); p.wtap[nt] = (short)(r * d->KW + s); }
          ++nt;
        }
      }
      p.ntaps = nt;
      const int rc = icamd_igemm_launch(p, (hipStream_t)stream);
      if (rc) return rc;
    }
  return ICAMD_OK;
}

int icamd_conv2d_dgrad(const icamd_conv_desc* d, const void* dy, const void* w_t, void* dx, const void* addend,
                       const uint8_t* addend_maskbits, void* stream) {
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.out + cw.in + 2 * cw.w + (addend ? cw.in : 0) + (addend_maskbits ? cw.in / 16 : 0), cw.flops);
  if (addend_maskbits != nullptr && (addend == nullptr || d == nullptr || d->Cin % 64 != 0)) return ICAMD_ERR_BAD_ARG;
  return dgrad_impl(d, dy, w_t, dx, addend, addend_maskbits, nullptr, stream);
}

int icamd_conv2d_dgrad_sub2(const icamd_conv_desc* d, const void* dy, const void* w_t, void* dx, const void* addend_sub2,
                            void* stream) {
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.out + cw.in + 2 * cw.w + cw.in / 4, cw.flops);
  if (addend_sub2 == nullptr) return ICAMD_ERR_BAD_ARG;
  return dgrad_impl(d, dy, w_t, dx, addend_sub2, nullptr, nullptr, stream, nullptr, 1);
}

int icamd_conv2d_dgrad_gelu(const icamd_conv_desc* d, const void* dy, const void* w_t, const void* z, void* dz,
                            void* stream) {
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.out + 2 * cw.in + 2 * cw.w, cw.flops);
  if (z == nullptr) return ICAMD_ERR_BAD_ARG;
  return dgrad_impl(d, dy, w_t, dz, nullptr, nullptr, nullptr, stream, z);
}

int icamd_conv2d_dgrad_stats_rows(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d)) return 0;
  int rows = 0;
  for (int ph = 0; ph < d->stride; ++ph)
    for (int pw = 0; pw < d->stride; ++pw) {
      const long long P = (d->IH - ph + d->stride - 1) / d->stride, Q = (d->IW - pw + d->stride - 1) / d->stride;
      if (P > 0 && Q > 0) rows += (int)((d->N * P * Q + 127) / 128);
    }
  return rows;
}

int icamd_conv2d_dgrad_bnbwd(const icamd_conv_desc* d, const void* dy, const void* w_t, void* g, const void* addend,
                             const icamd_bn_bwd_fuse* f, void* stream) {
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.out + 2 * cw.in + 2 * cw.w + (addend ? cw.in : 0), cw.flops);
  if (f == nullptr || f->y == nullptr || f->mean == nullptr || f->invstd == nullptr || f->partials == nullptr)
    return ICAMD_ERR_BAD_ARG;
  return dgrad_impl(d, dy, w_t, g, addend, nullptr, f, stream);
}

int icamd_conv2d_dgrad_bnred_supported(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d) || d->KH != 1 || d->KW != 1 || d->stride != 1 || d->pad != 0) return 0;
  return icamd_pw_resident_bnred_wanted((long long)d->N * d->IH * d->IW, d->Cin, d->Cout) ? 1 : 0;
}

int icamd_conv2d_dgrad_bnred(const icamd_conv_desc* d, const void* dy, const void* w_t, void* g, const void* addend,
                             const uint8_t* addend_bits, int addend_sub2, const void* bn_y, const uint8_t* bn_bits,
                             float* partials, void* stream) {
  ProfScope _prof(PC_IGEMM_DGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.out + 3 * cw.in + 2 * cw.w + cw.in / 16 + (addend_bits ? cw.in / 16 : 0), cw.flops);
  if (!conv_desc_ok(d) || dy == nullptr || w_t == nullptr || g == nullptr || addend == nullptr || bn_y == nullptr ||
      bn_bits == nullptr || partials == nullptr || (addend_sub2 && addend_bits != nullptr))
    return ICAMD_ERR_BAD_ARG;
  if (!icamd_conv2d_dgrad_bnred_supported(d)) return ICAMD_ERR_UNSUPPORTED;
  PwResidentParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)dy; p.B = (const bf16_t*)w_t; p.out = (bf16_t*)g; p.addend = (const bf16_t*)addend;
  p.addend_bits = addend_bits;
  p.bn_y = (const bf16_t*)bn_y; p.bn_bits = bn_bits; p.bn_part = partials;
  p.M = d->N * d->IH * d->IW; p.N = d->Cin; p.K = d->Cout;
  if (addend_sub2) { p.sub2_h = d->IH; p.sub2_w = d->IW; }
  return icamd_pw_resident_bnred_launch(p, (hipStream_t)stream);
}

size_t icamd_conv2d_wgrad_workspace_bytes(const icamd_conv_desc* d) {
  if (!conv_desc_ok(d)) return 0;
  int S = 1, rows = 0;
  const long long M = (long long)d->N * d->OH * d->OW;
  if (M >= (1ll << 30)) return 0;
  const int Ktot = d->KH * d->KW * d->Cin;
  icamd_wgrad_plan((int)M, d->Cout, Ktot, &S, &rows);
  if (icamd_wgrad_halo_wanted(d->KH, d->KW, d->stride, d->pad, d->OH, d->OW, d->Cin, d->Cout, M)) {
    int S2 = 1;   // the halo kernel has its own split; the bias-gradient form of the same layer stays on the general one
    icamd_wgrad_halo_plan((int)M, d->Cin, d->Cout, &S2, &rows);
    if (S2 > S) S = S2;
  }
  return wgrad_ws(nullptr, S, d->Cout, Ktot).bytes;   // filter slabs + one bias row per split
}

static int wgrad_impl(const icamd_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream);

int icamd_conv2d_wgrad(const icamd_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_WGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.in + cw.out + 4 * cw.w, cw.flops);
  return wgrad_impl(d, x, dy, dw, nullptr, accumulate, workspace, workspace_bytes, stream);
}

int icamd_conv2d_wgrad_bias(const icamd_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias,
                            int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  ProfScope _prof(PC_WGRAD, stream);
  const ConvWork cw = conv_work(d); _prof.work(cw.in + cw.out + 4 * cw.w, cw.flops);
  if (dbias == nullptr) return ICAMD_ERR_BAD_ARG;
  return wgrad_impl(d, x, dy, dw, dbias, accumulate, workspace, workspace_bytes, stream);
}

static int wgrad_impl(const icamd_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!conv_desc_ok(d) || x == nullptr || dy == nullptr || dw == nullptr || workspace == nullptr) return ICAMD_ERR_BAD_ARG;
  const size_t need = icamd_conv2d_wgrad_workspace_bytes(d);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const bf16_t*)x; p.dy = (const bf16_t*)dy; p.slab = (float*)workspace;
  p.N = d->N; p.IH = d->IH; p.IW = d->IW; p.Cin = d->Cin; p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout;
  p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad;
  p.M = d->N * d->OH * d->OW; p.Ktot = d->KH * d->KW * d->Cin;
  int rc;
  if (dbias == nullptr && icamd_wgrad_halo_wanted(d->KH, d->KW, d->stride, d->pad, d->OH, d->OW, d->Cin, d->Cout, p.M)) {
    icamd_wgrad_halo_plan(p.M, p.Cin, p.Cout, &p.S, &p.rows_per_split);
    rc = icamd_wgrad_halo_launch(p, (hipStream_t)stream);
  } else {
    icamd_wgrad_plan(p.M, p.Cout, p.Ktot, &p.S, &p.rows_per_split);
    if (dbias != nullptr) p.bias_slab = wgrad_ws(workspace, p.S, p.Cout, p.Ktot).bias_slab;
    rc = icamd_wgrad_launch(p, (hipStream_t)stream);
  }
  if (rc) return rc;
  rc = icamd_slab_reduce_launch(p.slab, dw, (long long)p.Cout * p.Ktot, p.S, accumulate, (hipStream_t)stream);
  if (rc || dbias == nullptr) return rc;
  return icamd_slab_reduce_launch(p.bias_slab, dbias, (long long)p.Cout, p.S, accumulate, (hipStream_t)stream);
}

}  // extern "C"
