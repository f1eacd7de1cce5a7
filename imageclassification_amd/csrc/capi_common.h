// What the C-ABI units (capi.hip, capi_conv_special.hip, capi_norm.hip, capi_tokens.hip, capi_step.hip) share: the in-process
// kernel timing scope, the convolution-descriptor check and the workspace layouts (workspace.h).  Host code only.
#pragma once
#include "../../include/icamd.h"
#include "common.h"
#include "icamd_internal.h"
#include "workspace.h"
#include <cstdlib>
#include <string.h>
#include <vector>

// ---- optional in-process kernel timing (HIP events on the launch stream), used by bench.py ------------------
enum ProfClass { PC_IGEMM_FWD = 0, PC_IGEMM_DGRAD, PC_WGRAD, PC_BN_FINALIZE, PC_BN_APPLY, PC_BN_BWD, PC_POOL, PC_PACK,
                 PC_LOSS, PC_OPTIM, PC_MISC, PC_ATTN_FWD, PC_ATTN_BWD, PC_LN_FWD, PC_LN_BWD, PC_ELEMWISE, PC_DWCONV, PC_FUSED_BWD, PC_FUSED_FWD, PC_COUNT };
// Besides the elapsed time every call books its ALGORITHMIC work (round 4): bytes = each operand tensor of the call
// read once and each result written once at the stored width (bf16 activations, fp32 parameters / gradients), two-pass
// kernels counted as the two passes they are; flops = 2 x multiply-adds of the contraction.  bench.py divides by the time.
struct ProfRec { int cls; hipEvent_t a, b; double bytes, flops; };
// The profiler state: one object for the whole library, defined in capi.hip next to icamd_prof_* (hidden: not part of the ABI).
#define ICAMD_HIDDEN __attribute__((visibility("hidden")))
extern ICAMD_HIDDEN bool g_prof_on;
extern ICAMD_HIDDEN std::vector<ProfRec> g_prof_recs;
extern ICAMD_HIDDEN std::vector<hipEvent_t> g_prof_pool;
ICAMD_HIDDEN hipEvent_t prof_event();
struct ProfScope {
  int cls; hipStream_t s; hipEvent_t a; bool on; double bytes = 0.0, flops = 0.0;
  ProfScope(int c, void* stream) : cls(c), s((hipStream_t)stream), on(g_prof_on) {
    if (on) { a = prof_event(); (void)hipEventRecord(a, s); }
  }
  void work(double b, double f = 0.0) { bytes = b; flops = f; }
  ~ProfScope() {
    if (on) { hipEvent_t b = prof_event(); (void)hipEventRecord(b, s); g_prof_recs.push_back({cls, a, b, bytes, flops}); }
  }
};
// operand sizes of a convolution call: input / output activations (bf16), filter elements, multiply-adds x 2
struct ConvWork { double in, out, w, flops; };
static ConvWork conv_work(const icamd_conv_desc* d) {
  ConvWork c = {0, 0, 0, 0};
  if (d == nullptr) return c;
  c.in = 2.0 * d->N * d->IH * d->IW * d->Cin;
  c.out = 2.0 * d->N * d->OH * d->OW * d->Cout;
  c.w = (double)d->Cout * d->KH * d->KW * d->Cin;
  c.flops = 2.0 * d->N * d->OH * d->OW * c.w;
  return c;
}

static bool conv_desc_ok(const icamd_conv_desc* d) {
  if (d == nullptr) return false;
  if (d->N <= 0 || d->IH <= 0 || d->IW <= 0 || d->Cin <= 0 || d->OH <= 0 || d->OW <= 0 || d->Cout <= 0) return false;
  if (d->KH <= 0 || d->KW <= 0 || d->stride <= 0 || d->pad < 0) return false;
  if (d->Cin % 64 == 0 && d->KH * d->KW > ICAMD_MAX_TAPS) return false;   // the general path derives taps arithmetically
  if (d->KH * d->KW > 1024) return false;
  if ((d->IH + 2 * d->pad - d->KH) / d->stride + 1 != d->OH) return false;
  if ((d->IW + 2 * d->pad - d->KW) / d->stride + 1 != d->OW) return false;
  return true;
}

// partial rows of the BatchNorm backward's reduce pass: one per block of the plan
static long long bn_bwd_blocks(long long rows, int C) {
  const int rpb = icamd_bn_bwd_rows_per_block(rows, C);
  return (rows + rpb - 1) / rpb;
}
