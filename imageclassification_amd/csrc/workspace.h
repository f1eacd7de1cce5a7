// Layouts of the caller-allocated workspaces that hold more than one region.  Each layout is ONE function: the `*_bytes` query calls
// it with a null base and returns `.bytes`, the entry (or launcher) calls it with the real base and uses the returned pointers, so
// the size and the carve cannot disagree.  The planned counts (block and segment numbers) are the caller's: the plan functions
// stay with their kernels.  Host code only: no HIP types, nothing of the project included; a plain C++17 compiler builds it
// (tests/workspace_layout_main.cpp does, under AddressSanitizer).
#pragma once
#include <cstddef>

inline size_t ws_round256(size_t v) { return (v + 255) / 256 * 256; }

// Bump carver over an optional base.  Regions follow one another; a region's size is rounded up to 256 B, so that every region
// starts 256 B aligned in a 256 B aligned workspace (take_exact: the few regions that have always been left unrounded).
struct WsCarver {
  char* base;
  size_t off;
  explicit WsCarver(void* b, size_t start = 0) : base((char*)b), off(start) {}
  template <typename T> T* take(size_t count) { return bump<T>(ws_round256(count * sizeof(T))); }
  template <typename T> T* take_exact(size_t count) { return bump<T>(count * sizeof(T)); }
  size_t bytes() const { return off; }
 private:
  template <typename T> T* bump(size_t nbytes) {
    T* p = base ? (T*)(base + off) : nullptr;   // no arithmetic on a null base
    off += nbytes;
    return p;
  }
};

// ---- the reduction block: BatchNorm finalize / backward, LayerNorm backward, column sums, layer-scale backward ---------------
// 256 B of arrival counters (ceil(C/64) uint32, zero before first use, self-resetting) | chunks [64][2][C] fp64 |
// partial rows [part_rows][2][C] fp32 | scratch [scratch_rows][C] fp32 (c1,c2 of a BatchNorm backward: 2; a discarded second sum
// in front of them: 3).  part_rows = 0: the partial rows are the caller's; 0 and 0: the block of icamd_bn_train_finalize.
struct ReduceWs { unsigned int* counters; double* chunks; float* part; float* scratch; size_t bytes; };
inline ReduceWs reduce_ws(void* base, int C, long long part_rows, int scratch_rows) {
  WsCarver c(base);
  ReduceWs w;
  w.counters = c.take<unsigned int>(64);
  w.chunks = c.take<double>((size_t)64 * 2 * C);
  w.part = c.take<float>((size_t)part_rows * 2 * C);
  w.scratch = c.take<float>((size_t)scratch_rows * C);
  w.bytes = c.bytes();
  return w;
}

// ---- squeeze-and-excitation backward (se_ops.hip), S row segments per sample --------------------------------------------------
// part [N*S][2][C] | AB [N][2][C] | dp2 [N][C] | ds [N][C] | k0 [N][C] | dh [N][256] | k2 [C]   (fp32)
struct SeBwdWs { float *part, *AB, *dp2, *ds, *k0, *dh, *k2; size_t bytes; };
inline SeBwdWs se_bwd_ws(void* base, int N, int S, int C) {
  WsCarver c(base);
  SeBwdWs w;
  const size_t nc = (size_t)N * C;
  w.part = c.take<float>((size_t)N * S * 2 * C);
  w.AB = c.take<float>(nc);   // [N][2][C] in a region sized as two rounded [N][C] ones
  c.take<float>(nc);
  w.dp2 = c.take<float>(nc);
  w.ds = c.take<float>(nc);
  w.k0 = c.take<float>(nc);
  w.dh = c.take<float>((size_t)N * 256);
  w.k2 = c.take<float>((size_t)C);
  w.bytes = c.bytes();
  return w;
}

// ---- global response normalisation (grn.hip), S row segments per sample -------------------------------------------------------
// partial rows [N][S][2][C] | per-sample rows of the parameter gradients [N][2][C]   (fp32)
struct GrnWs { float *part, *fin; size_t bytes; };
inline GrnWs grn_ws(void* base, int N, int S, int C) {
  WsCarver c(base);
  GrnWs w;
  w.part = c.take<float>((size_t)N * S * 2 * C);
  w.fin = c.take<float>((size_t)N * 2 * C);
  w.bytes = c.bytes();
  return w;
}

// ---- image pipeline (image_ops.hip) ---------------------------------------------------------------------------------------------
// tabs [B][tab_words] int32 | tmp [B][max_crop_h][out_w][3] u8 | img [B][out_h][out_w][3] u8; the augmenting pipeline appends
// img2 (as img) | aux [B][aux_per_image] u8 behind the same three, so that img is found at one offset by both.
struct ImageWs { int* tabs; unsigned char *tmp, *img; size_t bytes; };
inline ImageWs image_ws(void* base, int B, long long tab_words, int max_crop_h, int out_h, int out_w) {
  WsCarver c(base);
  ImageWs w;
  w.tabs = c.take<int>((size_t)B * tab_words);
  w.tmp = c.take<unsigned char>((size_t)B * max_crop_h * out_w * 3);
  w.img = c.take<unsigned char>((size_t)B * out_h * out_w * 3);
  w.bytes = c.bytes();
  return w;
}
struct ImageAugWs : ImageWs { unsigned char *img2, *aux; };
inline ImageAugWs image_aug_ws(void* base, int B, long long tab_words, int max_crop_h, int out_h, int out_w, int aux_per_image) {
  ImageAugWs w;
  (ImageWs&)w = image_ws(base, B, tab_words, max_crop_h, out_h, out_w);
  WsCarver c(base, w.bytes);   // goes on behind img
  w.img2 = c.take<unsigned char>((size_t)B * out_h * out_w * 3);
  w.aux = c.take<unsigned char>((size_t)B * aux_per_image);
  w.bytes = c.bytes();
  return w;
}

// ---- depthwise 7x7 weight gradient (dwconv.hip): one partial filter row [49][C] per workgroup row | one bias row [C] each, sized
// whether or not the bias is asked for   (fp32, neither rounded)
struct DwWgradWs { float *part, *part_b; size_t bytes; };
inline DwWgradWs dw_wgrad_ws(void* base, long long blocks, int C) {
  WsCarver c(base);
  DwWgradWs w;
  w.part = c.take_exact<float>((size_t)blocks * 49 * C);
  w.part_b = c.take_exact<float>((size_t)blocks * C);
  w.bytes = c.bytes();
  return w;
}

// ---- dense weight gradient (capi.hip): S filter slabs [S][Cout][Ktot] | S bias rows [S][Cout]   (fp32, neither rounded) --------
struct WgradWs { float *slab, *bias_slab; size_t bytes; };
inline WgradWs wgrad_ws(void* base, int S, int Cout, int Ktot) {
  WsCarver c(base);
  WgradWs w;
  w.slab = c.take_exact<float>((size_t)S * Cout * Ktot);
  w.bias_slab = c.take_exact<float>((size_t)S * Cout);
  w.bytes = c.bytes();
  return w;
}
