// Input pipeline on the GPU: everything the reference's train / eval transforms do AFTER JPEG decoding
// (/root/reference/datasets.py:121-144: timm.create_transform(scale=(1,1), ratio=(1,1), vflip=0.5, color_jitter=0.3,
// interpolation='bicubic', re_prob=0.25, re_mode='pixel') for training; Resize -> ToTensor -> Normalize for eval), on uint8
// HWC images of arbitrary sizes, one launch sequence per batch:
//   1. resample_coeffs_kernel  per image and axis: Pillow's filter windows and 22-bit integer weights (Resample.c), computed
//                              in double with FMA contraction OFF so that they equal the CPU's bit for bit;
//   2. resize_h_kernel         crop window + horizontal pass -> uint8 (rounded and clamped, as Pillow stores the pass);
//   3. resize_v_kernel         vertical pass (+ horizontal / vertical flip folded into the store index) -> uint8 [B][H][W][3];
//   4. jitter_kernel           torchvision ColorJitter on PIL semantics: brightness / contrast / saturation in a per-image
//                              order, PIL.ImageEnhance arithmetic (Image.blend truncation / clamping, integer luma, contrast
//                              pivot = rounded mean luma of the image AT THAT POINT of the chain: one workgroup per image);
//   5. finalize_kernel         ToTensor + Normalize -> fp32 NCHW, timm RandomErasing(mode='pixel') box filled with N(0,1).
// icamd_image_pipeline_aug runs timm's RandAugment between steps 4 and 5, two launches per op slot:
//   aug_stats_kernel           one workgroup per image: the slot's 3x256 LUT (exact integer histograms in LDS for autocontrast /
//                              equalize; closed forms for invert / posterize / solarize / solarize-add) or the contrast pivot;
//   aug_apply_kernel           one thread per output pixel, image ping -> pong: the bicubic affine gather with fill (Pillow's
//                              Geometry.c in double), LUT ops, ImageEnhance blends, SMOOTH (float, Filter.c order) + blend.
// Random decisions (flips, jitter order and factors, erase box, noise seed) are made on the host and arrive in the
// descriptors, so parity tests inject them.  Bit-exact against Pillow for steps 1-4 (tests/test_image_gpu.py).
#include "../../include/icamd.h"
#include "common.h"
#include "workspace.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

#pragma clang fp contract(off)
__device__ double filter_weight(int filt, double x) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (filt == 1) {         // bicubic, a = -0.5
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;   // bilinear
}

// grid: (ceil(out/64), 2 axes, B); one thread per output sample of one axis
__global__ __launch_bounds__(64) void resample_coeffs_kernel(const icamd_image_desc* __restrict__ descs, int out_h, int out_w,
                                                             int filt, int kmax, int* __restrict__ tabs, long long per_image) {
#pragma clang fp contract(off)
  const int b = blockIdx.z, axis = blockIdx.y;
  const int out_size = axis == 0 ? out_w : out_h;
  const int xx = blockIdx.x * 64 + threadIdx.x;
  if (xx >= out_size) return;
  const icamd_image_desc d = descs[b];
  const int in_size = axis == 0 ? d.crop_w : d.crop_h;
  int* bounds = tabs + (long long)b * per_image + (axis == 0 ? 0 : (long long)out_w * (2 + kmax));
  int* kk = bounds + (long long)out_size * 2;
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = (filt == 1 ? 2.0 : 1.0) * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > kmax) xmax = kmax;   // cannot happen when the host sized kmax from the same formula; keeps stores in bounds
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += filter_weight(filt, (x + xmin - center + 0.5) * ss);
  for (int x = 0; x < kmax; ++x) {
    int q = 0;
    if (x < xmax) {
      double w = filter_weight(filt, (x + xmin - center + 0.5) * ss);
      if (ww != 0.0) w = w / ww;
      q = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    kk[(long long)xx * kmax + x] = q;
  }
  bounds[xx * 2] = xmin;
  bounds[xx * 2 + 1] = xmax;
}

__device__ __forceinline__ unsigned char clip8(int v) {
  v >>= PRECISION_BITS;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// grid: (ceil(out_w*rows/256), 1, B): thread -> (row of the crop window, output column); tmp[b][row][ox][3]
__global__ __launch_bounds__(256) void resize_h_kernel(const unsigned char* __restrict__ src,
                                                       const icamd_image_desc* __restrict__ descs, int out_w, int kmax,
                                                       const int* __restrict__ tabs, long long per_image,
                                                       unsigned char* __restrict__ tmp, long long tmp_per_image) {
  const int b = blockIdx.z;
  const icamd_image_desc d = descs[b];
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)d.crop_h * out_w) return;
  const int row = (int)(idx / out_w), ox = (int)(idx - (long long)row * out_w);
  const int* bounds = tabs + (long long)b * per_image;
  const int* kk = bounds + (long long)out_w * 2 + (long long)ox * kmax;
  const int xmin = bounds[ox * 2], cnt = bounds[ox * 2 + 1];
  const unsigned char* line = src + d.src_offset + ((long long)(d.crop_top + row) * d.src_w + d.crop_left) * 3;
  unsigned char* o = tmp + (long long)b * tmp_per_image + ((long long)row * out_w + ox) * 3;
  if (d.crop_w == out_w) {   // Pillow skips a pass that does not change the size
    o[0] = line[ox * 3]; o[1] = line[ox * 3 + 1]; o[2] = line[ox * 3 + 2];
    return;
  }
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int w = kk[t];
    const unsigned char* px = line + (xmin + t) * 3;
    s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
  }
  o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
}

// grid: (ceil(out_h*out_w/256), 1, B); img[b][oy'][ox'][3] with the flips applied to the destination index
__global__ __launch_bounds__(256) void resize_v_kernel(const icamd_image_desc* __restrict__ descs, int out_h, int out_w, int kmax,
                                                       const int* __restrict__ tabs, long long per_image,
                                                       const unsigned char* __restrict__ tmp, long long tmp_per_image,
                                                       unsigned char* __restrict__ img) {
  const int b = blockIdx.z;
  const icamd_image_desc d = descs[b];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= out_h * out_w) return;
  const int oy = idx / out_w, ox = idx - oy * out_w;
  const int* bounds = tabs + (long long)b * per_image + (long long)out_w * (2 + kmax);
  const int* kk = bounds + (long long)out_h * 2 + (long long)oy * kmax;
  const int ymin = bounds[oy * 2], cnt = bounds[oy * 2 + 1];
  const unsigned char* col = tmp + (long long)b * tmp_per_image + (long long)ox * 3;
  unsigned char r0, r1, r2;
  if (d.crop_h == out_h) {
    const unsigned char* px = col + (long long)oy * out_w * 3;
    r0 = px[0]; r1 = px[1]; r2 = px[2];
  } else {
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < cnt; ++t) {
      const int w = kk[t];
      const unsigned char* px = col + (long long)(ymin + t) * out_w * 3;
      s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
    }
    r0 = clip8(s0); r1 = clip8(s1); r2 = clip8(s2);
  }
  const int dy = d.vflip ? out_h - 1 - oy : oy, dx = d.hflip ? out_w - 1 - ox : ox;
  unsigned char* o = img + ((long long)b * out_h * out_w + (long long)dy * out_w + dx) * 3;
  o[0] = r0; o[1] = r1; o[2] = r2;
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
// PIL Image.blend(degenerate, image, factor) on one uint8 sample (libImaging/Blend.c)
__device__ __forceinline__ int blend(int deg, int v, float f, bool inside) {
#pragma clang fp contract(off)
  const float t = (float)deg + f * ((float)v - (float)deg);   // separate multiply and add, as the C library's x86 build
  if (inside) return (int)t & 255;                     // (UINT8)(float): truncation toward zero, value already in [0, 255]
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// one workgroup per image, in place on img[b]
__global__ __launch_bounds__(256) void jitter_kernel(const icamd_image_desc* __restrict__ descs, int npix,
                                                     unsigned char* __restrict__ img) {
  __shared__ unsigned long long red[256];
  const icamd_image_desc d = descs[blockIdx.x];
  unsigned char* p = img + (long long)blockIdx.x * npix * 3;
  for (int k = 0; k < 3; ++k) {
    const int op = d.jitter_order[k];
    if (op < 0 || op > 2) continue;
    const float f = d.jitter_factor[op];
    const bool inside = f >= 0.f && f <= 1.f;
    int pivot = 0;
    if (op == 1) {                                     // contrast: rounded mean luma of the image as it is NOW
      unsigned long long s = 0;
      for (int i = threadIdx.x; i < npix; i += 256) s += (unsigned)luma(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
      red[threadIdx.x] = s;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
      }
      pivot = (int)((double)red[0] / (double)npix + 0.5);   // int(ImageStat.Stat(L).mean[0] + 0.5)
      __syncthreads();
    }
    for (int i = threadIdx.x; i < npix; i += 256) {
      const int r = p[i * 3], g = p[i * 3 + 1], b = p[i * 3 + 2];
      const int dg = op == 0 ? 0 : (op == 1 ? pivot : luma(r, g, b));
      p[i * 3] = (unsigned char)blend(dg, r, f, inside);
      p[i * 3 + 1] = (unsigned char)blend(dg, g, f, inside);
      p[i * 3 + 2] = (unsigned char)blend(dg, b, f, inside);
    }
    __syncthreads();   // the next operation reads what every thread wrote
  }
}

// ---- RandAugment (icamd_aug_op) ----

constexpr int AUG_LUT_BYTES = 768;   // per image: 3 x 256 LUT, then the contrast pivot as an int
constexpr int AUG_AUX_BYTES = AUG_LUT_BYTES + 16;

__device__ __forceinline__ bool aug_uses_lut(int kind) { return kind >= ICAMD_AUG_AUTOCONTRAST && kind <= ICAMD_AUG_SOLARIZE_ADD; }

// grid: B workgroups of 256; reads img[b] (the image before this slot's op), writes aux[b]
__global__ __launch_bounds__(256) void aug_stats_kernel(const icamd_aug_op* __restrict__ ops, int ops_per_image, int slot, int npix,
                                                        const unsigned char* __restrict__ img, unsigned char* __restrict__ aux) {
#pragma clang fp contract(off)
  __shared__ int hist[3 * 256];
  __shared__ unsigned long long red[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const icamd_aug_op op = ops[(long long)b * ops_per_image + slot];
  const unsigned char* p = img + (long long)b * npix * 3;
  unsigned char* lut = aux + (long long)b * AUG_AUX_BYTES;
  if (op.kind == ICAMD_AUG_CONTRAST) {               // pivot = int(ImageStat.Stat(L).mean[0] + 0.5), as jitter_kernel
    unsigned long long s = 0;
    for (int i = t; i < npix; i += 256) s += (unsigned)luma(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    if (t == 0) *(int*)(lut + AUG_LUT_BYTES) = (int)((double)red[0] / (double)npix + 0.5);
    return;
  }
  if (!aug_uses_lut(op.kind)) return;
  if (op.kind == ICAMD_AUG_AUTOCONTRAST || op.kind == ICAMD_AUG_EQUALIZE) {   // image.histogram(): exact counts per band
    for (int i = t; i < 3 * 256; i += 256) hist[i] = 0;
    __syncthreads();
    for (int i = t; i < npix; i += 256) {
      atomicAdd(&hist[p[i * 3]], 1);
      atomicAdd(&hist[256 + p[i * 3 + 1]], 1);
      atomicAdd(&hist[512 + p[i * 3 + 2]], 1);
    }
    __syncthreads();
    if (t < 3) {
      const int* h = hist + t * 256;
      unsigned char* l = lut + t * 256;
      if (op.kind == ICAMD_AUG_AUTOCONTRAST) {       // ImageOps.autocontrast(cutoff=0): stretch [lo, hi] to [0, 255]
        int lo = 0, hi = 255;
        while (lo < 255 && h[lo] == 0) ++lo;
        while (hi > 0 && h[hi] == 0) --hi;
        if (hi <= lo) {
          for (int i = 0; i < 256; ++i) l[i] = (unsigned char)i;
        } else {
          const double scale = 255.0 / (double)(hi - lo), offset = (double)(-lo) * scale;
          for (int i = 0; i < 256; ++i) {
            const int v = (int)((double)i * scale + offset);   // Python int(): truncation toward zero
            l[i] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
          }
        }
      } else {                                       // ImageOps.equalize: step = (total - count of the last used bin) // 255
        long long total = 0, last = 0;
        int used = 0;
        for (int i = 0; i < 256; ++i)
          if (h[i]) { total += h[i]; last = h[i]; ++used; }
        const long long step = used <= 1 ? 0 : (total - last) / 255;
        if (step == 0) {
          for (int i = 0; i < 256; ++i) l[i] = (unsigned char)i;
        } else {
          long long n = step / 2;
          for (int i = 0; i < 256; ++i) {
            const long long v = n / step;
            l[i] = (unsigned char)(v > 255 ? 255 : v);   // Image.point clips the table entries to 8 bits
            n += h[i];
          }
        }
      }
    }
    return;
  }
  for (int i = t; i < 3 * 256; i += 256) {
    const int v = i & 255;
    int r = v;
    if (op.kind == ICAMD_AUG_INVERT) {
      r = 255 - v;
    } else if (op.kind == ICAMD_AUG_POSTERIZE) {     // mask = ~(2 ** (8 - bits) - 1)
      r = op.arg >= 8 ? v : (op.arg <= 0 ? 0 : v & ~((1 << (8 - op.arg)) - 1));
    } else if (op.kind == ICAMD_AUG_SOLARIZE) {
      r = v < op.arg ? v : 255 - v;
    } else {                                         // solarize-add, threshold 128
      const int a = v + op.arg;
      r = v < 128 ? (a > 255 ? 255 : (a < 0 ? 0 : a)) : v;
    }
    lut[i] = (unsigned char)r;
  }
}

// Geometry.c BICUBIC: p1 + d * (p2 + d * (p3 + d * p4)) in double
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
  const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// Filter.c 3x3 on one band: rows y+1, y, y-1 (the kernel flipped), each a left-to-right sum of three float products
__device__ __forceinline__ int smooth3x3(const unsigned char* c, int row) {
#pragma clang fp contract(off)
  const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
  const unsigned char* dn = c + row;
  const unsigned char* up = c - row;
  float ss = 0.f;
  ss += ((float)dn[-3] * k1 + (float)dn[0] * k1) + (float)dn[3] * k1;
  ss += ((float)c[-3] * k1 + (float)c[0] * k5) + (float)c[3] * k1;
  ss += ((float)up[-3] * k1 + (float)up[0] * k1) + (float)up[3] * k1;
  if (ss <= 0.f) return 0;
  if (ss >= 255.f) return 255;
  return (int)((double)ss + 0.5);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid: (ceil(H*W/256), 1, B); src[b] -> dst[b] for this slot's op of image b
__global__ __launch_bounds__(256) void aug_apply_kernel(const icamd_aug_op* __restrict__ ops, int ops_per_image, int slot, int h,
                                                        int w, const unsigned char* __restrict__ aux,
                                                        const unsigned char* __restrict__ src, unsigned char* __restrict__ dst) {
#pragma clang fp contract(off)
  const int b = blockIdx.z;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= h * w) return;
  const icamd_aug_op& op = ops[(long long)b * ops_per_image + slot];
  const int kind = op.kind;
  const int y = idx / w, x = idx - y * w;
  const unsigned char* s = src + (long long)b * h * w * 3;
  const unsigned char* px = s + (long long)idx * 3;
  unsigned char* o = dst + ((long long)b * h * w + idx) * 3;
  int r = px[0], g = px[1], bl = px[2];
  if (kind == ICAMD_AUG_AFFINE) {                    // ImagingGenericTransform + affine_transform + bicubic_filter32RGB
    const double xin0 = op.affine[0] * ((double)x + 0.5) + op.affine[1] * ((double)y + 0.5) + op.affine[2];
    const double yin0 = op.affine[3] * ((double)x + 0.5) + op.affine[4] * ((double)y + 0.5) + op.affine[5];
    if (!(xin0 >= 0.0 && xin0 < (double)w && yin0 >= 0.0 && yin0 < (double)h)) {
      o[0] = op.fill[0]; o[1] = op.fill[1]; o[2] = op.fill[2];
      return;
    }
    const double xi = xin0 - 0.5, yi = yin0 - 0.5;
    const double fx = floor(xi), fy = floor(yi);
    const double dx = xi - fx, dy = yi - fy;
    const int x0 = (int)fx - 1, y0 = (int)fy - 1;
    int cx[4], ry[4];
    for (int k = 0; k < 4; ++k) {                    // edge rows / columns repeat (XCLIP, and v_k = v_k-1 past the last row)
      cx[k] = clampi(x0 + k, 0, w - 1) * 3;
      ry[k] = clampi(y0 + k, 0, h - 1);
    }
    int res[3];
    for (int c = 0; c < 3; ++c) {
      double v[4];
      for (int k = 0; k < 4; ++k) {
        const unsigned char* ln = s + (long long)ry[k] * w * 3 + c;
        v[k] = cubic((double)ln[cx[0]], (double)ln[cx[1]], (double)ln[cx[2]], (double)ln[cx[3]], dx);
      }
      const double v1 = cubic(v[0], v[1], v[2], v[3], dy);
      res[c] = v1 <= 0.0 ? 0 : (v1 >= 255.0 ? 255 : (int)v1);
    }
    o[0] = (unsigned char)res[0]; o[1] = (unsigned char)res[1]; o[2] = (unsigned char)res[2];
    return;
  }
  const unsigned char* a = aux + (long long)b * AUG_AUX_BYTES;
  if (aug_uses_lut(kind)) {
    o[0] = a[r]; o[1] = a[256 + g]; o[2] = a[512 + bl];
    return;
  }
  if (kind < ICAMD_AUG_COLOR || kind > ICAMD_AUG_SHARPNESS) {
    o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)bl;
    return;
  }
  const float f = op.factor;
  const bool inside = f >= 0.f && f <= 1.f;
  int d0, d1, d2;
  if (kind == ICAMD_AUG_COLOR) {
    d0 = d1 = d2 = luma(r, g, bl);
  } else if (kind == ICAMD_AUG_CONTRAST) {
    d0 = d1 = d2 = *(const int*)(a + AUG_LUT_BYTES);
  } else if (kind == ICAMD_AUG_BRIGHTNESS) {
    d0 = d1 = d2 = 0;
  } else if (x > 0 && x < w - 1 && y > 0 && y < h - 1) {   // SMOOTH leaves the outermost rows and columns as they are
    d0 = smooth3x3(px, w * 3);
    d1 = smooth3x3(px + 1, w * 3);
    d2 = smooth3x3(px + 2, w * 3);
  } else {
    d0 = r; d1 = g; d2 = bl;
  }
  o[0] = (unsigned char)blend(d0, r, f, inside);
  o[1] = (unsigned char)blend(d1, g, f, inside);
  o[2] = (unsigned char)blend(d2, bl, f, inside);
}

// counter-based noise for the erased box: two rounds of a 32-bit mixer per draw, Box-Muller
__device__ __forceinline__ unsigned int mix32(unsigned int x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float normal01(unsigned int seed, unsigned int idx) {
  const unsigned int a = mix32(seed ^ (idx * 2u + 1u)), b = mix32((seed + 0x9e3779b9u) ^ (idx * 2u + 2u));
  const float u1 = ((float)(a >> 8) + 0.5f) * (1.f / 16777216.f), u2 = ((float)(b >> 8) + 0.5f) * (1.f / 16777216.f);
  return sqrtf(-2.f * __logf(u1)) * __cosf(6.283185307179586f * u2);
}

// grid: (ceil(H*W/256), 3 channels, B) -> out[b][c][y][x] fp32
__global__ __launch_bounds__(256) void finalize_kernel(const icamd_image_desc* __restrict__ descs, int out_h, int out_w,
                                                       const unsigned char* __restrict__ img, float m0, float m1, float m2,
                                                       float s0, float s1, float s2, float* __restrict__ out) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= out_h * out_w) return;
  const icamd_image_desc d = descs[b];
  const int y = idx / out_w, x = idx - y * out_w;
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
  float v = ((float)img[((long long)b * out_h * out_w + idx) * 3 + c] / 255.f - mean) / sd;
  if (d.erase_h > 0 && d.erase_w > 0 && y >= d.erase_top && y < d.erase_top + d.erase_h && x >= d.erase_left &&
      x < d.erase_left + d.erase_w)
    v = normal01(d.erase_seed, (unsigned)((c * out_h + y) * out_w + x));
  out[(((long long)b * 3 + c) * out_h + y) * out_w + x] = v;
}

}  // namespace

extern "C" {

// int32 table words per image: both axes' bounds + weights
static long long tab_words(int out_h, int out_w, int kmax) { return (long long)(out_h + out_w) * (2 + kmax); }

size_t icamd_image_pipeline_workspace_bytes(int B, int max_crop_h, int out_h, int out_w, int kmax) {
  if (B <= 0 || max_crop_h <= 0 || out_h <= 0 || out_w <= 0 || kmax <= 0) return 0;
  return image_ws(nullptr, B, tab_words(out_h, out_w, kmax), max_crop_h, out_h, out_w).bytes;
}

int icamd_image_pipeline(const uint8_t* src, const icamd_image_desc* descs, int B, int max_crop_h, int out_h, int out_w,
                         int filter, int kmax, const float* mean3, const float* std3, float* out_nchw, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (src == nullptr || descs == nullptr || out_nchw == nullptr || workspace == nullptr || mean3 == nullptr || std3 == nullptr)
    return ICAMD_ERR_BAD_ARG;
  if (B <= 0 || out_h <= 0 || out_w <= 0 || kmax <= 0 || (filter != 0 && filter != 1)) return ICAMD_ERR_BAD_ARG;
  const size_t need = icamd_image_pipeline_workspace_bytes(B, max_crop_h, out_h, out_w, kmax);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const long long per_image = tab_words(out_h, out_w, kmax);
  const long long tmp_per_image = (long long)max_crop_h * out_w * 3;
  const ImageWs w = image_ws(workspace, B, per_image, max_crop_h, out_h, out_w);
  int* tabs = w.tabs;
  unsigned char *tmp = w.tmp, *img = w.img;
  const int omax = out_h > out_w ? out_h : out_w;
  hipLaunchKernelGGL(resample_coeffs_kernel, dim3((unsigned)((omax + 63) / 64), 2, (unsigned)B), dim3(64), 0, s, descs, out_h,
                     out_w, filter, kmax, tabs, per_image);
  hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)(((long long)max_crop_h * out_w + 255) / 256), 1, (unsigned)B), dim3(256), 0,
                     s, src, descs, out_w, kmax, tabs, per_image, tmp, tmp_per_image);
  hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((out_h * out_w + 255) / 256), 1, (unsigned)B), dim3(256), 0, s, descs, out_h,
                     out_w, kmax, tabs, per_image, tmp, tmp_per_image, img);
  hipLaunchKernelGGL(jitter_kernel, dim3((unsigned)B), dim3(256), 0, s, descs, out_h * out_w, img);
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((out_h * out_w + 255) / 256), 3, (unsigned)B), dim3(256), 0, s, descs, out_h,
                     out_w, img, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out_nchw);
  return icamd_launch_status();
}

size_t icamd_image_pipeline_aug_workspace_bytes(int B, int max_crop_h, int out_h, int out_w, int kmax) {
  if (icamd_image_pipeline_workspace_bytes(B, max_crop_h, out_h, out_w, kmax) == 0) return 0;
  return image_aug_ws(nullptr, B, tab_words(out_h, out_w, kmax), max_crop_h, out_h, out_w, AUG_AUX_BYTES).bytes;
}

int icamd_image_pipeline_aug(const uint8_t* src, const icamd_image_desc* descs, const icamd_aug_op* ops, int ops_per_image,
                             int B, int max_crop_h, int out_h, int out_w, int filter, int kmax, const float* mean3,
                             const float* std3, float* out_nchw, void* workspace, size_t workspace_bytes, void* stream) {
  if (src == nullptr || descs == nullptr || out_nchw == nullptr || workspace == nullptr || mean3 == nullptr || std3 == nullptr)
    return ICAMD_ERR_BAD_ARG;
  if (B <= 0 || out_h <= 0 || out_w <= 0 || kmax <= 0 || (filter != 0 && filter != 1)) return ICAMD_ERR_BAD_ARG;
  if (ops_per_image < 0 || ops_per_image > 16 || (ops_per_image > 0 && ops == nullptr)) return ICAMD_ERR_BAD_ARG;
  const size_t need = icamd_image_pipeline_aug_workspace_bytes(B, max_crop_h, out_h, out_w, kmax);
  if (need == 0 || workspace_bytes < need) return ICAMD_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  // icamd_image_pipeline's layout [tabs][tmp][img], then [img2][aux]: the final image must land in img (icamd_image_pipeline_u8),
  // so the resize writes to img2 when the number of ping-pong passes is odd
  const long long per_image = tab_words(out_h, out_w, kmax);
  const long long tmp_per_image = (long long)max_crop_h * out_w * 3;
  const ImageAugWs w = image_aug_ws(workspace, B, per_image, max_crop_h, out_h, out_w, AUG_AUX_BYTES);
  int* tabs = w.tabs;
  unsigned char *tmp = w.tmp, *img = w.img, *img2 = w.img2, *aux = w.aux;
  unsigned char* cur = ops_per_image % 2 ? img2 : img;
  unsigned char* nxt = ops_per_image % 2 ? img : img2;
  const int omax = out_h > out_w ? out_h : out_w;
  const unsigned pix_blocks = (unsigned)((out_h * out_w + 255) / 256);
  hipLaunchKernelGGL(resample_coeffs_kernel, dim3((unsigned)((omax + 63) / 64), 2, (unsigned)B), dim3(64), 0, s, descs, out_h,
                     out_w, filter, kmax, tabs, per_image);
  hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)(((long long)max_crop_h * out_w + 255) / 256), 1, (unsigned)B), dim3(256), 0,
                     s, src, descs, out_w, kmax, tabs, per_image, tmp, tmp_per_image);
  hipLaunchKernelGGL(resize_v_kernel, dim3(pix_blocks, 1, (unsigned)B), dim3(256), 0, s, descs, out_h, out_w, kmax, tabs,
                     per_image, tmp, tmp_per_image, cur);
  hipLaunchKernelGGL(jitter_kernel, dim3((unsigned)B), dim3(256), 0, s, descs, out_h * out_w, cur);
  for (int k = 0; k < ops_per_image; ++k) {
    hipLaunchKernelGGL(aug_stats_kernel, dim3((unsigned)B), dim3(256), 0, s, ops, ops_per_image, k, out_h * out_w, cur, aux);
    hipLaunchKernelGGL(aug_apply_kernel, dim3(pix_blocks, 1, (unsigned)B), dim3(256), 0, s, ops, ops_per_image, k, out_h, out_w,
                       aux, cur, nxt);
    unsigned char* t = cur;
    cur = nxt;
    nxt = t;
  }
  hipLaunchKernelGGL(finalize_kernel, dim3(pix_blocks, 3, (unsigned)B), dim3(256), 0, s, descs, out_h, out_w, img, mean3[0],
                     mean3[1], mean3[2], std3[0], std3[1], std3[2], out_nchw);
  return icamd_launch_status();
}

// the uint8 [B][H][W][3] image after resize / flips / jitter (what Pillow would hold before ToTensor): for parity tests
int icamd_image_pipeline_u8(const void* workspace, int B, int max_crop_h, int out_h, int out_w, int kmax, const uint8_t** img) {
  if (workspace == nullptr || img == nullptr) return ICAMD_ERR_BAD_ARG;
  *img = image_ws(const_cast<void*>(workspace), B, tab_words(out_h, out_w, kmax), max_crop_h, out_h, out_w).img;
  return ICAMD_OK;
}

}  // extern "C"
