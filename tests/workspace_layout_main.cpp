// Stand-alone check of csrc/workspace.h, built by tests/test_workspace_layout_cpu.py with -fsanitize=address,undefined.
// Reads one layout case per line from standard input:
//   reduce C part_rows scratch_rows | se N S C | grn N S C | image B tab_words max_crop_h out_h out_w |
//   image_aug B tab_words max_crop_h out_h out_w aux_per_image | wgrad S Cout Ktot
// For each it asks the layout for its size (null base: every pointer must come back null), allocates a block of EXACTLY that many
// bytes, carves it and writes every byte the kernels may touch in every region -- the extents below are stated from the kernels'
// indexing, not taken from the header -- so a total that falls short of its carve is an AddressSanitizer report.  It prints
//   <kind> <bytes> <offset of region 0> <offset of region 1> ...
#include "../imageclassification_amd/csrc/workspace.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Region { const void* p; size_t extent; };

static int fail(const char* what, const char* line) {
  fprintf(stderr, "workspace_layout_main: %s: %s\n", what, line);
  return 1;
}

// writes the regions of a carved block and prints the offsets; `sized` holds the pointers of the null-base call
static int check(const char* kind, size_t bytes, size_t bytes_sized, char* base, const std::vector<Region>& sized,
                 const std::vector<Region>& carved, const char* line) {
  if (bytes != bytes_sized) return fail("the size differs between a null and a real base", line);
  for (const Region& r : sized)
    if (r.p != nullptr) return fail("a null base gave a pointer", line);
  printf("%s %zu", kind, bytes);
  for (const Region& r : carved) {
    if (r.extent) memset((void*)r.p, 0xA5, r.extent);
    printf(" %zu", (size_t)((const char*)r.p - base));
  }
  printf("\n");
  return 0;
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    char kind[32];
    long long a[6] = {0, 0, 0, 0, 0, 0};
    const int n = sscanf(line, "%31s %lld %lld %lld %lld %lld %lld", kind, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) - 1;
    if (n < 0) continue;
    int rc;
    if (!strcmp(kind, "reduce") && n == 3) {
      const int C = (int)a[0], k = (int)a[2];
      const long long rows = a[1];
      const ReduceWs s = reduce_ws(nullptr, C, rows, k);
      char* base = (char*)malloc(s.bytes);
      const ReduceWs w = reduce_ws(base, C, rows, k);
      const size_t c = (size_t)C;
      rc = check(kind, w.bytes, s.bytes, base, {{s.counters, 0}, {s.chunks, 0}, {s.part, 0}, {s.scratch, 0}},
                 {{w.counters, 256}, {w.chunks, 64 * 2 * c * sizeof(double)}, {w.part, (size_t)rows * 2 * c * sizeof(float)},
                  {w.scratch, (size_t)k * c * sizeof(float)}}, line);
      free(base);
    } else if (!strcmp(kind, "se") && n == 3) {
      const int N = (int)a[0], S = (int)a[1], C = (int)a[2];
      const SeBwdWs s = se_bwd_ws(nullptr, N, S, C);
      char* base = (char*)malloc(s.bytes);
      const SeBwdWs w = se_bwd_ws(base, N, S, C);
      const size_t nc = (size_t)N * C * sizeof(float);
      rc = check(kind, w.bytes, s.bytes, base, {{s.part, 0}, {s.AB, 0}, {s.dp2, 0}, {s.ds, 0}, {s.k0, 0}, {s.dh, 0}, {s.k2, 0}},
                 {{w.part, (size_t)S * 2 * nc}, {w.AB, 2 * nc}, {w.dp2, nc}, {w.ds, nc}, {w.k0, nc},
                  {w.dh, (size_t)N * 256 * sizeof(float)}, {w.k2, (size_t)C * sizeof(float)}}, line);
      free(base);
    } else if (!strcmp(kind, "grn") && n == 3) {
      const int N = (int)a[0], S = (int)a[1], C = (int)a[2];
      const GrnWs s = grn_ws(nullptr, N, S, C);
      char* base = (char*)malloc(s.bytes);
      const GrnWs w = grn_ws(base, N, S, C);
      const size_t row = (size_t)N * 2 * C * sizeof(float);
      rc = check(kind, w.bytes, s.bytes, base, {{s.part, 0}, {s.fin, 0}}, {{w.part, (size_t)S * row}, {w.fin, row}}, line);
      free(base);
    } else if (!strcmp(kind, "image") && n == 5) {
      const int B = (int)a[0], mch = (int)a[2], oh = (int)a[3], ow = (int)a[4];
      const ImageWs s = image_ws(nullptr, B, a[1], mch, oh, ow);
      char* base = (char*)malloc(s.bytes);
      const ImageWs w = image_ws(base, B, a[1], mch, oh, ow);
      rc = check(kind, w.bytes, s.bytes, base, {{s.tabs, 0}, {s.tmp, 0}, {s.img, 0}},
                 {{w.tabs, (size_t)B * a[1] * 4}, {w.tmp, (size_t)B * mch * ow * 3}, {w.img, (size_t)B * oh * ow * 3}}, line);
      free(base);
    } else if (!strcmp(kind, "image_aug") && n == 6) {
      const int B = (int)a[0], mch = (int)a[2], oh = (int)a[3], ow = (int)a[4], aux = (int)a[5];
      const ImageAugWs s = image_aug_ws(nullptr, B, a[1], mch, oh, ow, aux);
      char* base = (char*)malloc(s.bytes);
      const ImageAugWs w = image_aug_ws(base, B, a[1], mch, oh, ow, aux);
      const size_t img = (size_t)B * oh * ow * 3;
      rc = check(kind, w.bytes, s.bytes, base, {{s.tabs, 0}, {s.tmp, 0}, {s.img, 0}, {s.img2, 0}, {s.aux, 0}},
                 {{w.tabs, (size_t)B * a[1] * 4}, {w.tmp, (size_t)B * mch * ow * 3}, {w.img, img}, {w.img2, img},
                  {w.aux, (size_t)B * aux}}, line);
      free(base);
    } else if (!strcmp(kind, "wgrad") && n == 3) {
      const int S = (int)a[0], Cout = (int)a[1], Ktot = (int)a[2];
      const WgradWs s = wgrad_ws(nullptr, S, Cout, Ktot);
      char* base = (char*)malloc(s.bytes);
      const WgradWs w = wgrad_ws(base, S, Cout, Ktot);
      const size_t sc = (size_t)S * Cout * sizeof(float);
      rc = check(kind, w.bytes, s.bytes, base, {{s.slab, 0}, {s.bias_slab, 0}}, {{w.slab, sc * Ktot}, {w.bias_slab, sc}}, line);
      free(base);
    } else {
      rc = fail("unknown case", line);
    }
    if (rc) return rc;
  }
  return 0;
}
