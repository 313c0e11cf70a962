// Stand-alone host check of devo_patch_select's argument handling (csrc/select.hip) under AddressSanitizer and UBSan: every call below is
// refused before the launch, so the program needs no GPU.  Host code only; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         devo_amd/csrc/select.hip tools/san_select.cpp -o /tmp/san_select && /tmp/san_select
// prints the 14 refusals and "0 unexpected return codes" (exit status = the number of unexpected ones; a sanitizer report aborts).
#include <cstdio>
#include <cstdint>
#include <cstdarg>
#include "../include/devo_hip.h"
namespace devo { void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); } }
int main() {
  float f[4]; int64_t i[4]; int c[4];
  int bad = 0;
  auto call = [&](int n, int h, int w, int m, int mode, int grid, int k, int pad, const float* noise, const int64_t* cx, int P, int* counts) {
    return devo_patch_select(f, 1, 1, 1, n, h, w, m, mode, grid, k, pad, noise, cx, cx, 0, 0, 0, 0, 0, 0, nullptr, 0, 0, 0, 0, 0, P, i, i, f, f, f, i, counts, nullptr);
  };
  bad += call(1, 8, 8, 4, 9, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;          // unknown mode
  bad += call(1, 8, 8, 4, DEVO_SELECT_TOPK, 1, 8, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_UNSUPPORTED;   // k
  bad += call(1, 8, 8, 4, DEVO_SELECT_MULTI, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;         // no noise
  bad += call(1, 8, 8, 4, DEVO_SELECT_NMS, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;           // no counts
  bad += call(1, 8, 8, 4, DEVO_SELECT_3XRANDOM, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;      // no candidates
  bad += call(1, 8, 8, 4, DEVO_SELECT_TOPK, 1, 4, 0, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;          // unpadded topk
  bad += call(1, 264, 256, 4, DEVO_SELECT_TOPK, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_UNSUPPORTED;  // 4224 cells
  bad += call(1, 8, 8, 6, DEVO_SELECT_TOPK, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;          // m % 4
  bad += call(1, 8, 8, 8, DEVO_SELECT_TOPK, 0, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;          // m > C
  bad += call(1, 8, 8, 5000, DEVO_SELECT_NMS, 0, 4, 1, nullptr, nullptr, 3, c) != DEVO_ERR_UNSUPPORTED;      // m > 4096
  bad += call(1, 8, 8, 2000, DEVO_SELECT_3XRANDOM, 0, 4, 1, nullptr, i, 3, nullptr) != DEVO_ERR_UNSUPPORTED; // 3 m > 4096
  bad += call(1, 2147483647, 2147483647, 4, DEVO_SELECT_TOPK, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_UNSUPPORTED;  // huge map
  bad += call(0, 8, 8, 4, DEVO_SELECT_TOPK, 1, 4, 1, nullptr, nullptr, 3, nullptr) != DEVO_ERR_ARG;
  bad += call(1, 8, 8, 4, DEVO_SELECT_TOPK, 1, 4, 1, nullptr, nullptr, 99, nullptr) != DEVO_ERR_ARG;
  printf("%d unexpected return codes\n", bad);
  return bad;
}
