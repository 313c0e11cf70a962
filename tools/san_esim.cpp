// Stand-alone host check of the argument handling of devo_esim_count, devo_esim_emit, devo_esim_sort_keys, devo_esim_decode,
// devo_esim_max_span_ns and devo_log_intensity (csrc/esim.hip) under AddressSanitizer and UBSan: every call below is refused before the
// launch, or has nothing to launch, so the program needs no GPU.  Host code only; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         devo_amd/csrc/esim.hip tools/san_esim.cpp -o /tmp/san_esim && /tmp/san_esim
// prints the refusals and "0 unexpected return codes" (exit status = the number of unexpected ones; a sanitizer report aborts).
#include <cstdio>
#include <cstdint>
#include <cstdarg>
#include "../include/devo_hip.h"
namespace devo { void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); } }
int main() {
  alignas(16) double buf[64];
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const float* f = (const float*)buf;
  const int64_t* l = (const int64_t*)buf;
  int64_t* lo = (int64_t*)buf;
  const float* f_odd = (const float*)((char*)buf + 2);
  const int64_t* l_odd = (const int64_t*)((char*)buf + 4);
  int bad = 0;
  // ---- the arguments the two passes share: (prev, frames, prev_stamp, stamps, T, H, W, ref, last_t, c_neg, c_pos, refractory_ns)
  for (int pass = 0; pass < 2; ++pass) {
    auto call = [&](const float* prev, const float* frames, const int64_t* ps, const int64_t* st, int T, int H, int W, const double* ref, const int64_t* last, double cn, double cp,
                    int64_t refr) {
      return pass == 0 ? devo_esim_count(prev, frames, ps, st, T, H, W, ref, last, cn, cp, refr, lo + 8, lo + 16, nullptr)
                       : devo_esim_emit(prev, frames, ps, st, T, H, W, ref, last, cn, cp, refr, l + 8, 4, lo + 16, buf + 24, lo + 32, nullptr);
    };
    bad += call(nullptr, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;                 // null tensors
    bad += call(f, nullptr, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, nullptr, l, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l, nullptr, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l, l, 2, 4, 4, nullptr, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l, l, 2, 4, 4, buf, nullptr, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    for (int T : {0, -1, INT32_MIN}) bad += call(f, f, l, l, T, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;      // no frame pair
    for (int side : {0, -4, DEVO_ESIM_MAX_SIDE + 1, INT32_MAX}) {                                 // frame sides outside 1 .. 32767
      bad += call(f, f, l, l, 2, side, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
      bad += call(f, f, l, l, 2, 4, side, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    }
    for (double c : {0.0, -0.2, 9.9e-4, nan, inf, -inf}) {                                        // thresholds below 1e-3 or not finite
      bad += call(f, f, l, l, 2, 4, 4, buf, l, c, 0.2, 0) != DEVO_ERR_ARG;
      bad += call(f, f, l, l, 2, 4, 4, buf, l, 0.2, c, 0) != DEVO_ERR_ARG;
    }
    for (int64_t r : {(int64_t)-1, INT64_MIN}) bad += call(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, r) != DEVO_ERR_ARG;   // negative refractory period
    bad += call(f_odd, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;                    // misaligned tensors
    bad += call(f, f_odd, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l_odd, l, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l, l_odd, 2, 4, 4, buf, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l, l, 2, 4, 4, (const double*)l_odd, l, 0.2, 0.2, 0) != DEVO_ERR_ARG;
    bad += call(f, f, l, l, 2, 4, 4, buf, l_odd, 0.2, 0.2, 0) != DEVO_ERR_ARG;
  }
  // ---- the outputs of each pass
  bad += devo_esim_count(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, nullptr, lo, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_count(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, lo, nullptr, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_count(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, (int64_t*)l_odd, lo, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_count(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, lo, (int64_t*)l_odd, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l, -1, lo + 16, buf + 24, lo + 32, nullptr) != DEVO_ERR_ARG;        // negative total
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, nullptr, 4, lo + 16, buf + 24, lo + 32, nullptr) != DEVO_ERR_ARG;  // null tensors
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l, 4, nullptr, buf + 24, lo + 32, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l, 4, lo + 16, nullptr, lo + 32, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l, 4, lo + 16, buf + 24, nullptr, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l_odd, 4, lo + 16, buf + 24, lo + 32, nullptr) != DEVO_ERR_ARG;    // misaligned
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l, 4, (int64_t*)l_odd, buf + 24, lo + 32, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l, 0.2, 0.2, 0, l, 4, lo + 16, buf, lo + 32, nullptr) != DEVO_ERR_ARG;             // new state aliases the old
  bad += devo_esim_emit(f, f, l, l, 2, 4, 4, buf, l + 40, 0.2, 0.2, 0, l, 4, lo + 16, buf + 24, lo + 40, nullptr) != DEVO_ERR_ARG;
  // ---- the sort: everything refused before rocPRIM is asked for its workspace
  bad += devo_esim_sort_keys(l, lo + 16, -1, 4, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, lo + 16, 8, 0, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, lo + 16, 8, 4, DEVO_ESIM_MAX_SIDE + 1, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, lo + 16, 8, 4, 4, -1, buf + 32, 64, nullptr) != DEVO_ERR_ARG;                                          // spans the key cannot hold
  bad += devo_esim_sort_keys(l, lo + 16, 8, 4, 4, devo_esim_max_span_ns(4, 4), buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(nullptr, lo + 16, 8, 4, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, nullptr, 8, 4, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, lo, 8, 4, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;                                              // in place
  bad += devo_esim_sort_keys(l_odd, lo + 16, 8, 4, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, (int64_t*)l_odd, 8, 4, 4, 1000, buf + 32, 64, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_sort_keys(l, lo + 16, 8, 4, 4, 1000, (char*)buf + 8, 64, nullptr) != DEVO_ERR_ARG;                                   // misaligned workspace
  bad += devo_esim_sort_keys(nullptr, nullptr, 0, 4, 4, 1000, nullptr, 0, nullptr) != DEVO_OK;                                          // no key: accepted without a launch
  bad += devo_esim_sort_workspace_bytes(0, 4, 4, 1000) != 0;
  bad += devo_esim_sort_workspace_bytes(-5, 4, 4, 1000) != 0;
  bad += devo_esim_sort_workspace_bytes(8, 0, 4, 1000) != 0;
  bad += devo_esim_sort_workspace_bytes(8, 4, 4, -1) != 0;
  // ---- decode
  int16_t* h = (int16_t*)buf;
  signed char* c = (signed char*)buf;
  bad += devo_esim_decode(l, -1, 4, 4, l, h, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 0, 4, l, h, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, DEVO_ESIM_MAX_SIDE + 1, l, h, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, nullptr, h, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(nullptr, 8, 4, 4, l, h, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, l, nullptr, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, l, h, nullptr, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, l, h, h, nullptr, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, l, h, h, lo, nullptr, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l_odd, 8, 4, 4, l, h, h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, l, (int16_t*)((char*)buf + 1), h, lo, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(l, 8, 4, 4, l, h, h, (int64_t*)l_odd, c, nullptr) != DEVO_ERR_ARG;
  bad += devo_esim_decode(nullptr, 0, 4, 4, l, nullptr, nullptr, nullptr, nullptr, nullptr) != DEVO_OK;     // no event: accepted without a launch
  // ---- the key's limit
  bad += devo_esim_max_span_ns(480, 640) != (int64_t)1 << 43;
  bad += devo_esim_max_span_ns(1, 1) != (int64_t)1 << 61;
  bad += devo_esim_max_span_ns(5, 7) != (int64_t)1 << 56;
  bad += devo_esim_max_span_ns(64, 64) != (int64_t)1 << 50;
  bad += devo_esim_max_span_ns(DEVO_ESIM_MAX_SIDE, DEVO_ESIM_MAX_SIDE) != (int64_t)1 << 32;
  for (int side : {0, -1, DEVO_ESIM_MAX_SIDE + 1, INT32_MAX, INT32_MIN}) bad += (devo_esim_max_span_ns(side, 4) != 0) + (devo_esim_max_span_ns(4, side) != 0);
  // ---- log intensity
  const unsigned char* u = (const unsigned char*)buf;
  float* fo = (float*)buf + 8;
  bad += devo_log_intensity(u, -1, f, fo, nullptr) != DEVO_ERR_ARG;
  bad += devo_log_intensity(u, 16, nullptr, fo, nullptr) != DEVO_ERR_ARG;
  bad += devo_log_intensity(nullptr, 16, f, fo, nullptr) != DEVO_ERR_ARG;
  bad += devo_log_intensity(u, 16, f, nullptr, nullptr) != DEVO_ERR_ARG;
  bad += devo_log_intensity(u, 16, f_odd, fo, nullptr) != DEVO_ERR_ARG;
  bad += devo_log_intensity(u, 16, f, (float*)((char*)buf + 2), nullptr) != DEVO_ERR_ARG;
  bad += devo_log_intensity(nullptr, 0, f, nullptr, nullptr) != DEVO_OK;                          // nothing to do
  printf("%d unexpected return codes\n", bad);
  return bad;
}
