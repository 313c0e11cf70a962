// Stand-alone host check of devo_traj_eval's argument handling (csrc/traj_eval.hip) under AddressSanitizer and UBSan: every call below is
// refused before the launch, so the program needs no GPU.  Host code only; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         devo_amd/csrc/traj_eval.hip tools/san_traj_eval.cpp -o /tmp/san_traj_eval && /tmp/san_traj_eval
// prints the 13 refusals and "0 unexpected return codes" (exit status = the number of unexpected ones; a sanitizer report aborts).
#include <cstdio>
#include <cstdint>
#include <cstdarg>
#include "../include/devo_hip.h"
namespace devo { void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); } }
int main() {
  alignas(16) double d[64]; int64_t off[4]; int st[4];
  int bad = 0;
  const size_t need = devo_traj_eval_workspace_bytes(8, DEVO_TRAJ_ASSOC_NEAREST);
  bad += need < 8 * (2 * sizeof(int) + sizeof(double));
  bad += devo_traj_eval_workspace_bytes(8, DEVO_TRAJ_ASSOC_INTERPOLATE) < need + 8 * 7 * sizeof(double);
  bad += devo_traj_eval_workspace_bytes(-5, DEVO_TRAJ_ASSOC_NEAREST) == 0;          // a negative total counts as empty: never a huge size
  auto call = [&](int B, int64_t ne, int64_t ng, int dtype, int assoc, int align, double max_diff, int delta, const void* est, const int64_t* eo, double* stats,
                  void* ws, size_t bytes) {
    return devo_traj_eval(est, d, eo, ne, d, d, off, ng, B, dtype, 0, assoc, align, max_diff, delta, stats, d, st, nullptr, nullptr, ws, bytes, nullptr);
  };
  const double nan = __builtin_nan("");
  bad += call(0, 8, 8, DEVO_F64, 0, 2, 1.0, 0, d, off, d, d, need) != DEVO_ERR_ARG;            // no pair
  bad += call(1, -1, 8, DEVO_F64, 0, 2, 1.0, 0, d, off, d, d, need) != DEVO_ERR_ARG;           // negative total
  bad += call(1, 8, 8, DEVO_F64, 0, 2, 1.0, 0, d, nullptr, d, d, need) != DEVO_ERR_ARG;        // no offsets
  bad += call(1, 8, 8, DEVO_F64, 0, 2, 1.0, 0, d, off, nullptr, d, need) != DEVO_ERR_ARG;      // no output
  bad += call(1, 8, 8, DEVO_F64, 0, 2, 1.0, 0, nullptr, off, d, d, need) != DEVO_ERR_ARG;      // poses missing
  bad += call(1, 8, 8, DEVO_F16, 0, 2, 1.0, 0, d, off, d, d, need) != DEVO_ERR_ARG;            // fp16 poses
  bad += call(1, 8, 8, DEVO_F64, 2, 2, 1.0, 0, d, off, d, d, need) != DEVO_ERR_ARG;            // unknown association
  bad += call(1, 8, 8, DEVO_F64, 0, 3, 1.0, 0, d, off, d, d, need) != DEVO_ERR_ARG;            // unknown alignment
  bad += call(1, 8, 8, DEVO_F64, 0, 2, -1.0, 0, d, off, d, d, need) != DEVO_ERR_ARG;           // negative max_diff
  bad += call(1, 8, 8, DEVO_F64, 0, 2, nan, 0, d, off, d, d, need) != DEVO_ERR_ARG;            // NaN max_diff
  bad += call(1, 8, 8, DEVO_F64, 0, 2, 1.0, -1, d, off, d, d, need) != DEVO_ERR_ARG;           // negative rpe_delta
  bad += call(1, 8, 8, DEVO_F64, 0, 2, 1.0, 0, d, off, d, d, need - 1) != DEVO_ERR_WORKSPACE;  // short workspace
  bad += call(1, 8, 8, DEVO_F64, 0, 2, 1.0, 0, d, off, d, (char*)d + 8, need) != DEVO_ERR_WORKSPACE;   // misaligned workspace
  printf("%d unexpected return codes\n", bad);
  return bad;
}
