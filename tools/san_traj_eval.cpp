// Stand-alone host check of devo_traj_eval's and devo_traj_rel_eval's argument handling (csrc/traj_eval.hip, csrc/traj_rel.hip, their shared
// csrc/traj_dev.h) under AddressSanitizer and UBSan: every call below is refused before the launch, so the program needs no GPU.  Host code
// only; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         devo_amd/csrc/traj_eval.hip devo_amd/csrc/traj_rel.hip tools/san_traj_eval.cpp -o /tmp/san_traj_eval && /tmp/san_traj_eval
// prints the 13 + 20 refusals and "0 unexpected return codes" (exit status = the number of unexpected ones; a sanitizer report aborts).
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

  // ---- devo_traj_rel_eval: its workspace holds the evaluation launch's, whatever the association; a negative total counts as empty
  for (int assoc : {DEVO_TRAJ_ASSOC_NEAREST, DEVO_TRAJ_ASSOC_INTERPOLATE}) {
    bad += devo_traj_rel_workspace_bytes(8, assoc, 1, 2) < devo_traj_eval_workspace_bytes(8, assoc);
    bad += devo_traj_rel_workspace_bytes(-5, assoc, 1, 2) != devo_traj_rel_workspace_bytes(0, assoc, 1, 2);
  }
  alignas(16) static char wsb[32768];
  const size_t rneed = devo_traj_rel_workspace_bytes(8, DEVO_TRAJ_ASSOC_NEAREST, 1, 2);
  bad += rneed + 8 > sizeof(wsb);
  struct Rel {
    int B = 1, D = 2, dtype = DEVO_F64, unit = DEVO_TRAJ_REL_UNIT_FRAMES, along = DEVO_TRAJ_REL_ALONG_GT, end = DEVO_TRAJ_REL_END_REACH;
    int mode = DEVO_TRAJ_REL_SCALE_VALUE;
    int64_t ne = 8;
    double scale = 1.0, delta1 = 2.0;
    bool no_deltas = false, no_stats = false;
    const double* scale_v = nullptr;
    size_t short_by = 0, shift = 0;
  };
  auto rel = [&](const Rel& r) {
    double deltas[DEVO_TRAJ_REL_MAX_DELTAS + 1];
    for (double& x : deltas) x = 1.0;
    deltas[1] = r.delta1;
    return devo_traj_rel_eval(d, d, off, r.ne, d, d, off, 8, r.B, r.dtype, 0, DEVO_TRAJ_ASSOC_NEAREST, 1.0, r.no_deltas ? nullptr : deltas, r.D, r.unit, 0, r.along,
                              r.end, r.mode, r.scale, r.scale_v, r.no_stats ? nullptr : d, st, nullptr, nullptr, wsb + r.shift, rneed - r.short_by, nullptr);
  };
  const double inf = __builtin_inf();
  Rel r;
  r = Rel(); r.B = 0; bad += rel(r) != DEVO_ERR_ARG;                                           // no pair
  r = Rel(); r.D = 0; bad += rel(r) != DEVO_ERR_ARG;                                           // no delta
  r = Rel(); r.D = DEVO_TRAJ_REL_MAX_DELTAS + 1; bad += rel(r) != DEVO_ERR_ARG;                // too many deltas
  r = Rel(); r.no_deltas = true; bad += rel(r) != DEVO_ERR_ARG;                                // null deltas
  for (double x : {0.0, -1.0, inf, nan}) { r = Rel(); r.delta1 = x; bad += rel(r) != DEVO_ERR_ARG; }   // a delta of 0, negative, inf, NaN
  r = Rel(); r.unit = DEVO_TRAJ_REL_UNIT_DEGREES + 1; bad += rel(r) != DEVO_ERR_ARG;           // unknown unit
  r = Rel(); r.along = 2; bad += rel(r) != DEVO_ERR_ARG;                                       // unknown along
  r = Rel(); r.end = 2; bad += rel(r) != DEVO_ERR_ARG;                                         // unknown end rule
  r = Rel(); r.mode = DEVO_TRAJ_REL_SCALE_PER_PAIR + 1; bad += rel(r) != DEVO_ERR_ARG;         // unknown scale mode
  r = Rel(); r.scale = 0.0; bad += rel(r) != DEVO_ERR_ARG;                                     // a given scale of 0
  r = Rel(); r.scale = inf; bad += rel(r) != DEVO_ERR_ARG;                                     // and of inf
  r = Rel(); r.mode = DEVO_TRAJ_REL_SCALE_PER_PAIR; bad += rel(r) != DEVO_ERR_ARG;             // per-pair scales missing
  r = Rel(); r.no_stats = true; bad += rel(r) != DEVO_ERR_ARG;                                 // no output
  r = Rel(); r.ne = -1; bad += rel(r) != DEVO_ERR_ARG;                                         // negative total
  r = Rel(); r.short_by = 1; bad += rel(r) != DEVO_ERR_WORKSPACE;                              // short workspace
  r = Rel(); r.shift = 8; bad += rel(r) != DEVO_ERR_WORKSPACE;                                 // misaligned workspace
  r = Rel(); r.dtype = DEVO_F16; bad += rel(r) != DEVO_ERR_ARG;                                // fp16 poses: the inner devo_traj_eval's refusal
  printf("%d unexpected return codes\n", bad);
  return bad;
}
