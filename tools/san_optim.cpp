// Stand-alone host check of the argument handling of devo_optim_chunks, devo_optim_moment_elems, devo_optim_plan, devo_optim_workspace_bytes
// and devo_optim_step (csrc/optim.hip) under AddressSanitizer and UBSan: every devo_optim_step call below is refused before the launch, and
// the plan is host code, so the program needs no GPU.  Host code only; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         devo_amd/csrc/optim.hip tools/san_optim.cpp -o /tmp/san_optim && /tmp/san_optim
// prints the refusals and "0 unexpected return codes" (exit status = the number of unexpected ones; a sanitizer report aborts).
#include <cstdio>
#include <cstdint>
#include <cstdarg>
#include <vector>
#include "../include/devo_hip.h"
namespace devo { void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); } }
int main() {
  alignas(16) double buf[64];
  alignas(16) static char ws_mem[1 << 15];
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  int bad = 0;
  // ---- the plan (host code: it runs here for real)
  const int C = DEVO_OPTIM_CHUNK;
  const int64_t numel[6] = {1, 3, 5, C, C + 1, 3 * C + 2};
  bad += devo_optim_chunks(numel, 6) != 1 + 1 + 1 + 1 + 2 + 4;
  bad += devo_optim_moment_elems(numel, 6) != 4 + 4 + 8 + C + (C + 4) + (3 * C + 4);
  std::vector<int32_t> table(4 * 10);
  int64_t offs[6];
  bad += devo_optim_plan(numel, 6, table.data(), offs) != DEVO_OK;
  const int64_t want_offs[6] = {0, 4, 8, 16, 16 + C, 20 + 2 * C};
  for (int t = 0; t < 6; ++t) bad += offs[t] != want_offs[t] || offs[t] % 4 != 0;
  const int32_t want[10][3] = {{0, 0, 1}, {1, 0, 3}, {2, 0, 5}, {3, 0, C}, {4, 0, C}, {4, C, 1}, {5, 0, C}, {5, C, C}, {5, 2 * C, C}, {5, 3 * C, 2}};
  for (int c = 0; c < 10; ++c) bad += table[4 * c] != want[c][0] || table[4 * c + 1] != want[c][1] || table[4 * c + 2] != want[c][2] || table[4 * c + 3] != 0;
  const int64_t big[2] = {INT32_MAX, 7};                                                          // the largest tensor: its last offset needs all 32 bits
  const int64_t big_chunks = devo_optim_chunks(big, 2);
  bad += big_chunks != ((int64_t)INT32_MAX + C - 1) / C + 1;
  std::vector<int32_t> big_table((size_t)(4 * big_chunks));
  bad += devo_optim_plan(big, 2, big_table.data(), offs) != DEVO_OK;
  bad += (uint32_t)big_table[(size_t)(4 * (big_chunks - 2) + 1)] != (uint32_t)(((int64_t)INT32_MAX - 1) / C * C) || big_table[(size_t)(4 * (big_chunks - 2) + 2)] != INT32_MAX % C;
  bad += big_table[(size_t)(4 * (big_chunks - 1))] != 1 || big_table[(size_t)(4 * (big_chunks - 1) + 2)] != 7 || offs[1] != (int64_t)INT32_MAX + 1;
  // sizes outside the limits
  const int64_t zero[2] = {4, 0}, neg[2] = {-1, 4}, huge[2] = {4, (int64_t)INT32_MAX + 1};
  for (const int64_t* s : {zero, neg, huge}) {
    bad += devo_optim_chunks(s, 2) != 0;
    bad += devo_optim_moment_elems(s, 2) != 0;
    bad += devo_optim_plan(s, 2, table.data(), offs) != DEVO_ERR_ARG;
  }
  for (int n : {0, -1, DEVO_OPTIM_MAX_TENSORS + 1, INT32_MIN}) {
    bad += devo_optim_chunks(numel, n) != 0;
    bad += devo_optim_moment_elems(numel, n) != 0;
    bad += devo_optim_plan(numel, n, table.data(), offs) != DEVO_ERR_ARG;
  }
  bad += devo_optim_chunks(nullptr, 6) != 0;
  bad += devo_optim_plan(nullptr, 6, table.data(), offs) != DEVO_ERR_ARG;
  bad += devo_optim_plan(numel, 6, nullptr, offs) != DEVO_ERR_ARG;
  bad += devo_optim_plan(numel, 6, table.data(), nullptr) != DEVO_ERR_ARG;
  bad += devo_optim_workspace_bytes() < (size_t)DEVO_OPTIM_MAX_PARTIALS * sizeof(double) || devo_optim_workspace_bytes() > sizeof(ws_mem);
  // ---- the step: everything below is refused before a launch
  const int32_t* tab = (const int32_t*)buf;
  const int64_t* tens = (const int64_t*)buf + 8;
  float *m = (float*)buf + 32, *v = (float*)buf + 64;
  int64_t* cnt = (int64_t*)buf + 48;
  double* gn = buf + 56;
  const void* grads[6] = {buf, nullptr, buf + 2, buf + 4, nullptr, buf + 6};
  const size_t wsb = devo_optim_workspace_bytes();
  struct A {
    const int32_t* tab; int64_t chunks; const int64_t* tens; const void* const* grads; const int64_t* numel; int n; float *m, *v;
    double lr, b1, b2, eps, wd, max_norm, bc1, bc2; int skip; int64_t* cnt; double* gn; void* ws; size_t wsb;
  };
  const A ok{tab, 10, tens, grads, numel, 6, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 10.0, 0.1, 0.001, 0, cnt, gn, ws_mem, wsb};
  auto call = [&](const A& a) {
    return devo_optim_step(a.tab, a.chunks, a.tens, a.grads, a.numel, a.n, a.m, a.v, a.lr, a.b1, a.b2, a.eps, a.wd, a.max_norm, a.bc1, a.bc2, a.skip, a.cnt, a.gn, a.ws, a.wsb,
                           nullptr);
  };
  auto refused = [&](A a) { bad += call(a) != DEVO_ERR_ARG; };
  A a = ok;
  a = ok, a.tab = nullptr, refused(a);                                                            // null pointers
  a = ok, a.tens = nullptr, refused(a);
  a = ok, a.grads = nullptr, refused(a);
  a = ok, a.numel = nullptr, refused(a);
  a = ok, a.m = nullptr, refused(a);
  a = ok, a.v = nullptr, refused(a);
  a = ok, a.gn = nullptr, refused(a);
  a = ok, a.ws = nullptr, refused(a);
  a = ok, a.tab = (const int32_t*)((char*)buf + 4), refused(a);                                   // misaligned tables, moments, outputs
  a = ok, a.tens = (const int64_t*)((char*)buf + 8), refused(a);
  a = ok, a.m = (float*)((char*)buf + 132), refused(a);
  a = ok, a.v = (float*)((char*)buf + 264), refused(a);
  a = ok, a.v = a.m, refused(a);                                                                  // one buffer for both moments
  a = ok, a.gn = (double*)((char*)buf + 4), refused(a);
  a = ok, a.ws = ws_mem + 4, refused(a);
  a = ok, a.wsb = wsb - 1, refused(a);                                                            // a workspace that is too small
  a = ok, a.wsb = 0, refused(a);
  for (int n : {0, -1, DEVO_OPTIM_MAX_TENSORS + 1}) a = ok, a.n = n, refused(a);                  // tensor counts and sizes outside the limits
  for (const int64_t* s : {zero, neg, huge}) a = ok, a.numel = s, a.n = 2, refused(a);
  for (int64_t c : {(int64_t)9, (int64_t)11, (int64_t)0, (int64_t)-1}) a = ok, a.chunks = c, refused(a);   // not the list's chunk count
  for (int t : {0, 2, 5}) {                                                                       // a gradient address that is not 16-byte aligned
    const void* g2[6] = {buf, nullptr, buf + 2, buf + 4, nullptr, buf + 6};
    g2[t] = (const char*)buf + 4 + 16 * t;
    a = ok, a.grads = g2, refused(a);
  }
  for (double x : {-1e-3, nan, inf, -inf}) a = ok, a.lr = x, refused(a);                          // hyperparameters
  for (double x : {-0.1, 1.0, 1.5, nan, inf}) {
    a = ok, a.b1 = x, refused(a);
    a = ok, a.b2 = x, refused(a);
  }
  for (double x : {-1e-8, nan, inf}) a = ok, a.eps = x, refused(a);
  for (double x : {-1e-2, nan, inf}) a = ok, a.wd = x, refused(a);
  a = ok, a.max_norm = nan, refused(a);
  for (double x : {0.0, -0.1, 1.5, nan, inf}) {                                                   // bias corrections outside (0, 1]
    a = ok, a.bc1 = x, refused(a);
    a = ok, a.bc2 = x, refused(a);
  }
  for (int s : {2, -1}) a = ok, a.skip = s, refused(a);
  a = ok, a.skip = 1, a.cnt = nullptr, refused(a);                                                // skip_nonfinite without its counters
  a = ok, a.skip = 1, a.cnt = (int64_t*)((char*)buf + 4), refused(a);
  printf("%d unexpected return codes\n", bad);
  return bad;
}
