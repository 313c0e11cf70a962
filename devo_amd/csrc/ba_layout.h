// The fastba workspace as the host sees it — shared by ba.hip (Gauss-Newton kernels, their dispatch) and ba_tables.hip (the graph index
// tables every BA call and the Update operator start from): the layout, the limits it depends on, and the few host functions one unit
// calls in the other.
#pragma once
#include "common.h"

namespace devo {

constexpr int BA_MAXN_LDS = 32;      // optimised poses per call whose system (6N <= 192 rows) lives in LDS
constexpr int BA_MAXN = 128;         // beyond BA_MAXN_LDS: the system stays in global memory (device atomics, k_ba_solve_t<true>); the limit is
                                     // the solver's LDS tables (factored diagonal blocks + inverses) and ba_sig's 8 bits for N
constexpr int ACC_MAX_WG = 256;      // partial systems written per iteration
constexpr int SCH_T = 32, SCH_K = 128;   // k_ba_schur's tile: SCH_T x SCH_T outputs per workgroup, SCH_K patches per chunk

struct BaMeta { int n_seg; int fail; int sig; int pad; };   // sig: what the workspace was prepared for (ba_sig)
__host__ __device__ __forceinline__ int ba_sig(int E, int N) { return (int)(0x5ec0de00u ^ ((unsigned)E * 2654435761u) ^ ((unsigned)N << 24)); }

// ------------------------------------------------------------------------------------------------- workspace
struct BaLayout {
  size_t meta, rank, counts, cursor, ku, perm_a, perm_b, kx, range, partials, S, y, dX, patch_rec, edge_ej, prec, ybar, total, partials_bytes;
  int max_seg, n_part;
};
// Waves per workgroup of the register-path accumulate kernel (N <= 16): what 160 KB of LDS hold — WAVES slabs + scratch + the atomic-path
// system.  (Above 16 poses: the 4 that size the general kernel's partials.)
inline int acc_waves(int N) { return N <= 11 ? 8 : N <= 14 ? 6 : 4; }

inline BaLayout ba_layout(int E, int Np, int N) {
  BaLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
  L.max_seg = E < Np ? E : Np;
  if (L.max_seg < 1) L.max_seg = 1;
  const int waves = acc_waves(N);
  int want = (L.max_seg + waves - 1) / waves;
  L.n_part = want < ACC_MAX_WG ? (want < 1 ? 1 : want) : ACC_MAX_WG;
  const size_t n6 = 6 * (size_t)N;
  L.meta = take(sizeof(BaMeta));
  L.rank = take(sizeof(int) * ((size_t)Np + 1));
  L.counts = take(sizeof(int) * ((size_t)L.max_seg + 1));
  L.cursor = take(sizeof(int) * (size_t)L.max_seg);
  L.ku = take(sizeof(int) * (size_t)(E > 0 ? E : 1));
  L.perm_a = take(sizeof(int) * (size_t)(E > 0 ? E : 1));
  L.perm_b = take(sizeof(int) * (size_t)(E > 0 ? E : 1));
  L.kx = take(sizeof(int) * (size_t)L.max_seg);
  L.range = take(sizeof(int) * 4);                                  // the multi-kernel preparation's id range
  L.partials_bytes = sizeof(float) * (size_t)L.n_part * (n6 * (n6 + 1) + n6 + 1);
  if (N > BA_MAXN_LDS) {                                            // no partial systems: the area only holds k_ba_schur's partial tiles
    const size_t nt = (n6 + 1 + SCH_T - 1) / SCH_T, ntile = nt * (nt + 1) / 2, nchunk = ((size_t)L.max_seg + SCH_K - 1) / SCH_K;
    L.partials_bytes = sizeof(float) * ntile * nchunk * SCH_T * SCH_T;
    if (L.partials_bytes > ((size_t)64 << 20)) L.partials_bytes = 16;   // (k_ba_schur then adds with atomics)
  }
  L.partials = take(L.partials_bytes);
  L.S = take(sizeof(float) * ((n6 + 1) * (n6 + 1) + 1));
  L.y = take(sizeof(float) * (n6 + 1));
  L.dX = take(sizeof(float) * (n6 + 1));
  L.patch_rec = take(sizeof(float) * 2 * (size_t)L.max_seg);
  L.edge_ej = take(sizeof(float) * (size_t)L.max_seg * (n6 > 0 ? n6 : 1));      // E column of every patch
  L.prec = take(sizeof(float) * 8 * (size_t)L.max_seg);                          // backward of devo_ba_solve_terms: per-patch adjoints
  L.ybar = take(sizeof(float) * (n6 + 1));
  L.total = off;
  return L;
}

// ------------------------------------------------------------------------------------------------- ba_tables.hip, called from ba.hip
struct PlanRider { int* plan; int nbins; int starts; };          // a plan buffer whose bins devo_transform has written: ordered during the BA
// The plan's geometry (frames, height; width and level ratio of a GROUP plan) -> the rider; `who` names the entry point in the error text.
__attribute__((visibility("hidden"))) int ba_plan_rider(const char* who, int* plan, int frames, int height, int width, int l1, PlanRider* rider);
// The plan's ordering step on its own: the only dispatch of k_order_only.
__attribute__((visibility("hidden"))) void launch_order_only(hipStream_t st, int E, const PlanRider& r);
// Graph preparation: kx = unique(kk) sorted, ku = inverse (ba_cuda.cu:435-437), edges grouped by patch.  rider.plan != NULL: also finish the
// lookup's locality plan (bins at plan + E + 1, see devo_transform) — in the same launch when the single-workgroup path is taken, else
// with the plan's own kernel.
__attribute__((visibility("hidden"))) int ba_prepare_impl(const int64_t* kk, int E, int Np, int N, void* ws, size_t ws_bytes, hipStream_t st,
                                                          PlanRider rider = PlanRider{nullptr, 0, 0});

}  // namespace devo
