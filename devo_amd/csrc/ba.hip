// fastba for gfx950: sparse Gauss-Newton bundle adjustment (inference variant) and the differentiable Gauss-Newton step of training.
// Replaces devo/fastba/ba_cuda.cu + ba.cpp (module cuda_ba, ba.cpp:152-157); the graph index tables are ba_tables.hip's, the fused
// reprojection (devo/projective_ops.py:53-105) transform.hip's.
//
// Design.  The reference accumulates the normal equations with 340 global float
// atomics per edge onto a few thousand addresses, then runs ~20 ATen launches + cuSOLVER (host sync) per
// Gauss-Newton iteration.  Here the edge list is grouped by patch once per call (ba_tables.hip: integer counting sort,
// bit-exact `unique`), and each iteration is four launches with no host synchronisation:
//   ba_accumulate : one WAVE per patch.  Lanes = the patch's edges.  Per-patch quantities (C, u, the
//                   source-frame E block, B_ii, v_i) are reduced with wavefront shuffles; the patch's
//                   column of E is completed in LDS, the Schur update  S -= Q e e^T, y -= Q u e  is
//                   applied patch-by-patch into an LDS-resident lower-triangular S (dense E is never
//                   materialised); one partial S per workgroup goes to HBM.
//   ba_reduce     : sums the partials in a fixed order, mirrors the triangle, applies the damping.
//   ba_solve      : one workgroup, LDS-resident blocked (6x6) Cholesky with the right-hand side carried as
//                   an extra row, blocked back-substitution.
//   ba_retract    : pose retraction Exp(dX) * G and per-patch depth update  dz = Q (u - e^T dX).
#include "ba_layout.h"
#include <cstddef>
#include "se3_dev.h"
#include "corr_tile.h"
#include "corr_plan.h"
#include <stdlib.h>
#include <type_traits>

namespace devo {

constexpr int ACC_WAVES = 8;         // waves per ba_accumulate workgroup
constexpr int ACC_THREADS = ACC_WAVES * 64;

// ------------------------------------------------------------------------------------------------- utilities
// Sum over the 64 lanes, returned to every lane.  Round 6: DPP adds on the vector ALU — the scan of corr_tile.h's wave_inclusive_sum (row_shr
// 1 / 2 / 4 / 8, row_bcast 15 / 31), the total in lane 63, v_readlane — where rounds 1-5 used a butterfly (six ds_bpermute round trips through the
// LDS crossbar per value).  All 64 lanes must be active (every caller's are).  The order of the additions differs from the butterfly's: results
// moved in the last bits, every kernel of this file uses the same form.
__device__ __forceinline__ float wave_sum(float v) {
  auto dpp = [](float x, auto ctrl, auto rows) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, decltype(rows)::value, 0xf, false)); };
  v += dpp(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
  v += dpp(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
  v += dpp(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
  v += dpp(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
  v += dpp(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
  v += dpp(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v |= (unsigned)__shfl_xor((int)v, off);
  return v;
}
__device__ __forceinline__ float readlane_f(float v, int lane) {       // lane must be wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ void lds_add(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int ftab_lookup(int my_le, int f) { return __shfl(my_le, f); }   // lane f holds table entry f
// LDS traffic of ONE wave is processed in order; this only stops the compiler from moving accesses across.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------- per-edge maths
struct EdgeTerms {
  float r[2], w[2], Jz[2];
  float Ji[2][6], Jj[2][6];
};

// Where an edge's target comes from: t[2e + c] alone, or (devo.py:330 folded in) the centre pixel of the reprojected patch
// plus the update operator's delta: base[e * se + c * sc + off] + t[2e + c] — the same single fp32 addition torch does.
struct TargetSrc { const float* t; const float* base; int se, sc, off; const float* terms; };
// terms != NULL (devo_ba_solve_terms): the per-edge residual / weight / Jacobians are GIVEN — 30 floats per edge:
// r[2] w[2] Jz[2] Ji[2][6] Jj[2][6], in this file's sign convention (v_i -= w r Ji, i.e. Ji = -d coords / d xi_i).
constexpr int BA_TERMS = 30;

// ba_cuda.cu:239-330 for one edge (fx,fy,cx,cy of intrinsics row 0).
__device__ __forceinline__ void edge_terms(const float* __restrict__ poses, const float* __restrict__ patches, int P,
                                           float fx, float fy, float cx, float cy, const TargetSrc& target,
                                           const float* __restrict__ weight, int ix, int jx, int kx, int e, EdgeTerms& T) {
  if (target.terms) {                                          // (wave-uniform) precomputed terms
    const float* t = target.terms + (int64_t)e * BA_TERMS;
    T.r[0] = t[0]; T.r[1] = t[1]; T.w[0] = t[2]; T.w[1] = t[3]; T.Jz[0] = t[4]; T.Jz[1] = t[5];
#pragma unroll
    for (int c = 0; c < 6; c++) { T.Ji[0][c] = t[6 + c]; T.Ji[1][c] = t[12 + c]; T.Jj[0][c] = t[18 + c]; T.Jj[1][c] = t[24 + c]; }
    return;
  }
  const float* pi = poses + (int64_t)ix * 7;
  const float* pj = poses + (int64_t)jx * 7;
  float ti[3] = {pi[0], pi[1], pi[2]}, qi[4] = {pi[3], pi[4], pi[5], pi[6]};
  float tj[3] = {pj[0], pj[1], pj[2]}, qj[4] = {pj[3], pj[4], pj[5], pj[6]};
  const int PPx = P * P, ctr = (P / 2) * P + (P / 2);     // centre pixel [1][1] (ba_cuda.cu:254-257)
  const float* pk = patches + (int64_t)kx * 3 * PPx;
  float Xi[4] = {(pk[ctr] - cx) / fx, (pk[PPx + ctr] - cy) / fy, 1.0f, pk[2 * PPx + ctr]};
  float tij[3], qij[4], Xj[4];
  fb_relSE3(ti, qi, tj, qj, tij, qij);
  fb_actSE3(tij, qij, Xi, Xj);
  const float X = Xj[0], Y = Xj[1], Z = Xj[2], W = Xj[3];
  // ba_cuda.cu:268 compares and divides in DOUBLE (`(Z >= 0.2) ? 1.0 / Z : 0.0`): (double)Z >= 0.2 <=> Z >= 0.2f, the quotient rounded once more to float
  const float d = (Z >= 0.2f) ? (float)(1.0 / (double)Z) : 0.0f;
  const float d2 = d * d;
  const float x1 = fx * (X / Z) + cx, y1 = fy * (Y / Z) + cy;
  float tgx = target.t[(int64_t)e * 2], tgy = target.t[(int64_t)e * 2 + 1];
  if (target.base) {
    const float* b = target.base + (int64_t)e * target.se + target.off;
    tgx = b[0] + tgx; tgy = b[target.sc] + tgy;
  }
  const float rx = tgx - x1, ry = tgy - y1;
  // ba_cuda.cu:277 `Z > 0.2` is a comparison in double: 0.2f = 0.2000000030 lies ABOVE the double 0.2, so (double)Z > 0.2 <=> Z >= 0.2f
  const bool inb = (sqrtf(rx * rx + ry * ry) < 128.0f) && (Z >= 0.2f) && (x1 > -64.0f) && (y1 > -64.0f) &&
                   (x1 < 2 * cx + 64.0f) && (y1 < 2 * cy + 64.0f);
  const float mask = inb ? 1.0f : 0.0f;
  T.r[0] = rx; T.r[1] = ry;
  T.w[0] = mask * weight[(int64_t)e * 2]; T.w[1] = mask * weight[(int64_t)e * 2 + 1];
  T.Jz[0] = fx * (tij[0] * d - tij[2] * (X * d2));
  T.Jz[1] = fy * (tij[1] * d - tij[2] * (Y * d2));
  T.Jj[0][0] = fx * W * d; T.Jj[0][1] = 0.0f; T.Jj[0][2] = fx * -X * W * d2;
  T.Jj[0][3] = fx * -X * Y * d2; T.Jj[0][4] = fx * (1 + X * X * d2); T.Jj[0][5] = fx * -Y * d;
  T.Jj[1][0] = 0.0f; T.Jj[1][1] = fy * W * d; T.Jj[1][2] = fy * -Y * W * d2;
  T.Jj[1][3] = fy * (-1 - Y * Y * d2); T.Jj[1][4] = fy * (X * Y * d2); T.Jj[1][5] = fy * X * d;
  fb_adjSE3(tij, qij, T.Jj[0], T.Ji[0]);
  fb_adjSE3(tij, qij, T.Jj[1], T.Ji[1]);
}

// ------------------------------------------------------------------------------------------------- accumulate
struct AccCtx {
  const float* poses; const float* patches; TargetSrc target; const float* weight;
  const int64_t* ii; const int64_t* jj; const int64_t* kk; const int* perm;
  float* patch_rec; float* patch_col;    // per patch: (Q, u) and its E column [6 N] (dz = Q (u - E^T dX), ba_cuda.cu:523)
  float fx, fy, cx, cy, lm;
  int P, t0, N, n6, LD;
};

// General per-patch accumulation (any number of edges, duplicated (patch, frame) pairs, edges of one patch with
// different source frames): lane-private blocks and the Schur rank-1 update go into the workgroup's LDS system
// with LDS atomics.  Correct for every input but slow (ds_add_f32 costs ~10 cycles per lane), so the kernels
// below only use it for the rare irregular patches.
// GLOBAL: S_lds / y_lds are the solver's image in GLOBAL memory, shared by every workgroup (more than BA_MAXN_LDS optimised poses:
// the per-workgroup system does not fit the LDS) — device-scope atomics, like the reference's (ba_cuda.cu:297-322); no Schur term.
template <bool GLOBAL>
__device__ __forceinline__ void sys_add(float* p, float v) {
  if (GLOBAL) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL = false>
__device__ __noinline__ void accumulate_segment_atomic(const AccCtx& K, int s, int a0, int m, float* S_lds, float* y_lds,
                                                       float* col, int lane, bool schur = true) {
  const float* __restrict__ poses = K.poses; const float* __restrict__ patches = K.patches;
  const TargetSrc target = K.target; const float* __restrict__ weight = K.weight;
  const int64_t* __restrict__ ii = K.ii; const int64_t* __restrict__ jj = K.jj; const int64_t* __restrict__ kk = K.kk;
  const int* __restrict__ perm = K.perm;
  float* patch_rec = K.patch_rec; float* patch_col = K.patch_col;
  const float fx = K.fx, fy = K.fy, cx = K.cx, cy = K.cy, lm = K.lm;
  const int P = K.P, t0 = K.t0, N = K.N, n6 = K.n6, LD = K.LD;
  for (int i = lane; i < n6; i += 64) col[i] = 0.0f;
  wave_lds_sync();
  float Csum = 0.0f, usum = 0.0f;
  unsigned fmask = 0;           // frames (relative to t0) this patch touches

  for (int base = 0; base < m; base += 64) {
    const bool act = base + lane < m;
    const int e = act ? perm[a0 + base + lane] : 0;
    EdgeTerms T;
    int ix = -1, jx = -1;
    if (act) {
      const int fi = (int)ii[e], fj = (int)jj[e];
      edge_terms(poses, patches, P, fx, fy, cx, cy, target, weight, fi, fj, (int)kk[e], e, T);
      ix = fi - t0; jx = fj - t0;
      if (ix >= N) ix = -1;
      if (jx >= N) jx = -1;
    } else {
      T.w[0] = T.w[1] = 0.0f; T.r[0] = T.r[1] = 0.0f; T.Jz[0] = T.Jz[1] = 0.0f;
#pragma unroll
      for (int c = 0; c < 6; c++) { T.Ji[0][c] = T.Ji[1][c] = T.Jj[0][c] = T.Jj[1][c] = 0.0f; }
    }
    // ---- patch-level scalars C, u (ba_cuda.cu:321-322)
    const float wz0 = T.w[0] * T.Jz[0], wz1 = T.w[1] * T.Jz[1];
    const float wr0 = T.w[0] * T.r[0], wr1 = T.w[1] * T.r[1];
    Csum += wz0 * T.Jz[0] + wz1 * T.Jz[1];
    usum += wz0 * T.r[0] + wz1 * T.r[1];
    float ej[6], ei[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      ej[c] = (jx >= 0) ? (wz0 * T.Jj[0][c] + wz1 * T.Jj[1][c]) : 0.0f;       // E_j += w Jz Jj   (:311)
      ei[c] = (ix >= 0) ? -(wz0 * T.Ji[0][c] + wz1 * T.Ji[1][c]) : 0.0f;      // E_i -= w Jz Ji   (:309)
    }
    if (N > 0) {
      if (!GLOBAL) {
        if (jx >= 0) fmask |= 1u << jx;
        if (ix >= 0) fmask |= 1u << ix;
      }
      // ---- frame-j blocks are lane-private (one edge per target frame): straight into LDS
      if (jx >= 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
          lds_add(&col[6 * jx + c], ej[c]);
          sys_add<GLOBAL>(&y_lds[6 * jx + c], wr0 * T.Jj[0][c] + wr1 * T.Jj[1][c]);                               // v_j += w r Jj (:316)
        }
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int c = 0; c <= a; c++)
            sys_add<GLOBAL>(&S_lds[(6 * jx + a) * LD + 6 * jx + c],
                    T.w[0] * T.Jj[0][a] * T.Jj[0][c] + T.w[1] * T.Jj[1][a] * T.Jj[1][c]);                 // B_jj (:299)
        if (ix >= 0) {
          // B_ij = -w Ji Jj^T and B_ji = its transpose (:300-303): keep the one in the lower triangle
          // (both when i == j: they land on the same diagonal block).
#pragma unroll
          for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
              const float vij = -(T.w[0] * T.Ji[0][a] * T.Jj[0][c] + T.w[1] * T.Ji[1][a] * T.Jj[1][c]);  // block (i,j)[a][c]
              if (ix > jx) sys_add<GLOBAL>(&S_lds[(6 * ix + a) * LD + 6 * jx + c], vij);
              else if (ix < jx) sys_add<GLOBAL>(&S_lds[(6 * jx + c) * LD + 6 * ix + a], vij);
              else { sys_add<GLOBAL>(&S_lds[(6 * ix + a) * LD + 6 * ix + c], vij); sys_add<GLOBAL>(&S_lds[(6 * ix + c) * LD + 6 * ix + a], vij); }
            }
        }
      }
      // ---- frame-i blocks: in DEVO graphs all edges of a patch share the source frame -> reduce the
      //      6x6 / 6x1 blocks across the wavefront with shuffles and add once; otherwise lane-private.
      const unsigned long long bi = __ballot(ix >= 0);
      if (bi) {
        const int ix0 = __shfl(ix, __ffsll((long long)bi) - 1);
        const bool uniform = (__ballot(ix >= 0 && ix != ix0) == 0ULL);
        if (uniform) {
#pragma unroll
          for (int c = 0; c < 6; c++) {
            const float vc = wave_sum(ei[c]);
            const float vv = wave_sum((ix >= 0) ? -(wr0 * T.Ji[0][c] + wr1 * T.Ji[1][c]) : 0.0f);        // v_i -= w r Ji (:314)
            if (lane == 0) { lds_add(&col[6 * ix0 + c], vc); sys_add<GLOBAL>(&y_lds[6 * ix0 + c], vv); }
          }
#pragma unroll
          for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c <= a; c++) {
              float v = (ix >= 0) ? (T.w[0] * T.Ji[0][a] * T.Ji[0][c] + T.w[1] * T.Ji[1][a] * T.Ji[1][c]) : 0.0f;   // B_ii (:297)
              v = wave_sum(v);
              if (lane == 0) sys_add<GLOBAL>(&S_lds[(6 * ix0 + a) * LD + 6 * ix0 + c], v);
            }
        } else if (ix >= 0) {
#pragma unroll
          for (int c = 0; c < 6; c++) {
            lds_add(&col[6 * ix + c], ei[c]);
            sys_add<GLOBAL>(&y_lds[6 * ix + c], -(wr0 * T.Ji[0][c] + wr1 * T.Ji[1][c]));
          }
#pragma unroll
          for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c <= a; c++)
              sys_add<GLOBAL>(&S_lds[(6 * ix + a) * LD + 6 * ix + c],
                      T.w[0] * T.Ji[0][a] * T.Ji[0][c] + T.w[1] * T.Ji[1][a] * T.Ji[1][c]);
        }
      }
    }
  }
  // ---- finish the patch: C, u, Q
  Csum = wave_sum(Csum);
  usum = wave_sum(usum);
  const float Q = 1.0f / (Csum + lm);                                   // ba_cuda.cu:492
  fmask = wave_or(fmask);
  if (lane == 0) { patch_rec[(int64_t)s * 2] = Q; patch_rec[(int64_t)s * 2 + 1] = usum; }
  if (N > 0) {
    wave_lds_sync();                                                    // the patch's E column is complete in LDS
    // ---- Schur complement, patch by patch:  S -= Q e e^T (lower triangle),  y -= Q u e   (:511-512)
    // The column is pulled into registers once (lane l holds rows l, l+64, l+128); column entries are then
    // broadcast with v_readlane, so the loop issues LDS atomics only — no LDS read sits between them.
    if (GLOBAL) {                                                       // any N: the column for k_ba_schur and the retraction
      for (int i = lane; i < n6; i += 64) patch_col[(int64_t)s * n6 + i] = col[i];
      wave_lds_sync();
      return;
    }
    float cr[3];
#pragma unroll
    for (int g = 0; g < 3; g++) cr[g] = (lane + 64 * g < n6) ? col[lane + 64 * g] : 0.0f;
#pragma unroll
    for (int g = 0; g < 3; g++) if (lane + 64 * g < n6) patch_col[(int64_t)s * n6 + lane + 64 * g] = cr[g];   // for the retraction
#pragma unroll
    for (int g = 0; g < 3 && schur; g++) {                              // (!schur: k_ba_schur subtracts E Q E^T afterwards)
      if (64 * g >= n6) break;                                          // uniform
      const int r = lane + 64 * g;
      const float qer = -Q * cr[g];
      const bool live = (r < n6) && (cr[g] != 0.0f);
      if (live) sys_add<GLOBAL>(&y_lds[r], qer * usum);
      for (unsigned mm = fmask; mm; mm &= mm - 1) {                     // uniform trip count
        const int fb = __ffs((int)mm) - 1;
        if (6 * fb > 64 * g + 63) break;                                // uniform: no row of this group reaches it
#pragma unroll
        for (int c = 0; c < 6; c++) {
          const int cc = 6 * fb + c;
          const float ec = readlane_f(cc < 64 ? cr[0] : (cc < 128 ? cr[1] : cr[2]), cc & 63);
          if (live && cc <= r) sys_add<GLOBAL>(&S_lds[r * LD + cc], qer * ec);
        }
      }
    }
    wave_lds_sync();
  }
}

// Partial systems are stored compactly: lower block triangle, block (fr, fc <= fr) at (fr (fr+1)/2 + fc) * 36 as a
// full 6x6 [a][b] (of a diagonal block only a >= b is meaningful), then y [n6].
__device__ __forceinline__ int tri_blocks(int N) { return N * (N + 1) / 2; }
__device__ __forceinline__ void block_of(int blk, int& fr, int& fc) {   // inverse of blk = fr (fr+1)/2 + fc
  fr = (int)((sqrtf(8.0f * (float)blk + 1.0f) - 1.0f) * 0.5f);
  while (fr * (fr + 1) / 2 > blk) fr--;
  while ((fr + 1) * (fr + 2) / 2 <= blk) fr++;
  fc = blk - fr * (fr + 1) / 2;
}

// Generic accumulate kernel (any N <= 32): every patch through the atomic path.
// LDS (dynamic): S_lds [n6 * LD] (lower triangle used), y_lds [n6], per-wave column buffers [ACC_WAVES][n6].
template <bool GLOBAL>
__global__ __launch_bounds__(ACC_THREADS) void k_ba_accumulate_t(
    const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ intr,
    const TargetSrc target, const float* __restrict__ weight, const float* __restrict__ lmbda,
    const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, const int64_t* __restrict__ kk,
    const int* __restrict__ perm, const int* __restrict__ seg_start, BaMeta* __restrict__ meta, int P, int t0,
    int N, float* __restrict__ partials, float* __restrict__ patch_rec, float* __restrict__ patch_col, int iter, int sig, int max_seg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n6 = 6 * N, LD = n6 + 1;
  // GLOBAL: `partials` is the solver's image itself ((n6 + 1) x LD, zeroed by the launcher; row n6 = the right-hand side), the LDS only
  // holds the waves' E columns
  float* S_lds = GLOBAL ? partials : smem;
  float* y_lds = S_lds + n6 * LD;
  float* col_all = GLOBAL ? smem : y_lds + n6;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* col = col_all + wave * n6;
  if (!GLOBAL) for (int i = tid; i < n6 * LD + n6; i += ACC_THREADS) smem[i] = 0.0f;
  __syncthreads();
  AccCtx K{poses, patches, target, weight, ii, jj, kk, perm, patch_rec, patch_col, intr[0], intr[1], intr[2], intr[3], lmbda[0],
           P, t0, N, n6, LD};
  // a workspace that was not prepared for this (E, N) is not touched: the call fails (status -1) instead of walking
  // garbage tables; a prepared graph may be solved many times (the sticky failure flag is reset here)
  const bool prepared = meta->sig == sig;
  const int n_seg = prepared ? min(meta->n_seg, max_seg) : 0;
  const bool defer = (iter >> 16) != 0;                        // the launcher's flag: the Schur term is left to k_ba_schur
  iter &= 0xffff;
  if (iter == 0 && blockIdx.x == 0 && tid == 0) meta->fail = prepared ? 0 : -1;
  for (int s = blockIdx.x * ACC_WAVES + wave; s < n_seg; s += gridDim.x * ACC_WAVES) {
    const int a0 = seg_start[s], m = seg_start[s + 1] - a0;
    accumulate_segment_atomic<GLOBAL>(K, s, a0, m, S_lds, y_lds, col, lane, !defer && !GLOBAL);
  }
  __syncthreads();
  if (N > 0 && !GLOBAL) {
    const int nt = tri_blocks(N) * 36;
    float* out = partials + (int64_t)blockIdx.x * (nt + n6);
    for (int i = tid; i < nt; i += ACC_THREADS) {
      int fr, fc;
      block_of(i / 36, fr, fc);
      const int ab = i % 36;
      out[i] = S_lds[(6 * fr + ab / 6) * LD + 6 * fc + ab % 6];
    }
    for (int i = tid; i < n6; i += ACC_THREADS) out[nt + i] = y_lds[i];
  }
}

// Register-path accumulate kernel for N <= NMAX optimised poses (the DEVO sizes: 7..14).
// Each wave keeps its OWN copy of the lower block-triangle of S: lane (a,b) = (lane/6, lane%6) < 36 holds entry [a][b]
// of every 6x6 block.  A regular patch (<= 64 edges, one source frame, distinct target frames) is folded in with
// wave-uniform control flow and plain LDS reads of a per-wave scratch that the patch's edge lanes filled: no atomics,
// fixed summation order.  Irregular patches take the atomic path into the workgroup's LDS system.  At the end the
// workgroup adds the wave copies and that system.
constexpr int SCR_ROWS = 28;     // per-edge scratch rows: Jj_x[6] Jj_y[6] Ji_x[6] Ji_y[6] w_x w_y (w r)_x (w r)_y
constexpr int SCR_LD = 48;       // slots per scratch row (a regular patch has <= that many edges)
// A wave keeps its copy of the block triangle in its own LDS slab (LDSFOLD; the layout of the compact partial).  The first patch of a wave
// STORES its blocks (no zero-fill, no read), later ones read-modify-write.  ~150 registers: two waves per SIMD, WAVES = 8 / 6 / 4 for
// N <= 11 / 14 / 16 by the LDS the slabs need — at cfg2 every wave has ONE patch.  Same sums in the same order per wave; the workgroup
// adds the slabs in wave order: deterministic.  (The register fold of rounds 2-5 — 105 accumulators per lane at N = 14, one wave per SIMD,
// instruction-issue bound: profiles/README.md, r02c — is in git history.)
template <int NMAX, int WAVES, bool LDSFOLD>
__global__ __launch_bounds__(WAVES * 64) void k_ba_accumulate_reg(
    const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ intr,
    const TargetSrc target, const float* __restrict__ weight, const float* __restrict__ lmbda,
    const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, const int64_t* __restrict__ kk,
    const int* __restrict__ perm, const int* __restrict__ seg_start, BaMeta* __restrict__ meta, int P, int t0,
    int N, float* __restrict__ partials, float* __restrict__ patch_rec, float* __restrict__ patch_col, int iter, int sig, int max_seg) {
  static_assert(LDSFOLD, "the block triangle is folded in LDS");
  constexpr int REG_WAVES = WAVES, REG_THREADS = WAVES * 64, SLD = SCR_LD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n6 = 6 * N, LD = n6 + 1;
  float* S_lds = smem;
  float* y_lds = S_lds + n6 * LD;
  float* col_all = y_lds + n6;
  float* scr_all = col_all + REG_WAVES * n6;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* col = col_all + wave * n6;
  float* scr = scr_all + wave * (SCR_ROWS * SLD);
  __shared__ int s_used_atomic;                                 // did any wave of this workgroup take the atomic path?
  {
    const int nz = n6 * LD + n6, nz4 = nz >> 2;                 // smem is 16-byte aligned
    float4* z4 = reinterpret_cast<float4*>(smem);
    for (int i = tid; i < nz4; i += REG_THREADS) z4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = (nz4 << 2) + tid; i < nz; i += REG_THREADS) smem[i] = 0.0f;
    if (tid == 0) s_used_atomic = 0;
  }
  __syncthreads();
  AccCtx K{poses, patches, target, weight, ii, jj, kk, perm, patch_rec, patch_col, intr[0], intr[1], intr[2], intr[3], lmbda[0],
           P, t0, N, n6, LD};

  const int pa = (lane < 36) ? lane / 6 : 0, pb = (lane < 36) ? lane % 6 : 0;    // this lane's position inside a 6x6 block
  const int nt = tri_blocks(N) * 36;
  float* tri_all = scr_all + REG_WAVES * (SCR_ROWS * SLD);     // [REG_WAVES][nt + n6]
  float* tri = tri_all + wave * (nt + n6);                     // this wave's compact copy
  bool fresh = true;                                           // nothing in the slab yet — the first patch stores

  // a workspace that was not prepared for this (E, N) is not touched: the call fails (status -1) instead of walking
  // garbage tables; a prepared graph may be solved many times (the sticky failure flag is reset here)
  const bool prepared = meta->sig == sig;
  const int n_seg = prepared ? min(meta->n_seg, max_seg) : 0;
  const bool ident = meta->pad != 0;                           // the edge list was grouped by patch already: perm is the identity (one
                                                               // dependent round trip less in front of the edge terms)
  if (iter == 0 && blockIdx.x == 0 && tid == 0) meta->fail = prepared ? 0 : -1;
  for (int s = blockIdx.x * REG_WAVES + wave; s < n_seg; s += gridDim.x * REG_WAVES) {
    const int a0 = seg_start[s], m = seg_start[s + 1] - a0;
    if (m > 64) { if (lane == 0) s_used_atomic = 1; accumulate_segment_atomic(K, s, a0, m, S_lds, y_lds, col, lane); continue; }
    const bool act = lane < m;
    const int e = act ? (ident ? a0 + lane : perm[a0 + lane]) : 0;
    EdgeTerms T;
    int ix = -1, jx = -1;
    if (act) {
      const int fi = (int)ii[e], fj = (int)jj[e];
      edge_terms(poses, patches, P, K.fx, K.fy, K.cx, K.cy, target, weight, fi, fj, (int)kk[e], e, T);
      ix = fi - t0; jx = fj - t0;
      if (ix >= N) ix = -1;
      if (jx >= N) jx = -1;
    } else {
      T.w[0] = T.w[1] = 0.0f; T.r[0] = T.r[1] = 0.0f; T.Jz[0] = T.Jz[1] = 0.0f;
#pragma unroll
      for (int c = 0; c < 6; c++) { T.Ji[0][c] = T.Ji[1][c] = T.Jj[0][c] = T.Jj[1][c] = 0.0f; }
    }
    // ---- regular?  one source frame, distinct target frames (frame -> lane table built through the column buffer)
    const unsigned long long bi = __ballot(ix >= 0);
    const int src = bi ? __shfl(ix, __ffsll((long long)bi) - 1) : -1;
    const bool mixed = __ballot(ix >= 0 && ix != src) != 0ULL;
    int* ftab = reinterpret_cast<int*>(col);                    // borrowed before the column is built
    if (lane < N) ftab[lane] = -1;
    wave_lds_sync();
    if (jx >= 0) ftab[jx] = lane;
    wave_lds_sync();
    const bool dup = (jx >= 0) && (ftab[jx] != lane);
    wave_lds_sync();
    // slot of every edge in the wave's scratch: its target frame if that is optimised (distinct per edge), else a slot
    // behind the N frame slots (fixed target frames only matter for the source-frame sums)
    const unsigned long long fixm = __ballot(act && jx < 0);
    const int nslot = N + __popcll(fixm);
    if (mixed || __ballot(dup) != 0ULL || nslot > SLD) {
      if (lane == 0) s_used_atomic = 1;
      accumulate_segment_atomic(K, s, a0, m, S_lds, y_lds, col, lane);
      continue;
    }
    const int slot = (jx >= 0) ? jx : N + __popcll(fixm & ((1ULL << lane) - 1ULL));

    // ---- per-edge quantities into the wave's scratch [row][slot]; the patch's E column into `col`
    for (int i = lane; i < n6; i += 64) col[i] = 0.0f;
#pragma unroll
    for (int r = 0; r < SCR_ROWS; r++) if (lane < SLD) scr[r * SLD + lane] = 0.0f;          // frames without an edge read zeros
    const float wz0 = T.w[0] * T.Jz[0], wz1 = T.w[1] * T.Jz[1];
    const float wr0 = T.w[0] * T.r[0], wr1 = T.w[1] * T.r[1];
    float Csum = wz0 * T.Jz[0] + wz1 * T.Jz[1];
    float usum = wz0 * T.r[0] + wz1 * T.r[1];
    float ej[6], ei[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      ej[c] = (jx >= 0) ? (wz0 * T.Jj[0][c] + wz1 * T.Jj[1][c]) : 0.0f;       // E_j += w Jz Jj   (ba_cuda.cu:311)
      ei[c] = (ix >= 0) ? -(wz0 * T.Ji[0][c] + wz1 * T.Ji[1][c]) : 0.0f;      // E_i -= w Jz Ji   (:309)
    }
    wave_lds_sync();
    if (act) {
#pragma unroll
      for (int c = 0; c < 6; c++) {
        scr[c * SLD + slot] = T.Jj[0][c];
        scr[(6 + c) * SLD + slot] = T.Jj[1][c];
        scr[(12 + c) * SLD + slot] = (ix >= 0) ? T.Ji[0][c] : 0.0f;
        scr[(18 + c) * SLD + slot] = (ix >= 0) ? T.Ji[1][c] : 0.0f;
      }
      scr[24 * SLD + slot] = T.w[0]; scr[25 * SLD + slot] = T.w[1];
      scr[26 * SLD + slot] = wr0;    scr[27 * SLD + slot] = wr1;
      if (jx >= 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) col[6 * jx + c] = ej[c];    // distinct target frames: plain stores
      }
    }
    Csum = wave_sum(Csum);
    usum = wave_sum(usum);
#pragma unroll
    for (int c = 0; c < 6; c++) ei[c] = wave_sum(ei[c]);
    wave_lds_sync();
    if (src >= 0 && lane == 0) {
#pragma unroll
      for (int c = 0; c < 6; c++) col[6 * src + c] += ei[c];
    }
    const float Q = 1.0f / (Csum + K.lm);                       // ba_cuda.cu:492
    if (lane == 0) { patch_rec[(int64_t)s * 2] = Q; patch_rec[(int64_t)s * 2 + 1] = usum; }
    wave_lds_sync();
    if (N == 0) continue;
    for (int i = lane; i < n6; i += 64) patch_col[(int64_t)s * n6 + i] = col[i];  // the patch's E column, for the retraction

    // ---- fold the patch into the wave's block triangle.  Everything a lane needs is pulled into registers
    //      with wide LDS reads first (frame slots 0..NSL-1: element [pa] / [pb] of every Jacobian row), then the 6x6 block
    //      entries are pure register arithmetic with no branches; slots without an edge hold zeros, block rows >= N are
    //      computed but never flushed.
    {
      constexpr int NSL = ((NMAX + 3) / 4) * 4;
      auto ld4 = [&](int row, int g4, float (&o)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(scr + row * SLD + 4 * g4);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
      };
      {
        // pass 1: Schur rank-1 term and the target-frame diagonal blocks
        float cr[NSL], cc[NSL], Dg[NSL];
#pragma unroll
        for (int g4 = 0; g4 < NSL / 4; g4++) {
          float jxa[4], jxb[4], jya[4], jyb[4], w0[4], w1[4];
          ld4(pa, g4, jxa); ld4(pb, g4, jxb); ld4(6 + pa, g4, jya); ld4(6 + pb, g4, jyb); ld4(24, g4, w0); ld4(25, g4, w1);
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int f = 4 * g4 + u;
            Dg[f] = w0[u] * jxa[u] * jxb[u] + w1[u] * jya[u] * jyb[u];            // B_jj += w Jj Jj^T      (:299)
            cr[f] = col[6 * f + pa];
            cc[f] = col[6 * f + pb];
          }
        }
        auto block_value = [&](int fr, int fc) {
          float v = -Q * cr[fr] * cc[fc];                        // Schur: S -= Q e e^T  (:511)
          if (fr == fc) v += Dg[fr];
          return v;
        };
        // the slab has tri_blocks(N) blocks (fr < N: wave-uniform).  First patch of the wave: stores only; later ones: a block
        // row's old values are fetched together (one LDS latency per row, not per block), then added and stored
        float* tp = tri + lane;
        if (lane < 36) {
          if (fresh) {
            int blk = 0;
#pragma unroll
            for (int fr = 0; fr < NMAX; fr++) {
#pragma unroll
              for (int fc = 0; fc <= fr; fc++, blk++) if (fr < N) tp[blk * 36] = block_value(fr, fc);
            }
          } else {
#pragma unroll
            for (int fr = 0; fr < NMAX; fr++) {
              if (fr < N) {
                float old[NMAX];
#pragma unroll
                for (int fc = 0; fc <= fr; fc++) old[fc] = tp[(fr * (fr + 1) / 2 + fc) * 36];
#pragma unroll
                for (int fc = 0; fc <= fr; fc++) tp[(fr * (fr + 1) / 2 + fc) * 36] = old[fc] + block_value(fr, fc);
              }
            }
          }
        }
      }
      if (src >= 0) {
        // pass 2 (source frame optimised): row and column `src` get the (i,j) / (j,i) blocks, the diagonal gets B_ii;
        // a self edge (target == source) puts B_ij + B_ji on the diagonal as well
        float Rr[NSL], Cq[NSL];
        float bii = 0.0f;
#pragma unroll
        for (int g4 = 0; g4 < NSL / 4; g4++) {
          float jxa[4], jxb[4], jya[4], jyb[4], ixa[4], ixb[4], iya[4], iyb[4], w0[4], w1[4];
          ld4(pa, g4, jxa); ld4(pb, g4, jxb); ld4(6 + pa, g4, jya); ld4(6 + pb, g4, jyb);
          ld4(12 + pa, g4, ixa); ld4(12 + pb, g4, ixb); ld4(18 + pa, g4, iya); ld4(18 + pb, g4, iyb);
          ld4(24, g4, w0); ld4(25, g4, w1);
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int f = 4 * g4 + u;
            Rr[f] = w0[u] * jxa[u] * ixb[u] + w1[u] * jya[u] * iyb[u];            // block (j,i): w Jj Ji^T  (:303)
            Cq[f] = w0[u] * ixa[u] * jxb[u] + w1[u] * iya[u] * jyb[u];            // block (i,j): w Ji Jj^T  (:302)
            bii += w0[u] * ixa[u] * ixb[u] + w1[u] * iya[u] * iyb[u];             // B_ii += w Ji Ji^T      (:297)
          }
        }
        for (int q = NSL; q < nslot; q++)                        // more fixed-target edges than spare slots (rare)
          bii += scr[24 * SLD + q] * scr[(12 + pa) * SLD + q] * scr[(12 + pb) * SLD + q] +
                 scr[25 * SLD + q] * scr[(18 + pa) * SLD + q] * scr[(18 + pb) * SLD + q];
        // the N blocks of row / column `src` of the slab, after pass 1's stores to the same addresses (LDS is in order)
#pragma unroll
        for (int f = 0; f < NMAX; f++) {
          if (f < N && lane < 36) {
            const int blk = (f < src) ? src * (src + 1) / 2 + f : f * (f + 1) / 2 + src;          // wave-uniform
            const float d = (f < src) ? -Cq[f] : (f > src) ? -Rr[f] : bii - (Rr[f] + Cq[f]);
            tri[blk * 36 + lane] += d;
          }
        }
      }
    }
    // ---- right-hand side rows lane, lane+64:  y = v - Q u e   (v_i -= w r Ji, v_j += w r Jj; :314-316, :512)
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int r = lane + 64 * g;
      if (r < n6) {
        const int f = r / 6, a = r - 6 * f;
        float v = -Q * usum * col[r];
        v += scr[26 * SLD + f] * scr[a * SLD + f] + scr[27 * SLD + f] * scr[(6 + a) * SLD + f];
        if (f == src) {                                          // v_i -= sum over the patch's edges of w r Ji: wide reads, no latency chain
          constexpr int NSL = ((NMAX + 3) / 4) * 4;
          float acc = 0.0f;
#pragma unroll
          for (int g4 = 0; g4 < NSL / 4; g4++) {
            const float4 p0 = *reinterpret_cast<const float4*>(scr + 26 * SLD + 4 * g4), p1 = *reinterpret_cast<const float4*>(scr + 27 * SLD + 4 * g4);
            const float4 j0 = *reinterpret_cast<const float4*>(scr + (12 + a) * SLD + 4 * g4), j1 = *reinterpret_cast<const float4*>(scr + (18 + a) * SLD + 4 * g4);
            acc += p0.x * j0.x + p1.x * j1.x;
            acc += p0.y * j0.y + p1.y * j1.y;
            acc += p0.z * j0.z + p1.z * j1.z;
            acc += p0.w * j0.w + p1.w * j1.w;
          }
          for (int q = NSL; q < nslot; q++) acc += scr[26 * SLD + q] * scr[(12 + a) * SLD + q] + scr[27 * SLD + q] * scr[(18 + a) * SLD + q];
          v -= acc;
        }
        float* yp = tri + nt + r;
        if (fresh) *yp = v;                                      // (wave-uniform)
        else *yp += v;
      }
    }
    fresh = false;
    wave_lds_sync();
  }

  // ---- the slab is complete (a wave without a regular patch clears it).  Then the workgroup adds the slabs and the atomic-path
  //      system in a fixed order and writes the compact partial
  if (N > 0 && fresh) for (int i = lane; i < nt + n6; i += 64) tri[i] = 0.0f;
  __syncthreads();
  if (N > 0) {
    float* out = partials + (int64_t)blockIdx.x * (nt + n6);
    const bool with_atomic = s_used_atomic != 0;               // workgroup-uniform; usually false: no index arithmetic then
    if (!with_atomic && ((nt + n6) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(tri_all) & 15) == 0) {
      // the usual case, four entries per lane and instruction: the same additions in the same order (wave 0's slab first)
      const int n4 = (nt + n6) >> 2;
      const float4* t4 = reinterpret_cast<const float4*>(tri_all);
      float4* o4 = reinterpret_cast<float4*>(out);
      for (int i = tid; i < n4; i += REG_THREADS) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int w = 0; w < REG_WAVES; w++) { const float4 a = t4[w * n4 + i]; v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
        o4[i] = v;
      }
    } else
    for (int i = tid; i < nt + n6; i += REG_THREADS) {
      float v = 0.0f;
      if (with_atomic) {
        if (i < nt) {
          int fr, fc;
          block_of(i / 36, fr, fc);
          const int ab = i % 36;
          v = S_lds[(6 * fr + ab / 6) * LD + 6 * fc + ab % 6];
        } else v = y_lds[i - nt];
      }
#pragma unroll
      for (int w = 0; w < REG_WAVES; w++) v += tri_all[w * (nt + n6) + i];
      out[i] = v;
    }
  }
}

// S = sum of the compact partials, mirrored; S_dd <- S_dd*(1+1e-4)+1 (ba_cuda.cu:517-518); y = sum.
// 512-thread workgroups: wave g sums partials [g*n_part/8, (g+1)*n_part/8) for 64 consecutive outputs (32 loads in
// flight), the eight wave results are combined through LDS in a fixed order.
// damping value that tells k_ba_reduce to leave the diagonal alone (the deferred Schur path damps afterwards): any other value,
// negative ones included, is applied as given
constexpr float BA_EP_DEFERRED = -3.402823466e38f;
__global__ __launch_bounds__(512) void k_ba_reduce(const float* __restrict__ partials, int n_part, int N, float* __restrict__ S,
                                                   float* __restrict__ y, float ep) {
  // One lane per entry of the COMPACT partial (lower block triangle + right-hand side): consecutive lanes read consecutive
  // addresses of every partial, 8 waves share the partials of 64 entries, the symmetric entry is written by the same lane
  // (the full-matrix form read every off-diagonal entry twice, 6 floats at a time).
  __shared__ float s_sum[8][64];
  const int n6 = 6 * N, nt = tri_blocks(N) * 36, stride = nt + n6;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int o = blockIdx.x * 64 + lane;
  const int per = (n_part + 7) / 8;
  const int p0 = g * per, p1 = min(n_part, p0 + per);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (o < stride) {
    const float* base = partials + o;
    // 32 loads in flight per lane (one round trip for the usual 256 partials), added in the order p0, p0 + 1, ... into the
    // eight accumulators exactly as a plain loop would
    for (int q0 = p0; q0 < p1; q0 += 32) {
      float v[32];
#pragma unroll
      for (int k = 0; k < 32; k++) v[k] = (q0 + k < p1) ? base[(int64_t)(q0 + k) * stride] : 0.0f;
#pragma unroll
      for (int k = 0; k < 32; k++) if (q0 + k < p1) acc[k & 7] += v[k];
    }
  }
  s_sum[g][lane] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (g == 0 && o < stride) {
    float sum = ((s_sum[0][lane] + s_sum[1][lane]) + (s_sum[2][lane] + s_sum[3][lane])) +
                ((s_sum[4][lane] + s_sum[5][lane]) + (s_sum[6][lane] + s_sum[7][lane]));
    // written as the solver's working matrix: (n6+1) rows of pitch n6+1, the right-hand side is row n6
    if (o < nt) {
      int fr, fc;
      block_of(o / 36, fr, fc);
      const int ab = o % 36, r = 6 * fr + ab / 6, c = 6 * fc + ab % 6;
      if (fr == fc && ab / 6 < ab % 6) return;                  // upper half of a diagonal block: its mirror writes it
      if (r == c && ep != BA_EP_DEFERRED) sum = sum + (1e-4f * sum + ep);   // ba_cuda.cu:518 (ep = 1); devo/ba.py:73 (ep = 10 in training); BA_EP_DEFERRED: k_ba_damp does it
      S[r * (n6 + 1) + c] = sum;
      if (r != c) S[c * (n6 + 1) + r] = sum;
    } else S[n6 * (n6 + 1) + (o - nt)] = sum;
  }
}

constexpr auto k_ba_accumulate = k_ba_accumulate_t<false>;

// ------------------------------------------------------------------------------------------------- deferred Schur term
// S_aug -= E^ diag(Q) E^^T for the general accumulate kernel at N > 16 (ba_cuda.cu:511-512 as ONE product instead of 17 k LDS
// atomics per patch: on gfx950 a 64-lane ds_add_f32 occupies the LDS for ~60 cycles, and at BASELINE's stress size the per-patch
// form spent 0.79 ms per iteration in them).  E^_p = [e_p ; u_p] is patch p's column of E with its right-hand-side scalar
// appended (patch_col / patch_rec), S_aug the solver's working image (rows x LD, row n6 = y^T; lower triangle).
// Workgroup = one 32 x 32 tile of the lower triangle x one chunk of 128 patches; 2 x 2 outputs per thread; float atomics into S
// (1 344 workgroups x 1 024 outputs at the stress size) — or, when the launcher has scratch for it (the partial systems' area is free
// by then), one partial tile per workgroup that k_ba_damp adds in a fixed order: bit-reproducible results.
__global__ __launch_bounds__(256) void k_ba_schur(const float* __restrict__ patch_rec, const float* __restrict__ patch_col,
                                                  const BaMeta* __restrict__ meta, int N, int max_seg, float* __restrict__ S,
                                                  float* __restrict__ part) {
  __shared__ float sa[SCH_K][SCH_T + 1], sb[SCH_K][SCH_T + 1];      // rows block (scaled by -Q), columns block
  const int n6 = 6 * N, LD = n6 + 1;
  int tr = 0, tc = 0;
  {                                                                   // blockIdx.x -> lower-triangle tile (tr >= tc)
    int t = blockIdx.x;
    while (t > tr) { t -= tr + 1; tr++; }
    tc = t;
  }
  const int n_seg = min(meta->n_seg, max_seg);
  const int k0 = blockIdx.y * SCH_K;
  if (k0 >= n_seg || meta->fail) return;
  const int tid = threadIdx.x;
  for (int i = tid; i < SCH_K * SCH_T; i += 256) {
    const int k = i / SCH_T, j = i - k * SCH_T;
    const int p = k0 + k;
    float a = 0.0f, b = 0.0f;
    if (p < n_seg) {
      const float q = patch_rec[(int64_t)p * 2], u = patch_rec[(int64_t)p * 2 + 1];
      const int ra = tr * SCH_T + j, cb = tc * SCH_T + j;
      const float ea = ra < n6 ? patch_col[(int64_t)p * n6 + ra] : (ra == n6 ? u : 0.0f);
      const float eb = cb < n6 ? patch_col[(int64_t)p * n6 + cb] : 0.0f;       // (column n6 of the image is not used)
      a = -q * ea; b = eb;
    }
    sa[k][j] = a; sb[k][j] = b;
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;                             // outputs (2 ty + {0,1}, 2 tx + {0,1})
  float v00 = 0.0f, v01 = 0.0f, v10 = 0.0f, v11 = 0.0f;
#pragma unroll 8
  for (int k = 0; k < SCH_K; k++) {
    const float a0 = sa[k][2 * ty], a1 = sa[k][2 * ty + 1], b0 = sb[k][2 * tx], b1 = sb[k][2 * tx + 1];
    v00 = fmaf(a0, b0, v00); v01 = fmaf(a0, b1, v01); v10 = fmaf(a1, b0, v10); v11 = fmaf(a1, b1, v11);
  }
  if (part) {                                                         // deterministic: the tile's partial, summed in chunk order by k_ba_damp
    float* o = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (SCH_T * SCH_T);
    o[(2 * ty) * SCH_T + 2 * tx] = v00; o[(2 * ty) * SCH_T + 2 * tx + 1] = v01;
    o[(2 * ty + 1) * SCH_T + 2 * tx] = v10; o[(2 * ty + 1) * SCH_T + 2 * tx + 1] = v11;
    return;
  }
  const int r0 = tr * SCH_T + 2 * ty, c0 = tc * SCH_T + 2 * tx;
  auto put = [&](int r, int c, float v) { if (r <= n6 && c < n6 && c <= r && v != 0.0f) atomicAdd(&S[(int64_t)r * LD + c], v); };
  put(r0, c0, v00); put(r0, c0 + 1, v01); put(r0 + 1, c0, v10); put(r0 + 1, c0 + 1, v11);
}

// S_dd <- S_dd * (1 + 1e-4) + ep after the deferred Schur term (what k_ba_reduce does when nothing is deferred), and the mirror of
// the lower triangle that k_ba_reduce wrote before the Schur term went in
__global__ void k_ba_damp(float* __restrict__ S, int N, float ep, const float* __restrict__ part, int nchunk_grid,
                          const BaMeta* __restrict__ meta, int max_seg) {
  const int n6 = 6 * N, LD = n6 + 1;
  const int nchunk = part ? (min(meta->n_seg, max_seg) + SCH_K - 1) / SCH_K : 0;      // chunks that hold patches (the others were not written)
  const bool dead = meta->fail != 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (n6 + 1) * n6; i += gridDim.x * blockDim.x) {
    const int r = i / n6, c = i - r * n6;                         // r <= n6 (row n6 = the right-hand side), c < n6
    if (c > r) continue;
    float v = S[(int64_t)r * LD + c];
    if (part && !dead) {
      const int tr = r / SCH_T, tc = c / SCH_T;
      const float* o = part + ((int64_t)(tr * (tr + 1) / 2 + tc) * nchunk_grid) * (SCH_T * SCH_T) + (r - tr * SCH_T) * SCH_T + (c - tc * SCH_T);
      float acc = 0.0f;
      for (int k = 0; k < nchunk; k++) acc += o[(int64_t)k * (SCH_T * SCH_T)];
      v += acc;
    }
    if (r == c) v = v + (1e-4f * v + ep);
    S[(int64_t)r * LD + c] = v;
    if (r != c && r < n6) S[(int64_t)c * LD + r] = v;
  }
}

// ------------------------------------------------------------------------------------------------- solve
// One workgroup.  A (n6+1) x LD lower-triangular working matrix lives in LDS; row n6 holds y^T, so after the
// factorisation row n6 is z = L^{-1} y.  Blocked by the 6x6 pose blocks; the diagonal block of the next step is factored by a
// look-ahead wave while the others run the trailing update (round 1's form, in which every panel thread factored it itself, is in git
// history).
constexpr int SOLVE_THREADS = 1024;

__device__ __forceinline__ bool chol6(float L[6][6], float inv[6]) {   // in-register lower Cholesky of a 6x6 block
  bool ok = true;                                                      // inv[c] = 1 / L[c][c]
#pragma unroll
  for (int c = 0; c < 6; c++) {
    float d = L[c][c];
#pragma unroll
    for (int k = 0; k < c; k++) d -= L[c][k] * L[c][k];
    if (!(d > 0.0f)) ok = false;
    inv[c] = __frsqrt_rn(d);                     // one v_rsq_f32 on the serial path instead of sqrt + divide
    L[c][c] = d * inv[c];
#pragma unroll
    for (int a = c + 1; a < 6; a++) {
      float v = L[a][c];
#pragma unroll
      for (int k = 0; k < c; k++) v -= L[a][k] * L[c][k];
      L[a][c] = v * inv[c];
    }
  }
  return ok;
}

// Row stride of the solver's LDS image (floats): even (8-byte operand pairs), >= n6 + 1 (the right-hand side is an extra row, the
// last column is spare), and = 36 (mod 64) where the LDS allows it: the matrix-core trailing update then reads its operands (16 rows x 4
// columns per instruction) and its 16 x 16 result tiles (4 rows x 16 columns per instruction) without a bank conflict.
__host__ __device__ inline int solve_ld(int n6) {
  for (int ld = 36; ld <= 164; ld += 64)
    if (ld >= n6 + 1) return ld;
  return n6 + 2;
}

// GLOBAL (more than BA_MAXN_LDS optimised poses: the image does not fit the LDS): the same algorithm IN PLACE on the global image
// (row stride n6 + 1; one workgroup = one CU = one L1, workgroup barriers order its global accesses); only the factored diagonal
// blocks, their inverses and the solution stay in LDS.  Slower by the latency ratio, correct for any N the LDS tables hold.
template <bool GLOBAL>
__global__ __launch_bounds__(SOLVE_THREADS) void k_ba_solve_t(const float* S, const float* __restrict__ y, int N,
                                                              float* __restrict__ dX, BaMeta* meta, int iter, int* status_flag) {
  extern __shared__ __attribute__((aligned(16))) float solve_smem[];
  __shared__ int s_fail;
  // LDS image: rows x LD with an EVEN row stride (the global image k_ba_reduce wrote has n6 + 1): panel columns start at even
  // offsets (j0 = 6 jb), so the trailing update reads its operands as 8-byte pairs
  const int n6 = 6 * N, LDG = n6 + 1, LD = GLOBAL ? LDG : solve_ld(n6), rows = n6 + 1;
  float* A = GLOBAL ? const_cast<float*>(S) : solve_smem;
  float* Ld = GLOBAL ? solve_smem : A + rows * LD;   // [N][36] factored diagonal blocks (diagonal stored as reciprocal)
  float* Li = Ld + N * 36;                      // [N][36] their inverses (for the back-substitution)
  float* xs = Li + N * 36;                      // [n6] solution
  const int tid = threadIdx.x;
  if (tid == 0) s_fail = 0;
  if (!GLOBAL) {
    // k_ba_reduce wrote this very image (rows x LD, the right-hand side is row n6); eight loads in flight per thread
    const int total = rows * LDG - 1;
    const float inv_ldg = 1.0f / (float)LDG;
    for (int i0 = tid; i0 < total; i0 += SOLVE_THREADS * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { const int i = i0 + SOLVE_THREADS * u; v[u] = (i < total) ? S[i] : 0.0f; }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = i0 + SOLVE_THREADS * u;
        const int r = (int)(((float)i + 0.5f) * inv_ldg);         // exact: i < 2^16, margin 0.5 / LDG
        if (i < total) A[r * LD + (i - r * LDG)] = v[u];
      }
    }
  }
  __syncthreads();
  if (iter == 0 && tid == 0 && status_flag) *status_flag = meta->fail < 0 ? -1 : 0;      // (the call's status word starts here: no fill in front of the call)
  if (meta->fail) {                              // an earlier iteration broke down: the reference call has thrown by now
    if (tid == 0 && meta->fail < 0 && status_flag) *status_flag = -1;          // (or the workspace was never prepared)
    return;
  }

  // Look-ahead: the 6x6 diagonal block of step jb + 1 is brought up to date and factored by ONE wave (the last) while the other
  // waves run the trailing update of step jb — the serial rsq chain of the block factorisation leaves the panel phase.  The
  // tiles of that block (t < 6) are nobody else's; its updated values only ever feed the factorisation, so they are not written
  // back.  Same operations in the same order as the plain form: bit-identical factors.
  __shared__ float s_dblk[36];
  __shared__ float s_dump[64];
  constexpr int LA_WAVE = SOLVE_THREADS / 64 - 1;
  typedef float tl_f4 __attribute__((ext_vector_type(4)));
  const int tl_wv = tid >> 6, tl_mm = tid & 15, tl_kq = (tid & 63) >> 4;      // trailing update: this wave's 16 x 16 tile, this lane's operand row / k
  int tl_I = 0;
  while ((tl_I + 1) * (tl_I + 2) / 2 <= tl_wv) tl_I++;
  const int tl_J = tl_wv - tl_I * (tl_I + 1) / 2;
  auto factor_block = [&](int jb1) {                // all lanes of the calling wave; s_dblk holds the block's lower triangle
    float L[6][6];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c <= a; c++) L[a][c] = s_dblk[a * 6 + c];
    float inv[6];
    const bool ok = chol6(L, inv);
    if ((tid & 63) == 0) {
      if (!ok) s_fail = 1;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c <= a; c++) Ld[jb1 * 36 + a * 6 + c] = (a == c) ? inv[a] : L[a][c];
    }
  };
  if (tid < 64) {                                   // block 0 as it was loaded
    if (tid < 36 && tid % 6 <= tid / 6) s_dblk[tid] = A[(tid / 6) * LD + tid % 6];
    wave_lds_sync();
    factor_block(0);
  }
  __syncthreads();
  for (int jb = 0; jb < N; jb++) {
    const int j0 = 6 * jb;
    const int r = j0 + 6 + tid;                  // this thread's panel row (if any)
    if (r < rows) {                              // panel:  x L_bb^T = A[r][block], L_bb from the look-ahead (broadcast reads)
      float Lb[6][6], inv[6], x[6];
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int c = 0; c < a; c++) Lb[a][c] = Ld[jb * 36 + a * 6 + c];
        inv[a] = Ld[jb * 36 + a * 7];
      }
#pragma unroll
      for (int c = 0; c < 6; c++) {
        float v = A[r * LD + j0 + c];
#pragma unroll
        for (int k = 0; k < c; k++) v -= x[k] * Lb[c][k];
        x[c] = v * inv[c];
      }
#pragma unroll
      for (int c = 0; c < 6; c++) A[r * LD + j0 + c] = x[c];
    }
    __syncthreads();
    const bool next = jb + 1 < N;
    if (next && (tid >> 6) == LA_WAVE) {
      const int l = tid & 63, a = l / 6, c = l % 6, j1 = j0 + 6;
      if (l < 36 && c <= a) {
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 6; q++) acc += A[(j1 + a) * LD + j0 + q] * A[(j1 + c) * LD + j0 + q];
        s_dblk[a * 6 + c] = A[(j1 + a) * LD + j1 + c] - acc;
      }
      wave_lds_sync();
      factor_block(jb + 1);
    }
    // Trailing update  A[r][c] -= sum_q L[r][j0 + q] L[c][j0 + q]  (r >= c >= j0 + 6; the rhs row included) on the matrix cores:
    // 16 x 16 tiles of the trailing lower triangle, one per wave (waves 0 .. 14; wave 15 is the look-ahead), each
    // D = A x B + C with v_mfma_f32_16x16x4_f32 twice (k = 0..3, 4..7; columns 6, 7 are zero) — exact fp32 products and sums in a fixed
    // order.  Per lane 4 operand values and 4 result values come out of LDS (the 2 x 2 register tiles of round 2 read 28 values for 4
    // results), all conflict-free with the row stride of solve_ld().  Inputs = the panel columns, outputs = the columns to their
    // right: disjoint.  The 6 x 6 block the look-ahead wave factors meanwhile is not written back (nobody reads it again).
    if ((tid >> 6) != LA_WAVE) {
      const int base = j0 + 6, T = (rows - base + 15) >> 4, ntl = T * (T + 1) / 2;
      for (int t = tl_wv; t < ntl; t += LA_WAVE) {
        int I = tl_I, J = tl_J;                                    // the wave's first tile: the same (I, J) in every step
        if (t != tl_wv) { I = 0; while ((I + 1) * (I + 2) / 2 <= t) I++; J = t - I * (I + 1) / 2; }      // (more than 14 poses only)
        const int rb = base + 16 * I, cb = base + 16 * J;
        const float* pr = A + __mul24(min(rb + tl_mm, rows - 1), LD) + j0;      // operand rows (clamped: their products only reach masked results)
        const float* pc_ = A + __mul24(min(cb + tl_mm, rows - 1), LD) + j0;
        const float a1 = pr[tl_kq], a2r = pr[4 + (tl_kq & 1)], b1 = -pc_[tl_kq], b2r = -pc_[4 + (tl_kq & 1)];
        const float a2 = (tl_kq < 2) ? a2r : 0.0f, b2 = (tl_kq < 2) ? b2r : 0.0f;
        const int cc = cb + tl_mm, r0 = rb + 4 * tl_kq;
        // results: every lane reads and writes 4 entries UNCONDITIONALLY (entries outside the lower triangle / the matrix / the
        // look-ahead block go to a dump word; a conditional LDS access costs hipcc a branch and a full wait each)
        tl_f4 c;
        float* dst[4];
        float* p0 = A + __mul24(r0, LD) + cc;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = r0 + i;
          const bool ok = r < rows && cc < n6 && cc <= r && !(next && r < base + 6);
          dst[i] = ok ? p0 + i * LD : s_dump + (tid & 63);
          c[i] = *dst[i];
        }
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, c, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++) *dst[i] = c[i];
      }
    }
    __syncthreads();
  }
  if (s_fail) {
    // breakdown: dX = 0 (devo/ba.py:16-20: CholeskySolver returns zeros, no gradient through the solve) — the callers of the
    // differentiable path copy / read dX afterwards, and the workspace is not zero-initialised
    for (int i = tid; i < 6 * N; i += SOLVE_THREADS) dX[i] = 0.0f;
    if (tid == 0) { meta->fail = iter + 1; if (status_flag) *status_flag = iter + 1; }
    return;
  }
  // inverses of the diagonal blocks (one thread per block): the back-substitution then has no serial 6-step chain
  if (tid < N) {
    float Lb[6][6], X[6][6];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c <= a; c++) Lb[a][c] = Ld[tid * 36 + a * 6 + c];      // diagonal = reciprocal
#pragma unroll
    for (int c = 0; c < 6; c++) {                // column c of L^-1 by forward substitution
#pragma unroll
      for (int a = 0; a < 6; a++) {
        if (a < c) { X[a][c] = 0.0f; continue; }
        float v = (a == c) ? 1.0f : 0.0f;
#pragma unroll
        for (int k = 0; k < a; k++) if (k >= c) v -= Lb[a][k] * X[k][c];
        X[a][c] = v * Lb[a][a];
      }
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c < 6; c++) Li[tid * 36 + a * 6 + c] = X[a][c];
  }
  __syncthreads();
  // back substitution  L^T x = z  (z = row n6), bottom-up by blocks, by ONE wave: no workgroup barriers (the other
  // waves are done).  x_b = L_bb^-T z_b from the inverse block, then the lanes update their rows of z.  The solution is
  // collected in LDS (a global store inside the loop would put a vmcnt wait into every step's fence).
  if (tid >= 64) return;
  // Register form: lane r keeps z[r] and z[r + 64] (n6 <= 128 here).  One wave issues one instruction every ~5 cycles, so
  // a step is priced by its instruction count: the block's six z values come through v_readlane, lane c < 6 forms x_b[c]
  // from column c of the inverse block (6 FMAs), x_b goes back to all lanes through v_readlane, every lane updates its own
  // rows (rows >= 64 only matter for the last blocks) — no LDS access and no fence in the dependency chain.  The LDS
  // operands of a step (inverse block, the block's rows of L) do not depend on the solution: fetched one step ahead.
  float* z = A + n6 * LD;
  if (n6 <= 128) {
  const int lr0 = min(tid, n6 - 1), lr1 = min(tid + 64, n6 - 1), lc = min(tid, 5);
  float z0 = (tid < n6) ? z[tid] : 0.0f, z1 = (tid + 64 < n6) ? z[tid + 64] : 0.0f;
  struct StepOps { float li[6], a0[6]; };
  auto fetch = [&](int jb, StepOps& o) {
    const float* Lb = Li + jb * 36 + lc;
    const float* rowp = A + (6 * jb) * LD + lr0;
#pragma unroll
    for (int k = 0; k < 6; k++) { o.li[k] = Lb[k * 6]; o.a0[k] = rowp[k * LD]; }    // (L^-T)[c][k] = (L^-1)[k][c], 0 for k < c
  };
  auto lane_value = [](float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); };
  auto step = [&](int jb, const StepOps& o) {
    const int j0 = 6 * jb;
    float xc = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int r = j0 + k;                                        // wave-uniform
      xc += o.li[k] * lane_value((r >= 64) ? z1 : z0, r & 63);
    }
    if (tid < 6) xs[j0 + tid] = xc;
    float xb[6];
#pragma unroll
    for (int k = 0; k < 6; k++) xb[k] = lane_value(xc, k);
    float v0 = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) v0 += o.a0[k] * xb[k];
    if (tid < j0) z0 -= v0;
    if (j0 > 64) {                                                 // wave-uniform
      const float* rowp = A + j0 * LD + lr1;
      float v1 = 0.0f;
#pragma unroll
      for (int k = 0; k < 6; k++) v1 += rowp[k * LD] * xb[k];
      if (tid + 64 < j0) z1 -= v1;
    }
  };
  {
    StepOps oa, ob;
    int jb = N - 1;
    fetch(jb, oa);
    while (true) {
      fetch(max(jb - 1, 0), ob);                                   // (unconditional: a branch around loads costs a full wait at the join)
      step(jb, oa);
      if (--jb < 0) break;
      fetch(max(jb - 1, 0), oa);
      step(jb, ob);
      if (--jb < 0) break;
    }
  }
  wave_lds_sync();
  } else {                                        // more than 21 optimised poses: z stays in LDS
    for (int jb = N - 1; jb >= 0; jb--) {
      const int j0 = 6 * jb;
      float zb[6], xb[6];
  #pragma unroll
      for (int c = 0; c < 6; c++) zb[c] = z[j0 + c];
  #pragma unroll
      for (int c = 0; c < 6; c++) {
        float v = 0.0f;
  #pragma unroll
        for (int k = c; k < 6; k++) v += Li[jb * 36 + k * 6 + c] * zb[k];       // (L^-T)[c][k] = (L^-1)[k][c]
        xb[c] = v;
      }
      if (tid < 6) xs[j0 + tid] = (tid == 0) ? xb[0] : (tid == 1) ? xb[1] : (tid == 2) ? xb[2] : (tid == 3) ? xb[3] : (tid == 4) ? xb[4] : xb[5];
      wave_lds_sync();                             // all reads of z[j0..j0+5] done before rows above are updated
      for (int r = tid; r < j0; r += 64) {
        float v = 0.0f;
  #pragma unroll
        for (int k = 0; k < 6; k++) v += A[(j0 + k) * LD + r] * xb[k];
        z[r] -= v;
      }
      wave_lds_sync();
    }
  }
  for (int i = tid; i < n6; i += 64) dX[i] = xs[i];
}


constexpr auto k_ba_solve = k_ba_solve_t<false>;

// ------------------------------------------------------------------------------------------------- solve, one barrier per block step
// The factorisation above spends two workgroup barriers per block step and its look-ahead wave waits for the panel.  This form
// (6 N <= 128) has ONE barrier per step and no panel phase at all:
//   * the CHAIN wave (wave 15, raised priority, alone on its SIMD) prepares block jb + 1 while the others
//     update: lane (a, c) solves rows a and c of the six rows below the current block against L_bb (a packed pair: one substitution),
//     D_{jb+1}[a][c] = A - x_a . x_c, the 21 values travel through v_readlane, the 6 x 6 Cholesky runs redundantly in every lane,
//     lane 0 writes the factor;
//   * the twelve TILE waves (waves 0-2, 4-6, 8-10, 12-14: the wave id modulo 4 picks the SIMD) solve the operand rows of their 16 x 16
//     tile against L_bb themselves (both rows as a packed pair — the same arithmetic in the same order as the panel phase above) and
//     feed them to the matrix cores; the panel X = L[r][block] is never written over its source (the chain wave reads the raw rows
//     concurrently) but TRANSPOSED into the upper triangle (A[j0 + k][r]), where the back-substitution reads it with unit stride;
//   * tile wave 11 (wave 14; its tile only exists in the first steps) also inverts L_bb for the back-substitution; waves 3, 7 and 11
//     only hold the barrier: the chain wave has its SIMD to itself.
// The kernel is bound by VALU issue (a wave64 instruction takes the SIMD for 4 cycles; four tile waves per SIMD), not by LDS or the
// matrix cores: which tile entries a lane may write is a per-lane step count computed once (jb < thr[i]), the look-ahead rows and the
// triangle are folded into it.
// Same operations in the same order as k_ba_solve: bit-identical solutions (tests/test_gpu_fastba.py checks that).
typedef float solve_f2 __attribute__((ext_vector_type(2)));
// FUSED (k_ba_solve_retract, round 6): the launch has G workgroups and EVERY one of them factorises the same 6N x 6N system (the same
// operations in the same order: the same bits; ~30 KB of S out of the L2 each) and then retracts its own share of the patches with the
// solution still in its LDS — workgroup 0 also retracts the poses and writes dX / the status.  No workgroup waits for another one: what
// k_ba_retract did behind a kernel boundary (4.9 us + the boundary for 14 poses and 1 440 dot products) rides on the solver's launch.
struct BaRetract { float* poses; float* patches; const float* patch_rec; const float* patch_col; const int* kx; int P, t0; };
template <bool FUSED>
__device__ __forceinline__ void ba_solve_chain_body(const float* __restrict__ S, const float* __restrict__ y, int N,
                                                    float* __restrict__ dX, BaMeta* meta, int iter, int* status_flag,
                                                    const BaRetract& ra, int G = 0) {   // G > 0: the launch's first G workgroups solve (others ride along)
  extern __shared__ __attribute__((aligned(16))) float A[];
  const bool lead = blockIdx.x == 0;                              // (the only workgroup of the unfused launch)
  const int n_seg_all = FUSED ? meta->n_seg : 0;
  // (a prefetch of the retraction's operands under the factorisation was measured — no gain: 19.5 us either way — and dropped: it would read
  // through tables that a never-prepared workspace does not have before the kernel knows the call has failed)
  constexpr int UP = 2;
  const int nw = (G > 0 ? G : (int)gridDim.x) * 16, w0 = (int)blockIdx.x * 16 + (int)(threadIdx.x >> 6);
  __shared__ int s_fail;
  __shared__ float s_dump[64];
  const int n6 = 6 * N, LDG = n6 + 1, LD = solve_ld(n6), rows = n6 + 1;
  float* Ld = A + rows * LD;                    // [N][36] factored diagonal blocks (diagonal stored as reciprocal)
  float* Li = Ld + N * 36;                      // [N][36] their inverses (for the back-substitution)
  float* xs = Li + N * 36;                      // [n6] solution
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  constexpr int CHAIN = 15, NTW = 12;                            // the chain wave, the number of tile waves
  const bool tile_wave = (wv & 3) != 3;
  const int tw = wv - (wv >> 2);                                 // tile waves numbered 0 .. 11
  if (wv == CHAIN) __builtin_amdgcn_s_setprio(3);
  if (tid == 0) s_fail = 0;
  const int failed_before = meta->fail;           // (in flight with the matrix: a load after the barrier would add its whole latency)
  {
    const int total = rows * LDG - 1;
    const float inv_ldg = 1.0f / (float)LDG;
    for (int i0 = tid; i0 < total; i0 += 1024 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { const int i = i0 + 1024 * u; v[u] = (i < total) ? S[i] : 0.0f; }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = i0 + 1024 * u;
        const int r = (int)(((float)i + 0.5f) * inv_ldg);         // exact: i < 2^16, margin 0.5 / LDG
        if (i < total) A[r * LD + (i - r * LDG)] = v[u];
      }
    }
  }
  __syncthreads();
  // the call's status word is (re)set by its first solver launch — no fill in front of the call (round 6: the word may live in pinned host memory,
  // devo_amd.fastba: no copy behind the call either); every workgroup of a fused launch factorises the same system and fails alike, the lead
  // writes after its own reset
  if (iter == 0 && lead && tid == 0 && status_flag) *status_flag = failed_before < 0 ? -1 : 0;
  if (failed_before) {                           // an earlier iteration broke down: the reference call has thrown by now
    if (lead && tid == 0 && failed_before < 0 && status_flag) *status_flag = -1;  // (or the workspace was never prepared)
    return;
  }
  auto lane_value = [](float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); };
  auto load_factor = [&](int jb, float Lb[6][6], float inv[6]) {        // broadcast reads
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int c = 0; c < a; c++) Lb[a][c] = Ld[jb * 36 + a * 6 + c];
      inv[a] = Ld[jb * 36 + a * 7];
    }
  };
  // x L_bb^T = v for two rows at once (.x / .y): v_pk_fma_f32 / v_pk_mul_f32, each half rounded like the scalar form
  auto solve_rows = [](const float* pa, const float* pc, const float Lb[6][6], const float inv[6], solve_f2 x[6]) {
    solve_f2 v[6];
#pragma unroll
    for (int q = 0; q < 6; q++) v[q] = solve_f2{pa[q], pc[q]};
#pragma unroll
    for (int c = 0; c < 6; c++) {
      solve_f2 t = v[c];
#pragma unroll
      for (int k = 0; k < c; k++) t -= x[k] * Lb[c][k];
      x[c] = t * inv[c];
    }
  };
  auto factor_and_store = [&](float L[6][6], int jb1) {            // every lane holds the same block
    float inv[6];
    const bool ok = chol6(L, inv);
    if (ln == 0) {
      if (!ok) s_fail = 1;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c <= a; c++) Ld[jb1 * 36 + a * 6 + c] = (a == c) ? inv[a] : L[a][c];
    }
  };
  typedef float tl_f4 __attribute__((ext_vector_type(4)));
  const int tl_mm = ln & 15, tl_kq = ln >> 4;                   // trailing update: this lane's operand row / k group
  // A tile (I, J) of the trailing lower triangle, in coordinates relative to its corner j1 = 6 (jb + 1): what a lane reads and writes
  // moves by (6, 6) per step, and WHETHER it may write entry i is "jb < thr[i]": inside the matrix (row < rows - j1, column < rows - 1 -
  // j1), on or below the diagonal, not one of the six rows the chain wave is factoring (nobody reads those again).
  struct Tile { int thr[4], thr_t, rel_mine, rel_a, idx0, keep; };
  auto steps_while = [](int X) { return (X + 5) / 6 - 1; };       // jb < steps_while(X)  <=>  6 (jb + 1) < X
  auto make_tile = [&](int t) {
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) I++;
    const int J = t - I * (I + 1) / 2;
    Tile tl;
    const int rrel0 = 16 * I + 4 * tl_kq, crel = 16 * J + tl_mm;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = rrel0 + i;
      tl.thr[i] = (crel <= r && r >= 6) ? min(steps_while(rows - r), steps_while(rows - 1 - crel)) : -1;
    }
    tl.rel_a = 16 * I + tl_mm;
    tl.rel_mine = (tl_kq < 2) ? tl.rel_a : crel;                  // lanes 0-31 solve the tile's operand rows, lanes 32-63 its operand columns' rows
    tl.keep = J == 0;
    tl.thr_t = (J == 0) ? steps_while(rows - tl.rel_a) : -1;
    tl.idx0 = (6 + rrel0) * LD + 6 + crel;
    return tl;
  };
  // One 16 x 16 tile of one step.  The substitution runs ONCE per wave: lanes 0-31 (k groups 0, 1) hold operand row a = rb + mm, lanes
  // 32-63 row c = cb + mm; the matrix-core operands of lane (mm, kq) are X[a][kq], X[a][4 + kq] (kq < 2) and -X[c][kq], -X[c][4 + kq]:
  // half of them are its own, the other half its partner's (lane ^ 32, the same mm, kq ^ 2), swapped with v_permlane32_swap.
  // the value lane ^ 32 holds: v_permlane32_swap (VALU; a ds_bpermute waits ~200 cycles in the LDS queue while the tiles run)
  auto from_partner = [&](float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(ln < 32 ? r[1] : r[0]);
  };
  auto do_tile = [&](const Tile& tl, int jb, const float Lb[6][6], const float inv[6]) {
    const int j0 = 6 * jb, j1 = j0 + 6;
    const float* pr = A + __mul24(min(j1 + tl.rel_mine, rows - 1), LD) + j0;      // (clamped: the products of such rows only reach masked results)
    float v[6], x[6];
#pragma unroll
    for (int q = 0; q < 6; q++) v[q] = pr[q];
    tl_f4 c;
    float* dst[4];
    float* p0 = A + tl.idx0 + jb * (6 * LD + 6);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      dst[i] = (jb < tl.thr[i]) ? p0 + i * LD : s_dump + ln;
      c[i] = *dst[i];
    }
#pragma unroll
    for (int cc = 0; cc < 6; cc++) {
      float t = v[cc];
#pragma unroll
      for (int k = 0; k < cc; k++) t -= x[k] * Lb[cc][k];
      x[cc] = t * inv[cc];
    }
    const bool odd = tl_kq & 1, hi = tl_kq & 2;
    const float u = odd ? x[1] : x[0], w = odd ? x[3] : x[2];
    const float mine = hi ? w : u, theirs = hi ? u : w;            // x[kq], and x[kq ^ 2]: what the partner needs of this lane's row
    const float s2 = odd ? x[5] : x[4];                           // x[4 + (kq & 1)]: the same index on both sides
    const float got1 = from_partner(theirs), got2 = from_partner(s2);
    const float a1 = hi ? got1 : mine, b1 = hi ? mine : got1;
    const float a2 = hi ? 0.0f : s2, b2 = hi ? 0.0f : got2;
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, -b1, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, -b2, c, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) *dst[i] = c[i];
    if (tl.keep) {                                                 // the panel itself, transposed: X[r][k] -> A[j0 + k][r]  (column-0 tiles cover every row once)
      const bool ok = jb < tl.thr_t;
      float* t1 = ok ? A + __mul24(j0 + tl_kq, LD) + j1 + tl.rel_a : s_dump + ln;
      float* t2 = (ok && !hi) ? A + __mul24(j0 + 4 + tl_kq, LD) + j1 + tl.rel_a : s_dump + ln;
      *t1 = a1;
      *t2 = a2;
    }
  };
  const Tile my_tile = make_tile(tile_wave ? tw : 0);
  if (wv == CHAIN) {                                            // block 0 as it was loaded
    float L[6][6];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c <= a; c++) L[a][c] = A[a * LD + c];
    factor_and_store(L, 0);
  }
  __syncthreads();
  // every role runs its own loop (a taken branch costs ~30 cycles: no role dispatch inside the steps); N barriers each
  auto step_barrier = [&] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  if (wv == CHAIN) {
    const int la = ln < 36 ? ln / 6 : 5, lc = ln < 36 ? ln % 6 : 5;
    for (int jb = 0; jb < N; jb++) {
      if (jb + 1 < N) {
        const int j0 = 6 * jb, j1 = j0 + 6;
        const float* pr = A + (j1 + la) * LD + j0;
        const float* pc = A + (j1 + lc) * LD + j0;
        const float dv = pr[6 + lc];
        float Lb[6][6], inv[6];
        solve_f2 x[6];
        load_factor(jb, Lb, inv);
        solve_rows(pr, pc, Lb, inv, x);
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 6; q++) acc += x[q].x * x[q].y;
        const float d = dv - acc;
        float L[6][6];
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int c = 0; c <= a; c++) L[a][c] = lane_value(d, a * 6 + c);
        factor_and_store(L, jb + 1);
      }
      step_barrier();
    }
  } else if (tile_wave) {
    for (int jb = 0; jb < N; jb++) {
      const int T = (rows - 6 * jb - 6 + 15) >> 4, ntl = T * (T + 1) / 2;
      // the inverse of L_bb (for the back-substitution) is the job of the first tile wave WITHOUT a tile in this step (the last one while
      // all have tiles): in the late steps, where one to three tiles are left, it is not on the step's critical path
      const bool do_inv = tw == min(ntl, NTW - 1);
      if (tw < ntl || do_inv) {
        float Lb[6][6], inv[6];
        load_factor(jb, Lb, inv);
        if (tw < ntl) do_tile(my_tile, jb, Lb, inv);
        for (int t = tw + NTW; t < ntl; t += NTW) do_tile(make_tile(t), jb, Lb, inv);      // (more than 12 tiles: the first steps of 13+ poses)
        if (do_inv) {                                               // lane c < 6: column c of L^-1 by forward substitution
          const int c = min(ln, 5);
          float X[6];
#pragma unroll
          for (int a = 0; a < 6; a++) {
            float v = (a == c) ? 1.0f : 0.0f;
#pragma unroll
            for (int k = 0; k < a; k++) v -= Lb[a][k] * X[k];      // (rows above c are exact zeros: the same sums as a triangular loop)
            X[a] = v * inv[a];
          }
          if (ln < 6) {
#pragma unroll
            for (int a = 0; a < 6; a++) Li[jb * 36 + a * 6 + c] = X[a];
          }
        }
      }
      step_barrier();
    }
  } else {
    for (int jb = 0; jb < N; jb++) step_barrier();
  }
  if (s_fail) {                                                    // (FUSED: every workgroup sees the same breakdown; nobody retracts)
    if (lead) {
      for (int i = tid; i < 6 * N; i += 1024) dX[i] = 0.0f;       // (see k_ba_solve)
      if (tid == 0) { meta->fail = iter + 1; if (status_flag) *status_flag = iter + 1; }
    }
    return;
  }
  // back substitution  L^T x = z  by ONE wave in registers (see k_ba_solve); z = the transposed panel entries of the rhs row
  // (column n6), the rows of L^T a lane needs are contiguous in its own row of the upper triangle
  if (!FUSED && tid >= 64) return;
  if (tid < 64) {
  const int lr0 = min(tid, n6 - 1), lr1 = min(tid + 64, n6 - 1), lc = min(tid, 5);
  float z0 = (tid < n6) ? A[tid * LD + n6] : 0.0f, z1 = (tid + 64 < n6) ? A[(tid + 64) * LD + n6] : 0.0f;
  struct StepOps { float li[6], a0[6]; };
  auto fetch = [&](int jb, StepOps& o) {
    const float* Lb = Li + jb * 36 + lc;
    const float* rowp = A + lr0 * LD + 6 * jb;
#pragma unroll
    for (int k = 0; k < 6; k++) { o.li[k] = Lb[k * 6]; o.a0[k] = rowp[k]; }    // (L^-T)[c][k] = (L^-1)[k][c], 0 for k < c
  };
  auto step = [&](auto jbc, const StepOps& o) {                     // jb is a compile-time constant: static lane indices, no branches
    constexpr int jb = decltype(jbc)::value, j0 = 6 * jb;
    float zb[6], xb[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {                                  // all six before the first use: a v_readlane whose result is needed at once
      const int r = j0 + k;                                        // costs ~20 cycles, six in a row ~25
      zb[k] = lane_value((r >= 64) ? z1 : z0, r & 63);
    }
    float xc = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) xc += o.li[k] * zb[k];
    if (tid < 6) xs[j0 + tid] = xc;
#pragma unroll
    for (int k = 0; k < 6; k++) xb[k] = lane_value(xc, k);
    float v0 = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) v0 += o.a0[k] * xb[k];
    if (tid < j0) z0 -= v0;
    if (j0 > 64) {
      const float* rowp = A + lr1 * LD + j0;
      float v1 = 0.0f;
#pragma unroll
      for (int k = 0; k < 6; k++) v1 += rowp[k] * xb[k];
      if (tid + 64 < j0) z1 -= v1;
    }
  };
  // The block steps as ONE unrolled chain jb = 21 .. 0 entered at jb = N - 1 (a switch with fall-through): every step has its lane indices,
  // its `rows >= 64` case and its operand addresses at compile time and there is no loop branch (a taken branch costs ~36 cycles) —
  // 237 instead of 499 cycles per step (tools/ubench/backsub_step.hip), the same arithmetic in the same order.
  {
    StepOps o0, o1;                                                // operands of the even / odd block steps
#define DEVO_BS_FIRST(JB) case JB: fetch(JB, (JB & 1) ? o1 : o0); break;
#define DEVO_BS_STEP(JB) case JB: if (JB > 0) fetch(JB > 0 ? JB - 1 : 0, (JB & 1) ? o0 : o1); step(std::integral_constant<int, JB>{}, (JB & 1) ? o1 : o0); [[fallthrough]];
    switch (N - 1) {
      DEVO_BS_FIRST(21) DEVO_BS_FIRST(20) DEVO_BS_FIRST(19) DEVO_BS_FIRST(18) DEVO_BS_FIRST(17) DEVO_BS_FIRST(16) DEVO_BS_FIRST(15) DEVO_BS_FIRST(14)
      DEVO_BS_FIRST(13) DEVO_BS_FIRST(12) DEVO_BS_FIRST(11) DEVO_BS_FIRST(10) DEVO_BS_FIRST(9) DEVO_BS_FIRST(8) DEVO_BS_FIRST(7) DEVO_BS_FIRST(6)
      DEVO_BS_FIRST(5) DEVO_BS_FIRST(4) DEVO_BS_FIRST(3) DEVO_BS_FIRST(2) DEVO_BS_FIRST(1) DEVO_BS_FIRST(0)
      default: break;
    }
    switch (N - 1) {
      DEVO_BS_STEP(21) DEVO_BS_STEP(20) DEVO_BS_STEP(19) DEVO_BS_STEP(18) DEVO_BS_STEP(17) DEVO_BS_STEP(16) DEVO_BS_STEP(15) DEVO_BS_STEP(14)
      DEVO_BS_STEP(13) DEVO_BS_STEP(12) DEVO_BS_STEP(11) DEVO_BS_STEP(10) DEVO_BS_STEP(9) DEVO_BS_STEP(8) DEVO_BS_STEP(7) DEVO_BS_STEP(6)
      DEVO_BS_STEP(5) DEVO_BS_STEP(4) DEVO_BS_STEP(3) DEVO_BS_STEP(2) DEVO_BS_STEP(1) DEVO_BS_STEP(0)
      default: break;
    }
#undef DEVO_BS_FIRST
#undef DEVO_BS_STEP
  }
  wave_lds_sync();
  if (lead) for (int i = tid; i < n6; i += 64) dX[i] = xs[i];
  }
  if constexpr (FUSED) {
    // ---- retraction with the solution in LDS (k_ba_retract's arithmetic in its order: the same bits).  One wave per patch, the loads of
    //      a wave's patches (two at cfg2) in flight together; the lead workgroup's first N threads retract the poses.
    __syncthreads();
    const int PP = ra.P * ra.P;
    const float x0 = (ln < n6) ? xs[ln] : 0.0f, x1 = (ln + 64 < n6) ? xs[ln + 64] : 0.0f;
    for (int sb = w0; sb < n_seg_all; sb += nw * UP) {
      float c0[UP], c1[UP], q[UP], u[UP], d0[UP];
      float* pd[UP];
#pragma unroll
      for (int k = 0; k < UP; k++) {
        const int s = sb + k * nw;
        const int sc = s < n_seg_all ? s : sb;
        const float* pc = ra.patch_col + (int64_t)sc * n6;
        c0[k] = (ln < n6) ? pc[ln] : 0.0f;
        c1[k] = (ln + 64 < n6) ? pc[ln + 64] : 0.0f;
        q[k] = ra.patch_rec[(int64_t)sc * 2];
        u[k] = ra.patch_rec[(int64_t)sc * 2 + 1];
        pd[k] = ra.patches + ((int64_t)ra.kx[sc] * 3 + 2) * PP;
        d0[k] = pd[k][0];                                          // reads pixel [0][0] (ba_cuda.cu:198)
      }
#pragma unroll
      for (int k = 0; k < UP; k++) {
        if (sb + k * nw >= n_seg_all) break;                       // (wave-uniform)
        float part = 0.0f;
        if (N > 0) {
          if (ln < n6) part += c0[k] * x0;
          if (ln + 64 < n6) part += c1[k] * x1;
          part = wave_sum(part);
        }
        const float dz = q[k] * (u[k] - part);                     // Q (u - E^T dX)  (ba_cuda.cu:523)
        float d = d0[k] + dz;
        d = (d > 20.0f) ? 1.0f : d;
        d = fmaxf(d, 1e-4f);
        for (int i = ln; i < PP; i += 64) pd[k][i] = d;
      }
    }
    if (lead && tid < N) {
      float* p = ra.poses + (int64_t)(ra.t0 + tid) * 7;
      float tt[3] = {p[0], p[1], p[2]}, qq[4] = {p[3], p[4], p[5], p[6]}, t1[3], q1[4], dx[6];
#pragma unroll
      for (int k = 0; k < 6; k++) dx[k] = xs[6 * tid + k];
      fb_retrSE3(dx, tt, qq, t1, q1);
      p[0] = t1[0]; p[1] = t1[1]; p[2] = t1[2]; p[3] = q1[0]; p[4] = q1[1]; p[5] = q1[2]; p[6] = q1[3];
    }
  }
}
__global__ __launch_bounds__(1024) void k_ba_solve_chain(const float* __restrict__ S, const float* __restrict__ y, int N,
                                                         float* __restrict__ dX, BaMeta* meta, int iter, int* status_flag) {
  ba_solve_chain_body<false>(S, y, N, dX, meta, iter, status_flag, BaRetract{});
}
__global__ __launch_bounds__(1024) void k_ba_solve_retract(const float* __restrict__ S, const float* __restrict__ y, int N,
                                                           float* __restrict__ dX, BaMeta* meta, int iter, int* status_flag,
                                                           BaRetract ra) {
  ba_solve_chain_body<true>(S, y, N, dX, meta, iter, status_flag, ra);
}

// k_ba_solve_retract with the ordering step of the NEXT lookup's locality plan (corr_plan.h) in the workgroups behind the G solving ones: the
// solver's launch is 19 us of 90 busy compute units, the ordering 9 us of twenty others — a plan only decides which edges run together, so the
// lookup of update iteration k + 1 can take the plan made from iteration k's coordinates (devo_ba_forward_prepared_delta_plan).
template <int CACHE>
__global__ __launch_bounds__(1024) void k_ba_solve_retract_order(const float* __restrict__ S, const float* __restrict__ y, int N,
                                                                 float* __restrict__ dX, BaMeta* meta, int iter, int* status_flag,
                                                                 BaRetract ra, int G, const int* __restrict__ bins, int BE, int nbins,
                                                                 int* __restrict__ order, int starts) {
  if ((int)blockIdx.x >= G) { corr_order_body<CACHE>(bins, BE, nbins, order, (int)blockIdx.x - G, (int)gridDim.x - G, starts != 0); return; }
  ba_solve_chain_body<true>(S, y, N, dX, meta, iter, status_flag, ra, G);
}

static_assert(SOLVE_THREADS == 1024, "k_ba_solve_chain is written for 16 waves");
typedef void (*solve_fn_t)(const float*, const float*, int, float*, BaMeta*, int, int*);
static solve_fn_t ba_solve_fn(int N) {
  static const bool v1 = getenv("DEVO_BA_SOLVE_V1") != nullptr;   // A/B and test switch: the two-barrier form for every N
  return (6 * N <= 128 && !v1) ? k_ba_solve_chain : k_ba_solve;
}

// ------------------------------------------------------------------------------------------------- retract
// poses[t0+i] <- Exp(dX_i) * poses[t0+i]  (ba_cuda.cu:160-188);  d <- d + dz; d>20 -> 1; d >= 1e-4 (:191-211)
__global__ void k_ba_retract(float* __restrict__ poses, float* __restrict__ patches, const float* __restrict__ dX,
                             const float* __restrict__ patch_rec, const float* __restrict__ patch_col,
                             const int* __restrict__ kx, const BaMeta* __restrict__ meta, int P, int t0, int N) {
  if (meta->fail) return;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = blockDim.x * gridDim.x;
  const int lane = threadIdx.x & 63, wave = gid >> 6, nwaves = gsz >> 6;
  const int n_seg = meta->n_seg, n6 = 6 * N;
  for (int s = wave; s < n_seg; s += nwaves) {                      // one wave per patch, lanes over the rows of its E column
    float part = 0.0f;
    if (N > 0) {
      const float* pc = patch_col + (int64_t)s * n6;
      for (int i = lane; i < n6; i += 64) part += pc[i] * dX[i];
      part = wave_sum(part);
    }
    const float dz = patch_rec[(int64_t)s * 2] * (patch_rec[(int64_t)s * 2 + 1] - part);   // Q (u - E^T dX)  (ba_cuda.cu:523)
    float* pd = patches + ((int64_t)kx[s] * 3 + 2) * P * P;
    float d = pd[0] + dz;                                          // reads pixel [0][0] (:198)
    d = (d > 20.0f) ? 1.0f : d;
    d = fmaxf(d, 1e-4f);
    __builtin_amdgcn_wave_barrier();                               // every lane has read pd[0] before it is rewritten
    for (int i = lane; i < P * P; i += 64) pd[i] = d;
  }
  for (int t = gid; t < N; t += gsz) {
    float* p = poses + (int64_t)(t0 + t) * 7;
    float tt[3] = {p[0], p[1], p[2]}, q[4] = {p[3], p[4], p[5], p[6]}, t1[3], q1[4];
    fb_retrSE3(dX + 6 * t, tt, q, t1, q1);
    p[0] = t1[0]; p[1] = t1[1]; p[2] = t1[2]; p[3] = q1[0]; p[4] = q1[1]; p[5] = q1[2]; p[6] = q1[3];
  }
}

// ------------------------------------------------------------------------------------------------- differentiable step
// devo_ba_solve_terms: the normal equations, Schur complement and Cholesky solve of ONE Gauss-Newton step from GIVEN edge
// terms (devo/ba.py:108-170 behind devo_amd.ba.BA; the caller's autograd graph produces r, w, Ji, Jj, Jz and consumes
// dX, dZ), and its adjoint.  Forward: the accumulate / reduce / solve kernels above + k_bt_dz.  Backward, with
//   dZ = Q (u - E^T dX),  dX = S'^-1 y,  S' = S + (ep + 1e-4 diag S),  S = B - E Q E^T,  y = v - E Q u,  Q = 1 / (C + lambda):
//   a = Q gdZ,  ybar = S'^-1 (gdX - E a)   (the SAME matrix: one more solve),  Sbar = -(ybar dX^T) (1 + 1e-4 on the diagonal),
// everything else is per patch (k_bt_patch) and per edge (k_bt_edge) arithmetic on dX, ybar and the E columns.
__global__ void k_bt_dz(const float* __restrict__ dX, const float* __restrict__ patch_rec, const float* __restrict__ patch_col,
                        const int* __restrict__ kx, const BaMeta* __restrict__ meta, int N, float* __restrict__ dZ, float* __restrict__ dX_out) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, wave = gid >> 6, nwaves = (blockDim.x * gridDim.x) >> 6;
  const int n_seg = meta->fail < 0 ? 0 : meta->n_seg, n6 = 6 * N;
  if (dX_out && wave == 0)                                              // the caller's copy of the pose update (was a separate device copy)
    for (int i = lane; i < n6; i += 64) dX_out[i] = dX[i];
  for (int s = wave; s < n_seg; s += nwaves) {
    float part = 0.0f;
    const float* pc = patch_col + (int64_t)s * n6;
    for (int i = lane; i < n6; i += 64) part += pc[i] * dX[i];
    part = wave_sum(part);
    if (lane == 0) dZ[kx[s]] = patch_rec[(int64_t)s * 2] * (patch_rec[(int64_t)s * 2 + 1] - part);
  }
}

// right-hand side of the adjoint solve, accumulated into the solver image's last row (which the caller initialised with gdX)
__global__ __launch_bounds__(256) void k_bt_rhs(float* __restrict__ rhs, const float* __restrict__ g_dZ, const float* __restrict__ patch_rec,
                                                const float* __restrict__ patch_col, const int* __restrict__ kx,
                                                const BaMeta* __restrict__ meta, int N) {
  const int n_seg = meta->fail < 0 ? 0 : meta->n_seg, n6 = 6 * N, d = threadIdx.x;
  if (d >= n6) return;
  float acc = 0.0f;
  for (int s = blockIdx.x; s < n_seg; s += gridDim.x) acc += patch_col[(int64_t)s * n6 + d] * (patch_rec[(int64_t)s * 2] * g_dZ[kx[s]]);
  atomicAdd(rhs + d, -acc);
}

// per patch: prec[s] = {dZ = Q (u - e.dX),  zbar = Q (gdZ - e.ybar)  [the adjoint of dZ after the solve],  Q,  gamma = sum ybar dX e^2}
__global__ void k_bt_patch(const float* __restrict__ dX, const float* __restrict__ ybar, const float* __restrict__ g_dZ,
                           const float* __restrict__ patch_rec, const float* __restrict__ patch_col, const int* __restrict__ kx,
                           const BaMeta* __restrict__ meta, int N, float* __restrict__ prec) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, wave = gid >> 6, nwaves = (blockDim.x * gridDim.x) >> 6;
  const int n_seg = meta->fail < 0 ? 0 : meta->n_seg, n6 = 6 * N;
  for (int s = wave; s < n_seg; s += nwaves) {
    float al = 0.0f, be = 0.0f, ga = 0.0f;
    const float* pc = patch_col + (int64_t)s * n6;
    for (int i = lane; i < n6; i += 64) { const float e = pc[i], x = dX[i], yb = ybar[i]; al += x * e; be += yb * e; ga += yb * x * e * e; }
    al = wave_sum(al); be = wave_sum(be); ga = wave_sum(ga);
    if (lane == 0) {
      const float Q = patch_rec[(int64_t)s * 2], u = patch_rec[(int64_t)s * 2 + 1], gz = g_dZ[kx[s]];
      float* o = prec + (int64_t)s * 8;
      o[0] = Q * (u - al); o[1] = Q * (gz - be); o[2] = Q; o[3] = ga;
    }
  }
}

// patch slot -> compact patch index (the inverse of kx; the index preparation's own edge -> patch map is not written on its
// fast path for patch-major edge lists)
__global__ void k_bt_inv(const int* __restrict__ kx, const BaMeta* __restrict__ meta, int* __restrict__ inv) {
  const int n_seg = meta->fail < 0 ? 0 : meta->n_seg;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += blockDim.x * gridDim.x) inv[kx[s]] = s;
}

// per edge: gradients of the 30 terms.  With  lambda_d = A_d . ybar + Jz_d zbar_k  (the adjoint of the linearised residual) and
// rho_d = r_d - A_d . dX - Jz_d dZ_k  (the residual after the step), A_d = row d of [-Ji | Jj] (fixed blocks zeroed):
//   d/dr = w lambda,  d/dw = lambda rho,  d/dJz = w (zbar rho - dZ lambda),  d/dA = w (rho ybar - lambda dX)
// (no large cancelling terms), plus the O(1e-4) terms of the diagonal damping S_dd (1 + 1e-4).
__global__ void k_bt_edge(const float* __restrict__ terms, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                          const int64_t* __restrict__ kk, const int* __restrict__ inv, const float* __restrict__ dX,
                          const float* __restrict__ ybar, const float* __restrict__ patch_col, const float* __restrict__ prec,
                          const BaMeta* __restrict__ meta, int E, int t0, int N, float* __restrict__ g_terms) {
  const int n6 = 6 * N;
  const bool ok = meta->fail >= 0;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    float* g = g_terms + (int64_t)e * BA_TERMS;
    if (!ok) { for (int c = 0; c < BA_TERMS; c++) g[c] = 0.0f; continue; }
    const float* t = terms + (int64_t)e * BA_TERMS;
    const int s = inv[kk[e]];
    int I = (int)ii[e] - t0, J = (int)jj[e] - t0;
    if (I < 0 || I >= N) I = -1;
    if (J < 0 || J >= N) J = -1;
    const float* pr = prec + (int64_t)s * 8;
    const float dZk = pr[0], zb = pr[1], Q = pr[2], ga = pr[3];
    float Y[12], X[12], tiny[12];                                 // [block I | block J] of ybar and dX; damping part of the E-column gradient
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const bool vi = I >= 0, vj = J >= 0;
      Y[c] = vi ? ybar[6 * I + c] : 0.0f; X[c] = vi ? dX[6 * I + c] : 0.0f;
      Y[6 + c] = vj ? ybar[6 * J + c] : 0.0f; X[6 + c] = vj ? dX[6 * J + c] : 0.0f;
      tiny[c] = vi ? 2e-4f * Q * (Y[c] * X[c] * patch_col[(int64_t)s * n6 + 6 * I + c]) : 0.0f;
      tiny[6 + c] = vj ? 2e-4f * Q * (Y[6 + c] * X[6 + c] * patch_col[(int64_t)s * n6 + 6 * J + c]) : 0.0f;
    }
    const float ctiny = -Q * Q * 1e-4f * ga;                      // damping part of the gradient of C
    const bool same = I >= 0 && I == J;                           // both ends in ONE pose block: the diagonal terms see the sum
#pragma unroll
    for (int d = 0; d < 2; d++) {
      const float r = t[d], w = t[2 + d], Jz = t[4 + d];
      float A[12];
#pragma unroll
      for (int c = 0; c < 6; c++) { A[c] = I >= 0 ? -t[6 + 6 * d + c] : 0.0f; A[6 + c] = J >= 0 ? t[18 + 6 * d + c] : 0.0f; }
      float p = 0.0f, q = 0.0f, mt = 0.0f, dd = 0.0f, dg[12];
#pragma unroll
      for (int c = 0; c < 12; c++) { p += A[c] * Y[c]; q += A[c] * X[c]; mt += A[c] * tiny[c]; }
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const float a0 = same ? A[c] + A[6 + c] : A[c], a1 = same ? a0 : A[6 + c];
        dg[c] = a0 * Y[c] * X[c]; dg[6 + c] = a1 * Y[6 + c] * X[6 + c];
        dd += same ? a0 * dg[c] : (A[c] * dg[c] + A[6 + c] * dg[6 + c]);
      }
      const float lam = p + Jz * zb, rho = r - q - Jz * dZk;
      g[d] = w * lam;
      g[2 + d] = lam * rho - 1e-4f * dd + Jz * mt + Jz * Jz * ctiny;
      g[4 + d] = w * (zb * rho - dZk * lam) + w * mt + 2.0f * w * Jz * ctiny;
#pragma unroll
      for (int c = 0; c < 12; c++) {
        const float Ab = w * (rho * Y[c] - lam * X[c]) - 2e-4f * w * dg[c] + w * Jz * tiny[c];
        if (c < 6) g[6 + 6 * d + c] = I >= 0 ? -Ab : 0.0f;          // Ji enters as -Ji
        else g[18 + 6 * d + (c - 6)] = J >= 0 ? Ab : 0.0f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- host: kernel choice
static size_t acc_reg_lds_bytes(int N) {
  const size_t n6 = 6 * (size_t)N, waves = acc_waves(N);
  return sizeof(float) * (n6 * (n6 + 1) + n6 + waves * n6 + 4 + waves * SCR_ROWS * SCR_LD + waves * ((size_t)N * (N + 1) / 2 * 36 + n6));
}
typedef void (*acc_fn_t)(const float*, const float*, const float*, TargetSrc, const float*, const float*, const int64_t*,
                         const int64_t*, const int64_t*, const int*, const int*, BaMeta*, int, int, int, float*, float*,
                         float*, int, int, int);
static acc_fn_t acc_reg_fn(int N) {
  return (N <= 8) ? k_ba_accumulate_reg<8, 8, true> : (N <= 11) ? k_ba_accumulate_reg<11, 8, true> :
         (N <= 14) ? k_ba_accumulate_reg<14, 6, true> : k_ba_accumulate_reg<16, 4, true>;
}

}  // namespace devo

using namespace devo;

extern "C" {
// ------------------------------------------------------------------------------------------------- host: devo_ba_forward*
size_t devo_ba_workspace_bytes(int E, int Np, int N) {
  if (E < 0 || Np < 0 || N < 0 || N > BA_MAXN) return 0;
  return ba_layout(E, Np, N).total;
}

// k_ba_schur + k_ba_damp behind k_ba_reduce(ep = BA_EP_DEFERRED): the Schur term of the general accumulate kernel as one product
static void ba_deferred_schur(hipStream_t st, const float* patch_rec, const float* patch_col, const BaMeta* meta, int N, int max_seg, float* S, float ep,
                              float* scratch, size_t scratch_bytes) {
  const int nt = (6 * N + 1 + SCH_T - 1) / SCH_T, ntile = nt * (nt + 1) / 2, nchunk = (max_seg + SCH_K - 1) / SCH_K;
  float* part = (size_t)ntile * nchunk * SCH_T * SCH_T * sizeof(float) <= scratch_bytes ? scratch : nullptr;     // else: float atomics
  hipLaunchKernelGGL(k_ba_schur, dim3((unsigned)ntile, (unsigned)nchunk), dim3(256), 0, st, patch_rec, patch_col, meta, N, max_seg, S, part);
  hipLaunchKernelGGL(k_ba_damp, dim3(blocks_for(36LL * N * N + 6 * N, 256, 256)), dim3(256), 0, st, S, N, ep, (const float*)part, nchunk, meta, max_seg);
}

static thread_local int g_ba_path = -1;                            // what the last devo_ba_forward of this thread launched
static int ba_check_args(const char* who, int E, int Nbuf, int Np, int P, int t0, int t1) {
  const int N = t1 - t0;
  if (!(E >= 0 && Np > 0 && Nbuf > 0 && P > 0)) { set_error("%s: bad sizes", who); return DEVO_ERR_ARG; }
  if (!(N >= 0 && t0 >= 0 && t1 <= Nbuf)) { set_error("%s: bad pose window [%d,%d) for %d poses", who, t0, t1, Nbuf); return DEVO_ERR_ARG; }
  if (N > BA_MAXN) { set_error("%s: %d optimised poses > %d supported", who, N, BA_MAXN); return DEVO_ERR_UNSUPPORTED; }
  return DEVO_OK;
}

int devo_ba_forward(float* poses, float* patches, const float* intrinsics, const float* target, const float* weight,
                    const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Nbuf, int Np,
                    int P, int t0, int t1, int iterations, void* ws, size_t ws_bytes, int* status_flag,
                    devo_stream_t stream) {
  int rc;
  if ((rc = ba_check_args("devo_ba_forward", E, Nbuf, Np, P, t0, t1))) return rc;
  if (E == 0 || iterations <= 0) return DEVO_OK;
  if ((rc = ba_prepare_impl(kk, E, Np, t1 - t0, ws, ws_bytes, (hipStream_t)stream))) return rc;
  return devo_ba_forward_prepared(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, E, Nbuf, Np, P, t0, t1,
                                  iterations, ws, ws_bytes, status_flag, stream);
}

static int ba_forward_impl(float* poses, float* patches, const float* intrinsics, const TargetSrc target, const float* weight,
                           const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Nbuf,
                           int Np, int P, int t0, int t1, int iterations, void* ws, size_t ws_bytes, int* status_flag,
                           devo_stream_t stream, PlanRider rider = PlanRider{nullptr, 0, 0});

int devo_ba_forward_prepared(float* poses, float* patches, const float* intrinsics, const float* target, const float* weight,
                             const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Nbuf,
                             int Np, int P, int t0, int t1, int iterations, void* ws, size_t ws_bytes, int* status_flag,
                             devo_stream_t stream) {
  return ba_forward_impl(poses, patches, intrinsics, TargetSrc{target, nullptr, 0, 0, 0}, weight, lmbda, ii, jj, kk, E, Nbuf, Np, P,
                         t0, t1, iterations, ws, ws_bytes, status_flag, stream);
}

int devo_ba_forward_prepared_delta(float* poses, float* patches, const float* intrinsics, const float* coords, int coords_edge_stride,
                                   int coords_xy_stride, int coords_centre, const float* delta, const float* weight,
                                   const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Nbuf,
                                   int Np, int P, int t0, int t1, int iterations, void* ws, size_t ws_bytes, int* status_flag,
                                   devo_stream_t stream) {
  DEVO_REQUIRE(coords != nullptr && coords_edge_stride > 0 && coords_xy_stride > 0 && coords_centre >= 0,
               "devo_ba_forward_prepared_delta: coords %p, strides %d / %d, centre %d", (const void*)coords, coords_edge_stride,
               coords_xy_stride, coords_centre);
  return ba_forward_impl(poses, patches, intrinsics, TargetSrc{delta, coords, coords_edge_stride, coords_xy_stride, coords_centre},
                         weight, lmbda, ii, jj, kk, E, Nbuf, Np, P, t0, t1, iterations, ws, ws_bytes, status_flag, stream);
}

static int ba_forward_impl(float* poses, float* patches, const float* intrinsics, const TargetSrc target, const float* weight,
                           const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Nbuf,
                           int Np, int P, int t0, int t1, int iterations, void* ws, size_t ws_bytes, int* status_flag,
                           devo_stream_t stream, PlanRider rider) {
  int rc;
  if ((rc = ba_check_args("devo_ba_forward", E, Nbuf, Np, P, t0, t1))) return rc;
  const int N = t1 - t0;
  if (E == 0) return DEVO_OK;
  if (iterations <= 0) {                                          // (no solver launch to ride on)
    if (rider.plan) { launch_order_only((hipStream_t)stream, E, rider); return check_launch("devo_ba_forward(order)"); }
    return DEVO_OK;
  }
  const BaLayout L = ba_layout(E, Np, N);
  if (ws == nullptr || ws_bytes < L.total) { set_error("devo_ba_forward: workspace %zu < %zu bytes", ws_bytes, L.total); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  BaMeta* meta = (BaMeta*)(w + L.meta);
  int* counts = (int*)(w + L.counts);
  int* perm_b = (int*)(w + L.perm_b);
  int* kx = (int*)(w + L.kx);
  float* partials = (float*)(w + L.partials);
  float* S = (float*)(w + L.S);
  float* y = (float*)(w + L.y);
  float* dX = (float*)(w + L.dX);
  float* patch_rec = (float*)(w + L.patch_rec);
  float* edge_ej = (float*)(w + L.edge_ej);
  // (with poses to optimise the first solver launch resets the status word; a structure-only call has no solver)
  if (status_flag && N == 0 && hipMemsetAsync(status_flag, 0, sizeof(int), st) != hipSuccess) { set_error("devo_ba_forward: memset failed"); return DEVO_ERR_LAUNCH; }

  const size_t n6 = 6 * (size_t)N;
  const float ep = 1.0f;                                          // ba_cuda.cu:518
  const bool big = N > BA_MAXN_LDS;                               // the system in global memory (see BA_MAXN)
  const size_t acc_lds = big ? sizeof(float) * (ACC_WAVES * n6 + 4) : sizeof(float) * (n6 * (n6 + 1) + n6 + ACC_WAVES * n6 + 4);
  const size_t solve_lds = big ? sizeof(float) * (72 * (size_t)N + n6 + 4) : sizeof(float) * ((n6 + 1) * (size_t)solve_ld((int)n6) + 72 * (size_t)N + n6 + 4);
  static const bool force_generic = getenv("DEVO_BA_GENERIC") != nullptr;   // test switch: the general accumulate kernel for every N
  const bool use_reg = (N <= 16) && !force_generic;
  const size_t acc_lds_used = use_reg ? acc_reg_lds_bytes(N) : acc_lds;
  acc_fn_t acc_fn = use_reg ? acc_reg_fn(N) : big ? k_ba_accumulate_t<true> : k_ba_accumulate;
  // what this call runs (devo_ba_last_path: accumulate kind | 4 * solve kind) and, once per process, a line when the system leaves the LDS
  g_ba_path = (use_reg ? 0 : big ? 2 : 1) | ((big ? 2 : (6 * N <= 128 ? 0 : 1)) << 2);
  if (big) {
    static bool noted = false;
    static const bool quiet = [] { const char* e = getenv("DEVO_LOG_FALLBACK"); return e && e[0] == '0'; }();
    if (!quiet && !noted) {
      noted = true;
      fprintf(stderr, "[devo_hip] cuda_ba.forward: %d optimised poses > %d: the reduced system lives in global memory (slower kernels); cuda_ba.last_path() names the kernels of every call\n", N, BA_MAXN_LDS);
    }
  }
  solve_fn_t solve_fn = big ? k_ba_solve_t<true> : ba_solve_fn(N);
  // round 6: the retraction rides on the solver's launch (k_ba_solve_retract: G workgroups factorise the same system, each retracts its
  // own patches).  G: one patch per wave, at most 128 workgroups.  DEVO_BA_FUSE_RETRACT=0: the two launches of rounds 1-5.
  static const bool fuse_env = [] { const char* e = getenv("DEVO_BA_FUSE_RETRACT"); return !(e && e[0] == '0'); }();
  const bool fuse_retract = fuse_env && N > 0 && solve_fn == k_ba_solve_chain;
  // (measured at cfg2, 1 440 patches, rocprofv3: G = 1 / 4 / 12 / 23 / 45 / 90 / 180 -> 93.9 / 37.5 / 24.7 / 21.3 / 19.6 / 19.2 / 19.1 us; the solver alone 19.5)
  const int retract_wgs = L.max_seg <= 16 ? 1 : (L.max_seg + 15) / 16 > 128 ? 128 : (L.max_seg + 15) / 16;
  if (fuse_retract && solve_lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)k_ba_solve_retract, hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds) != hipSuccess) {
    (void)hipGetLastError();
    set_error("devo_ba_forward: cannot reserve %zu bytes of LDS", solve_lds);
    return DEVO_ERR_LAUNCH;
  }
  if (acc_lds_used > 64 * 1024 || solve_lds > 64 * 1024) {
    if (hipFuncSetAttribute((const void*)acc_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)acc_lds_used) != hipSuccess ||
        hipFuncSetAttribute((const void*)solve_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds) != hipSuccess) {
      (void)hipGetLastError();
      set_error("devo_ba_forward: cannot reserve %zu / %zu bytes of LDS", acc_lds_used, solve_lds);
      return DEVO_ERR_LAUNCH;
    }
  }
  // the general kernel (N > 16) leaves the Schur term to ONE product afterwards (k_ba_schur)
  const bool defer = !use_reg && N > 0;
  for (int it = 0; it < iterations; it++) {
    if (big && hipMemsetAsync(S, 0, sizeof(float) * (n6 + 1) * (n6 + 1), st) != hipSuccess) { set_error("devo_ba_forward: memset failed"); return DEVO_ERR_LAUNCH; }
    hipLaunchKernelGGL(acc_fn, dim3(L.n_part), dim3(use_reg ? acc_waves(N) * 64 : ACC_THREADS), acc_lds_used, st, poses, patches, intrinsics, target,
                       weight, lmbda, ii, jj, kk, perm_b, counts, meta, P, t0, N, big ? S : partials, patch_rec, edge_ej, it | (defer ? 1 << 16 : 0), ba_sig(E, N), L.max_seg);
    if ((rc = check_launch("devo_ba_forward(accumulate)"))) return rc;
    if (N > 0) {
      if (!big) hipLaunchKernelGGL(k_ba_reduce, dim3((unsigned)((N * (N + 1) / 2 * 36 + n6 + 63) / 64)), dim3(512), 0, st, partials, L.n_part, N, S, y, defer ? BA_EP_DEFERRED : ep);
      if (defer) ba_deferred_schur(st, patch_rec, edge_ej, meta, N, L.max_seg, S, ep, partials, L.partials_bytes);
      if ((rc = check_launch("devo_ba_forward(reduce)"))) return rc;
      const long long order_ept = ((long long)E + ORDER_THREADS - 1) / ORDER_THREADS;
      if (fuse_retract && rider.plan && order_ept <= 32) {        // the next lookup's plan rides on this launch (once per call)
        typedef void (*ride_fn_t)(const float*, const float*, int, float*, BaMeta*, int, int*, BaRetract, int, const int*, int, int, int*, int);
        ride_fn_t ride = order_ept <= 8 ? k_ba_solve_retract_order<8> : order_ept <= 16 ? k_ba_solve_retract_order<16> :
                         order_ept <= 24 ? k_ba_solve_retract_order<24> : k_ba_solve_retract_order<32>;
        if (solve_lds > 48 * 1024 && hipFuncSetAttribute((const void*)ride, hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds) != hipSuccess) {
          (void)hipGetLastError();
          set_error("devo_ba_forward: cannot reserve %zu bytes of LDS", solve_lds);
          return DEVO_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(ride, dim3((unsigned)(retract_wgs + corr_order_workgroups(E, rider.nbins))), dim3(SOLVE_THREADS), solve_lds, st, S, y, N, dX, meta, it,
                           status_flag, BaRetract{poses, patches, patch_rec, edge_ej, kx, P, t0}, retract_wgs, (const int*)(rider.plan + E + 1), E,
                           rider.nbins, rider.plan, rider.starts);
        rider.plan = nullptr;                                     // done
      } else if (fuse_retract)
        hipLaunchKernelGGL(k_ba_solve_retract, dim3((unsigned)retract_wgs), dim3(SOLVE_THREADS), solve_lds, st, S, y, N, dX, meta, it, status_flag,
                           BaRetract{poses, patches, patch_rec, edge_ej, kx, P, t0});
      else
        hipLaunchKernelGGL(solve_fn, dim3(1), dim3(SOLVE_THREADS), solve_lds, st, S, y, N, dX, meta, it, status_flag);
      if ((rc = check_launch("devo_ba_forward(solve)"))) return rc;
    }
    if (!fuse_retract) {
      hipLaunchKernelGGL(k_ba_retract, dim3(blocks_for((long long)L.max_seg * 64 > N ? (long long)L.max_seg * 64 : N, 256, 2048)), dim3(256), 0, st, poses, patches, dX, patch_rec,
                         edge_ej, kx, meta, P, t0, N);
      if ((rc = check_launch("devo_ba_forward(retract)"))) return rc;
    }
  }
  if (rider.plan) launch_order_only(st, E, rider);               // (no fused solver launch in this call: structure-only, N > 21, switches)
  return check_launch("devo_ba_forward");
}

int devo_ba_forward_prepared_delta_plan(float* poses, float* patches, const float* intrinsics, const float* coords, int coords_edge_stride,
                                        int coords_xy_stride, int coords_centre, const float* delta, const float* weight,
                                        const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Nbuf,
                                        int Np, int P, int t0, int t1, int iterations, void* ws, size_t ws_bytes, int* status_flag,
                                        int* plan, int plan_frames, int plan_height, int plan_width, int plan_l1, devo_stream_t stream) {
  DEVO_REQUIRE(coords != nullptr && coords_edge_stride > 0 && coords_xy_stride > 0 && coords_centre >= 0,
               "devo_ba_forward_prepared_delta_plan: coords %p, strides %d / %d, centre %d", (const void*)coords, coords_edge_stride,
               coords_xy_stride, coords_centre);
  DEVO_REQUIRE(plan != nullptr && plan_frames > 0 && plan_height > 0, "devo_ba_forward_prepared_delta_plan: missing plan");
  PlanRider rider;
  int rc;
  if ((rc = ba_plan_rider("devo_ba_forward_prepared_delta_plan", plan, plan_frames, plan_height, plan_width, plan_l1, &rider))) return rc;
  return ba_forward_impl(poses, patches, intrinsics, TargetSrc{delta, coords, coords_edge_stride, coords_xy_stride, coords_centre},
                         weight, lmbda, ii, jj, kk, E, Nbuf, Np, P, t0, t1, iterations, ws, ws_bytes, status_flag, stream, rider);
}


int devo_ba_last_path(void) { return g_ba_path; }

// ---- one differentiable Gauss-Newton step from given edge terms (devo/ba.py:108-170) and its adjoint
static int bt_common(const char* who, int E, int Np, int N, size_t ws_bytes, void* ws, BaLayout* L) {
  if (!(E >= 0 && Np > 0 && N >= 0)) { set_error("%s: bad sizes", who); return DEVO_ERR_ARG; }
  if (N > BA_MAXN_LDS) { set_error("%s: %d optimised poses > %d supported by the differentiable solve", who, N, BA_MAXN_LDS); return DEVO_ERR_UNSUPPORTED; }
  *L = ba_layout(E, Np, N);
  if (ws == nullptr || ws_bytes < L->total) { set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, L->total); return DEVO_ERR_WORKSPACE; }
  return DEVO_OK;
}

int devo_ba_solve_terms(const float* terms, const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                        int Np, int t0, int N, float ep, void* ws, size_t ws_bytes, float* dX_out, float* dZ_out, int* status_flag,
                        devo_stream_t stream) {
  BaLayout L;
  int rc;
  if ((rc = bt_common("devo_ba_solve_terms", E, Np, N, ws_bytes, ws, &L))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t n6 = 6 * (size_t)N;
  // (dX | dZ in one buffer — devo_amd.backends.cuda_ba.solve_terms — are cleared by one fill)
  const bool joined = n6 > 0 && dZ_out == dX_out + n6;
  if ((joined ? hipMemsetAsync(dX_out, 0, sizeof(float) * (n6 + (size_t)Np), st)
              : hipMemsetAsync(dZ_out, 0, sizeof(float) * (size_t)Np, st)) != hipSuccess ||
      (!joined && n6 && hipMemsetAsync(dX_out, 0, sizeof(float) * n6, st) != hipSuccess) ||
      (status_flag && hipMemsetAsync(status_flag, 0, sizeof(int), st) != hipSuccess)) { set_error("devo_ba_solve_terms: memset failed"); return DEVO_ERR_LAUNCH; }
  if (E == 0) return DEVO_OK;
  if ((rc = ba_prepare_impl(kk, E, Np, N, ws, ws_bytes, st))) return rc;
  char* w = (char*)ws;
  BaMeta* meta = (BaMeta*)(w + L.meta);
  float* S = (float*)(w + L.S);
  float* dX = (float*)(w + L.dX);
  float* patch_rec = (float*)(w + L.patch_rec);
  float* patch_col = (float*)(w + L.edge_ej);
  const size_t acc_lds = sizeof(float) * (n6 * (n6 + 1) + n6 + ACC_WAVES * n6 + 4);
  const size_t solve_lds = sizeof(float) * ((n6 + 1) * (size_t)solve_ld((int)n6) + 72 * (size_t)N + n6 + 4);
  const bool use_reg = N <= 16;
  const size_t acc_lds_used = use_reg ? acc_reg_lds_bytes(N) : acc_lds;
  acc_fn_t acc_fn = use_reg ? acc_reg_fn(N) : k_ba_accumulate;
  if (acc_lds_used > 64 * 1024 || solve_lds > 64 * 1024) {
    if (hipFuncSetAttribute((const void*)acc_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)acc_lds_used) != hipSuccess ||
        hipFuncSetAttribute((const void*)ba_solve_fn(N), hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds) != hipSuccess) {
      (void)hipGetLastError();
      set_error("devo_ba_solve_terms: cannot reserve %zu / %zu bytes of LDS", acc_lds_used, solve_lds);
      return DEVO_ERR_LAUNCH;
    }
  }
  const bool defer = !use_reg && N > 0;                          // (the general kernel: the Schur term afterwards, see ba_forward_impl)
  // (poses / patches / intrinsics / weight are not read in terms mode; lmbda doubles as the 4-float intrinsics read)
  const TargetSrc src{nullptr, nullptr, 0, 0, 0, terms};
  hipLaunchKernelGGL(acc_fn, dim3(L.n_part), dim3(use_reg ? acc_waves(N) * 64 : ACC_THREADS), acc_lds_used, st, (const float*)nullptr, (const float*)nullptr,
                     (const float*)(w + L.y) /* 4 readable floats */, src, (const float*)nullptr, lmbda, ii, jj, kk, (int*)(w + L.perm_b), (int*)(w + L.counts),
                     meta, 3, t0, N, (float*)(w + L.partials), patch_rec, patch_col, defer ? 1 << 16 : 0, ba_sig(E, N), L.max_seg);
  if ((rc = check_launch("devo_ba_solve_terms(accumulate)"))) return rc;
  if (N > 0) {
    hipLaunchKernelGGL(k_ba_reduce, dim3((unsigned)((N * (N + 1) / 2 * 36 + n6 + 63) / 64)), dim3(512), 0, st, (float*)(w + L.partials), L.n_part, N, S,
                       (float*)(w + L.y), defer ? BA_EP_DEFERRED : ep);
    if (defer) ba_deferred_schur(st, patch_rec, patch_col, meta, N, L.max_seg, S, ep, (float*)(w + L.partials), L.partials_bytes);
    hipLaunchKernelGGL(ba_solve_fn(N), dim3(1), dim3(SOLVE_THREADS), solve_lds, st, S, (float*)(w + L.y), N, dX, meta, 0, status_flag);
    if ((rc = check_launch("devo_ba_solve_terms(solve)"))) return rc;
  }
  hipLaunchKernelGGL(k_bt_dz, dim3(blocks_for((long long)L.max_seg * 64, 256, 1024)), dim3(256), 0, st, dX, patch_rec, patch_col, (int*)(w + L.kx), meta, N, dZ_out,
                     N > 0 ? dX_out : nullptr);
  return check_launch("devo_ba_solve_terms");
}

int devo_ba_solve_terms_backward(const float* terms, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Np, int t0, int N, void* ws,
                                 size_t ws_bytes, const float* g_dX, const float* g_dZ, float* g_terms, devo_stream_t stream) {
  BaLayout L;
  int rc;
  if ((rc = bt_common("devo_ba_solve_terms_backward", E, Np, N, ws_bytes, ws, &L))) return rc;
  if (E == 0) return DEVO_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t n6 = 6 * (size_t)N;
  char* w = (char*)ws;
  BaMeta* meta = (BaMeta*)(w + L.meta);
  float* S = (float*)(w + L.S);
  float* dX = (float*)(w + L.dX);
  float* ybar = (float*)(w + L.ybar);
  float* patch_rec = (float*)(w + L.patch_rec);
  float* patch_col = (float*)(w + L.edge_ej);
  float* prec = (float*)(w + L.prec);
  const int* kx = (const int*)(w + L.kx);
  if (hipMemsetAsync(ybar, 0, sizeof(float) * (n6 + 1), st) != hipSuccess) { set_error("devo_ba_solve_terms_backward: memset failed"); return DEVO_ERR_LAUNCH; }
  if (N > 0) {
    float* rhs = S + n6 * (n6 + 1);                            // the solver image's right-hand-side row
    if (hipMemcpyAsync(rhs, g_dX, sizeof(float) * n6, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("devo_ba_solve_terms_backward: copy failed"); return DEVO_ERR_LAUNCH; }
    hipLaunchKernelGGL(k_bt_rhs, dim3(64), dim3(256), 0, st, rhs, g_dZ, patch_rec, patch_col, kx, meta, N);
    const size_t solve_lds = sizeof(float) * ((n6 + 1) * (size_t)solve_ld((int)n6) + 72 * (size_t)N + n6 + 4);
    hipLaunchKernelGGL(ba_solve_fn(N), dim3(1), dim3(SOLVE_THREADS), solve_lds, st, S, (float*)(w + L.y), N, ybar, meta, 0, (int*)nullptr);
    if ((rc = check_launch("devo_ba_solve_terms_backward(solve)"))) return rc;
  }
  hipLaunchKernelGGL(k_bt_patch, dim3(blocks_for((long long)L.max_seg * 64, 256, 1024)), dim3(256), 0, st, dX, ybar, g_dZ, patch_rec, patch_col, kx, meta, N, prec);
  int* inv = (int*)(w + L.rank);                                // [Np + 1] ints, free once the graph is prepared
  hipLaunchKernelGGL(k_bt_inv, dim3(blocks_for(L.max_seg, 256, 256)), dim3(256), 0, st, kx, meta, inv);
  hipLaunchKernelGGL(k_bt_edge, dim3(blocks_for(E, 128, 4096)), dim3(128), 0, st, terms, ii, jj, kk, inv, dX, ybar, patch_col, prec, meta, E, t0, N, g_terms);
  return check_launch("devo_ba_solve_terms_backward");
}

// devo/ba.py:95-106 in one kernel (training): the 30 per-edge numbers devo_ba_solve_terms takes, from transform's outputs.
//   r = gate * (target - centre),  w = gate * weight,  gate = valid * [|target - centre| < 250] * [centre inside bounds]
//   terms[e] = r(2) | w(2) | Jz(2) | -Ji(12) | Jj(12)
// and its adjoint (the gate is piecewise constant): d target = gate * g_r, d centre = -gate * g_r (written into the centre pixel of a
// zeroed coordinate cotangent), d weight = gate * g_w, d Jz = g_Jz, d Ji = -g_Ji, d Jj = g_Jj.
__global__ void k_ba_edge_terms(const float* __restrict__ coords, const float* __restrict__ valid, const float* __restrict__ Ji,
                                const float* __restrict__ Jj, const float* __restrict__ Jz, const float* __restrict__ target,
                                const float* __restrict__ weight, float b0, float b1, float b2, float b3, int E, int P,
                                float* __restrict__ terms, float* __restrict__ gate_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int c = P / 2;
  const float* ctr = coords + ((int64_t)(e * P + c) * P + c) * 2;
  const float cx = ctr[0], cy = ctr[1];
  const float rx = target[2 * e] - cx, ry = target[2 * e + 1] - cy;
  float gate = valid[e];
  gate *= (sqrtf(rx * rx + ry * ry) < 250.0f) ? 1.0f : 0.0f;
  gate *= (cx > b0 && cy > b1 && cx < b2 && cy < b3) ? 1.0f : 0.0f;
  float* t = terms + (int64_t)e * 30;
  t[0] = gate * rx; t[1] = gate * ry;
  t[2] = gate * weight[2 * e]; t[3] = gate * weight[2 * e + 1];
  t[4] = Jz[2 * e]; t[5] = Jz[2 * e + 1];
#pragma unroll
  for (int q = 0; q < 12; q++) { t[6 + q] = -Ji[12 * (int64_t)e + q]; t[18 + q] = Jj[12 * (int64_t)e + q]; }
  gate_out[e] = gate;
}

__global__ void k_ba_edge_terms_bwd(const float* __restrict__ g_terms, const float* __restrict__ gate, int E, int P,
                                    float* __restrict__ g_coords /* zeroed */, float* __restrict__ g_target, float* __restrict__ g_weight,
                                    float* __restrict__ g_Ji, float* __restrict__ g_Jj, float* __restrict__ g_Jz) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int c = P / 2;
  const float* g = g_terms + (int64_t)e * 30;
  const float gt = gate[e];
  const float grx = gt * g[0], gry = gt * g[1];
  g_target[2 * e] = grx; g_target[2 * e + 1] = gry;
  float* gc = g_coords + ((int64_t)(e * P + c) * P + c) * 2;
  gc[0] = -grx; gc[1] = -gry;
  g_weight[2 * e] = gt * g[2]; g_weight[2 * e + 1] = gt * g[3];
  g_Jz[2 * e] = g[4]; g_Jz[2 * e + 1] = g[5];
#pragma unroll
  for (int q = 0; q < 12; q++) { g_Ji[12 * (int64_t)e + q] = -g[6 + q]; g_Jj[12 * (int64_t)e + q] = g[18 + q]; }
}

int devo_ba_edge_terms(const float* coords, const float* valid, const float* Ji, const float* Jj, const float* Jz, const float* target,
                       const float* weight, const float* bounds /* host, 4 */, int E, int P, float* terms, float* gate, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && P > 0 && bounds != nullptr, "devo_ba_edge_terms: bad arguments");
  if (E == 0) return DEVO_OK;
  hipLaunchKernelGGL(k_ba_edge_terms, dim3(blocks_for(E, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, coords, valid, Ji, Jj, Jz, target, weight,
                     bounds[0], bounds[1], bounds[2], bounds[3], E, P, terms, gate);
  return check_launch("devo_ba_edge_terms");
}

int devo_ba_edge_terms_backward(const float* g_terms, const float* gate, int E, int P, float* g_coords, float* g_target, float* g_weight,
                                float* g_Ji, float* g_Jj, float* g_Jz, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && P > 0, "devo_ba_edge_terms_backward: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(g_coords, 0, sizeof(float) * 2 * (size_t)E * P * P, st) != hipSuccess) { set_error("devo_ba_edge_terms_backward: memset failed"); return DEVO_ERR_LAUNCH; }
  if (E == 0) return DEVO_OK;
  hipLaunchKernelGGL(k_ba_edge_terms_bwd, dim3(blocks_for(E, 256, 1 << 20)), dim3(256), 0, st, g_terms, gate, E, P, g_coords, g_target, g_weight, g_Ji,
                     g_Jj, g_Jz);
  return check_launch("devo_ba_edge_terms_backward");
}

}  // extern "C"

namespace devo {

#define LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)blockDim.x * gridDim.x)

template <typename T> DEVO_HD void store_grad7(T* p, const T* g6) {
#pragma unroll
  for (int k = 0; k < 6; k++) p[k] = g6[k];
  p[6] = T(0);
}

// The update step of the differentiable BA (devo/ba.py:172-182) as one kernel per direction: poses[fixedp .. fixedp + n_opt) <- Exp(dX_i) * pose_i
// (`poses.retr`), every patch's inverse depth <- clamp(d + dZ_k, dmin, dmax) over its P x P pixels, everything else copied.  The reference
// (and round 3) ran it as torch.stack / clamp / zeros / slice assignment + the Exp and Mul group ops: ~8 launches forward, ~12 backward.
// Work item i < N: pose i; item N + k: patch k.
__global__ void k_ba_apply_step(const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ dX, const float* __restrict__ dZ,
                                int N, int Np, int PP, int fixedp, int n_opt, float dmin, float dmax, float* __restrict__ poses_out, float* __restrict__ patches_out) {
  LOOP(i, (int64_t)N + Np) {
    if (i < N) {
      SE3<float> X = SE3<float>::load(poses + i * 7);
      if (i >= fixedp && i < fixedp + n_opt) X = se3_exp<float>(dX + (i - fixedp) * 6).mul(X);
      X.store(poses_out + i * 7);
    } else {
      const int64_t k = i - N;
      const float* p = patches + k * 3 * PP;
      float* o = patches_out + k * 3 * PP;
      const float dz = dZ[k];
      for (int j = 0; j < 2 * PP; j++) o[j] = p[j];
      for (int j = 2 * PP; j < 3 * PP; j++) o[j] = fminf(fmaxf(p[j] + dz, dmin), dmax);
    }
  }
}
// adjoint: g_poses_out [N,7] (lietorch's embedding: tangent in the first six), g_patches_out -> g_poses, g_patches, g_dX [6 n_opt], g_dZ [Np]
__global__ void k_ba_apply_step_bwd(const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ dX, const float* __restrict__ dZ,
                                    const float* __restrict__ g_poses_out, const float* __restrict__ g_patches_out, int N, int Np, int PP, int fixedp,
                                    int n_opt, float dmin, float dmax, float* __restrict__ g_poses, float* __restrict__ g_patches, float* __restrict__ g_dX,
                                    float* __restrict__ g_dZ) {
  LOOP(i, (int64_t)N + Np) {
    if (i < N) {
      if (i >= fixedp && i < fixedp + n_opt) {
        const float* a = dX + (i - fixedp) * 6;
        float g[7], o[6], ga7[7];
#pragma unroll
        for (int k = 0; k < 7; k++) g[k] = g_poses_out ? g_poses_out[i * 7 + k] : 0.0f;
        se3_exp<float>(a).row_times_Adj(g, o);                          // Mul's adjoint (lietorch_gpu.cu:112-125): d left = g, d right = g Adj(left)
        store_grad7(g_poses + i * 7, o);
        store_grad7(ga7, g);
        row_times_left_jacobian<float>(ga7, a, g_dX + (i - fixedp) * 6); // Exp's adjoint (:32-44)
      } else {
#pragma unroll
        for (int k = 0; k < 7; k++) g_poses[i * 7 + k] = g_poses_out ? g_poses_out[i * 7 + k] : 0.0f;
      }
    } else {
      const int64_t k = i - N;
      const float* p = patches + k * 3 * PP;
      const float* g = g_patches_out ? g_patches_out + k * 3 * PP : nullptr;
      float* o = g_patches + k * 3 * PP;
      const float dz = dZ[k];
      float s = 0.0f;
      for (int j = 0; j < 2 * PP; j++) o[j] = g ? g[j] : 0.0f;
      for (int j = 2 * PP; j < 3 * PP; j++) {
        const float d = p[j] + dz;
        const float gj = (g && d >= dmin && d <= dmax) ? g[j] : 0.0f;    // clamp passes the gradient inside [dmin, dmax] (ATen's clamp_backward mask)
        o[j] = gj; s += gj;
      }
      g_dZ[k] = s;
    }
  }
}

}  // namespace devo

extern "C" {

int devo_ba_apply_step(const float* poses, const float* patches, const float* dX, const float* dZ, int N, int Np, int P, int fixedp, int n_opt,
                       float dmin, float dmax, float* poses_out, float* patches_out, devo_stream_t s) {
  if (N < 0 || Np < 0 || P <= 0 || fixedp < 0 || n_opt < 0 || fixedp + n_opt > N) { set_error("devo_ba_apply_step: bad sizes"); return DEVO_ERR_ARG; }
  if (N + Np == 0) return DEVO_OK;
  if (!poses || !patches || !dZ || !poses_out || !patches_out || (n_opt > 0 && !dX)) { set_error("devo_ba_apply_step: null tensor"); return DEVO_ERR_ARG; }
  hipLaunchKernelGGL(k_ba_apply_step, dim3((unsigned)((N + Np + 255) / 256)), dim3(256), 0, (hipStream_t)s, poses, patches, dX, dZ, N, Np, P * P, fixedp, n_opt,
                     dmin, dmax, poses_out, patches_out);
  return check_launch("devo_ba_apply_step");
}
int devo_ba_apply_step_backward(const float* poses, const float* patches, const float* dX, const float* dZ, const float* g_poses_out, const float* g_patches_out,
                                int N, int Np, int P, int fixedp, int n_opt, float dmin, float dmax, float* g_poses, float* g_patches, float* g_dX,
                                float* g_dZ, devo_stream_t s) {
  if (N < 0 || Np < 0 || P <= 0 || fixedp < 0 || n_opt < 0 || fixedp + n_opt > N) { set_error("devo_ba_apply_step_backward: bad sizes"); return DEVO_ERR_ARG; }
  if (N + Np == 0) return DEVO_OK;
  if (!poses || !patches || !dZ || !g_poses || !g_patches || !g_dZ || (n_opt > 0 && (!dX || !g_dX))) { set_error("devo_ba_apply_step_backward: null tensor"); return DEVO_ERR_ARG; }
  hipLaunchKernelGGL(k_ba_apply_step_bwd, dim3((unsigned)((N + Np + 255) / 256)), dim3(256), 0, (hipStream_t)s, poses, patches, dX, dZ, g_poses_out, g_patches_out,
                     N, Np, P * P, fixedp, n_opt, dmin, dmax, g_poses, g_patches, g_dX, g_dZ);
  return check_launch("devo_ba_apply_step_backward");
}

}  // extern "C"
