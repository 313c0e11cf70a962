// The graph index tables of fastba and the Update operator for gfx950: the edge list grouped by patch (kx = unique(kk) sorted, segment
// starts, the edges of every patch in ascending order — ba_cuda.cu:435-437 as an integer counting sort, bit-exact `unique`), by ONE
// workgroup for E < 32 K edges and by the multi-kernel stages beyond; the same tables for the frame-pair key of the Update operator
// (devo_upd_graph_tables), their import into another workspace, and the temporal-neighbour helper (ba.cpp:127-139).
// The Gauss-Newton kernels that read these tables are in ba.hip, the workspace they live in is laid out by ba_layout.h.
#include "ba_layout.h"
#include <cstddef>
#include "corr_tile.h"
#include "corr_plan.h"
#include <stdlib.h>

namespace devo {

// ------------------------------------------------------------------------------------------------- scans
// In-place exclusive scan of data[0..n) by ONE workgroup of 1024 threads; data[n] = total (returned to all).  s_part: >= 48 ints.
// Round 6: every wave owns a contiguous span and walks it 64 consecutive elements at a time — coalesced loads, four steps in flight, a DPP scan per
// step, the carry in a scalar — where rounds 1-5 gave every THREAD a contiguous chunk and waited for each of its loads in turn: 191 us for the 131 072
// hash slots of cuda_ba.neighbors at DEVO's steady-state size (45 312 edges), ~0.75 us per element and thread.  Integer sums: any order, the same bits.
__device__ __forceinline__ int block_excl_scan_1024(int* data, int n, int* s_part) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int span = ((n + 16 * 64 - 1) / (16 * 64)) * 64;     // elements per wave, whole steps of 64
  const int lo = min(n, wave * span), hi = min(n, lo + span);
  constexpr int UB = 4;
  int s = 0;
  for (int i0 = lo; i0 < hi; i0 += 64 * UB) {
    int v[UB];
#pragma unroll
    for (int u = 0; u < UB; u++) { const int i = i0 + 64 * u + lane; v[u] = (i < hi) ? data[i] : 0; }
#pragma unroll
    for (int u = 0; u < UB; u++) s += v[u];
  }
  const int x = wave_inclusive_sum(s);
  if (lane == 63) s_part[wave] = x;              // the wave's total
  __syncthreads();
  if (wave == 0) {
    const int w = (lane < 16) ? s_part[lane] : 0;
    int y = w;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) { const int v = __shfl_up(y, off); if (lane >= off) y += v; }
    if (lane < 16) s_part[16 + lane] = y - w;   // exclusive prefix of every wave
    if (lane == 15) s_part[32] = y;             // grand total
  }
  __syncthreads();
  int carry = s_part[16 + wave];                 // (wave-uniform)
  for (int i0 = lo; i0 < hi; i0 += 64 * UB) {
    int v[UB];
#pragma unroll
    for (int u = 0; u < UB; u++) { const int i = i0 + 64 * u + lane; v[u] = (i < hi) ? data[i] : 0; }
#pragma unroll
    for (int u = 0; u < UB; u++) {
      const int i = i0 + 64 * u + lane;
      const int inc = wave_inclusive_sum(v[u]);
      if (i < hi) data[i] = carry + inc - v[u];
      carry += __builtin_amdgcn_readlane(inc, 63);
    }
  }
  const int total = s_part[32];
  if (t == 1023) data[n] = total;
  __syncthreads();
  return total;
}

// ------------------------------------------------------------------------------------------------- multi-kernel preparation
// ---- the multi-kernel preparation works on the RANGE of patch ids the edge list holds, not on all patch slots (round 6): DEVO's buffers have
// 2048 frames x 96 = 196 608 slots, a sliding-window graph touches the 2 112 patches of 22 frames — flags, scan and the unique-id sweep over the
// slots cost 380 us there, over the range 30.  range[0] = max(-k), range[1] = max(k) over the valid ids (both start at 0x80808080: "minus infinity").
__device__ __forceinline__ void kk_range_body(const int64_t* __restrict__ kk, int E, int Np, int* __restrict__ range) {
  int nlo = (int)0x80808080, hi = (int)0x80808080;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    const int64_t k = kk[e];
    if (k >= 0 && k < Np) { nlo = max(nlo, -(int)k); hi = max(hi, (int)k); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { nlo = max(nlo, __shfl_xor(nlo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  __shared__ int s_r[2][4];                                    // one pair of atomics per workgroup: they all hit one cache line
  if ((threadIdx.x & 63) == 0) { s_r[0][threadIdx.x >> 6] = nlo; s_r[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int a = max(max(s_r[0][0], s_r[0][1]), max(s_r[0][2], s_r[0][3])), b = max(max(s_r[1][0], s_r[1][1]), max(s_r[1][2], s_r[1][3]));
    if (b != (int)0x80808080) { atomicMax(&range[0], a); atomicMax(&range[1], b); }
  }
}
__global__ void k_kk_range(const int64_t* __restrict__ kk, int E, int Np, int* __restrict__ range) { kk_range_body(kk, E, Np, range); }
__device__ __forceinline__ void kk_range(const int* __restrict__ range, int& kmin, int& Rg) {
  const int nlo = range[0], hi = range[1];
  const bool any = hi != (int)0x80808080;
  kmin = any ? -nlo : 0;
  Rg = any ? hi - kmin + 1 : 0;
}
__device__ __forceinline__ void flag_ids_r_body(const int64_t* __restrict__ kk, int E, int Np, int* flags, const int* __restrict__ range) {
  int kmin, Rg;
  kk_range(range, kmin, Rg);
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    const int64_t k = kk[e];
    if (k >= 0 && k < Np) flags[(int)k - kmin] = 1;
  }
}
__global__ void k_flag_ids_r(const int64_t* __restrict__ kk, int E, int Np, int* flags, const int* __restrict__ range) { flag_ids_r_body(kk, E, Np, flags, range); }
// block_excl_scan_1024 over a length read on the device: mode 0 = the id range (range), mode 1 = min(*n_ptr, cap) (the segment counts: n_seg of them)
__device__ __forceinline__ void excl_scan_dev_body(int* data, const int* __restrict__ n_ptr, int mode, int cap, int* total_out) {
  __shared__ int s_part[1024];
  int n;
  if (mode == 0) { int kmin; kk_range(n_ptr, kmin, n); } else n = min(*n_ptr, cap);
  const int total = block_excl_scan_1024(data, n, s_part);
  if (threadIdx.x == 0 && total_out) *total_out = total;
  if (mode == 1) for (int i = n + 1 + threadIdx.x; i <= cap; i += 1024) data[i] = total;     // segment starts beyond n_seg = E: any reader sees empty tails
}
__global__ __launch_bounds__(1024) void k_excl_scan_dev(int* data, const int* __restrict__ n_ptr, int mode, int cap, int* total_out) { excl_scan_dev_body(data, n_ptr, mode, cap, total_out); }
// Few, large segments (the Update operator's frame-pair groups: 45 312 edges in 210 groups) make the per-edge device atomics of the counting and
// scattering passes queue on a handful of addresses (23 us each where the patch groups take 5): when n_seg <= SEG_LDS_MAX and the average segment
// holds >= 64 edges, every workgroup counts in LDS first and issues ONE device atomic per segment it met.
constexpr int SEG_LDS_MAX = 1024;
__device__ __forceinline__ bool seg_lds_path(int n_seg, int E) { return n_seg <= SEG_LDS_MAX && (long long)n_seg * 64 <= E; }
__device__ __forceinline__ void rank_edges_r_body(const int64_t* __restrict__ kk, int E, int Np, const int* __restrict__ rank, int* ku, int* kx,
                                                      int* counts, const int* __restrict__ range, const int* __restrict__ n_seg_p) {
  __shared__ int s_hist[SEG_LDS_MAX];
  int kmin, Rg;
  kk_range(range, kmin, Rg);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = blockDim.x * gridDim.x;
  const int n_seg = max(*n_seg_p, 1);                         // (edges with bad ids count for segment 0, even when no id is good)
  if (seg_lds_path(n_seg, E)) {
    for (int b = threadIdx.x; b < n_seg; b += blockDim.x) s_hist[b] = 0;
    __syncthreads();
    for (int e = gid; e < E; e += gsz) {
      const int64_t k = kk[e];
      const int r = (k >= 0 && k < Np) ? rank[(int)k - kmin] : 0;
      ku[e] = r;
      atomicAdd(&s_hist[r], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_seg; b += blockDim.x) { const int c = s_hist[b]; if (c) atomicAdd(&counts[b], c); }
  } else {
    for (int e = gid; e < E; e += gsz) {
      const int64_t k = kk[e];
      const int r = (k >= 0 && k < Np) ? rank[(int)k - kmin] : 0;
      ku[e] = r;
      atomicAdd(&counts[r], 1);
    }
  }
  for (int p = gid; p < Rg; p += gsz)
    if (rank[p + 1] != rank[p]) kx[rank[p]] = kmin + p;
}
__global__ __launch_bounds__(256) void k_rank_edges_r(const int64_t* __restrict__ kk, int E, int Np, const int* __restrict__ rank, int* ku, int* kx,
                                                      int* counts, const int* __restrict__ range, const int* __restrict__ n_seg_p) { rank_edges_r_body(kk, E, Np, rank, ku, kx, counts, range, n_seg_p); }
// (devo_ba_neighbors: the groups are hash slots)
__global__ void k_scatter_edges(const int* __restrict__ ku, int E, const int* __restrict__ seg_start, int* cursor, int* perm) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    int s = ku[e];
    perm[seg_start[s] + atomicAdd(&cursor[s], 1)] = e;
  }
}
// The same with the workgroup's edges ranked in LDS first (see seg_lds_path): one device atomic per (workgroup, segment) reserves the slots.
__device__ __forceinline__ void scatter_edges_seg_body(const int* __restrict__ ku, int E, const int* __restrict__ seg_start, int* cursor, int* perm,
                                                           const int* __restrict__ n_seg_p) {
  __shared__ int s_hist[SEG_LDS_MAX];
  const int n_seg = max(*n_seg_p, 1);
  const int gsz = blockDim.x * gridDim.x;
  if (!seg_lds_path(n_seg, E)) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gsz) {
      const int s = ku[e];
      perm[seg_start[s] + atomicAdd(&cursor[s], 1)] = e;
    }
    return;
  }
  for (int base = blockIdx.x * blockDim.x; base < E; base += gsz) {          // (uniform per workgroup: the barriers below are safe)
    for (int b = threadIdx.x; b < n_seg; b += blockDim.x) s_hist[b] = 0;
    __syncthreads();
    const int e = base + threadIdx.x;
    int s = 0, lr = 0;
    if (e < E) { s = ku[e]; lr = atomicAdd(&s_hist[s], 1); }
    __syncthreads();
    for (int b = threadIdx.x; b < n_seg; b += blockDim.x) { const int c = s_hist[b]; if (c) s_hist[b] = atomicAdd(&cursor[b], c); }
    __syncthreads();
    if (e < E) perm[seg_start[s] + s_hist[s] + lr] = e;
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_scatter_edges_seg(const int* __restrict__ ku, int E, const int* __restrict__ seg_start, int* cursor, int* perm,
                                                           const int* __restrict__ n_seg_p) { scatter_edges_seg_body(ku, E, seg_start, cursor, perm, n_seg_p); }
// Restore a deterministic (ascending edge id) order inside every segment: rank sort, one wave per segment.
__device__ __forceinline__ void sort_segments_body(const int* __restrict__ seg_start, BaMeta* __restrict__ meta, int sig, const int* __restrict__ in, int* out) {
  const int* n_seg_p = &meta->n_seg;
  if (blockIdx.x == 0 && threadIdx.x == 0) meta->sig = sig;      // the workspace now holds a prepared graph
  if (meta->pad) return;                                         // the list was already grouped: perm is the identity
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (blockDim.x * gridDim.x) >> 6;
  const int n_seg = *n_seg_p;
  for (int s = wave; s < n_seg; s += nwaves) {
    const int a = seg_start[s], m = seg_start[s + 1] - a;
    for (int i = lane; i < m; i += 64) {
      int x = in[a + i], r = 0;
      for (int j = 0; j < m; j++) r += (in[a + j] < x);
      out[a + r] = x;
    }
  }
}
__global__ void k_sort_segments(const int* __restrict__ seg_start, BaMeta* __restrict__ meta, int sig, const int* __restrict__ in, int* out) { sort_segments_body(seg_start, meta, sig, in, out); }

// ---- the multi-kernel preparation of TWO edge lists of one length in the same launches (devo_upd_graph_tables: the edges grouped by patch and by
// frame pair, once per frame in DEVO's steady state): blockIdx.y picks the problem, every stage is one launch instead of two — 11 launches for
// what took 22 (each ~4.5 us of a nearly idle chip).  One preparation keeps the plain-pointer kernels above: launched with gridDim.y = 1, the
// struct forms cost it ~1 us of its 30 (profiles/ba_split.txt).
struct Prep2 {
  const int64_t* kk[2]; BaMeta* meta[2]; int* rank[2]; int* counts[2]; int* cursor[2]; int* ku[2]; int* kx[2]; int* perm_a[2]; int* perm_b[2]; int* range[2];
};
__global__ void k_kk_range2(Prep2 p, int E, int Np) { const int y = blockIdx.y; kk_range_body(p.kk[y], E, Np, p.range[y]); }
__global__ void k_flag_ids_r2(Prep2 p, int E, int Np) { const int y = blockIdx.y; flag_ids_r_body(p.kk[y], E, Np, p.rank[y], p.range[y]); }
__global__ __launch_bounds__(1024) void k_excl_scan_dev2(Prep2 p, int mode, int cap) {
  const int y = blockIdx.y;
  if (mode == 0) excl_scan_dev_body(p.rank[y], p.range[y], 0, 0, &p.meta[y]->n_seg);
  else excl_scan_dev_body(p.counts[y], &p.meta[y]->n_seg, 1, cap, nullptr);
}
__global__ __launch_bounds__(256) void k_rank_edges_r2(Prep2 p, int E, int Np) {
  const int y = blockIdx.y;
  rank_edges_r_body(p.kk[y], E, Np, p.rank[y], p.ku[y], p.kx[y], p.counts[y], p.range[y], &p.meta[y]->n_seg);
}
__global__ __launch_bounds__(256) void k_scatter_edges_seg2(Prep2 p, int E) {
  const int y = blockIdx.y;
  scatter_edges_seg_body(p.ku[y], E, p.counts[y], p.cursor[y], p.perm_a[y], &p.meta[y]->n_seg);
}
__global__ void k_sort_segments2(Prep2 p, int sig) { const int y = blockIdx.y; sort_segments_body(p.counts[y], p.meta[y], sig, p.perm_a[y], p.perm_b[y]); }
// what the two hipMemsetAsync pairs of two preparations and the pair key's range fill did: the heads of both workspaces (meta | rank | counts | cursor)
// to zero, the three id ranges to "minus infinity" (0x80808080)
__global__ __launch_bounds__(256) void k_prep_clear2(int4* __restrict__ a0, int4* __restrict__ a1, long long n4, int* r0, int* r1, int* r2) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gsz = (long long)blockDim.x * gridDim.x;
  const int4 z = make_int4(0, 0, 0, 0);
  for (long long i = gid; i < n4; i += gsz) { a0[i] = z; a1[i] = z; }
  if (gid < 4) { r0[gid] = (int)0x80808080; r1[gid] = (int)0x80808080; r2[gid] = (int)0x80808080; }
}

// ------------------------------------------------------------------------------------------------- single-workgroup preparation
// Whole graph preparation in ONE launch (one workgroup of 1024 threads) for E <= 2^17:
//   range of kk -> presence flags over [kmin, kmax] -> rank (sorted unique patch ids, ba_cuda.cu:435-437)
//   -> per-patch edge counts -> segment starts -> scatter.   (The in-segment order is restored at the end.)
// Everything a lane needs a RETURNED atomic for lives in LDS when it fits (<= 16384 ids in range, <= 8192 unique
// patches — DEVO's sliding window is ~2k patches); otherwise the same arrays in the workspace are used.
constexpr int PREP_FLAGS_LDS = 16384;
constexpr int PREP_SEGS_LDS = 8192;
template <int CACHE>      // CACHE = 0: kk is re-read by every pass; else ceil(E / 1024) <= CACHE edges per thread in registers
__device__ __forceinline__ void ba_prepare_body(const int64_t* __restrict__ kk, int E, int Np, int max_seg, BaMeta* meta,
                                                int* g_rank, int* g_counts, int* g_cursor, int* ku, int* kx, int* perm_a,
                                                int* perm_b, int sig) {
  extern __shared__ int s_mem[];
  int* s_part = s_mem;                       // 1024
  int* s_flags = s_part + 1024;              // PREP_FLAGS_LDS + 1
  int* s_counts = s_flags + PREP_FLAGS_LDS + 1;   // PREP_SEGS_LDS + 1
  int* s_cursor = s_counts + PREP_SEGS_LDS + 1;   // PREP_SEGS_LDS
  __shared__ int s_min, s_max;
  const int t = threadIdx.x;
  if (t == 0) { s_min = 0x7fffffff; s_max = -1; }
  // patch id of edge t + 1024 i (or -1: out of range / no edge).  CACHED: all loads in flight at once, every later
  // pass runs from registers; otherwise kk is re-read by every pass.
  constexpr bool CACHED = CACHE > 0;
  int kreg[CACHED ? CACHE : 1];
  auto patch_of = [&](int i) -> int {
    if (CACHED) return kreg[i];
    const int e = t + 1024 * i;
    if (e >= E) return -1;
    const int64_t k = kk[e];
    return (k >= 0 && k < Np) ? (int)k : -1;
  };
  const int iters = CACHED ? CACHE : (E + 1023) / 1024;
  if (CACHED) {
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const int e = t + 1024 * i;
      int64_t k = -1;
      if (e < E) k = kk[e];
      kreg[i] = (k >= 0 && k < Np) ? (int)k : -1;
    }
  }
  // Already grouped?  If the patch ids are ascending along the edge list (kk-major graphs: enet.py:300-301, any list
  // built patch by patch) every segment is a run, the permutation is the identity and the whole counting sort below
  // can be skipped.  headmask bit i = edge t + 1024 i starts a run.
  __shared__ int s_last[16][CACHED ? CACHE : 1];
  unsigned long long headmask = 0ull;                           // (up to 64 edges per thread)
  int ascending = 0;
  if (CACHED) {
    const int lane_ = t & 63, wave_ = t >> 6;
    if (lane_ == 63) {
#pragma unroll
      for (int i = 0; i < (CACHED ? CACHE : 1); i++) s_last[wave_][i] = kreg[i];
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const int e = t + 1024 * i;
      int prev = __builtin_amdgcn_update_dpp(0, kreg[i], 0x138, 0xf, 0xf, false);   // wave_shr:1 (lane 0 replaced below)
      if (lane_ == 0) prev = (wave_ > 0) ? s_last[wave_ - 1][i] : (i > 0 ? s_last[15][i > 0 ? i - 1 : 0] : -1);
      if (e < E) {
        ok = ok && kreg[i] >= 0 && (e == 0 || prev <= kreg[i]);
        if (e == 0 || prev != kreg[i]) headmask |= 1ull << i;
      }
    }
    ascending = __syncthreads_and(ok ? 1 : 0);
  } else {
    __syncthreads();
  }
  if (CACHED && ascending) {
    // Segment starts = the run heads, permutation = identity (ascending edge ids inside every patch by construction), and
    // the segment of a head = the number of heads before it: heads per 64-edge chunk (chunk c = 16 i + wave covers edges
    // 64 c .. 64 c + 63) by ballot, one wave scans the <= 512 chunk counts, no flag array / id range needed.
    const int lane_ = t & 63, wave_ = t >> 6;
    constexpr int NCH = 16 * (CACHED ? CACHE : 1);
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const unsigned long long hb = __ballot((headmask >> i) & 1ull);
      if (lane_ == 0) s_part[16 * i + wave_] = __popcll(hb);
    }
    __syncthreads();
    // (the first NCH / 64 waves scan 64 chunk counts each; their totals are combined by every reader)
    constexpr int NW = NCH / 64;
    const int v = (wave_ < NW) ? s_part[t] : 0;
    const int x = wave_inclusive_sum(v);
    if (wave_ < NW && lane_ == 63) s_part[NCH + wave_] = x;
    __syncthreads();
    int carry = 0, n_seg = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) { const int tot = s_part[NCH + w]; if (w < wave_) carry += tot; n_seg += tot; }
    if (wave_ < NW) s_part[t] = carry + x - v;
    __syncthreads();
    if (t == 0) { meta->n_seg = n_seg; meta->fail = 0; meta->pad = 1; meta->sig = sig; }
    int cbase[CACHED ? CACHE : 1];                         // all chunk bases in flight at once, ahead of the divergent stores
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) cbase[i] = s_part[16 * i + wave_];
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const int e = t + 1024 * i;
      const bool head = (headmask >> i) & 1ull;
      const unsigned long long hb = __ballot(head);
      if (e < E) {
        perm_b[e] = e;
        if (head) { const int r = cbase[i] + __popcll(hb & ((1ull << lane_) - 1ull)); g_counts[r] = e; kx[r] = kreg[i]; }
      }
    }
    for (int i = n_seg + t; i <= max_seg; i += 1024) g_counts[i] = E;      // segment n_seg starts at E; empty tails
    return;
  }
  int lo = 0x7fffffff, hi = -1;
#pragma unroll
  for (int i = 0; i < iters; i++) { const int k = patch_of(i); if (k >= 0) { lo = min(lo, k); hi = max(hi, k); } }
  for (int off = 32; off >= 1; off >>= 1) { lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); }
  if ((t & 63) == 0) { atomicMin(&s_min, lo); atomicMax(&s_max, hi); }
  __syncthreads();
  const int kmin = s_min, kmax = s_max;
  const int Rg = (kmax >= kmin) ? kmax - kmin + 1 : 0;
  int* rank = (Rg <= PREP_FLAGS_LDS) ? s_flags : g_rank;
  for (int i = t; i <= Rg; i += 1024) rank[i] = 0;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < iters; i++) { const int k = patch_of(i); if (k >= 0) rank[k - kmin] = 1; }
  __syncthreads();
  const int n_seg = block_excl_scan_1024(rank, Rg, s_part);
  // (sig: the workspace holds a prepared graph once this kernel is through — the in-segment order is restored below)
  if (t == 0) { meta->n_seg = n_seg; meta->fail = 0; meta->pad = ascending; meta->sig = sig; }
  int* counts = (n_seg <= PREP_SEGS_LDS) ? s_counts : g_counts;
  int* cursor = (n_seg <= PREP_SEGS_LDS) ? s_cursor : g_cursor;
  for (int i = t; i <= n_seg; i += 1024) counts[i] = 0;
  for (int i = t; i < n_seg; i += 1024) cursor[i] = 0;
  __syncthreads();
  // Runs of consecutive lanes with the same segment (the edges of a patch are usually adjacent in the edge list) share
  // ONE LDS atomic issued by the first lane of the run — same-address LDS atomics serialise, and this workgroup is the
  // only one running.  (All lanes execute the ballots / shuffles; only the stores are guarded.)
  const int lane = t & 63;
  auto run_of = [&](int key, int& head_lane, int& next_head) {
    const int prev = __shfl_up(key, 1);
    const bool head = (lane == 0) || (prev != key);
    const unsigned long long H = __ballot(head);
    const unsigned long long upto = (2ULL << lane) - 1ULL;            // bits 0..lane (all ones for lane 63)
    head_lane = 63 - __clzll((long long)(H & upto));
    const unsigned long long above = H & ~upto;
    next_head = above ? __ffsll((long long)above) - 1 : 64;
  };
  // segment of every edge (edges with a bad patch id go to segment 0, like before).  CACHED: the run head's atomic
  // RETURNS the run's offset inside its segment, so every edge knows its place before the segment starts exist and the
  // scatter pass needs no second round of atomics.
  int posin[CACHED ? CACHE : 1];
  if (CACHED) {
    // three batched sweeps (LDS reads / shuffles / atomics are each issued back to back for all of a thread's edges —
    // interleaved per edge, every returned LDS atomic would serialise the whole dependent chain behind it)
    // (one packed register per edge besides its segment: 1024 threads leave 128 VGPRs per thread)
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const int k = kreg[i];
      kreg[i] = (t + 1024 * i < E) ? ((k >= 0) ? rank[k - kmin] : 0) : -1;
    }
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      int hl, nh;
      run_of(kreg[i], hl, nh);
      posin[i] = hl | (nh << 8);                               // head lane of my run | lane after its end
    }
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const int hl = posin[i] & 255, nh = posin[i] >> 8;
      int base = 0;
      if (kreg[i] >= 0 && hl == lane) base = atomicAdd(&counts[kreg[i]], nh - lane);   // E < 2^25: fits next to hl
      posin[i] = (base << 6) | hl;
    }
#pragma unroll
    for (int i = 0; i < (CACHED ? CACHE : 1); i++) {
      const int hl = posin[i] & 63;
      posin[i] = __shfl(posin[i] >> 6, hl) + (lane - hl);
    }
  } else {
    for (int i = 0; i < iters; i++) {
      const int e = t + 1024 * i;
      int r = -1;
      if (e < E) { const int k = patch_of(i); r = (k >= 0) ? rank[k - kmin] : 0; ku[e] = r; }   // ku: re-read by the scatter pass
      int hl, nh;
      run_of(r, hl, nh);
      if (r >= 0 && hl == lane) atomicAdd(&counts[r], nh - lane);
    }
  }
  for (int p = t; p < Rg; p += 1024)
    if (rank[p + 1] != rank[p]) kx[rank[p]] = kmin + p;
  __syncthreads();
  block_excl_scan_1024(counts, n_seg, s_part);
#pragma unroll
  for (int i = 0; i < iters; i++) {
    const int e = t + 1024 * i;
    if (CACHED) {
      const int sgm = kreg[i];
      if (sgm >= 0) perm_a[counts[sgm] + posin[i]] = e;
    } else {
      const int sgm = e < E ? ku[e] : -1;
      int hl, nh;
      run_of(sgm, hl, nh);
      int base = 0;
      if (sgm >= 0 && hl == lane) base = atomicAdd(&cursor[sgm], nh - lane);
      base = __shfl(base, hl);
      if (sgm >= 0) perm_a[counts[sgm] + base + (lane - hl)] = e;
    }
  }
  // publish the segment starts: entries beyond n_seg = E so that any reader sees empty tails
  for (int i = t; i <= max_seg; i += 1024) g_counts[i] = (i <= n_seg) ? counts[i] : E;
  // restore a deterministic (ascending edge id) order inside every segment: rank sort, one wave per segment (the work of
  // k_sort_segments, which the multi-kernel path for long edge lists launches)
  __threadfence_block();
  __syncthreads();
  // round 6: two segments per pass, one per half of the wave, the ranks from v_readlane instead of one (L1-hit) load per comparison, the next
  // pass's elements requested before this pass's ranks are counted — DEVO's steady-state graph (45 312 edges in devo.py's order, 2 112 patches of
  // ~21 edges) spent 260 of this kernel's 280 us in the loop below when every comparison was a load
  {
    const int wv16 = t >> 6, half = lane >> 5, l = lane & 31;
    auto fetch = [&](int pair, int& a, int& m, int& x) {
      const int sg = 2 * pair + half;
      a = 0; m = 0;
      if (sg < n_seg) { a = counts[sg]; m = counts[sg + 1] - a; }
      x = (l < m && m <= 32) ? perm_a[a + l] : 0x7fffffff;
    };
    const int npair = (n_seg + 1) >> 1;
    constexpr int SD = 6;                                        // passes whose elements are in flight together (one round trip per SD passes)
    for (int base = wv16; base < npair; base += 16 * SD) {
      int a[SD], m[SD], x[SD];
#pragma unroll
      for (int u = 0; u < SD; u++) {
        a[u] = 0; m[u] = 0; x[u] = 0x7fffffff;
        if (base + 16 * u < npair) fetch(base + 16 * u, a[u], m[u], x[u]);
      }
#pragma unroll
      for (int u = 0; u < SD; u++) {
        const int pair = base + 16 * u;
        if (pair >= npair) break;                                  // (wave-uniform)
        const int mmax = max(__builtin_amdgcn_readlane(m[u], 0), __builtin_amdgcn_readlane(m[u], 32));
        if (mmax <= 32) {
          int r = 0;
          for (int j = 0; j < mmax; j++) {
            const int xa = __builtin_amdgcn_readlane(x[u], j), xb = __builtin_amdgcn_readlane(x[u], 32 + j);     // (j is wave-uniform)
            r += ((half ? xb : xa) < x[u]) ? 1 : 0;
          }
          if (l < m[u]) perm_b[a[u] + r] = x[u];
        } else {
          // a long segment in the pair: the general loop for both (rare: a patch with more than 32 edges)
          for (int h = 0; h < 2; h++) {
            const int sg = 2 * pair + h;
            if (sg >= n_seg) break;
            const int a2 = counts[sg], m2 = counts[sg + 1] - a2;
            for (int i = lane; i < m2; i += 64) {
              const int x2 = perm_a[a2 + i];
              int r = 0;
              for (int jq = 0; jq < m2; jq++) r += (perm_a[a2 + jq] < x2);
              perm_b[a2 + r] = x2;
            }
          }
        }
      }
    }
  }
}

template <int CACHE>
__global__ __launch_bounds__(1024) void k_ba_prepare(const int64_t* __restrict__ kk, int E, int Np, int max_seg, BaMeta* meta,
                                                     int* g_rank, int* g_counts, int* g_cursor, int* ku, int* kx, int* perm_a,
                                                     int* perm_b, int sig) {
  ba_prepare_body<CACHE>(kk, E, Np, max_seg, meta, g_rank, g_counts, g_cursor, ku, kx, perm_a, perm_b, sig);
}

template <int CACHE>
__global__ __launch_bounds__(ORDER_THREADS) void k_order_only(const int* __restrict__ bins, int BE, int nbins, int* __restrict__ order, int starts) {
  corr_order_body<CACHE>(bins, BE, nbins, order, (int)blockIdx.x, (int)gridDim.x, starts != 0);
}

// Workgroup 0: the BA's index preparation; workgroups 1 .. G: the ordering step of the lookup's locality plan (corr_plan.h).
// Latency-bound kernels that do not depend on each other run side by side in one launch.
template <int CACHE>
__global__ __launch_bounds__(1024) void k_prepare_and_order(const int64_t* __restrict__ kk, int E, int Np, int max_seg, BaMeta* meta,
                                                            int* g_rank, int* g_counts, int* g_cursor, int* ku, int* kx, int* perm_a,
                                                            int* perm_b, int sig, const int* __restrict__ bins, int nbins, int* __restrict__ order,
                                                            int starts) {
  if (blockIdx.x == 0) ba_prepare_body<CACHE>(kk, E, Np, max_seg, meta, g_rank, g_counts, g_cursor, ku, kx, perm_a, perm_b, sig);
  else corr_order_body<CACHE>(bins, E, nbins, order, (int)blockIdx.x - 1, (int)gridDim.x - 1, starts != 0);
}

// ------------------------------------------------------------------------------------------------- temporal neighbours (hash grouping)
__device__ __forceinline__ unsigned hash64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return (unsigned)k;
}
__global__ void k_hash_group(const int64_t* __restrict__ ii, int E, unsigned long long* keys, unsigned cap_mask, int* slot_of, int* counts) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    const unsigned long long key = (unsigned long long)ii[e];
    unsigned h = hash64(key) & cap_mask;
    for (;;) {
      unsigned long long prev = atomicCAS(&keys[h], ~0ULL, key);
      if (prev == ~0ULL || prev == key) break;
      h = (h + 1) & cap_mask;
    }
    slot_of[e] = (int)h;
    atomicAdd(&counts[h], 1);
  }
}
// Where every group's edge list starts (round 6): the hash slots' counts become start offsets through ONE atomic per workgroup of 1 024 slots — a bump
// allocator — instead of an exclusive scan of all 2 E slots by a single workgroup (33 of the call's 69 us at 45 312 edges).  Which group lies where in
// `perm` depends on the order of the atomics; what the neighbours kernel reads from it does not.
__global__ __launch_bounds__(1024) void k_group_alloc(int* __restrict__ counts, int cap, int* __restrict__ total) {
  __shared__ int s_w[16];
  __shared__ int s_base;
  const int i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = i < cap ? counts[i] : 0;
  const int inc = wave_inclusive_sum(c);
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < 16; w++) { const int t = s_w[w]; s_w[w] = run; run += t; }
    s_base = run ? atomicAdd(total, run) : 0;
  }
  __syncthreads();
  if (i < cap) counts[i] = s_base + s_w[wave] + inc - c;
}
// ba.cpp:127-139: within the edges that share ii, order by (jj, edge index); previous / next or -1.
__global__ void k_neighbors(const int64_t* __restrict__ jj, int E, const int* __restrict__ slot_of, const int* __restrict__ start,
                            const int* __restrict__ count, const int* __restrict__ perm, int64_t* __restrict__ ix, int64_t* __restrict__ jx) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    const int s = slot_of[e], a = start[s], b = a + count[s];
    const int64_t je = jj[e];
    int64_t pj = 0, nj = 0; int pe = -1, ne = -1;
    for (int q = a; q < b; q++) {
      const int o = perm[q];
      if (o == e) continue;
      const int64_t jo = jj[o];
      const bool less = (jo < je) || (jo == je && o < e);
      if (less) { if (pe < 0 || jo > pj || (jo == pj && o > pe)) { pe = o; pj = jo; } }
      else      { if (ne < 0 || jo < nj || (jo == nj && o < ne)) { ne = o; nj = jo; } }
    }
    ix[e] = pe; jx[e] = ne;
  }
}

static unsigned next_pow2(unsigned v) { unsigned p = 1; while (p < v) p <<= 1; return p; }

// ------------------------------------------------------------------------------------------------- host: preparation
// the single workgroup keeps up to 32 edges per thread in registers; beyond (DEVO's steady-state graph: 45 312 edges) its uncached passes and its
// 16 waves sorting 2 112 segments take 280 us where the multi-kernel path — on the id RANGE — takes 30 (DEVO_BA_PREP_MULTI_FROM: tuning switch)
static bool prep_single_workgroup(int E) {
  static const int multi_from = [] { const char* e = getenv("DEVO_BA_PREP_MULTI_FROM"); return e ? atoi(e) : 32 * 1024 + 1; }();
  return E <= (1 << 17) && E < multi_from;
}

void launch_order_only(hipStream_t st, int E, const PlanRider& r) {
  typedef void (*order_fn_t)(const int*, int, int, int*, int);
  const long long per_thread = ((long long)E + ORDER_THREADS - 1) / ORDER_THREADS;
  order_fn_t order_fn = per_thread <= 8 ? k_order_only<8> : per_thread <= 16 ? k_order_only<16> : per_thread <= 24 ? k_order_only<24> :
                        per_thread <= 32 ? k_order_only<32> : per_thread <= 48 ? k_order_only<48> : per_thread <= 64 ? k_order_only<64> : k_order_only<0>;
  hipLaunchKernelGGL(order_fn, dim3((unsigned)corr_order_workgroups(E, r.nbins)), dim3(ORDER_THREADS), 0, st, r.plan + E + 1, E, r.nbins, r.plan, r.starts);
}

int ba_plan_rider(const char* who, int* plan, int frames, int height, int width, int l1, PlanRider* rider) {
  const CorrPlanGeom pg = corr_plan_geom(1, frames, height);
  DEVO_REQUIRE(pg.nb > 0, "%s: too many frames for a locality plan (%d)", who, frames);
  if (l1 >= 2) {                                              // GROUP plan (devo_corr_order): the bins' first slots go into the plan's tail
    const long long nb = corr_grp_nbins(1, frames, height, width, l1);
    DEVO_REQUIRE(nb > 0, "%s: no group plan for this geometry (%d frames of %d x %d)", who, frames, height, width);
    *rider = PlanRider{plan, (int)nb, 1};
  } else {
    *rider = PlanRider{plan, (int)corr_plan_nbins(1, frames, pg), 0};
  }
  return DEVO_OK;
}

int ba_prepare_impl(const int64_t* kk, int E, int Np, int N, void* ws, size_t ws_bytes, hipStream_t st, PlanRider rider) {
  const BaLayout L = ba_layout(E, Np, N);
  if (ws == nullptr || ws_bytes < L.total) { set_error("devo_ba_prepare: workspace %zu < %zu bytes", ws_bytes, L.total); return DEVO_ERR_WORKSPACE; }
  char* w = (char*)ws;
  BaMeta* meta = (BaMeta*)(w + L.meta);
  int* rank = (int*)(w + L.rank);
  int* counts = (int*)(w + L.counts);
  int* cursor = (int*)(w + L.cursor);
  int* ku = (int*)(w + L.ku);
  int* perm_a = (int*)(w + L.perm_a);
  int* perm_b = (int*)(w + L.perm_b);
  int* kx = (int*)(w + L.kx);
  if (prep_single_workgroup(E)) {
    const size_t prep_lds = sizeof(int) * (1024 + PREP_FLAGS_LDS + 1 + 2 * PREP_SEGS_LDS + 1 + 8);
    static PerDeviceOnce prep_attr;
    if (prep_attr.first()) {
      const void* fns[] = {(const void*)k_ba_prepare<0>, (const void*)k_ba_prepare<8>, (const void*)k_ba_prepare<16>, (const void*)k_ba_prepare<24>,
                           (const void*)k_ba_prepare<32>};
      for (const void* f : fns) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)prep_lds);
      (void)hipGetLastError();
    }
    typedef void (*prep_fn_t)(const int64_t*, int, int, int, BaMeta*, int*, int*, int*, int*, int*, int*, int*, int);
    const int ept = (E + 1023) / 1024;                         // edges per thread
    prep_fn_t prep = ept <= 8 ? k_ba_prepare<8> : ept <= 16 ? k_ba_prepare<16> : ept <= 24 ? k_ba_prepare<24> :
                     ept <= 32 ? k_ba_prepare<32> : k_ba_prepare<0>;
    if (rider.plan && ept <= 32) {
      typedef void (*both_fn_t)(const int64_t*, int, int, int, BaMeta*, int*, int*, int*, int*, int*, int*, int*, int, const int*, int, int*, int);
      both_fn_t both = ept <= 8 ? k_prepare_and_order<8> : ept <= 16 ? k_prepare_and_order<16> : ept <= 24 ? k_prepare_and_order<24> :
                       k_prepare_and_order<32>;
      static PerDeviceOnce both_attr;
      if (both_attr.first()) {
        const void* fns[] = {(const void*)k_prepare_and_order<8>, (const void*)k_prepare_and_order<16>, (const void*)k_prepare_and_order<24>,
                             (const void*)k_prepare_and_order<32>};
        for (const void* f : fns) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)prep_lds);
        (void)hipGetLastError();
      }
      hipLaunchKernelGGL(both, dim3(1 + (unsigned)corr_order_workgroups(E, rider.nbins)), dim3(1024), prep_lds, st, kk, E, Np, L.max_seg, meta, rank,
                         counts, cursor, ku, kx, perm_a, perm_b, ba_sig(E, N), rider.plan + E + 1, rider.nbins, rider.plan, rider.starts);
      rider.plan = nullptr;                                    // done
    } else {
      hipLaunchKernelGGL(prep, dim3(1), dim3(1024), prep_lds, st, kk, E, Np, L.max_seg, meta, rank, counts, cursor, ku, kx, perm_a, perm_b, ba_sig(E, N));
    }
  } else {
    // (meta, rank, counts, cursor are contiguous at the head of the workspace)
    int* range = (int*)(w + L.range);
    if (hipMemsetAsync(w + L.meta, 0, L.ku - L.meta, st) != hipSuccess || hipMemsetAsync(range, 0x80, sizeof(int) * 4, st) != hipSuccess) {
      (void)hipGetLastError(); set_error("devo_ba_prepare: memset failed"); return DEVO_ERR_LAUNCH;
    }
    const int eb = blocks_for(E, 256, 1024);
    hipLaunchKernelGGL(k_kk_range, dim3(blocks_for(E, 256 * 4, 256)), dim3(256), 0, st, kk, E, Np, range);
    hipLaunchKernelGGL(k_flag_ids_r, dim3(eb), dim3(256), 0, st, kk, E, Np, rank, range);
    hipLaunchKernelGGL(k_excl_scan_dev, dim3(1), dim3(1024), 0, st, rank, range, 0, 0, &meta->n_seg);
    hipLaunchKernelGGL(k_rank_edges_r, dim3(eb), dim3(256), 0, st, kk, E, Np, rank, ku, kx, counts, range, &meta->n_seg);
    hipLaunchKernelGGL(k_excl_scan_dev, dim3(1), dim3(1024), 0, st, counts, &meta->n_seg, 1, L.max_seg, (int*)nullptr);
    hipLaunchKernelGGL(k_scatter_edges_seg, dim3(eb), dim3(256), 0, st, ku, E, counts, cursor, perm_a, &meta->n_seg);
    hipLaunchKernelGGL(k_sort_segments, dim3(blocks_for((long long)L.max_seg * 64, 256, 1024)), dim3(256), 0, st, counts, meta, ba_sig(E, N), perm_a, perm_b);
  }
  if (rider.plan) launch_order_only(st, E, rider);            // the plan's ordering step on its own
  return check_launch("devo_ba_prepare");
}

}  // namespace devo

using namespace devo;

extern "C" {
int devo_ba_prepare(const int64_t* kk, int E, int Np, int N, void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && Np > 0 && N >= 0, "devo_ba_prepare: bad sizes");
  if (N > BA_MAXN) { set_error("devo_ba_prepare: %d optimised poses > %d supported", N, BA_MAXN); return DEVO_ERR_UNSUPPORTED; }
  if (E == 0) return DEVO_OK;
  return ba_prepare_impl(kk, E, Np, N, ws, ws_bytes, (hipStream_t)stream);
}

int devo_ba_prepared_tables(const void* ws, size_t ws_bytes, int E, int Np, int N, int* n_seg, int* kx, int* seg_start,
                            int* perm, devo_stream_t stream) {
  DEVO_REQUIRE(E > 0 && Np > 0 && N >= 0 && N <= BA_MAXN, "devo_ba_prepared_tables: bad sizes");
  const BaLayout L = ba_layout(E, Np, N);
  if (ws == nullptr || ws_bytes < L.total) { set_error("devo_ba_prepared_tables: workspace %zu < %zu bytes", ws_bytes, L.total); return DEVO_ERR_WORKSPACE; }
  const char* w = (const char*)ws;
  hipStream_t st = (hipStream_t)stream;
  bool ok = true;
  if (n_seg) ok = ok && hipMemcpyAsync(n_seg, w + L.meta + offsetof(BaMeta, n_seg), sizeof(int), hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (kx) ok = ok && hipMemcpyAsync(kx, w + L.kx, sizeof(int) * (size_t)L.max_seg, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (seg_start) ok = ok && hipMemcpyAsync(seg_start, w + L.counts, sizeof(int) * ((size_t)L.max_seg + 1), hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (perm) ok = ok && hipMemcpyAsync(perm, w + L.perm_b, sizeof(int) * (size_t)E, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); set_error("devo_ba_prepared_tables: copy failed"); return DEVO_ERR_LAUNCH; }
  return DEVO_OK;
}

// The index tables of one kk (n_seg, kx, segment starts, edges grouped by patch) from a workspace prepared for OTHER sizes of the same edge list —
// devo_upd_graph_tables' (Np = its bound, N = 0) — into this one: one launch instead of the preparation's nine.  devo.py:311,337 hand the same
// kk to the Update operator and, right behind it, to the BA.  Ids in [Np, src Np) exist as groups there and count as bad ids here (segment 0 of
// devo_ba_prepare): such a source leaves the destination UNPREPARED (sig 0: the BA reports status -1) instead of different tables.
__global__ __launch_bounds__(256) void k_import_tables(const BaMeta* __restrict__ smeta, const int* __restrict__ scounts, const int* __restrict__ sperm,
                                                       const int* __restrict__ skx, int ssig, BaMeta* __restrict__ dmeta, int* __restrict__ dcounts,
                                                       int* __restrict__ dperm, int* __restrict__ dkx, int E, int Np, int dmax_seg, int dsig) {
  const int n = smeta->n_seg;
  const bool ok = smeta->sig == ssig && n >= 0 && n <= dmax_seg && (n == 0 || skx[n - 1] < Np);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = blockDim.x * gridDim.x;
  if (gid == 0) { dmeta->n_seg = ok ? n : 0; dmeta->fail = 0; dmeta->sig = ok ? dsig : 0; dmeta->pad = ok ? smeta->pad : 0; }   // (pad: "perm is the identity")
  if (!ok) return;
  for (int i = gid; i <= dmax_seg; i += gsz) dcounts[i] = i <= n ? scounts[i] : E;
  for (int i = gid; i < n; i += gsz) dkx[i] = skx[i];
  for (int e = gid; e < E; e += gsz) dperm[e] = sperm[e];
}

int devo_ba_import_tables(const void* src_ws, size_t src_bytes, int src_Np, int src_N, void* ws, size_t ws_bytes, int E, int Np, int N,
                          devo_stream_t stream) {
  DEVO_REQUIRE(E > 0 && Np > 0 && N >= 0 && src_Np > 0 && src_N >= 0, "devo_ba_import_tables: bad sizes");
  if (N > BA_MAXN || src_N > BA_MAXN) { set_error("devo_ba_import_tables: %d / %d optimised poses > %d supported", N, src_N, BA_MAXN); return DEVO_ERR_UNSUPPORTED; }
  const BaLayout S = ba_layout(E, src_Np, src_N), D = ba_layout(E, Np, N);
  if (src_ws == nullptr || src_bytes < S.total) { set_error("devo_ba_import_tables: source workspace %zu < %zu bytes", src_bytes, S.total); return DEVO_ERR_WORKSPACE; }
  if (ws == nullptr || ws_bytes < D.total) { set_error("devo_ba_import_tables: workspace %zu < %zu bytes", ws_bytes, D.total); return DEVO_ERR_WORKSPACE; }
  const char* s = (const char*)src_ws;
  char* d = (char*)ws;
  hipLaunchKernelGGL(k_import_tables, dim3(blocks_for(E, 256, 256)), dim3(256), 0, (hipStream_t)stream, (const BaMeta*)(s + S.meta), (const int*)(s + S.counts),
                     (const int*)(s + S.perm_b), (const int*)(s + S.kx), ba_sig(E, src_N), (BaMeta*)(d + D.meta), (int*)(d + D.counts), (int*)(d + D.perm_b),
                     (int*)(d + D.kx), E, Np, D.max_seg, ba_sig(E, N));
  return check_launch("devo_ba_import_tables");
}

int devo_ba_prepare_plan(const int64_t* kk, int E, int Np, int N, void* ws, size_t ws_bytes, int* plan, int plan_frames,
                         int plan_height, int plan_width, int plan_l1, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && Np > 0 && N >= 0, "devo_ba_prepare_plan: bad sizes");
  if (N > BA_MAXN) { set_error("devo_ba_prepare_plan: %d optimised poses > %d supported", N, BA_MAXN); return DEVO_ERR_UNSUPPORTED; }
  DEVO_REQUIRE(plan != nullptr && plan_frames > 0 && plan_height > 0, "devo_ba_prepare_plan: missing plan");
  if (E == 0) return DEVO_OK;
  PlanRider rider;
  int rc;
  if ((rc = ba_plan_rider("devo_ba_prepare_plan", plan, plan_frames, plan_height, plan_width, plan_l1, &rider))) return rc;
  return ba_prepare_impl(kk, E, Np, N, ws, ws_bytes, (hipStream_t)stream, rider);
}

size_t devo_neighbors_workspace_bytes(int E) {
  if (E <= 0) return 256;
  const size_t cap = next_pow2((unsigned)(2 * (size_t)E));
  return align_up(8 * cap) + align_up(4 * (cap + 1)) + align_up(4 * cap) + 2 * align_up(4 * (size_t)E);
}

int devo_ba_neighbors(const int64_t* ii, const int64_t* jj, int64_t* ix, int64_t* jx, int E, void* ws, size_t ws_bytes,
                      devo_stream_t stream) {
  if (E <= 0) return DEVO_OK;
  const size_t need = devo_neighbors_workspace_bytes(E);
  if (ws == nullptr || ws_bytes < need) { set_error("devo_ba_neighbors: workspace %zu < %zu bytes", ws_bytes, need); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const size_t cap = next_pow2((unsigned)(2 * (size_t)E));
  char* w = (char*)ws;
  unsigned long long* keys = (unsigned long long*)w; w += align_up(8 * cap);
  int* counts = (int*)w; w += align_up(4 * (cap + 1));
  int* cursor = (int*)w; w += align_up(4 * cap);
  int* slot_of = (int*)w; w += align_up(4 * (size_t)E);
  int* perm = (int*)w;
  if (hipMemsetAsync(keys, 0xFF, 8 * cap, st) != hipSuccess ||
      hipMemsetAsync(counts, 0, (char*)slot_of - (char*)counts, st) != hipSuccess) { set_error("devo_ba_neighbors: memset failed"); return DEVO_ERR_LAUNCH; }
  const int eb = blocks_for(E, 256, 1024);
  hipLaunchKernelGGL(k_hash_group, dim3(eb), dim3(256), 0, st, ii, E, keys, (unsigned)(cap - 1), slot_of, counts);
  hipLaunchKernelGGL(k_group_alloc, dim3((unsigned)((cap + 1023) / 1024)), dim3(1024), 0, st, counts, (int)cap, counts + cap);   // (counts[cap]: zeroed above)
  hipLaunchKernelGGL(k_scatter_edges, dim3(eb), dim3(256), 0, st, slot_of, E, counts, cursor, perm);                // (cursor[s] ends as the group's size)
  hipLaunchKernelGGL(k_neighbors, dim3(eb), dim3(256), 0, st, jj, E, slot_of, counts, cursor, perm, ix, jx);
  return check_launch("devo_ba_neighbors");
}

// ---- the Update operator's graph tables in one call (round 6).  DEVO's inference hands the operator NEW ii / jj / kk tensors every frame
// (devo.py:228-231, :304-306), so what devo_amd.update builds per graph — neighbours by patch, groups by patch, groups by frame pair
// (enet.py:86-95) — is per-frame work: as torch ops + three separate preparations it was 250 us of a 1.2 ms frame (nine reductions / elementwise
// kernels for the pair key, a hash grouping for the neighbours that repeats the patch grouping, eight table copies).
// range[0..3] = max(-ii), max(ii), max(-jj), max(jj), all starting at 0x80808080.
__global__ void k_pair_range(const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, int E, int* __restrict__ range) {
  int v[4] = {(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x) {
    const int i = (int)ii[e], j = (int)jj[e];
    v[0] = max(v[0], -i); v[1] = max(v[1], i); v[2] = max(v[2], -j); v[3] = max(v[3], j);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = max(v[c], __shfl_xor(v[c], o));
  __shared__ int s_r[4][4];
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 4; c++) s_r[c][threadIdx.x >> 6] = v[c];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    atomicMax(&range[c], max(max(s_r[c][0], s_r[c][1]), max(s_r[c][2], s_r[c][3])));
  }
}
// key = (ii - min ii) * (max jj - min jj + 1) + (jj - min jj): the groups of ii * 12345 + jj (enet.py:94), keys within (frames in the window)^2
__global__ void k_pair_key(const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, int E, const int* __restrict__ range, int64_t* __restrict__ key) {
  const int imin = -range[0], jmin = -range[2], span = range[3] - jmin + 1;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += blockDim.x * gridDim.x)
    key[e] = (int64_t)((int)ii[e] - imin) * span + ((int)jj[e] - jmin);
}
// cuda_ba.neighbors (ba.cpp:127-139) from the PREPARED tables of the grouping key: one wave per segment, the members' (edge, jj) in the lanes.
__global__ __launch_bounds__(256) void k_neighbors_seg(const int64_t* __restrict__ jj, const BaMeta* __restrict__ meta, const int* __restrict__ seg_start,
                                                       const int* __restrict__ perm, int64_t* __restrict__ ix, int64_t* __restrict__ jx) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (blockDim.x * gridDim.x) >> 6;
  const int n_seg = meta->n_seg;
  for (int s = wave; s < n_seg; s += nwaves) {
    const int a = seg_start[s], m = seg_start[s + 1] - a;
    if (m <= 64) {
      const int e = lane < m ? perm[a + lane] : -1;
      const int je = lane < m ? (int)jj[e] : 0;
      int pj = 0, nj = 0, pe = -1, ne = -1;
      for (int q = 0; q < m; q++) {
        const int o = __builtin_amdgcn_readlane(e, q), jo = __builtin_amdgcn_readlane(je, q);
        if (o == e) continue;
        const bool less = (jo < je) || (jo == je && o < e);
        if (less) { if (pe < 0 || jo > pj || (jo == pj && o > pe)) { pe = o; pj = jo; } }
        else      { if (ne < 0 || jo < nj || (jo == nj && o < ne)) { ne = o; nj = jo; } }
      }
      if (lane < m) { ix[e] = pe; jx[e] = ne; }
    } else {
      for (int i = lane; i < m; i += 64) {
        const int e = perm[a + i];
        const int64_t je = jj[e];
        int64_t pj = 0, nj = 0; int pe = -1, ne = -1;
        for (int q = a; q < a + m; q++) {
          const int o = perm[q];
          if (o == e) continue;
          const int64_t jo = jj[o];
          const bool less = (jo < je) || (jo == je && o < e);
          if (less) { if (pe < 0 || jo > pj || (jo == pj && o > pe)) { pe = o; pj = jo; } }
          else      { if (ne < 0 || jo < nj || (jo == nj && o < ne)) { ne = o; nj = jo; } }
        }
        ix[e] = pe; jx[e] = ne;
      }
    }
  }
}

int devo_ba_table_offsets(int E, int Np, int N, size_t* offsets) {
  DEVO_REQUIRE(E > 0 && Np > 0 && N >= 0 && N <= BA_MAXN && offsets != nullptr, "devo_ba_table_offsets: bad sizes");
  const BaLayout L = ba_layout(E, Np, N);
  offsets[0] = L.meta + offsetof(BaMeta, n_seg);
  offsets[1] = L.kx;
  offsets[2] = L.counts;
  offsets[3] = L.perm_b;
  offsets[4] = (size_t)L.max_seg;
  return DEVO_OK;
}

int devo_upd_graph_tables(const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int bound, void* ws_kk, size_t ws_kk_bytes,
                          void* ws_ij, size_t ws_ij_bytes, int64_t* pair_key, int64_t* ix, int64_t* jx, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && bound > 0, "devo_upd_graph_tables: bad sizes");
  if (E == 0) return DEVO_OK;
  DEVO_REQUIRE(ii && jj && kk && ws_kk && ws_ij && pair_key, "devo_upd_graph_tables: missing argument");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  const BaLayout L = ba_layout(E, bound, 0);
  // beyond the single-workgroup preparation's size (DEVO's steady-state graph: 45 312 edges) both edge lists go through the multi-kernel stages
  // TOGETHER (Prep2): 11 launches for what the two preparations, their fills and the key's range fill did in 22
  static const bool dual_env = [] { const char* e = getenv("DEVO_UPD_TABLES_DUAL"); return !(e && e[0] == '0'); }();
  if (dual_env && !prep_single_workgroup(E)) {
    if (ws_kk_bytes < L.total || ws_ij_bytes < L.total) { set_error("devo_upd_graph_tables: workspace %zu / %zu < %zu bytes", ws_kk_bytes, ws_ij_bytes, L.total); return DEVO_ERR_WORKSPACE; }
    char* w0 = (char*)ws_kk;
    char* w1 = (char*)ws_ij;
    Prep2 p;
    const int64_t* keys[2] = {kk, pair_key};
    char* wsp[2] = {w0, w1};
    for (int y = 0; y < 2; y++) {
      p.kk[y] = keys[y]; p.meta[y] = (BaMeta*)(wsp[y] + L.meta); p.rank[y] = (int*)(wsp[y] + L.rank); p.counts[y] = (int*)(wsp[y] + L.counts);
      p.cursor[y] = (int*)(wsp[y] + L.cursor); p.ku[y] = (int*)(wsp[y] + L.ku); p.kx[y] = (int*)(wsp[y] + L.kx); p.perm_a[y] = (int*)(wsp[y] + L.perm_a);
      p.perm_b[y] = (int*)(wsp[y] + L.perm_b); p.range[y] = (int*)(wsp[y] + L.range);
    }
    int* prange = (int*)(pair_key + E);                             // (the two extra words of the key buffer)
    const long long n4 = (long long)((L.ku - L.meta) / 16);         // (every region of the layout is a multiple of 256 bytes)
    hipLaunchKernelGGL(k_prep_clear2, dim3(blocks_for(n4, 256, 2048)), dim3(256), 0, st, (int4*)(w0 + L.meta), (int4*)(w1 + L.meta), n4, p.range[0], p.range[1], prange);
    hipLaunchKernelGGL(k_pair_range, dim3(blocks_for(E, 256 * 4, 256)), dim3(256), 0, st, ii, jj, E, prange);
    hipLaunchKernelGGL(k_pair_key, dim3(blocks_for(E, 256, 1024)), dim3(256), 0, st, ii, jj, E, prange, pair_key);
    const unsigned eb = (unsigned)blocks_for(E, 256, 1024);
    hipLaunchKernelGGL(k_kk_range2, dim3(blocks_for(E, 256 * 4, 256), 2), dim3(256), 0, st, p, E, bound);
    hipLaunchKernelGGL(k_flag_ids_r2, dim3(eb, 2), dim3(256), 0, st, p, E, bound);
    hipLaunchKernelGGL(k_excl_scan_dev2, dim3(1, 2), dim3(1024), 0, st, p, 0, 0);
    hipLaunchKernelGGL(k_rank_edges_r2, dim3(eb, 2), dim3(256), 0, st, p, E, bound);
    hipLaunchKernelGGL(k_excl_scan_dev2, dim3(1, 2), dim3(1024), 0, st, p, 1, L.max_seg);
    hipLaunchKernelGGL(k_scatter_edges_seg2, dim3(eb, 2), dim3(256), 0, st, p, E);
    hipLaunchKernelGGL(k_sort_segments2, dim3(blocks_for((long long)L.max_seg * 64, 256, 1024), 2), dim3(256), 0, st, p, ba_sig(E, 0));
    if (ix && jx)
      hipLaunchKernelGGL(k_neighbors_seg, dim3(blocks_for((long long)L.max_seg * 64, 256, 1024)), dim3(256), 0, st, jj, (const BaMeta*)(w0 + L.meta),
                         (const int*)(w0 + L.counts), (const int*)(w0 + L.perm_b), ix, jx);
    return check_launch("devo_upd_graph_tables");
  }
  if ((rc = ba_prepare_impl(kk, E, bound, 0, ws_kk, ws_kk_bytes, st))) return rc;
  if (ix && jx) {
    const char* w = (const char*)ws_kk;
    hipLaunchKernelGGL(k_neighbors_seg, dim3(blocks_for((long long)L.max_seg * 64, 256, 1024)), dim3(256), 0, st, jj, (const BaMeta*)(w + L.meta),
                       (const int*)(w + L.counts), (const int*)(w + L.perm_b), ix, jx);
  }
  int* range = (int*)(pair_key + E);                                // (the two extra words of the key buffer)
  if (hipMemsetAsync(range, 0x80, sizeof(int) * 4, st) != hipSuccess) { (void)hipGetLastError(); set_error("devo_upd_graph_tables: memset failed"); return DEVO_ERR_LAUNCH; }
  hipLaunchKernelGGL(k_pair_range, dim3(blocks_for(E, 256 * 4, 256)), dim3(256), 0, st, ii, jj, E, range);
  hipLaunchKernelGGL(k_pair_key, dim3(blocks_for(E, 256, 1024)), dim3(256), 0, st, ii, jj, E, range, pair_key);
  if ((rc = ba_prepare_impl(pair_key, E, bound, 0, ws_ij, ws_ij_bytes, st))) return rc;
  return check_launch("devo_upd_graph_tables");
}

}  // extern "C"
