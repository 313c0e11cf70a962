// The patch-graph bookkeeping that closes every frame of DEVO's inference (devo/devo.py:225-239 append_factors / remove_factors,
// :258-265 motionmag, :267-306 keyframe) on the GPU, wave64, gfx950.
//   * k_motion_partials / k_motion_final: the keyframe motion test.  One pass over ALL edges, no compaction: an edge selects itself by
//     (ii == i & jj == j) or the reverse and evaluates pops.flow_mag on its P x P pixels (the arithmetic of the fused transform,
//     transform.hip k_transform: quaternions renormalised on load, Z clamped at 0.1 in proj, identity rotation for `tonly`).  Sums and counts
//     per direction: shuffle wave sums, one fp32 partial per workgroup, the partials added in fp64 in a fixed order by one workgroup.
//     No float atomics: the means are reproducible from run to run.  A direction without an edge yields 0 / 0 = NaN.
//   * k_compact_count / k_compact_scatter: a STABLE stream compaction of ii, jj, kk and the rows of net.  The keyframe decision
//     (double(mean_ij) + double(mean_ji)) / 2 < thresh is read from the device: if it holds, edges of frame k are dropped and the
//     survivors renumbered in the same pass, then the removal-window rule is applied to the renumbered edge.  Per-wave counts from a
//     64-bit ballot + popcount, per-workgroup offsets from the sum of the workgroup counts in front; rows of net move as 16-byte words.
//     The last workgroup writes {removed, n_edges, mean_ij, mean_ji} into a host-visible record: the caller waits once, for that.
//   * k_append: index tails written in place (ii = ix[patch_ids] gathered here) and the new net (old rows copied, new rows zero).
//   * k_append_frame: the same for the window edges of a new frame (devo.py:366-380, :541-542), whose patch and frame ids are computed
//     from (M, n, lifetime) instead of read: both append_factors calls of a frame in one launch, no index lists built on the host.
//   * k_shift_frames: rows k+1 .. n-1 of up to 8 tensors, addressed as byte rows, move down by one.  A thread owns a column chunk and
//     walks the rows in ascending order: it has read row r + 1 before it overwrites it, and nobody else touches its columns.
// Nothing here synchronises with the host.
#include <algorithm>
#include "common.h"
#include "se3_dev.h"

namespace {

using namespace devo;

constexpr int TB = 256;                     // 4 waves of 64
constexpr int WAVES = TB / 64;

struct Decision { int removed; int n_edges; float mean_ij; float mean_ji; };      // == the host record (DEVO_GRAPH_RECORD_BYTES)
struct MotionPartial { float s0, s1; int c0, c1; };
static_assert(sizeof(Decision) == DEVO_GRAPH_RECORD_BYTES, "record layout");

inline int tiles(int E) { return E > 0 ? (E + TB - 1) / TB : 1; }

// workspace: Decision | MotionPartial[nb] | int counts[nb], nb = tiles(capacity)
inline size_t ws_partials() { return align_up(sizeof(Decision)); }
inline size_t ws_counts(int nb) { return ws_partials() + align_up((size_t)nb * sizeof(MotionPartial)); }
inline size_t ws_total(int nb) { return ws_counts(nb) + align_up((size_t)nb * sizeof(int)); }

__device__ __forceinline__ void project(const SE3<float>& G, V3<float> X0, float w, float fx, float fy, float cx, float cy, float& u, float& v) {
  const V3<float> X1 = qrot(G.q, X0) + w * G.t;
  const float d = 1.0f / fmaxf(X1.z, 0.1f);
  u = fx * (d * X1.x) + cx;
  v = fy * (d * X1.y) + cy;
}

// sum over the P x P pixels of  beta |full - c0| + (1 - beta) |tonly - c0|   (projective_ops.py:111-121)
__device__ __forceinline__ float edge_flow(const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ intr,
                                           int64_t fi, int64_t fj, int64_t k, int PP, float beta) {
  const SE3<float> Gi = SE3<float>::load(poses + fi * 7), Gj = SE3<float>::load(poses + fj * 7);
  const SE3<float> Ginv = Gi.inv();
  const SE3<float> G = Gj.mul(Ginv), G0 = Gi.mul(Ginv);           // (c0 = transform(ii, ii): Gi * Gi^-1 as the kernel forms it, not the exact identity)
  SE3<float> Gt = G;
  Gt.q = Q4<float>{0.0f, 0.0f, 0.0f, 1.0f};
  const float fxi = intr[fi * 4], fyi = intr[fi * 4 + 1], cxi = intr[fi * 4 + 2], cyi = intr[fi * 4 + 3];
  const float fxj = intr[fj * 4], fyj = intr[fj * 4 + 1], cxj = intr[fj * 4 + 2], cyj = intr[fj * 4 + 3];
  const float* pk = patches + k * 3 * PP;
  float s = 0.0f;
  for (int p = 0; p < PP; p++) {
    const float w = pk[2 * PP + p];
    const V3<float> X0{(pk[p] - cxi) / fxi, (pk[PP + p] - cyi) / fyi, 1.0f};
    float u0, v0, u1, v1, u2, v2;
    project(G0, X0, w, fxi, fyi, cxi, cyi, u0, v0);
    project(G, X0, w, fxj, fyj, cxj, cyj, u1, v1);
    project(Gt, X0, w, fxj, fyj, cxj, cyj, u2, v2);
    const float full = sqrtf((u1 - u0) * (u1 - u0) + (v1 - v0) * (v1 - v0));
    const float trans = sqrtf((u2 - u0) * (u2 - u0) + (v2 - v0) * (v2 - v0));
    s += beta * full + (1.0f - beta) * trans;
  }
  return s;
}

__global__ __launch_bounds__(TB) void k_motion_partials(const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ intr,
                                                        const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, const int64_t* __restrict__ kk,
                                                        int E, int n_poses, int n_patches, int PP, int i, int j, float beta,
                                                        MotionPartial* __restrict__ part) {
  const int e = blockIdx.x * TB + threadIdx.x;
  float s0 = 0.0f, s1 = 0.0f;
  int c0 = 0, c1 = 0;
  if (e < E) {
    const int64_t a = ii[e], b = jj[e];
    const bool d0 = a == i && b == j, d1 = a == j && b == i;
    if (d0 || d1) {
      const int64_t k = kk[e];
      if (a >= 0 && a < n_poses && b >= 0 && b < n_poses && k >= 0 && k < n_patches) {
        const float v = edge_flow(poses, patches, intr, a, b, k, PP, beta);
        if (d0) { s0 = v; c0 = 1; }
        if (d1) { s1 = v; c1 = 1; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_down(s0, o, 64);
    s1 += __shfl_down(s1, o, 64);
    c0 += __shfl_down(c0, o, 64);
    c1 += __shfl_down(c1, o, 64);
  }
  __shared__ MotionPartial sh[WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = MotionPartial{s0, s1, c0, c1};
  __syncthreads();
  if (threadIdx.x == 0) {
    MotionPartial r = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) { r.s0 += sh[w].s0; r.s1 += sh[w].s1; r.c0 += sh[w].c0; r.c1 += sh[w].c1; }
    part[blockIdx.x] = r;
  }
}

// one workgroup: the partials in fp64, in an order that depends on nb alone; the decision as devo.py:272-274 takes it
__global__ __launch_bounds__(TB) void k_motion_final(const MotionPartial* __restrict__ part, int nb, int PP, double thresh, int E,
                                                     Decision* __restrict__ dec, Decision* __restrict__ record) {
  double s0 = 0.0, s1 = 0.0;
  long long c0 = 0, c1 = 0;
  for (int b = threadIdx.x; b < nb; b += TB) { s0 += (double)part[b].s0; s1 += (double)part[b].s1; c0 += part[b].c0; c1 += part[b].c1; }
  __shared__ double sh_s[2][TB];
  __shared__ long long sh_c[2][TB];
  sh_s[0][threadIdx.x] = s0; sh_s[1][threadIdx.x] = s1; sh_c[0][threadIdx.x] = c0; sh_c[1][threadIdx.x] = c1;
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh_s[0][threadIdx.x] += sh_s[0][threadIdx.x + o]; sh_s[1][threadIdx.x] += sh_s[1][threadIdx.x + o];
      sh_c[0][threadIdx.x] += sh_c[0][threadIdx.x + o]; sh_c[1][threadIdx.x] += sh_c[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Decision d;
    d.mean_ij = (float)(sh_s[0][0] / ((double)sh_c[0][0] * PP));        // 0 / 0: NaN, as mean() of an empty tensor
    d.mean_ji = (float)(sh_s[1][0] / ((double)sh_c[1][0] * PP));
    const double m = (double)d.mean_ij + (double)d.mean_ji;
    d.removed = (m / 2 < thresh) ? 1 : 0;                                // NaN: false
    d.n_edges = E;
    *dec = d;
    if (record) *record = d;
  }
}

struct Rule {
  const unsigned char* mask;       // a caller's mask (remove()): nothing else applies
  const int64_t* ix;
  int64_t ix_len;
  int k, M, n, window;
};

// does edge (a, b, c) survive?  Renumbers it in place when frame k goes (devo.py:282-287), then the window rule (:305) on the new numbers.
__device__ __forceinline__ bool survivor(const Rule& r, bool removed, int e, int64_t& a, int64_t& b, int64_t& c) {
  if (r.mask) return r.mask[e] == 0;
  int n = r.n;
  if (removed) {
    if (a == r.k || b == r.k) return false;
    if (a > r.k) { c -= r.M; a -= 1; }
    if (b > r.k) b -= 1;
    n -= 1;
  }
  if (c < 0 || c >= r.ix_len) return true;                               // (a patch index outside ix is never read: the edge stays)
  return !(r.ix[c] < (int64_t)(n - r.window));
}

__global__ __launch_bounds__(TB) void k_compact_count(const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, const int64_t* __restrict__ kk, int E,
                                                      Rule rule, const Decision* __restrict__ dec, int* __restrict__ counts) {
  const int e = blockIdx.x * TB + threadIdx.x;
  const bool removed = !rule.mask && dec->removed != 0;
  bool keep = false;
  if (e < E) {
    int64_t a = ii[e], b = jj[e], c = kk[e];
    keep = survivor(rule, removed, e, a, b, c);
  }
  const unsigned long long bal = __ballot(keep);
  __shared__ int sh[WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += sh[w];
    counts[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(TB) void k_compact_scatter(const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, const int64_t* __restrict__ kk,
                                                        const uint4* __restrict__ net, int E, int cpr, Rule rule, Decision* __restrict__ dec,
                                                        const int* __restrict__ counts, int64_t* __restrict__ ii_out, int64_t* __restrict__ jj_out,
                                                        int64_t* __restrict__ kk_out, uint4* __restrict__ net_out, Decision* __restrict__ record) {
  __shared__ int sh_wave[WAVES];
  __shared__ int sh_off[WAVES];
  __shared__ int sh_src[TB];
  // this workgroup's offset: the counts of the workgroups in front
  int part = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += TB) part += counts[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
  if ((threadIdx.x & 63) == 0) sh_off[threadIdx.x >> 6] = part;

  const int e = blockIdx.x * TB + threadIdx.x;
  const bool removed = !rule.mask && dec->removed != 0;
  bool keep = false;
  int64_t a = 0, b = 0, c = 0;
  if (e < E) {
    a = ii[e]; b = jj[e]; c = kk[e];
    keep = survivor(rule, removed, e, a, b, c);
  }
  const unsigned long long bal = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh_wave[wave] = __popcll(bal);
  __syncthreads();
  int offset = 0, before = 0, kept = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) { offset += sh_off[w]; if (w < wave) before += sh_wave[w]; kept += sh_wave[w]; }
  const int rank = before + __popcll(bal & ((1ull << lane) - 1ull));
  if (keep) {
    const int64_t d = (int64_t)offset + rank;
    ii_out[d] = a; jj_out[d] = b; kk_out[d] = c;
    sh_src[rank] = threadIdx.x;
  }
  __syncthreads();
  // rows of net: the kept rows of this tile, 16 bytes per lane
  const int64_t src0 = (int64_t)blockIdx.x * TB;
  for (int t = threadIdx.x; t < kept * cpr; t += TB) {
    const int r = t / cpr, col = t - r * cpr;
    net_out[((int64_t)offset + r) * cpr + col] = net[(src0 + sh_src[r]) * cpr + col];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    Decision d = *dec;
    if (rule.mask) { d.removed = 0; d.mean_ij = 0.0f; d.mean_ji = 0.0f; }
    d.n_edges = offset + kept;
    *record = d;
  }
}

__global__ __launch_bounds__(TB) void k_append(int64_t* __restrict__ ii, int64_t* __restrict__ jj, int64_t* __restrict__ kk, const uint4* __restrict__ net_old,
                                               uint4* __restrict__ net_new, const int64_t* __restrict__ ix, int64_t ix_len,
                                               const int64_t* __restrict__ patch_ids, const int64_t* __restrict__ frame_ids, int E, int n_new, int cpr) {
  const int64_t stride = (int64_t)gridDim.x * TB, t0 = (int64_t)blockIdx.x * TB + threadIdx.x;
  for (int64_t t = t0; t < n_new; t += stride) {
    const int64_t p = patch_ids[t];
    kk[E + t] = p;
    jj[E + t] = frame_ids[t];
    ii[E + t] = (p >= 0 && p < ix_len) ? ix[p] : -1;                     // (a patch outside ix: frame -1, nothing is read out of bounds)
  }
  const int64_t n_old = (int64_t)E * cpr, n_all = ((int64_t)E + n_new) * cpr;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int64_t t = t0; t < n_all; t += stride) net_new[t] = t < n_old ? net_old[t] : zero;
}

// the window edges of frame n - 1 (devo.py:366-380, :541-542), generated here instead of read from index lists: n_fwd forward edges
// (patch p0 + t -> frame n - 1), then the backward edges of the newest M patches, patch-major over the frames f0 .. n - 1
struct FrameEdges { int n_fwd, n_new, p0, pb0, f0, nf, last; };

inline FrameEdges frame_edges(int M, int n, int lifetime) {
  const int f0 = std::max(n - lifetime, 0), nf = n - f0;
  const long long n_fwd = (long long)M * (n - 1 - std::min(f0, n - 1)), n_new = n_fwd + (long long)M * nf;
  return FrameEdges{(int)n_fwd, (int)n_new, M * std::min(f0, n - 1), M * (n - 1), f0, nf, n - 1};
}

__global__ __launch_bounds__(TB) void k_append_frame(int64_t* __restrict__ ii, int64_t* __restrict__ jj, int64_t* __restrict__ kk, const uint4* __restrict__ net_old,
                                                     uint4* __restrict__ net_new, const int64_t* __restrict__ ix, int64_t ix_len, FrameEdges e, int E, int cpr) {
  const int64_t stride = (int64_t)gridDim.x * TB, t0 = (int64_t)blockIdx.x * TB + threadIdx.x;
  for (int64_t t = t0; t < e.n_new; t += stride) {
    int64_t p, f;
    if (t < e.n_fwd) { p = e.p0 + t; f = e.last; }
    else { const int64_t b = t - e.n_fwd, q = b / e.nf; p = e.pb0 + q; f = e.f0 + (b - q * e.nf); }
    kk[E + t] = p;
    jj[E + t] = f;
    ii[E + t] = p < ix_len ? ix[p] : -1;
  }
  const int64_t n_old = (int64_t)E * cpr, n_all = ((int64_t)E + e.n_new) * cpr;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int64_t t = t0; t < n_all; t += stride) net_new[t] = t < n_old ? net_old[t] : zero;
}

constexpr int SHIFT_MAX = DEVO_GRAPH_SHIFT_MAX;
struct ShiftArgs { unsigned char* p[SHIFT_MAX]; long long row_bytes[SHIFT_MAX]; long long first[SHIFT_MAX + 1]; int width[SHIFT_MAX]; int count; };

template <typename W>
__device__ __forceinline__ void shift_column(unsigned char* base, long long rb, int k, int n) {
  for (int r = k; r < n - 1; r++) *(W*)(base + (long long)r * rb) = *(const W*)(base + (long long)(r + 1) * rb);
}

__global__ __launch_bounds__(TB) void k_shift_frames(ShiftArgs a, int k, int n) {
  const long long total = a.first[a.count];
  for (long long t = (long long)blockIdx.x * TB + threadIdx.x; t < total; t += (long long)gridDim.x * TB) {
    int s = 0;
    while (s + 1 < a.count && t >= a.first[s + 1]) s++;
    const int w = a.width[s];
    unsigned char* base = a.p[s] + (t - a.first[s]) * w;
    const long long rb = a.row_bytes[s];
    if (w == 16) shift_column<uint4>(base, rb, k, n);
    else if (w == 8) shift_column<uint2>(base, rb, k, n);
    else if (w == 4) shift_column<unsigned>(base, rb, k, n);
    else if (w == 2) shift_column<unsigned short>(base, rb, k, n);
    else shift_column<unsigned char>(base, rb, k, n);
  }
}

int elem_bytes(int dtype) { return dtype == DEVO_F16 ? 2 : dtype == DEVO_F32 ? 4 : 0; }

int check_net(const char* what, const void* net, const void* net_out, int dim, int dtype, int* cpr) {
  const int eb = elem_bytes(dtype);
  DEVO_REQUIRE(eb != 0, "%s: net must be fp16 or fp32", what);
  DEVO_REQUIRE(dim > 0 && dim % 8 == 0, "%s: dim must be a positive multiple of 8 (rows move as 16-byte words), got %d", what, dim);
  DEVO_REQUIRE(((uintptr_t)net & 15) == 0 && ((uintptr_t)net_out & 15) == 0, "%s: net must be 16-byte aligned", what);
  *cpr = dim * eb / 16;
  return DEVO_OK;
}

int launch_compaction(const char* what, const int64_t* ii, const int64_t* jj, const int64_t* kk, const void* net, int64_t* ii_out, int64_t* jj_out,
                      int64_t* kk_out, void* net_out, int E, int cpr, const Rule& rule, void* ws, void* record, hipStream_t st) {
  DEVO_REQUIRE(E == 0 || (ii_out != ii && jj_out != jj && kk_out != kk && net_out != net), "%s: the outputs must not alias the inputs", what);
  const int nb = tiles(E);
  Decision* dec = (Decision*)ws;
  int* counts = (int*)((char*)ws + ws_counts(nb));
  hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(TB), 0, st, ii, jj, kk, E, rule, dec, counts);
  hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(TB), 0, st, ii, jj, kk, (const uint4*)net, E, cpr, rule, dec, counts, ii_out, jj_out, kk_out,
                     (uint4*)net_out, (Decision*)record);
  return check_launch(what);
}

int launch_motion(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                  int n_poses, int n_patches, int P, int i, int j, float beta, double thresh, void* ws, void* record, hipStream_t st) {
  const int nb = tiles(E);
  MotionPartial* part = (MotionPartial*)((char*)ws + ws_partials());
  hipLaunchKernelGGL(k_motion_partials, dim3(nb), dim3(TB), 0, st, poses, patches, intrinsics, ii, jj, kk, E, n_poses, n_patches, P * P, i, j, beta, part);
  hipLaunchKernelGGL(k_motion_final, dim3(1), dim3(TB), 0, st, part, nb, P * P, thresh, E, (Decision*)ws, (Decision*)record);
  return DEVO_OK;
}

}  // namespace

extern "C" {

size_t devo_graph_workspace_bytes(int capacity) { return capacity < 0 ? 0 : ws_total(tiles(capacity)); }

int devo_graph_motion(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                      int n_poses, int n_patches, int P, int i, int j, float beta, void* ws, size_t ws_bytes, void* record, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && n_poses > 0 && n_patches >= 0 && P > 0, "devo_graph_motion: bad sizes");
  DEVO_REQUIRE(ws && ws_bytes >= ws_total(tiles(E)), "devo_graph_motion: workspace too small");
  DEVO_REQUIRE(record, "devo_graph_motion: no record");
  launch_motion(poses, patches, intrinsics, ii, jj, kk, E, n_poses, n_patches, P, i, j, beta, 0.0, ws, record, (hipStream_t)stream);
  return check_launch("devo_graph_motion");
}

int devo_graph_keyframe(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii, const int64_t* jj, const int64_t* kk,
                        const void* net, const int64_t* ix, int64_t* ii_out, int64_t* jj_out, int64_t* kk_out, void* net_out, int E, int n_poses,
                        int n_patches, int64_t ix_len, int P, int dim, int net_dtype, int M, int n, int keyframe_index, double thresh,
                        int removal_window, float beta, void* ws, size_t ws_bytes, void* record, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && n_poses > 0 && n_patches >= 0 && P > 0 && ix_len >= 0 && M > 0, "devo_graph_keyframe: bad sizes");
  DEVO_REQUIRE(ws && ws_bytes >= ws_total(tiles(E)), "devo_graph_keyframe: workspace too small");
  DEVO_REQUIRE(record, "devo_graph_keyframe: no record");
  int cpr = 0;
  if (int rc = check_net("devo_graph_keyframe", net, net_out, dim, net_dtype, &cpr)) return rc;
  const int k = n - keyframe_index;
  launch_motion(poses, patches, intrinsics, ii, jj, kk, E, n_poses, n_patches, P, k - 1, k + 1, beta, thresh, ws, nullptr, (hipStream_t)stream);
  const Rule rule{nullptr, ix, ix_len, k, M, n, removal_window};
  return launch_compaction("devo_graph_keyframe", ii, jj, kk, net, ii_out, jj_out, kk_out, net_out, E, cpr, rule, ws, record, (hipStream_t)stream);
}

int devo_graph_remove(const int64_t* ii, const int64_t* jj, const int64_t* kk, const void* net, const unsigned char* mask, int64_t* ii_out,
                      int64_t* jj_out, int64_t* kk_out, void* net_out, int E, int dim, int net_dtype, void* ws, size_t ws_bytes, void* record,
                      devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && mask, "devo_graph_remove: bad arguments");
  DEVO_REQUIRE(ws && ws_bytes >= ws_total(tiles(E)), "devo_graph_remove: workspace too small");
  DEVO_REQUIRE(record, "devo_graph_remove: no record");
  int cpr = 0;
  if (int rc = check_net("devo_graph_remove", net, net_out, dim, net_dtype, &cpr)) return rc;
  const Rule rule{mask, nullptr, 0, 0, 0, 0, 0};
  return launch_compaction("devo_graph_remove", ii, jj, kk, net, ii_out, jj_out, kk_out, net_out, E, cpr, rule, ws, record, (hipStream_t)stream);
}

int devo_graph_append(int64_t* ii, int64_t* jj, int64_t* kk, const void* net_old, void* net_new, const int64_t* ix, int64_t ix_len,
                      const int64_t* patch_ids, const int64_t* frame_ids, int E, int n_new, int capacity, int dim, int net_dtype, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && n_new >= 0 && ix_len >= 0, "devo_graph_append: bad sizes");
  DEVO_REQUIRE((long long)E + n_new <= capacity, "devo_graph_append: %d + %d edges exceed the capacity %d", E, n_new, capacity);
  int cpr = 0;
  if (int rc = check_net("devo_graph_append", net_old, net_new, dim, net_dtype, &cpr)) return rc;
  if (E + n_new == 0) return DEVO_OK;
  const long long work = std::max<long long>(((long long)E + n_new) * cpr, n_new);
  hipLaunchKernelGGL(k_append, dim3(blocks_for(work, TB, 8192)), dim3(TB), 0, (hipStream_t)stream, ii, jj, kk, (const uint4*)net_old, (uint4*)net_new, ix,
                     ix_len, patch_ids, frame_ids, E, n_new, cpr);
  return check_launch("devo_graph_append");
}

int64_t devo_odom_append_frame_edges(int M, int n, int lifetime) {
  if (M <= 0 || n < 1 || lifetime < 1) return 0;
  const long long f0 = std::max(n - lifetime, 0);
  return (long long)M * (n - 1 - f0) + (long long)M * (n - f0);
}

int devo_odom_append_frame(int64_t* ii, int64_t* jj, int64_t* kk, const void* net_old, void* net_new, const int64_t* ix, int64_t ix_len, int M, int n,
                            int lifetime, int E, int capacity, int dim, int net_dtype, devo_stream_t stream) {
  DEVO_REQUIRE(E >= 0 && ix_len >= 0 && M > 0, "devo_odom_append_frame: bad sizes");
  DEVO_REQUIRE(n >= 1 && lifetime >= 1, "devo_odom_append_frame: a state of n = %d frames with a patch lifetime of %d has no window edges", n, lifetime);
  DEVO_REQUIRE((long long)M * n <= INT32_MAX, "devo_odom_append_frame: more than 2^31 patches");
  const long long n_new = devo_odom_append_frame_edges(M, n, lifetime);
  DEVO_REQUIRE(E + n_new <= capacity, "devo_odom_append_frame: %d + %lld edges exceed the capacity %d", E, n_new, capacity);
  DEVO_REQUIRE(ii && jj && kk && ix, "devo_odom_append_frame: null buffers");
  int cpr = 0;
  if (int rc = check_net("devo_odom_append_frame", net_old, net_new, dim, net_dtype, &cpr)) return rc;
  const long long work = std::max<long long>((E + n_new) * cpr, n_new);
  hipLaunchKernelGGL(k_append_frame, dim3(blocks_for(work, TB, 8192)), dim3(TB), 0, (hipStream_t)stream, ii, jj, kk, (const uint4*)net_old, (uint4*)net_new, ix,
                     ix_len, frame_edges(M, n, lifetime), E, cpr);
  return check_launch("devo_odom_append_frame");
}

int devo_graph_shift_frames(void* const* tensors, const int64_t* row_bytes, int count, int k, int n, devo_stream_t stream) {
  DEVO_REQUIRE(count >= 0 && count <= SHIFT_MAX, "devo_graph_shift_frames: at most %d tensors to a call, got %d", SHIFT_MAX, count);
  DEVO_REQUIRE(k >= 0 && n >= 0, "devo_graph_shift_frames: bad rows (k = %d, n = %d)", k, n);
  if (count == 0 || k >= n - 1) return DEVO_OK;
  ShiftArgs a;
  a.count = count;
  a.first[0] = 0;
  for (int s = 0; s < count; s++) {
    DEVO_REQUIRE(tensors[s] && row_bytes[s] > 0, "devo_graph_shift_frames: tensor %d is empty", s);
    int w = 16;
    while (w > 1 && (((uintptr_t)tensors[s] | (uintptr_t)row_bytes[s]) & (uintptr_t)(w - 1))) w >>= 1;
    a.p[s] = (unsigned char*)tensors[s];
    a.row_bytes[s] = row_bytes[s];
    a.width[s] = w;
    a.first[s + 1] = a.first[s] + row_bytes[s] / w;
  }
  for (int s = count; s < SHIFT_MAX; s++) { a.p[s] = nullptr; a.row_bytes[s] = 0; a.width[s] = 1; a.first[s + 1] = a.first[count]; }
  hipLaunchKernelGGL(k_shift_frames, dim3(blocks_for(a.first[count], TB, 4096)), dim3(TB), 0, (hipStream_t)stream, a, k, n);
  return check_launch("devo_graph_shift_frames");
}

}  // extern "C"
