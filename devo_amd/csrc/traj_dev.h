// What the trajectory kernels share (traj_eval.hip: association, alignment, ATE; traj_rel.hip: relative pose error), wave64, gfx950, fp64:
// the vector / quaternion algebra, the pose loads, the workgroup reductions (fixed order, no floating-point atomics), the order-preserving
// 64-bit image of a double and the median by a radix select over it, the accessor "match k -> pose" over the evaluation launch's compacted
// matches, and (host) the layout of that launch's workspace, which traj_rel.hip reads.  Workgroups of TB = 256 threads throughout.
// One copy of each; what the move did to the two files' device code and results is recorded in profiles/traj_dev.txt.
#pragma once
#include "common.h"
#include <math.h>

namespace devo {
namespace traj {

constexpr int TB = 256;
constexpr int WAVES = TB / 64;
constexpr int MAXR = 12;                       // values one reduction carries

struct V3 { double x, y, z; };
struct Q4 { double x, y, z, w; };

__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(dot(a, a)); }

__device__ __forceinline__ Q4 qconj(Q4 q) { return {-q.x, -q.y, -q.z, q.w}; }
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
// the rotation of a unit quaternion applied to v: v + 2 w (u x v) + 2 u x (u x v)
__device__ __forceinline__ V3 qrot(Q4 q, V3 v) {
  const V3 u = {q.x, q.y, q.z};
  const V3 c = cross(u, v);
  return v + 2.0 * (q.w * c + cross(u, c));
}
// the angle of a unit quaternion's rotation in [0, pi]: well conditioned at 0 and at pi, unlike arccos of the trace
__device__ __forceinline__ double qangle_rad(Q4 q) { return 2.0 * atan2(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), fabs(q.w)); }
__device__ __forceinline__ double qangle_deg(Q4 q) { return qangle_rad(q) * (180.0 / 3.14159265358979323846); }

template <typename T> __device__ __forceinline__ V3 load_pos(const T* __restrict__ p, long long i) {
  return {(double)p[7 * i], (double)p[7 * i + 1], (double)p[7 * i + 2]};
}
template <typename T> __device__ __forceinline__ Q4 load_quat(const T* __restrict__ p, long long i) {
  const double x = (double)p[7 * i + 3], y = (double)p[7 * i + 4], z = (double)p[7 * i + 5], w = (double)p[7 * i + 6];
  const double r = 1.0 / sqrt(x * x + y * y + z * z + w * w);
  return {x * r, y * r, z * r, w * r};
}

// K sums over the workgroup, every thread gets them: shuffles inside a wave, then the four waves' values added in order
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*sh)[MAXR]) {
  static_assert(K <= MAXR, "block_sum: too many values");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
  }
  __syncthreads();                                                   // (the previous reduction's values have been read)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[wv][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double r = sh[0][k];
#pragma unroll
    for (int w = 1; w < WAVES; w++) r += sh[w][k];
    v[k] = r;
  }
}

// min and max alike (fmin / fmax skip a NaN; the caller sets both to NaN when the sums are)
__device__ __forceinline__ void block_minmax(double& lo, double& hi, double (*sh)[MAXR]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_down(lo, o, 64));
    hi = fmax(hi, __shfl_down(hi, o, 64));
  }
  __syncthreads();
  if (lane == 0) { sh[wv][0] = lo; sh[wv][1] = hi; }
  __syncthreads();
  lo = sh[0][0]; hi = sh[0][1];
#pragma unroll
  for (int w = 1; w < WAVES; w++) { lo = fmin(lo, sh[w][0]); hi = fmax(hi, sh[w][1]); }
}

// fp64 -> u64 whose unsigned order is the order of the doubles, and back
__device__ __forceinline__ unsigned long long dkey(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dkey_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct SelectLds {
  unsigned hist[2][256];
  unsigned long long prefix[2];
  unsigned rank[2];
};

// numpy's median of the m values v[STRIDE k], k < n (m >= 1) — MASKED: of those whose ends[k] >= 0; else ends is not read and m = n: a radix
// select, 8-bit digits, an LDS histogram with integer atomics, both middle ranks in the same sweeps.  Every thread gets the result.
template <int STRIDE, bool MASKED>
__device__ __forceinline__ double block_median(const double* __restrict__ v, const int* __restrict__ ends, int n, int m, SelectLds& s) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  __syncthreads();                                                   // (the previous select's result has been read)
  if (tid == 0) {
    s.prefix[0] = s.prefix[1] = 0ull;
    s.rank[0] = (unsigned)((m - 1) / 2); s.rank[1] = (unsigned)(m / 2);
  }
  s.hist[0][tid] = 0u; s.hist[1][tid] = 0u;
  __syncthreads();
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 56 - 8 * pass;
    const unsigned long long p0 = s.prefix[0], p1 = s.prefix[1];
    const unsigned long long mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    for (int k = tid; k < n; k += TB) {
      if (MASKED && ends[k] < 0) continue;
      const unsigned long long key = dkey(v[STRIDE * (long long)k]);
      const unsigned digit = (unsigned)(key >> shift) & 255u;
      if ((key & mask) == p0) atomicAdd(&s.hist[0][digit], 1u);
      if ((key & mask) == p1) atomicAdd(&s.hist[1][digit], 1u);
    }
    __syncthreads();
    if (tid < 128) {                                                 // waves 0 and 1: one rank each, lane l owns bins 4 l .. 4 l + 3
      const int r = wv;
      const unsigned h0 = s.hist[r][4 * lane], h1 = s.hist[r][4 * lane + 1], h2 = s.hist[r][4 * lane + 2], h3 = s.hist[r][4 * lane + 3];
      const unsigned sum = h0 + h1 + h2 + h3;
      unsigned incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      const unsigned rank = s.rank[r];
      unsigned excl = incl - sum;
      if (excl <= rank && rank < incl) {                             // exactly one lane
        unsigned bin = 4u * lane;
        if (rank >= excl + h0) { excl += h0; bin++; if (rank >= excl + h1) { excl += h1; bin++; if (rank >= excl + h2) { excl += h2; bin++; } } }
        s.prefix[r] = (r == 0 ? p0 : p1) | ((unsigned long long)bin << shift);
        s.rank[r] = rank - excl;
      }
    }
    __syncthreads();
    s.hist[0][tid] = 0u; s.hist[1][tid] = 0u;
    __syncthreads();
  }
  return 0.5 * (dkey_value(s.prefix[0]) + dkey_value(s.prefix[1]));
}

// what a kernel knows of pair b's matches, as the evaluation launch compacts them: match k is the estimate's pose ie(k) and the ground truth's
// pose mj[k] / mi[k] (or, interpolating, the pose k of ipose)
template <typename T>
struct Matches {
  const T* est; const T* gt; const int* mi; const int* mj; const double* ipose;
  bool est_short, interp;
  // from a launch's argument block (est, gt, est_off, gt_off, assoc, mi, mj, ipose: whole-batch pointers) and the pair
  template <typename A>
  __device__ __forceinline__ Matches(const A& a, int b) {
    const long long eo = a.est_off[b], e1 = a.est_off[b + 1], go = a.gt_off[b], g1 = a.gt_off[b + 1];
    interp = a.assoc == DEVO_TRAJ_ASSOC_INTERPOLATE;
    est_short = interp || (e1 - eo) < (g1 - go);
    est = static_cast<const T*>(a.est) + 7 * eo;
    gt = static_cast<const T*>(a.gt) + 7 * go;
    mi = a.mi + eo; mj = a.mj + eo;
    ipose = interp ? a.ipose + 7 * eo : nullptr;
  }
  // from the pair's own pointers (the evaluation kernel: it writes the matches through them and reads them back through these)
  __device__ __forceinline__ Matches(const T* est, const T* gt, const int* mi, const int* mj, const double* ipose, bool est_short, bool interp)
      : est(est), gt(gt), mi(mi), mj(mj), ipose(ipose), est_short(est_short), interp(interp) {}
  __device__ __forceinline__ int ie(int k) const { return est_short ? mi[k] : mj[k]; }
  __device__ __forceinline__ V3 x(int k) const { return load_pos(est, ie(k)); }
  __device__ __forceinline__ Q4 qx(int k) const { return load_quat(est, ie(k)); }
  __device__ __forceinline__ V3 y(int k) const {
    if (interp) return V3{ipose[7 * (long long)k], ipose[7 * (long long)k + 1], ipose[7 * (long long)k + 2]};
    return load_pos(gt, est_short ? mj[k] : mi[k]);
  }
  __device__ __forceinline__ Q4 qy(int k) const {
    if (interp) return Q4{ipose[7 * (long long)k + 3], ipose[7 * (long long)k + 4], ipose[7 * (long long)k + 5], ipose[7 * (long long)k + 6]};
    return load_quat(gt, est_short ? mj[k] : mi[k]);
  }
};

// devo_traj_eval's workspace: the compacted matches (short index, long index), the errors, the interpolated poses; byte offsets, each
// aligned.  devo_traj_rel_eval reads the matches a launch left there through the same offsets.
struct EvalWs { size_t mi, mj, err, ipose, total; };
inline EvalWs eval_ws(int64_t total_est, int assoc) {
  EvalWs L;
  const size_t n = total_est > 0 ? (size_t)total_est : 0;
  size_t o = 0;
  L.mi = o; o += align_up(n * sizeof(int));
  L.mj = o; o += align_up(n * sizeof(int));
  L.err = o; o += align_up(n * sizeof(double));
  L.ipose = o; o += assoc == DEVO_TRAJ_ASSOC_INTERPOLATE ? align_up(n * 7 * sizeof(double)) : 0;
  L.total = o > 0 ? o : 256;
  return L;
}

}  // namespace traj
}  // namespace devo
