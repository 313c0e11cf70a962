// Trajectory evaluation on the GPU (what utils/eval_utils.py's ate / ate_real / log_results obtain from evo: association of two stamped
// trajectories, the Umeyama alignment, the absolute trajectory error and its statistics), wave64, gfx950: ONE launch, ONE workgroup of 256
// threads per pair of trajectories, all arithmetic in fp64.  The passes of a workgroup:
//   0. the pair's extents against the totals, the stamps' range (|s| < 2^53, finite) and the order of the long stamps.
//   1. association in chunks of 256 short poses: a binary search to the leftmost long stamp >= the short one, the nearer neighbour (the
//      lower on a tie, the leftmost of equal stamps), the test against max_diff — or, interpolating, the bracket and the interpolated pose;
//      the kept matches are compacted in short order (ballot + prefix counts) into the workspace: short index, long index, (pose).  The
//      sums of the matched positions go along.
//   2. Sigma, sigma_x^2 over the matches; the path length over the whole ground truth.
//   3. thread 0: the 3 x 3 one-sided Jacobi SVD (loss.hip's nuclear_norm3 iteration, here with V kept and U formed), the rank rule, the
//      reflection correction, R, c, t; broadcast through LDS.
//   4. the errors (to the workspace), their sums, min, max, the rotation angles, the relative pose errors.
//   5. the second pass of the standard deviation, and the median: a radix select over the order-preserving 64-bit image of the errors, 8-bit
//      digits, an LDS histogram with integer atomics, both middle ranks in the same sweeps.
// Every reduction is per-thread strided partials, then wave shuffles, then LDS across the four waves, in a fixed order: no floating-point
// atomics, bit-reproducible, independent of B.  Vector stores only.
// The algebra, the reductions, the select (block_median), the match accessor (Matches) and the workspace layout (eval_ws) are traj_dev.h's,
// shared with traj_rel.hip, whose launches read the matches this one leaves in its workspace.
#include "traj_dev.h"

namespace {

using namespace devo;
using namespace devo::traj;

constexpr double RANK_RULE = 1e-10;            // sigma_2 <= RANK_RULE * sigma_1: degenerate
constexpr double STAMP_LIMIT = 9007199254740992.0;   // 2^53

struct EvalArgs {
  const void* est; const void* est_t; const int64_t* est_off; long long total_est;
  const void* gt; const void* gt_t; const int64_t* gt_off; long long total_gt;
  int assoc, align, rpe_delta;
  double max_diff;
  int* mi; int* mj; double* err; double* ipose;
  double* stats; double* transform; int* status; double* errors_out; int* matched_out;
};

// The SVD of a 3 x 3 matrix by a one-sided Jacobi iteration (Hestenes) on its columns — loss.hip's nuclear_norm3 with V kept: a V = (u_q
// sigma_q).  On return the columns of a and v are sorted by decreasing norm, sig holds the norms.
__device__ void jacobi_svd3(double a[3][3], double v[3][3], double sig[3]) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) v[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int k = 0; k < 3; k++) { alpha += a[k][p] * a[k][p]; beta += a[k][q] * a[k][q]; gamma += a[k][p] * a[k][q]; }
        const double bound = 1e-17 * sqrt(alpha * beta);
        if (!(fabs(gamma) > bound) || gamma == 0.0) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int k = 0; k < 3; k++) {
          const double u = a[k][p], w = a[k][q];
          a[k][p] = cs * u - sn * w;
          a[k][q] = sn * u + cs * w;
          const double vu = v[k][p], vw = v[k][q];
          v[k][p] = cs * vu - sn * vw;
          v[k][q] = sn * vu + cs * vw;
        }
      }
    if (!rotated) break;
  }
  for (int q = 0; q < 3; q++) {
    const double n2 = a[0][q] * a[0][q] + a[1][q] * a[1][q] + a[2][q] * a[2][q];
    sig[q] = sqrt(n2 > 0.0 ? n2 : 0.0);
  }
  for (int pass = 0; pass < 2; pass++)                               // a three-element bubble sort of the columns, descending
    for (int q = 0; q < 2 - pass; q++)
      if (sig[q] < sig[q + 1]) {
        const double s = sig[q]; sig[q] = sig[q + 1]; sig[q + 1] = s;
        for (int k = 0; k < 3; k++) {
          const double t = a[k][q]; a[k][q] = a[k][q + 1]; a[k][q + 1] = t;
          const double w = v[k][q]; v[k][q] = v[k][q + 1]; v[k][q + 1] = w;
        }
      }
}

// a rotation matrix (row-major) as a unit quaternion with w >= 0: the largest of the four diagonal forms
__device__ Q4 quat_of(const double R[9]) {
  const double tr = R[0] + R[4] + R[8];
  Q4 q;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    q = {(R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s, 0.25 * s};
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
    q = {0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s, (R[7] - R[5]) / s};
  } else if (R[4] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
    q = {(R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s, (R[2] - R[6]) / s};
  } else {
    const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
    q = {(R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s, (R[3] - R[1]) / s};
  }
  const double r = (q.w < 0.0 ? -1.0 : 1.0) / sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return {q.x * r, q.y * r, q.z * r, q.w * r};
}

// the leftmost index in [0, n) whose stamp is >= s (n if there is none)
template <typename S>
__device__ __forceinline__ int lower_bound(const S* __restrict__ t, int n, double s) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)t[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <typename T, typename S>
__global__ __launch_bounds__(TB) void k_traj_eval(const EvalArgs a) {
  __shared__ double sh_red[WAVES][MAXR];
  __shared__ int sh_cnt[WAVES];
  __shared__ double sh_tf[20];                                       // R (9), c, t (3), q (4), flag
  __shared__ SelectLds sh_sel;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double* __restrict__ row = a.stats + (long long)b * DEVO_TRAJ_EVAL_COLS;
  double* __restrict__ tf = a.transform + (long long)b * 8;

  // the row of a flagged pair (every thread takes the same branch: `flags` is uniform wherever this is called)
  auto give_up = [&](int flags, int n) {
    if (tid == 0) {
      row[0] = (double)n;
      for (int c = 1; c < DEVO_TRAJ_EVAL_COLS; c++) row[c] = qnan;
      for (int c = 0; c < 8; c++) tf[c] = qnan;
      a.status[b] = flags;
    }
  };

  const long long eo = a.est_off[b], e1 = a.est_off[b + 1], go = a.gt_off[b], g1 = a.gt_off[b + 1];
  if (eo < 0 || e1 < eo || e1 > a.total_est || go < 0 || g1 < go || g1 > a.total_gt) { give_up(DEVO_TRAJ_BAD_OFFSETS, 0); return; }
  const long long ne_l = e1 - eo, ng_l = g1 - go;
  const bool interp = a.assoc == DEVO_TRAJ_ASSOC_INTERPOLATE;
  const bool est_short = interp || ne_l < ng_l;                      // (equal length: the ground truth is the short one)
  const long long ns_l = est_short ? ne_l : ng_l, nl_l = est_short ? ng_l : ne_l;
  const int ne = (int)(ne_l < 0x7fffffff ? ne_l : 0x7fffffff);
  if (a.errors_out)
    for (int i = tid; i < ne; i += TB) a.errors_out[eo + i] = qnan;
  if (a.matched_out)
    for (int i = tid; i < ne; i += TB) a.matched_out[eo + i] = -1;
  if (ns_l > DEVO_TRAJ_EVAL_MAX_MATCHES || nl_l > 0x7fffffff || ne_l > 0x7fffffff) { give_up(DEVO_TRAJ_TOO_LONG, 0); return; }
  const int ns = (int)ns_l, nl = (int)nl_l, ng = (int)ng_l;
  const T* __restrict__ est = static_cast<const T*>(a.est) + 7 * eo;
  const T* __restrict__ gt = static_cast<const T*>(a.gt) + 7 * go;
  const S* __restrict__ est_t = static_cast<const S*>(a.est_t) + eo;
  const S* __restrict__ gt_t = static_cast<const S*>(a.gt_t) + go;
  const S* __restrict__ st = est_short ? est_t : gt_t;
  const S* __restrict__ lt = est_short ? gt_t : est_t;
  int* __restrict__ mi = a.mi + eo;                                  // (ns <= ne: the pair's share of the workspace is its estimate's rows)
  int* __restrict__ mj = a.mj + eo;
  double* __restrict__ err = a.err + eo;
  double* __restrict__ ipose = interp ? a.ipose + 7 * eo : nullptr;

  // ---- pass 0: the stamps
  {
    int bad = 0;
    for (int i = tid; i < ns; i += TB) {
      const double s = (double)st[i];
      if (!(fabs(s) < STAMP_LIMIT)) bad |= DEVO_TRAJ_STAMP_RANGE;
    }
    for (int j = tid; j < nl; j += TB) {
      const double s = (double)lt[j];
      if (!(fabs(s) < STAMP_LIMIT)) bad |= DEVO_TRAJ_STAMP_RANGE;
      if (j + 1 < nl && !(s <= (double)lt[j + 1])) bad |= DEVO_TRAJ_UNSORTED;
    }
    const int range = __syncthreads_or(bad & DEVO_TRAJ_STAMP_RANGE), order = __syncthreads_or(bad & DEVO_TRAJ_UNSORTED);
    const int flags = (range ? DEVO_TRAJ_STAMP_RANGE : 0) | (order ? DEVO_TRAJ_UNSORTED : 0);
    if (flags) { give_up(flags, 0); return; }
  }

  // the estimate's and the ground truth's position and rotation of match k (the matches are read back through the pointers that write them)
  const Matches<T> M(est, gt, mi, mj, ipose, est_short, interp);

  // ---- pass 1: association, compaction, the sums of the matched positions
  int n = 0;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int base = 0; base < ns; base += TB) {
    const int i = base + tid;
    bool keep = false;
    int j = -1;
    double alpha = 0.0;
    if (i < ns && nl > 0) {
      const double s = (double)st[i];
      const int lo = lower_bound(lt, nl, s);
      if (interp) {
        if (s >= (double)lt[0] && s <= (double)lt[nl - 1]) {         // (then lo < nl)
          keep = true;
          const double hi_t = (double)lt[lo];
          if (hi_t == s) {
            j = lo;
          } else {                                                   // lt[lo - 1] < s < lt[lo]
            j = lo - 1;
            const double lo_t = (double)lt[j];
            alpha = (s - lo_t) / (hi_t - lo_t);
          }
        }
      } else {
        double d = 0.0;
        if (lo < nl) { j = lo; d = (double)lt[lo] - s; }
        if (lo > 0) {
          const double below = (double)lt[lo - 1], dl = s - below;
          if (lo == nl || dl <= d) { j = lower_bound(lt, lo, below); d = dl; }
        }
        keep = d <= a.max_diff;
      }
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) sh_cnt[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
      const int c = sh_cnt[w];
      before += w < wv ? c : 0;
      total += c;
    }
    if (keep) {
      const int k = n + before + __popcll(bal & ((1ull << lane) - 1ull));
      mi[k] = i;
      mj[k] = j;
      if (a.matched_out) a.matched_out[eo + i] = j;
      V3 y;
      if (interp) {
        const V3 p0 = load_pos(gt, j);
        Q4 q = load_quat(gt, j);
        y = p0;
        if (alpha > 0.0) {
          const V3 p1 = load_pos(gt, j + 1);
          Q4 q1 = load_quat(gt, j + 1);
          y = p0 + alpha * (p1 - p0);
          double d = q.x * q1.x + q.y * q1.y + q.z * q1.z + q.w * q1.w;
          if (d < 0.0) { q1 = {-q1.x, -q1.y, -q1.z, -q1.w}; d = -d; }                  // the shorter arc
          const Q4 v = {q1.x - d * q.x, q1.y - d * q.y, q1.z - d * q.z, q1.w - d * q.w};   // the part of q1 orthogonal to q
          const double sn = sqrt(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
          if (sn > 1e-12) {                                                              // (identical neighbours: q stays)
            const double th = alpha * atan2(sn, d), cq = cos(th), sq = sin(th) / sn;
            q = {cq * q.x + sq * v.x, cq * q.y + sq * v.y, cq * q.z + sq * v.z, cq * q.w + sq * v.w};
            const double r = 1.0 / sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
            q = {q.x * r, q.y * r, q.z * r, q.w * r};
          }
        }
        double* __restrict__ o = ipose + 7 * (long long)k;
        o[0] = y.x; o[1] = y.y; o[2] = y.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
      } else {
        y = load_pos(gt, est_short ? j : i);
      }
      const V3 x = load_pos(est, est_short ? i : j);
      acc[0] += x.x; acc[1] += x.y; acc[2] += x.z; acc[3] += y.x; acc[4] += y.y; acc[5] += y.z;
    }
    n += total;
    __syncthreads();                                                 // (sh_cnt is rewritten by the next chunk)
  }
  block_sum(acc, sh_red);                                            // (its barriers also publish mi, mj, ipose to the workgroup)
  const bool aligning = a.align != DEVO_TRAJ_ALIGN_NONE;
  if (n == 0) { give_up(DEVO_TRAJ_NO_MATCH, 0); return; }
  if (aligning && n < 3) { give_up(DEVO_TRAJ_TOO_FEW, n); return; }
  const double inv_n = 1.0 / (double)n;
  const V3 mx = {acc[0] * inv_n, acc[1] * inv_n, acc[2] * inv_n}, my = {acc[3] * inv_n, acc[4] * inv_n, acc[5] * inv_n};

  // ---- pass 2: Sigma (row-major, y rows, x columns), sigma_x^2, the ground truth's path length
  double cov[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (aligning)
    for (int k = tid; k < n; k += TB) {
      const V3 dx = M.x(k) - mx, dy = M.y(k) - my;
      cov[0] += dy.x * dx.x; cov[1] += dy.x * dx.y; cov[2] += dy.x * dx.z;
      cov[3] += dy.y * dx.x; cov[4] += dy.y * dx.y; cov[5] += dy.y * dx.z;
      cov[6] += dy.z * dx.x; cov[7] += dy.z * dx.y; cov[8] += dy.z * dx.z;
      cov[9] += dot(dx, dx);
    }
  for (int j = tid; j + 1 < ng; j += TB) cov[10] += norm(load_pos(gt, j + 1) - load_pos(gt, j));
  block_sum(cov, sh_red);
  const double path = cov[10];

  // ---- pass 3: R, c, t
  if (tid == 0) {
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, c = 1.0, flag = 0.0;
    V3 t = {0.0, 0.0, 0.0};
    if (aligning) {
      double A[3][3], V[3][3], sig[3];
      for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) A[r][q] = cov[3 * r + q] * inv_n;
      const double var_x = cov[9] * inv_n;
      jacobi_svd3(A, V, sig);
      if (!(sig[1] > RANK_RULE * sig[0])) {
        flag = 1.0;
      } else {
        const V3 a0 = {A[0][0], A[1][0], A[2][0]}, a1 = {A[0][1], A[1][1], A[2][1]}, a2 = {A[0][2], A[1][2], A[2][2]};
        const V3 v0 = {V[0][0], V[1][0], V[2][0]}, v1 = {V[0][1], V[1][1], V[2][1]}, v2 = {V[0][2], V[1][2], V[2][2]};
        const V3 u0 = (1.0 / sig[0]) * a0;
        V3 u1 = (1.0 / sig[1]) * a1;
        u1 = u1 - dot(u0, u1) * u0;                                  // (orthogonal to working precision already: one clean-up step)
        u1 = (1.0 / norm(u1)) * u1;
        const V3 u2 = cross(u0, u1), w2 = cross(v0, v1);             // the completed third vectors: det [u0 u1 u2] = det [v0 v1 w2] = +1
        // sign(det U det V) of the decomposition itself: u2 and w2 against the iteration's third columns (sigma_3 = 0: no term to sign)
        const double su = dot(u2, a2), sv = dot(w2, v2);
        const double s = (su < 0.0) != (sv < 0.0) ? -1.0 : 1.0;
        // U S V^T = u0 v0^T + u1 v1^T + (u2 w2^T with both completed by cross products: the sign is in them)
        const V3 U[3] = {u0, u1, u2}, W[3] = {v0, v1, w2};
        for (int q = 0; q < 9; q++) R[q] = 0.0;
        for (int m = 0; m < 3; m++) {
          R[0] += U[m].x * W[m].x; R[1] += U[m].x * W[m].y; R[2] += U[m].x * W[m].z;
          R[3] += U[m].y * W[m].x; R[4] += U[m].y * W[m].y; R[5] += U[m].y * W[m].z;
          R[6] += U[m].z * W[m].x; R[7] += U[m].z * W[m].y; R[8] += U[m].z * W[m].z;
        }
        if (a.align == DEVO_TRAJ_ALIGN_SIM3) c = (sig[0] + sig[1] + s * sig[2]) / var_x;
        const V3 rm = {R[0] * mx.x + R[1] * mx.y + R[2] * mx.z, R[3] * mx.x + R[4] * mx.y + R[5] * mx.z, R[6] * mx.x + R[7] * mx.y + R[8] * mx.z};
        t = my - c * rm;
      }
    }
    const Q4 q = quat_of(R);
    for (int m = 0; m < 9; m++) sh_tf[m] = R[m];
    sh_tf[9] = c; sh_tf[10] = t.x; sh_tf[11] = t.y; sh_tf[12] = t.z;
    sh_tf[13] = q.x; sh_tf[14] = q.y; sh_tf[15] = q.z; sh_tf[16] = q.w; sh_tf[17] = flag;
  }
  __syncthreads();
  if (sh_tf[17] != 0.0) { give_up(DEVO_TRAJ_DEGENERATE, n); return; }
  double R[9];
#pragma unroll
  for (int m = 0; m < 9; m++) R[m] = sh_tf[m];
  const double c = sh_tf[9];
  const V3 t = {sh_tf[10], sh_tf[11], sh_tf[12]};
  const Q4 qR = {sh_tf[13], sh_tf[14], sh_tf[15], sh_tf[16]};

  // ---- pass 4: the errors, the rotation angles, the relative pose errors
  // 0 sum e, 1 sum e^2, 2 sum angle, 3 sum angle^2, 4 sum |rpe t|^2, 5 sum rpe angle^2
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double lo = __longlong_as_double(0x7ff0000000000000ll), hi = -lo;
  const int delta = a.rpe_delta;
  const bool rpe = delta > 0 && delta < n;
  for (int k = tid; k < n; k += TB) {
    const V3 x = M.x(k), y = M.y(k);
    const V3 rx = {R[0] * x.x + R[1] * x.y + R[2] * x.z, R[3] * x.x + R[4] * x.y + R[5] * x.z, R[6] * x.x + R[7] * x.y + R[8] * x.z};
    const double e = norm(y - (c * rx + t));
    err[k] = e;
    if (a.errors_out) a.errors_out[eo + mi[k]] = e;
    sums[0] += e; sums[1] += e * e;
    lo = fmin(lo, e); hi = fmax(hi, e);
    const Q4 qx = M.qx(k), qy = M.qy(k);
    const double ang = qangle_deg(qmul(qconj(qy), qmul(qR, qx)));
    sums[2] += ang; sums[3] += ang * ang;
    if (rpe && k + delta < n) {
      const Q4 qx2 = M.qx(k + delta), qy2 = M.qy(k + delta);
      const V3 tp = qrot(qconj(qx), c * (M.x(k + delta) - x));   // P_k^-1 P_k+d
      const Q4 qp = qmul(qconj(qx), qx2);
      const V3 tq = qrot(qconj(qy), M.y(k + delta) - y);         // Q_k^-1 Q_k+d
      const Q4 qq = qmul(qconj(qy), qy2);
      const V3 te = qrot(qconj(qq), tp - tq);
      const double ae = qangle_deg(qmul(qconj(qq), qp));
      sums[4] += dot(te, te); sums[5] += ae * ae;
    }
  }
  block_sum(sums, sh_red);                                           // (its barriers also publish err)
  block_minmax(lo, hi, sh_red);
  const double mean = sums[0] * inv_n;

  // ---- pass 5: the standard deviation's second pass; the median
  double dev[1] = {0.0};
  bool nan = false;
  for (int k = tid; k < n; k += TB) {
    const double e = err[k];
    nan |= e != e;
    dev[0] += (e - mean) * (e - mean);
  }
  block_sum(dev, sh_red);
  const int any_nan = __syncthreads_or(nan ? 1 : 0);
  const double med = block_median<1, false>(err, nullptr, n, n, sh_sel);

  if (tid == 0) {
    const bool bad = sums[1] != sums[1];
    const double median = any_nan ? qnan : med;
    const int terms = rpe ? n - delta : 0;
    row[0] = (double)n;
    row[1] = sqrt(sums[1] * inv_n);
    row[2] = mean;
    row[3] = median;
    row[4] = sqrt(dev[0] * inv_n);
    row[5] = bad ? qnan : lo;
    row[6] = bad ? qnan : hi;
    row[7] = sums[1];
    row[8] = sqrt(sums[3] * inv_n);
    row[9] = sums[2] * inv_n;
    row[10] = path;
    row[11] = 100.0 * mean / path;
    row[12] = c;
    row[13] = rpe ? sqrt(sums[4] / (double)terms) : qnan;
    row[14] = rpe ? sqrt(sums[5] / (double)terms) : qnan;
    row[15] = (double)terms;
    tf[0] = c; tf[1] = t.x; tf[2] = t.y; tf[3] = t.z; tf[4] = qR.x; tf[5] = qR.y; tf[6] = qR.z; tf[7] = qR.w;
    a.status[b] = 0;
  }
}

}  // namespace

extern "C" size_t devo_traj_eval_workspace_bytes(int64_t total_est, int assoc) { return eval_ws(total_est, assoc).total; }

extern "C" int devo_traj_eval(const void* est, const void* est_stamps, const int64_t* est_off, int64_t total_est, const void* gt, const void* gt_stamps,
                              const int64_t* gt_off, int64_t total_gt, int B, int pose_dtype, int stamps_f64, int assoc, int align, double max_diff,
                              int rpe_delta, double* stats, double* transform, int* status, double* errors_out, int* matched_out, void* ws, size_t ws_bytes,
                              devo_stream_t stream) {
  DEVO_REQUIRE(B >= 1 && total_est >= 0 && total_gt >= 0, "traj_eval: B >= 1 and totals >= 0 expected (B %d, %lld estimated, %lld ground-truth poses)", B,
               (long long)total_est, (long long)total_gt);
  DEVO_REQUIRE(est_off && gt_off && stats && transform && status && ws, "traj_eval: null tensor");
  DEVO_REQUIRE((total_est == 0 || (est && est_stamps)) && (total_gt == 0 || (gt && gt_stamps)), "traj_eval: null poses or stamps");
  DEVO_REQUIRE(pose_dtype == DEVO_F32 || pose_dtype == DEVO_F64, "traj_eval: poses must be fp32 or fp64 (dtype code %d)", pose_dtype);
  DEVO_REQUIRE(assoc == DEVO_TRAJ_ASSOC_NEAREST || assoc == DEVO_TRAJ_ASSOC_INTERPOLATE, "traj_eval: unknown association %d", assoc);
  DEVO_REQUIRE(align >= DEVO_TRAJ_ALIGN_NONE && align <= DEVO_TRAJ_ALIGN_SIM3, "traj_eval: unknown alignment %d", align);
  DEVO_REQUIRE(assoc == DEVO_TRAJ_ASSOC_INTERPOLATE || max_diff >= 0.0, "traj_eval: max_diff must be >= 0 (a NaN is refused too)");
  DEVO_REQUIRE(rpe_delta >= 0, "traj_eval: rpe_delta %d", rpe_delta);
  const EvalWs L = eval_ws(total_est, assoc);
  if (ws_bytes < L.total || ((uintptr_t)ws & 15)) {
    set_error("traj_eval: workspace of %zu bytes at %p (%zu needed, 16-byte aligned)", ws_bytes, ws, L.total);
    return DEVO_ERR_WORKSPACE;
  }
  EvalArgs a;
  a.est = est; a.est_t = est_stamps; a.est_off = est_off; a.total_est = total_est;
  a.gt = gt; a.gt_t = gt_stamps; a.gt_off = gt_off; a.total_gt = total_gt;
  a.assoc = assoc; a.align = align; a.rpe_delta = rpe_delta; a.max_diff = max_diff;
  char* w = static_cast<char*>(ws);
  a.mi = reinterpret_cast<int*>(w + L.mi); a.mj = reinterpret_cast<int*>(w + L.mj);
  a.err = reinterpret_cast<double*>(w + L.err); a.ipose = reinterpret_cast<double*>(w + L.ipose);
  a.stats = stats; a.transform = transform; a.status = status; a.errors_out = errors_out; a.matched_out = matched_out;
  const hipStream_t s = (hipStream_t)stream;
  if (pose_dtype == DEVO_F32) {
    if (stamps_f64) hipLaunchKernelGGL((k_traj_eval<float, double>), dim3(B), dim3(TB), 0, s, a);
    else hipLaunchKernelGGL((k_traj_eval<float, int64_t>), dim3(B), dim3(TB), 0, s, a);
  } else {
    if (stamps_f64) hipLaunchKernelGGL((k_traj_eval<double, double>), dim3(B), dim3(TB), 0, s, a);
    else hipLaunchKernelGGL((k_traj_eval<double, int64_t>), dim3(B), dim3(TB), 0, s, a);
  }
  return check_launch("traj_eval");
}
