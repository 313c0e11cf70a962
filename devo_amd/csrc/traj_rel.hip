// Relative pose error on the GPU (what the reference's scripts/evaluate_rpe.py and the "rel stats" of utils/eval_utils.py:log_results report:
// the drift over sub-trajectories of a given length in frames, seconds, metres, radians or degrees), wave64, gfx950, all arithmetic in fp64.
// devo_traj_rel_eval runs devo_traj_eval first (association, and the Umeyama scale when it is asked for): that launch leaves the compacted
// matches in its workspace (mi, mj, the interpolated poses) and the scale in `transform`.  Two launches follow:
//   prepare, ONE workgroup of 256 per pair: the index u_k of every match (k, the estimate's stamp, or the cumulative path length / rotation
//      angle along the matched ground-truth or estimated poses) as a workgroup scan — per-thread serial chunks, an inclusive scan of the chunk
//      sums by wave shuffles, the four waves in order through LDS — its order for stamps, its range, the pair's scale.
//   errors, ONE workgroup of 256 per (pair, delta): a binary search for the end j of the sub-trajectory that starts at i ("reach": the first
//      j > i with u_j - u_i >= delta; "closest": the j nearest to u_i + delta, the lowest on a tie, dropped when j = n - 1), the error
//      E = (c . (X_i^-1 X_j))^-1 (Y_i^-1 Y_j) of every start, the sums, min, max, the second pass of the standard deviations, and both
//      medians by a radix select over the order-preserving 64-bit image of the errors.
// Every reduction is per-thread strided partials, then wave shuffles, then LDS across the four waves, in a fixed order: no floating-point
// atomics, bit-reproducible, independent of B and D.  Vector stores only.
// The algebra, the reductions, the select and the evaluation launch's workspace layout are traj_dev.h's, shared with traj_eval.hip.
#include "traj_dev.h"

namespace {

using namespace devo;
using namespace devo::traj;

constexpr int META = 4;                        // per pair: n, c, u_{n-1} - u_0, flags

struct RelArgs {
  const void* est; const void* est_t; const int64_t* est_off; long long total_est;
  const void* gt; const int64_t* gt_off; long long total_gt;
  int assoc, unit, relative, along, end, scale_mode, D;
  double scale; const double* scale_v;
  double deltas[DEVO_TRAJ_REL_MAX_DELTAS];
  const int* mi; const int* mj; const double* ipose;                 // the evaluation launch's workspace
  const double* ev_stats; const double* ev_tf; const int* ev_status; // and its outputs
  double* u; double* meta;
  double* err2; int* ends;                                           // [D, total_est, 2], [D, total_est]: the outputs when asked for, else workspace
  double* stats; int* status;
};

// the leftmost index in [0, n) whose value is >= s (n if there is none)
__device__ __forceinline__ int lower_bound(const double* __restrict__ u, int n, double s) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- prepare: one workgroup per pair
template <typename T, typename S>
__global__ __launch_bounds__(TB) void k_traj_rel_prepare(const RelArgs a) {
  __shared__ double sh_wave[WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double* __restrict__ meta = a.meta + (long long)b * META;
  // (every thread takes the same branch: the flags are uniform)
  auto give_up = [&](int flags) {
    if (tid == 0) { meta[0] = 0.0; meta[1] = qnan; meta[2] = qnan; meta[3] = (double)flags; }
  };
  const int ev = a.ev_status[b];
  if (ev) { give_up(ev); return; }
  const int n = (int)a.ev_stats[(long long)b * DEVO_TRAJ_EVAL_COLS];  // 1 <= n <= DEVO_TRAJ_EVAL_MAX_MATCHES and <= the estimate's rows
  if (n < 2) { give_up(DEVO_TRAJ_TOO_FEW); return; }
  const double c = a.scale_mode == DEVO_TRAJ_REL_SCALE_SIM3 ? a.ev_tf[(long long)b * 8] : a.scale_mode == DEVO_TRAJ_REL_SCALE_VALUE ? a.scale : a.scale_v[b];
  const Matches<T> M(a, b);
  const long long eo = a.est_off[b];
  const S* __restrict__ est_t = static_cast<const S*>(a.est_t) + eo;
  double* __restrict__ u = a.u + eo;
  const bool est_along = a.along == DEVO_TRAJ_REL_ALONG_EST;
  const int unit = a.unit;

  // the index itself (frames, stamps) or its increments (the scan below sums them)
  for (int k = tid; k < n; k += TB) {
    double d = 0.0;
    if (unit == DEVO_TRAJ_REL_UNIT_FRAMES) {
      d = (double)k;
    } else if (unit == DEVO_TRAJ_REL_UNIT_STAMPS) {
      d = (double)est_t[M.ie(k)];
    } else if (k > 0) {
      if (unit == DEVO_TRAJ_REL_UNIT_METRES) {
        d = est_along ? c * norm(M.x(k) - M.x(k - 1)) : norm(M.y(k) - M.y(k - 1));
      } else {
        const double ang = est_along ? qangle_rad(qmul(qconj(M.qx(k - 1)), M.qx(k))) : qangle_rad(qmul(qconj(M.qy(k - 1)), M.qy(k)));
        d = unit == DEVO_TRAJ_REL_UNIT_DEGREES ? ang * (180.0 / 3.14159265358979323846) : ang;
      }
    }
    u[k] = d;
  }
  __syncthreads();

  if (unit >= DEVO_TRAJ_REL_UNIT_METRES) {
    // an inclusive scan: thread t owns the chunk [t chunk, (t + 1) chunk); its sum, the wave's scan of the sums, the waves in order
    const int chunk = (n + TB - 1) / TB;
    const int beg = min(n, tid * chunk), fin = min(n, beg + chunk);
    double sum = 0.0;
    for (int k = beg; k < fin; k++) sum += u[k];
    double incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) sh_wave[wv] = incl;
    const double before = __shfl_up(incl, 1, 64);
    __syncthreads();
    double run = 0.0;
    for (int w = 0; w < WAVES; w++) run += w < wv ? sh_wave[w] : 0.0;
    if (lane > 0) run += before;
    for (int k = beg; k < fin; k++) { run += u[k]; u[k] = run; }       // (its own chunk only)
    __syncthreads();
  }

  int bad = 0;
  if (unit == DEVO_TRAJ_REL_UNIT_STAMPS)                               // the estimate's matched stamps must not decrease (finite: the association saw them)
    for (int k = tid; k + 1 < n; k += TB) bad |= u[k + 1] < u[k] ? 1 : 0;
  if (__syncthreads_or(bad)) { give_up(DEVO_TRAJ_UNSORTED); return; }
  if (tid == 0) { meta[0] = (double)n; meta[1] = c; meta[2] = u[n - 1] - u[0]; meta[3] = 0.0; }
}

// ---- errors: one workgroup per (pair, delta)
template <typename T>
__global__ __launch_bounds__(TB) void k_traj_rel_errors(const RelArgs a) {
  __shared__ double sh_red[WAVES][MAXR];
  __shared__ SelectLds sh_sel;
  const int b = blockIdx.x / a.D, d = blockIdx.x % a.D, tid = threadIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double* __restrict__ row = a.stats + ((long long)b * a.D + d) * DEVO_TRAJ_REL_COLS;
  const double* __restrict__ meta = a.meta + (long long)b * META;
  const int flags = (int)meta[3], n = (int)meta[0];
  const double c = meta[1];

  auto give_up = [&](int f) {
    if (tid == 0) {
      row[0] = 0.0;
      for (int k = 1; k < DEVO_TRAJ_REL_COLS; k++) row[k] = qnan;
      a.status[(long long)b * a.D + d] = f;
    }
  };
  if (flags & DEVO_TRAJ_BAD_OFFSETS) { give_up(flags); return; }       // (no rows of its own to fill)
  const long long eo = a.est_off[b], ne = a.est_off[b + 1] - eo;
  double* __restrict__ err2 = a.err2 + 2 * ((long long)d * a.total_est + eo);
  int* __restrict__ ends = a.ends + (long long)d * a.total_est + eo;
  for (long long i = tid; i < ne; i += TB) { err2[2 * i] = qnan; err2[2 * i + 1] = qnan; ends[i] = -1; }
  if (flags) { give_up(flags); return; }
  __syncthreads();

  const Matches<T> M(a, b);
  const double* __restrict__ u = a.u + eo;
  const double delta = a.relative ? a.deltas[d] * meta[2] : a.deltas[d];
  const bool reach = a.end == DEVO_TRAJ_REL_END_REACH;

  // 0 the number of pose pairs, 1 sum te, 2 sum te^2, 3 sum re, 4 sum re^2, 5 sum (u_j - u_i)
  double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double tlo = inf, thi = -inf, rlo = inf, rhi = -inf;
  for (int i = tid; i < n; i += TB) {
    const double ui = u[i];
    int j;
    bool valid;
    if (reach) {                                                     // the first j > i with u_j - u_i >= delta
      int lo = i + 1, hi = n;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u[mid] - ui >= delta) hi = mid; else lo = mid + 1;
      }
      j = lo;
      valid = j < n;
    } else {                                                         // the j nearest to u_i + delta, the lowest on a tie; dropped at the last match
      const double target = ui + delta;
      const int lb = lower_bound(u, n, target);
      if (lb == n) {
        j = lower_bound(u, n, u[n - 1]);
      } else if (lb == 0) {
        j = 0;
      } else {
        const double below = u[lb - 1];
        j = target - below <= u[lb] - target ? lower_bound(u, lb, below) : lb;
      }
      valid = j != n - 1;
    }
    if (!valid) continue;
    const Q4 qxi = M.qx(i), qyi = M.qy(i);
    const V3 ta = c * qrot(qconj(qxi), M.x(j) - M.x(i));               // c . (X_i^-1 X_j)
    const Q4 qa = qmul(qconj(qxi), M.qx(j));
    const V3 tb = qrot(qconj(qyi), M.y(j) - M.y(i));                   // Y_i^-1 Y_j
    const Q4 qb = qmul(qconj(qyi), M.qy(j));
    const double te = norm(qrot(qconj(qa), tb - ta));
    const double re = qangle_deg(qmul(qconj(qa), qb));
    err2[2 * (long long)i] = te; err2[2 * (long long)i + 1] = re; ends[i] = j;
    sums[0] += 1.0; sums[1] += te; sums[2] += te * te; sums[3] += re; sums[4] += re * re; sums[5] += u[j] - ui;
    tlo = fmin(tlo, te); thi = fmax(thi, te); rlo = fmin(rlo, re); rhi = fmax(rhi, re);
  }
  block_sum(sums, sh_red);                                           // (its barriers also publish err2 and ends)
  block_minmax(tlo, thi, sh_red);
  block_minmax(rlo, rhi, sh_red);
  const int m = (int)sums[0];
  if (m == 0) { give_up(DEVO_TRAJ_REL_NO_PAIR); return; }
  const double dm = (double)m, tmean = sums[1] / dm, rmean = sums[3] / dm;      // (divisions: an exact mean where the sum is an exact multiple)

  // the standard deviations' second pass; the medians
  double dev[2] = {0.0, 0.0};
  bool nan = false;
  for (int i = tid; i < n; i += TB) {
    if (ends[i] < 0) continue;
    const double te = err2[2 * (long long)i], re = err2[2 * (long long)i + 1];
    nan |= te != te || re != re;
    dev[0] += (te - tmean) * (te - tmean);
    dev[1] += (re - rmean) * (re - rmean);
  }
  block_sum(dev, sh_red);
  const int any_nan = __syncthreads_or(nan ? 1 : 0);
  const double tmed = block_median<2, true>(err2, ends, n, m, sh_sel);
  const double rmed = block_median<2, true>(err2 + 1, ends, n, m, sh_sel);

  if (tid == 0) {
    const bool tbad = sums[2] != sums[2], rbad = sums[4] != sums[4];
    row[0] = (double)m;
    row[1] = sqrt(sums[2] / dm);
    row[2] = tmean;
    row[3] = any_nan ? qnan : tmed;
    row[4] = sqrt(dev[0] / dm);
    row[5] = tbad ? qnan : tlo;
    row[6] = tbad ? qnan : thi;
    row[7] = sqrt(sums[4] / dm);
    row[8] = rmean;
    row[9] = any_nan ? qnan : rmed;
    row[10] = sqrt(dev[1] / dm);
    row[11] = rbad ? qnan : rlo;
    row[12] = rbad ? qnan : rhi;
    row[13] = delta;
    row[14] = sums[5] / dm;
    row[15] = c;
    a.status[(long long)b * a.D + d] = 0;
  }
}

struct WsLayout { size_t eval, ev_stats, ev_tf, ev_status, u, meta, err2, ends, total; };
WsLayout ws_layout(int64_t total_est, int assoc, int B, int D) {
  WsLayout L;
  const size_t n = total_est > 0 ? (size_t)total_est : 0, nb = B > 0 ? (size_t)B : 0, nd = D > 0 ? (size_t)D : 0;
  size_t o = 0;
  L.eval = o; o += align_up(eval_ws(total_est, assoc).total);
  L.ev_stats = o; o += align_up(nb * DEVO_TRAJ_EVAL_COLS * sizeof(double));
  L.ev_tf = o; o += align_up(nb * 8 * sizeof(double));
  L.ev_status = o; o += align_up(nb * sizeof(int));
  L.u = o; o += align_up(n * sizeof(double));
  L.meta = o; o += align_up(nb * META * sizeof(double));
  L.err2 = o; o += align_up(nd * n * 2 * sizeof(double));
  L.ends = o; o += align_up(nd * n * sizeof(int));
  L.total = o;
  return L;
}

}  // namespace

extern "C" size_t devo_traj_rel_workspace_bytes(int64_t total_est, int assoc, int B, int D) { return ws_layout(total_est, assoc, B, D).total; }

extern "C" int devo_traj_rel_eval(const void* est, const void* est_stamps, const int64_t* est_off, int64_t total_est, const void* gt, const void* gt_stamps,
                                  const int64_t* gt_off, int64_t total_gt, int B, int pose_dtype, int stamps_f64, int assoc, double max_diff,
                                  const double* deltas, int D, int unit, int relative, int along, int end, int scale_mode, double scale,
                                  const double* scale_per_pair, double* stats, int* status, double* errors_out, int* ends_out, void* ws, size_t ws_bytes,
                                  devo_stream_t stream) {
  DEVO_REQUIRE(B >= 1 && B <= 0x7fffffff / DEVO_TRAJ_REL_MAX_DELTAS, "traj_rel_eval: B %d", B);
  DEVO_REQUIRE(deltas && D >= 1 && D <= DEVO_TRAJ_REL_MAX_DELTAS, "traj_rel_eval: 1 .. %d deltas expected (%d)", DEVO_TRAJ_REL_MAX_DELTAS, D);
  for (int d = 0; d < D; d++) DEVO_REQUIRE(deltas[d] > 0.0 && deltas[d] < INFINITY, "traj_rel_eval: delta %d must be positive and finite (%g)", d, deltas[d]);
  DEVO_REQUIRE(unit >= DEVO_TRAJ_REL_UNIT_FRAMES && unit <= DEVO_TRAJ_REL_UNIT_DEGREES, "traj_rel_eval: unknown unit %d", unit);
  DEVO_REQUIRE(along == DEVO_TRAJ_REL_ALONG_GT || along == DEVO_TRAJ_REL_ALONG_EST, "traj_rel_eval: unknown along %d", along);
  DEVO_REQUIRE(end == DEVO_TRAJ_REL_END_REACH || end == DEVO_TRAJ_REL_END_CLOSEST, "traj_rel_eval: unknown end rule %d", end);
  DEVO_REQUIRE(scale_mode >= DEVO_TRAJ_REL_SCALE_SIM3 && scale_mode <= DEVO_TRAJ_REL_SCALE_PER_PAIR, "traj_rel_eval: unknown scale mode %d", scale_mode);
  DEVO_REQUIRE(scale_mode != DEVO_TRAJ_REL_SCALE_VALUE || (scale > 0.0 && scale < INFINITY), "traj_rel_eval: the scale must be positive and finite (%g)", scale);
  DEVO_REQUIRE(scale_mode != DEVO_TRAJ_REL_SCALE_PER_PAIR || scale_per_pair, "traj_rel_eval: null per-pair scales");
  DEVO_REQUIRE(stats && status && ws, "traj_rel_eval: null tensor");
  DEVO_REQUIRE(total_est >= 0, "traj_rel_eval: %lld estimated poses", (long long)total_est);
  const WsLayout L = ws_layout(total_est, assoc, B, D);
  if (ws_bytes < L.total || ((uintptr_t)ws & 15)) {
    set_error("traj_rel_eval: workspace of %zu bytes at %p (%zu needed, 16-byte aligned)", ws_bytes, ws, L.total);
    return DEVO_ERR_WORKSPACE;
  }
  char* w = static_cast<char*>(ws);
  double* ev_stats = reinterpret_cast<double*>(w + L.ev_stats);
  double* ev_tf = reinterpret_cast<double*>(w + L.ev_tf);
  int* ev_status = reinterpret_cast<int*>(w + L.ev_status);
  const EvalWs E = eval_ws(total_est, assoc);                        // the evaluation launch's own part of the workspace, at L.eval
  // association (and the Umeyama scale): the evaluation launch, which checks every argument it shares with this call
  const int rc = devo_traj_eval(est, est_stamps, est_off, total_est, gt, gt_stamps, gt_off, total_gt, B, pose_dtype, stamps_f64, assoc,
                                scale_mode == DEVO_TRAJ_REL_SCALE_SIM3 ? DEVO_TRAJ_ALIGN_SIM3 : DEVO_TRAJ_ALIGN_NONE, max_diff, 0, ev_stats, ev_tf, ev_status,
                                nullptr, nullptr, w + L.eval, E.total, stream);
  if (rc != DEVO_OK) return rc;

  RelArgs a;
  a.est = est; a.est_t = est_stamps; a.est_off = est_off; a.total_est = total_est;
  a.gt = gt; a.gt_off = gt_off; a.total_gt = total_gt;
  a.assoc = assoc; a.unit = unit; a.relative = relative ? 1 : 0; a.along = along; a.end = end; a.scale_mode = scale_mode; a.D = D;
  a.scale = scale; a.scale_v = scale_per_pair;
  for (int d = 0; d < DEVO_TRAJ_REL_MAX_DELTAS; d++) a.deltas[d] = d < D ? deltas[d] : 0.0;
  a.mi = reinterpret_cast<const int*>(w + L.eval + E.mi); a.mj = reinterpret_cast<const int*>(w + L.eval + E.mj);
  a.ipose = reinterpret_cast<const double*>(w + L.eval + E.ipose);
  a.ev_stats = ev_stats; a.ev_tf = ev_tf; a.ev_status = ev_status;
  a.u = reinterpret_cast<double*>(w + L.u); a.meta = reinterpret_cast<double*>(w + L.meta);
  a.err2 = errors_out ? errors_out : reinterpret_cast<double*>(w + L.err2);
  a.ends = ends_out ? ends_out : reinterpret_cast<int*>(w + L.ends);
  a.stats = stats; a.status = status;
  const hipStream_t s = (hipStream_t)stream;
  if (pose_dtype == DEVO_F32) {
    if (stamps_f64) hipLaunchKernelGGL((k_traj_rel_prepare<float, double>), dim3(B), dim3(TB), 0, s, a);
    else hipLaunchKernelGGL((k_traj_rel_prepare<float, int64_t>), dim3(B), dim3(TB), 0, s, a);
    hipLaunchKernelGGL((k_traj_rel_errors<float>), dim3(B * D), dim3(TB), 0, s, a);
  } else {
    if (stamps_f64) hipLaunchKernelGGL((k_traj_rel_prepare<double, double>), dim3(B), dim3(TB), 0, s, a);
    else hipLaunchKernelGGL((k_traj_rel_prepare<double, int64_t>), dim3(B), dim3(TB), 0, s, a);
    hipLaunchKernelGGL((k_traj_rel_errors<double>), dim3(B * D), dim3(TB), 0, s, a);
  }
  return check_launch("traj_rel_eval");
}
