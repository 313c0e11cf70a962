// Event stream -> voxel grid, and the voxel standardisation (utils/event_utils.py:180-232,
// utils/voxel_utils.py:6-28 == devo/devo.py:438-452) — the step in front of the feature encoders, on the GPU so that a
// raw event stream can be handed over as device arrays.
//   * k_voxelize: one event per thread votes into the 2x2x2 neighbouring voxels of (t, y, x); weights are evaluated in
//     fp64 like the reference (x, y, t are fp64 there) and added as fp32 with hardware float atomics (HBM/L2 atomics;
//     the summation ORDER differs from the reference's eight sequential index_add_ passes: results agree to fp32
//     rounding, not bit for bit).
//   * k_voxel_stats / k_voxel_normalise: count, sum and sum of squares of the non-zero voxels of every segment (fp64
//     accumulation; the reference sums in fp32), then  v <- (v != 0) * (v - mean) / std.
//   * windows (utils/load_utils.py:47-76 with EventSlicer, utils/event_utils.py:47-170): S windows [t0, t1) over ONE event
//     stream with ascending timestamps.  k_window_bounds finds every window's event range (lower_bound of t0 and of t1:
//     EventSlicer's t0 <= t < t1) and its first timestamp and duration on the device; k_voxelize_windows votes every window's
//     events into its own grid with the same per-event arithmetic as k_voxelize (its time axis normalised by the window's
//     own first and last event), optionally rectifying the raw integer coordinates through map[y, x] first
//     (load_utils.py:55).  No host round trip between the two launches.
//   * k_voxel_sum2 / k_voxel_hot_zero: RemoveHotPixelsVoxel's num_stds mode (event_utils.py:235-262) per segment: mean and
//     unbiased std over ALL voxels (zeros included, fp64 accumulation; the reference works in fp32), then every voxel with
//     |v| > mean + k std is zeroed.
//   * k_rescale_range / k_rescale_apply: voxel_utils.py:31-51 — positives divided by the maximum of ALL positives, negatives
//     by minus the minimum of ALL negatives (both global over the tensor, as the reference's 1-D masked selection makes
//     them); a polarity without entries is left as it is.
#include <algorithm>
#include "common.h"

namespace devo {

// the 2x2x2 trilinear vote of one event at (x, y, t) into grid [bins, H, W] (event_utils.py:213-230): weights in fp64,
// added as fp32; corners outside the grid and a NaN t (a window of one timestamp: 0 / 0) vote nowhere
__device__ __forceinline__ void vote8(float* __restrict__ grid, int H, int W, int bins, double x, double y, double t, float pol) {
  const double fx = floor(x), fy = floor(y), ft = floor(t);
#pragma unroll
  for (int cx = 0; cx < 2; cx++)
#pragma unroll
    for (int cy = 0; cy < 2; cy++)
#pragma unroll
      for (int ct = 0; ct < 2; ct++) {
        const double lx = fx + cx, ly = fy + cy, lt = ft + ct;
        if (lx >= 0 && ly >= 0 && lt >= 0 && lx <= W - 1 && ly <= H - 1 && lt <= bins - 1) {
          const double w = (double)pol * (1.0 - fabs(lx - x)) * (1.0 - fabs(ly - y)) * (1.0 - fabs(lt - t));
          atomicAdd(grid + ((int64_t)lt * H + (int64_t)ly) * W + (int64_t)lx, (float)w);
        }
      }
}

__global__ void k_voxelize(const float* __restrict__ xs, const float* __restrict__ ys, const double* __restrict__ ts,
                           const signed char* __restrict__ ps, int64_t N, int H, int W, int bins, float* __restrict__ grid) {
  const double t0 = ts[0], dur = ts[N - 1] - t0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const double x = (double)xs[i], y = (double)ys[i];
    const double t = (ts[i] - t0) * (double)(bins - 1) / dur;
    const float pol = (ps[i] == 0) ? -1.0f : (float)ps[i];                  // event_utils.py:198
    vote8(grid, H, W, bins, x, y, t, pol);
  }
}

// stats[s] = {count of non-zeros, sum, sum of squares} of segment s (len elements each); 3 doubles per segment,
// zeroed by the launcher; per-workgroup partials are combined with fp64 atomics.
__global__ __launch_bounds__(256) void k_voxel_stats(const float* __restrict__ v, int64_t len, double* __restrict__ stats) {
  __shared__ double s_red[3][4];
  const int seg = blockIdx.y;
  const float* p = v + (int64_t)seg * len;
  double c = 0.0, s = 0.0, q = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
    const float a = p[i];
    if (a != 0.0f) { c += 1.0; s += (double)a; q += (double)a * (double)a; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { c += __shfl_xor(c, off); s += __shfl_xor(s, off); q += __shfl_xor(q, off); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_red[0][wave] = c; s_red[1][wave] = s; s_red[2][wave] = q; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double t = (s_red[threadIdx.x][0] + s_red[threadIdx.x][1]) + (s_red[threadIdx.x][2] + s_red[threadIdx.x][3]);
    atomicAdd(stats + 3 * seg + threadIdx.x, t);
  }
}

// all_nonempty = every segment has a non-zero (the reference normalises only then, voxel_utils.py:19)
__global__ void k_voxel_normalise(float* __restrict__ v, int64_t len, int nseg, const double* __restrict__ stats) {
  for (int s = 0; s < nseg; s++) if (!(stats[3 * s] > 0.0)) return;
  const int seg = blockIdx.y;
  const double cnt = stats[3 * seg];
  const float mean = (float)(stats[3 * seg + 1] / cnt);
  const float sd = sqrtf((float)(stats[3 * seg + 2] / cnt) - mean * mean);
  float* p = v + (int64_t)seg * len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    const float a = p[i];
    p[i] = (a != 0.0f) ? (a - mean) / sd : 0.0f * ((a - mean) / sd);       // mask * (...): 0 * finite = 0, like the reference
  }
}


// ---- windows over one stream

// zero n 32-bit words.  The front-end entry points clear their outputs and workspaces with this kernel rather than with
// hipMemsetAsync: captured into a HIP graph, the memset of a window batch's grids was not seen again at replay (the
// replayed grids held the buffer's earlier contents), the kernel is replayed like every other launch
__global__ void k_zero_words(uint32_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}


__device__ __forceinline__ double ts_at(const double* ts, int64_t i) { return ts[i]; }
__device__ __forceinline__ double ts_at(const int64_t* ts, int64_t i) { return (double)ts[i]; }   // microseconds: exact below 2^53

// first index whose timestamp is >= t (N when there is none)
template <typename TS>
__device__ __forceinline__ int64_t lower_bound_ts(const TS* __restrict__ ts, int64_t N, double t) {
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ts_at(ts, mid) < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one thread per window: range[2 s] = first event, range[2 s + 1] = one past the last; info[2 s] = first timestamp,
// info[2 s + 1] = duration (last - first); counts[s] = number of events (optional)
template <typename TS>
__global__ void k_window_bounds(const TS* __restrict__ ts, int64_t N, const double* __restrict__ t0, const double* __restrict__ t1, int S,
                                int64_t* __restrict__ range, double* __restrict__ info, int64_t* __restrict__ counts) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t a = lower_bound_ts(ts, N, t0[s]);
  int64_t b = lower_bound_ts(ts, N, t1[s]);
  if (b < a) b = a;                                                        // t1 <= t0: an empty window
  range[2 * s] = a;
  range[2 * s + 1] = b;
  info[2 * s] = (b > a) ? ts_at(ts, a) : 0.0;
  info[2 * s + 1] = (b > a) ? ts_at(ts, b - 1) - ts_at(ts, a) : 0.0;
  if (counts != nullptr) counts[s] = b - a;
}

// `bpw` workgroups per window (window s = blockIdx.x / bpw) sweep that window's events.  RECT: xs, ys are raw int32 sensor
// coordinates, looked up in map [H, W, 2] (an event outside the sensor is dropped); otherwise xs, ys are f32 coordinates.
template <typename TS, bool RECT>
__global__ __launch_bounds__(256) void k_voxelize_windows(const void* __restrict__ xs_, const void* __restrict__ ys_, const TS* __restrict__ ts,
                                                          const signed char* __restrict__ ps, const int64_t* __restrict__ range,
                                                          const double* __restrict__ info, const float* __restrict__ map, int H, int W,
                                                          int bins, int bpw, float* __restrict__ out) {
  const int s = blockIdx.x / bpw, b = blockIdx.x - s * bpw;
  const int64_t lo = range[2 * s], hi = range[2 * s + 1];
  const double tfirst = info[2 * s], dur = info[2 * s + 1];
  float* grid = out + (int64_t)s * bins * H * W;
  for (int64_t i = lo + (int64_t)b * 256 + threadIdx.x; i < hi; i += (int64_t)bpw * 256) {
    double x, y;
    if (RECT) {
      const int xi = ((const int*)xs_)[i], yi = ((const int*)ys_)[i];
      if (xi < 0 || yi < 0 || xi >= W || yi >= H) continue;
      const float* r = map + 2 * ((int64_t)yi * W + xi);                      // load_utils.py:55  rect = rectify_map[y, x]
      x = (double)r[0];
      y = (double)r[1];
    } else {
      x = (double)((const float*)xs_)[i];
      y = (double)((const float*)ys_)[i];
    }
    const double t = (ts_at(ts, i) - tfirst) * (double)(bins - 1) / dur;
    const float pol = (ps[i] == 0) ? -1.0f : (float)ps[i];
    vote8(grid, H, W, bins, x, y, t, pol);
  }
}

// ---- hot pixels

// stats[2 seg] += sum, stats[2 seg + 1] += sum of squares of segment seg (zeros included); `bps` workgroups per segment
__global__ __launch_bounds__(256) void k_voxel_sum2(const float* __restrict__ v, int64_t len, int bps, double* __restrict__ stats) {
  __shared__ double s_red[2][4];
  const int seg = blockIdx.x / bps, b = blockIdx.x - seg * bps;
  const float* p = v + (int64_t)seg * len;
  double s = 0.0, q = 0.0;
  for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < len; i += (int64_t)bps * 256) {
    const double a = (double)p[i];
    s += a;
    q += a * a;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { s += __shfl_xor(s, off); q += __shfl_xor(q, off); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_red[0][wave] = s; s_red[1][wave] = q; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double t = (s_red[threadIdx.x][0] + s_red[threadIdx.x][1]) + (s_red[threadIdx.x][2] + s_red[threadIdx.x][3]);
    atomicAdd(stats + 2 * seg + threadIdx.x, t);
  }
}

// v <- 0 where |v| > mean + k std (torch.std: unbiased, n - 1; one element gives NaN and nothing is zeroed, like the reference)
__global__ __launch_bounds__(256) void k_voxel_hot_zero(float* __restrict__ v, int64_t len, int bps, double k, const double* __restrict__ stats) {
  const int seg = blockIdx.x / bps, b = blockIdx.x - seg * bps;
  const double n = (double)len, sum = stats[2 * seg], mean = sum / n;
  double var = (stats[2 * seg + 1] - sum * mean) / (n - 1.0);
  if (var < 0.0) var = 0.0;                                                  // rounding; a NaN (n = 1) stays NaN
  const double thr = mean + k * sqrt(var);
  float* p = v + (int64_t)seg * len;
  for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < len; i += (int64_t)bps * 256)
    if (fabs((double)p[i]) > thr) p[i] = 0.0f;
}

// ---- rescale

// mx[0] = bits of the largest positive entry, mx[1] = bits of minus the smallest negative one (0 = none); the bit patterns of
// non-negative floats order like the floats, so an unsigned atomicMax finds them
__global__ __launch_bounds__(256) void k_rescale_range(const float* __restrict__ v, int64_t n, unsigned* __restrict__ mx) {
  float pmax = 0.0f, nmax = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = v[i];
    if (a > 0.0f) pmax = fmaxf(pmax, a);
    if (a < 0.0f) nmax = fmaxf(nmax, -a);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { pmax = fmaxf(pmax, __shfl_xor(pmax, off)); nmax = fmaxf(nmax, __shfl_xor(nmax, off)); }
  if ((threadIdx.x & 63) == 0) {
    if (pmax > 0.0f) atomicMax(mx, __float_as_uint(pmax));
    if (nmax > 0.0f) atomicMax(mx + 1, __float_as_uint(nmax));
  }
}

__global__ __launch_bounds__(256) void k_rescale_apply(const float* __restrict__ v, float* __restrict__ out, int64_t n, const unsigned* __restrict__ mx) {
  const float pmax = __uint_as_float(mx[0]), nmax = __uint_as_float(mx[1]);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = v[i];
    out[i] = (a > 0.0f) ? a / pmax : (a < 0.0f) ? a / nmax : a;             // a / -vx_min: the negation is exact
  }
}

}  // namespace devo

using namespace devo;

namespace {
// bytes: a multiple of 4
int zero_async(void* p, size_t bytes, hipStream_t st, const char* what) {
  const int64_t n = (int64_t)(bytes / 4);
  hipLaunchKernelGGL(k_zero_words, dim3(blocks_for(n, 256 * 4, 4096)), dim3(256), 0, st, (uint32_t*)p, n);
  return check_launch(what);
}
}  // namespace

extern "C" {

int devo_voxelize(const float* xs, const float* ys, const double* ts, const signed char* ps, int64_t N, int H, int W, int bins,
                  float* grid, devo_stream_t stream) {
  DEVO_REQUIRE(N >= 0 && H > 0 && W > 0 && bins > 0, "devo_voxelize: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(grid, 0, sizeof(float) * (size_t)bins * H * W, st) != hipSuccess) { set_error("devo_voxelize: memset failed"); return DEVO_ERR_LAUNCH; }
  if (N == 0) return DEVO_OK;                                  // empty stream: empty grid (event_utils.py:187)
  hipLaunchKernelGGL(k_voxelize, dim3(blocks_for(N, 256, 4096)), dim3(256), 0, st, xs, ys, ts, ps, N, H, W, bins, grid);
  return check_launch("devo_voxelize");
}

size_t devo_voxel_std_workspace_bytes(int nseg) { return sizeof(double) * 3 * (size_t)(nseg > 0 ? nseg : 1); }

int devo_voxel_std(float* vox, int nseg, int64_t len, void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(nseg >= 0 && len >= 0, "devo_voxel_std: bad sizes");
  if (nseg == 0 || len == 0) return DEVO_OK;
  if (ws == nullptr || ws_bytes < devo_voxel_std_workspace_bytes(nseg)) { set_error("devo_voxel_std: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, devo_voxel_std_workspace_bytes(nseg), st) != hipSuccess) { set_error("devo_voxel_std: memset failed"); return DEVO_ERR_LAUNCH; }
  const unsigned bx = (unsigned)blocks_for(len, 256 * 8, 512);
  hipLaunchKernelGGL(k_voxel_stats, dim3(bx, (unsigned)nseg), dim3(256), 0, st, vox, len, (double*)ws);
  hipLaunchKernelGGL(k_voxel_normalise, dim3(bx, (unsigned)nseg), dim3(256), 0, st, vox, len, nseg, (const double*)ws);
  return check_launch("devo_voxel_std");
}

size_t devo_voxelize_windows_workspace_bytes(int S) { return (2 * sizeof(int64_t) + 2 * sizeof(double)) * (size_t)(S > 0 ? S : 1); }

int devo_voxelize_windows(const void* xs, const void* ys, const void* ts, int ts_i64, const signed char* ps, int64_t N, const double* t0,
                          const double* t1, int S, const float* rectify_map, int H, int W, int bins, float* out, int64_t* counts, void* ws,
                          size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(N >= 0 && S >= 0 && H > 0 && W > 0 && bins > 0, "devo_voxelize_windows: bad sizes");
  if (S == 0) return DEVO_OK;
  if (ws == nullptr || ws_bytes < devo_voxelize_windows_workspace_bytes(S)) { set_error("devo_voxelize_windows: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  int rc = zero_async(out, sizeof(float) * (size_t)S * bins * H * W, st, "devo_voxelize_windows (zero)");
  if (rc != DEVO_OK) return rc;
  if (N == 0)                                                   // empty stream: every window is empty
    return counts != nullptr ? zero_async(counts, sizeof(int64_t) * (size_t)S, st, "devo_voxelize_windows (zero)") : DEVO_OK;
  int64_t* range = (int64_t*)ws;
  double* info = (double*)(range + 2 * (size_t)S);
  const unsigned nb = (unsigned)((S + 255) / 256);
  if (ts_i64) hipLaunchKernelGGL(k_window_bounds<int64_t>, dim3(nb), dim3(256), 0, st, (const int64_t*)ts, N, t0, t1, S, range, info, counts);
  else hipLaunchKernelGGL(k_window_bounds<double>, dim3(nb), dim3(256), 0, st, (const double*)ts, N, t0, t1, S, range, info, counts);
  rc = check_launch("devo_voxelize_windows (bounds)");
  if (rc != DEVO_OK) return rc;
  // the event ranges are on the device only: size the sweep by the mean window (~8 events per thread), at most 1024 workgroups a window
  const long long per = (N + S - 1) / S;
  const int bpw = (int)std::min<long long>(std::max<long long>((per + 2047) / 2048, 1), std::min<long long>(1024, INT32_MAX / S));
  const dim3 grid((unsigned)((long long)S * bpw)), block(256);
  if (rectify_map != nullptr) {
    if (ts_i64) hipLaunchKernelGGL((k_voxelize_windows<int64_t, true>), grid, block, 0, st, xs, ys, (const int64_t*)ts, ps, range, info, rectify_map, H, W, bins, bpw, out);
    else hipLaunchKernelGGL((k_voxelize_windows<double, true>), grid, block, 0, st, xs, ys, (const double*)ts, ps, range, info, rectify_map, H, W, bins, bpw, out);
  } else {
    if (ts_i64) hipLaunchKernelGGL((k_voxelize_windows<int64_t, false>), grid, block, 0, st, xs, ys, (const int64_t*)ts, ps, range, info, nullptr, H, W, bins, bpw, out);
    else hipLaunchKernelGGL((k_voxelize_windows<double, false>), grid, block, 0, st, xs, ys, (const double*)ts, ps, range, info, nullptr, H, W, bins, bpw, out);
  }
  return check_launch("devo_voxelize_windows");
}

size_t devo_voxel_hot_pixels_workspace_bytes(int nseg) { return sizeof(double) * 2 * (size_t)(nseg > 0 ? nseg : 1); }

int devo_voxel_hot_pixels(float* vox, int nseg, int64_t len, double num_stds, void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(nseg >= 0 && len >= 0, "devo_voxel_hot_pixels: bad sizes");
  if (nseg == 0 || len == 0) return DEVO_OK;
  if (ws == nullptr || ws_bytes < devo_voxel_hot_pixels_workspace_bytes(nseg)) { set_error("devo_voxel_hot_pixels: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const int rc = zero_async(ws, devo_voxel_hot_pixels_workspace_bytes(nseg), st, "devo_voxel_hot_pixels (zero)");
  if (rc != DEVO_OK) return rc;
  const int bps = std::min(blocks_for(len, 256 * 8, 512), std::max(INT32_MAX / nseg, 1));
  const dim3 grid((unsigned)((long long)nseg * bps)), block(256);
  hipLaunchKernelGGL(k_voxel_sum2, grid, block, 0, st, (const float*)vox, len, bps, (double*)ws);
  hipLaunchKernelGGL(k_voxel_hot_zero, grid, block, 0, st, vox, len, bps, num_stds, (const double*)ws);
  return check_launch("devo_voxel_hot_pixels");
}

size_t devo_voxel_rescale_workspace_bytes(void) { return 2 * sizeof(unsigned); }

int devo_voxel_rescale(const float* vox, float* out, int64_t n, void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(n >= 0, "devo_voxel_rescale: bad size");
  if (n == 0) return DEVO_OK;
  if (ws == nullptr || ws_bytes < devo_voxel_rescale_workspace_bytes()) { set_error("devo_voxel_rescale: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const int rc = zero_async(ws, devo_voxel_rescale_workspace_bytes(), st, "devo_voxel_rescale (zero)");
  if (rc != DEVO_OK) return rc;
  const unsigned nb = (unsigned)blocks_for(n, 256 * 8, 1024);
  hipLaunchKernelGGL(k_rescale_range, dim3(nb), dim3(256), 0, st, vox, n, (unsigned*)ws);
  hipLaunchKernelGGL(k_rescale_apply, dim3(nb), dim3(256), 0, st, vox, out, n, (const unsigned*)ws);
  return check_launch("devo_voxel_rescale");
}

}  // extern "C"
