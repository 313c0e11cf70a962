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
//   * k_aug_gray_sum / k_aug_apply / k_aug_std: voxel_augment (voxel_utils.py:55-136) — [rescale on the fly], quantise to uint8 R / B
//     images, one torchvision op, back to float, std from exact integer statistics; compiled without FMA contraction.
#include <algorithm>
#include <cmath>
#include "common.h"
#include "voxel_sigma.h"

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
  const float sd = voxel_sigma_f32((float)(stats[3 * seg + 2] / cnt), mean);                     // (the fused multiply-add this line always compiled to)
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
  // one atomic per workgroup and sign: same-address atomics serialise in L2, one per wave cost ~0.1 ms over 92 MB
  __shared__ float s_red[2][4];
  if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = pmax; s_red[1][threadIdx.x >> 6] = nmax; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float m = fmaxf(fmaxf(s_red[threadIdx.x][0], s_red[threadIdx.x][1]), fmaxf(s_red[threadIdx.x][2], s_red[threadIdx.x][3]));
    if (m > 0.0f) atomicMax(mx + threadIdx.x, __float_as_uint(m));
  }
}

__global__ __launch_bounds__(256) void k_rescale_apply(const float* __restrict__ v, float* __restrict__ out, int64_t n, const unsigned* __restrict__ mx) {
  const float pmax = __uint_as_float(mx[0]), nmax = __uint_as_float(mx[1]);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = v[i];
    out[i] = (a > 0.0f) ? a / pmax : (a < 0.0f) ? a / nmax : a;             // a / -vx_min: the negation is exact
  }
}

// ---- voxel augmentation (voxel_utils.py:55-136: rescale -> evs2rgb -> uint8 -> one torchvision 0.13 uint8 tensor op -> float ->
// rgb2evs -> std).  One image is one (segment, bin) slice with channels R = negative part, G = 0, B = positive part.  Every value
// is formed in the reference's order with single fp32 roundings: hipcc contracts a*b + c into an FMA by default, and one FMA moves
// a uint8 truncation boundary, so nothing below may be contracted.
#pragma clang fp contract(off)

enum { AUG_BRIGHTNESS = 0, AUG_CONTRAST, AUG_INVERT, AUG_POSTERIZE, AUG_SATURATION, AUG_SHARPNESS, AUG_SOLARIZE, AUG_NUM_OPS };

struct AugArgs {
  int op, nimg, H, W, rescale;
  float r, omr;                 // _blend: ratio (an fp32 table value) and (float)(1.0 - ratio) formed in double
  int mask, thr;                // posterize: q & mask; solarize: q >= thr (the threshold rounded up: q is an integer)
};

// (x).to(torch.uint8) of a value in [0, 255] (truncation); clamped first, as _blend does, so no input is undefined behaviour
__device__ __forceinline__ int to_u8(float x) { return (int)fminf(fmaxf(x, 0.0f), 255.0f); }

// [rescale] -> evs2rgb -> (255 * rgb).to(uint8) of one voxel: R = negative part, B = positive part (G is 0)
__device__ __forceinline__ void quantise(float a, bool rescale, float pmax, float nmax, int& R, int& B) {
  if (rescale) a = (a > 0.0f) ? a / pmax : (a < 0.0f) ? a / nmax : a;
  R = (a < 0.0f) ? to_u8(255.0f * -a) : 0;
  B = (a > 0.0f) ? to_u8(255.0f * a) : 0;
}

// rgb_to_grayscale: (0.2989 * r + 0.587 * g + 0.114 * b).to(uint8), three fp32 products and two fp32 adds, g = 0
__device__ __forceinline__ int gray_u8(int R, int B) {
  float l = 0.2989f * (float)R;
  l = l + 0.587f * 0.0f;
  l = l + 0.114f * (float)B;
  return to_u8(l);
}

// _blend: (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(uint8)
__device__ __forceinline__ int blend_u8(int q, float img2, float r, float omr) {
  float v = r * (float)q;
  v = v + omr * img2;
  return to_u8(v);
}

// one channel value q through the op; `other` is the contrast mean, the saturation grayscale or the sharpness blur
__device__ __forceinline__ int aug_u8(int q, const AugArgs& a, float other) {
  switch (a.op) {
    case AUG_BRIGHTNESS: return blend_u8(q, 0.0f, a.r, a.omr);
    case AUG_CONTRAST:
    case AUG_SATURATION:
    case AUG_SHARPNESS: return blend_u8(q, other, a.r, a.omr);
    case AUG_INVERT: return 255 - q;
    case AUG_POSTERIZE: return q & a.mask;
    default: return q >= a.thr ? 255 - q : q;                              // solarize
  }
}

// _blurred_degenerate_image at an interior pixel: round(conv([[1,1,1],[1,5,1],[1,1,1]] / 13)).  k / 13 for an integer k is never
// within 1/26 of a tie, far beyond the fp32 rounding of any summation order, so round(k / 13) = floor((2k + 13) / 26) exactly
__device__ __forceinline__ int blur_u8(int sum9, int centre) { return (2 * (sum9 + 4 * centre) + 13) / 26; }

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ row, int x0, int W, float v[4]) {
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(row + x0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (x0 + k < W) ? row[x0 + k] : 0.0f;
  }
}

// gsum[img] = sum over the image of its uint8 grayscale (adjust_contrast's mean, exact); `bpi` workgroups per image
template <bool VEC>
__global__ __launch_bounds__(256) void k_aug_gray_sum(const float* __restrict__ vox, AugArgs a, int bpi, const unsigned* __restrict__ mx,
                                                      unsigned long long* __restrict__ gsum) {
  __shared__ unsigned long long s_red[4];
  const int img = blockIdx.x / bpi, b = blockIdx.x - img * bpi;
  const int64_t len = (int64_t)a.H * a.W;
  const float* p = vox + (int64_t)img * len;
  const float pmax = __uint_as_float(mx[0]), nmax = __uint_as_float(mx[1]);
  unsigned long long s = 0;
  for (int64_t i = ((int64_t)b * 256 + threadIdx.x) * 4; i < len; i += (int64_t)bpi * 256 * 4) {
    float v[4];
    load4<VEC>(p + i, 0, (int)(len - i < 4 ? len - i : 4), v);             // VEC: len is a multiple of 4
    unsigned t = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      int R, B;
      quantise(v[k], a.rescale, pmax, nmax, R, B);
      t += (i + k < len) ? (unsigned)gray_u8(R, B) : 0u;
    }
    s += t;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(gsum + img, (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
}

// the op pass: every thread takes 4 neighbouring voxels of one row (a 16-byte load when VEC), quantises, applies the op, writes
// B'/255 + (-(R'/255)) and, with `stats`, adds the segment's exact integer statistics of d = B' - R' (count of d != 0, sum d,
// sum d^2) for the standardisation.  Sharpness reads the rows above and below from the caches.  `bps` workgroups per segment.
template <bool VEC>
__global__ __launch_bounds__(256) void k_aug_apply(const float* __restrict__ vox, float* __restrict__ out, AugArgs a, int bps,
                                                   const unsigned* __restrict__ mx, const unsigned long long* __restrict__ gsum,
                                                   unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long s_red[3][4];
  const int seg = blockIdx.x / bps, b = blockIdx.x - seg * bps;
  const int H = a.H, W = a.W, Wq = (W + 3) >> 2;
  const int64_t per_img = (int64_t)H * Wq, groups = (int64_t)a.nimg * per_img, img_len = (int64_t)H * W;
  const float pmax = __uint_as_float(mx[0]), nmax = __uint_as_float(mx[1]);
  const bool sharp = a.op == AUG_SHARPNESS && H > 2 && W > 2;              // adjust_sharpness returns a 2-pixel image unchanged
  const float fimg_len = (float)img_len;
  unsigned long long cnt = 0, s1 = 0, s2 = 0;                               // s1: two's complement
  for (int64_t g = (int64_t)b * 256 + threadIdx.x; g < groups; g += (int64_t)bps * 256) {
    const int i = (int)(g / per_img);
    const int64_t rem = g - (int64_t)i * per_img;
    const int y = (int)(rem / Wq), x0 = (int)(rem - (int64_t)y * Wq) * 4;
    const int64_t img = (int64_t)seg * a.nimg + i;
    const float* src = vox + img * img_len;
    float v[4];
    load4<VEC>(src + (int64_t)y * W, x0, W, v);
    int R[4], B[4];
#pragma unroll
    for (int k = 0; k < 4; k++) quantise(v[k], a.rescale, pmax, nmax, R[k], B[k]);
    int Ro[4], Bo[4];
    if (a.op != AUG_SHARPNESS) {
      const float mean = (a.op == AUG_CONTRAST) ? (float)gsum[img] / fimg_len : 0.0f;   // torch.mean on CPU: sum / N
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float other = (a.op == AUG_SATURATION) ? (float)gray_u8(R[k], B[k]) : mean;
        Ro[k] = aug_u8(R[k], a, other);
        Bo[k] = aug_u8(B[k], a, other);
      }
    } else if (!sharp) {
#pragma unroll
      for (int k = 0; k < 4; k++) { Ro[k] = R[k]; Bo[k] = B[k]; }
    } else {
      // blur of the interior pixels (1 <= x, y <= size - 2); border pixels blend with themselves (result = img.clone())
      int bR[4], bB[4];
#pragma unroll
      for (int k = 0; k < 4; k++) { bR[k] = R[k]; bB[k] = B[k]; }
      if (y >= 1 && y <= H - 2) {
        int nR[3][6], nB[3][6];
#pragma unroll
        for (int dy = 0; dy < 3; dy++) {
          const float* row = src + (int64_t)(y - 1 + dy) * W;
          float w[4];
          if (dy == 1) {
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = v[k];
          } else {
            load4<VEC>(row, x0, W, w);
          }
          const float left = (x0 > 0) ? row[x0 - 1] : 0.0f, right = (x0 + 4 < W) ? row[x0 + 4] : 0.0f;
          quantise(left, a.rescale, pmax, nmax, nR[dy][0], nB[dy][0]);
#pragma unroll
          for (int k = 0; k < 4; k++) quantise(w[k], a.rescale, pmax, nmax, nR[dy][k + 1], nB[dy][k + 1]);
          quantise(right, a.rescale, pmax, nmax, nR[dy][5], nB[dy][5]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int x = x0 + k;
          if (x >= 1 && x <= W - 2) {
            int sr = 0, sb = 0;
#pragma unroll
            for (int dy = 0; dy < 3; dy++)
#pragma unroll
              for (int dx = 0; dx < 3; dx++) { sr += nR[dy][k + dx]; sb += nB[dy][k + dx]; }
            bR[k] = blur_u8(sr, R[k]);
            bB[k] = blur_u8(sb, B[k]);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        Ro[k] = aug_u8(R[k], a, (float)bR[k]);
        Bo[k] = aug_u8(B[k], a, (float)bB[k]);
      }
    }
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      o[k] = (float)Bo[k] / 255.0f + (-((float)Ro[k] / 255.0f));          // .to(float32) / 255, then rgb2evs: pos + (-neg)
      const int d = Bo[k] - Ro[k];
      if (x0 + k < W && d != 0) { cnt += 1; s1 += (unsigned long long)(long long)d; s2 += (unsigned long long)(d * d); }
    }
    float* dst = out + img * img_len + (int64_t)y * W;
    if (VEC) {
      *reinterpret_cast<float4*>(dst + x0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) if (x0 + k < W) dst[x0 + k] = o[k];
    }
  }
  if (stats == nullptr) return;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { cnt += __shfl_xor(cnt, off); s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_red[0][wave] = cnt; s_red[1][wave] = s1; s_red[2][wave] = s2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long t = (s_red[threadIdx.x][0] + s_red[threadIdx.x][1]) + (s_red[threadIdx.x][2] + s_red[threadIdx.x][3]);
    atomicAdd(stats + 3 * seg + threadIdx.x, t);
  }
}

// std(voxs) (sequence-wise) of the op pass's output in place, from its exact integer statistics: the outputs are d / 255, so
// mean = sum d / (255 n) and E[v^2] = sum d^2 / (255^2 n); then v <- (v != 0) * (v - mean) / std as k_voxel_normalise.  Nothing
// changes if a segment has no non-zero voxel (voxel_utils.py:19).
template <bool VEC>
__global__ __launch_bounds__(256) void k_aug_std(float* __restrict__ v, int64_t len, int nseg, int bps, const unsigned long long* __restrict__ stats) {
  for (int s = 0; s < nseg; s++) if (stats[3 * s] == 0) return;
  const int seg = blockIdx.x / bps, b = blockIdx.x - seg * bps;
  const double cnt = (double)stats[3 * seg];
  const float mean = (float)((double)(long long)stats[3 * seg + 1] / (255.0 * cnt));
  const float ex2 = (float)((double)stats[3 * seg + 2] / (65025.0 * cnt));
  const float sd = sqrtf(ex2 - mean * mean);
  float* p = v + (int64_t)seg * len;
  auto f = [&](float x) { return (x != 0.0f) ? (x - mean) / sd : 0.0f * ((x - mean) / sd); };
  if (VEC) {
    for (int64_t i = ((int64_t)b * 256 + threadIdx.x) * 4; i < len; i += (int64_t)bps * 256 * 4) {
      float4 t = *reinterpret_cast<const float4*>(p + i);
      t.x = f(t.x); t.y = f(t.y); t.z = f(t.z); t.w = f(t.w);
      *reinterpret_cast<float4*>(p + i) = t;
    }
  } else {
    for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < len; i += (int64_t)bps * 256) p[i] = f(p[i]);
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

// [0, 8): rescale extremes (2 u32); then u64 grayscale sums [nseg * nimg]; then u64 {count, sum d, sum d^2} [nseg]
size_t devo_voxel_augment_workspace_bytes(int nseg, int nimg) {
  const size_t s = nseg > 0 ? (size_t)nseg : 1, i = nimg > 0 ? (size_t)nimg : 1;
  return 8 + sizeof(unsigned long long) * (s * i + 3 * s);
}

int devo_voxel_augment(const float* vox, float* out, int nseg, int nimg, int H, int W, int rescale, int op, double factor, int standardise,
                       void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(nseg >= 0 && nimg >= 0 && H > 0 && W > 0 && (int64_t)nseg * nimg <= INT32_MAX, "devo_voxel_augment: bad sizes");
  DEVO_REQUIRE(op >= 0 && op < AUG_NUM_OPS, "devo_voxel_augment: unknown op %d", op);
  const bool blend = op == AUG_BRIGHTNESS || op == AUG_CONTRAST || op == AUG_SATURATION || op == AUG_SHARPNESS;
  DEVO_REQUIRE(!blend || (factor >= 0.0 && factor < 1e30), "devo_voxel_augment: the blend factor must be a finite non-negative number");
  DEVO_REQUIRE(op != AUG_POSTERIZE || (factor >= 0.0 && factor <= 8.0 && factor == (double)(int)factor), "devo_voxel_augment: posterize bits must be an integer in [0, 8]");
  DEVO_REQUIRE(op != AUG_SOLARIZE || (factor <= 255.0 && factor == factor), "devo_voxel_augment: the solarize threshold must be at most 255");
  if (nseg == 0 || nimg == 0) return DEVO_OK;
  DEVO_REQUIRE(vox != nullptr && out != nullptr && vox != out, "devo_voxel_augment: out must be a separate buffer");
  if (ws == nullptr || ws_bytes < devo_voxel_augment_workspace_bytes(nseg, nimg)) { set_error("devo_voxel_augment: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  int rc = zero_async(ws, devo_voxel_augment_workspace_bytes(nseg, nimg), st, "devo_voxel_augment (zero)");
  if (rc != DEVO_OK) return rc;
  unsigned* mx = (unsigned*)ws;
  unsigned long long* gsum = (unsigned long long*)((char*)ws + 8);
  unsigned long long* stats = gsum + (size_t)nseg * nimg;

  AugArgs a;
  a.op = op; a.nimg = nimg; a.H = H; a.W = W; a.rescale = rescale ? 1 : 0;
  a.r = (float)factor;
  a.omr = (float)(1.0 - factor);
  a.mask = (op == AUG_POSTERIZE) ? ((0xFF << (8 - (int)factor)) & 0xFF) : 0xFF;
  a.thr = (op == AUG_SOLARIZE) ? (int)std::max(std::ceil(factor), -1.0) : 0;

  const int64_t img_len = (int64_t)H * W, n = (int64_t)nseg * nimg * img_len;
  if (rescale) hipLaunchKernelGGL(k_rescale_range, dim3((unsigned)blocks_for(n, 256 * 8, 1024)), dim3(256), 0, st, vox, n, mx);
  const bool vec = (W % 4 == 0) && ((uintptr_t)vox % 16 == 0) && ((uintptr_t)out % 16 == 0);
  if (op == AUG_CONTRAST) {
    const int nim = nseg * nimg;
    const int bpi = std::min(blocks_for(img_len, 256 * 4 * 4, 256), std::max(INT32_MAX / nim, 1));
    const dim3 grid((unsigned)((long long)nim * bpi)), block(256);
    if (vec) hipLaunchKernelGGL(k_aug_gray_sum<true>, grid, block, 0, st, vox, a, bpi, (const unsigned*)mx, gsum);
    else hipLaunchKernelGGL(k_aug_gray_sum<false>, grid, block, 0, st, vox, a, bpi, (const unsigned*)mx, gsum);
  }
  const int64_t groups = (int64_t)nimg * H * ((W + 3) / 4);
  const int bps = std::min(blocks_for(groups, 256 * 2, 2048), std::max(4096 / nseg, 1));
  const dim3 grid((unsigned)((long long)nseg * bps)), block(256);
  unsigned long long* st_out = standardise ? stats : nullptr;
  if (vec) hipLaunchKernelGGL(k_aug_apply<true>, grid, block, 0, st, vox, out, a, bps, (const unsigned*)mx, (const unsigned long long*)gsum, st_out);
  else hipLaunchKernelGGL(k_aug_apply<false>, grid, block, 0, st, vox, out, a, bps, (const unsigned*)mx, (const unsigned long long*)gsum, st_out);
  rc = check_launch("devo_voxel_augment");
  if (rc != DEVO_OK || !standardise) return rc;
  const int64_t len = (int64_t)nimg * img_len;
  const bool vec_std = (len % 4 == 0) && ((uintptr_t)out % 16 == 0);
  const int bps_std = std::min(blocks_for(len, 256 * 4 * 4, 2048), std::max(4096 / nseg, 1));
  const dim3 grid_std((unsigned)((long long)nseg * bps_std));
  if (vec_std) hipLaunchKernelGGL(k_aug_std<true>, grid_std, block, 0, st, out, len, nseg, bps_std, (const unsigned long long*)stats);
  else hipLaunchKernelGGL(k_aug_std<false>, grid_std, block, 0, st, out, len, nseg, bps_std, (const unsigned long long*)stats);
  return check_launch("devo_voxel_augment (std)");
}

}  // extern "C"
