// Event simulation (devo_amd/simulate.py; include/devo_hip.h): contrast-threshold events from consecutive log-intensity frames, what the
// reference's scripts/convert_tartan.py:198-297 obtains from esim_torch.ESIM.  The model is stated in the header; every pixel walks the
// call's frame pairs on its own, so one thread owns one pixel and a wave reads 64 consecutive pixels of a frame row.
//   k_esim_count   the whole per-pixel walk (refractory test included) without writing an event: per-pixel counts and the status word.
//                  It commits nothing.
//   k_esim_emit    the same walk again from the same state; every emitted event is ONE 64-bit key
//                  (stamp - first stamp) << (pixel bits + 1) | pixel << 1 | (polarity > 0), written at the pixel's offset (the inclusive scan
//                  of the counts); the new ref / last_t go to buffers of their own.
//   (sort)         rocPRIM's keys-only radix sort over the bits the call's keys can have set: nothing travels with a key.
//   k_esim_decode  sorted keys -> x, y, t, p.  The keys' integer order is the events' total order (t, y W + x, p).
//   k_log_intensity  uint8 -> fp32 through a 256-entry table the host computed.
// All model arithmetic is fp64 with one rounding per operation in the order the header states: nothing below may be contracted into an FMA.
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>
#include "common.h"

#pragma clang fp contract(off)

namespace {
using namespace devo;

constexpr int TB = 256;                                       // decode, log_intensity
constexpr int TW = 64;                                        // the two walks: one wave per block, so the blocks spread evenly over the CUs
constexpr int64_t NO_EVENT = INT64_MIN;                      // DEVO_ESIM_NO_EVENT
constexpr double MAX_CROSSINGS = (double)DEVO_ESIM_MAX_CROSSINGS;

struct EsimArgs {
  const float* prev;            // [HW] the frame before the call's first
  const float* frames;          // [T, HW]
  const int64_t* prev_stamp;    // [1]
  const int64_t* stamps;        // [T]
  const double* ref;            // [HW] state (read only)
  const int64_t* last_t;        // [HW] state (read only)
  int64_t HW, refractory, max_span;
  double c_neg, c_pos;
  int T, shift;                 // shift = pixel bits + 1
};

inline int pixel_bits(int64_t hw) {
  int b = 1;
  while (((int64_t)1 << b) < hw) ++b;
  return b;
}

// one past the highest bit a key of a call that spans span_ns can have set; 0 for arguments the entry points refuse
inline unsigned key_end_bit(int H, int W, int64_t span_ns) {
  const int64_t limit = devo_esim_max_span_ns(H, W);
  if (limit == 0 || span_ns < 0 || span_ns >= limit) return 0u;
  unsigned b = 0;
  while (((int64_t)1 << b) <= span_ns) ++b;
  return (unsigned)pixel_bits((int64_t)H * W) + 1u + b;
}

inline hipError_t sort_keys(void* ws, size_t& bytes, const int64_t* keys, int64_t* sorted, int64_t n, unsigned end_bit, hipStream_t s) {
  return rocprim::radix_sort_keys(ws, bytes, reinterpret_cast<const unsigned long long*>(keys), reinterpret_cast<unsigned long long*>(sorted), (size_t)n, 0u, end_bit, s);
}

// One frame pair of pixel i (i0f at t0 -> i1f at t1).  EMIT: keys are written at [pos, end) (never outside it) and every crossing is visited;
// otherwise the emitted events are counted, and without a refractory period (LOOP = false) a pair's n crossings are n events: stamps never
// decrease along a pixel's walk, so `t_k - last_t >= 0` holds for each of them.  `st` collects DEVO_ESIM_* status bits.
template <bool EMIT, bool LOOP>
__device__ __forceinline__ void esim_pair(const EsimArgs& a, int64_t i, float i0f, float i1f, int64_t t0, int64_t t1, int64_t t_first, double& ref, int64_t& last, int& st,
                                          int64_t* __restrict__ keys, int64_t& pos, int64_t end, int64_t& count) {
  if (!(t1 > t0)) st |= DEVO_ESIM_STAMPS;
  else if ((uint64_t)t1 - (uint64_t)t_first >= (uint64_t)a.max_span) st |= DEVO_ESIM_SPAN;
  if (!isfinite(i1f)) st |= DEVO_ESIM_NONFINITE;
  if (st) return;
  const double i0 = (double)i0f, i1 = (double)i1f;
  const double d = i1 - ref;
  const bool up = d >= 0.0;
  const double C = up ? a.c_pos : a.c_neg;
  const double q = floor((up ? d : -d) / C);
  if (!(q <= MAX_CROSSINGS)) {                                 // (a NaN ref lands here too)
    st |= DEVO_ESIM_CROSSINGS;
    return;
  }
  const int n = (int)q;
  if (n <= 0) return;
  if (!EMIT && !LOOP) {
    count += n;
    const double step = (double)n * C;
    ref = up ? ref + step : ref - step;
    return;
  }
  const double den = i1 - i0, dt = (double)(t1 - t0);
  double Lk = ref;
  for (int k = 1; k <= n; ++k) {
    const double step = (double)k * C;
    Lk = up ? ref + step : ref - step;
    double f = 1.0;
    if (den != 0.0) {
      f = (Lk - i0) / den;
      f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
    }
    const int64_t tk = t0 + (int64_t)floor(f * dt);
    if (last == NO_EVENT || tk - last >= a.refractory) {
      last = tk;
      if (EMIT) {
        if (pos < end) keys[pos] = (int64_t)(((uint64_t)(tk - t_first) << a.shift) | ((uint64_t)i << 1) | (up ? 1ull : 0ull));
        ++pos;
      }
      ++count;
    }
  }
  ref = Lk;
}

// The walk of pixel i over the call's T pairs -> the number of emitted events.  A pixel's pairs depend on each other through ref, so a
// thread has little to overlap a load with: the frames are fetched CHUNK at a time, all of a chunk's loads in flight together, before its
// pairs are walked.  A pixel that sets a status bit stops there.
constexpr int CHUNK = 8;
template <bool EMIT, bool LOOP>
__device__ __forceinline__ int64_t esim_walk(const EsimArgs& a, int64_t i, double& ref, int64_t& last, int& st, int64_t* __restrict__ keys, int64_t pos, int64_t end) {
  float i0f = a.prev[i];
  if (!isfinite(i0f)) st |= DEVO_ESIM_NONFINITE;
  const int64_t t_first = *a.prev_stamp;
  int64_t t0 = t_first, count = 0;
  for (int j0 = 0; j0 < a.T && st == 0; j0 += CHUNK) {
    float v[CHUNK];
#pragma unroll
    for (int u = 0; u < CHUNK; ++u) v[u] = (j0 + u < a.T) ? a.frames[(int64_t)(j0 + u) * a.HW + i] : 0.0f;
#pragma unroll
    for (int u = 0; u < CHUNK; ++u) {
      if (j0 + u < a.T && st == 0) {
        const int64_t t1 = a.stamps[j0 + u];
        esim_pair<EMIT, LOOP>(a, i, i0f, v[u], t0, t1, t_first, ref, last, st, keys, pos, end, count);
        i0f = v[u];
        t0 = t1;
      }
    }
  }
  return count;
}

// status_span[0] |= the status bits (one atomic per wave that has any: none on a healthy call), status_span[1] = the call's time span.  The sum of
// the counts is NOT formed here: one atomic per wave on one address costs more than the whole walk; it is the last entry of the counts' scan.
template <bool LOOP>
__global__ __launch_bounds__(TW) void k_esim_count(EsimArgs a, int64_t* __restrict__ counts, unsigned long long* __restrict__ status_span) {
  const int64_t i = (int64_t)blockIdx.x * TW + threadIdx.x;
  int st = 0;
  if (i < a.HW) {
    double ref = a.ref[i];
    int64_t last = a.last_t[i];
    counts[i] = esim_walk<false, LOOP>(a, i, ref, last, st, nullptr, 0, 0);
  }
  for (int o = 32; o > 0; o >>= 1) st |= __shfl_down(st, o);
  if ((threadIdx.x & 63) == 0 && st) atomicOr(&status_span[0], (unsigned long long)st);
  if (i == 0) status_span[1] = (unsigned long long)a.stamps[a.T - 1] - (unsigned long long)*a.prev_stamp;
}

__global__ __launch_bounds__(TW) void k_esim_emit(EsimArgs a, const int64_t* __restrict__ incl, int64_t total, int64_t* __restrict__ keys, double* __restrict__ ref_out,
                                                  int64_t* __restrict__ last_out) {
  const int64_t i = (int64_t)blockIdx.x * TW + threadIdx.x;
  if (i >= a.HW) return;
  double ref = a.ref[i];
  int64_t last = a.last_t[i];
  int64_t pos = i ? incl[i - 1] : 0, end = incl[i];
  if (pos < 0) pos = end = 0;                                  // (offsets that are not a scan of counts write nothing)
  if (end > total) end = total;
  int st = 0;
  esim_walk<true, true>(a, i, ref, last, st, keys, pos, end);
  ref_out[i] = ref;
  last_out[i] = last;
}

__global__ __launch_bounds__(TB) void k_esim_decode(const int64_t* __restrict__ keys, int64_t n, int W, int shift, const int64_t* __restrict__ first_stamp,
                                                    int16_t* __restrict__ x, int16_t* __restrict__ y, int64_t* __restrict__ t, int8_t* __restrict__ p) {
  const int64_t t_first = *first_stamp;
  const uint64_t mask = ((uint64_t)1 << (shift - 1)) - 1;
  for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < n; e += (int64_t)gridDim.x * TB) {
    const uint64_t k = (uint64_t)keys[e];
    const int64_t pix = (int64_t)((k >> 1) & mask);
    const int64_t row = pix / W;
    x[e] = (int16_t)(pix - row * W);
    y[e] = (int16_t)row;
    t[e] = t_first + (int64_t)(k >> shift);
    p[e] = (k & 1) ? (int8_t)1 : (int8_t)-1;
  }
}

// n4 groups of four pixels as one 4-byte load and one 16-byte store (0 when the pointers are not aligned for them), the rest one by one
__global__ __launch_bounds__(TB) void k_log_intensity(const uint8_t* __restrict__ img, int64_t n, int64_t n4, const float* __restrict__ table, float* __restrict__ out) {
  __shared__ float lut[256];
  lut[threadIdx.x] = table[threadIdx.x];                       // TB == 256
  __syncthreads();
  const int64_t gid = (int64_t)blockIdx.x * TB + threadIdx.x, stride = (int64_t)gridDim.x * TB;
  for (int64_t g = gid; g < n4; g += stride) {
    const uchar4 v = reinterpret_cast<const uchar4*>(img)[g];
    reinterpret_cast<float4*>(out)[g] = make_float4(lut[v.x], lut[v.y], lut[v.z], lut[v.w]);
  }
  for (int64_t e = n4 * 4 + gid; e < n; e += stride) out[e] = lut[img[e]];
}

int fill_args(const char* what, const float* prev, const float* frames, const int64_t* prev_stamp, const int64_t* stamps, int T, int H, int W, const double* ref,
              const int64_t* last_t, double c_neg, double c_pos, int64_t refractory_ns, EsimArgs& a) {
  DEVO_REQUIRE(prev && frames && prev_stamp && stamps && ref && last_t, "%s: null tensor", what);
  DEVO_REQUIRE(T >= 1, "%s: %d frames", what, T);
  DEVO_REQUIRE(H >= 1 && W >= 1 && H <= DEVO_ESIM_MAX_SIDE && W <= DEVO_ESIM_MAX_SIDE, "%s: frame %d x %d (sides 1 .. %d: int16 coordinates)", what, H, W, DEVO_ESIM_MAX_SIDE);
  DEVO_REQUIRE(std::isfinite(c_neg) && std::isfinite(c_pos) && c_neg >= DEVO_ESIM_MIN_THRESHOLD && c_pos >= DEVO_ESIM_MIN_THRESHOLD,
               "%s: contrast thresholds must be finite and at least %g (got %g, %g)", what, DEVO_ESIM_MIN_THRESHOLD, c_neg, c_pos);
  DEVO_REQUIRE(refractory_ns >= 0, "%s: negative refractory period", what);
  DEVO_REQUIRE((uintptr_t)prev % 4 == 0 && (uintptr_t)frames % 4 == 0 && (uintptr_t)prev_stamp % 8 == 0 && (uintptr_t)stamps % 8 == 0 && (uintptr_t)ref % 8 == 0 &&
               (uintptr_t)last_t % 8 == 0, "%s: misaligned tensor", what);
  a.prev = prev, a.frames = frames, a.prev_stamp = prev_stamp, a.stamps = stamps, a.ref = ref, a.last_t = last_t;
  a.HW = (int64_t)H * W;
  a.refractory = refractory_ns;
  a.max_span = devo_esim_max_span_ns(H, W);
  a.c_neg = c_neg, a.c_pos = c_pos;
  a.T = T;
  a.shift = pixel_bits(a.HW) + 1;
  return DEVO_OK;
}

}  // namespace

extern "C" int64_t devo_esim_max_span_ns(int H, int W) {
  if (H < 1 || W < 1 || H > DEVO_ESIM_MAX_SIDE || W > DEVO_ESIM_MAX_SIDE) return 0;
  return (int64_t)1 << (62 - pixel_bits((int64_t)H * W));
}

extern "C" int devo_esim_count(const float* prev, const float* frames, const int64_t* prev_stamp, const int64_t* stamps, int T, int H, int W, const double* ref,
                               const int64_t* last_t, double c_neg, double c_pos, int64_t refractory_ns, int64_t* counts, int64_t* status_span, devo_stream_t stream) {
  EsimArgs a;
  const int rc = fill_args("esim_count", prev, frames, prev_stamp, stamps, T, H, W, ref, last_t, c_neg, c_pos, refractory_ns, a);
  if (rc != DEVO_OK) return rc;
  DEVO_REQUIRE(counts && status_span, "esim_count: null output");
  DEVO_REQUIRE((uintptr_t)counts % 8 == 0 && (uintptr_t)status_span % 8 == 0, "esim_count: misaligned output");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status_span, 0, 2 * sizeof(int64_t), s) != hipSuccess) return check_launch("esim_count (memset)");
  const dim3 grid((unsigned)((a.HW + TW - 1) / TW)), block(TW);
  if (refractory_ns > 0) hipLaunchKernelGGL(k_esim_count<true>, grid, block, 0, s, a, counts, (unsigned long long*)status_span);
  else hipLaunchKernelGGL(k_esim_count<false>, grid, block, 0, s, a, counts, (unsigned long long*)status_span);
  return check_launch("esim_count");
}

extern "C" int devo_esim_emit(const float* prev, const float* frames, const int64_t* prev_stamp, const int64_t* stamps, int T, int H, int W, const double* ref,
                              const int64_t* last_t, double c_neg, double c_pos, int64_t refractory_ns, const int64_t* offsets, int64_t total, int64_t* keys,
                              double* ref_out, int64_t* last_t_out, devo_stream_t stream) {
  EsimArgs a;
  const int rc = fill_args("esim_emit", prev, frames, prev_stamp, stamps, T, H, W, ref, last_t, c_neg, c_pos, refractory_ns, a);
  if (rc != DEVO_OK) return rc;
  DEVO_REQUIRE(total >= 0, "esim_emit: %lld events", (long long)total);
  DEVO_REQUIRE(offsets && ref_out && last_t_out && (keys || total == 0), "esim_emit: null tensor");
  DEVO_REQUIRE((uintptr_t)offsets % 8 == 0 && (uintptr_t)keys % 8 == 0 && (uintptr_t)ref_out % 8 == 0 && (uintptr_t)last_t_out % 8 == 0, "esim_emit: misaligned tensor");
  DEVO_REQUIRE((const void*)ref_out != (const void*)ref && (const void*)last_t_out != (const void*)last_t, "esim_emit: the new state must not alias the old one");
  const dim3 grid((unsigned)((a.HW + TW - 1) / TW)), block(TW);
  hipLaunchKernelGGL(k_esim_emit, grid, block, 0, (hipStream_t)stream, a, offsets, total, keys, ref_out, last_t_out);
  return check_launch("esim_emit");
}

extern "C" size_t devo_esim_sort_workspace_bytes(int64_t n, int H, int W, int64_t span_ns) {
  const unsigned end_bit = key_end_bit(H, W, span_ns);
  size_t bytes = 0;
  if (n <= 0 || end_bit == 0u || sort_keys(nullptr, bytes, nullptr, nullptr, n, end_bit, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return align_up(bytes);
}

extern "C" int devo_esim_sort_keys(const int64_t* keys, int64_t* sorted, int64_t n, int H, int W, int64_t span_ns, void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(n >= 0, "esim_sort_keys: %lld keys", (long long)n);
  const unsigned end_bit = key_end_bit(H, W, span_ns);
  DEVO_REQUIRE(end_bit != 0u, "esim_sort_keys: frame %d x %d with a span of %lld ns", H, W, (long long)span_ns);
  DEVO_REQUIRE(n == 0 || (keys && sorted && keys != sorted), "esim_sort_keys: null tensor, or sorting in place");
  DEVO_REQUIRE((uintptr_t)keys % 8 == 0 && (uintptr_t)sorted % 8 == 0 && (uintptr_t)ws % 16 == 0, "esim_sort_keys: misaligned tensor");
  if (n == 0) return DEVO_OK;
  size_t need = 0;
  if (sort_keys(nullptr, need, nullptr, nullptr, n, end_bit, (hipStream_t)stream) != hipSuccess) return check_launch("esim_sort_keys (workspace query)");
  if (need > ws_bytes || (need && !ws)) {
    set_error("esim_sort_keys: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return DEVO_ERR_WORKSPACE;
  }
  size_t given = ws_bytes;
  if (sort_keys(ws, given, keys, sorted, n, end_bit, (hipStream_t)stream) != hipSuccess) return check_launch("esim_sort_keys");
  return check_launch("esim_sort_keys");
}

extern "C" int devo_esim_decode(const int64_t* keys, int64_t n, int H, int W, const int64_t* first_stamp, int16_t* x, int16_t* y, int64_t* t, signed char* p,
                                devo_stream_t stream) {
  DEVO_REQUIRE(n >= 0, "esim_decode: %lld events", (long long)n);
  DEVO_REQUIRE(H >= 1 && W >= 1 && H <= DEVO_ESIM_MAX_SIDE && W <= DEVO_ESIM_MAX_SIDE, "esim_decode: frame %d x %d (sides 1 .. %d)", H, W, DEVO_ESIM_MAX_SIDE);
  DEVO_REQUIRE(first_stamp && (n == 0 || (keys && x && y && t && p)), "esim_decode: null tensor");
  DEVO_REQUIRE((uintptr_t)keys % 8 == 0 && (uintptr_t)first_stamp % 8 == 0 && (uintptr_t)x % 2 == 0 && (uintptr_t)y % 2 == 0 && (uintptr_t)t % 8 == 0,
               "esim_decode: misaligned tensor");
  if (n == 0) return DEVO_OK;
  hipLaunchKernelGGL(k_esim_decode, dim3(blocks_for(n, TB)), dim3(TB), 0, (hipStream_t)stream, keys, n, W, pixel_bits((int64_t)H * W) + 1, first_stamp, x, y, t,
                     (int8_t*)p);
  return check_launch("esim_decode");
}

extern "C" int devo_log_intensity(const unsigned char* images, int64_t n, const float* table, float* out, devo_stream_t stream) {
  DEVO_REQUIRE(n >= 0, "log_intensity: %lld pixels", (long long)n);
  DEVO_REQUIRE(table && (n == 0 || (images && out)), "log_intensity: null tensor");
  DEVO_REQUIRE((uintptr_t)table % 4 == 0 && (uintptr_t)out % 4 == 0, "log_intensity: misaligned tensor");
  if (n == 0) return DEVO_OK;
  const int64_t n4 = ((uintptr_t)images % 4 == 0 && (uintptr_t)out % 16 == 0) ? n >> 2 : 0;
  hipLaunchKernelGGL(k_log_intensity, dim3(blocks_for(n4 ? n4 : n, TB, 1 << 16)), dim3(TB), 0, (hipStream_t)stream, images, n, n4, table, out);
  return check_launch("log_intensity");
}
