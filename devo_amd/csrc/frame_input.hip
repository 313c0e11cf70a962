// What DEVO.__call__ does to a new voxel grid before the Patchifier sees it (devo/devo.py:406-467: the event-density gate of the first
// frame, the normalisation, the 346-column crop), and the median of the motion probe (:256), wave64, gfx950.  The reference runs them
// with `.item()` round trips and boolean-mask indexing on every frame; here a frame's input is two launches and the probe's median one,
// and what the host may want to look at lands in a pinned record.  No float atomics: every floating-point sum is an fp64 sum in an
// order fixed by the size of the input alone, so a result is the same bits from run to run.
//   * k_input_stats<T>: a grid that depends on the number of voxels only; every workgroup reduces its strided share to one Partial
//     {count of non-zeros, sum, sum of squares, largest positive, largest -negative, smallest and largest non-zero}.
//   * k_input_apply<T>: every workgroup folds the (at most 256) partials again, in the same order, so all of them hold the same
//     statistics without a launch in between; workgroup 0 writes the record; then out = norm(x) over the cropped grid.
//     std: mean and sigma are formed in fp64 and rounded once; the difference and the quotient are fp32.  Where all non-zero voxels are
//     EQUAL (sigma = 0) the statistics are formed by the function events.hip's k_voxel_normalise forms them with (voxel_sigma.h: fp32, the
//     variance by one fused multiply-add), so the package has one answer for that input (see input_sigma_equal).
//   * k_probe_median<T>: ONE workgroup; the norms of delta [M, 2] (exact products and one rounding each for the sum and the root in
//     fp64, rounded to fp32: the values `delta.norm(dim=-1).float()` holds), the exact select of median_select.h for the lower middle
//     value, one counting pass for the upper one, their mean formed in fp64 and rounded once (torch.quantile(., 0.5): linear interpolation).
#include <cmath>
#include <hip/hip_fp16.h>
#include "common.h"
#include "median_select.h"
#include "voxel_sigma.h"

namespace {

using namespace devo;

constexpr int TB = 256;
constexpr int IN_MAX_PARTS = 256;                 // partials of k_input_stats: one per thread of a workgroup of k_input_apply
constexpr int IN_PER_BLOCK = TB * 32;             // voxels to a workgroup of k_input_stats before the grid stops growing
constexpr int PM_KEYS = DEVO_PROBE_MEDIAN_MAX / TB;
static_assert(PM_KEYS * TB == DEVO_PROBE_MEDIAN_MAX, "probe median bound");

struct Partial { double cnt, sum, sq; float pmax, nmax, vmin, vmax; };

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }

__device__ __forceinline__ void fold(Partial& a, const Partial& b) {
  a.cnt += b.cnt; a.sum += b.sum; a.sq += b.sq;
  a.pmax = fmaxf(a.pmax, b.pmax); a.nmax = fmaxf(a.nmax, b.nmax); a.vmin = fminf(a.vmin, b.vmin); a.vmax = fmaxf(a.vmax, b.vmax);
}
__device__ __forceinline__ Partial empty_partial() { return Partial{0.0, 0.0, 0.0, 0.0f, 0.0f, INFINITY, -INFINITY}; }

// every thread of the workgroup calls this; all return the fold of all 256 values: a butterfly inside each wave (a + b == b + a: the
// lanes agree bit for bit), then the four waves' values in their order
__device__ __forceinline__ Partial block_fold(Partial p) {
  __shared__ Partial s_red[TB / 64];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Partial o;
    o.cnt = __shfl_xor(p.cnt, off); o.sum = __shfl_xor(p.sum, off); o.sq = __shfl_xor(p.sq, off);
    o.pmax = __shfl_xor(p.pmax, off); o.nmax = __shfl_xor(p.nmax, off); o.vmin = __shfl_xor(p.vmin, off); o.vmax = __shfl_xor(p.vmax, off);
    fold(p, o);
  }
  __syncthreads();                                 // (a second call in one kernel: the first one's reads are done)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = p;
  __syncthreads();
  Partial r = s_red[0];
#pragma unroll
  for (int w = 1; w < TB / 64; w++) fold(r, s_red[w]);
  return r;
}

template <typename T>
__global__ __launch_bounds__(TB) void k_input_stats(const T* __restrict__ v, int64_t n, Partial* __restrict__ parts) {
  Partial p = empty_partial();
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    const float a = to_f32(v[i]);
    if (a != 0.0f) {
      p.cnt += 1.0; p.sum += (double)a; p.sq += (double)a * (double)a;
      if (a > 0.0f) p.pmax = fmaxf(p.pmax, a);
      if (a < 0.0f) p.nmax = fmaxf(p.nmax, -a);
      p.vmin = fminf(p.vmin, a); p.vmax = fmaxf(p.vmax, a);
    }
  }
  p = block_fold(p);
  if (threadIdx.x == 0) parts[blockIdx.x] = p;
}

// sigma of a grid whose non-zero voxels all equal `a`, as events.std computes it (voxel_sigma.h, the expression of k_voxel_normalise:
// mean = a exactly, mean square = fl32(a^2)): the rounding error of a^2, so 0, a tiny positive number or NaN; the quotient
// (a - mean) / sd is then 0 or NaN
__device__ __forceinline__ float input_sigma_equal(float a) { return voxel_sigma_f32((float)((double)a * (double)a), a); }

struct InputArgs {
  const void* vox; float* out; const Partial* parts; double* record;
  int64_t n_in, n_out;
  int parts_n, W, Wout, x0, norm;
};

template <typename T>
__global__ __launch_bounds__(TB) void k_input_apply(InputArgs a) {
  Partial p = threadIdx.x < a.parts_n ? a.parts[threadIdx.x] : empty_partial();
  p = block_fold(p);
  // c0, c1: mean and sigma (std), largest positive and largest -negative (rescale)
  float c0 = 0.0f, c1 = 0.0f;
  const bool any = p.cnt > 0.0;
  if (a.norm == DEVO_INPUT_STD && any) {
    if (p.vmin == p.vmax) {
      c0 = p.vmin;
      c1 = input_sigma_equal(p.vmin);
    } else {
      const double mean = p.sum / p.cnt;
      c0 = (float)mean;
      c1 = (float)sqrt(p.sq / p.cnt - mean * mean);
    }
  } else if (a.norm == DEVO_INPUT_RESCALE) {
    c0 = p.pmax; c1 = p.nmax;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.record[0] = p.cnt; a.record[1] = (double)a.n_in; a.record[2] = (double)c0; a.record[3] = (double)c1;
  }
  const T* v = (const T*)a.vox;
  const bool std_ = a.norm == DEVO_INPUT_STD && any;           // (without a non-zero voxel the input is returned as it is, devo.py:444)
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < a.n_out; i += (int64_t)gridDim.x * TB) {
    const int64_t row = i / a.Wout;
    const float x = to_f32(v[row * a.W + (i - row * a.Wout) + a.x0]);
    float y = x;
    if (std_) {
      const float q = __fdiv_rn(x - c0, c1);
      y = x != 0.0f ? q : 0.0f * q;                            // mask * (...), devo.py:452
    } else if (a.norm == DEVO_INPUT_RESCALE) {
      y = x > 0.0f ? __fdiv_rn(x, c0) : x < 0.0f ? __fdiv_rn(x, c1) : x;      // x / -vx_min: the negation is exact
    }
    a.out[i] = y;
  }
}

template <typename T>
__global__ __launch_bounds__(TB) void k_probe_median(const T* __restrict__ delta, int M, float* __restrict__ out) {
  __shared__ unsigned s_cnt[TB / 64], s_min[TB / 64];
  const int tid = threadIdx.x;
  unsigned keys[PM_KEYS];
  bool nan = false;
#pragma unroll
  for (int s = 0; s < PM_KEYS; s++) {
    const int i = s * TB + tid;
    keys[s] = 0u;
    if (i < M) {
      const double x = (double)to_f32(delta[2 * i]), y = (double)to_f32(delta[2 * i + 1]);
      const float r = (float)sqrt(x * x + y * y);
      nan |= r != r;
      keys[s] = fkey(r);
    }
  }
  const float lo = select_lower_median<TB, PM_KEYS>(keys, nan, M, tid);       // rank (M - 1) / 2
  // the value of rank M / 2: `lo` again if enough values are <= lo, else the smallest value above it
  const unsigned klo = fkey(lo);
  unsigned cnt = 0u, mn = 0xffffffffu;
#pragma unroll
  for (int s = 0; s < PM_KEYS; s++) {
    if (s * TB + tid < M) {
      if (keys[s] <= klo) cnt++; else mn = min(mn, keys[s]);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { cnt += __shfl_xor(cnt, off); mn = min(mn, (unsigned)__shfl_xor(mn, off)); }
  if ((tid & 63) == 0) { s_cnt[tid >> 6] = cnt; s_min[tid >> 6] = mn; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TB / 64; w++) { cnt += s_cnt[w]; mn = min(mn, s_min[w]); }
    float r = lo;
    if (lo == lo && (unsigned)(M / 2) >= cnt) r = (float)(0.5 * ((double)lo + (double)fkey_value(mn)));
    out[0] = r;
  }
}

inline int stats_blocks(int64_t n) { return blocks_for(n, IN_PER_BLOCK, IN_MAX_PARTS); }

}  // namespace

extern "C" {

size_t devo_odom_input_workspace_bytes(int64_t numel) { return numel <= 0 ? 0 : align_up((size_t)stats_blocks(numel) * sizeof(Partial)); }

int devo_odom_input(const void* vox, int dtype, int bins, int H, int W, int norm, float* out, void* ws, size_t ws_bytes, double* record,
                     devo_stream_t stream) {
  DEVO_REQUIRE(dtype == DEVO_F32 || dtype == DEVO_F16, "devo_odom_input: the voxel grid is fp32 or fp16");
  DEVO_REQUIRE(bins > 0 && H > 0 && W > 0, "devo_odom_input: bad sizes (%d, %d, %d)", bins, H, W);
  DEVO_REQUIRE(norm == DEVO_INPUT_NONE || norm == DEVO_INPUT_RESCALE || norm == DEVO_INPUT_STD, "devo_odom_input: unknown normalisation %d", norm);
  DEVO_REQUIRE(vox && out && record, "devo_odom_input: null buffers");
  const int64_t n_in = (int64_t)bins * H * W;
  DEVO_REQUIRE(ws && ws_bytes >= devo_odom_input_workspace_bytes(n_in), "devo_odom_input: workspace too small");
  const bool crop = W == DEVO_INPUT_CROP_WIDTH;                // devo.py:466-467
  const int Wout = crop ? W - 2 : W;
  const int nb = stats_blocks(n_in);
  const InputArgs a{vox, out, (const Partial*)ws, record, n_in, (int64_t)bins * H * Wout, nb, W, Wout, crop ? 1 : 0, norm};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks_for(a.n_out, TB * 4, 2048)), block(TB);
  if (dtype == DEVO_F32) {
    hipLaunchKernelGGL(k_input_stats<float>, dim3(nb), block, 0, st, (const float*)vox, n_in, (Partial*)ws);
    hipLaunchKernelGGL(k_input_apply<float>, grid, block, 0, st, a);
  } else {
    hipLaunchKernelGGL(k_input_stats<__half>, dim3(nb), block, 0, st, (const __half*)vox, n_in, (Partial*)ws);
    hipLaunchKernelGGL(k_input_apply<__half>, grid, block, 0, st, a);
  }
  return check_launch("devo_odom_input");
}

int devo_odom_probe_median(const void* delta, int dtype, int M, float* out, devo_stream_t stream) {
  DEVO_REQUIRE(dtype == DEVO_F32 || dtype == DEVO_F16, "devo_odom_probe_median: delta is fp32 or fp16");
  DEVO_REQUIRE(delta && out, "devo_odom_probe_median: null buffers");
  DEVO_REQUIRE(M >= 1, "devo_odom_probe_median: no values");
  if (M > DEVO_PROBE_MEDIAN_MAX) {
    set_error("devo_odom_probe_median: the median over %d values exceeds the supported %d", M, DEVO_PROBE_MEDIAN_MAX);
    return DEVO_ERR_UNSUPPORTED;
  }
  if (dtype == DEVO_F32) hipLaunchKernelGGL(k_probe_median<float>, dim3(1), dim3(TB), 0, (hipStream_t)stream, (const float*)delta, M, out);
  else hipLaunchKernelGGL(k_probe_median<__half>, dim3(1), dim3(TB), 0, (hipStream_t)stream, (const __half*)delta, M, out);
  return check_launch("devo_odom_probe_median");
}

}  // extern "C"
