// The tail of a training sample on the GPU (devo/data_readers/base.py:356-371, EVSDDataset.__getitem__): the resize of
// transform_rescale (utils/transform_utils.py:9-28) and EVSDAugmentor's jitter, zoom and centre crop
// (devo/data_readers/augmentation.py:79-174), then the depth normalisation s = .7 * quantile(disps, .98).
//   * k_resample: bilinear (align_corners=False) or nearest resize of [B, C, H, W] to each sample's own (Hs, Ws), of which only
//     the crop window [y0, y0 + Hc) x [x0, x0 + Wc) is computed; the scaled image is never formed.  Optional jitter is added to
//     every source tap before the interpolation, from a caller's noise tensor or from a counter-based hash of (seed, source
//     index), so every output that reads a tap sees the same noise whatever the zoom or the launch shape.
//   * k_q_hist / k_q_count / k_q_apply: an exact per-sample quantile by radix select over the order-preserving bit image of the
//     floats (11 + 11 + 10 bits, per-wave LDS histograms, one global merge per workgroup), the next larger value, ATen's lerp,
//     then disps /= s and poses[..., :3] *= s.  Every pass is launched unconditionally and reads its state from the workspace,
//     which k_q_clear resets: the call has no host synchronisation and can be captured into a graph.
// Arithmetic is ATen's CPU arithmetic (torch 2.10, the build the reference's DataLoader workers run): its generic separable
// bilinear kernel and its scalar lerp are compiled with FMA contraction, so the FMAs below are written out where ATen's
// build forms them and nothing else may be contracted.
#include <algorithm>
#include <cmath>
#include "common.h"

#pragma clang fp contract(off)

namespace {

using namespace devo;

constexpr int RS_MAX = DEVO_RESAMPLE_MAX_BATCH;

struct ResampleSample { int Hs, Ws, y0, x0; unsigned s0, s1; };
struct ResampleArgs { ResampleSample s[RS_MAX]; };

__device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// u in [0, 1) with 24 bits, as torch.rand's float: a hash of (seed, source element index within the sample)
__device__ __forceinline__ float hash_uniform(unsigned s0, unsigned s1, unsigned idx) {
  const unsigned h = fmix32(fmix32(idx * 0x9e3779b1u ^ s0) + s1);
  return (float)(h >> 8) * 0x1p-24f;
}

// ATen compute_source_index_and_lambda (align_corners=False, no explicit scale): the source index is contracted into an FMA
__device__ __forceinline__ void lin_taps(int d, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  if (in == out) { i0 = i1 = d; l0 = 1.0f; l1 = 0.0f; return; }
  const float scale = (float)in / (float)out;
  float src = fmaf(scale, (float)d + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  i0 = min((int)floorf(src), in - 1);
  l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l0 = 1.0f - l1;
}

// ATen nearest_idx
__device__ __forceinline__ int nearest_tap(int d, int in, int out) {
  if (in == out) return d;
  if (out == 2 * in) return d >> 1;
  const float scale = (float)in / (float)out;
  return min((int)floorf((float)d * scale), in - 1);
}

// voxel_color_jitter's order: v + ((u - 0.5) * 2) * 1e-4, one fp32 rounding per op
__device__ __forceinline__ float jitter(float v, float u) { return v + ((u - 0.5f) * 2.0f) * 1e-4f; }

// one output per thread: block 64 x 4 over (x, y) of the crop, grid.z = (sample, channel) of this chunk
__global__ __launch_bounds__(256) void k_resample(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W, int Hc, int Wc,
                                                   int mode, const float* __restrict__ noise, int hashed, ResampleArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= Wc || y >= Hc) return;
  const int b = blockIdx.z / C;
  const ResampleSample p = a.s[b];
  const int64_t plane = (int64_t)H * W;
  const unsigned in_sample = (unsigned)((int64_t)(blockIdx.z - b * C) * plane);      // < 2^32 (checked on the host)
  const float* s = src + (int64_t)blockIdx.z * plane;
  const float* nz = noise ? noise + (int64_t)blockIdx.z * plane : nullptr;
  auto tap = [&](int iy, int ix) {
    const int64_t o = (int64_t)iy * W + ix;
    const float v = s[o];
    if (nz) return jitter(v, nz[o]);
    if (hashed) return jitter(v, hash_uniform(p.s0, p.s1, in_sample + (unsigned)o));
    return v;
  };
  const int sy = y + p.y0, sx = x + p.x0;
  float r;
  if (mode == DEVO_RESAMPLE_NEAREST) {
    r = tap(nearest_tap(sy, H, p.Hs), nearest_tap(sx, W, p.Ws));
  } else {
    int h0, h1, w0, w1;
    float lh0, lh1, lw0, lw1;
    lin_taps(sy, H, p.Hs, h0, h1, lh0, lh1);
    lin_taps(sx, W, p.Ws, w0, w1, lw0, lw1);
    // ATen's separable generic kernel: the inner dimension is W, the outer H; t0 * w0 + t1 * w1 contracted as fma(t0, w0, t1 * w1)
    const float t0 = fmaf(tap(h0, w0), lw0, tap(h0, w1) * lw1);
    const float t1 = fmaf(tap(h1, w0), lw0, tap(h1, w1) * lw1);
    r = fmaf(t0, lh0, t1 * lh1);
  }
  dst[(int64_t)blockIdx.z * Hc * Wc + (int64_t)y * Wc + x] = r;
}

// ---- quantile by radix select.  Workspace per sample (u32 words): hist1[2048] (key bits 31..21), hist2[2048] (20..10),
// hist3[1024] (9..0), then the state: [0] bin1, [1] rank left after bin1, [2] bin2, [3] rank left after bin2, [4] key of the lower
// order statistic, [5] count of keys <= it, [6] smallest key above it (cleared to ~0).
constexpr int QW_H1 = 0, QW_H2 = 2048, QW_H3 = 4096, QW_ST = 5120, QW_PER = 5128;

__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  if (f != f) return 0xffffffffu;                        // every NaN sorts last (torch.sort's order)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float fkey_value(unsigned k) {
  if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void k_q_clear(unsigned* __restrict__ ws, int B) {
  const int64_t n = (int64_t)B * QW_PER;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    ws[i] = (i % QW_PER == QW_ST + 6) ? 0xffffffffu : 0u;
}

// the rank in fp32 as torch.quantile forms it (q * last_index; the last index when a NaN is present), and its two integer ranks
struct Rank { float r; unsigned lo, hi; };
__device__ __forceinline__ Rank quantile_rank(int64_t n, float q, bool nan) {
  const int64_t last = n - 1;
  Rank k;
  k.r = nan ? (float)last : q * (float)last;
  const int64_t lo = (int64_t)k.r, hi = (int64_t)ceilf(k.r);
  k.lo = (unsigned)std::min<int64_t>(std::max<int64_t>(lo, 0), last);
  k.hi = (unsigned)std::min<int64_t>(std::max<int64_t>(hi, 0), last);
  return k;
}

// the bin of `hist` (nbins = 1024 or 2048) that holds rank k, and the rank within it; 256 threads, every thread gets the result
__device__ void select_bin(const unsigned* __restrict__ hist, int nbins, unsigned k, unsigned& bin, unsigned& krem) {
  __shared__ unsigned s_sum[256];
  __shared__ unsigned s_res[2];
  if (threadIdx.x == 0) { s_res[0] = 0u; s_res[1] = 0u; }
  const int per = nbins / 256, t = threadIdx.x;
  unsigned c[8], tot = 0;
  for (int j = 0; j < per; j++) { c[j] = hist[t * per + j]; tot += c[j]; }
  s_sum[t] = tot;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {                 // inclusive scan
    const unsigned v = t >= off ? s_sum[t - off] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  unsigned below = s_sum[t] - tot;
  if (k >= below && k < s_sum[t]) {
    for (int j = 0; j < per; j++) {
      if (k < below + c[j]) { s_res[0] = (unsigned)(t * per + j); s_res[1] = k - below; break; }
      below += c[j];
    }
  }
  __syncthreads();
  bin = s_res[0];
  krem = s_res[1];
  __syncthreads();
}

// one histogram pass over sample b's keys whose top bits equal `prefix` (shift_hi: bits above the digit; shift: the digit's low bit)
template <bool VEC>
__device__ void hist_pass(const float* __restrict__ v, int64_t n, int bps, int blk, unsigned* __restrict__ ghist, int nbins, int shift,
                          int shift_hi, unsigned prefix) {
  __shared__ unsigned s_h[4][2048];
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * 2048; i += 256) (&s_h[0][0])[i] = 0u;
  __syncthreads();
  const unsigned mask = (unsigned)nbins - 1u;
  auto add = [&](float f) {
    const unsigned k = fkey(f);
    if (shift_hi >= 32 || (k >> shift_hi) == prefix) atomicAdd(&s_h[wave][(k >> shift) & mask], 1u);
  };
  if (VEC) {
    const int64_t nq = n >> 2;
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < nq; i += (int64_t)bps * 256) {
      const float4 q = reinterpret_cast<const float4*>(v)[i];
      add(q.x); add(q.y); add(q.z); add(q.w);
    }
  } else {
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < n; i += (int64_t)bps * 256) add(v[i]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256) {
    const unsigned c = (s_h[0][i] + s_h[1][i]) + (s_h[2][i] + s_h[3][i]);
    if (c) atomicAdd(ghist + i, c);
  }
}

// pass 1 (digit 31..21), pass 2 (20..10, after bin1) or pass 3 (9..0, after bin2); grid = B * bps
template <bool VEC>
__global__ __launch_bounds__(256) void k_q_hist(const float* __restrict__ disps, int64_t n, int bps, float q, int pass, unsigned* __restrict__ ws) {
  const int b = blockIdx.x / bps, blk = blockIdx.x - b * bps;
  const float* v = disps + (int64_t)b * n;
  unsigned* w = ws + (int64_t)b * QW_PER;
  if (pass == 1) {
    hist_pass<VEC>(v, n, bps, blk, w + QW_H1, 2048, 21, 32, 0u);
  } else if (pass == 2) {
    const Rank k = quantile_rank(n, q, w[QW_H1 + 2047] != 0u);        // bin 2047 of the top digit holds exactly the NaNs
    unsigned bin1, k1;
    select_bin(w + QW_H1, 2048, k.lo, bin1, k1);
    if (blk == 0 && threadIdx.x == 0) { w[QW_ST + 0] = bin1; w[QW_ST + 1] = k1; }
    hist_pass<VEC>(v, n, bps, blk, w + QW_H2, 2048, 10, 21, bin1);
  } else {
    const unsigned bin1 = w[QW_ST + 0], k1 = w[QW_ST + 1];
    unsigned bin2, k2;
    select_bin(w + QW_H2, 2048, k1, bin2, k2);
    if (blk == 0 && threadIdx.x == 0) { w[QW_ST + 2] = bin2; w[QW_ST + 3] = k2; }
    hist_pass<VEC>(v, n, bps, blk, w + QW_H3, 1024, 0, 10, (bin1 << 11) | bin2);
  }
}

// the lower order statistic's key from hist3, then the count of keys <= it and the smallest key above it
template <bool VEC>
__global__ __launch_bounds__(256) void k_q_count(const float* __restrict__ disps, int64_t n, int bps, unsigned* __restrict__ ws) {
  __shared__ unsigned s_c[4], s_m[4];
  const int b = blockIdx.x / bps, blk = blockIdx.x - b * bps;
  const float* v = disps + (int64_t)b * n;
  unsigned* w = ws + (int64_t)b * QW_PER;
  unsigned bin3, k3;
  select_bin(w + QW_H3, 1024, w[QW_ST + 3], bin3, k3);
  const unsigned key = (w[QW_ST + 0] << 21) | (w[QW_ST + 2] << 10) | bin3;
  if (blk == 0 && threadIdx.x == 0) w[QW_ST + 4] = key;
  unsigned cnt = 0, mn = 0xffffffffu;
  auto add = [&](float f) {
    const unsigned k = fkey(f);
    cnt += k <= key ? 1u : 0u;
    if (k > key) mn = min(mn, k);
  };
  if (VEC) {
    const int64_t nq = n >> 2;
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < nq; i += (int64_t)bps * 256) {
      const float4 q = reinterpret_cast<const float4*>(v)[i];
      add(q.x); add(q.y); add(q.z); add(q.w);
    }
  } else {
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < n; i += (int64_t)bps * 256) add(v[i]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { cnt += __shfl_xor(cnt, off); mn = min(mn, (unsigned)__shfl_xor(mn, off)); }
  if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = cnt; s_m[threadIdx.x >> 6] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(w + QW_ST + 5, (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]));
    atomicMin(w + QW_ST + 6, min(min(s_m[0], s_m[1]), min(s_m[2], s_m[3])));
  }
}

// s = factor * lerp(lower, upper, rank - lower rank) (ATen's lerp, contracted as its CPU build contracts it), then
// disps /= s, poses[..., :3] *= s and s_out[b] = s
template <bool VEC>
__global__ __launch_bounds__(256) void k_q_apply(float* __restrict__ disps, int64_t n, int bps, float q, float factor, float* __restrict__ poses,
                                                 int P, int pose_stride, float* __restrict__ s_out, const unsigned* __restrict__ ws) {
  const int b = blockIdx.x / bps, blk = blockIdx.x - b * bps;
  const unsigned* w = ws + (int64_t)b * QW_PER;
  const Rank k = quantile_rank(n, q, w[QW_H1 + 2047] != 0u);
  const unsigned key = w[QW_ST + 4];
  const float lo = fkey_value(key);
  const float hi = (k.hi == k.lo || w[QW_ST + 5] > k.hi) ? lo : fkey_value(w[QW_ST + 6]);
  const float wt = k.r - (float)k.lo;
  const float d = hi - lo;
  const float qv = fabsf(wt) < 0.5f ? fmaf(wt, d, lo) : fmaf(-d, 1.0f - wt, hi);
  const float s = factor * qv;
  float* v = disps + (int64_t)b * n;
  if (blk == 0) {
    if (threadIdx.x == 0 && s_out) s_out[b] = s;
    if (poses)
      for (int i = threadIdx.x; i < 3 * P; i += 256) {
        float* p = poses + ((int64_t)b * P + i / 3) * pose_stride + i % 3;
        *p = *p * s;
      }
  }
  if (VEC) {
    const int64_t nq = n >> 2;
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < nq; i += (int64_t)bps * 256) {
      float4 t = reinterpret_cast<float4*>(v)[i];
      t.x = __fdiv_rn(t.x, s); t.y = __fdiv_rn(t.y, s); t.z = __fdiv_rn(t.z, s); t.w = __fdiv_rn(t.w, s);
      reinterpret_cast<float4*>(v)[i] = t;
    }
  } else {
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < n; i += (int64_t)bps * 256) v[i] = __fdiv_rn(v[i], s);
  }
}

}  // namespace

extern "C" {

int devo_voxel_resample(const float* src, float* dst, int B, int C, int H, int W, int Hc, int Wc, const int* params, int mode, const float* noise,
                        const uint64_t* seeds, devo_stream_t stream) {
  DEVO_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0, "devo_voxel_resample: bad sizes");
  DEVO_REQUIRE(mode == DEVO_RESAMPLE_BILINEAR || mode == DEVO_RESAMPLE_NEAREST, "devo_voxel_resample: unknown mode %d", mode);
  DEVO_REQUIRE((int64_t)C * H * W <= (int64_t)UINT32_MAX, "devo_voxel_resample: more than 2^32 elements per sample");
  DEVO_REQUIRE((int64_t)RS_MAX * C <= 65535, "devo_voxel_resample: C = %d is too large", C);
  if (B == 0) return DEVO_OK;
  DEVO_REQUIRE(src != nullptr && dst != nullptr && params != nullptr && src != dst, "devo_voxel_resample: null or aliased buffers");
  for (int b = 0; b < B; b++) {
    const int* p = params + 4 * b;
    DEVO_REQUIRE(p[0] > 0 && p[1] > 0 && p[2] >= 0 && p[3] >= 0 && (int64_t)p[2] + Hc <= p[0] && (int64_t)p[3] + Wc <= p[1],
                 "devo_voxel_resample: sample %d: the crop %dx%d at (%d, %d) does not fit the scaled size %dx%d", b, Hc, Wc, p[2], p[3], p[0], p[1]);
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t in_per = (int64_t)C * H * W, out_per = (int64_t)C * Hc * Wc;
  for (int b0 = 0; b0 < B; b0 += RS_MAX) {
    const int nb = std::min(RS_MAX, B - b0);
    ResampleArgs a;
    for (int j = 0; j < nb; j++) {
      const int* p = params + 4 * (b0 + j);
      const uint64_t sd = seeds ? seeds[b0 + j] : 0ull;
      a.s[j] = ResampleSample{p[0], p[1], p[2], p[3], (unsigned)sd, (unsigned)(sd >> 32)};
    }
    const dim3 grid((unsigned)((Wc + 63) / 64), (unsigned)((Hc + 3) / 4), (unsigned)(nb * C));
    hipLaunchKernelGGL(k_resample, grid, dim3(256), 0, st, src + b0 * in_per, dst + b0 * out_per, C, H, W, Hc, Wc, mode,
                       noise ? noise + b0 * in_per : nullptr, (noise == nullptr && seeds != nullptr) ? 1 : 0, a);
    const int rc = check_launch("devo_voxel_resample");
    if (rc != DEVO_OK) return rc;
  }
  return DEVO_OK;
}

size_t devo_depth_normalise_workspace_bytes(int B) { return sizeof(unsigned) * QW_PER * (size_t)(B > 0 ? B : 1); }

int devo_depth_normalise(float* disps, int64_t n, int B, float* poses, int P, int pose_stride, float q, float factor, float* s_out, void* ws,
                         size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(B >= 0 && n > 0 && n <= INT32_MAX && P >= 0, "devo_depth_normalise: bad sizes");
  DEVO_REQUIRE(poses == nullptr || pose_stride >= 3, "devo_depth_normalise: a pose has at least 3 translation entries");
  DEVO_REQUIRE(q >= 0.0f && q <= 1.0f, "devo_depth_normalise: q must lie in [0, 1]");
  if (B == 0) return DEVO_OK;
  DEVO_REQUIRE(disps != nullptr, "devo_depth_normalise: null disparities");
  if (ws == nullptr || ws_bytes < devo_depth_normalise_workspace_bytes(B)) { set_error("devo_depth_normalise: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  unsigned* w = (unsigned*)ws;
  const bool vec = (n % 4 == 0) && ((uintptr_t)disps % 16 == 0);
  const int bps = std::min(blocks_for(n, 256 * 32, 512), std::max(4096 / B, 1));
  const dim3 grid((unsigned)((int64_t)B * bps)), block(256);
  hipLaunchKernelGGL(k_q_clear, dim3((unsigned)blocks_for((int64_t)B * QW_PER, 256, 1024)), block, 0, st, w, B);
  for (int pass = 1; pass <= 3; pass++) {
    if (vec) hipLaunchKernelGGL(k_q_hist<true>, grid, block, 0, st, (const float*)disps, n, bps, q, pass, w);
    else hipLaunchKernelGGL(k_q_hist<false>, grid, block, 0, st, (const float*)disps, n, bps, q, pass, w);
  }
  if (vec) hipLaunchKernelGGL(k_q_count<true>, grid, block, 0, st, (const float*)disps, n, bps, w);
  else hipLaunchKernelGGL(k_q_count<false>, grid, block, 0, st, (const float*)disps, n, bps, w);
  if (vec) hipLaunchKernelGGL(k_q_apply<true>, grid, block, 0, st, disps, n, bps, q, factor, poses, P, pose_stride, s_out, (const unsigned*)w);
  else hipLaunchKernelGGL(k_q_apply<false>, grid, block, 0, st, disps, n, bps, q, factor, poses, P, pose_stride, s_out, (const unsigned*)w);
  return check_launch("devo_depth_normalise");
}

}  // extern "C"
