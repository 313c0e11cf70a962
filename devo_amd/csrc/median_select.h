// The exact lower median of up to NT * KEYS fp32 values held in registers by ONE workgroup of NT threads (wave64, gfx950): a radix select
// over the order-preserving u32 image of fp32, four passes of 8 bits, integer counts only.  A pass is a 256-bin histogram in LDS (integer
// atomics) and a scan of it by the first wave.  This is the select of frames.hip's k_begin_frame, statement for statement; train_graph.hip
// (k_tg_frame) uses it from here.  frames.hip keeps its own copy: calling this function from k_begin_frame changed that kernel's
// generated code, and its bits were not to move.
#pragma once
#include <hip/hip_runtime.h>

namespace devo {

// fp32 -> u32 whose unsigned order is the order of the floats (-0 below +0), and back
__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// keys[s] is the key of value s * NT + tid (values at or beyond `count` are ignored); nan: this thread met a NaN.  Every thread of the
// workgroup calls this; all return the value of rank (count - 1) / 2, or NaN if any thread met one (torch.median).  One call site per kernel (the LDS is the function's).
template <int NT, int KEYS>
__device__ __forceinline__ float select_lower_median(const unsigned (&keys)[KEYS], bool nan, int count, int tid) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_rank;
  __shared__ int sh_nan;
  if (tid == 0) { sh_prefix = 0u; sh_rank = (unsigned)((count - 1) / 2); sh_nan = 0; }
  if (tid < 256) hist[tid] = 0u;
  __syncthreads();
  if (nan) sh_nan = 1;
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    const unsigned prefix = sh_prefix;
    const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
#pragma unroll
    for (int s = 0; s < KEYS; s++) {
      const int i = s * NT + tid;
      if (i < count && (keys[s] & mask) == prefix) atomicAdd(&hist[(keys[s] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {                                          // the first wave: lane l owns bins 4 l .. 4 l + 3
      const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
      const unsigned sum = h0 + h1 + h2 + h3;
      unsigned incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (tid >= o) incl += up;
      }
      const unsigned rank = sh_rank;
      unsigned excl = incl - sum;
      if (excl <= rank && rank < incl) {                     // exactly one lane
        unsigned bin = 4u * tid;
        if (rank >= excl + h0) { excl += h0; bin++; if (rank >= excl + h1) { excl += h1; bin++; if (rank >= excl + h2) { excl += h2; bin++; } } }
        sh_prefix = prefix | (bin << shift);
        sh_rank = rank - excl;
      }
    }
    __syncthreads();
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
  }
  return sh_nan ? __uint_as_float(0x7fc00000u) : fkey_value(sh_prefix);      // (torch.median: NaN if there is one)
}

}  // namespace devo
