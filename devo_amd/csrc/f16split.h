// fp32 operands on the fp16 matrix cores: the ONE copy of what linear.hip, linear_dw.hip, mlp2.hip, gemm_rs.hip, update.hip and corr_mm.h
// share — the exact hi / lo split, the power-of-two scales around it, the LDS-DMA request, the wave-local LDS hand-off, the reductions
// over a DPP row and the weight packers' column gather.  Every fp32 value x becomes the fp16 pair hi = rn(x), lo = rn(x - hi) (x = hi + lo to 2^-22 relative) and a product runs as
// hi lo' + lo hi' + hi hi' with fp32 accumulation.  Include at file scope (the header opens namespace devo itself).
#pragma once
#include <hip/hip_runtime.h>

namespace devo {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------- split
// Two fp32 values -> their fp16 hi halves packed in h, their lo halves packed in l: hi = rn(x), lo = rn(x - hi)
// (v_cvt_pk_f16_f32: two values per instruction; v_fma_mix: fp32 arithmetic on the fp16 hi.)
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
  // (mixlo keeps the destination's upper half, which mixhi then overwrites: no initialisation needed)
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(a));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(b));
}
// 8 fp32 values -> fp16 hi (8) and lo (8), as 16 bytes each
__device__ __forceinline__ void split8(const float (&x)[8], u4& hi, u4& lo) {
  unsigned h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; j++) split2(x[2 * j], x[2 * j + 1], h[j], l[j]);
  hi = u4{h[0], h[1], h[2], h[3]};
  lo = u4{l[0], l[1], l[2], l[3]};
}
// ... as MFMA operands
__device__ __forceinline__ void split8(const float (&x)[8], h8& hi, h8& lo) {
  u4 hv, lv;
  split8(x, hv, lv);
  hi = __builtin_bit_cast(h8, hv);
  lo = __builtin_bit_cast(h8, lv);
}

// ---------------------------------------------------------------------------------------------------------------- scales
// fp16 has 5 exponent bits, so operands are scaled by powers of two (exact) before the split and the product is scaled back.
constexpr int F16_SPLIT_EXP_TARGET = 8;           // a scale puts its reference magnitude into [2^8, 2^9)
constexpr float F16_SPLIT_RAISE = 16384.f;        // ... and is raised when a scaled value exceeds 2^14 (fp16's largest: 65504)

// biased exponent of the power of two that brings magnitude m into [2^TARGET, 2^(TARGET+1))
__device__ __forceinline__ int scale_exp(float m) {
  int e = (int)((__float_as_uint(m) >> 23) & 255u);
  e = e < 16 ? 16 : e;                             // zero / tiny reference: a finite scale (2^(8 + 111))
  return 127 + F16_SPLIT_EXP_TARGET + 127 - e;     // in [16, 246]
}
// the power of two with that biased exponent (clamped to the finite ones; 0 gives 0.f)
__device__ __forceinline__ float pow2_biased(int biased) { return __uint_as_float((unsigned)(biased < 0 ? 0 : (biased > 254 ? 254 : biased)) << 23); }

// ---------------------------------------------------------------------------------------------------------------- LDS-DMA
// 16 bytes per lane from (descriptor, per-lane offset, scalar offset) to lds_addr + 16 * lane (lds_addr goes through m0; an offset with
// bit 31 set is out of the descriptor's range: no access, zeros).  hipcc's waitcnt insertion does not know these requests: the caller
// counts its own vmcnt before it reads the bytes or lets a barrier publish them.
__device__ __forceinline__ void lds_dma16(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned soff, unsigned lds_addr) {
  lds_addr = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr);
  soff = (unsigned)__builtin_amdgcn_readfirstlane((int)soff);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(voff), "s"(rs), "s"(lds_addr), "s"(soff) : "memory");
}
// ... with no scalar offset (an immediate 0: routing this through the form above would cost an SGPR move per request)
__device__ __forceinline__ void lds_dma16(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned lds_addr) {
  lds_addr = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rs), "s"(lds_addr) : "memory");
}

// ---------------------------------------------------------------------------------------------------------------- within a wave
// Hand-off through LDS between the lanes of ONE wave: what the lanes wrote before it is what they read behind it.  A wave's LDS
// operations execute in order; the release / acquire pair around the wave barrier pins the compiler's.  (NOT corr.hip's wave_lds_fence,
// which is a seq_cst fence: the two compile differently.)
__device__ __forceinline__ void wave_lds_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum / maximum over the 16 lanes of a DPP row, result in all of them (row_ror 8, 4, 2, 1): no LDS round trips.
__device__ __forceinline__ float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false)));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- weight images
// One lane's 16 bytes of a packed fp16 B-operand image (k_pack_weight_f16, k_rs_pack_f16, k_mlp2_pack): the eight halves k0 .. k0 + 7 of
// column n of a weight whose element (n, k) lies at W[n * s_n + k * s_k], zeros past K.  (__half's only member is a _Float16: the packers
// pass their weight reinterpreted.)
__device__ __forceinline__ u4 gather8_f16(const _Float16* __restrict__ W, int64_t s_n, int64_t s_k, int n, int k0, int K) {
  h8 v;
#pragma unroll
  for (int e = 0; e < 8; e++) v[e] = k0 + e < K ? W[(int64_t)n * s_n + (int64_t)(k0 + e) * s_k] : (_Float16)0.f;
  return __builtin_bit_cast(u4, v);
}

}  // namespace devo
