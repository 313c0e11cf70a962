// The fp32 standard deviation of the voxel standardisation (devo/devo.py:450, utils/voxel_utils.py:22): sqrt(E[x^2] - mean^2) with the
// subtraction as ONE fused multiply-add.  events.hip (k_voxel_normalise) and frame_input.hip (a grid whose non-zero voxels are all equal)
// both call this, so the package has one answer where sigma is 0: the rounding error of the fp32 mean square — 0, a tiny number or NaN.
#pragma once
#include <hip/hip_runtime.h>

namespace devo {

__device__ __forceinline__ float voxel_sigma_f32(float mean_sq, float mean) { return sqrtf(__fmaf_rn(-mean, mean, mean_sq)); }

}  // namespace devo
