// Stand-alone host check of the argument handling of devo_camera_undistort_points, devo_camera_distort_points and devo_image_remap
// (csrc/camera.hip) under AddressSanitizer and UBSan: every call below is refused before the launch, or has nothing to launch, so the
// program needs no GPU.  Host code only; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         devo_amd/csrc/camera.hip tools/san_camera.cpp -o /tmp/san_camera && /tmp/san_camera
// prints the refusals and "0 unexpected return codes" (exit status = the number of unexpected ones; a sanitizer report aborts).
#include <cstdio>
#include <cstdint>
#include <cstdarg>
#include "../include/devo_hip.h"
namespace devo { void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); } }
int main() {
  alignas(16) double buf[64];
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const double K[4] = {200.0, 201.0, 120.0, 90.0}, Kn[4] = {180.0, 180.0, 120.0, 90.0};
  const double K_nan[4] = {200.0, nan, 120.0, 90.0}, K_inf[4] = {200.0, 201.0, inf, 90.0}, K_zero[4] = {0.0, 201.0, 120.0, 90.0};
  const double d5[5] = {-0.3, 0.1, 0.001, 0.001, 0.0}, d_nan[5] = {-0.3, nan, 0.0, 0.0, 0.0};
  const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, R_nan[9] = {1, 0, 0, 0, nan, 0, 0, 0, 1};
  int bad = 0;
  using Fn = int (*)(const void*, int64_t, int, int, int, int, const double*, const double*, int, const double*, const double*, void*, int, int*, devo_stream_t);
  const Fn fns[2] = {&devo_camera_undistort_points, &devo_camera_distort_points};
  for (int f = 0; f < 2; ++f) {
    auto call = [&](const void* pts, int64_t n, int H, int W, int in_dt, int model, const double* k, const double* dist, int nd, const double* r, const double* kn, void* out,
                    int out_dt) { return fns[f](pts, n, H, W, in_dt, model, k, dist, nd, r, kn, out, out_dt, nullptr, nullptr); };
    bad += call(buf, -1, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;              // negative count
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, nullptr, DEVO_F64) != DEVO_ERR_ARG;          // no output
    bad += call(buf, 8, 0, 0, DEVO_F16, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;              // fp16 points
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, buf, DEVO_U8) != DEVO_ERR_ARG;               // uint8 output
    bad += call(nullptr, 8, 3, 3, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, buf, DEVO_F32) != DEVO_ERR_ARG;          // grid: H * W != n
    bad += call(nullptr, 0, 0, 4, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, buf, DEVO_F32) != DEVO_ERR_ARG;          // grid: empty
    bad += call(nullptr, -4, -2, 2, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, Kn, buf, DEVO_F32) != DEVO_ERR_ARG;        // grid: negative side
    bad += call(buf, 8, 0, 0, DEVO_F64, 3, K, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;                            // unknown model
    bad += call(buf, 8, 0, 0, DEVO_F64, -1, K, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, nullptr, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;        // no K
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K_nan, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;          // non-finite K
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K_inf, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K_zero, d5, 5, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;         // zero focal length
    for (int nd : {-1, 0, 1, 2, 3, 6, 8, 14})                                                                           // coefficient counts
      bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, nd, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;
    for (int nd : {-1, 0, 3, 5})
      bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_EQUIDISTANT, K, d5, nd, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;
    for (int nd : {-1, 1, 4, 5})
      bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_PINHOLE, K, d5, nd, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, nullptr, 4, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;          // no coefficients
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d_nan, 4, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;            // non-finite coefficient
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_EQUIDISTANT, K, d_nan, 4, R, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R_nan, Kn, buf, DEVO_F64) != DEVO_ERR_ARG;           // non-finite R
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, K_nan, buf, DEVO_F64) != DEVO_ERR_ARG;            // non-finite K_new
    bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, K_zero, buf, DEVO_F64) != DEVO_ERR_ARG;
    if (f == 1) bad += call(buf, 8, 0, 0, DEVO_F64, DEVO_CAM_RADTAN, K, d5, 5, R, nullptr, buf, DEVO_F64) != DEVO_ERR_ARG;   // distort needs K_new
    // valid arguments, nothing to do: accepted without a launch (the equidistant limit is computed on the way)
    bad += call(buf, 0, 0, 0, DEVO_F64, DEVO_CAM_EQUIDISTANT, K, d5, 4, nullptr, Kn, nullptr, DEVO_F32) != DEVO_OK;
    bad += call(buf, 0, 0, 0, DEVO_F32, DEVO_CAM_PINHOLE, K, nullptr, 0, R, Kn, buf, DEVO_F64) != DEVO_OK;
  }
  auto remap = [&](const void* img, int B, int H, int W, int C, int in_dt, const float* map, int Ho, int Wo, void* out, int out_dt) {
    return devo_image_remap(img, B, H, W, C, in_dt, map, Ho, Wo, out, out_dt, nullptr);
  };
  const float* map = (const float*)buf;
  bad += remap(nullptr, 1, 4, 4, 3, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;                                  // null tensors
  bad += remap(buf, 1, 4, 4, 3, DEVO_U8, nullptr, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 4, 3, DEVO_U8, map, 2, 2, nullptr, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 0, 4, 4, 3, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;                                      // sizes
  bad += remap(buf, 1, 0, 4, 3, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, -4, 3, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 4, 3, DEVO_U8, map, 0, 2, buf, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 4, 3, DEVO_U8, map, 2, -1, buf, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 1 << 24, 3, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;                                // a side fp32 cannot index
  bad += remap(buf, 1, 4, 4, 0, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;                                      // channels
  bad += remap(buf, 1, 4, 4, 5, DEVO_U8, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 4, 3, DEVO_F16, map, 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;                                     // dtypes
  bad += remap(buf, 1, 4, 4, 3, DEVO_F64, map, 2, 2, buf, DEVO_F32) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 4, 3, DEVO_U8, map, 2, 2, buf, DEVO_F64) != DEVO_ERR_ARG;
  bad += remap((char*)buf + 4, 1, 4, 4, 4, DEVO_F32, map, 2, 2, buf, DEVO_F32) != DEVO_ERR_ARG;                          // misaligned for whole-pixel loads
  bad += remap(buf, 1, 4, 4, 4, DEVO_U8, map, 2, 2, (char*)buf + 2, DEVO_U8) != DEVO_ERR_ARG;
  bad += remap(buf, 1, 4, 4, 1, DEVO_U8, (const float*)((char*)buf + 4), 2, 2, buf, DEVO_U8) != DEVO_ERR_ARG;
  printf("%d unexpected return codes\n", bad);
  return bad;
}
