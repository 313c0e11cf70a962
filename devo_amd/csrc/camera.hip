// Camera models (devo_amd/camera.py; include/devo_hip.h): what the reference obtains from OpenCV at load time — the rectification map of an
// event sensor (utils/load_utils.py:675-702, :1041-1058; scripts/pp_*.py), the undistortion of points, and per frame the undistortion of
// RGB images (devo/stream.py:26,74; evals/eval_rgb/eval_tum.py:53).
//   k_cam_undistort   raw pixel -> ideal pixel: normalise with K, invert the lens model, rotate, project with K_new.  fp64 throughout: it runs
//                     once per scene on at most ~1e6 points, the inverse of a strongly distorted model is ill-conditioned near the image
//                     border, and the map decides where every event of the scene votes.
//   k_cam_distort     ideal pixel -> raw pixel (closed form): the source map of image undistortion.
//   k_remap<...>      bilinear gather, one thread per output pixel for all channels and all B images: the map is read once per pixel.
// The calibration (K, the coefficients, R, K_new, the equidistant limit) travels by value in the kernel arguments.
#include <cmath>
#include "common.h"

namespace {
using namespace devo;

constexpr int TB = 256;

struct CamArgs {
  double fx, fy, cx, cy;        // K
  double k[5];                  // radtan: k1 k2 p1 p2 k3; equidistant: k1..k4
  double R[9];                  // row-major; the identity when absent
  double nfx, nfy, ncx, ncy;    // K_new; (1, 1, 0, 0) when absent (normalised coordinates)
  double theta_lim, theta_dmax; // equidistant: the monotone range of theta_d(theta) and its image
  int model, has_R;
};

__device__ __forceinline__ double eq_poly(const double* k, double t2) { return 1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))); }
__device__ __forceinline__ double eq_dpoly(const double* k, double t2) {
  return 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * 9.0 * k[3])));
}

// radtan forward model at (x, y) with its Jacobian
__device__ __forceinline__ void radtan_fwd(const double* k, double x, double y, double& xd, double& yd, double& j11, double& j12, double& j21, double& j22) {
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  const double r2 = x * x + y * y;
  const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
  const double D = k1 + r2 * (2.0 * k2 + r2 * 3.0 * k3);          // d rad / d r2
  xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
  yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
  j11 = rad + 2.0 * x * x * D + 2.0 * p1 * y + 6.0 * p2 * x;
  j12 = 2.0 * x * y * D + 2.0 * p1 * x + 2.0 * p2 * y;
  j21 = j12;
  j22 = rad + 2.0 * y * y * D + 6.0 * p1 * y + 2.0 * p2 * x;
}

// Newton on the two-dimensional forward model from the distorted point; valid = converged with det J > 0 at every iterate (the principal branch)
__device__ bool radtan_inverse(const double* k, double xd, double yd, double& x, double& y) {
  x = xd;
  y = yd;
  for (int it = 0; it < 30; ++it) {
    double fx, fy, a, b, c, d;
    radtan_fwd(k, x, y, fx, fy, a, b, c, d);
    const double det = a * d - b * c;
    if (!(det > 0.0)) return false;
    const double ex = fx - xd, ey = fy - yd;
    const double dx = (d * ex - b * ey) / det, dy = (a * ey - c * ex) / det;
    x -= dx;
    y -= dy;
    if (fabs(dx) + fabs(dy) < 1e-12) return true;
  }
  return false;
}

// theta (1 + k1 theta^2 + ...) = theta_d on [0, theta_lim], where the left side rises: Newton kept inside a shrinking bracket
__device__ double equi_inverse(const double* k, double theta_d, double theta_lim) {
  double lo = 0.0, hi = theta_lim;
  double t = fmin(theta_d, theta_lim);
  for (int it = 0; it < 64; ++it) {
    const double t2 = t * t;
    const double f = t * eq_poly(k, t2) - theta_d;
    if (f == 0.0) break;
    if (f > 0.0) hi = t; else lo = t;
    double tn = t - f / eq_dpoly(k, t2);
    if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
    const double step = fabs(tn - t);
    t = tn;
    if (step <= 2.3e-16 * t || !(hi > lo)) break;
  }
  return t;
}

template <typename T>
__device__ __forceinline__ void load_point(const void* pts, int64_t i, int W, double& u, double& v) {
  if (pts) {
    const T* p = (const T*)pts + 2 * i;
    u = (double)p[0];
    v = (double)p[1];
  } else {
    u = (double)(i % W);
    v = (double)(i / W);
  }
}

template <typename T>
__device__ __forceinline__ void store_point(void* out, int64_t i, double u, double v) {
  if constexpr (sizeof(T) == 8) ((double2*)out)[i] = make_double2(u, v);
  else ((float2*)out)[i] = make_float2((float)u, (float)v);
}

// one integer atomic per wave that has an invalid point
__device__ __forceinline__ void count_invalid(bool invalid, int* counter) {
  const unsigned long long m = __ballot(invalid);
  if (counter && m && invalid && (int)(__lane_id()) == __ffsll((long long)m) - 1) atomicAdd(counter, __popcll(m));
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(TB) k_cam_undistort(const void* pts, int64_t n, int W, CamArgs a, void* out, int* invalid_count) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const bool active = i < n;
  bool ok = true;
  double x = 0.0, y = 0.0;
  if (active) {
    double u, v;
    load_point<TI>(pts, i, W, u, v);
    const double xd = (u - a.cx) / a.fx, yd = (v - a.cy) / a.fy;
    if (a.model == DEVO_CAM_RADTAN) {
      ok = radtan_inverse(a.k, xd, yd, x, y);
    } else if (a.model == DEVO_CAM_EQUIDISTANT) {
      const double td = sqrt(xd * xd + yd * yd);
      ok = td < a.theta_dmax;                                     // (a NaN input is invalid too)
      if (ok && td > 0.0) {
        const double s = tan(equi_inverse(a.k, td, a.theta_lim)) / td;
        x = xd * s;
        y = yd * s;
      }
    } else {
      x = xd;
      y = yd;
      ok = x == x && y == y;
    }
    if (ok) {
      if (a.has_R) {
        const double X = a.R[0] * x + a.R[1] * y + a.R[2], Y = a.R[3] * x + a.R[4] * y + a.R[5], Z = a.R[6] * x + a.R[7] * y + a.R[8];
        x = X / Z;
        y = Y / Z;
      }
      x = a.nfx * x + a.ncx;
      y = a.nfy * y + a.ncy;
    } else {
      x = y = __builtin_nan("");
    }
    store_point<TO>(out, i, x, y);
  }
  count_invalid(active && !ok, invalid_count);
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(TB) k_cam_distort(const void* pts, int64_t n, int W, CamArgs a, void* out, int* invalid_count) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const bool active = i < n;
  bool ok = true;
  if (active) {
    double u, v;
    load_point<TI>(pts, i, W, u, v);
    double x = (u - a.ncx) / a.nfx, y = (v - a.ncy) / a.nfy, z = 1.0;
    if (a.has_R) {                                                // R^T
      const double X = a.R[0] * x + a.R[3] * y + a.R[6], Y = a.R[1] * x + a.R[4] * y + a.R[7], Z = a.R[2] * x + a.R[5] * y + a.R[8];
      x = X;
      y = Y;
      z = Z;
    }
    ok = z > 0.0 && x == x && y == y;
    double xd = 0.0, yd = 0.0;
    if (ok) {
      x /= z;
      y /= z;
      if (a.model == DEVO_CAM_RADTAN) {
        double j0, j1, j2, j3;
        radtan_fwd(a.k, x, y, xd, yd, j0, j1, j2, j3);
      } else if (a.model == DEVO_CAM_EQUIDISTANT) {
        const double r = sqrt(x * x + y * y);
        const double t = atan(r);
        ok = t <= a.theta_lim;
        const double s = r > 0.0 ? t * eq_poly(a.k, t * t) / r : 1.0;
        xd = x * s;
        yd = y * s;
      } else {
        xd = x;
        yd = y;
      }
    }
    if (ok) {
      xd = a.fx * xd + a.cx;
      yd = a.fy * yd + a.cy;
    } else {
      xd = yd = __builtin_nan("");
    }
    store_point<TO>(out, i, xd, yd);
  }
  count_invalid(active && !ok, invalid_count);
}

// ------------------------------------------------------------------------------------------------ remap
template <typename T> __device__ __forceinline__ T to_out(float v);
template <> __device__ __forceinline__ float to_out<float>(float v) { return v; }
template <> __device__ __forceinline__ uint8_t to_out<uint8_t>(float v) { return (uint8_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }   // nearest even, saturating; NaN -> 0

template <typename T, int C> struct alignas(sizeof(T) * (C == 3 ? 1 : C)) Pixel { T c[C]; };

template <typename TI, typename TO, int C>
__global__ void __launch_bounds__(TB) k_remap(const TI* __restrict__ img, int B, int H, int W, const float2* __restrict__ map, int64_t n_out, TO* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_out) return;
  const float2 m = map[i];
  const bool inside = m.x > -1.0f && m.x < (float)W && m.y > -1.0f && m.y < (float)H;    // false for NaN: every tap outside
  const float fx0 = floorf(m.x), fy0 = floorf(m.y);
  const float wx = m.x - fx0, wy = m.y - fy0;                     // exact in fp32
  const int x0 = inside ? (int)fx0 : 0, y0 = inside ? (int)fy0 : 0;
  const bool cx0 = inside && x0 >= 0, cx1 = inside && x0 + 1 < W, cy0 = inside && y0 >= 0, cy1 = inside && y0 + 1 < H;
  const float w00 = (1.0f - wx) * (1.0f - wy), w01 = wx * (1.0f - wy), w10 = (1.0f - wx) * wy, w11 = wx * wy;
  const size_t plane = (size_t)H * W;
  const size_t o00 = (size_t)(cy0 ? y0 : 0) * W + (cx0 ? x0 : 0), o01 = (size_t)(cy0 ? y0 : 0) * W + (cx1 ? x0 + 1 : 0);
  const size_t o10 = (size_t)(cy1 ? y0 + 1 : 0) * W + (cx0 ? x0 : 0), o11 = (size_t)(cy1 ? y0 + 1 : 0) * W + (cx1 ? x0 + 1 : 0);
  const bool t00 = cx0 && cy0, t01 = cx1 && cy0, t10 = cx0 && cy1, t11 = cx1 && cy1;
  using PI = Pixel<TI, C>;
  using PO = Pixel<TO, C>;
  const PI* src = (const PI*)img;
  PO* dst = (PO*)out;
  for (int b = 0; b < B; ++b) {
    const PI* p = src + b * plane;
    float v[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[ch] = 0.0f;
    if (t00) { const PI q = p[o00];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] += w00 * (float)q.c[ch]; }
    if (t01) { const PI q = p[o01];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] += w01 * (float)q.c[ch]; }
    if (t10) { const PI q = p[o10];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] += w10 * (float)q.c[ch]; }
    if (t11) { const PI q = p[o11];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] += w11 * (float)q.c[ch]; }
    PO r;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) r.c[ch] = to_out<TO>(v[ch]);
    dst[(size_t)b * n_out + i] = r;
  }
}

template <typename TI, typename TO>
void launch_remap(const void* img, int B, int H, int W, int C, const float* map, int64_t n_out, void* out, hipStream_t s) {
  const dim3 grid((unsigned)((n_out + TB - 1) / TB)), block(TB);
  switch (C) {
    case 1: hipLaunchKernelGGL((k_remap<TI, TO, 1>), grid, block, 0, s, (const TI*)img, B, H, W, (const float2*)map, n_out, (TO*)out); break;
    case 2: hipLaunchKernelGGL((k_remap<TI, TO, 2>), grid, block, 0, s, (const TI*)img, B, H, W, (const float2*)map, n_out, (TO*)out); break;
    case 3: hipLaunchKernelGGL((k_remap<TI, TO, 3>), grid, block, 0, s, (const TI*)img, B, H, W, (const float2*)map, n_out, (TO*)out); break;
    default: hipLaunchKernelGGL((k_remap<TI, TO, 4>), grid, block, 0, s, (const TI*)img, B, H, W, (const float2*)map, n_out, (TO*)out); break;
  }
}

// ------------------------------------------------------------------------------------------------ host side
bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

double h_poly(const double* k, double t) {
  const double t2 = t * t;
  return t * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
}
double h_dpoly(const double* k, double t) {
  const double t2 = t * t;
  return 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * 9.0 * k[3])));
}

// the smallest positive root of d theta_d / d theta in (0, pi / 2], or pi / 2: a scan of 4096 steps for the first sign change, then bisection
double equi_theta_lim(const double* k) {
  const double half_pi = 1.5707963267948966;
  const int steps = 4096;
  double a = 0.0;
  for (int i = 1; i <= steps; ++i) {
    const double b = half_pi * i / steps;
    if (!(h_dpoly(k, b) > 0.0)) {
      double lo = a, hi = b;
      for (int it = 0; it < 100; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (h_dpoly(k, mid) > 0.0) lo = mid; else hi = mid;
      }
      return lo;
    }
    a = b;
  }
  return half_pi;
}

int fill_args(const char* what, int64_t n, const void* points, int H, int W, int in_dtype, int model, const double* K, const double* dist, int n_dist, const double* R,
              const double* K_new, bool need_K_new, const void* out, int out_dtype, CamArgs& a) {
  DEVO_REQUIRE(n >= 0 && n <= (int64_t)1 << 36, "%s: %lld points", what, (long long)n);
  DEVO_REQUIRE(out || n == 0, "%s: null output", what);
  DEVO_REQUIRE((in_dtype == DEVO_F32 || in_dtype == DEVO_F64) && (out_dtype == DEVO_F32 || out_dtype == DEVO_F64), "%s: points are fp32 or fp64 (dtype codes %d, %d)", what,
               in_dtype, out_dtype);
  DEVO_REQUIRE(points || (H >= 1 && W >= 1 && (int64_t)H * W == n), "%s: without points the grid is H x W = n (H %d, W %d, n %lld)", what, H, W, (long long)n);
  DEVO_REQUIRE(model == DEVO_CAM_PINHOLE || model == DEVO_CAM_RADTAN || model == DEVO_CAM_EQUIDISTANT, "%s: unknown lens model %d", what, model);
  DEVO_REQUIRE(K, "%s: null K", what);
  DEVO_REQUIRE(finite_all(K, 4) && K[0] != 0.0 && K[1] != 0.0, "%s: K must be finite with non-zero focal lengths", what);
  DEVO_REQUIRE(n_dist == (model == DEVO_CAM_PINHOLE ? 0 : 4) || (model == DEVO_CAM_RADTAN && n_dist == 5), "%s: %d coefficients for lens model %d (pinhole 0, radtan 4 or 5, equidistant 4)",
               what, n_dist, model);
  DEVO_REQUIRE(n_dist == 0 || dist, "%s: null coefficients", what);
  DEVO_REQUIRE(n_dist == 0 || finite_all(dist, n_dist), "%s: non-finite coefficient", what);
  DEVO_REQUIRE(!R || finite_all(R, 9), "%s: non-finite R", what);
  DEVO_REQUIRE(K_new || !need_K_new, "%s: null K_new", what);
  DEVO_REQUIRE(!K_new || (finite_all(K_new, 4) && K_new[0] != 0.0 && K_new[1] != 0.0), "%s: K_new must be finite with non-zero focal lengths", what);
  a.fx = K[0], a.fy = K[1], a.cx = K[2], a.cy = K[3];
  for (int i = 0; i < 5; ++i) a.k[i] = i < n_dist ? dist[i] : 0.0;
  for (int i = 0; i < 9; ++i) a.R[i] = R ? R[i] : (i % 4 == 0 ? 1.0 : 0.0);
  a.has_R = R != nullptr;
  a.nfx = K_new ? K_new[0] : 1.0, a.nfy = K_new ? K_new[1] : 1.0, a.ncx = K_new ? K_new[2] : 0.0, a.ncy = K_new ? K_new[3] : 0.0;
  a.model = model;
  a.theta_lim = a.theta_dmax = 0.0;
  if (model == DEVO_CAM_EQUIDISTANT) {
    a.theta_lim = equi_theta_lim(a.k);
    a.theta_dmax = h_poly(a.k, a.theta_lim);
  }
  return DEVO_OK;
}

}  // namespace

extern "C" int devo_camera_undistort_points(const void* points, int64_t n, int H, int W, int in_dtype, int model, const double* K, const double* dist, int n_dist,
                                            const double* R, const double* K_new, void* out, int out_dtype, int* invalid_count, devo_stream_t stream) {
  CamArgs a;
  const int rc = fill_args("camera_undistort_points", n, points, H, W, in_dtype, model, K, dist, n_dist, R, K_new, false, out, out_dtype, a);
  if (rc != DEVO_OK) return rc;
  if (n == 0) return DEVO_OK;
  const dim3 grid((unsigned)((n + TB - 1) / TB)), block(TB);
  const hipStream_t s = (hipStream_t)stream;
  if (in_dtype == DEVO_F32) {
    if (out_dtype == DEVO_F32) hipLaunchKernelGGL((k_cam_undistort<float, float>), grid, block, 0, s, points, n, W, a, out, invalid_count);
    else hipLaunchKernelGGL((k_cam_undistort<float, double>), grid, block, 0, s, points, n, W, a, out, invalid_count);
  } else {
    if (out_dtype == DEVO_F32) hipLaunchKernelGGL((k_cam_undistort<double, float>), grid, block, 0, s, points, n, W, a, out, invalid_count);
    else hipLaunchKernelGGL((k_cam_undistort<double, double>), grid, block, 0, s, points, n, W, a, out, invalid_count);
  }
  return check_launch("camera_undistort_points");
}

extern "C" int devo_camera_distort_points(const void* points, int64_t n, int H, int W, int in_dtype, int model, const double* K, const double* dist, int n_dist,
                                          const double* R, const double* K_new, void* out, int out_dtype, int* invalid_count, devo_stream_t stream) {
  CamArgs a;
  const int rc = fill_args("camera_distort_points", n, points, H, W, in_dtype, model, K, dist, n_dist, R, K_new, true, out, out_dtype, a);
  if (rc != DEVO_OK) return rc;
  if (n == 0) return DEVO_OK;
  const dim3 grid((unsigned)((n + TB - 1) / TB)), block(TB);
  const hipStream_t s = (hipStream_t)stream;
  if (in_dtype == DEVO_F32) {
    if (out_dtype == DEVO_F32) hipLaunchKernelGGL((k_cam_distort<float, float>), grid, block, 0, s, points, n, W, a, out, invalid_count);
    else hipLaunchKernelGGL((k_cam_distort<float, double>), grid, block, 0, s, points, n, W, a, out, invalid_count);
  } else {
    if (out_dtype == DEVO_F32) hipLaunchKernelGGL((k_cam_distort<double, float>), grid, block, 0, s, points, n, W, a, out, invalid_count);
    else hipLaunchKernelGGL((k_cam_distort<double, double>), grid, block, 0, s, points, n, W, a, out, invalid_count);
  }
  return check_launch("camera_distort_points");
}

extern "C" int devo_image_remap(const void* images, int B, int H, int W, int C, int in_dtype, const float* map, int Ho, int Wo, void* out, int out_dtype,
                                devo_stream_t stream) {
  DEVO_REQUIRE(images && map && out, "image_remap: null tensor");
  DEVO_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "image_remap: B %d, image %d x %d, output %d x %d", B, H, W, Ho, Wo);
  DEVO_REQUIRE(C >= 1 && C <= 4, "image_remap: 1 to 4 channels (got %d)", C);
  DEVO_REQUIRE((in_dtype == DEVO_U8 || in_dtype == DEVO_F32) && (out_dtype == DEVO_U8 || out_dtype == DEVO_F32), "image_remap: images are uint8 or fp32 (dtype codes %d, %d)",
               in_dtype, out_dtype);
  DEVO_REQUIRE(W < (1 << 24) && H < (1 << 24), "image_remap: image sides below 2^24 (fp32 coordinates)");
  const size_t esz = in_dtype == DEVO_F32 ? 4 : 1, osz = out_dtype == DEVO_F32 ? 4 : 1;
  const size_t va = C == 3 ? 1 : (size_t)C;                       // the kernel loads and stores whole pixels where a pixel is 1, 2 or 4 elements
  DEVO_REQUIRE((uintptr_t)images % (esz * va) == 0 && (uintptr_t)out % (osz * va) == 0 && (uintptr_t)map % 8 == 0, "image_remap: misaligned tensor");
  const int64_t n_out = (int64_t)Ho * Wo;
  const hipStream_t s = (hipStream_t)stream;
  if (in_dtype == DEVO_U8) {
    if (out_dtype == DEVO_U8) launch_remap<uint8_t, uint8_t>(images, B, H, W, C, map, n_out, out, s);
    else launch_remap<uint8_t, float>(images, B, H, W, C, map, n_out, out, s);
  } else {
    if (out_dtype == DEVO_U8) launch_remap<float, uint8_t>(images, B, H, W, C, map, n_out, out, s);
    else launch_remap<float, float>(images, B, H, W, C, map, n_out, out, s);
  }
  return check_launch("image_remap");
}
