// The training frame graph of one scene on the GPU (devo/data_readers/base.py:263-286 over rgbd_utils.py:104-141 and the data readers'
// projective_ops.py), wave64, gfx950: the mean flow magnitude between all pairs of frames and the neighbour lists drawn from it.
//   * k_fg_disps: ONE workgroup per frame.  The frame's mean (fp64 partial sums, in-wave shuffles, the waves' sums added in wave order)
//     replaces every depth below 0.01; 1 / depth is written.
//   * k_fg_frames: per frame the rotation matrix and translation of its camera-to-world pose and its intrinsics, in fp64: the table the
//     pair kernel forms G_ij from.
//   * k_fg_pairs: the directed sums S_ij = sum mag * valid and V_ij = sum valid.  A workgroup owns ONE source frame i and a block of
//     FG_TJ = 64 target frames.  It stages the source's back-projected pixels (X, Y, disparity, x, y) in LDS once per chunk of FG_CHUNK
//     pixels (the 30 x 40 map is one chunk: the divisions by fx, fy are paid once per 64 targets); each of its 4 waves then owns WHOLE
//     pairs, FG_JW = 4 at a time: G_ij = P_j P_i^-1 is formed per wave in fp64 from the frame table, rounded to fp32 and made
//     wave-uniform (readfirstlane: scalar registers), every lane walks the pixels lane, lane + 64, ... and keeps one (S, V) per pair, and
//     a butterfly of shuffles adds the 64 lanes.  A pair never leaves its wave, so the cross-wave step of the reduction is empty and the
//     order of every sum is fixed: no atomics, bit-reproducible.  Each directed pair is computed once.
//   * k_fg_combine: matrix[i, j] = scale * (S_ij + S_ji) / (V_ij + V_ji), the lower frame's direction first in both sums (bitwise
//     symmetric), +inf where 10 (V_ij + V_ji) < 7 * 2 h w (integers: the reference's fp32 mean < 0.7, its tie kept finite).
//   * k_fg_degree / k_fg_scan / k_fg_fill: the lists in CSR form: one wave per row counts matrix < max_flow (ballot + popcount), one
//     workgroup scans the degrees into rowptr, one wave per row writes its columns in ascending order (ballot + prefix count).
// Pair indices are 64-bit.  No float atomics anywhere.
#include "common.h"

namespace {

using namespace devo;

constexpr int TB = 256;                      // 4 waves of 64
constexpr int WAVES = TB / 64;
constexpr int FG_JW = 4;                     // pairs a wave carries at once
constexpr int FG_TJ = 64;                    // target frames per workgroup
constexpr int FG_GROUPS = FG_TJ / (WAVES * FG_JW);
constexpr int FG_CHUNK = 1536;               // source pixels staged in LDS at a time: 5 floats each, 30 KB
constexpr int FG_TABLE = 16;                 // doubles per frame: R (9, row-major, camera to world), t (3), fx fy cx cy
constexpr int SCAN_TB = 1024;
static_assert(FG_GROUPS * WAVES * FG_JW == FG_TJ, "target block");

__device__ __forceinline__ float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__global__ __launch_bounds__(TB) void k_fg_disps(const float* __restrict__ depths, float* __restrict__ disps, int hw) {
  const float* src = depths + (long long)blockIdx.x * hw;
  float* dst = disps + (long long)blockIdx.x * hw;
  double s = 0.0;
  for (int p = threadIdx.x; p < hw; p += TB) s += (double)src[p];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ double sh[WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  double total = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) total += sh[w];
  const float mean = (float)(total / (double)hw);
  for (int p = threadIdx.x; p < hw; p += TB) {
    const float d = src[p];
    dst[p] = 1.0f / (d < 0.01f ? mean : d);
  }
}

__global__ __launch_bounds__(TB) void k_fg_frames(const float* __restrict__ poses, const float* __restrict__ intrinsics, double* __restrict__ table, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= N) return;
  const float* p = poses + (long long)i * 7;
  const double x = p[3], y = p[4], z = p[5], w = p[6];
  double* o = table + (long long)i * FG_TABLE;
  // lietorch's rotation of a vector by (x, y, z, w): v + 2 w (u x v) + 2 u x (u x v), as a matrix
  o[0] = 1.0 - 2.0 * (y * y + z * z); o[1] = 2.0 * (x * y - w * z);       o[2] = 2.0 * (x * z + w * y);
  o[3] = 2.0 * (x * y + w * z);       o[4] = 1.0 - 2.0 * (x * x + z * z); o[5] = 2.0 * (y * z - w * x);
  o[6] = 2.0 * (x * z - w * y);       o[7] = 2.0 * (y * z + w * x);       o[8] = 1.0 - 2.0 * (x * x + y * y);
  o[9] = p[0]; o[10] = p[1]; o[11] = p[2];
#pragma unroll
  for (int k = 0; k < 4; k++) o[12 + k] = intrinsics[(long long)i * 4 + k];
}

// G_ij = P_j P_i^-1 on the world-to-camera poses P = (R^T, -R^T t): rotation R_j^T R_i, translation R_j^T (t_i - t_j); projection with j's intrinsics
struct Pair { float r[9], t[3], fx, fy, cx, cy; };

__device__ __forceinline__ Pair pair_of(const double* __restrict__ table, int i, int j) {
  Pair g;
  const double* b = table + (long long)j * FG_TABLE;
  g.fx = uniform((float)b[12]); g.fy = uniform((float)b[13]); g.cx = uniform((float)b[14]); g.cy = uniform((float)b[15]);
  if (i == j) {                              // the reference's fixed pose of a frame against itself
#pragma unroll
    for (int k = 0; k < 9; k++) g.r[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    g.t[0] = -0.1f; g.t[1] = 0.0f; g.t[2] = 0.0f;
    return g;
  }
  const double* a = table + (long long)i * FG_TABLE;
  const double d0 = a[9] - b[9], d1 = a[10] - b[10], d2 = a[11] - b[11];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) g.r[3 * r + c] = uniform((float)(b[r] * a[c] + b[3 + r] * a[3 + c] + b[6 + r] * a[6 + c]));
    g.t[r] = uniform((float)(b[r] * d0 + b[3 + r] * d1 + b[6 + r] * d2));
  }
  return g;
}

__global__ __launch_bounds__(TB) void k_fg_pairs(const double* __restrict__ table, const float* __restrict__ disps, float* __restrict__ S, int* __restrict__ V,
                                                 int N, int h, int w) {
  __shared__ float sX[FG_CHUNK], sY[FG_CHUNK], sD[FG_CHUNK], sx[FG_CHUNK], sy[FG_CHUNK];
  const int i = blockIdx.x, j0 = blockIdx.y * FG_TJ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hw = h * w;
  const double* a = table + (long long)i * FG_TABLE;
  const float fx = (float)a[12], fy = (float)a[13], cx = (float)a[14], cy = (float)a[15];
  const float* disp = disps + (long long)i * hw;

  // (the group loop stays rolled: one group's 64 uniform pose values fill the scalar registers)
#pragma unroll 1
  for (int g = 0; g < FG_GROUPS; g++) {
    const int jb = j0 + (g * WAVES + wave) * FG_JW;             // wave-uniform
    Pair G[FG_JW];
#pragma unroll
    for (int t = 0; t < FG_JW; t++) G[t] = pair_of(table, i, min(jb + t, N - 1));
    float acc[FG_JW];
    int cnt[FG_JW];
#pragma unroll
    for (int t = 0; t < FG_JW; t++) { acc[t] = 0.0f; cnt[t] = 0; }
    for (int base = 0; base < hw; base += FG_CHUNK) {
      const int n = min(FG_CHUNK, hw - base);
      if (g == 0 || hw > FG_CHUNK) {                            // a map of one chunk is staged once for all 64 targets
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += TB) {
          const int p = base + q, yy = p / w, xx = p - yy * w;
          sx[q] = (float)xx; sy[q] = (float)yy;
          sX[q] = ((float)xx - cx) / fx; sY[q] = ((float)yy - cy) / fy;
          sD[q] = disp[p];
        }
        __syncthreads();
      }
      if (jb >= N) continue;
      for (int q = lane; q < n; q += 64) {
        const float X = sX[q], Y = sY[q], d = sD[q], px = sx[q], py = sy[q];
#pragma unroll
        for (int t = 0; t < FG_JW; t++) {
          const Pair& P = G[t];
          const float x1 = fmaf(P.r[0], X, fmaf(P.r[1], Y, fmaf(P.t[0], d, P.r[2])));
          const float y1 = fmaf(P.r[3], X, fmaf(P.r[4], Y, fmaf(P.t[1], d, P.r[5])));
          const float z1 = fmaf(P.r[6], X, fmaf(P.r[7], Y, fmaf(P.t[2], d, P.r[8])));
          const float iz = 1.0f / (z1 < 0.1f ? 1.0f : z1);
          const float fu = fmaf(P.fx, x1 * iz, P.cx) - px, fv = fmaf(P.fy, y1 * iz, P.cy) - py;
          const float mag = fminf(sqrtf(fmaf(fu, fu, fv * fv)), 100.0f);
          const bool valid = z1 > 0.2f;
          acc[t] += valid ? mag : 0.0f;
          cnt[t] += valid ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < FG_JW; t++) {
      float s = acc[t];
      int c = cnt[t];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
      if (lane == 0 && jb + t < N) {
        const long long at = (long long)i * N + (jb + t);
        S[at] = s; V[at] = c;
      }
    }
  }
}

__global__ __launch_bounds__(TB) void k_fg_combine(const float* __restrict__ S, const int* __restrict__ V, float* __restrict__ matrix, int N, long long need14,
                                                   float scale) {
  const long long total = (long long)N * N, stride = (long long)gridDim.x * TB;
  for (long long e = (long long)blockIdx.x * TB + threadIdx.x; e < total; e += stride) {
    const long long i = e / N, j = e - i * N;
    const long long lo = i < j ? e : j * N + i, hi = i < j ? j * N + i : e;      // the lower frame's direction first: [i, j] and [j, i] add alike
    const float s = S[lo] + S[hi];
    const long long v = (long long)V[lo] + V[hi];
    matrix[e] = 10 * v < need14 ? __int_as_float(0x7f800000) : (s / (float)v) * scale;
  }
}

// one wave per row: how many entries lie below max_flow
__global__ __launch_bounds__(TB) void k_fg_degree(const float* __restrict__ matrix, int N, float max_flow, int* __restrict__ degree) {
  const int row = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* m = matrix + (long long)row * N;
  int n = 0;
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    n += __popcll(__ballot(j < N && m[j] < max_flow));
  }
  if (lane == 0) degree[row] = n;
}

// rowptr[0] = 0, rowptr[r + 1] = degree[0] + ... + degree[r]: one workgroup, each thread a run of consecutive rows
__global__ __launch_bounds__(SCAN_TB) void k_fg_scan(const int* __restrict__ degree, int N, int64_t* __restrict__ rowptr) {
  __shared__ long long sh[SCAN_TB];
  const int per = (N + SCAN_TB - 1) / SCAN_TB, first = threadIdx.x * per, last = min(first + per, N);
  long long s = 0;
  for (int r = first; r < last; r++) s += degree[r];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < SCAN_TB; o <<= 1) {
    const long long add = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  long long run = sh[threadIdx.x] - s;
  if (threadIdx.x == 0) rowptr[0] = 0;
  for (int r = first; r < last; r++) { run += degree[r]; rowptr[r + 1] = run; }
}

// one wave per row: the columns below max_flow in ascending order, and their distances
__global__ __launch_bounds__(TB) void k_fg_fill(const float* __restrict__ matrix, int N, float max_flow, const int64_t* __restrict__ rowptr, int64_t* __restrict__ cols,
                                                float* __restrict__ dists, long long capacity) {
  const int row = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* m = matrix + (long long)row * N;
  long long at = rowptr[row];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    const float x = j < N ? m[j] : 0.0f;
    const bool keep = j < N && x < max_flow;
    const unsigned long long b = __ballot(keep);
    const long long dst = at + __popcll(b & below);
    if (keep && dst < capacity) { cols[dst] = j; dists[dst] = x; }
    at += __popcll(b);
  }
}

size_t table_bytes(int N) { return align_up((size_t)N * FG_TABLE * sizeof(double)); }
size_t sums_bytes(int N) { return align_up((size_t)N * N * sizeof(float)); }
size_t degree_bytes(int N) { return align_up((size_t)N * sizeof(int)); }

bool sizes_ok(int N, int h, int w) { return N > 0 && N <= DEVO_FRAME_GRAPH_MAX_FRAMES && h > 0 && w > 0; }

}  // namespace

extern "C" {

size_t devo_frame_graph_workspace_bytes(int N, int h, int w) {
  if (!sizes_ok(N, h, w) || 2ll * h * w >= DEVO_FRAME_GRAPH_MAX_POINTS) return 0;
  return table_bytes(N) + 2 * sums_bytes(N) + degree_bytes(N);
}

int devo_frame_graph_disps(const float* depths, float* disps, int N, int h, int w, devo_stream_t stream) {
  DEVO_REQUIRE(depths && disps && sizes_ok(N, h, w), "devo_frame_graph_disps: bad arguments (N = %d, h = %d, w = %d)", N, h, w);
  if (2ll * h * w >= DEVO_FRAME_GRAPH_MAX_POINTS) {
    set_error("devo_frame_graph_disps: maps of %d x %d: 2 h w must stay below %d", h, w, DEVO_FRAME_GRAPH_MAX_POINTS);
    return DEVO_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(k_fg_disps, dim3(N), dim3(TB), 0, (hipStream_t)stream, depths, disps, h * w);
  return check_launch("devo_frame_graph_disps");
}

int devo_frame_graph_distances(const float* poses, const float* disps, const float* intrinsics, int N, int h, int w, float scale, float* matrix, void* ws,
                               size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(poses && disps && intrinsics && matrix && sizes_ok(N, h, w), "devo_frame_graph_distances: bad arguments (N = %d, h = %d, w = %d)", N, h, w);
  if (2ll * h * w >= DEVO_FRAME_GRAPH_MAX_POINTS) {
    set_error("devo_frame_graph_distances: maps of %d x %d: 2 h w must stay below %d (the 0.7 rule is decided on integers that agree with the fp32 mean)", h, w,
              DEVO_FRAME_GRAPH_MAX_POINTS);
    return DEVO_ERR_UNSUPPORTED;
  }
  if (!ws || ws_bytes < devo_frame_graph_workspace_bytes(N, h, w)) {
    set_error("devo_frame_graph_distances: workspace too small");
    return DEVO_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* table = (double*)ws;
  float* S = (float*)((char*)ws + table_bytes(N));
  int* V = (int*)((char*)S + sums_bytes(N));
  hipLaunchKernelGGL(k_fg_frames, dim3(blocks_for(N, TB)), dim3(TB), 0, st, poses, intrinsics, table, N);
  hipLaunchKernelGGL(k_fg_pairs, dim3(N, (N + FG_TJ - 1) / FG_TJ), dim3(TB), 0, st, (const double*)table, disps, S, V, N, h, w);
  hipLaunchKernelGGL(k_fg_combine, dim3(blocks_for((long long)N * N, TB, 8192)), dim3(TB), 0, st, (const float*)S, (const int*)V, matrix, N, 14ll * h * w, scale);
  return check_launch("devo_frame_graph_distances");
}

int devo_frame_graph_lists(const float* matrix, int N, float max_flow, int64_t* rowptr, int64_t* cols, float* dists, int64_t capacity, void* ws, size_t ws_bytes,
                           devo_stream_t stream) {
  DEVO_REQUIRE(matrix && rowptr && N > 0 && N <= DEVO_FRAME_GRAPH_MAX_FRAMES, "devo_frame_graph_lists: bad arguments (N = %d)", N);
  DEVO_REQUIRE((cols == nullptr) == (dists == nullptr) && capacity >= 0, "devo_frame_graph_lists: cols and dists come together");
  if (!ws || ws_bytes < table_bytes(N) + 2 * sums_bytes(N) + degree_bytes(N)) {
    set_error("devo_frame_graph_lists: workspace too small");
    return DEVO_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 rows((N + WAVES - 1) / WAVES);
  if (!cols) {
    int* degree = (int*)((char*)ws + table_bytes(N) + 2 * sums_bytes(N));
    hipLaunchKernelGGL(k_fg_degree, rows, dim3(TB), 0, st, matrix, N, max_flow, degree);
    hipLaunchKernelGGL(k_fg_scan, dim3(1), dim3(SCAN_TB), 0, st, (const int*)degree, N, rowptr);
  } else {
    hipLaunchKernelGGL(k_fg_fill, rows, dim3(TB), 0, st, matrix, N, max_flow, (const int64_t*)rowptr, cols, dists, (long long)capacity);
  }
  return check_launch("devo_frame_graph_lists");
}

}  // extern "C"
