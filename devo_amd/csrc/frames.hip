// The per-frame state of DEVO's inference that lies between the kernels of the update step, the Patchifier and the patch graph
// (devo/devo.py:487-488, :502-520 the frame store; :342-344 the point cloud; :179-196, :276-280, :534 the relative-pose log and
// terminate()), wave64, gfx950.  Group operations are se3_dev.h's: quaternions renormalised on load, as lietorch's kernels do.
//   * k_begin_frame: ONE workgroup of 1024 threads writes row n of poses / patches / intrinsics / tstamps from rows < n and the
//     arguments.  The depth is the LOWER median of the 3 M P P depth values of the last three frames: an exact radix select over the
//     order-preserving bit image of fp32, four passes of 8 bits.  Every thread holds its (at most 32) keys in registers, so the
//     values are read once; a pass is a 256-bin histogram in LDS (integer atomics) and a scan of it by the first wave.  One thread of
//     the last wave evaluates the motion model meanwhile.
//   * k_point_cloud: one thread per patch, the centre pixel only: X = G[ix[k]]^-1 (x, y, 1, d), out[k] = X[:3] / X[3].
//   * k_traj_record: one thread, parent[t1] = t0 and rel[t1] = P[k] P[k-1]^-1 with t0, t1 read on the device (or the identity and
//     the host's t, t0 for a skipped frame).
//   * k_traj_init / k_traj_round: terminate() as parallel pointer jumping.  init: a frame that is a keyframe (a binary search in
//     tstamps[:n], which the state machine keeps strictly increasing — checked here) starts as a root holding its pose, any other as
//     (rel[t], parent[t]).  round: acc[t] <- acc[t] acc[p], par[t] <- par[p], double-buffered; after r rounds a frame has absorbed
//     2^r links, so ceil(log2(counter)) rounds resolve every chain whatever its depth.  The kernel that runs last inverts the poses
//     and reports a frame that is still unresolved through the status word.
// Nothing here synchronises with the host; `status` is a host-visible word (pinned), written with plain vector stores.
#include <algorithm>
#include "common.h"
#include "se3_dev.h"

namespace {

using namespace devo;

constexpr int TB = 256;
constexpr int BF_TB = 1024;                                   // k_begin_frame: 16 waves
constexpr int BF_KEYS = DEVO_FRAME_MEDIAN_MAX / BF_TB;        // keys per thread
static_assert(BF_KEYS * BF_TB == DEVO_FRAME_MEDIAN_MAX, "median bound");

// fp32 -> u32 whose unsigned order is the order of the floats (-0 below +0), and back
__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct BeginArgs {
  float* poses; float* patches; float* intrinsics; int64_t* tstamps;
  const float* new_patches; const float* new_intrinsics; const float* depth;      // depth: [M] or NULL (median)
  int64_t counter;
  int M, PP, n, model;
  float res, damping;
};

// poses[n] = Exp(damping Log(P[n-1] P[n-2]^-1)) P[n-1]   (devo.py:503-509)
__device__ __forceinline__ void motion_model(float* poses, int n, int model, float damping) {
  const float* p1 = poses + (int64_t)(n - 1) * 7;
  float* out = poses + (int64_t)n * 7;
  if (model != DEVO_FRAME_DAMPED_LINEAR) {
#pragma unroll
    for (int c = 0; c < 7; c++) out[c] = p1[c];
    return;
  }
  const SE3<float> P1 = SE3<float>::load(p1), P2 = SE3<float>::load(poses + (int64_t)(n - 2) * 7);
  float xi[6];
  se3_log(P1.mul(P2.inv()), xi);
#pragma unroll
  for (int c = 0; c < 6; c++) xi[c] *= damping;
  se3_exp(xi).mul(P1).store(out);
}

__global__ __launch_bounds__(BF_TB) void k_begin_frame(BeginArgs a) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_rank;
  __shared__ int sh_nan;
  const int tid = threadIdx.x;
  const int MPP = a.M * a.PP;
  if (tid == BF_TB - 1) {
    if (a.n > 1) motion_model(a.poses, a.n, a.model, a.damping);
    a.tstamps[a.n] = a.counter;
  }
  if (tid >= BF_TB - 64 && tid < BF_TB - 60) {
    const int c = tid - (BF_TB - 64);
    a.intrinsics[(int64_t)a.n * 4 + c] = __fdiv_rn(a.new_intrinsics[c], a.res);
  }
  float med = 0.0f;
  if (!a.depth) {
    const int count = 3 * MPP;                                 // <= DEVO_FRAME_MEDIAN_MAX (the host refuses more)
    const float* src = a.patches + (int64_t)(a.n - 3) * MPP * 3;
    unsigned keys[BF_KEYS];
    bool nan = false;
#pragma unroll
    for (int s = 0; s < BF_KEYS; s++) {
      const int i = s * BF_TB + tid;
      keys[s] = 0u;
      if (i < count) {
        const int patch = i / a.PP, p = i - patch * a.PP;      // patch counts over the three frames
        const float v = src[((int64_t)patch * 3 + 2) * a.PP + p];
        nan |= v != v;
        keys[s] = fkey(v);
      }
    }
    if (tid == 0) { sh_prefix = 0u; sh_rank = (unsigned)((count - 1) / 2); sh_nan = 0; }
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    if (nan) sh_nan = 1;
    for (int pass = 0; pass < 4; pass++) {
      const int shift = 24 - 8 * pass;
      const unsigned prefix = sh_prefix;
      const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
#pragma unroll
      for (int s = 0; s < BF_KEYS; s++) {
        const int i = s * BF_TB + tid;
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
    med = sh_nan ? __uint_as_float(0x7fc00000u) : fkey_value(sh_prefix);      // (torch.median: NaN if there is one)
  }
  // row n of patches: channels 0, 1 from the new frame, channel 2 the depth
  float* row = a.patches + (int64_t)a.n * MPP * 3;
  for (int i = tid; i < 3 * MPP; i += BF_TB) {
    const int pc = i / a.PP, patch = pc / 3, c = pc - patch * 3;
    row[i] = c < 2 ? a.new_patches[i] : (a.depth ? a.depth[patch] : med);
  }
}

__global__ __launch_bounds__(TB) void k_point_cloud(const float* __restrict__ poses, const float* __restrict__ patches, const float* __restrict__ intr,
                                                    const int64_t* __restrict__ ix, int n_poses, int P, int first, int m, float* __restrict__ out) {
  const int k = first + blockIdx.x * TB + threadIdx.x;
  if (k >= m) return;
  const int64_t f = ix[k];
  float* o = out + (int64_t)k * 3;
  if (f < 0 || f >= n_poses) {                                 // (a frame outside the buffers is never read)
    o[0] = o[1] = o[2] = __uint_as_float(0x7fc00000u);
    return;
  }
  const int PP = P * P, c = (P / 2) * P + P / 2;
  const float* pk = patches + (int64_t)k * 3 * PP + c;
  const float fx = intr[f * 4], fy = intr[f * 4 + 1], cx = intr[f * 4 + 2], cy = intr[f * 4 + 3];
  const float d = pk[2 * PP];
  const V3<float> X0{(pk[0] - cx) / fx, (pk[PP] - cy) / fy, 1.0f};
  const SE3<float> Gi = SE3<float>::load(poses + f * 7).inv();
  const V3<float> X = qrot(Gi.q, X0) + d * Gi.t;               // act4 (se3.h:53-56): the fourth component stays d
  o[0] = X.x / d; o[1] = X.y / d; o[2] = X.z / d;
}

// ---- trajectory ----------------------------------------------------------------------------------
__global__ void k_traj_record(const float* __restrict__ poses, const int64_t* __restrict__ tstamps, int k, int64_t t, int64_t t0,
                              int64_t* __restrict__ parent, float* __restrict__ rel, int capacity, int* __restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  SE3<float> dP;
  if (poses) {                                                 // devo.py:276-280
    t0 = tstamps[k - 1];
    t = tstamps[k];
    dP = SE3<float>::load(poses + (int64_t)k * 7).mul(SE3<float>::load(poses + (int64_t)(k - 1) * 7).inv());
  } else {                                                     // devo.py:534
    dP.t = V3<float>{0.0f, 0.0f, 0.0f};
    dP.q = Q4<float>{0.0f, 0.0f, 0.0f, 1.0f};
  }
  if (t < 0 || t >= capacity || t0 < 0 || t0 >= t) { *status = DEVO_FRAME_STATUS_BAD_ENTRY; return; }
  parent[t] = t0;
  dP.store(rel + t * 7);
}

struct TrajBuf { float* acc; int* par; };

// the kernel that runs last: the inverse of every pose (devo.py:196); a frame that no chain of entries ties to a keyframe is reported
__device__ __forceinline__ void traj_finish(const SE3<float>& X, int par, int t, float* __restrict__ out, int* __restrict__ status) {
  if (par != -1) {
    if (*(volatile int*)status == 0) *status = DEVO_FRAME_STATUS_MISSING;      // (an earlier finding — a bad entry, unsorted keyframes — is the cause: it stays)
#pragma unroll
    for (int c = 0; c < 7; c++) out[(int64_t)t * 7 + c] = __uint_as_float(0x7fc00000u);
    return;
  }
  X.inv().store(out + (int64_t)t * 7);
}

__global__ __launch_bounds__(TB) void k_traj_init(const float* __restrict__ poses, const int64_t* __restrict__ tstamps, int n, int counter,
                                                  const int64_t* __restrict__ parent, const float* __restrict__ rel, TrajBuf dst, int final,
                                                  float* __restrict__ out, int* __restrict__ status) {
  const int t = blockIdx.x * TB + threadIdx.x;
  if (t > 0 && t < n && !(tstamps[t] > tstamps[t - 1])) *status = DEVO_FRAME_STATUS_UNSORTED;
  if (t >= counter) return;
  int lo = 0, hi = n;                                          // the first i with tstamps[i] >= t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tstamps[mid] < t) lo = mid + 1; else hi = mid;
  }
  const float* src;
  int par;
  if (lo < n && tstamps[lo] == t) {                            // a keyframe wins over a log entry (`t in self.traj`, devo.py:180)
    src = poses + (int64_t)lo * 7;
    par = -1;
  } else {
    const int64_t p = parent[t];
    src = rel + (int64_t)t * 7;
    par = (p >= 0 && p < t) ? (int)p : -2;                     // -2: no entry; nothing is read through it
  }
  if (final) {
    traj_finish(SE3<float>::load(src), par, t, out, status);
    return;
  }
#pragma unroll
  for (int c = 0; c < 7; c++) dst.acc[(int64_t)t * 7 + c] = par == -2 ? 0.0f : src[c];
  dst.par[t] = par;
}

__global__ __launch_bounds__(TB) void k_traj_round(TrajBuf src, TrajBuf dst, int counter, int final, float* __restrict__ out, int* __restrict__ status) {
  const int t = blockIdx.x * TB + threadIdx.x;
  if (t >= counter) return;
  int par = src.par[t];
  SE3<float> X = SE3<float>::load(src.acc + (int64_t)t * 7);
  if (par >= 0) {
    X = X.mul(SE3<float>::load(src.acc + (int64_t)par * 7));
    par = src.par[par];
  } else if (par == -1 && !final) {                            // a resolved frame is carried over bit for bit
#pragma unroll
    for (int c = 0; c < 7; c++) dst.acc[(int64_t)t * 7 + c] = src.acc[(int64_t)t * 7 + c];
    dst.par[t] = -1;
    return;
  }
  if (final) {
    traj_finish(X, par, t, out, status);
    return;
  }
  X.store(dst.acc + (int64_t)t * 7);
  dst.par[t] = par;
}

inline int traj_rounds(int counter) {                          // the smallest r with 2^r >= counter
  int r = 0;
  while ((1ll << r) < counter) r++;
  return r;
}
inline size_t ws_acc(int counter) { return align_up((size_t)counter * 7 * sizeof(float)); }
inline size_t ws_par(int counter) { return align_up((size_t)counter * sizeof(int)); }

}  // namespace

extern "C" {

int devo_frame_begin(float* poses, float* patches, float* intrinsics, int64_t* tstamps, int N, int M, int P, int n, const float* new_patches,
                     const float* new_intrinsics, int64_t counter, float res, int motion_model, float damping, const float* depth,
                     devo_stream_t stream) {
  DEVO_REQUIRE(poses && patches && intrinsics && tstamps && new_patches && new_intrinsics, "devo_frame_begin: null buffers");
  DEVO_REQUIRE(N > 0 && M > 0 && P > 0 && P <= 1024, "devo_frame_begin: bad sizes");
  DEVO_REQUIRE(n >= 0 && n < N, "devo_frame_begin: row n = %d lies outside the %d rows of the buffers", n, N);
  DEVO_REQUIRE((long long)M * P * P * 3 <= INT32_MAX, "devo_frame_begin: a frame of more than 2^31 patch elements");
  DEVO_REQUIRE(motion_model == DEVO_FRAME_DAMPED_LINEAR || motion_model == DEVO_FRAME_COPY_LAST, "devo_frame_begin: unknown motion model %d", motion_model);
  if (!depth) {
    DEVO_REQUIRE(n >= 3, "devo_frame_begin: the median depth is taken over the last three frames, n = %d", n);
    if ((long long)3 * M * P * P > DEVO_FRAME_MEDIAN_MAX) {
      set_error("devo_frame_begin: the median over %lld depth values exceeds the supported %d", (long long)3 * M * P * P, DEVO_FRAME_MEDIAN_MAX);
      return DEVO_ERR_UNSUPPORTED;
    }
  }
  const BeginArgs a{poses, patches, intrinsics, tstamps, new_patches, new_intrinsics, depth, counter, M, P * P, n, motion_model, res, damping};
  hipLaunchKernelGGL(k_begin_frame, dim3(1), dim3(BF_TB), 0, (hipStream_t)stream, a);
  return check_launch("devo_frame_begin");
}

int devo_frame_point_cloud(const float* poses, const float* patches, const float* intrinsics, const int64_t* ix, int n_poses, int n_patches, int64_t ix_len,
                           int P, int M, int m, int start_frame, float* out, devo_stream_t stream) {
  DEVO_REQUIRE(n_poses > 0 && n_patches >= 0 && P > 0 && M > 0 && start_frame >= 0, "devo_frame_point_cloud: bad sizes");
  DEVO_REQUIRE(m >= 0 && m <= n_patches && m <= ix_len, "devo_frame_point_cloud: m = %d exceeds the %d patches or the %lld entries of ix", m, n_patches, (long long)ix_len);
  const long long first = (long long)start_frame * M;
  if (first >= m) return DEVO_OK;
  DEVO_REQUIRE(poses && patches && intrinsics && ix && out, "devo_frame_point_cloud: null buffers");
  hipLaunchKernelGGL(k_point_cloud, dim3(blocks_for(m - first, TB)), dim3(TB), 0, (hipStream_t)stream, poses, patches, intrinsics, ix, n_poses, P, (int)first, m, out);
  return check_launch("devo_frame_point_cloud");
}

int devo_frame_record_removed(const float* poses, const int64_t* tstamps, int n_poses, int k, int64_t* parent, float* rel, int capacity, int* status,
                              devo_stream_t stream) {
  DEVO_REQUIRE(poses && tstamps && parent && rel && status && capacity > 0, "devo_frame_record_removed: bad arguments");
  DEVO_REQUIRE(k >= 1 && k < n_poses, "devo_frame_record_removed: frame k = %d needs a frame in front of it inside the %d rows", k, n_poses);
  hipLaunchKernelGGL(k_traj_record, dim3(1), dim3(64), 0, (hipStream_t)stream, poses, tstamps, k, (int64_t)0, (int64_t)0, parent, rel, capacity, status);
  return check_launch("devo_frame_record_removed");
}

int devo_frame_record_skipped(int64_t t, int64_t t0, int64_t* parent, float* rel, int capacity, int* status, devo_stream_t stream) {
  DEVO_REQUIRE(parent && rel && status && capacity > 0, "devo_frame_record_skipped: bad arguments");
  DEVO_REQUIRE(t >= 0 && t < capacity, "devo_frame_record_skipped: frame %lld lies outside the capacity %d", (long long)t, capacity);
  DEVO_REQUIRE(t0 >= 0 && t0 < t, "devo_frame_record_skipped: the parent %lld of frame %lld must be an earlier frame", (long long)t0, (long long)t);
  hipLaunchKernelGGL(k_traj_record, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)nullptr, (const int64_t*)nullptr, 0, t, t0, parent, rel, capacity, status);
  return check_launch("devo_frame_record_skipped");
}

size_t devo_frame_complete_workspace_bytes(int counter) { return counter <= 0 ? 0 : 2 * (ws_acc(counter) + ws_par(counter)); }

int devo_frame_complete(const float* poses, const int64_t* tstamps, int n, int counter, const int64_t* parent, const float* rel, int capacity, float* out,
                        void* ws, size_t ws_bytes, int* status, devo_stream_t stream) {
  DEVO_REQUIRE(n >= 0 && counter >= 0 && capacity > 0, "devo_frame_complete: bad sizes");
  DEVO_REQUIRE(counter <= capacity, "devo_frame_complete: counter = %d exceeds the capacity %d", counter, capacity);
  if (counter == 0) return DEVO_OK;
  DEVO_REQUIRE(poses && tstamps && parent && rel && out && status, "devo_frame_complete: null buffers");
  const int rounds = traj_rounds(counter);
  if (rounds > 0 && (ws == nullptr || ws_bytes < devo_frame_complete_workspace_bytes(counter))) { set_error("devo_frame_complete: workspace too small"); return DEVO_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  TrajBuf buf[2];
  buf[0] = TrajBuf{(float*)w, (int*)(w + 2 * ws_acc(counter))};
  buf[1] = TrajBuf{(float*)(w + ws_acc(counter)), (int*)(w + 2 * ws_acc(counter) + ws_par(counter))};
  const dim3 grid(blocks_for(std::max(counter, n), TB)), block(TB);
  hipLaunchKernelGGL(k_traj_init, grid, block, 0, st, poses, tstamps, n, counter, parent, rel, buf[0], rounds == 0 ? 1 : 0, out, status);
  for (int r = 0; r < rounds; r++)
    hipLaunchKernelGGL(k_traj_round, dim3(blocks_for(counter, TB)), block, 0, st, buf[r & 1], buf[(r + 1) & 1], counter, r == rounds - 1 ? 1 : 0, out, status);
  return check_launch("devo_frame_complete");
}

int devo_frame_complete_launches(int counter) { return counter <= 0 ? 0 : 1 + traj_rounds(counter); }

}  // extern "C"
