// The growing patch graph of DEVO's training loop (devo/enet.py:297-339 and the edge selections of :359-369) on the GPU, wave64, gfx950.
// The reference starts on the first frames, then adds one frame per iteration: it prepends the new frame's edges, extends the recurrent
// state `net` with zero rows, copies the previous pose, initialises the new depths with a median, sometimes drops the edges of frame
// n - 4, and selects the close (0 < |ii - jj| <= 2) and far (<= 16) edges every iteration.  Here one growth is three launches:
//   * k_tg_frame: ONE workgroup of 1024 threads writes poses' (row n = row n - 1) and patches' (channel 2 of frame n = the LOWER median
//     of channel 2 of frames n - 2 and n - 1, the exact radix select of median_select.h) as NEW tensors; everything else is copied.
//   * k_tg_count / k_tg_scatter: a STABLE three-way stream compaction over the VIRTUAL edge list [new edges | old edges].  A new edge is
//     computed from its position (no index tensors are built), an old one is read.  Per tile the number of survivors, of close survivors
//     and of far survivors: 64-bit ballot + popcount per wave; workgroup offsets from the counts of the tiles in front.  The scatter
//     writes the survivors' (ii, jj, kk), the rows of net' (zero rows for new edges, 16-byte words), the old-row -> new-row map the
//     adjoint needs, and the close / far lists (position in the new list and the gathered triple).  Without a drop every edge survives and
//     the same two kernels run.  All totals are known on the host: nothing is read back.
//   * k_tg_net_backward: the adjoint of net -> net' under a drop: grad_old[r] = 0 + grad_new[map[r]], zero for a dropped row.  A gather:
//     every old row has at most one image.  (Without a drop the adjoint is a slice and launches nothing.)
// The initial graph is the same pair of kernels over a virtual list of new edges only.  Every scatter store is guarded by its buffer's
// capacity.  Nothing here synchronises with the host; no float atomics.
#include <algorithm>
#include "common.h"
#include "median_select.h"

namespace {

using namespace devo;

constexpr int TB = 256;                     // 4 waves of 64
constexpr int WAVES = TB / 64;
constexpr int FR_TB = 1024;                                   // k_tg_frame: 16 waves
constexpr int FR_KEYS = DEVO_FRAME_MEDIAN_MAX / FR_TB;        // keys per thread
static_assert(FR_KEYS * FR_TB == DEVO_FRAME_MEDIAN_MAX, "median bound");

inline int tiles(long long E) { return E > 0 ? (int)((E + TB - 1) / TB) : 1; }

// the virtual edge list: n_new edges in closed form, then the E_old edges of `ii, jj, kk`
struct Virtual {
  const int64_t* ii; const int64_t* jj; const int64_t* kk;
  int E_old, n_new, M, n, init;            // init: the initial graph on n frames; else the growth to frame n
  int drop;                                // frame whose edges go (enet.py:332), or a negative number
};

__device__ __forceinline__ void edge_at(const Virtual& v, int e, int64_t& a, int64_t& b, int64_t& c) {
  if (e >= v.n_new) { a = v.ii[e - v.n_new]; b = v.jj[e - v.n_new]; c = v.kk[e - v.n_new]; return; }
  if (v.init) {                            // flatmeshgrid(where(ix < n), arange(n)): enet.py:300-301
    c = e / v.n; b = e - (int)c * v.n; a = c / v.M;
    return;
  }
  const int first = v.n * v.M;             // flatmeshgrid(where(ix < n), [n]) then flatmeshgrid(where(ix == n), arange(n + 1)): enet.py:321-322
  if (e < first) { c = e; b = v.n; a = e / v.M; return; }
  const int r = e - first, q = r / (v.n + 1);
  c = first + q; b = r - q * (v.n + 1); a = v.n;
}

// bit 0: survives, bit 1: close, bit 2: far
__device__ __forceinline__ int classify(const Virtual& v, int64_t a, int64_t b) {
  if (a == v.drop || b == v.drop) return 0;
  const int64_t d = a > b ? a - b : b - a;
  return 1 | ((d > 0 && d <= 2) ? 2 : 0) | ((d > 0 && d <= 16) ? 4 : 0);
}

__global__ __launch_bounds__(TB) void k_tg_count(Virtual v, int* __restrict__ counts) {
  const int e = blockIdx.x * TB + threadIdx.x;
  int f = 0;
  if (e < v.n_new + v.E_old) {
    int64_t a, b, c;
    edge_at(v, e, a, b, c);
    f = classify(v, a, b);
  }
  const unsigned long long b0 = __ballot(f & 1), b1 = __ballot(f & 2), b2 = __ballot(f & 4);
  __shared__ int sh[3][WAVES];
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = __popcll(b0); sh[1][threadIdx.x >> 6] = __popcll(b1); sh[2][threadIdx.x >> 6] = __popcll(b2); }
  __syncthreads();
  if (threadIdx.x < 3) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += sh[threadIdx.x][w];
    counts[3 * blockIdx.x + threadIdx.x] = s;
  }
}

struct Lists { int64_t* idx; long long idx_cap; int64_t* close; long long close_cap; int64_t* far; long long far_cap; };     // rows of `cap` entries each

__device__ __forceinline__ void list_store(int64_t* list, long long cap, long long at, int64_t pos, int64_t a, int64_t b, int64_t c) {
  if (at < cap) { list[at] = pos; list[cap + at] = a; list[2 * cap + at] = b; list[3 * cap + at] = c; }
}

__global__ __launch_bounds__(TB) void k_tg_scatter(Virtual v, const int* __restrict__ counts, Lists out, const uint4* __restrict__ net_old,
                                                   uint4* __restrict__ net_new, int cpr, int E_new, int* __restrict__ map) {
  __shared__ int sh_wave[3][WAVES];
  __shared__ int sh_off[3][WAVES];
  __shared__ int sh_src[TB];
  // this workgroup's offsets: the counts of the workgroups in front
  int p0 = 0, p1 = 0, p2 = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += TB) { p0 += counts[3 * b]; p1 += counts[3 * b + 1]; p2 += counts[3 * b + 2]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { p0 += __shfl_down(p0, o, 64); p1 += __shfl_down(p1, o, 64); p2 += __shfl_down(p2, o, 64); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh_off[0][wave] = p0; sh_off[1][wave] = p1; sh_off[2][wave] = p2; }

  const int e = blockIdx.x * TB + threadIdx.x;
  const bool live = e < v.n_new + v.E_old;
  int f = 0;
  int64_t a = 0, b = 0, c = 0;
  if (live) {
    edge_at(v, e, a, b, c);
    f = classify(v, a, b);
  }
  const unsigned long long bal[3] = {__ballot(f & 1), __ballot(f & 2), __ballot(f & 4)};
  if (lane == 0) { sh_wave[0][wave] = __popcll(bal[0]); sh_wave[1][wave] = __popcll(bal[1]); sh_wave[2][wave] = __popcll(bal[2]); }
  __syncthreads();
  int offset[3], rank[3], kept = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    int off = 0, before = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { off += sh_off[s][w]; if (w < wave) before += sh_wave[s][w]; if (s == 0) kept += sh_wave[0][w]; }
    offset[s] = off;
    rank[s] = before + __popcll(bal[s] & below);
  }
  const long long d = (long long)offset[0] + rank[0];
  if (f & 1) {
    if (d < out.idx_cap) { out.idx[d] = a; out.idx[out.idx_cap + d] = b; out.idx[2 * out.idx_cap + d] = c; }
    sh_src[rank[0]] = e;
    if (f & 2) list_store(out.close, out.close_cap, (long long)offset[1] + rank[1], d, a, b, c);
    if (f & 4) list_store(out.far, out.far_cap, (long long)offset[2] + rank[2], d, a, b, c);
  }
  if (map && live && e >= v.n_new) map[e - v.n_new] = (f & 1) ? (int)d : -1;
  if (cpr == 0) return;
  __syncthreads();
  // rows of net': the surviving rows of this tile, 16 bytes per lane; a new edge's row is zero
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int t = threadIdx.x; t < kept * cpr; t += TB) {
    const int r = t / cpr, col = t - r * cpr;
    const long long row = (long long)offset[0] + r;
    const int src = sh_src[r];
    if (row < E_new) net_new[row * cpr + col] = src < v.n_new ? zero : net_old[(long long)(src - v.n_new) * cpr + col];
  }
}

// 0 + x in the row's format, on the bits: -0 becomes +0, everything else stays.  The torch composition's adjoint of net[:, keep] is
// zeros.index_put_(accumulate=True): it ADDS the gathered row to a zero row, and the results are compared bit for bit.
template <bool F16>
__device__ __forceinline__ unsigned add_to_zero(unsigned w) {
  if (!F16) return w == 0x80000000u ? 0u : w;
  if ((w & 0xffffu) == 0x8000u) w &= 0xffff0000u;
  if ((w >> 16) == 0x8000u) w &= 0x0000ffffu;
  return w;
}

template <bool F16>
__global__ __launch_bounds__(TB) void k_tg_net_backward(const uint4* __restrict__ grad_new, const int* __restrict__ map, uint4* __restrict__ grad_old,
                                                        int E_old, int E_new, int cpr) {
  const long long total = (long long)E_old * cpr, stride = (long long)gridDim.x * TB;
  for (long long t = (long long)blockIdx.x * TB + threadIdx.x; t < total; t += stride) {
    const long long r = t / cpr;
    const int col = (int)(t - r * cpr), d = map[r];
    uint4 g = make_uint4(0u, 0u, 0u, 0u);
    if (d >= 0 && d < E_new) {
      g = grad_new[(long long)d * cpr + col];
      g.x = add_to_zero<F16>(g.x); g.y = add_to_zero<F16>(g.y); g.z = add_to_zero<F16>(g.z); g.w = add_to_zero<F16>(g.w);
    }
    grad_old[t] = g;
  }
}

// poses' and patches' of the growth to frame n (1 <= n < N), as new tensors (enet.py:320, :338)
__global__ __launch_bounds__(FR_TB) void k_tg_frame(const unsigned* __restrict__ poses_in, unsigned* __restrict__ poses_out, int N,
                                                    const float* __restrict__ patches_in, float* __restrict__ patches_out, int M, int PP, int n) {
  const int tid = threadIdx.x;
  const int lo = n >= 2 ? n - 2 : 0;                          // (ix == n - 1) | (ix == n - 2)
  const int count = (n - lo) * M * PP;                        // <= DEVO_FRAME_MEDIAN_MAX (the host refuses more)
  const float* src = patches_in + (long long)lo * M * 3 * PP;
  unsigned keys[FR_KEYS];
  bool nan = false;
#pragma unroll
  for (int s = 0; s < FR_KEYS; s++) {
    const int i = s * FR_TB + tid;
    keys[s] = 0u;
    if (i < count) {
      const int patch = i / PP, p = i - patch * PP;           // patch counts over the two frames
      const float x = src[((long long)patch * 3 + 2) * PP + p];
      nan |= x != x;
      keys[s] = fkey(x);
    }
  }
  const float med = select_lower_median<FR_TB, FR_KEYS>(keys, nan, count, tid);
  for (int i = tid; i < N * 7; i += FR_TB) {
    const int row = i / 7;
    poses_out[i] = row == n ? poses_in[i - 7] : poses_in[i];
  }
  const long long first = (long long)n * M * 3 * PP, last = first + (long long)M * 3 * PP, total = (long long)N * M * 3 * PP;
  for (long long i = tid; i < total; i += FR_TB) {
    float x = patches_in[i];
    if (i >= first && i < last && ((i - first) / PP) % 3 == 2) x = med;
    patches_out[i] = x;
  }
}

int elem_bytes(int dtype) { return dtype == DEVO_F16 ? 2 : dtype == DEVO_F32 ? 4 : 0; }

size_t ws_total(long long capacity) { return align_up((size_t)tiles(capacity) * 3 * sizeof(int)); }

int launch_lists(const char* what, const Virtual& v, const Lists& out, const void* net_old, void* net_new, int cpr, int E_new, int* map, void* ws,
                 size_t ws_bytes, hipStream_t st) {
  const long long E = (long long)v.n_new + v.E_old;
  DEVO_REQUIRE(ws && ws_bytes >= ws_total(E), "%s: workspace too small", what);
  DEVO_REQUIRE(out.idx && out.close && out.far && out.idx_cap >= E_new && out.close_cap >= 0 && out.far_cap >= 0, "%s: bad output buffers", what);
  const int nb = tiles(E);
  int* counts = (int*)ws;
  hipLaunchKernelGGL(k_tg_count, dim3(nb), dim3(TB), 0, st, v, counts);
  hipLaunchKernelGGL(k_tg_scatter, dim3(nb), dim3(TB), 0, st, v, counts, out, (const uint4*)net_old, (uint4*)net_new, cpr, E_new, map);
  return check_launch(what);
}

}  // namespace

extern "C" {

size_t devo_train_graph_workspace_bytes(int capacity) { return capacity < 0 ? 0 : ws_total(capacity); }

int devo_train_graph_init(int64_t* idx, int64_t idx_cap, int M, int init_frames, int64_t* close, int64_t close_cap, int64_t* far_, int64_t far_cap,
                          void* ws, size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(M > 0 && init_frames > 0 && init_frames <= DEVO_TRAIN_GRAPH_MAX_FRAMES, "devo_train_graph_init: bad sizes (M = %d, init_frames = %d)", M, init_frames);
  const long long E = (long long)init_frames * init_frames * M;
  DEVO_REQUIRE(E <= (1ll << 30) && E <= idx_cap, "devo_train_graph_init: %lld edges exceed the capacity %lld", E, (long long)idx_cap);
  const Virtual v{nullptr, nullptr, nullptr, 0, (int)E, M, init_frames, 1, -1};
  const Lists out{idx, idx_cap, close, close_cap, far_, far_cap};
  return launch_lists("devo_train_graph_init", v, out, nullptr, nullptr, 0, (int)E, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int devo_train_graph_grow(const int64_t* src_idx, int64_t src_cap, int E_old, int64_t* dst_idx, int64_t dst_cap, int E_new, int M, int n, int drop,
                          const void* net_old, void* net_new, int dim, int net_dtype, int* map, const float* poses_in, float* poses_out, int N,
                          const float* patches_in, float* patches_out, int P, int64_t* close, int64_t close_cap, int64_t* far_, int64_t far_cap, void* ws,
                          size_t ws_bytes, devo_stream_t stream) {
  DEVO_REQUIRE(M > 0 && P > 0 && N <= DEVO_TRAIN_GRAPH_MAX_FRAMES && n >= 1 && n < N, "devo_train_graph_grow: bad sizes (M = %d, P = %d, N = %d, n = %d)", M, P, N, n);
  DEVO_REQUIRE(2ll * M * P * P <= DEVO_FRAME_MEDIAN_MAX, "devo_train_graph_grow: the median selects from at most %d values, got 2 * %d * %d * %d", DEVO_FRAME_MEDIAN_MAX, M, P, P);
  const long long n_new = (long long)M * (2 * n + 1), E = n_new + E_old;
  DEVO_REQUIRE(E_old >= 0 && E_old <= src_cap && E <= (1ll << 30) && E_new >= 0 && E_new <= E && E_new <= dst_cap, "devo_train_graph_grow: bad edge counts (%d old, %d new)", E_old, E_new);
  DEVO_REQUIRE(src_idx && dst_idx && src_idx != dst_idx, "devo_train_graph_grow: the new index buffer must not be the old one");
  DEVO_REQUIRE(!drop || map, "devo_train_graph_grow: a drop needs the row map");
  DEVO_REQUIRE(poses_in && poses_out && patches_in && patches_out && poses_in != poses_out && patches_in != patches_out, "devo_train_graph_grow: poses' and patches' are new tensors");
  const int eb = elem_bytes(net_dtype);
  DEVO_REQUIRE(eb != 0, "devo_train_graph_grow: net must be fp16 or fp32");
  DEVO_REQUIRE(dim > 0 && dim % 8 == 0, "devo_train_graph_grow: dim must be a positive multiple of 8 (rows move as 16-byte words), got %d", dim);
  DEVO_REQUIRE(net_new && (net_old || E_old == 0) && net_new != net_old && ((uintptr_t)net_old & 15) == 0 && ((uintptr_t)net_new & 15) == 0, "devo_train_graph_grow: net and net' must be distinct and 16-byte aligned");
  hipLaunchKernelGGL(k_tg_frame, dim3(1), dim3(FR_TB), 0, (hipStream_t)stream, (const unsigned*)poses_in, (unsigned*)poses_out, N, patches_in, patches_out, M, P * P, n);
  const Virtual v{src_idx, src_idx + src_cap, src_idx + 2 * src_cap, E_old, (int)n_new, M, n, 0, drop ? n - 4 : -1};
  const Lists out{dst_idx, dst_cap, close, close_cap, far_, far_cap};
  return launch_lists("devo_train_graph_grow", v, out, net_old, net_new, dim * eb / 16, E_new, drop ? map : nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int devo_train_graph_net_backward(const void* grad_new, const int* map, void* grad_old, int E_old, int E_new, int dim, int net_dtype, devo_stream_t stream) {
  const int eb = elem_bytes(net_dtype);
  DEVO_REQUIRE(eb != 0 && dim > 0 && dim % 8 == 0, "devo_train_graph_net_backward: fp16 or fp32 rows of a multiple of 8 values");
  DEVO_REQUIRE(E_old >= 0 && E_new >= 0 && map && grad_old && (grad_new || E_new == 0), "devo_train_graph_net_backward: bad arguments");
  DEVO_REQUIRE(((uintptr_t)grad_new & 15) == 0 && ((uintptr_t)grad_old & 15) == 0, "devo_train_graph_net_backward: the gradients must be 16-byte aligned");
  if (E_old == 0) return DEVO_OK;
  const int cpr = dim * eb / 16;
  const dim3 grid(blocks_for((long long)E_old * cpr, TB, 8192));
  if (net_dtype == DEVO_F16) hipLaunchKernelGGL(k_tg_net_backward<true>, grid, dim3(TB), 0, (hipStream_t)stream, (const uint4*)grad_new, map, (uint4*)grad_old, E_old, E_new, cpr);
  else hipLaunchKernelGGL(k_tg_net_backward<false>, grid, dim3(TB), 0, (hipStream_t)stream, (const uint4*)grad_new, map, (uint4*)grad_old, E_old, E_new, cpr);
  return check_launch("devo_train_graph_net_backward");
}

}  // extern "C"
