// The training loss of one update iteration (train.py:172-236, metrics :254-266) on the GPU, wave64, gfx950, fp32 / fp64.
//   * k_flow_edges: one lane per close edge: the P x P residual norms, their minimum and its FIRST position, the mask v > 0.5, the
//     count of pixels below a quarter pixel (px1, unmasked).  Shuffle wave sums, one partial per workgroup.  The adjoint's direction
//     (x - y) / |x - y| at the minimising pixel is kept per edge (zero for an invalid edge or a zero norm): backward only scales it.
//   * k_score_edges / k_score_patches (the last iteration only, train.py:189-203): per edge c = (-log(mean w) / 2 + 1) * min residual
//     under the mask v >= 0.5 (>=, not >: the reference's two masks differ), the sum of c * scores[kk] as workgroup partials; per patch
//     the entropy term -log(max(score, 1e-6)) and its derivative.  The scatter of c over kk: fp32 / fp64 atomics into a vector the
//     patch kernel cleared in front, or (deterministic) the patch kernel behind the edge kernel, every patch adding its edges in
//     ascending edge order.
//   * k_loss_tail, ONE workgroup: the partials added in fp64 in a fixed order, and the pose term (train.py:207-234): both pose sets
//     inverted, the Sim(3) scale of Kabsch-Umeyama s = min(Var / nuclear norm(H), 10) with the singular values of the 3 x 3 H from a
//     one-sided Jacobi iteration in fp64 (no reflection correction, as the reference; finite for a rank-deficient H; H = 0: s = 10),
//     the n (n - 1) ordered pairs, their log, the norms and the fractions below 1e-3 / 1e-2.  The adjoint with respect to Gs (s is a
//     constant, Ps is data) is what lietorch's rules give through inv, scale, index, inv, mul, inv, log and the norms; a pose adds
//     its pairs' terms in ascending partner order (no atomics).  Writes the statistics, the weighted loss and the two 1 / #valid.
//   * k_loss_backward: the kept adjoints times the incoming gradient and the weights -> whole gradients (no memset needed).
// Nothing here synchronises with the host; a run is reproducible bit for bit (but for the atomic scatter).
#include "common.h"
#include "se3_dev.h"

namespace {

using namespace devo;

constexpr int TB = 256;
constexpr int WAVES = TB / 64;
constexpr int PATCHES_PER_WG = 32;          // k_score_patches: 32 patches x 8 edge segments
constexpr int SEGMENTS = TB / PATCHES_PER_WG;
constexpr int NSUM = 12;                    // values the tail adds over the workgroup

struct FlowPartial { double sum; int valid; int px; };
struct ScorePartial { double sum; int valid; int pad; };

inline int tiles(int n, int per = TB) { return n > 0 ? (n + per - 1) / per : 1; }

// ---- layout of `state` (T = the tensors' element type) ------------------------------------------------------------------------
struct Layout {
  size_t aux, dir, arg, gG, gA, gB, c, h, pf, ps, pe, total;
  int nbf, nbs, nbp;
};
Layout layout(int Ec, int n, int Ef, int n_patches, size_t eb) {
  Layout L;
  L.nbf = tiles(Ec); L.nbs = tiles(Ef); L.nbp = tiles(n_patches, PATCHES_PER_WG);
  size_t o = 0;
  L.aux = o; o += align_up(DEVO_LOSS_AUX * eb);
  L.dir = o; o += align_up((size_t)Ec * 2 * eb);
  L.arg = o; o += align_up((size_t)Ec * sizeof(int));
  L.gG = o;  o += align_up((size_t)n * 7 * eb);
  L.gA = o;  o += align_up((size_t)n_patches * eb);
  L.gB = o;  o += align_up((size_t)n_patches * eb);
  L.c = o;   o += align_up((size_t)Ef * eb);
  L.h = o;   o += align_up((size_t)n * n * 6 * eb);
  L.pf = o;  o += align_up((size_t)L.nbf * sizeof(FlowPartial));
  L.ps = o;  o += align_up((size_t)L.nbs * sizeof(ScorePartial));
  L.pe = o;  o += align_up((size_t)L.nbp * sizeof(double));
  L.total = o;
  return L;
}

template <typename T> __device__ __forceinline__ T t_log(T x);
template <> __device__ __forceinline__ float t_log<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double t_log<double>(double x) { return log(x); }

// the minimum of the PP residual norms of one edge and its first position (torch.min: a NaN wins)
template <typename T>
__device__ __forceinline__ T edge_min(const T* __restrict__ x, const T* __restrict__ y, int PP, int& arg, int& below) {
  T m = T(0);
  arg = 0; below = 0;
  for (int p = 0; p < PP; p++) {
    const T dx = x[2 * p] - y[2 * p], dy = x[2 * p + 1] - y[2 * p + 1];
    const T e = t_sqrt<T>(dx * dx + dy * dy);
    below += e < T(0.25) ? 1 : 0;
    if (p == 0 || e < m || (e != e && m == m)) { m = e; arg = p; }
  }
  return m;
}

template <typename T>
__global__ __launch_bounds__(TB) void k_flow_edges(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ v, int Ec, int PP,
                                                   T* __restrict__ dir, int* __restrict__ argmin, FlowPartial* __restrict__ part) {
  const int e = blockIdx.x * TB + threadIdx.x;
  double s = 0.0;
  int nv = 0, px = 0;
  if (e < Ec) {
    const T* xe = x + (size_t)e * PP * 2;
    const T* ye = y + (size_t)e * PP * 2;
    int a, below;
    const T m = edge_min(xe, ye, PP, a, below);
    px = below;
    const bool ok = v[e] > T(0.5);
    T d0 = T(0), d1 = T(0);
    if (ok) {
      s = (double)m; nv = 1;
      if (m > T(0)) { d0 = (xe[2 * a] - ye[2 * a]) / m; d1 = (xe[2 * a + 1] - ye[2 * a + 1]) / m; }      // (a zero norm: zero, as torch's norm)
    }
    dir[2 * e] = d0; dir[2 * e + 1] = d1;
    argmin[e] = ok ? a : -1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o, 64);
    nv += __shfl_down(nv, o, 64);
    px += __shfl_down(px, o, 64);
  }
  __shared__ FlowPartial sh[WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = FlowPartial{s, nv, px};
  __syncthreads();
  if (threadIdx.x == 0) {
    FlowPartial r = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) { r.sum += sh[w].sum; r.valid += sh[w].valid; r.px += sh[w].px; }
    part[blockIdx.x] = r;
  }
}

template <typename T>
__global__ __launch_bounds__(TB) void k_score_edges(const T* __restrict__ scores, int n_patches, const T* __restrict__ v, const T* __restrict__ x,
                                                    const T* __restrict__ y, const T* __restrict__ w, const int64_t* __restrict__ kk, int Ef, int PP,
                                                    int atomic, T* __restrict__ c_out, T* __restrict__ gB, ScorePartial* __restrict__ part) {
  const int e = blockIdx.x * TB + threadIdx.x;
  double s = 0.0;
  int nv = 0;
  if (e < Ef) {
    const int64_t k = kk[e];
    T c = T(0);
    if (v[e] >= T(0.5) && k >= 0 && k < n_patches) {                   // (a patch index outside scores: the edge is not counted, nothing is read)
      int a, below;
      const T m = edge_min(x + (size_t)e * PP * 2, y + (size_t)e * PP * 2, PP, a, below);
      c = (T(-0.5) * t_log<T>((w[2 * e] + w[2 * e + 1]) * T(0.5)) + T(1)) * m;
      s = (double)(c * scores[k]);
      nv = 1;
      if (atomic) atomicAdd(gB + k, c);
    }
    c_out[e] = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o, 64);
    nv += __shfl_down(nv, o, 64);
  }
  __shared__ ScorePartial sh[WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ScorePartial{s, nv, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    ScorePartial r = sh[0];
#pragma unroll
    for (int w2 = 1; w2 < WAVES; w2++) { r.sum += sh[w2].sum; r.valid += sh[w2].valid; }
    part[blockIdx.x] = r;
  }
}

// 32 patches to a workgroup.  gather = 0: clears gB in front of the atomic scatter.  gather = 1 (behind k_score_edges): lane (segment s,
// patch p) adds the c of its patch's edges in segment s in ascending order, the 8 segments are added in order.
template <typename T>
__global__ __launch_bounds__(TB) void k_score_patches(const T* __restrict__ scores, int n_patches, const int64_t* __restrict__ kk, const T* __restrict__ c,
                                                      int Ef, int gather, T* __restrict__ gA, T* __restrict__ gB, double* __restrict__ part) {
  const int pl = threadIdx.x % PATCHES_PER_WG, seg = threadIdx.x / PATCHES_PER_WG;
  const int k = blockIdx.x * PATCHES_PER_WG + pl;
  __shared__ T sh[SEGMENTS][PATCHES_PER_WG];
  __shared__ double sh_e[PATCHES_PER_WG];
  if (gather) {
    const int chunk = (Ef + SEGMENTS - 1) / SEGMENTS;
    const int e0 = seg * chunk, e1 = min(Ef, e0 + chunk);
    T acc = T(0);
    if (k < n_patches)
      for (int e = e0; e < e1; e++)
        if (kk[e] == (int64_t)k) acc += c[e];
    sh[seg][pl] = acc;
  }
  __syncthreads();
  if (seg == 0) {
    double ent = 0.0;
    if (k < n_patches) {
      const T s = scores[k];
      const bool above = s > T(1e-6);
      ent = -(double)t_log<T>(above ? s : T(1e-6));
      gA[k] = above ? T(-1) / (s * T(n_patches)) : T(0);               // d/ds of mean(-log(max(s, 1e-6)))
      T acc = T(0);
      if (gather)
        for (int g = 0; g < SEGMENTS; g++) acc += sh[g][pl];
      gB[k] = acc;
    }
    sh_e[pl] = ent;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    for (int p = 0; p < PATCHES_PER_WG; p++) r += sh_e[p];
    part[blockIdx.x] = r;
  }
}

// the sum of the singular values of a 3 x 3 matrix: one-sided Jacobi (Hestenes) on its columns, fp64.  Columns that are already
// orthogonal (a rank-deficient or zero matrix among them) are left alone: the result is finite whenever the matrix is.
__device__ double nuclear_norm3(double a[3][3]) {
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int k = 0; k < 3; k++) { alpha += a[k][p] * a[k][p]; beta += a[k][q] * a[k][q]; gamma += a[k][p] * a[k][q]; }
        const double bound = 1e-17 * sqrt(alpha * beta);
        if (!(fabs(gamma) > bound) || gamma == 0.0) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int k = 0; k < 3; k++) {
          const double u = a[k][p], w = a[k][q];
          a[k][p] = cs * u - sn * w;
          a[k][q] = sn * u + cs * w;
        }
      }
    if (!rotated) break;
  }
  double s = 0.0;
  for (int q = 0; q < 3; q++) {
    const double n2 = a[0][q] * a[0][q] + a[1][q] * a[1][q] + a[2][q] * a[2][q];
    s += sqrt(n2 > 0.0 ? n2 : 0.0);
  }
  return s;
}

struct TailArgs {
  int Ec, PP, n, n_patches, has_scores, use_pose;
  int nbf, nbs, nbp;
  double flow_weight, pose_weight, scores_weight;
};

template <typename T>
__global__ __launch_bounds__(TB) void k_loss_tail(const T* __restrict__ Gs, const T* __restrict__ Ps, TailArgs a, const FlowPartial* __restrict__ pf,
                                                  const ScorePartial* __restrict__ ps, const double* __restrict__ pe, T* __restrict__ h,
                                                  T* __restrict__ gG, T* __restrict__ aux, T* __restrict__ loss, float* __restrict__ stats) {
  __shared__ T sh_A[DEVO_LOSS_MAX_POSES][7], sh_B[DEVO_LOSS_MAX_POSES][7];      // the inverted pose sets (prediction, ground truth)
  __shared__ double sh_s;
  __shared__ double sh_sum[NSUM][TB];
  const int n = a.n, t = threadIdx.x;
  double acc[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; k++) acc[k] = 0.0;
  // 0 flow sum, 1 flow valid, 2 px1 count, 3 scorer sum, 4 scorer valid, 5 entropy, 6 tr, 7 ro, 8 r1, 9 r2, 10 t1, 11 t2
  for (int b = t; b < a.nbf; b += TB) { acc[0] += pf[b].sum; acc[1] += pf[b].valid; acc[2] += pf[b].px; }
  if (a.has_scores) {
    for (int b = t; b < a.nbs; b += TB) { acc[3] += ps[b].sum; acc[4] += ps[b].valid; }
    for (int b = t; b < a.nbp; b += TB) acc[5] += pe[b];
  }

  if (t < n) {
    SE3<T>::load(Gs + t * 7).inv().store(sh_A[t]);
    SE3<T>::load(Ps + t * 7).inv().store(sh_B[t]);
  }
  __syncthreads();
  if (t == 0) {                                                         // kabsch_umeyama(t2, t1), train.py:54-65, in fp64
    double EA[3] = {0, 0, 0}, EB[3] = {0, 0, 0};
    for (int p = 0; p < n; p++)
      for (int k = 0; k < 3; k++) { EA[k] += (double)sh_B[p][k]; EB[k] += (double)sh_A[p][k]; }
    for (int k = 0; k < 3; k++) { EA[k] /= n; EB[k] /= n; }
    double var = 0.0, H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int p = 0; p < n; p++) {
      double ca[3], cb[3];
      for (int k = 0; k < 3; k++) { ca[k] = (double)sh_B[p][k] - EA[k]; cb[k] = (double)sh_A[p][k] - EB[k]; }
      var += ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) H[r][c] += ca[r] * cb[c];
    }
    var /= n;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) H[r][c] /= n;
    double s = var / nuclear_norm3(H);                                  // x / 0 = +inf -> 10; 0 / 0 = NaN stays NaN, as clamp(max=10)
    if (s > 10.0) s = 10.0;
    sh_s = s;
  }
  __syncthreads();
  const T s = (T)sh_s;
  const int npairs = n * (n - 1);
  const T inv_pairs = T(1) / T(npairs);
  for (int r = t; r < npairs; r += TB) {
    const int i = r / (n - 1), jr = r - i * (n - 1), j = jr + (jr >= i ? 1 : 0);
    SE3<T> Ai = SE3<T>::load(sh_A[i]), Aj = SE3<T>::load(sh_A[j]);
    Ai.t = s * Ai.t; Aj.t = s * Aj.t;                                   // P1.scale(s)
    const SE3<T> Aii = Ai.inv();
    const SE3<T> dP = Aii.mul(Aj);
    const SE3<T> dG = SE3<T>::load(sh_B[i]).inv().mul(SE3<T>::load(sh_B[j]));
    T e[6];
    se3_log<T>(dP.mul(dG.inv()), e);
    const T tr = t_sqrt<T>(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const T ro = t_sqrt<T>(e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
    acc[6] += (double)tr; acc[7] += (double)ro;
    acc[8] += ro < T(0.001) ? 1.0 : 0.0; acc[9] += ro < T(0.01) ? 1.0 : 0.0;
    acc[10] += tr < T(0.001) ? 1.0 : 0.0; acc[11] += tr < T(0.01) ? 1.0 : 0.0;
    // d(mean tr + mean ro) / d e, through log (J_l^-1), the outer mul (left operand: unchanged), then with m = . Adj(Ai'^-1):
    // + m to pose j (right operand of the inner mul), - m to pose i (inv of the left operand)
    T ge[6], gz[6], m[6];
    const T wt = tr > T(0) ? inv_pairs / tr : T(0), wr = ro > T(0) ? inv_pairs / ro : T(0);
    ge[0] = wt * e[0]; ge[1] = wt * e[1]; ge[2] = wt * e[2]; ge[3] = wr * e[3]; ge[4] = wr * e[4]; ge[5] = wr * e[5];
    row_times_left_jacobian_inverse<T>(ge, e, gz);
    Aii.row_times_Adj(gz, m);
#pragma unroll
    for (int k = 0; k < 6; k++) h[(size_t)(i * n + j) * 6 + k] = m[k];
  }
  __threadfence();
  __syncthreads();
  if (t < n) {
    T g[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    for (int q = 0; q < n; q++) {
      if (q == t) continue;
#pragma unroll
      for (int k = 0; k < 6; k++) g[k] += h[(size_t)(q * n + t) * 6 + k] - h[(size_t)(t * n + q) * 6 + k];
    }
    g[0] *= s; g[1] *= s; g[2] *= s;                                    // scale: t * s on the data
    T o[6];
    SE3<T>::load(sh_A[t]).row_times_Adj(g, o);                          // Gs.inv(): - g Adj(Gs^-1)
#pragma unroll
    for (int k = 0; k < 6; k++) gG[t * 7 + k] = -o[k];
    gG[t * 7 + 6] = T(0);
  }

#pragma unroll
  for (int k = 0; k < NSUM; k++) sh_sum[k][t] = acc[k];
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < NSUM; k++) sh_sum[k][t] += sh_sum[k][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double nvf = sh_sum[1][0], nvs = sh_sum[4][0];
    const double flow = sh_sum[0][0] / nvf;                             // 0 / 0: NaN, as mean() of an empty tensor
    const double tr = sh_sum[6][0] / npairs, ro = sh_sum[7][0] / npairs, pose = tr + ro;
    const double sc = a.has_scores ? sh_sum[3][0] / nvs + sh_sum[5][0] / a.n_patches : 0.0;
    double total = a.flow_weight * flow + a.scores_weight * sc;
    if (a.use_pose) total += a.pose_weight * pose;
    stats[0] = (float)flow; stats[1] = (float)pose; stats[2] = (float)tr; stats[3] = (float)ro;
    stats[4] = (float)(sh_sum[2][0] / ((double)a.Ec * a.PP));
    stats[5] = (float)(sh_sum[8][0] / npairs); stats[6] = (float)(sh_sum[9][0] / npairs);
    stats[7] = (float)(sh_sum[10][0] / npairs); stats[8] = (float)(sh_sum[11][0] / npairs);
    stats[9] = (float)sc; stats[10] = (float)sh_s;
    loss[0] = (T)total;
    aux[0] = (T)(nvf > 0.0 ? 1.0 / nvf : 0.0);                          // (no valid edge: the mean of nothing passes no gradient)
    aux[1] = (T)(nvs > 0.0 ? 1.0 / nvs : 0.0);
    aux[2] = (T)flow; aux[3] = (T)pose; aux[4] = (T)sc; aux[5] = (T)sh_s;
  }
}

template <typename T>
__global__ __launch_bounds__(TB) void k_loss_backward(const T* __restrict__ g, const T* __restrict__ aux, const T* __restrict__ dir, const int* __restrict__ argmin,
                                                      const T* __restrict__ gG, const T* __restrict__ gA, const T* __restrict__ gB, int Ec, int PP, int n,
                                                      int n_patches, T fw, T pw, T sw, T* __restrict__ g_coords, T* __restrict__ g_Gs, T* __restrict__ g_scores) {
  const T up = g[0];
  const int64_t n_px = g_coords ? (int64_t)Ec * PP : 0, n_g = g_Gs ? (int64_t)n * 7 : 0, n_s = g_scores ? n_patches : 0;
  const T cf = up * fw * aux[0], cp = up * pw, cs = up * sw, inv_s = aux[1];
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n_px + n_g + n_s; i += (int64_t)gridDim.x * TB) {
    if (i < n_px) {
      const int64_t e = i / PP;
      const bool hit = argmin[e] == (int)(i - e * PP);
      g_coords[2 * i] = hit ? cf * dir[2 * e] : T(0);
      g_coords[2 * i + 1] = hit ? cf * dir[2 * e + 1] : T(0);
    } else if (i < n_px + n_g) {
      const int64_t k = i - n_px;
      g_Gs[k] = cp * gG[k];
    } else {
      const int64_t k = i - n_px - n_g;
      g_scores[k] = cs * (gA[k] + gB[k] * inv_s);
    }
  }
}

template <typename T>
int forward_t(const T* x, const T* y, const T* v, int Ec, int P, const T* Gs, const T* Ps, int n, const T* scores, int n_patches, const T* v_full, const T* x_full,
              const T* y_full, const T* ba_weights, const int64_t* kk, int Ef, int deterministic, double fw, double pw, double sw, int use_pose, T* loss,
              float* stats, char* state, hipStream_t st) {
  const Layout L = layout(Ec, n, Ef, n_patches, sizeof(T));
  const int PP = P * P, has_scores = scores != nullptr;
  T* gA = (T*)(state + L.gA);
  T* gB = (T*)(state + L.gB);
  T* c = (T*)(state + L.c);
  hipLaunchKernelGGL(k_flow_edges<T>, dim3(L.nbf), dim3(TB), 0, st, x, y, v, Ec, PP, (T*)(state + L.dir), (int*)(state + L.arg), (FlowPartial*)(state + L.pf));
  if (has_scores) {
    if (!deterministic)
      hipLaunchKernelGGL(k_score_patches<T>, dim3(L.nbp), dim3(TB), 0, st, scores, n_patches, kk, c, Ef, 0, gA, gB, (double*)(state + L.pe));
    hipLaunchKernelGGL(k_score_edges<T>, dim3(L.nbs), dim3(TB), 0, st, scores, n_patches, v_full, x_full, y_full, ba_weights, kk, Ef, PP, deterministic ? 0 : 1, c, gB,
                       (ScorePartial*)(state + L.ps));
    if (deterministic)
      hipLaunchKernelGGL(k_score_patches<T>, dim3(L.nbp), dim3(TB), 0, st, scores, n_patches, kk, c, Ef, 1, gA, gB, (double*)(state + L.pe));
  }
  const TailArgs a{Ec, PP, n, n_patches, has_scores, use_pose, L.nbf, L.nbs, L.nbp, fw, pw, sw};
  hipLaunchKernelGGL(k_loss_tail<T>, dim3(1), dim3(TB), 0, st, Gs, Ps, a, (const FlowPartial*)(state + L.pf), (const ScorePartial*)(state + L.ps),
                     (const double*)(state + L.pe), (T*)(state + L.h), (T*)(state + L.gG), (T*)(state + L.aux), loss, stats);
  return check_launch("devo_loss_forward");
}

template <typename T>
int backward_t(const T* g, const char* state, int Ec, int P, int n, int Ef, int n_patches, double fw, double pw, double sw, T* g_coords, T* g_Gs, T* g_scores,
               hipStream_t st) {
  const Layout L = layout(Ec, n, Ef, n_patches, sizeof(T));
  const long long work = (g_coords ? (long long)Ec * P * P : 0) + (g_Gs ? n * 7 : 0) + (g_scores ? n_patches : 0);
  if (work == 0) return DEVO_OK;
  hipLaunchKernelGGL(k_loss_backward<T>, dim3(blocks_for(work, TB, 4096)), dim3(TB), 0, st, g, (const T*)(state + L.aux), (const T*)(state + L.dir),
                     (const int*)(state + L.arg), (const T*)(state + L.gG), (const T*)(state + L.gA), (const T*)(state + L.gB), Ec, P * P, n, n_patches, (T)fw, (T)pw,
                     (T)sw, g_coords, g_Gs, g_scores);
  return check_launch("devo_loss_backward");
}

int check_sizes(const char* what, int Ec, int P, int n, int Ef, int n_patches, int dtype) {
  DEVO_REQUIRE(dtype == DEVO_F32 || dtype == DEVO_F64, "%s: dtype must be F32 or F64", what);
  DEVO_REQUIRE(Ec >= 1 && P >= 1 && Ef >= 0 && n_patches >= 0, "%s: bad sizes (Ec = %d, P = %d, Ef = %d, n_patches = %d)", what, Ec, P, Ef, n_patches);
  DEVO_REQUIRE(n >= 2 && n <= DEVO_LOSS_MAX_POSES, "%s: 2 <= n <= %d poses, got %d", what, DEVO_LOSS_MAX_POSES, n);
  return DEVO_OK;
}

}  // namespace

extern "C" {

size_t devo_loss_state_bytes(int Ec, int n, int Ef, int n_patches, int dtype) {
  if (Ec < 0 || n < 0 || Ef < 0 || n_patches < 0 || (dtype != DEVO_F32 && dtype != DEVO_F64)) return 0;
  return layout(Ec, n, Ef, n_patches, dtype == DEVO_F64 ? 8 : 4).total;
}

int devo_loss_forward(const void* x, const void* y, const void* v, int Ec, int P, const void* Gs, const void* Ps, int n, const void* scores, int n_patches,
                      const void* v_full, const void* x_full, const void* y_full, const void* ba_weights, const int64_t* kk, int Ef, int deterministic,
                      double flow_weight, double pose_weight, double scores_weight, int use_pose, void* loss, float* stats, void* state, size_t state_bytes,
                      int dtype, devo_stream_t stream) {
  if (!scores) { Ef = 0; n_patches = 0; }
  if (int rc = check_sizes("devo_loss_forward", Ec, P, n, Ef, n_patches, dtype)) return rc;
  DEVO_REQUIRE(x && y && v && Gs && Ps && loss && stats && state, "devo_loss_forward: null tensor");
  DEVO_REQUIRE(!scores || (n_patches >= 1 && (Ef == 0 || (v_full && x_full && y_full && ba_weights && kk))), "devo_loss_forward: the scorer term needs all its tensors");
  DEVO_REQUIRE(state_bytes >= devo_loss_state_bytes(Ec, n, Ef, n_patches, dtype), "devo_loss_forward: state too small");
  DEVO_REQUIRE(((uintptr_t)state & 15) == 0, "devo_loss_forward: state must be 16-byte aligned");
#define ARGS(T) (const T*)x, (const T*)y, (const T*)v, Ec, P, (const T*)Gs, (const T*)Ps, n, (const T*)scores, n_patches, (const T*)v_full, (const T*)x_full,            \
                (const T*)y_full, (const T*)ba_weights, kk, Ef, deterministic, flow_weight, pose_weight, scores_weight, use_pose, (T*)loss, stats, (char*)state,         \
                (hipStream_t)stream
  return dtype == DEVO_F64 ? forward_t<double>(ARGS(double)) : forward_t<float>(ARGS(float));
#undef ARGS
}

int devo_loss_backward(const void* g, const void* state, size_t state_bytes, int Ec, int P, int n, int Ef, int n_patches, double flow_weight, double pose_weight,
                       double scores_weight, void* g_coords, void* g_Gs, void* g_scores, int dtype, devo_stream_t stream) {
  if (int rc = check_sizes("devo_loss_backward", Ec, P, n, Ef, n_patches, dtype)) return rc;
  DEVO_REQUIRE(g && state, "devo_loss_backward: null tensor");
  DEVO_REQUIRE(state_bytes >= devo_loss_state_bytes(Ec, n, Ef, n_patches, dtype), "devo_loss_backward: state too small");
  DEVO_REQUIRE(!g_scores || n_patches >= 1, "devo_loss_backward: no scorer term was computed");
  if (dtype == DEVO_F64)
    return backward_t<double>((const double*)g, (const char*)state, Ec, P, n, Ef, n_patches, flow_weight, pose_weight, scores_weight, (double*)g_coords, (double*)g_Gs,
                              (double*)g_scores, (hipStream_t)stream);
  return backward_t<float>((const float*)g, (const char*)state, Ec, P, n, Ef, n_patches, flow_weight, pose_weight, scores_weight, (float*)g_coords, (float*)g_Gs,
                           (float*)g_scores, (hipStream_t)stream);
}

}  // extern "C"
