// Batched group ops of SO3, RxSO3, SE3 and Sim3 for gfx950, and their orthogonal projector: one group element per lane, grid-stride,
// fp32 / fp64, one kernel set templated on (group, scalar).  Replaces the group dispatch of the reference's Eigen-templated kernels
// (devo/lietorch/src/lietorch_gpu.cu:20-294, dispatch.h) behind lietorch_backends.* (lietorch.cpp:286-316).
// The entry points devo_lie_* take the group id; devo_se3_* are devo_lie_*(3, ...).  The maths is lie_dev.h's; SE3 computes with se3_dev.h there.
// These ops are launch/latency bound (batch = E .. 9E elements of 16-64 B): one launch per op with coalesced rows staged through registers.
// No LDS, no atomics, no cross-lane traffic: every lane reads rows i of its operands and writes rows i of its outputs.
#include "common.h"
#include "lie_dev.h"

namespace devo {

#define LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)blockDim.x * gridDim.x)
#define GN LieG<G>::N
#define GK LieG<G>::K

// exp_bwd, log_bwd, adj_bwd, adjT_bwd and jinv have an SE3 body of their own: se3_dev.h on the operands in memory, the loads in this order.
// It is there for the bits (lie_dev.h, "SE3"): another order of the loads changes which multiplies become fmas, hence last bits.
template <int G, typename T> __global__ void __launch_bounds__(256) kg_exp(const T* a, T* X, int64_t n) {
  LOOP(i, n) { elem_store<G, T>(lie_exp<G, T>(tan_load<G, T>(a + i * GK)), X + i * GN); }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_exp_bwd(const T* grad, const T* a, T* da, int64_t n) {
  LOOP(i, n) {                                                                          // lietorch_gpu.cu:32-44
    if constexpr (G == 3) row_times_left_jacobian<T>(grad + i * GN, a + i * GK, da + i * GK);
    else tan_store<G, T>(row_times_jl<G, T>(tan_load<G, T>(grad + i * GN), tan_load<G, T>(a + i * GK)), da + i * GK);
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_log(const T* X, T* a, int64_t n) {
  LOOP(i, n) { tan_store<G, T>(lie_log<G, T>(elem_load<G, T>(X + i * GN)), a + i * GK); }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_log_bwd(const T* grad, const T* X, T* dX, int64_t n) {
  LOOP(i, n) {                                                                          // :58-70
    if constexpr (G == 3) {
      T a[6], o[6];
      se3_log<T>(SE3<T>::load(X + i * GN), a);
      row_times_left_jacobian_inverse<T>(grad + i * GK, a, o);
      grad_store<G, T>(tan_load<G, T>(o), dX + i * GN);
    } else {
      const Tan<T> a = lie_log<G, T>(elem_load<G, T>(X + i * GN));
      grad_store<G, T>(row_times_jl_inv<G, T>(tan_load<G, T>(grad + i * GK), a), dX + i * GN);
    }
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_inv(const T* X, T* Y, int64_t n) {
  LOOP(i, n) { elem_store<G, T>(elem_inv(elem_load<G, T>(X + i * GN)), Y + i * GN); }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_inv_bwd(const T* grad, const T* X, T* dX, int64_t n) {
  LOOP(i, n) {                                                                          // :85-97  -dY * Adj(X^-1)
    const Elem<T> Y = elem_inv(elem_load<G, T>(X + i * GN));
    grad_store<G, T>(tan_neg(elem_adjT<G>(Y, tan_load<G, T>(grad + i * GN))), dX + i * GN);
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_mul(const T* X, const T* Y, T* Z, int64_t n) {
  LOOP(i, n) { elem_store<G, T>(elem_mul(elem_load<G, T>(X + i * GN), elem_load<G, T>(Y + i * GN)), Z + i * GN); }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_mul_bwd(const T* grad, const T* X, T* dX, T* dY, int64_t n) {
  LOOP(i, n) {                                                                          // :112-125
    const Tan<T> g = tan_load<G, T>(grad + i * GN);
    grad_store<G, T>(g, dX + i * GN);
    grad_store<G, T>(elem_adjT<G>(elem_load<G, T>(X + i * GN), g), dY + i * GN);
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_adj(const T* X, const T* a, T* b, int64_t n) {
  LOOP(i, n) { tan_store<G, T>(elem_adj<G>(elem_load<G, T>(X + i * GN), tan_load<G, T>(a + i * GK)), b + i * GK); }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_adj_bwd(const T* grad, const T* X, const T* a, T* dX, T* da, int64_t n) {
  LOOP(i, n) {                                                                          // :140-157
    if constexpr (G == 3) {
      const SE3<T> S = SE3<T>::load(X + i * GN);
      T b[6], o[6], db[6];
#pragma unroll
      for (int k = 0; k < 6; k++) db[k] = grad[i * GK + k];
      S.adj(a + i * GK, b);
      S.row_times_Adj(db, da + i * GK);
      row_times_small_adj<T>(db, b, o);
      grad_store<G, T>(tan_neg(tan_load<G, T>(o)), dX + i * GN);
    } else {
      const Elem<T> E = elem_load<G, T>(X + i * GN);
      const Tan<T> db = tan_load<G, T>(grad + i * GK), b = elem_adj<G>(E, tan_load<G, T>(a + i * GK));
      tan_store<G, T>(elem_adjT<G>(E, db), da + i * GK);
      grad_store<G, T>(tan_neg(row_times_ad<G>(db, b)), dX + i * GN);
    }
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_adjT(const T* X, const T* a, T* b, int64_t n) {
  LOOP(i, n) { tan_store<G, T>(elem_adjT<G>(elem_load<G, T>(X + i * GN), tan_load<G, T>(a + i * GK)), b + i * GK); }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_adjT_bwd(const T* grad, const T* X, const T* a, T* dX, T* da, int64_t n) {
  LOOP(i, n) {                                                                          // :173-188
    if constexpr (G == 3) {
      const SE3<T> S = SE3<T>::load(X + i * GN);
      T Adb[6], o[6], av[6];
#pragma unroll
      for (int k = 0; k < 6; k++) av[k] = a[i * GK + k];
      S.adj(grad + i * GK, Adb);
#pragma unroll
      for (int k = 0; k < 6; k++) da[i * GK + k] = Adb[k];
      row_times_small_adj<T>(av, Adb, o);
      grad_store<G, T>(tan_neg(tan_load<G, T>(o)), dX + i * GN);
    } else {
      const Tan<T> Adb = elem_adj<G>(elem_load<G, T>(X + i * GN), tan_load<G, T>(grad + i * GK));
      tan_store<G, T>(Adb, da + i * GK);
      grad_store<G, T>(tan_neg(row_times_ad<G>(tan_load<G, T>(a + i * GK), Adb)), dX + i * GN);
    }
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_act(const T* X, const T* p, T* q, int64_t n) {
  LOOP(i, n) {
    const V3<T> r = elem_act(elem_load<G, T>(X + i * GN), V3<T>{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]});
    q[i * 3] = r.x; q[i * 3 + 1] = r.y; q[i * 3 + 2] = r.z;
  }
}
// The point Jacobians (so3.h:210-220, rxso3.h:302-315, se3.h:203-217, sim3.h:193-209) at q = X p:  [w I, hat(-q), q] for (tau, phi, sigma),
// w = 1 for 3-points;  g * hat(-q) = q x g.
template <int G, typename T> __global__ void __launch_bounds__(256) kg_act_bwd(const T* grad, const T* X, const T* p, T* dX, T* dp, int64_t n) {
  LOOP(i, n) {                                                                          // :204-221
    const Elem<T> E = elem_load<G, T>(X + i * GN);
    const V3<T> g{grad[i * 3], grad[i * 3 + 1], grad[i * 3 + 2]};
    const V3<T> pp = elem_act(E, V3<T>{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]});
    const V3<T> d = row_times_sR<G>(g, E);
    dp[i * 3] = d.x; dp[i * 3 + 1] = d.y; dp[i * 3 + 2] = d.z;
    grad_store<G, T>(Tan<T>{g, cross(pp, g), dot(g, pp)}, dX + i * GN);
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_act4(const T* X, const T* p, T* q, int64_t n) {
  LOOP(i, n) {                                                                          // so3.h:62-65, rxso3.h:65-68, se3.h:53-56, sim3.h:60-63
    const Elem<T> E = elem_load<G, T>(X + i * GN);
    const T w = p[i * 4 + 3];
    const V3<T> r = E.s * qrot(E.q, V3<T>{p[i * 4], p[i * 4 + 1], p[i * 4 + 2]}) + w * E.t;
    q[i * 4] = r.x; q[i * 4 + 1] = r.y; q[i * 4 + 2] = r.z; q[i * 4 + 3] = w;
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_act4_bwd(const T* grad, const T* X, const T* p, T* dX, T* dp, int64_t n) {
  LOOP(i, n) {                                                                          // :238-256
    const Elem<T> E = elem_load<G, T>(X + i * GN);
    const V3<T> g{grad[i * 4], grad[i * 4 + 1], grad[i * 4 + 2]};
    const T g3 = grad[i * 4 + 3], w = p[i * 4 + 3];
    const V3<T> pp = E.s * qrot(E.q, V3<T>{p[i * 4], p[i * 4 + 1], p[i * 4 + 2]}) + w * E.t;
    const V3<T> d = row_times_sR<G>(g, E);                                              // dq * Matrix4x4: first 3 columns g (sR), last g.t + g3
    dp[i * 4] = d.x; dp[i * 4 + 1] = d.y; dp[i * 4 + 2] = d.z; dp[i * 4 + 3] = dot(g, E.t) + g3;
    grad_store<G, T>(Tan<T>{w * g, cross(pp, g), dot(g, pp)}, dX + i * GN);
  }
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_as_matrix(const T* X, T* M, int64_t n) {
  LOOP(i, n) { elem_matrix4(elem_load<G, T>(X + i * GN), M + i * 16); }                  // :258-269
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_projector(const T* X, T* P, int64_t n) {
  LOOP(i, n) { elem_projector<G, T>(elem_load<G, T>(X + i * GN), P + i * (GN * GN)); }   // :271-280
}
template <int G, typename T> __global__ void __launch_bounds__(256) kg_jinv(const T* X, const T* a, T* b, int64_t n) {
  LOOP(i, n) {                                                                          // :283-294
    if constexpr (G == 3) {
      T l[6];
      se3_log<T>(SE3<T>::load(X + i * GN), l);
      left_jacobian_inverse_times<T>(l, a + i * GK, b + i * GK);
    } else {
      const Tan<T> l = lie_log<G, T>(elem_load<G, T>(X + i * GN));
      tan_store<G, T>(jl_inv_times<G, T>(l, tan_load<G, T>(a + i * GK)), b + i * GK);
    }
  }
}

}  // namespace devo

using namespace devo;

#define CP(x) ((const T*)(x))
#define MP(x) ((T*)(x))
#define LIE_LAUNCH(GID, KERNEL, ...)                                                                                           \
  {                                                                                                                            \
    constexpr int G = GID;                                                                                                     \
    if (dtype == DEVO_F32) { typedef float T; hipLaunchKernelGGL((KERNEL<G, T>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); } \
    else { typedef double T; hipLaunchKernelGGL((KERNEL<G, T>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__); }                \
  }
#define LIE_DISPATCH(NAME, KERNEL, ...)                                                                  \
  do {                                                                                                   \
    if (group < 1 || group > 4) { set_error(NAME ": group id must be 1 (SO3), 2 (RxSO3), 3 (SE3) or 4 (Sim3), got %d", group); return DEVO_ERR_ARG; } \
    if (n < 0) { set_error(NAME ": negative batch"); return DEVO_ERR_ARG; }                              \
    if (dtype != DEVO_F32 && dtype != DEVO_F64) { set_error(NAME ": dtype must be F32 or F64"); return DEVO_ERR_UNSUPPORTED; } \
    if (n == 0) return DEVO_OK;                                                                          \
    hipStream_t st = (hipStream_t)s;                                                                     \
    const int blocks = blocks_for(n, 256, 4096);                                                         \
    if (group == 1) LIE_LAUNCH(1, KERNEL, __VA_ARGS__)                                                   \
    else if (group == 2) LIE_LAUNCH(2, KERNEL, __VA_ARGS__)                                              \
    else if (group == 3) LIE_LAUNCH(3, KERNEL, __VA_ARGS__)                                              \
    else LIE_LAUNCH(4, KERNEL, __VA_ARGS__)                                                              \
    return check_launch(NAME);                                                                           \
  } while (0)

extern "C" {

int devo_lie_exp(int group, const void* a, void* X, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_exp", kg_exp, CP(a), MP(X), n); }
int devo_lie_exp_backward(int group, const void* grad, const void* a, void* da, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_exp_backward", kg_exp_bwd, CP(grad), CP(a), MP(da), n); }
int devo_lie_log(int group, const void* X, void* a, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_log", kg_log, CP(X), MP(a), n); }
int devo_lie_log_backward(int group, const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_log_backward", kg_log_bwd, CP(grad), CP(X), MP(dX), n); }
int devo_lie_inv(int group, const void* X, void* Y, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_inv", kg_inv, CP(X), MP(Y), n); }
int devo_lie_inv_backward(int group, const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_inv_backward", kg_inv_bwd, CP(grad), CP(X), MP(dX), n); }
int devo_lie_mul(int group, const void* X, const void* Y, void* Z, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_mul", kg_mul, CP(X), CP(Y), MP(Z), n); }
int devo_lie_mul_backward(int group, const void* grad, const void* X, const void* Y, void* dX, void* dY, int64_t n, int dtype, devo_stream_t s) { (void)Y; LIE_DISPATCH("devo_lie_mul_backward", kg_mul_bwd, CP(grad), CP(X), MP(dX), MP(dY), n); }
int devo_lie_adj(int group, const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_adj", kg_adj, CP(X), CP(a), MP(b), n); }
int devo_lie_adj_backward(int group, const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_adj_backward", kg_adj_bwd, CP(grad), CP(X), CP(a), MP(dX), MP(da), n); }
int devo_lie_adjT(int group, const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_adjT", kg_adjT, CP(X), CP(a), MP(b), n); }
int devo_lie_adjT_backward(int group, const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_adjT_backward", kg_adjT_bwd, CP(grad), CP(X), CP(a), MP(dX), MP(da), n); }
int devo_lie_act(int group, const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_act", kg_act, CP(X), CP(p), MP(q), n); }
int devo_lie_act_backward(int group, const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_act_backward", kg_act_bwd, CP(grad), CP(X), CP(p), MP(dX), MP(dp), n); }
int devo_lie_act4(int group, const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_act4", kg_act4, CP(X), CP(p), MP(q), n); }
int devo_lie_act4_backward(int group, const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_act4_backward", kg_act4_bwd, CP(grad), CP(X), CP(p), MP(dX), MP(dp), n); }
int devo_lie_as_matrix(int group, const void* X, void* T44, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_as_matrix", kg_as_matrix, CP(X), MP(T44), n); }
int devo_lie_jinv(int group, const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_jinv", kg_jinv, CP(X), CP(a), MP(b), n); }
int devo_lie_projector(int group, const void* X, void* P, int64_t n, int dtype, devo_stream_t s) { LIE_DISPATCH("devo_lie_projector", kg_projector, CP(X), MP(P), n); }

// the SE3 entry points of earlier ABI versions: group id 3
int devo_se3_exp(const void* a, void* X, int64_t n, int dtype, devo_stream_t s) { return devo_lie_exp(3, a, X, n, dtype, s); }
int devo_se3_exp_backward(const void* grad, const void* a, void* da, int64_t n, int dtype, devo_stream_t s) { return devo_lie_exp_backward(3, grad, a, da, n, dtype, s); }
int devo_se3_log(const void* X, void* a, int64_t n, int dtype, devo_stream_t s) { return devo_lie_log(3, X, a, n, dtype, s); }
int devo_se3_log_backward(const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s) { return devo_lie_log_backward(3, grad, X, dX, n, dtype, s); }
int devo_se3_inv(const void* X, void* Y, int64_t n, int dtype, devo_stream_t s) { return devo_lie_inv(3, X, Y, n, dtype, s); }
int devo_se3_inv_backward(const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s) { return devo_lie_inv_backward(3, grad, X, dX, n, dtype, s); }
int devo_se3_mul(const void* X, const void* Y, void* Z, int64_t n, int dtype, devo_stream_t s) { return devo_lie_mul(3, X, Y, Z, n, dtype, s); }
int devo_se3_mul_backward(const void* grad, const void* X, const void* Y, void* dX, void* dY, int64_t n, int dtype, devo_stream_t s) { return devo_lie_mul_backward(3, grad, X, Y, dX, dY, n, dtype, s); }
int devo_se3_adj(const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s) { return devo_lie_adj(3, X, a, b, n, dtype, s); }
int devo_se3_adj_backward(const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n, int dtype, devo_stream_t s) { return devo_lie_adj_backward(3, grad, X, a, dX, da, n, dtype, s); }
int devo_se3_adjT(const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s) { return devo_lie_adjT(3, X, a, b, n, dtype, s); }
int devo_se3_adjT_backward(const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n, int dtype, devo_stream_t s) { return devo_lie_adjT_backward(3, grad, X, a, dX, da, n, dtype, s); }
int devo_se3_act(const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s) { return devo_lie_act(3, X, p, q, n, dtype, s); }
int devo_se3_act_backward(const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n, int dtype, devo_stream_t s) { return devo_lie_act_backward(3, grad, X, p, dX, dp, n, dtype, s); }
int devo_se3_act4(const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s) { return devo_lie_act4(3, X, p, q, n, dtype, s); }
int devo_se3_act4_backward(const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n, int dtype, devo_stream_t s) { return devo_lie_act4_backward(3, grad, X, p, dX, dp, n, dtype, s); }
int devo_se3_as_matrix(const void* X, void* T44, int64_t n, int dtype, devo_stream_t s) { return devo_lie_as_matrix(3, X, T44, n, dtype, s); }
int devo_se3_jinv(const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s) { return devo_lie_jinv(3, X, a, b, n, dtype, s); }

}  // extern "C"
