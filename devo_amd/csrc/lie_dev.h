// SO(3), RxSO(3), SE(3) and Sim(3) device maths for gfx950 on top of se3_dev.h — header-only, no Eigen.
// Semantics follow the reference's group classes (devo/lietorch/include/so3.h:27-220, rxso3.h:32-315, se3.h:36-217, sim3.h:33-209);
// the numerics of the RxSO3 / Sim3 Jacobians do not: see w_coef and sim3_jl_rows below.
//
//   group  id  element (N)            tangent (K)
//   SO3    1   q_xyzw            (4)  phi              (3)
//   RxSO3  2   q_xyzw, s         (5)  phi, sigma       (4)
//   SE3    3   t, q_xyzw         (7)  tau, phi         (6)
//   Sim3   4   t, q_xyzw, s      (8)  tau, phi, sigma  (7)
//
// One generic implementation: an element is (t, q, s) with t = 0 / s = 1 where the group has none, a tangent (tau, phi, sigma) with
// tau = 0 / sigma = 0 likewise, and every formula below is Sim3's, which restricts to the three others.  SE3 is the exception where that
// restriction would not be se3_dev.h's arithmetic: see "SE3" below.
#pragma once
#include "se3_dev.h"

namespace devo {

template <typename T> struct LieConsts;
// w_series_max: below it the W coefficients come from their series in theta^2 (w_coef), above it from the closed forms.
// series_tol: the Sim3 Jacobian recursion (sim3_jl_rows) stops once every entry of a term is below it (jl_max_terms caps it), and the
// series of g_12 in w_coef once a term is below it relative to the sum.
template <> struct LieConsts<float>  { static constexpr float  w_series_max = 1.0f; static constexpr float  series_tol = 1e-9f; static constexpr int jl_max_terms = 64; };
template <> struct LieConsts<double> { static constexpr double w_series_max = 0.3;  static constexpr double series_tol = 1e-18; static constexpr int jl_max_terms = 64; };

template <typename T> DEVO_HD T t_exp(T x);
template <> DEVO_HD float  t_exp<float>(float x)   { return expf(x); }
template <> DEVO_HD double t_exp<double>(double x) { return exp(x); }
template <typename T> DEVO_HD T t_expm1(T x);
template <> DEVO_HD float  t_expm1<float>(float x)   { return expm1f(x); }
template <> DEVO_HD double t_expm1<double>(double x) { return expm1(x); }
template <typename T> DEVO_HD T t_log(T x);
template <> DEVO_HD float  t_log<float>(float x)   { return logf(x); }
template <> DEVO_HD double t_log<double>(double x) { return log(x); }
template <typename T> DEVO_HD T t_max(T a, T b) { return a > b ? a : b; }
template <typename T> DEVO_HD T vmaxabs(V3<T> v) { return t_max(t_abs(v.x), t_max(t_abs(v.y), t_abs(v.z))); }

template <int G> struct LieG {
  static_assert(G >= 1 && G <= 4, "group id");
  static constexpr bool HAS_T = (G == 3 || G == 4), HAS_S = (G == 2 || G == 4);
  static constexpr int K = 3 + (HAS_T ? 3 : 0) + (HAS_S ? 1 : 0), N = K + 1;
  static constexpr int QO = HAS_T ? 3 : 0;           // offset of q in an element and of phi in a tangent; s at QO + 4, sigma at QO + 3
};

template <typename T> struct Tan { V3<T> tau, phi; T sigma; };
template <typename T> struct Elem { V3<T> t; Q4<T> q; T s; };

template <int G, typename T> DEVO_HD Tan<T> tan_load(const T* a) {
  constexpr int o = LieG<G>::QO;
  Tan<T> v;
  v.tau = LieG<G>::HAS_T ? V3<T>{a[0], a[1], a[2]} : V3<T>{T(0), T(0), T(0)};
  v.phi = {a[o], a[o + 1], a[o + 2]};
  v.sigma = LieG<G>::HAS_S ? a[o + 3] : T(0);
  return v;
}
template <int G, typename T> DEVO_HD void tan_store(const Tan<T>& v, T* a) {
  constexpr int o = LieG<G>::QO;
  if (LieG<G>::HAS_T) { a[0] = v.tau.x; a[1] = v.tau.y; a[2] = v.tau.z; }
  a[o] = v.phi.x; a[o + 1] = v.phi.y; a[o + 2] = v.phi.z;
  if (LieG<G>::HAS_S) a[o + 3] = v.sigma;
}
// the gradient of a group element: a tangent in the first K of the N slots, the last one zero (what the reference's kernels leave in
// their zero-initialised outputs, lietorch_gpu.cu:68,95,122)
template <int G, typename T> DEVO_HD void grad_store(const Tan<T>& v, T* p) {
  tan_store<G, T>(v, p);
  p[LieG<G>::K] = T(0);
}
template <int G, typename T> DEVO_HD Elem<T> elem_load(const T* p) {                    // so3.h:31-37, rxso3.h:37-39, se3.h:34, sim3.h:40-41
  constexpr int o = LieG<G>::QO;
  Elem<T> X;
  X.t = LieG<G>::HAS_T ? V3<T>{p[0], p[1], p[2]} : V3<T>{T(0), T(0), T(0)};
  X.q = qnormalize(Q4<T>{p[o], p[o + 1], p[o + 2], p[o + 3]});
  X.s = LieG<G>::HAS_S ? p[o + 4] : T(1);
  return X;
}
template <int G, typename T> DEVO_HD void elem_store(const Elem<T>& X, T* p) {
  constexpr int o = LieG<G>::QO;
  if (LieG<G>::HAS_T) { p[0] = X.t.x; p[1] = X.t.y; p[2] = X.t.z; }
  p[o] = X.q.x; p[o + 1] = X.q.y; p[o + 2] = X.q.z; p[o + 3] = X.q.w;
  if (LieG<G>::HAS_S) p[o + 4] = X.s;
}

// ---- SE3 --------------------------------------------------------------------------------------
// SE3 keeps the arithmetic of se3_dev.h, which ba.hip, loss.hip, frames.hip, graph.hip and transform.hip compute with.  With s = 1 and no
// sigma most generic formulas are se3_dev.h's to the bit (load / store, inv, mul, act, the 4x4 matrix: x * 1 and x + 0 * t fold away).
// Not so where se3_dev.h rotates with the matrix qmat(q) (Adj, Adj^T, the point gradient), where x + 0 * y would have to equal x
// (row_times_ad: it does not for a non-finite y), and in exp / log and the Jacobians, whose Q block se3_dev.h has in closed form (se3_calcQ)
// where Sim3 sums a series.  elem_adj, elem_adjT, row_times_sR, lie_exp and lie_log start with an `if constexpr (G == 3)` that calls se3_dev.h
// through these converters.  row_times_ad and the three Jacobian products refuse G = 3 (SE3_IN_KERNEL): the kernels that need them (adj_bwd,
// adjT_bwd, exp_bwd, log_bwd, jinv in lie.hip) call se3_dev.h on the operands in memory, in the order the SE3-only kernels had.  Through the
// converters the compiler pairs multiplies and adds into fmas differently (the choice follows the order of the loads), which moves last bits.
#define SE3_IN_KERNEL(G) static_assert(G != 3, "SE3: lie.hip's kernel calls se3_dev.h directly (see \"SE3\" in lie_dev.h)")
template <typename T> struct Tan6 { T v[6]; };
template <typename T> DEVO_HD Tan6<T> tan6(const Tan<T>& a) { Tan6<T> r; tan_store<3, T>(a, r.v); return r; }
template <typename T> DEVO_HD Tan<T> tan_of(const Tan6<T>& r) { return tan_load<3, T>(r.v); }
template <typename T> DEVO_HD SE3<T> se3_of(const Elem<T>& X) { SE3<T> Y; Y.t = X.t; Y.q = X.q; return Y; }
template <typename T> DEVO_HD Elem<T> elem_of(const SE3<T>& X) { return Elem<T>{X.t, X.q, T(1)}; }

// ---- group structure --------------------------------------------------------------------------
template <typename T> DEVO_HD Elem<T> elem_inv(const Elem<T>& X) {                      // so3.h:43, rxso3.h:46-48, sim3.h:43-45
  Elem<T> Y;
  Y.q = qnormalize(qconj(X.q));
  Y.s = T(1) / X.s;
  Y.t = -(Y.s * qrot(Y.q, X.t));
  return Y;
}
template <typename T> DEVO_HD Elem<T> elem_mul(const Elem<T>& X, const Elem<T>& Y) {   // so3.h:51, rxso3.h:55-57, sim3.h:52-54
  Elem<T> Z;
  Z.q = qnormalize(qmul(X.q, Y.q));
  Z.s = X.s * Y.s;
  Z.t = X.t + X.s * qrot(X.q, Y.t);
  return Z;
}
template <typename T> DEVO_HD V3<T> elem_act(const Elem<T>& X, V3<T> p) { return X.s * qrot(X.q, p) + X.t; }      // rxso3.h:59-63, sim3.h:56-58
// Adj = [[sR, [t]x R, -t], [0, R, 0], [0, 0, 1]]   (sim3.h:89-101; rxso3.h:70-74 and so3.h:67 are its lower-right blocks)
template <int G, typename T> DEVO_HD Tan<T> elem_adj(const Elem<T>& X, const Tan<T>& a) {
  if constexpr (G == 3) { Tan6<T> b; se3_of(X).adj(tan6(a).v, b.v); return tan_of(b); }
  Tan<T> b;
  b.phi = qrot(X.q, a.phi);
  b.tau = X.s * qrot(X.q, a.tau) + cross(X.t, b.phi) - a.sigma * X.t;
  b.sigma = a.sigma;
  return b;
}
template <int G, typename T> DEVO_HD Tan<T> elem_adjT(const Elem<T>& X, const Tan<T>& a) {   // Adj^T a == (a^T Adj)^T
  if constexpr (G == 3) { Tan6<T> b; se3_of(X).adjT(tan6(a).v, b.v); return tan_of(b); }
  const Q4<T> qi = qconj(X.q);
  Tan<T> b;
  b.tau = X.s * qrot(qi, a.tau);
  b.phi = qrot(qi, cross(a.tau, X.t) + a.phi);                                          // ([t]x R)^T a0 = R^T (a0 x t)
  b.sigma = a.sigma - dot(X.t, a.tau);
  return b;
}
// a(1xK) * ad(b),  ad(b) = [[Phi + sigma I, Tau, -tau], [0, Phi, 0], [0, 0, 0]]  (sim3.h:126-142);  row * hat(v) = row x v
template <int G, typename T> DEVO_HD Tan<T> row_times_ad(const Tan<T>& a, const Tan<T>& b) {
  SE3_IN_KERNEL(G);
  Tan<T> o;
  o.tau = cross(a.tau, b.phi) + b.sigma * a.tau;
  o.phi = cross(a.tau, b.tau) + cross(a.phi, b.phi);
  o.sigma = -dot(a.tau, b.tau);
  return o;
}
// g(1x3) * (sR): the point gradient of act / act4
template <int G, typename T> DEVO_HD V3<T> row_times_sR(V3<T> g, const Elem<T>& X) {
  if constexpr (G == 3) return mulTv(qmat(X.q), g);
  return X.s * qrot(qconj(X.q), g);
}
template <typename T> DEVO_HD Tan<T> tan_neg(const Tan<T>& a) { return Tan<T>{-a.tau, -a.phi, -a.sigma}; }

// ---- W(phi, sigma) = sum_k (Phi + sigma I)^k / (k+1)! = C I + A Phi + B Phi^2 -------------------
// rxso3.h:190-233 takes A, B, C from closed forms with four corner cases switched at 1e-6.  Those forms subtract nearly equal numbers
// whenever theta is small (B = (C - Re f) / theta^2 keeps eps / theta^2 for any sigma) and when theta and sigma are small together.
// Here: with f(z) = (e^z - 1)/z and g_n(sigma) = int_0^1 s^n e^(s sigma) ds = f^(n)(sigma),
//     C = g_0,   A = Im f(sigma + i theta) / theta = sum_k (-theta^2)^k g_(2k+1) / (2k+1)!,
//                B = (C - Re f(sigma + i theta)) / theta^2 = sum_k (-theta^2)^k g_(2k+2) / (2k+2)!.
// Below w_series_max, for every sigma: six terms of each (first dropped term theta^12 / 14!: 6e-18 at 0.3, 1e-11 at 1.0), g_12 from its
// own series sum_j sigma^j / (j! (13 + j)) and g_11 .. g_0 by the downward recurrence g_(n-1) = (e^sigma - sigma g_n) / n, which damps
// errors.  Above it the closed forms, with e^sigma cos(theta) - 1 built from expm1 and sin^2(theta/2) so that sigma -> 0 costs nothing;
// what is left loses at most about 6 / theta^2 ulps of C.  One switch in theta covers the four corners.
template <typename T> struct WCoef { T A, B, C; };
template <typename T> DEVO_HD WCoef<T> w_coef(T theta2, T theta, T sigma) {
  WCoef<T> w;
  const T es = t_exp<T>(sigma);
  if (theta < LieConsts<T>::w_series_max) {
    T term = T(1), g = T(1.0 / 13.0);                                                   // g_12
    for (int j = 1; j < 48; j++) {
      term *= sigma / T(j);
      const T add = term / T(13 + j);
      g += add;
      if (t_abs(add) <= LieConsts<T>::series_tol * t_abs(g)) break;
    }
    constexpr double inv_factorial[13] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                                          1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0};
    const T x = -theta2;
    T A = T(0), B = T(0);
#pragma unroll
    for (int n = 12; n >= 1; n--) {
      const T c = g * T(inv_factorial[n]);
      if (n & 1) A = A * x + c; else B = B * x + c;
      g = (es - sigma * g) / T(n);
    }
    w.A = A; w.B = B; w.C = g;
  } else {
    const T em = t_expm1<T>(sigma), sn = t_sin<T>(theta), cs = t_cos<T>(theta), sh = t_sin<T>(T(0.5) * theta);
    const T a = es * sn, bm1 = em * cs - T(2) * sh * sh, c = theta2 + sigma * sigma;
    w.C = sigma == T(0) ? T(1) : em / sigma;
    w.A = (a * sigma - bm1 * theta) / (theta * c);
    w.B = (w.C - (bm1 * sigma + a * theta) / c) / theta2;
  }
  return w;
}
// The inverse lies in the same algebra: W^-1 = c I + a Phi + b Phi^2.  On the rotation plane W acts as p + i A theta with p = C - B theta^2,
// so with D = p^2 + A^2 theta^2:  c = 1/C,  a = -A / D,  b = (A^2 - B p) / (C D)  — no division by theta, nothing that cancels (D = |f|^2
// vanishes only at theta = 2 pi, sigma = 0).  Replaces both rxso3.h:235-284 and the numerical W.inverse() of sim3.h:151.
template <typename T> DEVO_HD WCoef<T> w_inv_coef(const WCoef<T>& w, T theta2) {
  const T p = w.C - w.B * theta2, D = p * p + w.A * w.A * theta2;
  WCoef<T> r;
  r.C = T(1) / w.C;
  r.A = -w.A / D;
  r.B = (w.A * w.A - w.B * p) / (w.C * D);
  return r;
}
template <typename T> DEVO_HD V3<T> abc_apply(const WCoef<T>& w, V3<T> phi, V3<T> v) {  // (C I + A Phi + B Phi^2) v
  const V3<T> pv = cross(phi, v);
  return w.C * v + w.A * pv + w.B * cross(phi, pv);
}
template <typename T> DEVO_HD V3<T> abc_applyT(const WCoef<T>& w, V3<T> phi, V3<T> v) { // Phi^T = -Phi
  const V3<T> pv = cross(phi, v);
  return w.C * v - w.A * pv + w.B * cross(phi, pv);
}
// SO3's left Jacobian and its inverse in the same form, coefficients from se3_dev.h (series-backed already)
template <typename T> DEVO_HD WCoef<T> so3_jl_coef(T theta2, T theta) { return {jc_one_minus_cos<T>(theta2, theta), jc_t_minus_sin<T>(theta2, theta), T(1)}; }
template <typename T> DEVO_HD WCoef<T> so3_jl_inv_coef(T theta2, T theta) { return {T(-0.5), jc_inv<T>(theta2, theta), T(1)}; }

// ---- exp / log --------------------------------------------------------------------------------
template <int G, typename T> DEVO_HD Elem<T> lie_exp(const Tan<T>& a) {                 // so3.h:153-168, rxso3.h:168-188, se3.h:134-142, sim3.h:156-165
  if constexpr (G == 3) return elem_of(se3_exp<T>(tan6(a).v));
  Elem<T> X;
  X.q = so3_exp(a.phi);
  X.s = LieG<G>::HAS_S ? t_exp<T>(a.sigma) : T(1);
  X.t = {T(0), T(0), T(0)};
  if (LieG<G>::HAS_T) {
    const T theta2 = dot(a.phi, a.phi), theta = t_sqrt<T>(theta2);
    X.t = abc_apply(LieG<G>::HAS_S ? w_coef<T>(theta2, theta, a.sigma) : so3_jl_coef<T>(theta2, theta), a.phi, a.tau);
  }
  return X;
}
template <int G, typename T> DEVO_HD Tan<T> lie_log(const Elem<T>& X) {                 // so3.h:115-151, rxso3.h:131-166, se3.h:124-132, sim3.h:145-154
  if constexpr (G == 3) { Tan6<T> a; se3_log<T>(se3_of(X), a.v); return tan_of(a); }
  Tan<T> a;
  a.phi = so3_log(X.q);
  a.sigma = LieG<G>::HAS_S ? t_log<T>(X.s) : T(0);
  a.tau = {T(0), T(0), T(0)};
  if (LieG<G>::HAS_T) {
    const T theta2 = dot(a.phi, a.phi), theta = t_sqrt<T>(theta2);
    a.tau = abc_apply(LieG<G>::HAS_S ? w_inv_coef<T>(w_coef<T>(theta2, theta, a.sigma), theta2) : so3_jl_inv_coef<T>(theta2, theta), a.phi, X.t);
  }
  return a;
}

// ---- left Jacobians ---------------------------------------------------------------------------
// J_l(a) = sum_k ad(a)^k / (k+1)!.  ad is block upper-triangular, so
//     J_l = [[W(phi, sigma), Q, u], [0, J_so3(phi), 0], [0, 0, 1]]
// (SE3: sigma = 0, no last row / column; RxSO3 and SO3: the lower-right blocks, where rxso3.h:286-300 is already exact).
// sim3.h:167-191 truncates the series at ad^4 (a stray ';' drops ad^5) and uses a truncated Bernoulli polynomial for the inverse: wrong by
// 1.4 / 0.17 for tangents of unit size.  Here W and J_so3 come from their coefficients, and only Q (3x3) and u (3) from the recursion on
// the top three rows:  [P, Q, u]_(k+1) = [P M, P Tau + Q Phi, -P tau] / (k + 2),  M = Phi + sigma I,  [P, Q, u]_0 = [I, 0, 0],
// summed until a whole term is below series_tol (about 35 terms at theta = pi, |sigma| = 1, a handful for small arguments).  tau enters
// linearly, so the terms stay of the size of the result: nothing cancels.  Rows are kept as vectors: row * hat(v) = row x v.
template <typename T> struct JlRows { V3<T> Q[3]; V3<T> u; };
template <typename T> DEVO_HD JlRows<T> sim3_jl_rows(const Tan<T>& a) {
  V3<T> P[3] = {{T(1), T(0), T(0)}, {T(0), T(1), T(0)}, {T(0), T(0), T(1)}}, Q[3] = {{T(0), T(0), T(0)}, {T(0), T(0), T(0)}, {T(0), T(0), T(0)}};
  JlRows<T> J;
  T ut[3] = {T(0), T(0), T(0)}, us[3] = {T(0), T(0), T(0)};
#pragma unroll
  for (int r = 0; r < 3; r++) J.Q[r] = {T(0), T(0), T(0)};
  for (int k = 0; k < LieConsts<T>::jl_max_terms; k++) {
    const T f = T(1) / T(k + 2);
    T m = T(0);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const V3<T> Pn = f * (cross(P[r], a.phi) + a.sigma * P[r]);
      Q[r] = f * (cross(P[r], a.tau) + cross(Q[r], a.phi));
      ut[r] = -f * dot(P[r], a.tau);
      P[r] = Pn;
      J.Q[r] = J.Q[r] + Q[r];
      us[r] += ut[r];
      m = t_max(m, t_max(t_max(vmaxabs(P[r]), vmaxabs(Q[r])), t_abs(ut[r])));
    }
    if (!(m > LieConsts<T>::series_tol)) break;                                              // (a NaN ends the loop too)
  }
  J.u = {us[0], us[1], us[2]};
  return J;
}
template <typename T> DEVO_HD V3<T> rowsT_times(const V3<T>* Q, V3<T> g) { return g.x * Q[0] + g.y * Q[1] + g.z * Q[2]; }      // Q^T g
template <typename T> DEVO_HD V3<T> rows_times(const V3<T>* Q, V3<T> v) { return {dot(Q[0], v), dot(Q[1], v), dot(Q[2], v)}; }  // Q v

// g(1xK) * J_l(a): the adjoint of Exp (lietorch_gpu.cu:32-44)
template <int G, typename T> DEVO_HD Tan<T> row_times_jl(const Tan<T>& g, const Tan<T>& a) {
  SE3_IN_KERNEL(G);
  const T theta2 = dot(a.phi, a.phi), theta = t_sqrt<T>(theta2);
  Tan<T> o;
  o.phi = abc_applyT(so3_jl_coef<T>(theta2, theta), a.phi, g.phi);
  o.sigma = g.sigma;
  o.tau = {T(0), T(0), T(0)};
  if (LieG<G>::HAS_T) {
    const JlRows<T> J = sim3_jl_rows(a);
    o.tau = abc_applyT(w_coef<T>(theta2, theta, a.sigma), a.phi, g.tau);
    o.phi = o.phi + rowsT_times(J.Q, g.tau);
    o.sigma += dot(J.u, g.tau);
  }
  return o;
}
// g(1xK) * J_l(a)^-1 by block back-substitution: the adjoint of Log (lietorch_gpu.cu:58-70)
template <int G, typename T> DEVO_HD Tan<T> row_times_jl_inv(const Tan<T>& g, const Tan<T>& a) {
  SE3_IN_KERNEL(G);
  const T theta2 = dot(a.phi, a.phi), theta = t_sqrt<T>(theta2);
  const WCoef<T> ji = so3_jl_inv_coef<T>(theta2, theta);
  Tan<T> o;
  o.tau = {T(0), T(0), T(0)};
  o.sigma = g.sigma;
  V3<T> g1 = g.phi;
  if (LieG<G>::HAS_T) {
    const JlRows<T> J = sim3_jl_rows(a);
    o.tau = abc_applyT(w_inv_coef<T>(w_coef<T>(theta2, theta, a.sigma), theta2), a.phi, g.tau);
    g1 = g1 - rowsT_times(J.Q, o.tau);
    o.sigma -= dot(J.u, o.tau);
  }
  o.phi = abc_applyT(ji, a.phi, g1);
  return o;
}
// J_l(a)^-1 v: the forward op Jinv (lietorch_gpu.cu:283-294), the same inverse
template <int G, typename T> DEVO_HD Tan<T> jl_inv_times(const Tan<T>& a, const Tan<T>& v) {
  SE3_IN_KERNEL(G);
  const T theta2 = dot(a.phi, a.phi), theta = t_sqrt<T>(theta2);
  Tan<T> o;
  o.phi = abc_apply(so3_jl_inv_coef<T>(theta2, theta), a.phi, v.phi);
  o.sigma = v.sigma;
  o.tau = {T(0), T(0), T(0)};
  if (LieG<G>::HAS_T) {
    const JlRows<T> J = sim3_jl_rows(a);
    const V3<T> rhs = v.tau - rows_times(J.Q, o.phi) - v.sigma * J.u;
    o.tau = abc_apply(w_inv_coef<T>(w_coef<T>(theta2, theta, a.sigma), theta2), a.phi, rhs);
  }
  return o;
}

// ---- matrices ---------------------------------------------------------------------------------
template <typename T> DEVO_HD void elem_matrix4(const Elem<T>& X, T* m) {               // row-major [[sR, t], [0, 1]]  (sim3.h:72-77, rxso3.h:80-85, so3.h:75-79)
  const M3<T> R = qmat(X.q);
  const T tv[3] = {X.t.x, X.t.y, X.t.z};
#pragma unroll
  for (int r = 0; r < 3; r++) { m[r * 4] = X.s * R.m[r][0]; m[r * 4 + 1] = X.s * R.m[r][1]; m[r * 4 + 2] = X.s * R.m[r][2]; m[r * 4 + 3] = tv[r]; }
  m[12] = T(0); m[13] = T(0); m[14] = T(0); m[15] = T(1);
}
// d(embedded coordinates) / d(left perturbation), row-major N x N with the last column zero (so3.h:81-91, rxso3.h:87-102, se3.h:114-122,
// sim3.h:79-87): what ToVec / FromVec differentiate through
template <int G, typename T> DEVO_HD void elem_projector(const Elem<T>& X, T* P) {
  constexpr int N = LieG<G>::N, o = LieG<G>::QO;
#pragma unroll
  for (int k = 0; k < N * N; k++) P[k] = T(0);
  if (LieG<G>::HAS_T) {
    const M3<T> H = hat(-X.t);
    const T tv[3] = {X.t.x, X.t.y, X.t.z};
#pragma unroll
    for (int r = 0; r < 3; r++) {
      P[r * N + r] = T(1);
#pragma unroll
      for (int c = 0; c < 3; c++) P[r * N + 3 + c] = H.m[r][c];
      if (LieG<G>::HAS_S) P[r * N + 6] = tv[r];
    }
  }
  const M3<T> Hq = hat(V3<T>{-X.q.x, -X.q.y, -X.q.z});
  const T qv[3] = {X.q.x, X.q.y, X.q.z};
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) P[(o + r) * N + o + c] = T(0.5) * ((r == c ? X.q.w : T(0)) + Hq.m[r][c]);
    P[(o + 3) * N + o + r] = T(-0.5) * qv[r];
  }
  if (LieG<G>::HAS_S) P[(o + 4) * N + o + 3] = X.s;
}

}  // namespace devo
