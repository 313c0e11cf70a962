// Optimiser step (devo_amd/optim.py; include/devo_hip.h): gradient-norm clip + AdamW over a list of fp32 tensors that live wherever torch
// put them, what the reference's train.py:248-249 does with clip_grad_norm_ and torch.optim.AdamW.  The tensors are cut into chunks of
// DEVO_OPTIM_CHUNK elements; the chunk table (tensor, element offset, length) depends only on the sizes and is built once on the host
// (devo_optim_plan).  The moments live in two flat buffers, every tensor's slice on a 16-byte boundary.
//   k_optim_norm    sum of g^2 in fp64 (every fp32 g widened first): block b walks chunks b, b + grid, ... and writes ONE partial to
//                   partials[b].  No atomics: the partials and the order they are summed in depend on the sizes alone.
//   k_optim_update  every block sums the partials itself in one fixed order, forms norm and coef, and updates its chunks.  Gradients are read,
//                   never written.
//   k_optim_count   skip_nonfinite only: advances the applied / skipped counters after the update has read them.
// Parameter addresses and moment offsets sit in a device table written once.  The gradient addresses change every step and travel as KERNEL
// ARGUMENTS, DEVO_OPTIM_GROUP tensors per launch: a launch carries its own copy, so the host may enqueue step k + 1 before the device has run
// step k, and nothing is synchronised.  (More than DEVO_OPTIM_GROUP tensors: one norm and one update launch per group; the partials of all
// groups are summed by every update block.)
// The fp32 element arithmetic is torch's single-tensor AdamW, one rounding per operation: nothing below may be contracted into an FMA.
#include <cmath>
#include "common.h"

#pragma clang fp contract(off)

namespace {
using namespace devo;

constexpr int TB = 256;
constexpr int CH = DEVO_OPTIM_CHUNK;
constexpr int GROUP = DEVO_OPTIM_GROUP;
constexpr int MAX_BLOCKS = DEVO_OPTIM_MAX_PARTIALS;          // of ALL norm launches of a step together

struct GradPtrs { const float* g[GROUP]; };                   // 2 KB of kernel arguments
struct Hyper {
  double lr, beta1, beta2, bc1, bc2, max_norm;                // max_norm < 0: no clipping
  float decay, one_minus_beta1, beta2f, one_minus_beta2, eps;
  int skip_nonfinite;
};

// the sum of the block's 256 values in one fixed tree, in every thread
__device__ __forceinline__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = TB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// thread t adds partials t, t + 256, ... in that order, then the tree: the same value in every block of every launch of the step
__device__ __forceinline__ double sum_partials(const double* __restrict__ partials, int n, double* sh) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += TB) acc += partials[i];
  return block_sum(acc, sh);
}

__global__ __launch_bounds__(TB) void k_optim_norm(const int4* __restrict__ chunks, int64_t c0, int64_t c1, int t0, GradPtrs gp, double* __restrict__ partials) {
  __shared__ double sh[TB];
  double acc = 0.0;
  for (int64_t c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
    const int4 ch = chunks[c];                                 // (tensor, element offset, length, -)
    const float* g = gp.g[ch.x - t0];
    if (g == nullptr) continue;                                // no gradient this step: the tensor is skipped whole
    g += (uint32_t)ch.y;
    const int n4 = ch.z >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int i = threadIdx.x; i < n4; i += TB) {
      const float4 q = g4[i];
      const double x = (double)q.x, y = (double)q.y, z = (double)q.z, w = (double)q.w;
      acc += x * x;
      acc += y * y;
      acc += z * z;
      acc += w * w;
    }
    if ((int)threadIdx.x < (ch.z & 3)) {
      const double x = (double)g[4 * n4 + threadIdx.x];
      acc += x * x;
    }
  }
  const double total = block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__device__ __forceinline__ void adamw(float& p, float g, float& m, float& v, float coef, float decay, float omb1, float b2, float omb2, float neg_step, float bc2s, float eps) {
  g = g * coef;
  p = p * decay;
  m = m + (g - m) * omb1;
  v = v * b2 + (omb2 * g) * g;
  const float denom = sqrtf(v) / bc2s + eps;
  p = p + (neg_step * m) / denom;
}

__global__ __launch_bounds__(TB) void k_optim_update(const int4* __restrict__ chunks, int64_t c0, int64_t c1, int t0, GradPtrs gp, const int64_t* __restrict__ tensors,
                                                     float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, const double* __restrict__ partials, int n_partials,
                                                     Hyper h, const int64_t* __restrict__ counters, double* __restrict__ grad_norm) {
  __shared__ double sh[TB];
  const double norm = sqrt(sum_partials(partials, n_partials, sh));
  if (grad_norm != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *grad_norm = norm;     // (the first launch of the step only)
  double bc1 = h.bc1, bc2 = h.bc2;
  if (h.skip_nonfinite) {
    if (!isfinite(norm)) return;                               // nothing at all is written to p, m, v
    const double t = (double)(counters[0] + 1);               // the steps APPLIED so far, this one included
    bc1 = 1.0 - pow(h.beta1, t);
    bc2 = 1.0 - pow(h.beta2, t);
  }
  double cd = 1.0;
  if (h.max_norm >= 0.0) {
    cd = h.max_norm / (norm + 1e-6);
    cd = cd > 1.0 ? 1.0 : cd;                                 // (a NaN stays a NaN, as torch's clamp leaves it)
  }
  const float coef = (float)cd, neg_step = (float)(-(h.lr / bc1)), bc2s = (float)sqrt(bc2);
  for (int64_t c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
    const int4 ch = chunks[c];
    const float* g = gp.g[ch.x - t0];
    if (g == nullptr) continue;
    const int64_t off = (int64_t)(uint32_t)ch.y;
    g += off;
    float* p = reinterpret_cast<float*>(tensors[2 * ch.x]) + off;
    const int64_t mo = tensors[2 * ch.x + 1] + off;
    float *m = exp_avg + mo, *v = exp_avg_sq + mo;
    const int n4 = ch.z >> 2;
    for (int i = threadIdx.x; i < n4; i += TB) {
      const float4 G = reinterpret_cast<const float4*>(g)[i];
      float4 P = reinterpret_cast<float4*>(p)[i], M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
      adamw(P.x, G.x, M.x, V.x, coef, h.decay, h.one_minus_beta1, h.beta2f, h.one_minus_beta2, neg_step, bc2s, h.eps);
      adamw(P.y, G.y, M.y, V.y, coef, h.decay, h.one_minus_beta1, h.beta2f, h.one_minus_beta2, neg_step, bc2s, h.eps);
      adamw(P.z, G.z, M.z, V.z, coef, h.decay, h.one_minus_beta1, h.beta2f, h.one_minus_beta2, neg_step, bc2s, h.eps);
      adamw(P.w, G.w, M.w, V.w, coef, h.decay, h.one_minus_beta1, h.beta2f, h.one_minus_beta2, neg_step, bc2s, h.eps);
      reinterpret_cast<float4*>(p)[i] = P;
      reinterpret_cast<float4*>(m)[i] = M;
      reinterpret_cast<float4*>(v)[i] = V;
    }
    if ((int)threadIdx.x < (ch.z & 3)) {
      const int i = 4 * n4 + threadIdx.x;
      float P = p[i], M = m[i], V = v[i];
      adamw(P, g[i], M, V, coef, h.decay, h.one_minus_beta1, h.beta2f, h.one_minus_beta2, neg_step, bc2s, h.eps);
      p[i] = P;
      m[i] = M;
      v[i] = V;
    }
  }
}

__global__ __launch_bounds__(TB) void k_optim_count(const double* __restrict__ partials, int n_partials, int64_t* __restrict__ counters) {
  __shared__ double sh[TB];
  const double norm = sqrt(sum_partials(partials, n_partials, sh));
  if (threadIdx.x == 0) counters[isfinite(norm) ? 0 : 1] += 1;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline int64_t chunks_of(int64_t numel) { return (numel + CH - 1) / CH; }
inline int64_t padded(int64_t numel) { return (numel + 3) / 4 * 4; }

// 1 .. DEVO_OPTIM_MAX_TENSORS tensors of 1 .. 2^31 - 1 elements
int sizes_ok(const int64_t* numel, int n_tensors, const char* what) {
  DEVO_REQUIRE(numel != nullptr, "%s: numel is null", what);
  DEVO_REQUIRE(n_tensors >= 1 && n_tensors <= DEVO_OPTIM_MAX_TENSORS, "%s: %d tensors (1 .. %d)", what, n_tensors, DEVO_OPTIM_MAX_TENSORS);
  for (int t = 0; t < n_tensors; ++t)
    DEVO_REQUIRE(numel[t] >= 1 && numel[t] <= (int64_t)INT32_MAX, "%s: tensor %d has %lld elements (1 .. 2^31 - 1)", what, t, (long long)numel[t]);
  return DEVO_OK;
}

}  // namespace

extern "C" {

int64_t devo_optim_chunks(const int64_t* numel, int n_tensors) {
  if (sizes_ok(numel, n_tensors, "devo_optim_chunks") != DEVO_OK) return 0;
  int64_t n = 0;
  for (int t = 0; t < n_tensors; ++t) n += chunks_of(numel[t]);
  return n;
}

int64_t devo_optim_moment_elems(const int64_t* numel, int n_tensors) {
  if (sizes_ok(numel, n_tensors, "devo_optim_moment_elems") != DEVO_OK) return 0;
  int64_t n = 0;
  for (int t = 0; t < n_tensors; ++t) n += padded(numel[t]);
  return n;
}

size_t devo_optim_workspace_bytes(void) { return (size_t)(DEVO_OPTIM_MAX_PARTIALS + DEVO_OPTIM_MAX_TENSORS / DEVO_OPTIM_GROUP) * sizeof(double); }

int devo_optim_plan(const int64_t* numel, int n_tensors, int32_t* chunk_table, int64_t* moment_offsets) {
  if (int rc = sizes_ok(numel, n_tensors, "devo_optim_plan")) return rc;
  DEVO_REQUIRE(chunk_table != nullptr && moment_offsets != nullptr, "devo_optim_plan: null output");
  int64_t c = 0, mo = 0;
  for (int t = 0; t < n_tensors; ++t) {
    moment_offsets[t] = mo;
    mo += padded(numel[t]);
    for (int64_t off = 0; off < numel[t]; off += CH, ++c) {
      const int64_t len = numel[t] - off < CH ? numel[t] - off : CH;
      chunk_table[4 * c + 0] = t;
      chunk_table[4 * c + 1] = (int32_t)(uint32_t)off;
      chunk_table[4 * c + 2] = (int32_t)len;
      chunk_table[4 * c + 3] = 0;
    }
  }
  return DEVO_OK;
}

int devo_optim_step(const int32_t* chunk_table, int64_t n_chunks, const int64_t* tensor_table, const void* const* grads, const int64_t* numel, int n_tensors,
                    float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double bc1, double bc2,
                    int skip_nonfinite, int64_t* counters, double* grad_norm, void* workspace, size_t workspace_bytes, devo_stream_t stream) {
  if (int rc = sizes_ok(numel, n_tensors, "devo_optim_step")) return rc;
  DEVO_REQUIRE(chunk_table != nullptr && tensor_table != nullptr && grads != nullptr && exp_avg != nullptr && exp_avg_sq != nullptr && grad_norm != nullptr,
               "devo_optim_step: null argument");
  DEVO_REQUIRE(aligned16(chunk_table) && aligned16(tensor_table) && aligned16(exp_avg) && aligned16(exp_avg_sq) && ((uintptr_t)grad_norm & 7u) == 0 && exp_avg != exp_avg_sq,
               "devo_optim_step: the tables and the moment buffers must be 16-byte aligned (and the two moment buffers distinct)");
  DEVO_REQUIRE(n_chunks == devo_optim_chunks(numel, n_tensors), "devo_optim_step: %lld chunks, the sizes give %lld", (long long)n_chunks,
               (long long)devo_optim_chunks(numel, n_tensors));
  DEVO_REQUIRE(std::isfinite(lr) && lr >= 0.0, "devo_optim_step: lr %g", lr);
  DEVO_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "devo_optim_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
  DEVO_REQUIRE(std::isfinite(eps) && eps >= 0.0, "devo_optim_step: eps %g", eps);
  DEVO_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.0, "devo_optim_step: weight_decay %g", weight_decay);
  DEVO_REQUIRE(!std::isnan(max_norm), "devo_optim_step: max_norm is NaN (negative: no clipping)");
  DEVO_REQUIRE(skip_nonfinite == 0 || skip_nonfinite == 1, "devo_optim_step: skip_nonfinite %d", skip_nonfinite);
  if (skip_nonfinite)
    DEVO_REQUIRE(counters != nullptr && ((uintptr_t)counters & 7u) == 0, "devo_optim_step: skip_nonfinite needs the two int64 counters");
  else
    DEVO_REQUIRE(bc1 > 0.0 && bc1 <= 1.0 && bc2 > 0.0 && bc2 <= 1.0, "devo_optim_step: bias corrections (%g, %g) outside (0, 1]", bc1, bc2);
  DEVO_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7u) == 0 && workspace_bytes >= devo_optim_workspace_bytes(),
               "devo_optim_step: workspace of %zu bytes, %zu needed (8-byte aligned)", workspace_bytes, devo_optim_workspace_bytes());
  for (int t = 0; t < n_tensors; ++t) DEVO_REQUIRE(aligned16(grads[t]), "devo_optim_step: the gradient of tensor %d is not 16-byte aligned", t);

  Hyper h;
  h.lr = lr, h.beta1 = beta1, h.beta2 = beta2, h.bc1 = skip_nonfinite ? 1.0 : bc1, h.bc2 = skip_nonfinite ? 1.0 : bc2, h.max_norm = max_norm;
  h.decay = (float)(1.0 - lr * weight_decay), h.one_minus_beta1 = (float)(1.0 - beta1), h.beta2f = (float)beta2, h.one_minus_beta2 = (float)(1.0 - beta2), h.eps = (float)eps;
  h.skip_nonfinite = skip_nonfinite;
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)workspace;
  const int4* chunks = (const int4*)chunk_table;
  const int n_groups = (n_tensors + GROUP - 1) / GROUP;
  // per group: its chunk range and its share of the norm blocks (at least one, never more than its chunks)
  int64_t c_begin[DEVO_OPTIM_MAX_TENSORS / DEVO_OPTIM_GROUP + 1];
  int blocks[DEVO_OPTIM_MAX_TENSORS / DEVO_OPTIM_GROUP], n_partials = 0;
  c_begin[0] = 0;
  for (int gi = 0; gi < n_groups; ++gi) {
    int64_t c = 0;
    for (int t = gi * GROUP; t < n_tensors && t < (gi + 1) * GROUP; ++t) c += chunks_of(numel[t]);
    c_begin[gi + 1] = c_begin[gi] + c;
    int64_t b = n_chunks <= MAX_BLOCKS ? c : c * MAX_BLOCKS / n_chunks;
    blocks[gi] = (int)(b < 1 ? 1 : b);
    n_partials += blocks[gi];
  }
  GradPtrs gp;
  for (int pass = 0; pass < 2; ++pass) {
    int base = 0;
    for (int gi = 0; gi < n_groups; ++gi) {
      const int t0 = gi * GROUP;
      for (int j = 0; j < GROUP; ++j) gp.g[j] = t0 + j < n_tensors ? (const float*)grads[t0 + j] : nullptr;
      if (pass == 0)
        hipLaunchKernelGGL(k_optim_norm, dim3(blocks[gi]), dim3(TB), 0, s, chunks, c_begin[gi], c_begin[gi + 1], t0, gp, partials + base);
      else
        hipLaunchKernelGGL(k_optim_update, dim3(blocks_for(c_begin[gi + 1] - c_begin[gi], 1, MAX_BLOCKS)), dim3(TB), 0, s, chunks, c_begin[gi], c_begin[gi + 1], t0, gp,
                           tensor_table, exp_avg, exp_avg_sq, (const double*)partials, n_partials, h, (const int64_t*)counters, gi == 0 ? grad_norm : (double*)nullptr);
      base += blocks[gi];
    }
  }
  if (skip_nonfinite) hipLaunchKernelGGL(k_optim_count, dim3(1), dim3(TB), 0, s, (const double*)partials, n_partials, counters);
  return check_launch("devo_optim_step");
}

}  // extern "C"
