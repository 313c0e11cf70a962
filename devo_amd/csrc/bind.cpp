// Compiled binding of libdevo_hip.so: the reference's three pybind11 extension modules — cuda_corr (devo/altcorr/correlation.cpp:57-63),
// cuda_ba (devo/fastba/ba.cpp:152-157), lietorch_backends (devo/lietorch/src/lietorch.cpp:286-316) — with the reference's function names,
// positional signatures and torch::Tensor arguments, as sub-modules of devo_amd._C, plus the same entry points as torch.ops.devo_hip.*.
// Every function allocates its outputs with ATen, takes c10::hip::getCurrentHIPStream() and calls the C ABI of include/devo_hip.h: no
// kernels here, no torch types below this file.  Errors surface as c10::Error -> Python RuntimeError, like the reference's TORCH_CHECK.
// devo_amd/backends/*.py (ctypes) stay as the no-compile form of this BINDING; neither has a CPU path.
//
// Host-side state kept here (what the reference's modules do not need because they read NCHW / fp32 directly):
//   * per tensor VERSION (storage address, version counter, sizes, strides, dtype; the cache keeps the source alive): the channel-blocked
//     (fp16) or split-blocked (fp32) copy of a pyramid level and the patch operand of the dense-product lookup kernel — DEVO rewrites both
//     once per frame, not per update iteration;
//   * the BA workspace of the last problem size per device.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <cstdlib>
#include <algorithm>
#include <list>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>
#include "../../include/devo_hip.h"

namespace {

using at::Tensor;
typedef std::vector<Tensor> TensorList;

// (ROCm builds of torch call their devices "cuda": the masquerading accessor is c10::hip::getCurrentHIPStream for that device type)
void* stream_of(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

void check(int rc, const char* what) {
  TORCH_CHECK(rc == DEVO_OK, what, " failed (code ", rc, "): ", devo_last_error());
}

int dtype_code(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return DEVO_F32;
    case at::kHalf: return DEVO_F16;
    case at::kDouble: return DEVO_F64;
    default: TORCH_CHECK(false, "devo_amd: unsupported dtype ", t.scalar_type());
  }
  return -1;
}

template <typename... Ts>
void require_gpu(const Ts&... ts) {
  for (const Tensor* t : {&ts...})
    TORCH_CHECK(!t->defined() || t->is_cuda(), "devo_amd: tensors must live on the GPU (the HIP path has no CPU fallback)");
}

Tensor idx(const Tensor& t) { return t.to(at::kLong).contiguous(); }
Tensor f32c(const Tensor& t) { return t.to(at::kFloat).contiguous(); }

bool env_off(const char* name) { const char* e = std::getenv(name); return e && e[0] == '0'; }
bool env_on(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }

// ------------------------------------------------------------------------------------------------ version-keyed caches
struct VersionKey {
  const void* ptr; int64_t version; std::vector<int64_t> sizes, strides; at::ScalarType dtype; int flavour;
  bool operator==(const VersionKey& o) const {
    return ptr == o.ptr && version == o.version && dtype == o.dtype && flavour == o.flavour && sizes == o.sizes && strides == o.strides;
  }
};
VersionKey key_of(const Tensor& t, int flavour) {
  return VersionKey{t.data_ptr(), t._version(), t.sizes().vec(), t.strides().vec(), t.scalar_type(), flavour};
}
struct Entry { VersionKey key; Tensor src, a, b; };     // (source kept alive: an equal key is the same storage with the same contents)
struct Lru {
  std::list<Entry> items; size_t cap; std::mutex mu;
  explicit Lru(size_t c) : cap(c) {}
  bool get(const VersionKey& k, Entry* out) {
    std::lock_guard<std::mutex> g(mu);
    for (auto it = items.begin(); it != items.end(); ++it)
      if (it->key == k) { items.splice(items.end(), items, it); *out = items.back(); return true; }
    return false;
  }
  void put(Entry e) {
    std::lock_guard<std::mutex> g(mu);
    for (auto it = items.begin(); it != items.end();) it = (it->key.ptr == e.key.ptr && it->key.flavour == e.key.flavour) ? items.erase(it) : std::next(it);   // older versions
    while (items.size() >= cap) items.pop_front();
    items.push_back(std::move(e));
  }
  void clear() { std::lock_guard<std::mutex> g(mu); items.clear(); }
};
Lru g_levels(4), g_patches(4), g_cl(4);

// ---- per-slot maintenance of a converted ring (round 6).  The reference writes ONE slot of its ring buffers per frame
// (`self.fmap1_[:, self.n % self.mem] = ...`, `self.gmap_[self.n % self.mem] = ...`: devo/devo.py:523-527; keyframe removal moves a few
// slots, :288-291) and then looks the whole ring up: re-converting 32 frames for one new one costs as much as the fp16 lookup itself.
// devo_amd.backends.install() wraps torch.Tensor.__setitem__ (devo_amd/backends/ring.py): a write into a tensor this cache holds a
// converted copy of is RECORDED here — (version counter after the write, element range) — and a later lookup whose key differs from a
// cached entry only in the version converts just the frames / patches the recorded writes touched, PROVIDED every version in between is
// accounted for by a record with a known range (each __setitem__ bumps the counter by exactly one; any other in-place operation leaves a
// gap and the whole tensor is converted again, as in rounds 1-5).  Sound by construction: nothing is assumed about unrecorded writes.
struct WriteRec { uint32_t version; int64_t off, len; };              // elements from the tensor's data_ptr; len < 0: region unknown
std::mutex g_wr_mu;
std::vector<std::pair<const void*, std::vector<WriteRec>>> g_writes;  // a handful of tensors: linear search
struct ConvStats { int64_t level_full = 0, level_frames = 0, patch_full = 0, patch_ranges = 0, patches_partial = 0; } g_conv;
constexpr size_t MAX_WRITE_RECS = 512;

bool is_tracked(const void* ptr) {
  for (Lru* c : {&g_levels, &g_patches}) {
    std::lock_guard<std::mutex> g(c->mu);
    for (const auto& e : c->items) if (e.key.ptr == ptr) return true;
  }
  return false;
}
void note_write(const void* ptr, uint32_t version_after, int64_t off, int64_t len) {
  std::lock_guard<std::mutex> g(g_wr_mu);
  for (auto& kv : g_writes)
    if (kv.first == ptr) {
      if (kv.second.size() >= MAX_WRITE_RECS) kv.second.clear();     // (a gap: the next lookup converts everything)
      kv.second.push_back({version_after, off, len});
      return;
    }
  g_writes.push_back({ptr, {{version_after, off, len}}});
}
void forget_writes(const void* ptr, uint32_t upto) {                  // records of versions <= upto are spent
  std::lock_guard<std::mutex> g(g_wr_mu);
  for (auto it = g_writes.begin(); it != g_writes.end(); ++it)
    if (it->first == ptr) {
      auto& v = it->second;
      v.erase(std::remove_if(v.begin(), v.end(), [&](const WriteRec& r) { return (int32_t)(r.version - upto) <= 0; }), v.end());
      if (v.empty()) g_writes.erase(it);
      return;
    }
}
// every version in (v0, v1] has a record with a known range -> their ranges; else false
bool writes_between(const void* ptr, uint32_t v0, uint32_t v1, std::vector<std::pair<int64_t, int64_t>>* ranges) {
  const uint32_t need = v1 - v0;
  if (need == 0 || need > MAX_WRITE_RECS) return false;
  std::lock_guard<std::mutex> g(g_wr_mu);
  for (auto& kv : g_writes)
    if (kv.first == ptr) {
      std::vector<char> seen(need, 0);
      for (const WriteRec& r : kv.second) {
        const uint32_t d = r.version - v0 - 1;                         // 0 .. need - 1 for the versions wanted
        if (d >= need) continue;
        if (r.len < 0 || seen[d]) return false;
        seen[d] = 1;
        ranges->push_back({r.off, r.off + r.len});
      }
      for (char c : seen) if (!c) return false;
      return true;
    }
  return false;
}
// an entry of the same tensor (storage, shape, strides, dtype, flavour) at an OLDER version
bool find_older(Lru& c, const VersionKey& k, Entry* out) {
  std::lock_guard<std::mutex> g(c.mu);
  for (auto& e : c.items)
    if (e.key.ptr == k.ptr && e.key.flavour == k.flavour && e.key.dtype == k.dtype && e.key.sizes == k.sizes && e.key.strides == k.strides && e.key.version != k.version) {
      *out = e;
      return true;
    }
  return false;
}
bool slot_updates() { static const bool on = !env_off("DEVO_RING_SLOTS"); return on; }

constexpr int64_t PLAN_MIN_EDGES = 2048, NCHW_CONVERT_MIN_EDGES = 1024;
bool mm_kernel() { static const bool on = !env_off("DEVO_CORR_MM") && !env_off("DEVO_CORR_MFMA"); return on; }

// One pyramid level as the C ABI wants it
struct Level { Tensor data, exps; int64_t strides[5]; int cblock; int H, W, n; };

Level describe(const Tensor& f, const Tensor& exps, int C, bool split) {
  Level l;
  l.data = f; l.exps = exps; l.cblock = 0;
  if (f.dim() == 6) {
    l.cblock = split ? DEVO_CBLOCK_SPLIT8 : (int)f.size(5);
    TORCH_CHECK(f.stride(5) == 1 && f.size(2) * f.size(5) == C, "cuda_corr: malformed channel-blocked fmap2");
  }
  for (int i = 0; i < 5; i++) l.strides[i] = f.stride(i);
  l.n = (int)f.size(1); l.H = (int)f.size(3); l.W = (int)f.size(4);
  return l;
}

// cuda_corr._fast_layout of the ctypes binding: NCHW fp16 -> cached channel-blocked copy; fp32 (any layout) -> cached split-blocked copy
// when the dense-product kernel will take the call
Level fast_level(const Tensor& fmap2, int64_t n_edges, bool allow_split) {
  const bool blocked = fmap2.dim() == 6;
  const int C = (int)(fmap2.size(2) * (blocked ? fmap2.size(5) : 1));
  const auto dt = fmap2.scalar_type();
  if ((dt != at::kHalf && dt != at::kFloat) || n_edges <= 0) return describe(fmap2, Tensor(), C, false);
  const bool want_split = allow_split && mm_kernel() && dt == at::kFloat && C % 32 == 0 && C <= 128 && fmap2.numel() > 0;
  const int64_t B = fmap2.size(0), n = fmap2.size(1), H = fmap2.size(3), W = fmap2.size(4);
  if (!want_split) {
    const bool nchw = !blocked && C % 8 == 0 && fmap2.stride(2) == H * W && fmap2.stride(3) == W && fmap2.stride(4) == 1 && B * n > 0;
    if (!nchw || n_edges < NCHW_CONVERT_MIN_EDGES || env_on("DEVO_CORR_NCHW_DIRECT")) return describe(fmap2, Tensor(), C, false);
  }
  const VersionKey k = key_of(fmap2, want_split ? 1 : 0);
  Entry e;
  if (g_levels.get(k, &e)) return describe(e.a, e.b, C, want_split);
  void* st = stream_of(fmap2);
  // the same ring at an older version whose every write since is on record: convert the frames those writes touched, in place
  if (slot_updates() && !blocked && fmap2.is_contiguous() && find_older(g_levels, k, &e) && devo_stream_capturing(st) == 0) {
    std::vector<std::pair<int64_t, int64_t>> ranges;
    if (writes_between(k.ptr, (uint32_t)e.key.version, (uint32_t)k.version, &ranges)) {
      const int64_t per = (int64_t)C * H * W, total = B * n;
      std::vector<char> dirty((size_t)total, 0);
      for (auto& r : ranges)
        for (int64_t f = std::max<int64_t>(0, r.first / per); f < total && f * per < r.second; f++) dirty[(size_t)f] = 1;
      const int64_t es = fmap2.element_size();
      for (int64_t f = 0; f < total; f++) {
        if (!dirty[(size_t)f]) continue;
        int64_t f1 = f;
        while (f1 + 1 < total && dirty[(size_t)(f1 + 1)] && (f1 + 1) / n == f / n) f1++;              // a run of frames of one batch entry
        const int64_t b = f / n, f0 = f - b * n, cnt = f1 - f + 1;
        const char* src = (const char*)fmap2.data_ptr() + (b * fmap2.stride(0) + f0 * fmap2.stride(1)) * es;
        char* dst = (char*)e.a.data_ptr() + (b * e.a.stride(0) + f0 * e.a.stride(1)) * es;
        if (want_split) {
          const int64_t f2s[4] = {fmap2.stride(1), fmap2.stride(2), fmap2.stride(3), fmap2.stride(4)};
          Tensor scratch = at::empty({cnt}, e.b.options());
          check(devo_corr_pyramid_split_frames(src, f2s, 0, (int)cnt, C, (int)H, (int)W, dst, e.a.stride(1), e.b.data_ptr<int>() + b * n + f0, scratch.data_ptr<int>(), st),
                "cuda_corr: fp32 ring slot -> split-blocked");
        } else {
          check(devo_pyramid_build(src, dst, nullptr, (int)cnt, C, (int)H, (int)W, fmap2.stride(1), e.a.stride(1), 0, dtype_code(fmap2), st), "cuda_corr: NCHW ring slot -> channel-blocked");
        }
        g_conv.level_frames += cnt;
        f = f1;
      }
      e.key = k; e.src = fmap2;
      g_levels.put(e);                                          // (replaces the older version's entry: same converted tensors)
      forget_writes(k.ptr, (uint32_t)k.version);
      return describe(e.a, e.b, C, want_split);
    }
  }
  e = Entry();
  e.key = k; e.src = fmap2;
  g_conv.level_full++;
  forget_writes(k.ptr, (uint32_t)k.version);
  if (want_split) {
    e.a = at::empty({B, n, C / 8, H, W, 8}, fmap2.options());
    e.b = at::empty({B * n + n}, fmap2.options().dtype(at::kInt));
    const int64_t f2s[4] = {fmap2.stride(1), fmap2.stride(2), fmap2.stride(3), fmap2.stride(4)};
    for (int64_t b = 0; b < B; b++)                           // ascending: call b's scratch is the (not yet written) slice of b + 1
      check(devo_corr_pyramid_split((const char*)fmap2.data_ptr() + b * fmap2.stride(0) * 4, f2s, blocked ? (int)fmap2.size(5) : 0, (int)n, C, (int)H, (int)W,
                                    (char*)e.a.data_ptr() + b * e.a.stride(0) * 4, e.a.stride(1), e.b.data_ptr<int>() + b * n, st), "cuda_corr: fp32 level -> split-blocked");
  } else {
    e.a = at::empty({B, n, C / 8, H, W, 8}, fmap2.options());
    const int64_t es = fmap2.element_size();
    for (int64_t b = 0; b < B; b++)
      check(devo_pyramid_build((const char*)fmap2.data_ptr() + b * fmap2.stride(0) * es, (char*)e.a.data_ptr() + b * e.a.stride(0) * es, nullptr, (int)n, C, (int)H, (int)W,
                               fmap2.stride(1), e.a.stride(1), 0, dtype_code(fmap2), st), "cuda_corr: NCHW -> channel-blocked");
  }
  g_levels.put(e);
  return describe(e.a, e.b, C, want_split);
}

Tensor patch_operand(const Tensor& fmap1) {            // undefined: the lookup takes the other kernels
  const int64_t C = fmap1.size(2);
  if (!mm_kernel() || fmap1.size(3) != 3 || fmap1.size(4) != 3 || C % 32 != 0 || fmap1.numel() == 0 ||
      (fmap1.scalar_type() != at::kHalf && fmap1.scalar_type() != at::kFloat))
    return Tensor();
  const VersionKey k = key_of(fmap1, 2);
  Entry e;
  if (g_patches.get(k, &e)) return e.a;
  const int64_t n = fmap1.size(0) * fmap1.size(1);
  void* st = stream_of(fmap1);
  if (slot_updates() && fmap1.is_contiguous() && find_older(g_patches, k, &e) && devo_stream_capturing(st) == 0) {   // (see fast_level)
    std::vector<std::pair<int64_t, int64_t>> ranges;
    if (writes_between(k.ptr, (uint32_t)e.key.version, (uint32_t)k.version, &ranges)) {
      const int64_t per = C * 9;
      for (auto& r : ranges) {
        const int64_t p0 = std::max<int64_t>(0, r.first / per), p1 = std::min<int64_t>(n, (r.second + per - 1) / per);
        if (p1 <= p0) continue;
        check(devo_corr_patch_transpose_range(fmap1.data_ptr(), e.a.data_ptr(), (int)n, (int)p0, (int)(p1 - p0), (int)C, dtype_code(fmap1), st), "cuda_corr.patches_transposed (slot)");
        g_conv.patch_ranges++; g_conv.patches_partial += p1 - p0;
      }
      e.key = k; e.src = fmap1;
      g_patches.put(e);
      forget_writes(k.ptr, (uint32_t)k.version);
      return e.a;
    }
  }
  e = Entry();
  const size_t nbytes = devo_corr_patch_operand_bytes((int)n, (int)C, dtype_code(fmap1));
  TORCH_CHECK(nbytes > 0, "cuda_corr: C = ", C, " unsupported by the patch operand (C % 8)");
  e.key = k; e.src = fmap1;
  g_conv.patch_full++;
  forget_writes(k.ptr, (uint32_t)k.version);
  e.a = at::empty({(int64_t)nbytes}, fmap1.options().dtype(at::kByte));
  check(devo_corr_patch_transpose(fmap1.data_ptr(), e.a.data_ptr(), (int)n, (int)C, dtype_code(fmap1), stream_of(fmap1)), "cuda_corr.patches_transposed");
  g_patches.put(e);
  return e.a;
}

Tensor make_plan(const Tensor& coords, const Tensor& jj, int n_frames, int height, float coord_scale, int radius) {
  const int64_t B = coords.size(0), E = coords.size(1);
  Tensor order = at::empty({2 * B * E + 2}, coords.options().dtype(at::kInt));
  check(devo_corr_order(coords.data_ptr<float>(), jj.data_ptr<int64_t>(), order.data_ptr<int>(), (int)B, (int)E, n_frames, (int)coords.size(3), height, coord_scale,
                        radius, 0, 0, stream_of(coords)), "cuda_corr.plan");
  return order;
}

void corr_prep(const Tensor& fmap1, const Tensor& fmap2, const Tensor& coords, bool allow_blocked) {
  TORCH_CHECK(fmap1.scalar_type() == fmap2.scalar_type(), "cuda_corr: fmap1 and fmap2 must have the same dtype");
  TORCH_CHECK(fmap1.dim() == 5 && (fmap2.dim() == 5 || (allow_blocked && fmap2.dim() == 6)) && coords.dim() == 5,
              "cuda_corr: expected fmap1 [B,Np,C,P,P], fmap2 [B,n,C,H,W], coords [B,E,2,P,P]");
}

struct LastPlan { const void* jj = nullptr; uint32_t ver = 0; int64_t BE = 0; int n = 0, radius = 0; void* stream = nullptr; Tensor plan; };
thread_local LastPlan g_last_plan;                                    // the plan a per-level call made, for the call right behind it

// corr forward writing element l of edge (b, e) at out[(b E + e) estride + l lstride + offset]
void corr_forward_into(Tensor& out, const Tensor& fmap1_, const Tensor& fmap2, const Tensor& coords_, const Tensor& ii_, const Tensor& jj_, int radius,
                       int64_t estride, int64_t lstride, int64_t offset, const Tensor& order_, double coord_div) {
  require_gpu(fmap1_, fmap2, coords_, ii_, jj_);
  corr_prep(fmap1_, fmap2, coords_, true);
  c10::DeviceGuard guard(fmap1_.device());
  const Tensor fmap1 = fmap1_.contiguous(), coords = f32c(coords_), ii = idx(ii_), jj = idx(jj_);
  const int64_t B = coords.size(0), E = coords.size(1), P = coords.size(3), Np = fmap1.size(1), C = fmap1.size(2);
  const Tensor f1t = patch_operand(fmap1);
  const Level lv = fast_level(fmap2, B * E, f1t.defined() && lstride > 0);
  Tensor order = order_;
  if (!order.defined() && B * E >= PLAN_MIN_EDGES) {
    // DEVO calls corr once per pyramid level with the SAME index tensors (devo.py:215-216): the second call takes the plan the first one made
    // — "one plan serves every level of a pyramid", and a plan only decides which edges run together: the result does not depend on it by
    // one bit (tests/test_gpu_altcorr.py::test_lookup_results_do_not_depend_on_the_plan).  A plan is handed on ONCE, to the call right behind
    // the one that made it, and only for the same jj tensor (storage, version, size), frame count and stream.
    auto& last = g_last_plan;
    void* st = stream_of(coords);
    if (devo_stream_capturing(st) != 0) {                     // a capture executes nothing: a plan made now holds garbage until the graph runs
      last = LastPlan();                                      // — neither handed on nor taken over
      order = make_plan(coords, jj, lv.n, lv.H, (float)coord_div, radius);
    } else if (last.plan.defined() && last.jj == jj_.data_ptr() && last.ver == jj_._version() && last.BE == B * E && last.n == lv.n && last.radius == radius && last.stream == st &&
        last.plan.device() == coords.device()) {
      order = last.plan;
      last.plan = Tensor();
    } else {
      order = make_plan(coords, jj, lv.n, lv.H, (float)coord_div, radius);
      last.jj = jj_.data_ptr(); last.ver = jj_._version(); last.BE = B * E; last.n = lv.n; last.radius = radius; last.stream = st; last.plan = order;
    }
  }
  check(devo_corr_forward(fmap1.data_ptr(), lv.data.data_ptr(), coords.data_ptr<float>(), ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), out.data_ptr(), (int)B, (int)E,
                          (int)Np, lv.n, (int)C, (int)P, lv.H, lv.W, lv.strides, lv.cblock, estride, lstride, offset, radius, dtype_code(fmap1),
                          order.defined() ? order.data_ptr<int>() : nullptr, (float)coord_div, f1t.defined() ? f1t.data_ptr() : nullptr,
                          lv.exps.defined() ? lv.exps.data_ptr<int>() : nullptr, stream_of(fmap1)), "cuda_corr.forward");
}

// ------------------------------------------------------------------------------------------------ cuda_corr (correlation.cpp:57-63)
TensorList corr_forward(Tensor fmap1, Tensor fmap2, Tensor coords, Tensor ii, Tensor jj, int64_t radius) {       // correlation.cpp:58
  const int64_t B = coords.size(0), E = coords.size(1), P = coords.size(3), Dm = 2 * radius + 1;
  Tensor out = at::empty({B, E, Dm, Dm, P, P}, fmap1.options());
  corr_forward_into(out, fmap1, fmap2, coords, ii, jj, (int)radius, Dm * Dm * P * P, 1, 0, Tensor(), 1.0);
  return {out};
}

thread_local int g_last_bwd_path = -1;

TensorList corr_backward(Tensor fmap1_, Tensor fmap2_, Tensor coords_, Tensor ii_, Tensor jj_, Tensor grad_, int64_t radius) {   // correlation.cpp:59
  require_gpu(fmap1_, fmap2_, coords_, ii_, jj_, grad_);
  corr_prep(fmap1_, fmap2_, coords_, false);
  if (fmap1_.scalar_type() != at::kFloat) {
    // the reference dispatches its backward over half / float / double with a FLOAT gradient accessor (correlation_kernel.cu:146,280);
    // here the kernel is fp32: other dtypes are computed in fp32 and cast back
    const auto dt = fmap1_.scalar_type();
    TensorList g = corr_backward(fmap1_.to(at::kFloat), fmap2_.to(at::kFloat), coords_, ii_, jj_, grad_.to(at::kFloat), radius);
    return {g[0].to(dt), g[1].to(dt)};
  }
  c10::DeviceGuard guard(fmap1_.device());
  const Tensor fmap1 = fmap1_.contiguous(), coords = f32c(coords_), ii = idx(ii_), jj = idx(jj_), grad = f32c(grad_);
  Tensor fmap2 = fmap2_;
  const int64_t B = coords.size(0), E = coords.size(1), P = coords.size(3), Np = fmap1.size(1), C = fmap1.size(2);
  const int64_t n2 = fmap2.size(1), H2 = fmap2.size(3), W2 = fmap2.size(4);
  auto is_cl = [&](const Tensor& f) { return f.stride(2) == 1 && f.stride(4) == C && f.stride(3) == W2 * C && f.stride(1) >= H2 * W2 * C; };
  bool cl = is_cl(fmap2);
  if (!cl && C % 128 == 0 && B * E >= NCHW_CONVERT_MIN_EDGES && !env_on("DEVO_CORR_NCHW_DIRECT") &&
      devo_corr_backward_workspace_bytes((int)B, (int)E, (int)Np, (int)n2, (int)C, (int)radius, 1) > 0) {
    // the product form reads a channels-last copy, cached per version of the tensor: a training step calls backward once per update
    // iteration and level on the SAME pyramid tensors (enet.py:203-216)
    const VersionKey k = key_of(fmap2, 3);
    Entry e;
    if (!g_cl.get(k, &e)) {
      e.key = k; e.src = fmap2.detach();
      e.a = fmap2.detach().permute({0, 1, 3, 4, 2}).contiguous().permute({0, 1, 4, 2, 3});
      g_cl.put(e);
    }
    fmap2 = e.a;
    cl = true;
  }
  Tensor d1 = at::empty_like(fmap1), d2;
  if (cl) {
    d2 = at::empty({B, n2, H2, W2, C}, fmap2.options()).permute({0, 1, 4, 2, 3});
    if (d2.strides() != fmap2.strides()) d2 = at::empty_strided(fmap2.sizes(), fmap2.strides(), fmap2.options());
  } else {
    d2 = at::empty_strided(fmap2.sizes(), fmap2.strides(), fmap2.options());
  }
  int64_t span = 1;
  for (int i = 0; i < 5; i++) span += (fmap2.size(i) - 1) * fmap2.stride(i);
  const size_t nws = devo_corr_backward_workspace_bytes((int)B, (int)E, (int)Np, (int)n2, (int)C, (int)radius, cl ? 1 : 0);
  Tensor ws = nws ? at::empty({(int64_t)nws}, fmap1.options().dtype(at::kByte)) : Tensor();
  const int64_t f2s[5] = {fmap2.stride(0), fmap2.stride(1), fmap2.stride(2), fmap2.stride(3), fmap2.stride(4)};
  check(devo_corr_backward(fmap1.data_ptr(), fmap2.data_ptr(), coords.data_ptr<float>(), ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), grad.data_ptr<float>(),
                           d1.data_ptr(), d2.data_ptr(), (int)B, (int)E, (int)Np, (int)n2, (int)C, (int)P, (int)H2, (int)W2, f2s, span, (int)radius, dtype_code(fmap1),
                           nws ? ws.data_ptr() : nullptr, nws, stream_of(fmap1)), "cuda_corr.backward");
  g_last_bwd_path = devo_corr_backward_last_path();
  return {d1, d2};
}

std::string corr_last_backward_path() {
  static const char* names[3] = {"atomic", "segments", "product"};
  return (g_last_bwd_path >= 0 && g_last_bwd_path < 3) ? names[g_last_bwd_path] : "";
}

TensorList patchify_forward(Tensor net, Tensor coords_, int64_t radius) {                  // correlation.cpp:61
  require_gpu(net, coords_);
  TORCH_CHECK(net.dim() == 4 && coords_.dim() == 3, "cuda_corr.patchify_forward: expected net [B,C,H,W], coords [B,M,2]");
  c10::DeviceGuard guard(net.device());
  const Tensor coords = f32c(coords_);
  const int64_t B = coords.size(0), M = coords.size(1), C = net.size(1), H = net.size(2), W = net.size(3), D = 2 * radius + 2;
  Tensor out = at::empty({B, M, C, D, D}, net.options());
  const int64_t ns[4] = {net.stride(0), net.stride(1), net.stride(2), net.stride(3)};
  check(devo_patchify_forward(net.data_ptr(), coords.data_ptr<float>(), out.data_ptr(), (int)B, (int)M, (int)C, (int)H, (int)W, ns, (int)radius, dtype_code(net),
                              stream_of(net)), "cuda_corr.patchify_forward");
  return {out};
}

TensorList patchify_backward(Tensor net, Tensor coords_, Tensor gradient_, int64_t radius) {    // correlation.cpp:62
  require_gpu(net, coords_, gradient_);
  if (net.scalar_type() == at::kHalf)                     // scattered in fp32 (hardware float atomics), cast back like the forward's dtype
    return {patchify_backward(net.to(at::kFloat), coords_, gradient_.to(at::kFloat), radius)[0].to(at::kHalf)};
  c10::DeviceGuard guard(net.device());
  const Tensor coords = f32c(coords_), gradient = gradient_.to(net.scalar_type()).contiguous();
  const int64_t B = coords.size(0), M = coords.size(1), C = net.size(1), H = net.size(2), W = net.size(3);
  // the gradient in net's own layout when that is a dense permutation (channels-last from the encoders' convolutions), contiguous otherwise
  int64_t span = 1;
  for (int i = 0; i < 4; i++) span += (net.size(i) - 1) * net.stride(i);
  const bool dense = net.numel() > 0 && span == net.numel();
  Tensor out = dense ? at::empty_strided(net.sizes(), net.strides(), net.options()) : at::empty({B, C, H, W}, net.options());
  const int64_t gs[4] = {out.stride(0), out.stride(1), out.stride(2), out.stride(3)};
  check(devo_patchify_backward(coords.data_ptr<float>(), gradient.data_ptr(), out.data_ptr(), (int)B, (int)M, (int)C, (int)H, (int)W, gs, (int)radius, dtype_code(net),
                               stream_of(net)), "cuda_corr.patchify_backward");
  return {out};
}

// ------------------------------------------------------------------------------------------------ cuda_ba (ba.cpp:152-157)
// One live workspace per (problem size, device, STREAM): two streams never share scratch, and a workspace that is replaced stays alive until
// the work enqueued on it has run (the caching allocator frees a block for reuse on the stream it was allocated on: a stream-ordered free).
struct WsKey { int E, Np, N, dev; void* stream; bool operator==(const WsKey& o) const { return E == o.E && Np == o.Np && N == o.N && dev == o.dev && stream == o.stream; } };
std::mutex g_ws_mu;
WsKey g_ws_key{-1, -1, -1, -1, nullptr};
Tensor g_ws;

Tensor ba_workspace(int E, int Np, int N, const at::Device& dev, void* stream) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  const WsKey k{E, Np, N, (int)dev.index(), stream};
  if (g_ws.defined() && g_ws_key == k) return g_ws;
  const size_t nbytes = devo_ba_workspace_bytes(E, Np, N);
  TORCH_CHECK(nbytes > 0, "cuda_ba: unsupported problem size (E=", E, ", Np=", Np, ", N=", N, "; at most 128 optimised poses)");
  g_ws = at::empty({(int64_t)nbytes}, at::TensorOptions().dtype(at::kByte).device(dev));     // one live workspace: the graph size changes once per frame
  g_ws_key = k;
  return g_ws;
}

// The index half of cuda_ba.forward (unique patches, edges grouped by patch: ba_cuda.cu:435-437) depends on kk alone, and DEVO calls the BA
// again and again on one graph (18 update iterations per training sequence, train.py / enet.py:313-361; 12 at initialisation, devo.py:545).
// The prepared tables of the LAST call are kept with the workspace they live in: key = (kk's storage address and version counter, E, patch
// slots, window size, workspace, stream); the cache keeps kk and the workspace alive, so an equal key is the same storage with the same
// contents.  A hit runs devo_ba_forward_prepared: one launch (12.6 us at cfg2) less per call.  Never consulted or filled while the stream is
// being captured into a graph (a capture executes nothing: the tables would not exist).  DEVO_BA_PREP_CACHE=0 switches it off.
struct PrepKey {
  const void* kk = nullptr; uint32_t ver = 0; int64_t E = -1; int Np = -1, N = -1; const void* ws = nullptr; void* stream = nullptr;
  bool operator==(const PrepKey& o) const { return kk == o.kk && ver == o.ver && E == o.E && Np == o.Np && N == o.N && ws == o.ws && stream == o.stream; }
};
std::mutex g_prep_mu;
PrepKey g_prep_key;
Tensor g_prep_kk, g_prep_ws;
int64_t g_prep_hits = 0, g_prep_misses = 0;
void ba_prep_invalidate() { std::lock_guard<std::mutex> g(g_prep_mu); g_prep_key = PrepKey(); g_prep_kk = Tensor(); g_prep_ws = Tensor(); }

// ba.cpp:153.  Mutates poses ([1,Nbuf,7]) and patches ([1,Np,3,P,P]) in place and returns [] (devo/fastba/ba.py:7-8 passes poses.data;
// devo/devo.py:337 relies on the mutation).  ws / status / prepared: extras of this package's callers (devo_amd.fastba).
TensorList ba_forward(Tensor poses, Tensor patches, Tensor intrinsics_, Tensor target_, Tensor weight_, Tensor lmbda_, Tensor ii_, Tensor jj_, Tensor kk_,
                      int64_t t0, int64_t t1, int64_t iterations, c10::optional<Tensor> ws_, c10::optional<Tensor> status_, bool prepared) {
  require_gpu(poses, patches, intrinsics_, target_, weight_, lmbda_, ii_, jj_, kk_);
  TORCH_CHECK(poses.scalar_type() == at::kFloat && poses.is_contiguous(), "cuda_ba.forward: poses must be a contiguous float32 tensor (it is updated in place)");
  TORCH_CHECK(patches.scalar_type() == at::kFloat && patches.is_contiguous(), "cuda_ba.forward: patches must be a contiguous float32 tensor (it is updated in place)");
  c10::DeviceGuard guard(poses.device());
  const int64_t P = patches.size(-1), Nbuf = poses.numel() / 7, Np = patches.numel() / (3 * P * P);
  const Tensor ii = idx(ii_), jj = idx(jj_), kk = idx(kk_);
  const int64_t E = ii.numel();
  const Tensor intrinsics = f32c(intrinsics_), target = f32c(target_), weight = f32c(weight_), lmbda = f32c(lmbda_.reshape({-1}));
  TORCH_CHECK(!(prepared && !(ws_.has_value() && ws_->defined())), "cuda_ba.forward: prepared=True needs the workspace that prepare() filled");
  void* st = stream_of(poses);
  Tensor ws = (ws_.has_value() && ws_->defined()) ? *ws_ : ba_workspace((int)E, (int)Np, (int)(t1 - t0), poses.device(), st);
  int* status = (status_.has_value() && status_->defined()) ? status_->data_ptr<int>() : nullptr;
  static const bool prep_cache = !env_off("DEVO_BA_PREP_CACHE");
  if (!prepared && prep_cache && E > 0 && iterations > 0) {
    if (devo_stream_capturing(st) != 0) ba_prep_invalidate();          // (a graph replay rewrites the workspace's tables behind the cache's back)
    else if (!kk_.is_inference()) {
      const PrepKey k{kk_.data_ptr(), (uint32_t)kk_._version(), E, (int)Np, (int)(t1 - t0), ws.data_ptr(), st};
      std::lock_guard<std::mutex> g(g_prep_mu);
      if (g_prep_key == k) { prepared = true; g_prep_hits++; }
      else { g_prep_key = k; g_prep_kk = kk_; g_prep_ws = ws; g_prep_misses++; }     // this call prepares: the tables are in `ws` behind it
    }
  } else if (prepared) ba_prep_invalidate();                           // the caller's own prepare() filled the workspace: not the cached graph's tables
  auto fn = prepared ? devo_ba_forward_prepared : devo_ba_forward;
  check(fn(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), target.data_ptr<float>(), weight.data_ptr<float>(), lmbda.data_ptr<float>(),
           ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), (int)E, (int)Nbuf, (int)Np, (int)P, (int)t0, (int)t1, (int)iterations, ws.data_ptr(),
           (size_t)ws.numel(), status, st), "cuda_ba.forward");
  return {};
}

TensorList ba_neighbors(Tensor ii_, Tensor jj_) {                       // ba.cpp:154 -> [ix, jx] (int64, on the GPU); no device<->host round trip
  require_gpu(ii_, jj_);
  c10::DeviceGuard guard(ii_.device());
  const Tensor ii = idx(ii_), jj = idx(jj_);
  const int64_t E = ii.numel();
  Tensor ix = at::empty({E}, ii.options()), jx = at::empty({E}, ii.options());
  Tensor ws = at::empty({(int64_t)devo_neighbors_workspace_bytes((int)E)}, ii.options().dtype(at::kByte));
  check(devo_ba_neighbors(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), ix.data_ptr<int64_t>(), jx.data_ptr<int64_t>(), (int)E, ws.data_ptr(), (size_t)ws.numel(),
                          stream_of(ii)), "cuda_ba.neighbors");
  return {ix, jx};
}

Tensor ba_reproject(Tensor poses_, Tensor patches_, Tensor intrinsics_, Tensor ii_, Tensor jj_, Tensor kk_) {      // ba.cpp:155 -> coords [1, E, 2, P, P]
  require_gpu(poses_, patches_, intrinsics_, ii_, jj_, kk_);
  c10::DeviceGuard guard(poses_.device());
  const int64_t P = patches_.size(-1);
  const Tensor ii = idx(ii_), jj = idx(jj_), kk = idx(kk_), poses = f32c(poses_), patches = f32c(patches_), intrinsics = f32c(intrinsics_);
  const int64_t E = ii.numel();
  Tensor coords = at::empty({1, E, 2, P, P}, poses.options());
  check(devo_ba_reproject(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(),
                          kk.data_ptr<int64_t>(), coords.data_ptr<float>(), (int)E, (int)P, stream_of(poses)), "cuda_ba.reproject");
  return coords;
}

// the fused form of devo/projective_ops.py:53-105 that DEVO.update really calls (no plan, no Jacobians: devo_amd.backends.cuda_ba.transform
// has the full argument list); layout "pp2": [1,E,P,P,2], "2pp": [1,E,2,P,P]
Tensor ba_transform(Tensor poses_, Tensor patches_, Tensor intrinsics_, Tensor ii_, Tensor jj_, Tensor kk_, bool layout_2pp) {
  require_gpu(poses_, patches_, intrinsics_, ii_, jj_, kk_);
  c10::DeviceGuard guard(poses_.device());
  const int64_t P = patches_.size(-1);
  const Tensor ii = idx(ii_), jj = idx(jj_), kk = idx(kk_), poses = f32c(poses_), patches = f32c(patches_), intrinsics = f32c(intrinsics_);
  const int64_t E = ii.numel();
  Tensor c = layout_2pp ? at::empty({1, E, 2, P, P}, poses.options()) : at::empty({1, E, P, P, 2}, poses.options());
  check(devo_transform(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(),
                       layout_2pp ? nullptr : c.data_ptr<float>(), layout_2pp ? c.data_ptr<float>() : nullptr, nullptr, nullptr, nullptr, nullptr, (int)E, (int)P, 0,
                       nullptr, 0, 0, 0, 0, 0, stream_of(poses)), "cuda_ba.transform");
  return c;
}

// ------------------------------------------------------------------------------------------------ lietorch_backends (lietorch.cpp:286-316): SO3, RxSO3, SE3, Sim3
// Operand kinds: the last dimension of every operand is checked against the group (the reference reads whatever is there).
enum LieDim { LIE_N = -1, LIE_K = -2 };   // an element (N), a tangent (K); 3 and 4 stand for themselves (points)
inline int64_t lie_dim(int64_t group_id, int what) {
  static const int64_t N[5] = {0, 4, 5, 7, 8};                                                         // dispatch.h, so3.h:14-15 ... sim3.h:19-20
  return what == LIE_N ? N[group_id] : what == LIE_K ? N[group_id] - 1 : what;
}
inline void lie_chk(int64_t group_id, std::initializer_list<std::pair<const Tensor*, int>> ts) {
  TORCH_CHECK(group_id >= 1 && group_id <= 4, "lietorch_backends (devo_amd): group_id must be 1 (SO3), 2 (RxSO3), 3 (SE3) or 4 (Sim3), got ", group_id);
  const Tensor& first = *ts.begin()->first;
  for (const auto& tw : ts) {
    const Tensor* t = tw.first;
    TORCH_CHECK(t->is_cuda(), "devo_amd: tensors must live on the GPU (the HIP path has no CPU fallback)");
    TORCH_CHECK(t->is_contiguous(), "lietorch_backends: input must be contiguous");                    // lietorch.cpp:7
    TORCH_CHECK(t->scalar_type() == at::kFloat || t->scalar_type() == at::kDouble, "lietorch_backends: float32/float64 only, got ", t->scalar_type());
    TORCH_CHECK(t->scalar_type() == first.scalar_type(), "lietorch_backends: mixed dtypes");
    const int64_t want = lie_dim(group_id, tw.second);
    TORCH_CHECK(t->dim() >= 2 && t->size(-1) == want && t->size(0) == first.size(0) && t->numel() == t->size(0) * want, "lietorch_backends: expected a [", first.size(0),
                ", ", want, "] tensor for group ", group_id, ", got ", t->sizes());
  }
}
typedef int (*un_fn)(int, const void*, void*, int64_t, int, devo_stream_t);
typedef int (*unb_fn)(int, const void*, const void*, void*, int64_t, int, devo_stream_t);
typedef int (*bin_fn)(int, const void*, const void*, void*, int64_t, int, devo_stream_t);
typedef int (*binb_fn)(int, const void*, const void*, const void*, void*, void*, int64_t, int, devo_stream_t);

template <un_fn F, int IN, int OUT>
Tensor lie_unary(int64_t gid, Tensor X) {
  lie_chk(gid, {{&X, IN}});
  c10::DeviceGuard guard(X.device());
  Tensor out = at::empty({X.size(0), lie_dim(gid, OUT)}, X.options());
  check(F((int)gid, X.data_ptr(), out.data_ptr(), X.size(0), dtype_code(X), stream_of(X)), "lietorch_backends");
  return out;
}
template <unb_fn F, int GRAD, int IN, int OUT>
TensorList lie_unary_bwd(int64_t gid, Tensor grad, Tensor X) {
  lie_chk(gid, {{&grad, GRAD}, {&X, IN}});
  c10::DeviceGuard guard(X.device());
  Tensor out = at::empty({X.size(0), lie_dim(gid, OUT)}, X.options());
  check(F((int)gid, grad.data_ptr(), X.data_ptr(), out.data_ptr(), X.size(0), dtype_code(X), stream_of(X)), "lietorch_backends");
  return {out};
}
template <bin_fn F, int Y, int OUT>
Tensor lie_binary(int64_t gid, Tensor X, Tensor y) {
  lie_chk(gid, {{&X, LIE_N}, {&y, Y}});
  c10::DeviceGuard guard(X.device());
  Tensor out = at::empty({X.size(0), lie_dim(gid, OUT)}, X.options());
  check(F((int)gid, X.data_ptr(), y.data_ptr(), out.data_ptr(), X.size(0), dtype_code(X), stream_of(X)), "lietorch_backends");
  return out;
}
template <binb_fn F, int GRAD, int Y>
TensorList lie_binary_bwd(int64_t gid, Tensor grad, Tensor X, Tensor y) {
  lie_chk(gid, {{&grad, GRAD}, {&X, LIE_N}, {&y, Y}});
  c10::DeviceGuard guard(X.device());
  Tensor dX = at::empty({X.size(0), lie_dim(gid, LIE_N)}, X.options()), dy = at::empty({X.size(0), lie_dim(gid, Y)}, X.options());
  check(F((int)gid, grad.data_ptr(), X.data_ptr(), y.data_ptr(), dX.data_ptr(), dy.data_ptr(), X.size(0), dtype_code(X), stream_of(X)), "lietorch_backends");
  return {dX, dy};
}
Tensor lie_as_matrix(int64_t gid, Tensor X) {
  lie_chk(gid, {{&X, LIE_N}});
  c10::DeviceGuard guard(X.device());
  Tensor out = at::empty({X.size(0), 4, 4}, X.options());
  check(devo_lie_as_matrix((int)gid, X.data_ptr(), out.data_ptr(), X.size(0), dtype_code(X), stream_of(X)), "devo_lie_as_matrix");
  return out;
}
Tensor lie_projector(int64_t gid, Tensor X) {                                                          // lietorch.cpp:312: [n, N, N]
  lie_chk(gid, {{&X, LIE_N}});
  c10::DeviceGuard guard(X.device());
  const int64_t N = lie_dim(gid, LIE_N);
  Tensor out = at::empty({X.size(0), N, N}, X.options());
  check(devo_lie_projector((int)gid, X.data_ptr(), out.data_ptr(), X.size(0), dtype_code(X), stream_of(X)), "devo_lie_projector");
  return out;
}

// extras for devo_amd.backends.cuda_corr (one cache for both bindings)
std::tuple<Tensor, c10::optional<Tensor>, int64_t> corr_fast_layout(Tensor fmap2, int64_t n_edges, bool allow_split) {
  require_gpu(fmap2);
  c10::DeviceGuard guard(fmap2.device());
  const Level l = fast_level(fmap2, n_edges, allow_split);
  return {l.data, l.exps.defined() ? c10::optional<Tensor>(l.exps) : c10::nullopt, (int64_t)l.cblock};
}
c10::optional<Tensor> corr_patch_operand(Tensor fmap1) {
  require_gpu(fmap1);
  c10::DeviceGuard guard(fmap1.device());
  const Tensor t = patch_operand(fmap1.contiguous());
  return t.defined() ? c10::optional<Tensor>(t) : c10::nullopt;
}
// ------------------------------------------------------------------------------------------------ patch graph (devo_amd/graph.py; csrc/graph.hip)
// Thin forms of the devo_graph_* entry points: tensors for pointers, the current stream of the index tensors' device.  `record` is a pinned
// HOST tensor the kernels write (devo_hip.h); the Python class owns the buffers, the event and the version counters.
const int64_t* i64p(const Tensor& t) { return t.data_ptr<int64_t>(); }
void pg_check_idx(const char* what, const Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous(), what, ": index tensors must be contiguous int64 tensors on the GPU");
}
void pg_geometry(const char* what, const Tensor& poses, const Tensor& patches, const Tensor& intrinsics) {
  require_gpu(poses, patches, intrinsics);
  TORCH_CHECK(poses.scalar_type() == at::kFloat && poses.is_contiguous() && patches.scalar_type() == at::kFloat && patches.is_contiguous() &&
              intrinsics.scalar_type() == at::kFloat && intrinsics.is_contiguous(), what, ": poses, patches and intrinsics must be contiguous float32 tensors");
}

void pg_motion(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ii, Tensor jj, Tensor kk, int64_t E, int64_t i, int64_t j, double beta, Tensor ws, Tensor record) {
  pg_geometry("patch_graph.motion", poses, patches, intrinsics);
  pg_check_idx("patch_graph.motion", ii); pg_check_idx("patch_graph.motion", jj); pg_check_idx("patch_graph.motion", kk);
  c10::DeviceGuard guard(ii.device());
  const int64_t P = patches.size(-1);
  check(devo_graph_motion(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), i64p(ii), i64p(jj), i64p(kk), (int)E, (int)(poses.numel() / 7),
                          (int)(patches.numel() / (3 * P * P)), (int)P, (int)i, (int)j, (float)beta, ws.data_ptr(), (size_t)ws.numel(), record.data_ptr(), stream_of(ii)),
        "patch_graph.motion");
}

void pg_keyframe(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ii, Tensor jj, Tensor kk, Tensor net, Tensor ix, Tensor ii_out, Tensor jj_out, Tensor kk_out,
                 Tensor net_out, int64_t E, int64_t M, int64_t n, int64_t keyframe_index, double thresh, int64_t removal_window, double beta, Tensor ws, Tensor record) {
  pg_geometry("patch_graph.keyframe", poses, patches, intrinsics);
  for (const Tensor* t : {&ii, &jj, &kk, &ix, &ii_out, &jj_out, &kk_out}) pg_check_idx("patch_graph.keyframe", *t);
  require_gpu(net, net_out);
  c10::DeviceGuard guard(ii.device());
  const int64_t P = patches.size(-1);
  check(devo_graph_keyframe(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), i64p(ii), i64p(jj), i64p(kk), net.data_ptr(), i64p(ix),
                            ii_out.data_ptr<int64_t>(), jj_out.data_ptr<int64_t>(), kk_out.data_ptr<int64_t>(), net_out.data_ptr(), (int)E, (int)(poses.numel() / 7),
                            (int)(patches.numel() / (3 * P * P)), ix.numel(), (int)P, (int)net.size(-1), dtype_code(net), (int)M, (int)n, (int)keyframe_index, thresh,
                            (int)removal_window, (float)beta, ws.data_ptr(), (size_t)ws.numel(), record.data_ptr(), stream_of(ii)), "patch_graph.keyframe");
}

void pg_remove(Tensor ii, Tensor jj, Tensor kk, Tensor net, Tensor mask, Tensor ii_out, Tensor jj_out, Tensor kk_out, Tensor net_out, int64_t E, Tensor ws, Tensor record) {
  for (const Tensor* t : {&ii, &jj, &kk, &ii_out, &jj_out, &kk_out}) pg_check_idx("patch_graph.remove", *t);
  require_gpu(net, net_out, mask);
  TORCH_CHECK((mask.scalar_type() == at::kBool || mask.scalar_type() == at::kByte) && mask.is_contiguous(), "patch_graph.remove: the mask must be a contiguous bool tensor");
  c10::DeviceGuard guard(ii.device());
  check(devo_graph_remove(i64p(ii), i64p(jj), i64p(kk), net.data_ptr(), (const unsigned char*)mask.data_ptr(), ii_out.data_ptr<int64_t>(), jj_out.data_ptr<int64_t>(),
                          kk_out.data_ptr<int64_t>(), net_out.data_ptr(), (int)E, (int)net.size(-1), dtype_code(net), ws.data_ptr(), (size_t)ws.numel(), record.data_ptr(),
                          stream_of(ii)), "patch_graph.remove");
}

void pg_append(Tensor ii, Tensor jj, Tensor kk, Tensor net_old, Tensor net_new, Tensor ix, Tensor patch_ids, Tensor frame_ids, int64_t E, int64_t n_new) {
  for (const Tensor* t : {&ii, &jj, &kk, &ix, &patch_ids, &frame_ids}) pg_check_idx("patch_graph.append", *t);
  require_gpu(net_old, net_new);
  c10::DeviceGuard guard(ii.device());
  check(devo_graph_append(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), net_old.data_ptr(), net_new.data_ptr(), i64p(ix), ix.numel(), i64p(patch_ids),
                          i64p(frame_ids), (int)E, (int)n_new, (int)ii.numel(), (int)net_new.size(-1), dtype_code(net_new), stream_of(ii)), "patch_graph.append");
}

void pg_append_frame(Tensor ii, Tensor jj, Tensor kk, Tensor net_old, Tensor net_new, Tensor ix, int64_t M, int64_t n, int64_t lifetime, int64_t E) {
  for (const Tensor* t : {&ii, &jj, &kk, &ix}) pg_check_idx("patch_graph.append_frame", *t);
  require_gpu(net_old, net_new);
  c10::DeviceGuard guard(ii.device());
  check(devo_odom_append_frame(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), net_old.data_ptr(), net_new.data_ptr(), i64p(ix), ix.numel(), (int)M,
                               (int)n, (int)lifetime, (int)E, (int)ii.numel(), (int)net_new.size(-1), dtype_code(net_new), stream_of(ii)), "patch_graph.append_frame");
}

void pg_shift_frames(TensorList tensors, int64_t k, int64_t n) {
  if (tensors.empty()) return;
  std::vector<void*> ptrs;
  std::vector<int64_t> rows;
  for (const Tensor& t : tensors) {
    require_gpu(t);
    TORCH_CHECK(t.dim() >= 1 && t.is_contiguous() && t.size(0) >= n && t.device() == tensors[0].device(), "patch_graph.shift_frames: contiguous tensors of at least n rows on one device");
    ptrs.push_back(t.data_ptr());
    rows.push_back(t.size(0) ? (int64_t)(t.numel() / t.size(0) * t.element_size()) : 0);
  }
  c10::DeviceGuard guard(tensors[0].device());
  check(devo_graph_shift_frames(ptrs.data(), rows.data(), (int)ptrs.size(), (int)k, (int)n, stream_of(tensors[0])), "patch_graph.shift_frames");
}

// ------------------------------------------------------------------------------------------------ training graph (devo_amd/train_graph.py; csrc/train_graph.hip)
// Thin forms of the devo_train_graph_* entry points.  idx: int64 [3, cap] (ii, jj, kk); close / far: int64 [4, cap] (position, ii, jj, kk).  The Python
// class owns the buffers, the size model and the version counters.
void tg_check_rows(const char* what, const Tensor& t, int64_t rows) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous() && t.dim() == 2 && t.size(0) == rows, what, ": expected a contiguous int64 [", rows, ", cap] tensor on the GPU");
}
void tg_init(Tensor idx, int64_t M, int64_t init_frames, Tensor close, Tensor far_, Tensor ws) {
  tg_check_rows("train_graph.init", idx, 3); tg_check_rows("train_graph.init", close, 4); tg_check_rows("train_graph.init", far_, 4);
  require_gpu(ws);
  c10::DeviceGuard guard(idx.device());
  check(devo_train_graph_init(idx.data_ptr<int64_t>(), idx.size(1), (int)M, (int)init_frames, close.data_ptr<int64_t>(), close.size(1), far_.data_ptr<int64_t>(), far_.size(1),
                              ws.data_ptr(), (size_t)ws.numel(), stream_of(idx)), "train_graph.init");
}
void tg_grow(Tensor src, int64_t E_old, Tensor dst, int64_t E_new, int64_t M, int64_t n, bool drop, Tensor net_old, Tensor net_new, const c10::optional<Tensor>& map,
             Tensor poses_in, Tensor poses_out, Tensor patches_in, Tensor patches_out, Tensor close, Tensor far_, Tensor ws) {
  tg_check_rows("train_graph.grow", src, 3); tg_check_rows("train_graph.grow", dst, 3); tg_check_rows("train_graph.grow", close, 4); tg_check_rows("train_graph.grow", far_, 4);
  pg_geometry("train_graph.grow", poses_in, patches_in, poses_out);
  pg_geometry("train_graph.grow", poses_out, patches_out, poses_out);
  require_gpu(net_old, net_new, ws);
  TORCH_CHECK(net_old.is_contiguous() && net_new.is_contiguous() && net_old.scalar_type() == net_new.scalar_type() && net_old.size(-1) == net_new.size(-1) &&
              net_old.numel() == E_old * net_old.size(-1) && net_new.numel() == E_new * net_new.size(-1), "train_graph.grow: net [E_old, dim] and net' [E_new, dim], contiguous, one dtype");
  TORCH_CHECK(poses_out.numel() == poses_in.numel() && patches_out.numel() == patches_in.numel() && patches_in.dim() >= 3, "train_graph.grow: poses' and patches' have the shapes of poses and patches");
  const bool has = map.has_value() && map->defined();
  TORCH_CHECK(!has || (map->is_cuda() && map->scalar_type() == at::kInt && map->is_contiguous() && map->numel() >= E_old), "train_graph.grow: map must be a contiguous int32 tensor of E_old entries on the GPU");
  c10::DeviceGuard guard(src.device());
  const int64_t P = patches_in.size(-1), N = poses_in.numel() / 7;
  TORCH_CHECK(patches_in.numel() == N * M * 3 * P * P, "train_graph.grow: patches must hold M patches for each of the ", N, " poses");
  check(devo_train_graph_grow(i64p(src), src.size(1), (int)E_old, dst.data_ptr<int64_t>(), dst.size(1), (int)E_new, (int)M, (int)n, drop ? 1 : 0, net_old.data_ptr(),
                              net_new.data_ptr(), (int)net_new.size(-1), dtype_code(net_new), has ? map->data_ptr<int>() : nullptr, poses_in.data_ptr<float>(),
                              poses_out.data_ptr<float>(), (int)N, patches_in.data_ptr<float>(), patches_out.data_ptr<float>(), (int)P, close.data_ptr<int64_t>(),
                              close.size(1), far_.data_ptr<int64_t>(), far_.size(1), ws.data_ptr(), (size_t)ws.numel(), stream_of(src)), "train_graph.grow");
}
void tg_net_backward(Tensor grad_new, Tensor map, Tensor grad_old, int64_t E_new) {
  require_gpu(grad_new, map, grad_old);
  TORCH_CHECK(grad_new.is_contiguous() && grad_old.is_contiguous() && grad_new.scalar_type() == grad_old.scalar_type() && grad_new.size(-1) == grad_old.size(-1) &&
              grad_new.numel() == E_new * grad_new.size(-1), "train_graph.net_backward: contiguous gradients of one dtype and row length");
  TORCH_CHECK(map.scalar_type() == at::kInt && map.is_contiguous() && map.numel() * grad_old.size(-1) == grad_old.numel(), "train_graph.net_backward: map must be a contiguous int32 tensor of E_old entries");
  c10::DeviceGuard guard(map.device());
  check(devo_train_graph_net_backward(grad_new.data_ptr(), map.data_ptr<int>(), grad_old.data_ptr(), (int)map.numel(), (int)E_new, (int)grad_old.size(-1), dtype_code(grad_old),
                                      stream_of(map)), "train_graph.net_backward");
}

// ------------------------------------------------------------------------------------------------ frame graph (devo_amd/frame_graph.py; csrc/frame_graph.hip)
// The devo_frame_graph_* entry points on tensors: fp32, contiguous, on the GPU; each call owns its workspace (this runs once per scene).
void fg_check(const char* what, const Tensor& t, int64_t dims) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.dim() == dims, what, ": expected a contiguous float32 tensor of ", dims, " dimensions on the GPU");
}
Tensor fg_workspace(const char* what, const Tensor& like, int64_t N, int64_t h, int64_t w) {
  TORCH_CHECK(N >= 1 && N <= DEVO_FRAME_GRAPH_MAX_FRAMES, what, ": 1 <= N <= ", DEVO_FRAME_GRAPH_MAX_FRAMES, ", got ", N);
  TORCH_CHECK(h >= 1 && w >= 1 && 2 * h * w < DEVO_FRAME_GRAPH_MAX_POINTS, what, ": maps of ", h, " x ", w, " are not supported: 2 h w must stay below ", DEVO_FRAME_GRAPH_MAX_POINTS);
  return at::empty({(int64_t)devo_frame_graph_workspace_bytes((int)N, (int)h, (int)w)}, like.options().dtype(at::kByte));
}
Tensor fg_disps(Tensor depths) {
  fg_check("frame_graph.disps", depths, 3);
  c10::DeviceGuard guard(depths.device());
  fg_workspace("frame_graph.disps", depths, depths.size(0), depths.size(1), depths.size(2));      // (the size checks)
  Tensor out = at::empty_like(depths);
  check(devo_frame_graph_disps(depths.data_ptr<float>(), out.data_ptr<float>(), (int)depths.size(0), (int)depths.size(1), (int)depths.size(2), stream_of(depths)),
        "frame_graph.disps");
  return out;
}
Tensor fg_distances(Tensor poses, Tensor disps, Tensor intrinsics, double scale) {
  fg_check("frame_graph.distances", poses, 2); fg_check("frame_graph.distances", disps, 3); fg_check("frame_graph.distances", intrinsics, 2);
  const int64_t N = disps.size(0);
  TORCH_CHECK(poses.size(0) == N && poses.size(1) == 7 && intrinsics.size(0) == N && intrinsics.size(1) == 4 && poses.device() == disps.device() &&
              intrinsics.device() == disps.device(), "frame_graph.distances: poses [N, 7], disps [N, h, w] and intrinsics [N, 4] of one N on one device");
  c10::DeviceGuard guard(disps.device());
  Tensor ws = fg_workspace("frame_graph.distances", disps, N, disps.size(1), disps.size(2));
  Tensor matrix = at::empty({N, N}, disps.options());
  check(devo_frame_graph_distances(poses.data_ptr<float>(), disps.data_ptr<float>(), intrinsics.data_ptr<float>(), (int)N, (int)disps.size(1), (int)disps.size(2), (float)scale,
                                   matrix.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), stream_of(disps)), "frame_graph.distances");
  return matrix;
}
// (rowptr i64 [N + 1], cols i64, dists f32); waits once for the total length
TensorList fg_lists(Tensor matrix, double max_flow) {
  fg_check("frame_graph.lists", matrix, 2);
  const int64_t N = matrix.size(0);
  TORCH_CHECK(matrix.size(1) == N, "frame_graph.lists: the matrix is square");
  c10::DeviceGuard guard(matrix.device());
  Tensor ws = fg_workspace("frame_graph.lists", matrix, N, 1, 1);
  Tensor rowptr = at::empty({N + 1}, matrix.options().dtype(at::kLong));
  check(devo_frame_graph_lists(matrix.data_ptr<float>(), (int)N, (float)max_flow, rowptr.data_ptr<int64_t>(), nullptr, nullptr, 0, ws.data_ptr(), (size_t)ws.numel(),
                               stream_of(matrix)), "frame_graph.lists");
  const int64_t total = rowptr[N].item<int64_t>();
  Tensor cols = at::empty({total}, rowptr.options()), dists = at::empty({total}, matrix.options());
  if (total > 0)
    check(devo_frame_graph_lists(matrix.data_ptr<float>(), (int)N, (float)max_flow, rowptr.data_ptr<int64_t>(), cols.data_ptr<int64_t>(), dists.data_ptr<float>(), total,
                                 ws.data_ptr(), (size_t)ws.numel(), stream_of(matrix)), "frame_graph.lists");
  return {rowptr, cols, dists};
}

// ------------------------------------------------------------------------------------------------ patch selection (devo_amd/select.py; csrc/select.hip)
// devo_patch_select on tensors: scores f32 [n, h, w] (any strides), the outputs are allocated here.  The Python module checks modes and sizes, draws
// the noise / candidates and reads the nms counts.  -> {x, y, xy, scores, patches, index, counts (nms; empty otherwise)}
TensorList patch_select(const Tensor& scores, int64_t m, int64_t mode, bool grid, int64_t k, bool pad, const c10::optional<Tensor>& noise,
                        const c10::optional<Tensor>& cand_x, const c10::optional<Tensor>& cand_y, int64_t offset, bool clamp, int64_t cx0, int64_t cx1, int64_t cy0,
                        int64_t cy1, const c10::optional<Tensor>& disps, int64_t P) {
  TORCH_CHECK(scores.is_cuda() && scores.scalar_type() == at::kFloat && scores.dim() == 3, "select: scores must be a float32 tensor [n, h, w] on the GPU");
  const int64_t n = scores.size(0), h = scores.size(1), w = scores.size(2);
  TORCH_CHECK(n >= 1 && h >= 1 && w >= 1 && m >= 1 && m <= DEVO_SELECT_MAX_CELLS && P >= 1, "select: n, h, w, P >= 1 and 1 <= m <= ", DEVO_SELECT_MAX_CELLS);
  const int64_t f = grid ? 2 * k : k;
  TORCH_CHECK(k >= 1, "select: k >= 1");
  const int64_t C = pad ? ((h + (f - h % f) % f) / k) * ((w + (f - w % f) % f) / k) : (h / k) * (w / k);
  const bool has_noise = noise.has_value() && noise->defined(), has_cand = cand_x.has_value() && cand_x->defined() && cand_y.has_value() && cand_y->defined();
  const bool has_disps = disps.has_value() && disps->defined();
  if (mode == DEVO_SELECT_MULTI)
    TORCH_CHECK(has_noise && noise->is_cuda() && noise->scalar_type() == at::kFloat && noise->is_contiguous() && noise->dim() == 2 && noise->size(0) == n &&
                noise->size(1) == C + 16 * m && noise->device() == scores.device(), "select: multi takes noise float32 [n, C + 16 m] = [", n, ", ", C + 16 * m, "] on the scores' device");
  if (mode == DEVO_SELECT_3XRANDOM) {
    TORCH_CHECK(has_cand, "select: 3xrandom takes candidates (x, y)");
    for (const Tensor* t : {&*cand_x, &*cand_y})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous() && t->dim() == 2 && t->size(0) == n && t->size(1) == 3 * m && t->device() == scores.device(),
                  "select: candidates must be contiguous int64 tensors [n, 3 m] on the scores' device");
  }
  if (has_disps)
    TORCH_CHECK(disps->is_cuda() && disps->scalar_type() == at::kFloat && disps->dim() == 3 && disps->size(0) == n && disps->device() == scores.device(),
                "select: disps must be a float32 tensor [n, H, W] on the scores' device");
  c10::DeviceGuard guard(scores.device());
  const auto fo = scores.options().memory_format(c10::nullopt), lo = fo.dtype(at::kLong);
  Tensor x = at::empty({n, m}, lo), y = at::empty({n, m}, lo), index = at::empty({n * m}, lo), xy = at::empty({n, m, 2}, fo), sc = at::empty({n, m}, fo);
  Tensor patches = at::empty({n * m, 3, P, P}, fo), counts = at::empty({mode == DEVO_SELECT_NMS ? n : 0}, fo.dtype(at::kInt));
  check(devo_patch_select(scores.data_ptr<float>(), scores.stride(0), scores.stride(1), scores.stride(2), (int)n, (int)h, (int)w, (int)m, (int)mode, grid ? 1 : 0, (int)k,
                          pad ? 1 : 0, mode == DEVO_SELECT_MULTI ? noise->data_ptr<float>() : nullptr, mode == DEVO_SELECT_3XRANDOM ? i64p(*cand_x) : nullptr,
                          mode == DEVO_SELECT_3XRANDOM ? i64p(*cand_y) : nullptr, (int)offset, clamp ? 1 : 0, (int)cx0, (int)cx1, (int)cy0, (int)cy1,
                          has_disps ? disps->data_ptr<float>() : nullptr, has_disps ? disps->stride(0) : 0, has_disps ? disps->stride(1) : 0, has_disps ? disps->stride(2) : 0,
                          has_disps ? (int)disps->size(1) : 0, has_disps ? (int)disps->size(2) : 0, (int)P, x.data_ptr<int64_t>(), y.data_ptr<int64_t>(), xy.data_ptr<float>(),
                          sc.data_ptr<float>(), patches.data_ptr<float>(), index.data_ptr<int64_t>(), mode == DEVO_SELECT_NMS ? counts.data_ptr<int>() : nullptr,
                          stream_of(scores)), "select");
  return {x, y, xy, sc, patches, index, counts};
}

// ------------------------------------------------------------------------------------------------ trajectory evaluation (devo_amd/evaluation.py; csrc/traj_eval.hip)
// devo_traj_eval on tensors: packed poses [total, 7] (fp32 or fp64, both alike), stamps [total] (int64 or fp64, both alike), offsets i64 [B + 1] on
// the GPU.  The outputs and the workspace are allocated here; the Python module packs, checks the offsets and reads the status.
// -> {stats f64 [B, DEVO_TRAJ_EVAL_COLS], transform f64 [B, 8], status i32 [B], errors f64 [total_est] or [0], matched i32 [total_est] or [0]}
TensorList traj_eval(const Tensor& est, const Tensor& est_stamps, const Tensor& est_off, const Tensor& gt, const Tensor& gt_stamps, const Tensor& gt_off, int64_t assoc,
                     int64_t align, double max_diff, int64_t rpe_delta, bool want_errors, bool want_matched) {
  require_gpu(est, est_stamps, est_off, gt, gt_stamps, gt_off);
  for (const Tensor* t : {&est, &gt})
    TORCH_CHECK(t->dim() == 2 && t->size(1) == 7 && t->is_contiguous() && (t->scalar_type() == at::kFloat || t->scalar_type() == at::kDouble) &&
                t->scalar_type() == est.scalar_type() && t->device() == est.device(), "evaluation: poses must be contiguous [N, 7] tensors of one dtype (float32 or float64) on one GPU");
  for (const Tensor* t : {&est_stamps, &gt_stamps})
    TORCH_CHECK(t->dim() == 1 && t->is_contiguous() && (t->scalar_type() == at::kLong || t->scalar_type() == at::kDouble) && t->scalar_type() == est_stamps.scalar_type() &&
                t->device() == est.device(), "evaluation: stamps must be contiguous [N] tensors of one dtype (int64 or float64) on the poses' GPU");
  TORCH_CHECK(est_stamps.numel() == est.size(0) && gt_stamps.numel() == gt.size(0), "evaluation: one stamp per pose expected");
  pg_check_idx("evaluation", est_off);
  pg_check_idx("evaluation", gt_off);
  const int64_t B = est_off.numel() - 1;
  TORCH_CHECK(B >= 1 && gt_off.numel() == B + 1 && B <= INT32_MAX && est_off.device() == est.device() && gt_off.device() == est.device(),
              "evaluation: offsets must be two int64 [B + 1] tensors on the poses' GPU");
  TORCH_CHECK(rpe_delta >= 0 && rpe_delta <= INT32_MAX, "evaluation: rpe_delta ", rpe_delta);
  c10::DeviceGuard guard(est.device());
  const auto fo = est.options().dtype(at::kDouble).memory_format(c10::nullopt);
  const int64_t total_est = est.size(0);
  Tensor stats = at::empty({B, DEVO_TRAJ_EVAL_COLS}, fo), transform = at::empty({B, 8}, fo), status = at::empty({B}, fo.dtype(at::kInt));
  Tensor errors = at::empty({want_errors ? total_est : 0}, fo), matched = at::empty({want_matched ? total_est : 0}, fo.dtype(at::kInt));
  const size_t bytes = devo_traj_eval_workspace_bytes(total_est, (int)assoc);
  Tensor ws = at::empty({(int64_t)bytes}, fo.dtype(at::kByte));
  check(devo_traj_eval(est.data_ptr(), est_stamps.data_ptr(), i64p(est_off), total_est, gt.data_ptr(), gt_stamps.data_ptr(), i64p(gt_off), gt.size(0), (int)B,
                       dtype_code(est), est_stamps.scalar_type() == at::kDouble ? 1 : 0, (int)assoc, (int)align, max_diff, (int)rpe_delta, stats.data_ptr<double>(),
                       transform.data_ptr<double>(), status.data_ptr<int>(), want_errors ? errors.data_ptr<double>() : nullptr,
                       want_matched ? matched.data_ptr<int>() : nullptr, ws.data_ptr(), bytes, stream_of(est)), "evaluation");
  return {stats, transform, status, errors, matched};
}

// devo_traj_rel_eval on the same tensors (csrc/traj_rel.hip): deltas are host numbers, scale_mode DEVO_TRAJ_REL_SCALE_* with `scale` (VALUE) or
// `scales` f64 [B] on the GPU (PER_PAIR).
// -> {stats f64 [B, D, DEVO_TRAJ_REL_COLS], status i32 [B, D], errors f64 [D, total_est, 2] or [0], ends i32 [D, total_est] or [0]}
TensorList traj_rel_eval(const Tensor& est, const Tensor& est_stamps, const Tensor& est_off, const Tensor& gt, const Tensor& gt_stamps, const Tensor& gt_off, int64_t assoc,
                         double max_diff, std::vector<double> deltas, int64_t unit, bool relative, int64_t along, int64_t end, int64_t scale_mode, double scale,
                         const c10::optional<Tensor>& scales, bool want_errors) {
  require_gpu(est, est_stamps, est_off, gt, gt_stamps, gt_off);
  for (const Tensor* t : {&est, &gt})
    TORCH_CHECK(t->dim() == 2 && t->size(1) == 7 && t->is_contiguous() && (t->scalar_type() == at::kFloat || t->scalar_type() == at::kDouble) &&
                t->scalar_type() == est.scalar_type() && t->device() == est.device(), "evaluation: poses must be contiguous [N, 7] tensors of one dtype (float32 or float64) on one GPU");
  for (const Tensor* t : {&est_stamps, &gt_stamps})
    TORCH_CHECK(t->dim() == 1 && t->is_contiguous() && (t->scalar_type() == at::kLong || t->scalar_type() == at::kDouble) && t->scalar_type() == est_stamps.scalar_type() &&
                t->device() == est.device(), "evaluation: stamps must be contiguous [N] tensors of one dtype (int64 or float64) on the poses' GPU");
  TORCH_CHECK(est_stamps.numel() == est.size(0) && gt_stamps.numel() == gt.size(0), "evaluation: one stamp per pose expected");
  pg_check_idx("evaluation", est_off);
  pg_check_idx("evaluation", gt_off);
  const int64_t B = est_off.numel() - 1, D = (int64_t)deltas.size();
  TORCH_CHECK(B >= 1 && gt_off.numel() == B + 1 && B <= INT32_MAX / DEVO_TRAJ_REL_MAX_DELTAS && est_off.device() == est.device() && gt_off.device() == est.device(),
              "evaluation: offsets must be two int64 [B + 1] tensors on the poses' GPU");
  TORCH_CHECK(D >= 1 && D <= DEVO_TRAJ_REL_MAX_DELTAS, "evaluation: 1 .. ", DEVO_TRAJ_REL_MAX_DELTAS, " deltas expected (", D, ")");
  const bool per_pair = scale_mode == DEVO_TRAJ_REL_SCALE_PER_PAIR;
  TORCH_CHECK(!per_pair || (scales.has_value() && scales->defined() && scales->is_cuda() && scales->device() == est.device() && scales->scalar_type() == at::kDouble &&
                            scales->dim() == 1 && scales->numel() == B && scales->is_contiguous()),
              "evaluation: one scale per pair expected, a contiguous float64 [B] tensor on the poses' GPU");
  c10::DeviceGuard guard(est.device());
  const auto fo = est.options().dtype(at::kDouble).memory_format(c10::nullopt);
  const int64_t total_est = est.size(0);
  Tensor stats = at::empty({B, D, DEVO_TRAJ_REL_COLS}, fo), status = at::empty({B, D}, fo.dtype(at::kInt));
  Tensor errors = want_errors ? at::empty({D, total_est, 2}, fo) : at::empty({0}, fo);
  Tensor ends = want_errors ? at::empty({D, total_est}, fo.dtype(at::kInt)) : at::empty({0}, fo.dtype(at::kInt));
  const size_t bytes = devo_traj_rel_workspace_bytes(total_est, (int)assoc, (int)B, (int)D);
  Tensor ws = at::empty({(int64_t)bytes}, fo.dtype(at::kByte));
  check(devo_traj_rel_eval(est.data_ptr(), est_stamps.data_ptr(), i64p(est_off), total_est, gt.data_ptr(), gt_stamps.data_ptr(), i64p(gt_off), gt.size(0), (int)B,
                           dtype_code(est), est_stamps.scalar_type() == at::kDouble ? 1 : 0, (int)assoc, max_diff, deltas.data(), (int)D, (int)unit, relative ? 1 : 0,
                           (int)along, (int)end, (int)scale_mode, scale, per_pair ? scales->data_ptr<double>() : nullptr, stats.data_ptr<double>(),
                           status.data_ptr<int>(), want_errors ? errors.data_ptr<double>() : nullptr, want_errors ? ends.data_ptr<int>() : nullptr, ws.data_ptr(),
                           bytes, stream_of(est)), "evaluation");
  return {stats, status, errors, ends};
}

// ------------------------------------------------------------------------------------------------ camera models (devo_amd/camera.py; csrc/camera.hip)
// devo_camera_undistort_points / devo_camera_distort_points on tensors: points [n, 2] (fp32 or fp64) or none (the H x W pixel grid, on GPU
// `device`); K (4), dist, R (9 or empty), K_new (4 or empty) are host numbers.  -> {out [n, 2] or [H, W, 2], invalid i32 [1] or [0]}
TensorList camera_points(const c10::optional<Tensor>& points, int64_t H, int64_t W, int64_t device, int64_t model, std::vector<double> K, std::vector<double> dist,
                         std::vector<double> R, std::vector<double> K_new, bool distort, bool out_f64, bool count) {
  const bool grid = !(points.has_value() && points->defined());
  TORCH_CHECK(K.size() == 4 && (R.empty() || R.size() == 9) && (K_new.empty() || K_new.size() == 4), "camera: K and K_new have 4 entries, R has 9");
  TORCH_CHECK(H >= 0 && W >= 0 && H <= INT32_MAX && W <= INT32_MAX && dist.size() <= 5, "camera: sizes");
  int64_t n;
  at::TensorOptions o;
  if (grid) {
    n = H * W;
    o = at::TensorOptions().device(c10::Device(c10::kCUDA, (c10::DeviceIndex)device));
  } else {
    require_gpu(*points);
    TORCH_CHECK(points->dim() == 2 && points->size(1) == 2 && points->is_contiguous() && (points->scalar_type() == at::kFloat || points->scalar_type() == at::kDouble),
                "camera: points must be a contiguous [n, 2] tensor of float32 or float64");
    n = points->size(0);
    o = points->options().memory_format(c10::nullopt);
  }
  c10::DeviceGuard guard(o.device());
  Tensor out = grid ? at::empty({H, W, 2}, o.dtype(out_f64 ? at::kDouble : at::kFloat)) : at::empty({n, 2}, o.dtype(out_f64 ? at::kDouble : at::kFloat));
  Tensor invalid = count ? at::zeros({1}, o.dtype(at::kInt)) : at::empty({0}, o.dtype(at::kInt));
  auto* fn = distort ? &devo_camera_distort_points : &devo_camera_undistort_points;
  check(fn(grid ? nullptr : points->data_ptr(), n, (int)H, (int)W, grid ? DEVO_F64 : dtype_code(*points), (int)model, K.data(), dist.empty() ? nullptr : dist.data(),
           (int)dist.size(), R.empty() ? nullptr : R.data(), K_new.empty() ? nullptr : K_new.data(), out.data_ptr(), out_f64 ? DEVO_F64 : DEVO_F32,
           count ? invalid.data_ptr<int>() : nullptr, stream_of(out)), distort ? "camera.distort_points" : "camera.undistort_points");
  return {out, invalid};
}

// devo_image_remap on tensors: images [B, H, W, C] (uint8 or float32, contiguous), map float32 [Ho, Wo, 2]; `out` [B, Ho, Wo, C] is allocated when absent
Tensor image_remap(const Tensor& images, const Tensor& map, const c10::optional<Tensor>& out_, bool out_u8) {
  require_gpu(images, map);
  TORCH_CHECK(images.dim() == 4 && images.is_contiguous() && (images.scalar_type() == at::kByte || images.scalar_type() == at::kFloat) && images.numel() > 0,
              "camera.remap: images must be a contiguous [B, H, W, C] tensor of uint8 or float32");
  TORCH_CHECK(map.dim() == 3 && map.size(2) == 2 && map.is_contiguous() && map.scalar_type() == at::kFloat && map.device() == images.device() && map.numel() > 0,
              "camera.remap: map must be a contiguous float32 [Ho, Wo, 2] tensor on the images' GPU");
  const int64_t B = images.size(0), H = images.size(1), W = images.size(2), C = images.size(3), Ho = map.size(0), Wo = map.size(1);
  TORCH_CHECK(B <= INT32_MAX && H <= INT32_MAX && W <= INT32_MAX && Ho <= INT32_MAX && Wo <= INT32_MAX, "camera.remap: sizes");
  c10::DeviceGuard guard(images.device());
  const auto dt = out_u8 ? at::kByte : at::kFloat;
  Tensor out;
  if (out_.has_value() && out_->defined()) {
    out = *out_;
    TORCH_CHECK(out.is_cuda() && out.device() == images.device() && out.scalar_type() == dt && out.is_contiguous() && out.sizes() == at::IntArrayRef({B, Ho, Wo, C}),
                "camera.remap: out must be a contiguous [B, Ho, Wo, C] tensor of the output dtype on the images' GPU");
  } else {
    out = at::empty({B, Ho, Wo, C}, images.options().dtype(dt).memory_format(c10::nullopt));
  }
  check(devo_image_remap(images.data_ptr(), (int)B, (int)H, (int)W, (int)C, images.scalar_type() == at::kByte ? (int)DEVO_U8 : (int)DEVO_F32, map.data_ptr<float>(), (int)Ho, (int)Wo,
                         out.data_ptr(), out_u8 ? (int)DEVO_U8 : (int)DEVO_F32, stream_of(images)), "camera.remap");
  return out;
}

// ------------------------------------------------------------------------------------------------ event simulation (devo_amd/simulate.py; csrc/esim.hip)
// Thin forms of the devo_esim_* entry points: prev [H, W] and frames [T, H, W] fp32, prev_stamp [1] and stamps [T] int64, ref [H, W] fp64,
// last_t [H, W] int64, all contiguous on one GPU.  The Python module owns the state, reads the status word, scans the counts and sorts the keys.
void esim_inputs(const char* what, const Tensor& prev, const Tensor& frames, const Tensor& prev_stamp, const Tensor& stamps, const Tensor& ref, const Tensor& last_t) {
  require_gpu(prev, frames, prev_stamp, stamps, ref, last_t);
  TORCH_CHECK(frames.dim() == 3 && frames.size(0) >= 1 && frames.size(0) <= INT32_MAX && frames.size(1) <= INT32_MAX && frames.size(2) <= INT32_MAX &&
              frames.scalar_type() == at::kFloat && frames.is_contiguous(), what, ": frames must be a contiguous float32 [T, H, W] tensor");
  const int64_t T = frames.size(0), HW = frames.size(1) * frames.size(2);
  TORCH_CHECK(prev.scalar_type() == at::kFloat && prev.numel() == HW && prev.is_contiguous() && ref.scalar_type() == at::kDouble && ref.numel() == HW && ref.is_contiguous() &&
              last_t.scalar_type() == at::kLong && last_t.numel() == HW && last_t.is_contiguous(), what, ": prev float32, ref float64 and last_t int64 must be contiguous [H, W]");
  TORCH_CHECK(prev_stamp.scalar_type() == at::kLong && prev_stamp.numel() == 1 && stamps.scalar_type() == at::kLong && stamps.numel() == T && stamps.is_contiguous(), what,
              ": prev_stamp [1] and stamps [T] must be int64");
  for (const Tensor* t : {&prev, &prev_stamp, &stamps, &ref, &last_t}) TORCH_CHECK(t->device() == frames.device(), what, ": tensors on different devices");
}

TensorList esim_count(const Tensor& prev, const Tensor& frames, const Tensor& prev_stamp, const Tensor& stamps, const Tensor& ref, const Tensor& last_t, double c_neg,
                      double c_pos, int64_t refractory_ns) {
  esim_inputs("simulate.count", prev, frames, prev_stamp, stamps, ref, last_t);
  c10::DeviceGuard guard(frames.device());
  const auto lo = frames.options().dtype(at::kLong).memory_format(c10::nullopt);
  Tensor counts = at::empty({frames.size(1) * frames.size(2)}, lo), status_span = at::empty({2}, lo);
  check(devo_esim_count(prev.data_ptr<float>(), frames.data_ptr<float>(), prev_stamp.data_ptr<int64_t>(), stamps.data_ptr<int64_t>(), (int)frames.size(0), (int)frames.size(1),
                        (int)frames.size(2), ref.data_ptr<double>(), last_t.data_ptr<int64_t>(), c_neg, c_pos, refractory_ns, counts.data_ptr<int64_t>(),
                        status_span.data_ptr<int64_t>(), stream_of(frames)), "simulate.count");
  return {counts, status_span};
}

// -> {keys [total] (unsorted), ref_out, last_t_out}
TensorList esim_emit(const Tensor& prev, const Tensor& frames, const Tensor& prev_stamp, const Tensor& stamps, const Tensor& ref, const Tensor& last_t, double c_neg,
                     double c_pos, int64_t refractory_ns, const Tensor& offsets, int64_t total) {
  esim_inputs("simulate.emit", prev, frames, prev_stamp, stamps, ref, last_t);
  TORCH_CHECK(offsets.is_cuda() && offsets.device() == frames.device() && offsets.scalar_type() == at::kLong && offsets.numel() == ref.numel() && offsets.is_contiguous() && total >= 0,
              "simulate.emit: offsets must be a contiguous int64 [H * W] tensor on the frames' GPU");
  c10::DeviceGuard guard(frames.device());
  Tensor keys = at::empty({total}, offsets.options().memory_format(c10::nullopt)), ref_out = at::empty_like(ref), last_out = at::empty_like(last_t);
  check(devo_esim_emit(prev.data_ptr<float>(), frames.data_ptr<float>(), prev_stamp.data_ptr<int64_t>(), stamps.data_ptr<int64_t>(), (int)frames.size(0), (int)frames.size(1),
                       (int)frames.size(2), ref.data_ptr<double>(), last_t.data_ptr<int64_t>(), c_neg, c_pos, refractory_ns, offsets.data_ptr<int64_t>(), total,
                       total ? keys.data_ptr<int64_t>() : nullptr, ref_out.data_ptr<double>(), last_out.data_ptr<int64_t>(), stream_of(frames)), "simulate.emit");
  return {keys, ref_out, last_out};
}

// the call's keys in ascending order: rocPRIM's keys-only radix sort over the bits a call of `span_ns` can set (devo_esim_sort_keys)
Tensor esim_sort(const Tensor& keys, int64_t H, int64_t W, int64_t span_ns) {
  require_gpu(keys);
  TORCH_CHECK(keys.dim() == 1 && keys.scalar_type() == at::kLong && keys.is_contiguous() && H >= 1 && W >= 1 && H <= INT32_MAX && W <= INT32_MAX, "simulate.sort: keys int64 [N]");
  c10::DeviceGuard guard(keys.device());
  const int64_t n = keys.numel();
  Tensor sorted = at::empty_like(keys);
  if (n == 0) return sorted;
  const size_t bytes = devo_esim_sort_workspace_bytes(n, (int)H, (int)W, span_ns);
  Tensor ws = at::empty({(int64_t)bytes}, keys.options().dtype(at::kByte).memory_format(c10::nullopt));
  check(devo_esim_sort_keys(keys.data_ptr<int64_t>(), sorted.data_ptr<int64_t>(), n, (int)H, (int)W, span_ns, bytes ? ws.data_ptr() : nullptr, bytes, stream_of(keys)),
        "simulate.sort");
  return sorted;
}

// sorted keys -> {x int16, y int16, t int64, p int8}
TensorList esim_decode(const Tensor& keys, int64_t H, int64_t W, const Tensor& first_stamp) {
  require_gpu(keys, first_stamp);
  TORCH_CHECK(keys.dim() == 1 && keys.scalar_type() == at::kLong && keys.is_contiguous() && first_stamp.scalar_type() == at::kLong && first_stamp.numel() == 1 &&
              first_stamp.device() == keys.device() && H >= 1 && W >= 1 && H <= INT32_MAX && W <= INT32_MAX, "simulate.decode: keys int64 [N], first_stamp int64 [1] on one GPU");
  c10::DeviceGuard guard(keys.device());
  const int64_t n = keys.numel();
  const auto o = keys.options().memory_format(c10::nullopt);
  Tensor x = at::empty({n}, o.dtype(at::kShort)), y = at::empty({n}, o.dtype(at::kShort)), t = at::empty({n}, o), p = at::empty({n}, o.dtype(at::kChar));
  check(devo_esim_decode(n ? keys.data_ptr<int64_t>() : nullptr, n, (int)H, (int)W, first_stamp.data_ptr<int64_t>(), n ? x.data_ptr<int16_t>() : nullptr,
                         n ? y.data_ptr<int16_t>() : nullptr, n ? t.data_ptr<int64_t>() : nullptr, n ? (signed char*)p.data_ptr<int8_t>() : nullptr, stream_of(keys)),
        "simulate.decode");
  return {x, y, t, p};
}

Tensor log_intensity(const Tensor& images, const Tensor& table) {
  require_gpu(images, table);
  TORCH_CHECK(images.scalar_type() == at::kByte && images.is_contiguous() && table.scalar_type() == at::kFloat && table.numel() == 256 && table.is_contiguous() &&
              table.device() == images.device(), "simulate.log_intensity: images contiguous uint8, table float32 [256] on the images' GPU");
  c10::DeviceGuard guard(images.device());
  Tensor out = at::empty(images.sizes(), images.options().dtype(at::kFloat).memory_format(c10::nullopt));
  const int64_t n = images.numel();
  check(devo_log_intensity(n ? images.data_ptr<uint8_t>() : nullptr, n, table.data_ptr<float>(), out.data_ptr<float>(), stream_of(images)), "simulate.log_intensity");
  return out;
}

// ------------------------------------------------------------------------------------------------ optimiser step (devo_amd/optim.py; csrc/optim.hip)
// Thin forms of the devo_optim_* entry points.  The Python module owns the tables, the moment buffers and every refusal that names a parameter;
// the gradient addresses of a step arrive as integers (0: no gradient) and leave as kernel arguments.
// sizes -> {chunk table int32 [chunks, 4], moment offsets int64 [n], elements of one moment buffer int64 [1]}, HOST tensors
TensorList optim_plan(std::vector<int64_t> numel) {
  TORCH_CHECK(!numel.empty() && numel.size() <= (size_t)DEVO_OPTIM_MAX_TENSORS, "optim.plan: ", numel.size(), " tensors (1 .. ", DEVO_OPTIM_MAX_TENSORS, ")");
  const int n = (int)numel.size();
  const int64_t chunks = devo_optim_chunks(numel.data(), n), elems = devo_optim_moment_elems(numel.data(), n);
  TORCH_CHECK(chunks > 0 && elems > 0, "optim.plan: ", devo_last_error());
  Tensor table = at::empty({chunks, 4}, at::TensorOptions().dtype(at::kInt)), offsets = at::empty({(int64_t)n}, at::TensorOptions().dtype(at::kLong));
  check(devo_optim_plan(numel.data(), n, table.data_ptr<int32_t>(), offsets.data_ptr<int64_t>()), "optim.plan");
  return {table, offsets, at::full({1}, elems, at::TensorOptions().dtype(at::kLong))};
}

void optim_step(const Tensor& chunk_table, const Tensor& tensor_table, std::vector<int64_t> grad_addrs, std::vector<int64_t> numel, Tensor& exp_avg, Tensor& exp_avg_sq,
                double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double bc1, double bc2, bool skip_nonfinite, Tensor& counters,
                Tensor& grad_norm, Tensor& workspace) {
  require_gpu(chunk_table, tensor_table, exp_avg, exp_avg_sq, counters, grad_norm, workspace);
  const int64_t n = (int64_t)numel.size();
  TORCH_CHECK(n >= 1 && n <= DEVO_OPTIM_MAX_TENSORS && (int64_t)grad_addrs.size() == n, "optim.step: ", n, " sizes and ", grad_addrs.size(), " gradient addresses (1 .. ",
              DEVO_OPTIM_MAX_TENSORS, " of each)");
  const int64_t chunks = devo_optim_chunks(numel.data(), (int)n), elems = devo_optim_moment_elems(numel.data(), (int)n);
  TORCH_CHECK(chunks > 0, "optim.step: ", devo_last_error());
  TORCH_CHECK(chunk_table.scalar_type() == at::kInt && chunk_table.is_contiguous() && chunk_table.dim() == 2 && chunk_table.size(0) == chunks && chunk_table.size(1) == 4,
              "optim.step: chunk_table must be the plan's contiguous int32 [", chunks, ", 4]");
  TORCH_CHECK(tensor_table.scalar_type() == at::kLong && tensor_table.is_contiguous() && tensor_table.dim() == 2 && tensor_table.size(0) == n && tensor_table.size(1) == 2,
              "optim.step: tensor_table must be a contiguous int64 [", n, ", 2]");
  TORCH_CHECK(exp_avg.scalar_type() == at::kFloat && exp_avg.is_contiguous() && exp_avg.numel() == elems && exp_avg_sq.scalar_type() == at::kFloat &&
              exp_avg_sq.is_contiguous() && exp_avg_sq.numel() == elems, "optim.step: the moment buffers must be contiguous float32 [", elems, "]");
  TORCH_CHECK(counters.scalar_type() == at::kLong && counters.is_contiguous() && counters.numel() == 2 && grad_norm.scalar_type() == at::kDouble && grad_norm.numel() == 1 &&
              workspace.scalar_type() == at::kByte && workspace.is_contiguous(), "optim.step: counters int64 [2], grad_norm float64 [1], workspace uint8");
  for (const Tensor* t : {&tensor_table, (const Tensor*)&exp_avg, (const Tensor*)&exp_avg_sq, (const Tensor*)&counters, (const Tensor*)&grad_norm, (const Tensor*)&workspace})
    TORCH_CHECK(t->device() == chunk_table.device(), "optim.step: tensors on different devices");
  c10::DeviceGuard guard(chunk_table.device());
  std::vector<const void*> grads((size_t)n);
  for (int64_t i = 0; i < n; ++i) grads[(size_t)i] = (const void*)(intptr_t)grad_addrs[(size_t)i];
  check(devo_optim_step(chunk_table.data_ptr<int32_t>(), chunks, tensor_table.data_ptr<int64_t>(), grads.data(), numel.data(), (int)n, exp_avg.data_ptr<float>(),
                        exp_avg_sq.data_ptr<float>(), lr, beta1, beta2, eps, weight_decay, max_norm, bc1, bc2, skip_nonfinite ? 1 : 0, counters.data_ptr<int64_t>(),
                        grad_norm.data_ptr<double>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(chunk_table)), "optim.step");
}

// ------------------------------------------------------------------------------------------------ frame state (devo_amd/frames.py; csrc/frames.hip)
// Thin forms of the devo_frame_* entry points.  `status` is a pinned HOST tensor the kernels write (devo_hip.h); the Python module checks
// shapes, owns the log and the workspace and reads the status.
void fr_begin(Tensor poses, Tensor patches, Tensor intrinsics, Tensor tstamps, int64_t M, int64_t n, Tensor new_patches, Tensor new_intrinsics, int64_t counter, double res,
              int64_t motion_model, double damping, const c10::optional<Tensor>& depth) {
  pg_geometry("frames.begin_frame", poses, patches, intrinsics);
  pg_geometry("frames.begin_frame", new_patches, new_patches, new_intrinsics);
  pg_check_idx("frames.begin_frame", tstamps);
  const bool has = depth.has_value() && depth->defined();
  TORCH_CHECK(!has || (depth->is_cuda() && depth->scalar_type() == at::kFloat && depth->is_contiguous()), "frames.begin_frame: depth must be a contiguous float32 tensor on the GPU");
  c10::DeviceGuard guard(poses.device());
  check(devo_frame_begin(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), tstamps.data_ptr<int64_t>(), (int)(poses.numel() / 7), (int)M,
                         (int)patches.size(-1), (int)n, new_patches.data_ptr<float>(), new_intrinsics.data_ptr<float>(), counter, (float)res, (int)motion_model, (float)damping,
                         has ? depth->data_ptr<float>() : nullptr, stream_of(poses)), "frames.begin_frame");
}

void fr_point_cloud(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ix, int64_t M, int64_t m, int64_t start_frame, Tensor out) {
  pg_geometry("frames.point_cloud", poses, patches, intrinsics);
  pg_check_idx("frames.point_cloud", ix);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() >= 3 * m, "frames.point_cloud: out must be a contiguous float32 tensor of at least m rows");
  c10::DeviceGuard guard(poses.device());
  const int64_t P = patches.size(-1);
  check(devo_frame_point_cloud(poses.data_ptr<float>(), patches.data_ptr<float>(), intrinsics.data_ptr<float>(), i64p(ix), (int)(poses.numel() / 7),
                               (int)(patches.numel() / (3 * P * P)), ix.numel(), (int)P, (int)M, (int)m, (int)start_frame, out.data_ptr<float>(), stream_of(poses)),
        "frames.point_cloud");
}

void fr_check_log(const char* what, const Tensor& parent, const Tensor& rel, const Tensor& status) {
  pg_check_idx(what, parent);
  TORCH_CHECK(rel.is_cuda() && rel.scalar_type() == at::kFloat && rel.is_contiguous() && rel.numel() == 7 * parent.numel(), what, ": rel must be float32 [capacity, 7] on the GPU");
  TORCH_CHECK(!status.is_cuda() && status.is_pinned() && status.scalar_type() == at::kInt && status.numel() >= 1, what, ": the status word must be a pinned int32 host tensor");
}

void fr_record_removed(Tensor poses, Tensor tstamps, int64_t k, Tensor parent, Tensor rel, Tensor status) {
  pg_geometry("frames.record_removed", poses, poses, poses);
  pg_check_idx("frames.record_removed", tstamps);
  fr_check_log("frames.record_removed", parent, rel, status);
  c10::DeviceGuard guard(parent.device());
  check(devo_frame_record_removed(poses.data_ptr<float>(), i64p(tstamps), (int)std::min<int64_t>(poses.numel() / 7, tstamps.numel()), (int)k, parent.data_ptr<int64_t>(),
                                  rel.data_ptr<float>(), (int)parent.numel(), status.data_ptr<int>(), stream_of(parent)), "frames.record_removed");
}

void fr_record_skipped(int64_t t, int64_t t0, Tensor parent, Tensor rel, Tensor status) {
  fr_check_log("frames.record_skipped", parent, rel, status);
  c10::DeviceGuard guard(parent.device());
  check(devo_frame_record_skipped(t, t0, parent.data_ptr<int64_t>(), rel.data_ptr<float>(), (int)parent.numel(), status.data_ptr<int>(), stream_of(parent)),
        "frames.record_skipped");
}

void fr_complete(Tensor poses, Tensor tstamps, int64_t n, int64_t counter, Tensor parent, Tensor rel, Tensor out, Tensor ws, Tensor status) {
  pg_geometry("frames.complete", poses, poses, poses);
  pg_check_idx("frames.complete", tstamps);
  fr_check_log("frames.complete", parent, rel, status);
  TORCH_CHECK(n <= poses.numel() / 7 && n <= tstamps.numel(), "frames.complete: n exceeds the frame buffers");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() >= 7 * counter && ws.is_cuda() && ws.is_contiguous(),
              "frames.complete: out must be float32 [counter, 7] on the GPU");
  c10::DeviceGuard guard(parent.device());
  check(devo_frame_complete(poses.data_ptr<float>(), i64p(tstamps), (int)n, (int)counter, i64p(parent), rel.data_ptr<float>(), (int)parent.numel(), out.data_ptr<float>(),
                            ws.data_ptr(), (size_t)(ws.numel() * ws.element_size()), status.data_ptr<int>(), stream_of(parent)), "frames.complete");
}

// devo_odom_input / devo_odom_probe_median (csrc/frame_input.hip).  `record` (4 doubles) and the median's `out` may be pinned HOST tensors.
void fr_check_host_visible(const char* what, const Tensor& t, at::ScalarType dt, int64_t n) {
  TORCH_CHECK((t.is_cuda() || t.is_pinned()) && t.scalar_type() == dt && t.is_contiguous() && t.numel() >= n, what, ": expected a contiguous GPU or pinned host tensor of at least ", n,
              " elements");
}

void fr_input(Tensor vox, int64_t norm, Tensor out, Tensor ws, Tensor record) {
  require_gpu(vox, out, ws);
  TORCH_CHECK(vox.dim() == 3 && vox.is_contiguous() && (vox.scalar_type() == at::kFloat || vox.scalar_type() == at::kHalf), "frames.frame_input: the voxel grid must be a contiguous fp32 or fp16 [bins, H, W] tensor");
  const int64_t W = vox.size(2), Wout = W == DEVO_INPUT_CROP_WIDTH ? W - 2 : W;
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() == vox.size(0) * vox.size(1) * Wout, "frames.frame_input: out must be a contiguous float32 tensor of bins x H x ", Wout, " elements");
  fr_check_host_visible("frames.frame_input (record)", record, at::kDouble, 4);
  c10::DeviceGuard guard(vox.device());
  check(devo_odom_input(vox.data_ptr(), dtype_code(vox), (int)vox.size(0), (int)vox.size(1), (int)W, (int)norm, out.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(),
                        record.data_ptr<double>(), stream_of(vox)), "frames.frame_input");
}

void fr_probe_median(Tensor delta, Tensor out) {
  require_gpu(delta);
  TORCH_CHECK(delta.is_contiguous() && delta.numel() % 2 == 0 && (delta.scalar_type() == at::kFloat || delta.scalar_type() == at::kHalf), "frames.probe_median: delta must be a contiguous fp32 or fp16 [1, M, 2] tensor");
  fr_check_host_visible("frames.probe_median (out)", out, at::kFloat, 1);
  c10::DeviceGuard guard(delta.device());
  check(devo_odom_probe_median(delta.data_ptr(), dtype_code(delta), (int)(delta.numel() / 2), out.data_ptr<float>(), stream_of(delta)), "frames.probe_median");
}

// ------------------------------------------------------------------------------------------------ training loss (devo_amd/losses.py; csrc/loss.hip)
// Thin forms of devo_loss_forward / devo_loss_backward: the outputs and the state are allocated here, nothing else happens on the host.
void loss_check(const char* what, const Tensor& t, at::ScalarType dt) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous(), what, ": contiguous GPU tensors of one floating dtype (fp32 or fp64)");
}
const void* opt_ptr(const c10::optional<Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr() : nullptr; }

// -> {loss T [1], stats f32 [DEVO_LOSS_STATS], state u8}
TensorList loss_forward(const Tensor& x, const Tensor& y, const Tensor& v, const Tensor& Gs, const Tensor& Ps, const c10::optional<Tensor>& scores,
                        const c10::optional<Tensor>& v_full, const c10::optional<Tensor>& x_full, const c10::optional<Tensor>& y_full,
                        const c10::optional<Tensor>& ba_weights, const c10::optional<Tensor>& kk, bool deterministic, double flow_weight, double pose_weight,
                        double scores_weight, bool use_pose) {
  const at::ScalarType dt = x.scalar_type();
  for (const Tensor* t : {&x, &y, &v, &Gs, &Ps}) loss_check("losses.forward", *t, dt);
  const bool has = scores.has_value() && scores->defined();
  int64_t Ef = 0, n_patches = 0;
  if (has) {
    TORCH_CHECK(v_full && x_full && y_full && ba_weights && kk, "losses.forward: the scorer term needs v_full, x_full, y_full, ba_weights and kk");
    for (const Tensor* t : {&*scores, &*v_full, &*x_full, &*y_full, &*ba_weights}) loss_check("losses.forward", *t, dt);
    pg_check_idx("losses.forward", *kk);
    Ef = kk->numel(); n_patches = scores->numel();
    TORCH_CHECK(v_full->numel() == Ef && ba_weights->numel() == 2 * Ef && x_full->numel() == y_full->numel(), "losses.forward: the scorer term's tensors disagree in size");
  }
  TORCH_CHECK(x.dim() >= 3 && x.size(-1) == 2 && x.size(-2) == x.size(-3), "losses.forward: coords must be [.., P, P, 2]");
  const int64_t P = x.size(-2), Ec = v.numel(), n = Gs.numel() / 7;
  TORCH_CHECK(x.numel() == Ec * P * P * 2 && y.numel() == x.numel() && Ps.numel() == Gs.numel(), "losses.forward: sizes disagree");
  TORCH_CHECK(!has || x_full->numel() == Ef * P * P * 2, "losses.forward: coords_full must be [Ef, P, P, 2]");
  c10::DeviceGuard guard(x.device());
  const int code = dtype_code(x);
  const size_t bytes = devo_loss_state_bytes((int)Ec, (int)n, (int)Ef, (int)n_patches, code);
  Tensor loss = at::empty({1}, x.options()), stats = at::empty({DEVO_LOSS_STATS}, x.options().dtype(at::kFloat));
  Tensor state = at::empty({(int64_t)bytes}, x.options().dtype(at::kByte));
  check(devo_loss_forward(x.data_ptr(), y.data_ptr(), v.data_ptr(), (int)Ec, (int)P, Gs.data_ptr(), Ps.data_ptr(), (int)n, opt_ptr(scores), (int)n_patches, opt_ptr(v_full),
                          opt_ptr(x_full), opt_ptr(y_full), opt_ptr(ba_weights), has ? i64p(*kk) : nullptr, (int)Ef, deterministic ? 1 : 0, flow_weight, pose_weight,
                          scores_weight, use_pose ? 1 : 0, loss.data_ptr(), stats.data_ptr<float>(), state.data_ptr(), bytes, code, stream_of(x)), "losses.forward");
  return {loss, stats, state};
}

// -> {g_coords [Ec, P, P, 2], g_Gs [n, 7], g_scores [n_patches]}; an empty tensor where it was not asked for
TensorList loss_backward(const Tensor& g, const Tensor& state, int64_t Ec, int64_t P, int64_t n, int64_t Ef, int64_t n_patches, double flow_weight, double pose_weight,
                         double scores_weight, bool need_coords, bool need_Gs, bool need_scores) {
  TORCH_CHECK(g.is_cuda() && g.numel() == 1 && state.is_cuda() && state.scalar_type() == at::kByte && state.is_contiguous(), "losses.backward: bad arguments");
  c10::DeviceGuard guard(g.device());
  const auto o = g.options();
  Tensor gc = at::empty({need_coords ? Ec : 0, P, P, 2}, o), gG = at::empty({need_Gs ? n : 0, 7}, o), gs = at::empty({need_scores ? n_patches : 0}, o);
  check(devo_loss_backward(g.data_ptr(), state.data_ptr(), (size_t)state.numel(), (int)Ec, (int)P, (int)n, (int)Ef, (int)n_patches, flow_weight, pose_weight, scores_weight,
                           need_coords ? gc.data_ptr() : nullptr, need_Gs ? gG.data_ptr() : nullptr, need_scores ? gs.data_ptr() : nullptr, dtype_code(g), stream_of(g)),
        "losses.backward");
  return {gc, gG, gs};
}

// a kernel wrote the tensor through its raw pointer: what an in-place ATen operation would have done to the version counter (shared by every
// view of the storage), so that the version-keyed caches above and devo_amd.update's graph tables see the write.  No launch.
void bump_version(Tensor t) { t.unsafeGetTensorImpl()->bump_version(); }

void clear_caches() {
  g_levels.clear(); g_patches.clear(); g_cl.clear();
  g_last_plan = LastPlan();
  ba_prep_invalidate();
  { std::lock_guard<std::mutex> g(g_wr_mu); g_writes.clear(); }
  std::lock_guard<std::mutex> g(g_ws_mu);
  g_ws = Tensor(); g_ws_key = WsKey{-1, -1, -1, -1, nullptr};
}

// torch.ops forms of the in-place / list-returning functions
TensorList ba_forward_op(Tensor poses, Tensor patches, Tensor intrinsics, Tensor target, Tensor weight, Tensor lmbda, Tensor ii, Tensor jj, Tensor kk, int64_t t0, int64_t t1,
                         int64_t iterations) {
  return ba_forward(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, iterations, c10::nullopt, c10::nullopt, false);
}

}  // namespace

// torch.ops.devo_hip.* (north_star's wording; the reference itself registers pybind modules only)
TORCH_LIBRARY(devo_hip, m) {
  m.def("corr_forward(Tensor fmap1, Tensor fmap2, Tensor coords, Tensor ii, Tensor jj, int radius) -> Tensor[]");
  m.def("corr_backward(Tensor fmap1, Tensor fmap2, Tensor coords, Tensor ii, Tensor jj, Tensor grad, int radius) -> Tensor[]");
  m.def("patchify_forward(Tensor net, Tensor coords, int radius) -> Tensor[]");
  m.def("patchify_backward(Tensor net, Tensor coords, Tensor gradient, int radius) -> Tensor[]");
  m.def("ba_forward(Tensor(a!) poses, Tensor(b!) patches, Tensor intrinsics, Tensor target, Tensor weight, Tensor lmbda, Tensor ii, Tensor jj, Tensor kk, int t0, int t1, int iterations) -> Tensor[]");
  m.def("ba_neighbors(Tensor ii, Tensor jj) -> Tensor[]");
  m.def("ba_reproject(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ii, Tensor jj, Tensor kk) -> Tensor");
  m.def("se3_exp(int group_id, Tensor a) -> Tensor");
  m.def("se3_log(int group_id, Tensor X) -> Tensor");
  m.def("se3_inv(int group_id, Tensor X) -> Tensor");
  m.def("se3_mul(int group_id, Tensor X, Tensor Y) -> Tensor");
  m.def("se3_adj(int group_id, Tensor X, Tensor a) -> Tensor");
  m.def("se3_adjT(int group_id, Tensor X, Tensor a) -> Tensor");
  m.def("se3_act(int group_id, Tensor X, Tensor p) -> Tensor");
  m.def("se3_act4(int group_id, Tensor X, Tensor p) -> Tensor");
  m.def("se3_projector(int group_id, Tensor X) -> Tensor");
  m.def("loss_forward(Tensor x, Tensor y, Tensor v, Tensor Gs, Tensor Ps, Tensor? scores, Tensor? v_full, Tensor? x_full, Tensor? y_full, Tensor? ba_weights, Tensor? kk, "
        "bool deterministic, float flow_weight, float pose_weight, float scores_weight, bool use_pose) -> Tensor[]");
  m.def("loss_backward(Tensor g, Tensor state, int Ec, int P, int n, int Ef, int n_patches, float flow_weight, float pose_weight, float scores_weight, bool need_coords, "
        "bool need_Gs, bool need_scores) -> Tensor[]");
  m.def("frame_graph_disps(Tensor depths) -> Tensor");
  m.def("frame_graph_distances(Tensor poses, Tensor disps, Tensor intrinsics, float scale) -> Tensor");
  m.def("frame_graph_lists(Tensor matrix, float max_flow) -> Tensor[]");
  m.def("patch_select(Tensor scores, int m, int mode, bool grid, int k, bool pad, Tensor? noise, Tensor? cand_x, Tensor? cand_y, int offset, bool clamp, int cx0, int cx1, "
        "int cy0, int cy1, Tensor? disps, int P) -> Tensor[]");
  m.def("traj_eval(Tensor est, Tensor est_stamps, Tensor est_off, Tensor gt, Tensor gt_stamps, Tensor gt_off, int assoc, int align, float max_diff, int rpe_delta, "
        "bool want_errors, bool want_matched) -> Tensor[]");
  m.def("traj_rel_eval(Tensor est, Tensor est_stamps, Tensor est_off, Tensor gt, Tensor gt_stamps, Tensor gt_off, int assoc, float max_diff, float[] deltas, int unit, "
        "bool relative, int along, int end, int scale_mode, float scale, Tensor? scales, bool want_errors) -> Tensor[]");
  m.def("camera_points(Tensor? points, int H, int W, int device, int model, float[] K, float[] dist, float[] R, float[] K_new, bool distort, bool out_f64, bool count) "
        "-> Tensor[]");
  m.def("image_remap(Tensor images, Tensor map, Tensor? out, bool out_u8) -> Tensor");
  m.def("esim_count(Tensor prev, Tensor frames, Tensor prev_stamp, Tensor stamps, Tensor ref, Tensor last_t, float c_neg, float c_pos, int refractory_ns) -> Tensor[]");
  m.def("esim_emit(Tensor prev, Tensor frames, Tensor prev_stamp, Tensor stamps, Tensor ref, Tensor last_t, float c_neg, float c_pos, int refractory_ns, Tensor offsets, "
        "int total) -> Tensor[]");
  m.def("esim_sort(Tensor keys, int H, int W, int span_ns) -> Tensor");
  m.def("esim_decode(Tensor keys, int H, int W, Tensor first_stamp) -> Tensor[]");
  m.def("log_intensity(Tensor images, Tensor table) -> Tensor");
  m.def("optim_plan(int[] numel) -> Tensor[]");
  m.def("optim_step(Tensor chunk_table, Tensor tensor_table, int[] grad_addrs, int[] numel, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, "
        "float eps, float weight_decay, float max_norm, float bc1, float bc2, bool skip_nonfinite, Tensor(c!) counters, Tensor(d!) grad_norm, Tensor(e!) workspace) -> ()");
}
TORCH_LIBRARY_IMPL(devo_hip, CompositeExplicitAutograd, m) {
  m.impl("corr_forward", &corr_forward);
  m.impl("corr_backward", &corr_backward);
  m.impl("patchify_forward", &patchify_forward);
  m.impl("patchify_backward", &patchify_backward);
  m.impl("ba_forward", &ba_forward_op);
  m.impl("ba_neighbors", &ba_neighbors);
  m.impl("ba_reproject", &ba_reproject);
  m.impl("se3_exp", &lie_unary<devo_lie_exp, LIE_K, LIE_N>);
  m.impl("se3_log", &lie_unary<devo_lie_log, LIE_N, LIE_K>);
  m.impl("se3_inv", &lie_unary<devo_lie_inv, LIE_N, LIE_N>);
  m.impl("se3_mul", &lie_binary<devo_lie_mul, LIE_N, LIE_N>);
  m.impl("se3_adj", &lie_binary<devo_lie_adj, LIE_K, LIE_K>);
  m.impl("se3_adjT", &lie_binary<devo_lie_adjT, LIE_K, LIE_K>);
  m.impl("se3_act", &lie_binary<devo_lie_act, 3, 3>);
  m.impl("se3_act4", &lie_binary<devo_lie_act4, 4, 4>);
  m.impl("se3_projector", &lie_projector);
  m.impl("loss_forward", &loss_forward);
  m.impl("loss_backward", &loss_backward);
  m.impl("frame_graph_disps", &fg_disps);
  m.impl("frame_graph_distances", &fg_distances);
  m.impl("frame_graph_lists", &fg_lists);
  m.impl("patch_select", &patch_select);
  m.impl("traj_eval", &traj_eval);
  m.impl("traj_rel_eval", &traj_rel_eval);
  m.impl("camera_points", &camera_points);
  m.impl("image_remap", &image_remap);
  m.impl("esim_count", &esim_count);
  m.impl("esim_emit", &esim_emit);
  m.impl("esim_sort", &esim_sort);
  m.impl("esim_decode", &esim_decode);
  m.impl("log_intensity", &log_intensity);
  m.impl("optim_plan", &optim_plan);
  m.impl("optim_step", &optim_step);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "devo_amd._C: compiled binding of libdevo_hip.so with the reference's module interfaces";
  m.def("abi_version", []() { return devo_abi_version(); });
  m.def("clear_caches", &clear_caches, "drop the cached pyramid copies, patch operands and the BA workspace");
  namespace py = pybind11;

  auto corr = m.def_submodule("cuda_corr", "devo/altcorr/correlation.cpp:57-63");
  corr.def("forward", &corr_forward, "correlation.cpp:58");
  corr.def("backward", &corr_backward, "correlation.cpp:59");
  corr.def("patchify_forward", &patchify_forward, "correlation.cpp:61");
  corr.def("patchify_backward", &patchify_backward, "correlation.cpp:62");
  corr.def("last_backward_path", &corr_last_backward_path);
  corr.def("last_forward_path", [] {
    static const char* names[] = {"dense-product", "mfma4x4", "staged", "generic", "dense-product-groups"};
    const int p = devo_corr_forward_last_path();
    return std::string((p >= 0 && p < 5) ? names[p] : "");
  }, "the kernel the last forward lookup of this thread launched (devo_corr_forward_last_path)");
  corr.def("_fast_layout", &corr_fast_layout, py::arg("fmap2"), py::arg("n_edges"), py::arg("allow_split") = true);
  corr.def("_patch_operand", &corr_patch_operand);
  corr.def("_cached_levels", []() { std::lock_guard<std::mutex> g(g_levels.mu); return (int64_t)g_levels.items.size(); });
  corr.def("_is_tracked", [](int64_t ptr) { return is_tracked((const void*)(intptr_t)ptr); }, "does the cache hold a converted copy of the tensor at this address?");
  corr.def("_note_write", [](int64_t ptr, int64_t version_after, int64_t off, int64_t len) { note_write((const void*)(intptr_t)ptr, (uint32_t)version_after, off, len); },
           "a __setitem__ wrote elements [off, off + len) of the tensor at `ptr` and left its version counter at `version_after` (len < 0: region unknown)");
  corr.def("_convert_stats", [] {
    return std::make_tuple(g_conv.level_full, g_conv.level_frames, g_conv.patch_full, g_conv.patch_ranges, g_conv.patches_partial);
  }, "(whole levels converted, single frames converted, whole patch operands, patch ranges, patches in them) since the module was loaded");

  auto ba = m.def_submodule("cuda_ba", "devo/fastba/ba.cpp:152-157");
  ba.def("forward", &ba_forward, "ba.cpp:153 (in place, returns [])", py::arg("poses"), py::arg("patches"), py::arg("intrinsics"), py::arg("target"), py::arg("weight"),
         py::arg("lmbda"), py::arg("ii"), py::arg("jj"), py::arg("kk"), py::arg("t0"), py::arg("t1"), py::arg("iterations"), py::arg("ws") = py::none(),
         py::arg("status") = py::none(), py::arg("prepared") = false);
  ba.def("neighbors", &ba_neighbors, "ba.cpp:154");
  ba.def("_prep_invalidate", &ba_prep_invalidate, "forget the prepared index tables of the last forward() (an explicit prepare() rewrote the workspace)");
  ba.def("_prep_stats", [] { std::lock_guard<std::mutex> g(g_prep_mu); return std::make_pair(g_prep_hits, g_prep_misses); },
         "(hits, misses) of forward()'s prepared-table cache since the module was loaded");
  ba.def("last_path", [] {
    static const char* acc[] = {"register", "lds", "global"};
    static const char* sol[] = {"chain", "lds", "global"};
    const int p = devo_ba_last_path();
    return p < 0 ? std::string("") : std::string("accumulate:") + acc[p & 3] + " solve:" + sol[(p >> 2) & 3];
  }, "the kernels the last forward() of this thread ran (devo_ba_last_path)");
  ba.def("reproject", &ba_reproject, "ba.cpp:155");
  ba.def("transform_coords", &ba_transform, py::arg("poses"), py::arg("patches"), py::arg("intrinsics"), py::arg("ii"), py::arg("jj"), py::arg("kk"),
         py::arg("layout_2pp") = false);

  auto pg = m.def_submodule("patch_graph", "devo_amd.graph: devo/devo.py:225-239, :258-306 on the graph");
  pg.def("motion", &pg_motion);
  pg.def("keyframe", &pg_keyframe);
  pg.def("remove", &pg_remove);
  pg.def("append", &pg_append);
  pg.def("append_frame", &pg_append_frame);
  pg.def("append_frame_edges", [](int64_t M, int64_t n, int64_t lifetime) { return (int64_t)devo_odom_append_frame_edges((int)M, (int)n, (int)lifetime); });
  pg.def("shift_frames", &pg_shift_frames);
  pg.def("workspace_bytes", [](int64_t capacity) { return (int64_t)devo_graph_workspace_bytes((int)capacity); });
  auto tg = m.def_submodule("train_graph", "devo_amd.train_graph: devo/enet.py:297-339, :359-369 on the graph");
  tg.def("init", &tg_init);
  tg.def("grow", &tg_grow);
  tg.def("net_backward", &tg_net_backward);
  tg.def("workspace_bytes", [](int64_t capacity) { return (int64_t)devo_train_graph_workspace_bytes((int)capacity); });
  auto fg = m.def_submodule("frame_graph", "devo_amd.frame_graph: devo/data_readers/base.py:263-286 over rgbd_utils.py:104-141");
  fg.def("disps", &fg_disps);
  fg.def("distances", &fg_distances);
  fg.def("lists", &fg_lists);
  fg.def("workspace_bytes", [](int64_t N, int64_t h, int64_t w) { return (int64_t)devo_frame_graph_workspace_bytes((int)N, (int)h, (int)w); });
  auto sel = m.def_submodule("select", "devo_amd.select: devo/selector.py:50-287 and the tail of enet.py:100-200 in one launch");
  sel.def("patch_select", &patch_select);
  sel.attr("MAX_CELLS") = (int64_t)DEVO_SELECT_MAX_CELLS;
  auto ev = m.def_submodule("evaluation", "devo_amd.evaluation: utils/eval_utils.py's ate / ate_real (association, Umeyama alignment, ATE) in one launch");
  ev.def("traj_eval", &traj_eval);
  ev.def("workspace_bytes", [](int64_t total_est, int64_t assoc) { return (int64_t)devo_traj_eval_workspace_bytes(total_est, (int)assoc); });
  ev.attr("COLS") = (int64_t)DEVO_TRAJ_EVAL_COLS;
  ev.def("traj_rel_eval", &traj_rel_eval);
  ev.def("rel_workspace_bytes", [](int64_t total_est, int64_t assoc, int64_t B, int64_t D) {
    return (int64_t)devo_traj_rel_workspace_bytes(total_est, (int)assoc, (int)B, (int)D);
  });
  ev.attr("REL_COLS") = (int64_t)DEVO_TRAJ_REL_COLS;
  ev.attr("MAX_MATCHES") = (int64_t)DEVO_TRAJ_EVAL_MAX_MATCHES;
  auto cam = m.def_submodule("camera", "devo_amd.camera: rectification maps, point (un)distortion and image remap (what the reference takes from OpenCV)");
  cam.def("points", &camera_points);
  cam.def("remap", &image_remap);
  auto sim = m.def_submodule("simulate", "devo_amd.simulate: contrast-threshold event simulation (the reference's esim_torch.ESIM in scripts/convert_tartan.py)");
  sim.def("count", &esim_count);
  sim.def("emit", &esim_emit);
  sim.def("sort", &esim_sort);
  sim.def("decode", &esim_decode);
  sim.def("log_intensity", &log_intensity);
  sim.def("max_span_ns", [](int64_t H, int64_t W) { return (H > INT32_MAX || W > INT32_MAX) ? (int64_t)0 : devo_esim_max_span_ns((int)H, (int)W); });
  auto opt = m.def_submodule("optim", "devo_amd.optim: gradient-norm clip + AdamW in two launches (the reference's train.py:248-249)");
  opt.def("plan", &optim_plan);
  opt.def("step", &optim_step);
  opt.def("workspace_bytes", []() { return (int64_t)devo_optim_workspace_bytes(); });
  opt.attr("CHUNK") = (int64_t)DEVO_OPTIM_CHUNK;
  auto fr = m.def_submodule("frames", "devo_amd.frames: devo/devo.py:179-196, :276-280, :342-344, :487-520, :534 on the GPU");
  fr.def("begin_frame", &fr_begin);
  fr.def("point_cloud", &fr_point_cloud);
  fr.def("record_removed", &fr_record_removed);
  fr.def("record_skipped", &fr_record_skipped);
  fr.def("complete", &fr_complete);
  fr.def("complete_workspace_bytes", [](int64_t counter) { return (int64_t)devo_frame_complete_workspace_bytes((int)counter); });
  fr.def("complete_launches", [](int64_t counter) { return (int64_t)devo_frame_complete_launches((int)counter); });
  fr.def("frame_input", &fr_input);
  fr.def("frame_input_workspace_bytes", [](int64_t numel) { return (int64_t)devo_odom_input_workspace_bytes(numel); });
  fr.def("probe_median", &fr_probe_median);
  auto losses = m.def_submodule("losses", "devo_amd.losses: train.py:172-236, :254-266");
  losses.def("forward", &loss_forward);
  losses.def("backward", &loss_backward);
  losses.def("state_bytes", [](int64_t Ec, int64_t n, int64_t Ef, int64_t n_patches, int64_t dtype) {
    return (int64_t)devo_loss_state_bytes((int)Ec, (int)n, (int)Ef, (int)n_patches, (int)dtype);
  });
  m.def("bump_version", &bump_version, "count a raw-pointer write as an in-place edit of the tensor (no launch)");

  auto lie = m.def_submodule("lietorch_backends", "devo/lietorch/src/lietorch.cpp:286-316 (SO3, RxSO3, SE3, Sim3)");
  lie.def("expm", &lie_unary<devo_lie_exp, LIE_K, LIE_N>);
  lie.def("expm_backward", &lie_unary_bwd<devo_lie_exp_backward, LIE_N, LIE_K, LIE_K>);
  lie.def("logm", &lie_unary<devo_lie_log, LIE_N, LIE_K>);
  lie.def("logm_backward", &lie_unary_bwd<devo_lie_log_backward, LIE_K, LIE_N, LIE_N>);
  lie.def("inv", &lie_unary<devo_lie_inv, LIE_N, LIE_N>);
  lie.def("inv_backward", &lie_unary_bwd<devo_lie_inv_backward, LIE_N, LIE_N, LIE_N>);
  lie.def("mul", &lie_binary<devo_lie_mul, LIE_N, LIE_N>);
  lie.def("mul_backward", &lie_binary_bwd<devo_lie_mul_backward, LIE_N, LIE_N>);
  lie.def("adj", &lie_binary<devo_lie_adj, LIE_K, LIE_K>);
  lie.def("adj_backward", &lie_binary_bwd<devo_lie_adj_backward, LIE_K, LIE_K>);
  lie.def("adjT", &lie_binary<devo_lie_adjT, LIE_K, LIE_K>);
  lie.def("adjT_backward", &lie_binary_bwd<devo_lie_adjT_backward, LIE_K, LIE_K>);
  lie.def("act", &lie_binary<devo_lie_act, 3, 3>);
  lie.def("act_backward", &lie_binary_bwd<devo_lie_act_backward, 3, 3>);
  lie.def("act4", &lie_binary<devo_lie_act4, 4, 4>);
  lie.def("act4_backward", &lie_binary_bwd<devo_lie_act4_backward, 4, 4>);
  lie.def("as_matrix", &lie_as_matrix);
  lie.def("projector", &lie_projector);
  lie.def("Jinv", &lie_binary<devo_lie_jinv, LIE_K, LIE_K>);
}
