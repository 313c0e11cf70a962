// Patch selection on the GPU (devo/selector.py:50-287, PatchSelector, and the tail of enet.py:100-200 behind it), wave64, gfx950: ONE launch,
// ONE workgroup per frame, does the zero padding (never materialised), both poolings, the ranking, the mode's choice of cells and pixels, the
// shift back into the map and every tensor the Patchifier derives from the chosen centres (x, y, xy, scores, index, the closed-form patches).
//   * pooling: every SEL_K x SEL_K cell of the padded map gets its maximum with the first position in row-major order (topk, nms) or its
//     mean (multi: the 16 terms added in row-major order, times 1/16).  The map is read from global memory (it is L2-resident; a padded
//     178 x 318 map would not fit the LDS), the pooled values live in LDS as sort entries.
//   * ranking: one total order everywhere.  A sort entry is 64 bits: the key's order-preserving integer image in the high word, the
//     complement of the flat cell index in the low word, so "higher key first, lower index first on equal keys" is ONE unsigned comparison.
//     A bitonic network sorts the entries in LDS, each quadrant of the 2 x 2 grid in a power-of-two segment of its own (padded with zeros,
//     which rank behind every real entry).  No float atomics, nothing depends on scheduling: bit-reproducible.
//   * topk: the m best cells (m / 4 per quadrant), k-major and quadrant-minor as the reference's _grid2_coords_up writes them.
//   * multi: sampling without replacement as an exponential race on the caller's Exp(1) noise: key = (mean + 1e-7) / noise[cell] (no
//     epsilon without the grid, as the reference), the largest keys win in decreasing order; the pixel of output slot s is the first
//     maximum of (win[j] + 1e-7) / noise[C + 16 s + j] over the reference's window (unfold(padding = 1): it starts one pixel up-left of
//     the cell), and — as in the reference — the offset is applied to the cell's own origin.  Noise <= 0 (or NaN) counts as FLT_MIN.
//   * nms: a 3 x 3 box at every cell's maximum (the top / left clamp shifts it), category = frame or the reference's quadrant test (the box
//     corner in PIXELS against half the POOLED size), greedy suppression at IoU > 0.4 in rank order.  Boxes of cells two apart cannot
//     touch, so keep[c] = no kept neighbour of c's category that ranks before c overlaps it: iterated as a whole-map fixpoint from "all
//     kept" (cell of rank r is final after r + 1 rounds: longest suppression chain + 1 rounds of one barrier, at most C + 1), then the survivors are compacted in rank order
//     (ballot + prefix counts) and counted.  Slots beyond the count repeat the last survivor.
//   * 3xrandom: the caller's 3 m candidates, their scores (0 in the padding) sorted ascending and stable, the last m kept, and — as the
//     reference's _3xrandom — returned as x + 1, y + 1.
// Vector stores only.
#include "common.h"

namespace {

using namespace devo;

constexpr int TB = 1024;                     // 16 waves of 64: one workgroup is one frame
constexpr int WAVES = TB / 64;
constexpr int MAXC = DEVO_SELECT_MAX_CELLS;  // cells per frame, sort entries, output slots
constexpr int CPT = MAXC / TB;               // cells a thread owns
constexpr int SEL_K = 4;                     // the reference's KERNEL_SIZE
constexpr float SEL_EPS = 1e-7f;
constexpr float SEL_TINY = 1.17549435e-38f;  // FLT_MIN
static_assert(MAXC % TB == 0 && MAXC <= 65536, "cell indices are kept in 16 bits");

struct SelArgs {
  const float* scores; long long s_n, s_h, s_w;
  int n, h, w, m, mode, grid, pad, top, left, h1, w1, S, offset, clamp, cx0, cx1, cy0, cy1, H, W, P;
  const float* noise; const int64_t* cand_x; const int64_t* cand_y;
  const float* disps; long long d_n, d_h, d_w;
  int64_t* x; int64_t* y; float* xy; float* out_scores; float* patches; int64_t* index; int* counts;
};

__device__ __forceinline__ unsigned key_bits(float v) {
  const unsigned b = __float_as_uint(v + 0.0f);                   // (-0 -> +0: equal keys have equal images)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float noise_at(const float* __restrict__ nz, int i) {
  const float v = nz[i];
  return v > 0.0f ? v : SEL_TINY;
}

__global__ __launch_bounds__(TB) void k_select(const SelArgs a) {
  __shared__ unsigned long long s_ent[MAXC];                      // sort entries; the chosen centres (int2) once the cells are chosen
  __shared__ unsigned short s_sel[MAXC];                          // output slot -> cell (3xrandom: candidate)
  __shared__ unsigned short s_rank[MAXC];                         // nms: cell -> rank
  __shared__ unsigned char s_off[MAXC];                           // cell -> offset of its maximum, row-major in the cell
  __shared__ unsigned char s_keep[2][MAXC];
  __shared__ int s_wave[WAVES];
  const int f = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ map = a.scores + (long long)f * a.s_n;
  const int C = a.h1 * a.w1, m = a.m, S = a.S;
  const bool quads = a.grid && (a.mode == DEVO_SELECT_TOPK || a.mode == DEVO_SELECT_MULTI);
  const int h2 = a.h1 / 2, w2 = a.w1 / 2;
  const int T = (quads ? 4 : 1) * S;
  // the padded map at (yp, xp): 0 outside the map itself
  auto rd = [&](long long yp, long long xp) -> float {
    const long long yy = yp - a.top, xx = xp - a.left;
    return (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) ? map[yy * a.s_h + xx * a.s_w] : 0.0f;
  };

  for (int i = tid; i < T; i += TB) s_ent[i] = 0ull;
  __syncthreads();
  if (a.mode == DEVO_SELECT_3XRANDOM) {
    const int64_t* __restrict__ qx = a.cand_x + (long long)f * 3 * m;
    const int64_t* __restrict__ qy = a.cand_y + (long long)f * 3 * m;
    for (int i = tid; i < 3 * m; i += TB)                         // ascending and stable = the reverse of (key, index) descending
      s_ent[i] = ((unsigned long long)key_bits(rd(qy[i], qx[i])) << 32) | (unsigned)i;
  } else {
    const float* __restrict__ nz = a.noise + (long long)f * (C + 16 * m);
    for (int c = tid; c < C; c += TB) {
      const int cy = c / a.w1, cx = c - cy * a.w1;
      float best = rd(SEL_K * cy, SEL_K * cx), sum = best;
      int off = 0;
#pragma unroll
      for (int j = 1; j < SEL_K * SEL_K; j++) {
        const float v = rd(SEL_K * cy + j / SEL_K, SEL_K * cx + j % SEL_K);
        sum += v;
        if (v > best) { best = v; off = j; }
      }
      s_off[c] = (unsigned char)off;
      float key = best;
      if (a.mode == DEVO_SELECT_MULTI) {
        const float mean = sum * (1.0f / (SEL_K * SEL_K));
        key = __fdiv_rn(a.grid ? mean + SEL_EPS : mean, noise_at(nz, c));
      }
      int pos = c;
      if (quads) {
        const int qy = cy >= h2, qx = cx >= w2;
        pos = (2 * qy + qx) * S + (cy - qy * h2) * w2 + (cx - qx * w2);
      }
      s_ent[pos] = ((unsigned long long)key_bits(key) << 32) | (0xFFFFFFFFu - (unsigned)c);
    }
  }
  __syncthreads();

  // bitonic network, every S-aligned segment on its own, descending
  for (int k2 = 2; k2 <= S; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < T / 2; t += TB) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const bool desc = (i & k2) == 0 || k2 == S;
        const unsigned long long u = s_ent[i], v = s_ent[p];
        if ((u < v) == desc) { s_ent[i] = v; s_ent[p] = u; }
      }
      __syncthreads();
    }

  if (a.mode == DEVO_SELECT_3XRANDOM) {
    for (int s = tid; s < m; s += TB) s_sel[s] = (unsigned short)(unsigned)s_ent[m - 1 - s];
  } else if (a.mode != DEVO_SELECT_NMS) {
    for (int s = tid; s < m; s += TB) {
      const unsigned long long e = quads ? s_ent[(s & 3) * S + (s >> 2)] : s_ent[s];
      s_sel[s] = (unsigned short)(0xFFFFFFFFu - (unsigned)e);
    }
  } else {
    for (int p = tid; p < C; p += TB) s_rank[0xFFFFFFFFu - (unsigned)s_ent[p]] = (unsigned short)p;
    __syncthreads();
    // per cell: which of the 8 neighbours would suppress it if kept (same category, ranks before it, IoU > 0.4).  Box corners in half pixels.
    unsigned mask[CPT];
#pragma unroll
    for (int r = 0; r < CPT; r++) {
      const int c = r * TB + tid;
      mask[r] = 0u;
      if (c < C) {
        const int cy = c / a.w1, cx = c - cy * a.w1, o = s_off[c], rk = s_rank[c];
        const int X1 = max(2 * (SEL_K * cx + o % SEL_K) - 3, 0), Y1 = max(2 * (SEL_K * cy + o / SEL_K) - 3, 0);
        const int cat = a.grid ? (X1 >= a.w1) + 2 * (Y1 >= a.h1) : 0;          // x1 < w1 / 2 in pixels against the pooled size
#pragma unroll
        for (int b = 0; b < 8; b++) {
          const int d = b < 4 ? b : b + 1, ny = cy + d / 3 - 1, nx = cx + d % 3 - 1;
          if (ny < 0 || ny >= a.h1 || nx < 0 || nx >= a.w1) continue;
          const int q = ny * a.w1 + nx, qo = s_off[q];
          if (s_rank[q] > rk) continue;
          const int QX = max(2 * (SEL_K * nx + qo % SEL_K) - 3, 0), QY = max(2 * (SEL_K * ny + qo / SEL_K) - 3, 0);
          const int qcat = a.grid ? (QX >= a.w1) + 2 * (QY >= a.h1) : 0;
          if (qcat != cat) continue;
          const float iw = 0.5f * (float)max(6 - abs(X1 - QX), 0), ih = 0.5f * (float)max(6 - abs(Y1 - QY), 0);
          const float inter = iw * ih;
          if (__fdiv_rn(inter, 18.0f - inter) > 0.4f) mask[r] |= 1u << b;
        }
        s_keep[0][c] = 1;
      }
    }
    __syncthreads();
    int cur = 0;
    for (;;) {
      int changed = 0;
#pragma unroll
      for (int r = 0; r < CPT; r++) {
        const int c = r * TB + tid;
        if (c < C) {
          const int cy = c / a.w1, cx = c - cy * a.w1;
          unsigned char keep = 1;
#pragma unroll
          for (int b = 0; b < 8; b++) {
            const int d = b < 4 ? b : b + 1;
            if (((mask[r] >> b) & 1u) && s_keep[cur][(cy + d / 3 - 1) * a.w1 + cx + d % 3 - 1]) keep = 0;
          }
          changed |= keep != s_keep[cur][c];
          s_keep[cur ^ 1][c] = keep;
        }
      }
      cur ^= 1;
      if (!__syncthreads_or(changed)) break;
    }
    // the survivors in rank order
    int base = 0;
    const int lane = tid & 63, wv = tid >> 6;
    for (int p0 = 0; p0 < C; p0 += TB) {
      const int p = p0 + tid;
      const unsigned cell = p < C ? 0xFFFFFFFFu - (unsigned)s_ent[p] : 0u;
      const bool flag = p < C && s_keep[cur][cell];
      const unsigned long long bal = __ballot(flag);
      if (lane == 0) s_wave[wv] = __popcll(bal);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int q = 0; q < WAVES; q++) {
        const int cnt = s_wave[q];
        before += q < wv ? cnt : 0;
        total += cnt;
      }
      const int slot = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (flag && slot < m) s_sel[slot] = (unsigned short)cell;
      base += total;
      __syncthreads();
    }
    if (tid == 0) a.counts[f] = base;
    for (int s = base + tid; s < m; s += TB) s_sel[s] = s_sel[base - 1];       // (the best cell always survives: base >= 1)
  }
  __syncthreads();

  // the centres: back out of the padding, into the map, the caller's offset and range
  int2* s_pos = reinterpret_cast<int2*>(s_ent);
  for (int s = tid; s < m; s += TB) {
    const int sel = s_sel[s];
    long long xp, yp;
    float sc = 0.0f;
    if (a.mode == DEVO_SELECT_3XRANDOM) {
      xp = a.cand_x[(long long)f * 3 * m + sel];
      yp = a.cand_y[(long long)f * 3 * m + sel];
      sc = rd(yp, xp);
    } else {
      const int cy = sel / a.w1, cx = sel - cy * a.w1;
      int o = s_off[sel];
      if (a.mode == DEVO_SELECT_MULTI) {
        const float* __restrict__ nz = a.noise + (long long)f * (C + 16 * m) + C + 16 * s;
        float best = 0.0f;
#pragma unroll
        for (int j = 0; j < SEL_K * SEL_K; j++) {
          const float v = __fdiv_rn(rd(SEL_K * cy - 1 + j / SEL_K, SEL_K * cx - 1 + j % SEL_K) + SEL_EPS, noise_at(nz, j));
          if (j == 0 || v > best) { best = v; o = j; }
        }
      }
      xp = SEL_K * cx + o % SEL_K;
      yp = SEL_K * cy + o / SEL_K;
    }
    if (a.mode == DEVO_SELECT_3XRANDOM) {                                      // (the reference's _3xrandom returns x + 1, y + 1: before the shift)
      xp = min(max(xp, -(1ll << 30)), 1ll << 30) + 1;
      yp = min(max(yp, -(1ll << 30)), 1ll << 30) + 1;
    }
    int xi = (int)(xp - a.left), yi = (int)(yp - a.top);
    if (a.pad) {
      xi = min(max(xi, 0), a.w - 1);
      yi = min(max(yi, 0), a.h - 1);
    }
    if (a.mode != DEVO_SELECT_3XRANDOM) sc = map[yi * a.s_h + xi * a.s_w];
    xi += a.offset;
    yi += a.offset;
    if (a.clamp) {
      xi = min(max(xi, a.cx0), a.cx1);
      yi = min(max(yi, a.cy0), a.cy1);
    }
    const long long o = (long long)f * m + s;
    a.x[o] = xi;
    a.y[o] = yi;
    a.xy[2 * o] = (float)xi;
    a.xy[2 * o + 1] = (float)yi;
    a.out_scores[o] = sc;
    a.index[o] = f;
    s_pos[s] = make_int2(xi, yi);
  }
  __syncthreads();

  // patches [m, 3, P, P]: pixel (x + j - r, y + i - r) and its inverse depth (1 without a depth map; with one, the gather's zero outside the frame
  // and the coordinates zeroed there as well)
  const int P = a.P, PP = P * P, r = P / 2;
  float* __restrict__ out = a.patches + (long long)f * m * 3 * PP;
  const float* __restrict__ dm = a.disps ? a.disps + (long long)f * a.d_n : nullptr;
  for (int e = tid; e < m * 3 * PP; e += TB) {
    const int s = e / (3 * PP), q = e - s * 3 * PP, ch = q / PP, i = (q - ch * PP) / P, j = q - ch * PP - i * P;
    const int2 c = s_pos[s];
    const int X = c.x + j - r, Y = c.y + i - r;
    float v;
    if (dm) {
      const bool inside = X >= 0 && X < a.W && Y >= 0 && Y < a.H;
      const float in = inside ? 1.0f : 0.0f;
      v = ch == 0 ? (float)X * in : ch == 1 ? (float)Y * in : inside ? dm[Y * a.d_h + X * a.d_w] : 0.0f;
    } else {
      v = ch == 0 ? (float)X : ch == 1 ? (float)Y : 1.0f;
    }
    out[e] = v;
  }
}

int pow2_ceil(int v) {
  int s = 1;
  while (s < v) s <<= 1;
  return s;
}

}  // namespace

extern "C" int devo_patch_select(const float* scores, int64_t s_n, int64_t s_h, int64_t s_w, int n, int h, int w, int m, int mode, int grid, int k, int pad,
                                 const float* noise, const int64_t* cand_x, const int64_t* cand_y, int offset, int clamp, int cx0, int cx1, int cy0, int cy1,
                                 const float* disps, int64_t d_n, int64_t d_h, int64_t d_w, int H, int W, int P, int64_t* x, int64_t* y, float* xy,
                                 float* out_scores, float* patches, int64_t* index, int* counts, devo_stream_t stream) {
  DEVO_REQUIRE(scores && x && y && xy && out_scores && patches && index, "patch_select: null tensor");
  DEVO_REQUIRE(n >= 1 && h >= 1 && w >= 1 && m >= 1 && P >= 1 && P <= 15, "patch_select: n, h, w, m >= 1 and 1 <= P <= 15 expected (n %d, h %d, w %d, m %d, P %d)", n, h, w, m, P);
  DEVO_REQUIRE(mode >= DEVO_SELECT_TOPK && mode <= DEVO_SELECT_3XRANDOM, "patch_select: unknown mode %d", mode);
  if (k != SEL_K) {
    set_error("patch_select: cells of %d x %d (the kernel is built for the reference's 4 x 4 cells)", k, k);
    return DEVO_ERR_UNSUPPORTED;
  }
  if (h > (1 << 24) || w > (1 << 24)) {
    set_error("patch_select: a %d x %d map (at most %d pixels a side)", h, w, 1 << 24);
    return DEVO_ERR_UNSUPPORTED;
  }
  DEVO_REQUIRE(pad || mode == DEVO_SELECT_3XRANDOM, "patch_select: only 3xrandom runs on the unpadded map");
  DEVO_REQUIRE(mode != DEVO_SELECT_MULTI || noise, "patch_select: multi needs its noise");
  DEVO_REQUIRE(mode != DEVO_SELECT_NMS || counts, "patch_select: nms needs the survivor counts");
  DEVO_REQUIRE(mode != DEVO_SELECT_3XRANDOM || (cand_x && cand_y), "patch_select: 3xrandom needs its candidates");
  DEVO_REQUIRE(!disps || (H >= 1 && W >= 1), "patch_select: a depth map of %d x %d", H, W);
  DEVO_REQUIRE(!clamp || (cx0 <= cx1 && cy0 <= cy1), "patch_select: empty clamp range");
  const int f = grid ? 2 * SEL_K : SEL_K;
  const int ph = pad ? (f - h % f) % f : 0, pw = pad ? (f - w % f) % f : 0;
  SelArgs a;
  a.scores = scores; a.s_n = s_n; a.s_h = s_h; a.s_w = s_w;
  a.n = n; a.h = h; a.w = w; a.m = m; a.mode = mode; a.grid = grid ? 1 : 0; a.pad = pad ? 1 : 0;
  a.top = ph / 2; a.left = pw / 2;                                            // (the extra pixel of an odd padding goes to the bottom / right)
  a.h1 = (h + ph) / SEL_K; a.w1 = (w + pw) / SEL_K;
  a.offset = offset; a.clamp = clamp ? 1 : 0; a.cx0 = cx0; a.cx1 = cx1; a.cy0 = cy0; a.cy1 = cy1;
  a.H = H; a.W = W; a.P = P;
  a.noise = noise; a.cand_x = cand_x; a.cand_y = cand_y;
  a.disps = disps; a.d_n = d_n; a.d_h = d_h; a.d_w = d_w;
  a.x = x; a.y = y; a.xy = xy; a.out_scores = out_scores; a.patches = patches; a.index = index; a.counts = counts;
  const long long C = (long long)a.h1 * a.w1;
  if (m > MAXC) {
    set_error("patch_select: %d patches per frame (at most %d)", m, MAXC);
    return DEVO_ERR_UNSUPPORTED;
  }
  if (mode == DEVO_SELECT_3XRANDOM) {
    if (3 * m > MAXC) {
      set_error("patch_select: 3xrandom ranks 3 m = %d candidates per frame (at most %d)", 3 * m, MAXC);
      return DEVO_ERR_UNSUPPORTED;
    }
    a.S = pow2_ceil(3 * m);
  } else {
    if (C > MAXC) {
      set_error("patch_select: a %d x %d map has %lld cells per frame (at most %d)", h, w, C, MAXC);
      return DEVO_ERR_UNSUPPORTED;
    }
    if (mode == DEVO_SELECT_NMS) {
      a.S = pow2_ceil((int)C);
    } else if (grid) {
      DEVO_REQUIRE(m % 4 == 0 && m / 4 <= C / 4, "patch_select: %d patches from the 4 quadrants of %lld cells", m, C);
      a.S = pow2_ceil((int)(C / 4));
    } else {
      DEVO_REQUIRE(m <= C, "patch_select: %d patches from %lld cells", m, C);
      a.S = pow2_ceil((int)C);
    }
  }
  hipLaunchKernelGGL(k_select, dim3(n), dim3(TB), 0, (hipStream_t)stream, a);
  return check_launch("patch_select");
}
