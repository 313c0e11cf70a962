/* libdevo_hip.so — C ABI of the MI355X-native (gfx950) DEVO update + bundle-adjustment hot path.
 *
 * Every entry point replaces one function of the reference's three pybind11 extension modules
 * (cuda_corr, cuda_ba, lietorch_backends); the reference binding it stands in for is cited as
 * file:line relative to the tum-vision/DEVO tree.  Conventions:
 *   - all pointers are DEVICE pointers (HBM) unless marked host; nothing is allocated or freed
 *     inside a call; scratch space is passed in as `ws` (size from the matching *_workspace_bytes);
 *   - every call only ENQUEUES work on `stream` (a hipStream_t; NULL = the legacy default stream
 *     the reference launches on) and never synchronises with the host;
 *   - return value: DEVO_OK (0) or a DEVO_ERR_* code; devo_last_error() gives the message
 *     (the Python layer raises RuntimeError, as the reference's TORCH_CHECK / C++ exceptions do);
 *   - index arrays are int64 (torch.long), as in the reference;
 *   - `dtype`: DEVO_F32 / DEVO_F16 / DEVO_F64 select the element type of the floating tensors
 *     named "T*" below (void* in the signature).
 */
#ifndef DEVO_HIP_H
#define DEVO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* devo_stream_t; /* hipStream_t */

enum { DEVO_OK = 0, DEVO_ERR_ARG = 1, DEVO_ERR_LAUNCH = 2, DEVO_ERR_UNSUPPORTED = 3, DEVO_ERR_WORKSPACE = 4 };
enum { DEVO_F32 = 0, DEVO_F16 = 1, DEVO_F64 = 2 };

#define DEVO_ABI_VERSION 9 /* (devo_lie_*: SO3, RxSO3, SE3, Sim3 by group id, and devo_lie_projector joined version 9: new symbols, no argument list changed);
                               2: fp32 split formats (devo_corr_pyramid_split, exponents), group plans (plan buffer tail); 3: per-slot conversions of a ring
                              (devo_corr_pyramid_split_frames, devo_corr_patch_transpose_range), devo_stream_capturing; 4: devo_ba_table_offsets, devo_upd_graph_tables; 5: devo_ba_forward_prepared_delta_plan, devo_ba_import_tables, devo_upd_rs_corr_f16_net32,
                              devo_upd_rs_gru_f16_out32, devo_instnorm_cl, devo_instnorm_bias_cl, devo_bias_act_cl;
                              6: devo_voxelize_windows, devo_voxel_hot_pixels, devo_voxel_rescale (and their workspace queries);
                              7: devo_voxel_augment, devo_voxel_augment_workspace_bytes;
                              8: devo_voxel_resample, devo_depth_normalise, devo_depth_normalise_workspace_bytes;
                              9: devo_graph_motion, devo_graph_keyframe, devo_graph_remove, devo_graph_append, devo_graph_shift_frames, devo_graph_workspace_bytes
                                 (devo_loss_state_bytes, devo_loss_forward, devo_loss_backward joined version 9: new symbols, no argument list changed;
                                  so did devo_frame_begin, devo_frame_point_cloud, devo_frame_record_removed, devo_frame_record_skipped,
                                  devo_frame_complete, devo_frame_complete_workspace_bytes, devo_frame_complete_launches; and devo_train_graph_init,
                                  devo_train_graph_grow, devo_train_graph_net_backward, devo_train_graph_workspace_bytes; and devo_frame_graph_disps,
                                  devo_frame_graph_distances, devo_frame_graph_lists, devo_frame_graph_workspace_bytes; and devo_patch_select; and devo_traj_eval,
                                  devo_traj_eval_workspace_bytes; and devo_camera_undistort_points, devo_camera_distort_points, devo_image_remap;
                                  and devo_esim_count, devo_esim_emit, devo_esim_sort_keys, devo_esim_sort_workspace_bytes, devo_esim_decode, devo_esim_max_span_ns,
                                  devo_log_intensity; and devo_optim_chunks, devo_optim_moment_elems, devo_optim_workspace_bytes, devo_optim_plan,
                                  devo_optim_step; and devo_odom_input, devo_odom_input_workspace_bytes, devo_odom_probe_median,
                                  devo_odom_append_frame, devo_odom_append_frame_edges; and devo_traj_rel_eval, devo_traj_rel_workspace_bytes);
                              callers compare with devo_abi_version() */
int devo_abi_version(void);
const char* devo_last_error(void); /* thread-local message of the last failing call */
/* 1 while `stream` is being captured into a HIP graph (a capture executes nothing: a binding must not cache device state a captured call
 * would have produced — the prepared BA tables, a locality plan), 0 when it is not, -1 if the runtime cannot tell. */
int devo_stream_capturing(devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * altcorr  (reference module cuda_corr: devo/altcorr/correlation.cpp:57-63)
 * ---------------------------------------------------------------------------------------------- */

/* cuda_corr.forward  (correlation.cpp:58 -> correlation_kernel.cu:193-233, kernel :82-136).
 *   fmap1  T [B, Np, C, P, P] contiguous                (patch features, "gmap")
 *   fmap2  T [B, n2, C, H2, W2] with ELEMENT strides f2s[5] = (b, n, c, h, w); channels-last
 *            storage (c stride 1) selects the LDS-staged fast kernel, anything else the generic one
 *   coords f32 [B, E, 2, P, P] contiguous (x then y)
 *   ii, jj i64 [E]  (patch index into fmap1 dim 1, frame index into fmap2 dim 1)
 *   out    T: logical tensor [B, E, D-1 (x offset), D-1 (y offset), P, P], D = 2*radius+2 — i.e. the
 *            reference's permuted result — element (b,e,l) with l the row-major logical index is
 *            written at out[(b*E + e) * out_estride + l * out_lstride + out_offset].
 *            (out_estride = (D-1)^2*P*P, out_lstride = 1, out_offset = 0 gives a contiguous tensor;
 *             out_lstride = 2 and out_offset = level writes straight into the stacked
 *             [B, E, (D-1)^2*P*P, 2] buffer that devo/devo.py:217 / enet.py:216 build with torch.stack.)
 *   order  optional locality plan from devo_corr_order (NULL = process edges in list order).
 *   fmap1_t optional: fmap1 as devo_corr_patch_transpose lays it out.  With it, fp16 lookups into channels-last or channel-blocked
 *          storage (C = 128 / 256) and fp32 lookups into SPLIT-BLOCKED storage (cblock = DEVO_CBLOCK_SPLIT8, devo_corr_pyramid_split;
 *          C % 32 == 0, C <= 128) run as one dense product per edge on v_mfma_f32_16x16x32_f16 (csrc/corr_mm.h; fp32 values enter as
 *          fp16 hi + lo pairs of the value scaled by a power of two per patch / frame: 2^-22 relative per factor at any magnitude, fp32
 *          accumulation).  NULL, or raw fp32 storage: the 4x4 matrix-core kernel with exact fp32 products (csrc/corr_mfma.h) or, for
 *          other layouts, the staged / generic kernels.
 *   fmap2_exps: i32 [B * n2], the scale exponents devo_corr_pyramid_split wrote next to a split-blocked level (NULL otherwise). */
#define DEVO_CBLOCK_SPLIT8 (-8)
int devo_corr_forward(const void* fmap1, const void* fmap2, const float* coords, const int64_t* ii,
                      const int64_t* jj, void* out, int B, int E, int Np, int n2, int C, int P, int H2, int W2,
                      const int64_t* f2s /* host, 5 */, int cblock, int64_t out_estride, int64_t out_lstride,
                      int64_t out_offset, int radius, int dtype, const int* order /* plan buffer of devo_corr_order, i32 [2*B*E + 2], or NULL */,
                      float coord_div /* coords are divided by this in the kernel (correctly rounded IEEE division; pyramid level
                                         scale, 1 = as given; DEVO's scales 1 and 4 are exact either way) */,
                      const void* fmap1_t, const int* fmap2_exps, devo_stream_t stream);

/* Both levels of a 2-level pyramid lookup (devo/devo.py:215-217) in ONE launch: workgroups of the fine and the coarse
 * level alternate on every CU (the fine level waits on memory, the coarse one is LDS/VALU-bound), each writing its
 * slice of the edge's output record (out_offset[l], stride out_lstride).  Same results as two devo_corr_forward
 * calls.  Only for levels the staged kernel reads (channels-last or channel-blocked storage, fp32/fp16); otherwise
 * DEVO_ERR_UNSUPPORTED is returned and nothing is launched. */
int devo_corr_forward_pyramid2(const void* fmap1, const void* fmap2_l0, const void* fmap2_l1, const float* coords,
                               const int64_t* ii, const int64_t* jj, void* out, int B, int E, int Np, int n2, int C,
                               int P, const int* hw /* host: H0, W0, H1, W1 */, const int64_t* f2s /* host: 5 + 5 */,
                               const int* cblock /* host, 2 */, int64_t out_estride, int64_t out_lstride,
                               const int64_t* out_offset /* host, 2 */, int radius, int dtype, const int* order,
                               const float* coord_div /* host, 2 */,
                               const void* fmap1_t /* optional, as for devo_corr_forward: the dense-product kernel does both levels of an
                                                      edge in one wave */,
                               const int* fmap2_exps_l0, const int* fmap2_exps_l1 /* scale exponents of split-blocked levels, or NULL */,
                               int order_kind /* DEVO_PLAN_EDGES: `order` is an edge plan (or NULL); DEVO_PLAN_GROUPS: a group plan
                                                 (devo_corr_order with l1 = 4 on level 0's coordinates) — radius 3, C = 128, level 1 = the
                                                 quarter-resolution level in 8-channel blocks: level 1 is then read from LDS regions shared by
                                                 the edges of a group (csrc/corr_mm.h, the group form); same results */,
                               devo_stream_t stream);

/* fmap1 T [n_patches, C, 3, 3] -> fmap1_t, the patch operand of the dense-product lookup kernel, an opaque buffer of
 * devo_corr_patch_operand_bytes(n_patches, C, dtype) bytes (16-byte aligned) — fp16: the transposed features [n_patches, 9, C]; fp32:
 * [n_patches, 9, C / 8] split records of 32 bytes, fp16 (hi0..7 | lo0..7) with x 2^-e = hi + lo, followed by one scale exponent e (i32) per
 * patch (e puts the patch's largest magnitude into [2^13, 2^14): no magnitude overflows or underflows fp16).  C % 8 == 0.  The patch
 * features of DEVO change once per frame, not per update iteration: convert once, reuse.  DEVO_F32 / DEVO_F16. */
size_t devo_corr_patch_operand_bytes(int n_patches, int C, int dtype);
int devo_corr_patch_transpose(const void* fmap1, void* fmap1_t, int n_patches, int C, int dtype, devo_stream_t stream);
/* The same for patches [first, first + count) of an operand of n_patches (records and exponents of the others untouched): the reference
 * rewrites one frame's patches per frame (`self.gmap_[self.n % self.mem] = gmap`, devo/devo.py:524), so the operand of the ring's
 * patch features is maintained slot by slot. */
int devo_corr_patch_transpose_range(const void* fmap1, void* fmap1_t, int n_patches, int first, int count, int C, int dtype, devo_stream_t stream);

/* fp32 pyramid level -> the SPLIT-BLOCKED format the dense-product lookup kernel multiplies (no reference counterpart; the reference's
 * kernel reads fp32 NCHW, correlation_kernel.cu:82-136).  F frames fmap2 f32 [F, C, H, W] in ANY layout: element strides f2s[4] = (frame,
 * channel or channel block, row, column), cblock > 1 = channel-blocked with cblock contiguous channels per block, else plain strides.
 * dst f32-sized [F, C/8, H, W, 8] (frame stride dst_fstride elements, 16-byte aligned): the strides of an 8-channel blocked level, every
 * 32-byte pixel block holding fp16 (hi0..7 | lo0..7) with x 2^-e = hi + lo, e = exps[f] (one exponent per frame: its largest magnitude
 * lands in [2^13, 2^14)).  exps i32 [2 F]: the exponents, then F ints of scratch.  Two launches (max, convert); the pyramid of DEVO
 * changes once per frame, not per update iteration: convert once per version, pass cblock = DEVO_CBLOCK_SPLIT8 + exps to the lookups. */
int devo_corr_pyramid_split(const void* fmap2, const int64_t* f2s /* host, 4 */, int cblock, int F, int C, int H, int W, void* dst,
                            int64_t dst_fstride, int* exps, devo_stream_t stream);
/* devo_corr_pyramid_split with the F ints of scratch given separately (`exps` i32 [F] receives the exponents only): frames [k, k + F) of a
 * ring buffer are converted in place of their old records — exps = ring_exps + k, dst = ring_dst + k * dst_fstride — while the other
 * frames keep theirs (`self.fmap1_[:, self.n % self.mem] = ...`, devo/devo.py:526-527: one slot per frame). */
int devo_corr_pyramid_split_frames(const void* fmap2, const int64_t* f2s /* host, 4 */, int cblock, int F, int C, int H, int W, void* dst,
                                   int64_t dst_fstride, int* exps, int* scratch /* i32 [F] */, devo_stream_t stream);

/* Locality plan for devo_corr_forward (no reference counterpart: the reference walks edges in list order).
 * order i32 [2*B*E + 2] (the plan buffer; devo_corr_forward reads the first B*E + 1 entries and the last one (number of DEAD edges at
 * the end of the order, 0 for a single-level plan), the rest is scratch of this call): first the HEAVY edge slots (union box of the 9 windows clearly larger than a compact patch's at
 * this radius — more than 128 positions for radius <= 3, more than 256 for radius <= 5 — or larger than the staged
 * kernel's LDS tile: they run 2-4x longer and should start first), then the others sorted by (batch, target frame jj,
 * bin of the patch centre: 16-row bands x 8-px columns, numbered in blocks of 4 bands x ~64 px), so that the lookup
 * kernel's XCD-aware schedule streams every feature row through an L2 about once; order[B*E] = number of heavy
 * edges.  `coord_scale`
 * is the factor the caller divides coords by for the pyramid level whose height is H2 (1 for level 0); one
 * plan serves all levels of a pyramid.  The plan only changes WHICH edges run together, never any result. */
int devo_corr_order(const float* coords, const int64_t* jj, int* order, int B, int E, int n2, int P, int H2,
                    float coord_scale, int radius,
                    int W2 /* width of the plan's level; only read when l1 >= 2 */,
                    int l1 /* 0: edge plan (above).  >= 2 (DEVO: 4): GROUP plan for devo_corr_forward_pyramid2(order_kind = DEVO_PLAN_GROUPS) —
                              the lookup has a second level at 1 / l1 of this resolution, radius 3; `order` is then i32
                              [DEVO_CORR_PLAN_INTS(B*E)].  A group = the edges of one target frame whose patch centre lies in one tile of
                              6 x 6 level-1 cells; the plan sorts the edges by group (same prefix as an edge plan: any lookup accepts it) and
                              stores every group's first slot behind the 2*B*E + 2 ints.  Classes: DEAD edges (union box outside the frame at
                              both levels: every output is 0) go BEHIND all others, order[2*B*E + 1] = their number; HEAVY (in front) = more
                              than 128 level-0 box positions, or a level-1 box that leaves the group's 15 x 15 region (patch pixels more than
                              a level-1 cell from the centre).  DEVO_ERR_UNSUPPORTED when the frames have more than 4095 groups together
                              (or radius != 3): use an edge plan */,
                    devo_stream_t stream);
#define DEVO_CORR_PLAN_TAIL 4104
#define DEVO_CORR_PLAN_INTS(BE) (2 * (BE) + 2 + DEVO_CORR_PLAN_TAIL) /* ints of a plan buffer that can hold a group plan (an edge plan uses the first 2 BE + 2) */
#define DEVO_PLAN_EDGES 0
#define DEVO_PLAN_GROUPS 1

/* Pyramid build for the lookup (devo/devo.py:526-527: fmap1_[slot] = avg_pool2d(fmap, 1, 1), fmap2_[slot] =
 * avg_pool2d(fmap, 4, 4); devo/utils.py:70-79): F frames fmap T [F, C, H, W] (contiguous frames, frame stride
 * fmap_fstride elements) -> channel-blocked level 0  l0 T [F, C/8, H, W, 8] and level 1  l1 T [F, C/8, H/4, W/4, 8]
 * (4x4 mean; NULL = skip), frame strides l0_fstride / l1_fstride so that a frame can be written into a slot of a
 * ring buffer.  One pass over the input.  DEVO_F32 / DEVO_F16 (fp32 accumulation). */
int devo_pyramid_build(const void* fmap, void* l0, void* l1, int F, int C, int H, int W, int64_t fmap_fstride,
                       int64_t l0_fstride, int64_t l1_fstride, int dtype, devo_stream_t stream);

/* cuda_corr.backward  (correlation.cpp:59 -> correlation_kernel.cu:236-286, kernel :139-190).
 *   grad f32: the gradient of the logical [B,E,D-1,D-1,P,P] output, contiguous.
 *   fmap1_grad [B,Np,C,P,P] contiguous, fmap2_grad with the strides of fmap2: both are ZEROED and then
 *   accumulated here.  DEVO_F32 only (the reference's grad accessor is float, :146,280).
 *   ws / ws_bytes: scratch of devo_corr_backward_workspace_bytes(B, E, Np, n2, C, radius, channels_last) bytes, 16-byte aligned (the
 *   window gradients, the frames' window lists, fmap1 transposed: the product form for channels-last fmap2 with C % 128 == 0,
 *   DESIGN.md 3.2).  channels_last = 1 when the C channels of a pixel of fmap2 are contiguous and pixels / rows are C / W*C elements
 *   apart; every other layout takes the one-kernel atomic path and the query returns 0.  NULL or too small: the atomic path as well.
 *   The library never allocates.  devo_corr_backward_last_path(): which path the calling thread's last devo_corr_backward took. */
#define DEVO_CORR_BWD_ATOMIC   0
#define DEVO_CORR_BWD_SEGMENTS 1
#define DEVO_CORR_BWD_PRODUCT  2
size_t devo_corr_backward_workspace_bytes(int B, int E, int Np, int n2, int C, int radius, int channels_last);
int devo_corr_backward_last_path(void);
/* Which kernel the last forward lookup of the calling thread launched: 0 the dense-product kernel (corr_mm.h: the default for blocked fp16 /
 * split-blocked fp32 levels), 4 its group form (level 1 from LDS), 1 the exact-fp32 4x4 matrix-core kernel (raw fp32 blocked / channels-last
 * levels, DEVO_CORR_MM=0), 2 the staged tap-centric kernel (other channel counts, DEVO_CORR_MFMA=0; ~2x), 3 the generic kernel (fp64, raw NCHW,
 * unaligned strides; ~24x); -1 before the first call.  The first call of a process that takes kernel 2 or 3 with >= 2048 edges also says so on
 * stderr (DEVO_LOG_FALLBACK=0: silent). */
int devo_corr_forward_last_path(void);
/* What the last devo_ba_forward* of the calling thread ran: accumulate kind (0 register-resident, N <= 16; 1 general in LDS; 2 global memory, N > 32)
 * + 4 * solve kind (0 one-barrier chain, 6N <= 128; 1 general in LDS; 2 global memory); -1 before the first call.  The first call of a process
 * whose system leaves the LDS says so on stderr (DEVO_LOG_FALLBACK=0: silent). */
int devo_ba_last_path(void);
int devo_corr_backward(const void* fmap1, const void* fmap2, const float* coords, const int64_t* ii,
                       const int64_t* jj, const float* grad, void* fmap1_grad, void* fmap2_grad, int B, int E,
                       int Np, int n2, int C, int P, int H2, int W2, const int64_t* f2s /* host, 5 */,
                       int64_t f2_numel_span /* elements spanned by fmap2 storage */, int radius, int dtype,
                       void* ws, size_t ws_bytes, devo_stream_t stream);

/* cuda_corr.patchify_forward  (correlation.cpp:61 -> correlation_kernel.cu:288-307, kernel :16-47).
 *   net T [B, C, H, W] with element strides ns[4]; coords f32 [B, M, 2]; out T [B, M, C, D, D] contiguous
 *   (zero where the tap is out of bounds). */
int devo_patchify_forward(const void* net, const float* coords, void* out, int B, int M, int C, int H, int W,
                          const int64_t* ns /* host, 4 */, int radius, int dtype, devo_stream_t stream);

/* cuda_corr.patchify_backward  (correlation.cpp:62 -> correlation_kernel.cu:310-333, kernel :49-80).
 *   grad T [B, M, C, D, D] contiguous -> net_grad T [B, C, H, W] (zeroed here) with element strides gs[4] (host; NULL: contiguous; any
 *   dense permutation, e.g. channels-last — the layout the encoders' convolutions take their gradient in). F32/F64. */
int devo_patchify_backward(const float* coords, const void* grad, void* net_grad, int B, int M, int C, int H,
                           int W, const int64_t* gs, int radius, int dtype, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * fastba  (reference module cuda_ba: devo/fastba/ba.cpp:152-157)
 * ---------------------------------------------------------------------------------------------- */

/* 0 when the sizes are not supported: N = t1 - t0 <= 128 optimised poses per call (the reference has no limit, ba_cuda.cu:516-522; DEVO
 * uses <= 14).  Up to 32 the reduced system lives in one workgroup's LDS; beyond, in global memory (device-scope atomics like the
 * reference's, the blocked Cholesky in place on the global image). */
size_t devo_ba_workspace_bytes(int E, int Np /* patch slots = patches.shape[1] */, int N /* t1 - t0 */);

/* cuda_ba.forward  (ba.cpp:153 -> ba_cuda.cu:422-540).  IN-PLACE on poses and patches, returns nothing.
 *   poses f32 [Nbuf,7]; patches f32 [Np,3,P,P]; intrinsics f32 [>=1,4] (row 0 only, ba_cuda.cu:233-237);
 *   target, weight f32 [E,2]; lmbda f32 [1]; ii,jj,kk i64 [E]; frames < t0 are fixed; t1-t0 == 0 is the
 *   structure-only branch.  A Cholesky breakdown (the reference's cuSOLVER exception, swallowed by
 *   devo/devo.py:336-340) leaves poses/patches of that iteration untouched and sets *status_flag (i32,
 *   device, may be NULL) to the failing iteration + 1. */
int devo_ba_forward(float* poses, float* patches, const float* intrinsics, const float* target,
                    const float* weight, const float* lmbda, const int64_t* ii, const int64_t* jj,
                    const int64_t* kk, int E, int Nbuf, int Np, int P, int t0, int t1, int iterations, void* ws,
                    size_t ws_bytes, int* status_flag, devo_stream_t stream);

/* The same call split in two, for callers that know the graph before target/weight are ready (in DEVO: before the
 * correlation lookup and the update network, devo/devo.py:213-240): devo_ba_prepare does the index work of
 * ba_cuda.cu:435-437 (unique patches, edges grouped by patch; depends on kk only) — e.g. on a second stream —
 * and devo_ba_forward_prepared runs the Gauss-Newton iterations on the prepared workspace.  A prepared workspace
 * stays valid (any number of forward calls) until kk, E, Np or t1 - t0 change.  devo_ba_forward_prepared on a
 * workspace that was not prepared for this (E, t1 - t0) touches nothing and sets *status_flag to -1. */
int devo_ba_prepare(const int64_t* kk, int E, int Np, int N /* t1 - t0 */, void* ws, size_t ws_bytes,
                    devo_stream_t stream);
/* devo_ba_prepare + the ordering step of the lookup's locality plan (devo_corr_order with coords = NULL) in ONE launch:
 * both are single-workgroup, latency-bound kernels that do not depend on each other, so they run as two workgroups side
 * by side.  plan: i32 [2E + 2] (group plans: [DEVO_CORR_PLAN_INTS(E)]) whose bins devo_transform(..., plan, plan_frames, plan_height,
 * radius, plan_width, plan_l1) has written (batch 1); afterwards it is the finished plan for devo_corr_forward*.  plan_width, plan_l1:
 * the values given to devo_transform (l1 = 0: edge plan). */
int devo_ba_prepare_plan(const int64_t* kk, int E, int Np, int N /* t1 - t0 */, void* ws, size_t ws_bytes, int* plan,
                         int plan_frames, int plan_height, int plan_width, int plan_l1, devo_stream_t stream);
/* Inspection of a prepared workspace (tests / debugging): copies (device to device, any pointer may be NULL)
 * *n_seg = number of distinct patches with edges, kx i32 [min(E,Np)] = their ids ascending (the first output of
 * torch::_unique(kk), ba_cuda.cu:435-437), seg_start i32 [min(E,Np)+1] and perm i32 [E]: the edges of patch kx[s]
 * are perm[seg_start[s] .. seg_start[s+1]) in ascending edge order (the inverse map of _unique, grouped). */
int devo_ba_prepared_tables(const void* ws, size_t ws_bytes, int E, int Np, int N, int* n_seg, int* kx,
                            int* seg_start, int* perm, devo_stream_t stream);
/* The same tables IN PLACE: byte offsets into a prepared workspace of (E, Np, N) — offsets[0] the i32 n_seg, [1] kx, [2] seg_start, [3] perm —
 * and offsets[4] = min(E, Np), the element count of kx (seg_start has one more).  A caller that owns the workspace reads the tables where
 * they lie (devo_amd.update's group tables: eight device copies per frame of DEVO's steady state otherwise).  No device work. */
int devo_ba_table_offsets(int E, int Np, int N, size_t* offsets /* [5] */);
/* The index tables of a kk from a workspace prepared for other sizes of the SAME edge list (src_Np patch slots, src_N optimised poses: e.g.
 * devo_upd_graph_tables' patch-group workspace: its bound, 0) into `ws` (Np, N): one launch instead of devo_ba_prepare's nine — devo.py:311,337
 * hand the same kk to the Update operator and, right behind it, to the BA.  Afterwards `ws` is what devo_ba_prepare(kk, E, Np, N) leaves, provided
 * every id of kk is below Np; a source with ids in [Np, src_Np) leaves `ws` unprepared (the BA then reports status -1). */
int devo_ba_import_tables(const void* src_ws, size_t src_bytes, int src_Np, int src_N, void* ws, size_t ws_bytes, int E, int Np, int N,
                          devo_stream_t stream);
int devo_ba_forward_prepared(float* poses, float* patches, const float* intrinsics, const float* target,
                             const float* weight, const float* lmbda, const int64_t* ii, const int64_t* jj,
                             const int64_t* kk, int E, int Nbuf, int Np, int P, int t0, int t1, int iterations,
                             void* ws, size_t ws_bytes, int* status_flag, devo_stream_t stream);

/* devo_ba_forward_prepared with devo/devo.py:330 (`target = coords[..., P//2, P//2] + delta`) folded in: the target of
 * edge e, component c is coords[e * coords_edge_stride + c * coords_xy_stride + coords_centre] + delta[2e + c] — the same
 * single fp32 addition, so the result is bit-identical to forming `target` first; one elementwise launch less per
 * update iteration.  coords: the f32 buffer devo_transform wrote ([E,2,P,P]: strides 2PP, PP, centre (P/2)(P+1);
 * [E,P,P,2]: strides 2PP, 1, centre 2 (P/2)(P+1)); delta f32 [E,2] (the update operator's output). */
int devo_ba_forward_prepared_delta(float* poses, float* patches, const float* intrinsics, const float* coords,
                                   int coords_edge_stride, int coords_xy_stride, int coords_centre, const float* delta,
                                   const float* weight, const float* lmbda, const int64_t* ii, const int64_t* jj,
                                   const int64_t* kk, int E, int Nbuf, int Np, int P, int t0, int t1, int iterations,
                                   void* ws, size_t ws_bytes, int* status_flag, devo_stream_t stream);

/* devo_ba_forward_prepared_delta, and the ordering step of a locality plan (devo_corr_order / devo_ba_prepare_plan's second half) for the
 * buffer `plan` whose bins devo_transform(..., plan, ...) has written — carried by extra workgroups of the first Gauss-Newton iteration's
 * solver launch (no launch of its own, nothing on the critical path; a separate launch where this call has no such solver launch).  A plan
 * only decides which edges run together: the lookup of update iteration k + 1 (devo.py:308-344 runs them back to back on one patch graph)
 * takes the plan made from iteration k's coordinates, the BA of iteration k carries its ordering.  Same results as the two calls. */
int devo_ba_forward_prepared_delta_plan(float* poses, float* patches, const float* intrinsics, const float* coords,
                                        int coords_edge_stride, int coords_xy_stride, int coords_centre, const float* delta,
                                        const float* weight, const float* lmbda, const int64_t* ii, const int64_t* jj,
                                        const int64_t* kk, int E, int Nbuf, int Np, int P, int t0, int t1, int iterations,
                                        void* ws, size_t ws_bytes, int* status_flag, int* plan, int plan_frames, int plan_height,
                                        int plan_width, int plan_l1, devo_stream_t stream);

/* One differentiable Gauss-Newton step of devo/ba.py:108-170 (normal equations, Schur complement over the patches, damped
 * Cholesky solve) from GIVEN per-edge terms, for devo_amd.ba.BA (the reference builds it with ten matmuls + ten
 * torch_scatter.scatter_sum calls and solves with CholeskySolver, ba.py:12-37).
 * terms f32 [E,30]: r[2] w[2] Jz[2] Ji[2][6] Jj[2][6] with Ji = MINUS d coords / d xi_i (this library's sign convention);
 * frames < t0 or >= t0 + N are fixed; damping S_dd + ep + 1e-4 S_dd (ba.py:73); lmbda f32 [1] on the device.
 * Outputs: dX f32 [6 N] (zero when the factorisation breaks down, like ba.py:16-20; *status_flag = 1 then),
 * dZ f32 [Np] per patch SLOT (zero for patches without an edge).  N <= 32 here.  The workspace (devo_ba_workspace_bytes(E, Np, N)) keeps
 * what the adjoint needs: pass it unmodified to devo_ba_solve_terms_backward. */
int devo_ba_solve_terms(const float* terms, const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                        int Np, int t0, int N, float ep, void* ws, size_t ws_bytes, float* dX, float* dZ, int* status_flag,
                        devo_stream_t stream);

/* Adjoint of devo_ba_solve_terms (what autograd derives for ba.py:108-170 + CholeskySolver.backward, ba.py:28-37): from the
 * gradients of dX [6 N] and dZ [Np] to the gradient of the 30 terms of every edge, g_terms f32 [E,30].  One more solve with
 * the saved matrix, then per-patch and per-edge kernels. */
int devo_ba_solve_terms_backward(const float* terms, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int Np, int t0, int N, void* ws,
                                 size_t ws_bytes, const float* g_dX, const float* g_dZ, float* g_terms, devo_stream_t stream);

/* The update step behind the differentiable solve (devo/ba.py:172-182: `poses.retr(dX)` on the optimised window, inverse depth + dZ clamped to
 * [dmin, dmax] over every patch's P x P pixels, torch.stack) as ONE kernel per direction instead of ~8 / ~12 ATen + SE3 launches; fp32.
 * poses [N,7], patches [Np,3,P,P], dX [6 n_opt] (NULL when n_opt == 0), dZ [Np].  The backward takes the gradients of both outputs (either
 * may be NULL = zero; pose gradients in lietorch's embedding, tangent in the first six of seven) and returns all four input gradients. */
int devo_ba_apply_step(const float* poses, const float* patches, const float* dX, const float* dZ, int N, int Np, int P, int fixedp, int n_opt,
                       float dmin, float dmax, float* poses_out, float* patches_out, devo_stream_t s);
int devo_ba_apply_step_backward(const float* poses, const float* patches, const float* dX, const float* dZ, const float* g_poses_out,
                                const float* g_patches_out, int N, int Np, int P, int fixedp, int n_opt, float dmin, float dmax,
                                float* g_poses, float* g_patches, float* g_dX, float* g_dZ, devo_stream_t s);

/* devo/ba.py:95-106 for the differentiable BA (training): residuals, gate and the 30 per-edge numbers of devo_ba_solve_terms from
 * the outputs of devo_transform(jacobian): coords [E,P,P,2], valid [E], Ji / Jj [E,2,6], Jz [E,2], target / weight [E,2], bounds (host:
 * x0, y0, x1, y1) -> terms [E,30] = r | w | Jz | -Ji | Jj and the gate [E] (kept for the adjoint). */
int devo_ba_edge_terms(const float* coords, const float* valid, const float* Ji, const float* Jj, const float* Jz, const float* target,
                       const float* weight, const float* bounds /* host, 4 */, int E, int P, float* terms, float* gate, devo_stream_t stream);
/* its adjoint: g_terms [E,30] -> g_coords [E,P,P,2] (zeroed here; only the centre pixel carries gradient), g_target, g_weight [E,2],
 * g_Ji, g_Jj [E,2,6], g_Jz [E,2]. */
int devo_ba_edge_terms_backward(const float* g_terms, const float* gate, int E, int P, float* g_coords, float* g_target, float* g_weight,
                                float* g_Ji, float* g_Jj, float* g_Jz, devo_stream_t stream);

/* Adjoint of devo_transform (what autograd derives for devo/projective_ops.py:53-105, second-order terms of the Jacobians
 * included): cotangents of the coordinates g_coords f32 [E,P,P,2|3] ("pp2" layout; NULL = none) and of the centre pixel's
 * Jacobians g_Ji / g_Jj f32 [E,2,6], g_Jz f32 [E,2] (NULL = none) -> g_poses f32 [Nbuf,7] (6-vector of the left perturbation
 * G <- Exp(xi) G in the first six slots, lietorch's convention: lietorch_gpu.cu:174-256) and g_patches f32 [Np,3,P,P]; both are
 * zeroed and accumulated here.  flags as devo_transform (1 = depth channel, 2 = translation only). */
int devo_transform_vjp(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii, const int64_t* jj,
                       const int64_t* kk, const float* g_coords, const float* g_Ji, const float* g_Jj, const float* g_Jz, int E,
                       int Nbuf, int Np, int P, int flags, float* g_poses, float* g_patches, devo_stream_t stream);

size_t devo_neighbors_workspace_bytes(int E);

/* cuda_ba.neighbors  (ba.cpp:154 -> ba.cpp:104-149): for every edge the previous / next edge of the same
 * ii[e] ordered by jj (stable), -1 at the ends.  ix, jx i64 [E] on the device; bit-exact. */
int devo_ba_neighbors(const int64_t* ii, const int64_t* jj, int64_t* ix, int64_t* jx, int E, void* ws,
                      size_t ws_bytes, devo_stream_t stream);

/* cuda_ba.reproject  (ba.cpp:155 -> ba_cuda.cu:543-575, kernel :368-418): coords f32 [E,2,P,P], no Z clamp. */
int devo_ba_reproject(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii,
                      const int64_t* jj, const int64_t* kk, float* coords, int E, int P, devo_stream_t stream);

/* Fused restatement of devo/projective_ops.py:53-105 `transform` (the reprojection DEVO.update really
 * calls, devo/devo.py:222): per-frame intrinsics [n,4], Z clamped at 0.1 in the projection.
 *   coords  f32 [E, P, P, 2 (+1 if depth)]  when coords_pp2 != NULL   (reference layout, :70)
 *   coords_2pp f32 [E, 2, P, P] when != NULL (the permute(0,1,4,2,3).contiguous() of devo.py:223)
 *   valid   f32 [E] or NULL (Z > 0.2 at the centre pixel, :100/:103)
 *   Ji, Jj  f32 [E,2,6], Jz f32 [E,2] or NULL  (:73-98; Ji already negated as in :96)
 *   flags   bit0 = depth, bit1 = tonly
 *   plan    optional locality-plan buffer of the lookup (i32 [2*E + 2], group plans [DEVO_CORR_PLAN_INTS(E)], see devo_corr_order): while the
 *           coordinates are still in registers the kernel writes every edge's plan bin (for a pyramid whose
 *           level 0 has plan_frames frames of plan_height rows, lookup radius plan_radius) into the buffer's
 *           scratch half; devo_corr_order(coords = NULL, ...) then only sorts.  P == 3.  NULL = no plan. */
int devo_transform(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii,
                   const int64_t* jj, const int64_t* kk, float* coords_pp2, float* coords_2pp, float* valid,
                   float* Ji, float* Jj, float* Jz, int E, int P, int flags, int* plan, int plan_frames,
                   int plan_height, int plan_radius, int plan_width, int plan_l1 /* as W2, l1 of devo_corr_order */,
                   devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * lietorch SE3 subset  (reference module lietorch_backends: devo/lietorch/src/lietorch.cpp:286-316,
 * group_id 3 only; kernels lietorch_gpu.cu:20-294).  X: T [n,7], tangent: T [n,6], gradients of group
 * elements are written to the first 6 of 7 slots (slot 7 = 0).  dtype F32 or F64.
 * ---------------------------------------------------------------------------------------------- */
int devo_se3_exp(const void* a, void* X, int64_t n, int dtype, devo_stream_t s);                    /* :287 expm */
int devo_se3_exp_backward(const void* grad, const void* a, void* da, int64_t n, int dtype, devo_stream_t s);
int devo_se3_log(const void* X, void* a, int64_t n, int dtype, devo_stream_t s);                    /* :290 logm */
int devo_se3_log_backward(const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s);
int devo_se3_inv(const void* X, void* Y, int64_t n, int dtype, devo_stream_t s);                    /* :293 inv */
int devo_se3_inv_backward(const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s);
int devo_se3_mul(const void* X, const void* Y, void* Z, int64_t n, int dtype, devo_stream_t s);     /* :296 mul */
int devo_se3_mul_backward(const void* grad, const void* X, const void* Y, void* dX, void* dY, int64_t n,
                          int dtype, devo_stream_t s);
int devo_se3_adj(const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s);     /* :299 adj */
int devo_se3_adj_backward(const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n,
                          int dtype, devo_stream_t s);
int devo_se3_adjT(const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s);    /* :302 adjT */
int devo_se3_adjT_backward(const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n,
                           int dtype, devo_stream_t s);
int devo_se3_act(const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s);     /* :305 act */
int devo_se3_act_backward(const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n,
                          int dtype, devo_stream_t s);
int devo_se3_act4(const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s);    /* :308 act4 */
int devo_se3_act4_backward(const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n,
                           int dtype, devo_stream_t s);
int devo_se3_as_matrix(const void* X, void* T44, int64_t n, int dtype, devo_stream_t s);            /* :313 as_matrix */
int devo_se3_jinv(const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s);    /* :314 Jinv */

/* ------------------------------------------------------------------------------------------------
 * lietorch, all four groups (dispatch.h): group 1 SO3 (X [n,4] = q_xyzw, tangent [n,3] = phi), 2 RxSO3 (X [n,5] = q, s; tangent
 * [n,4] = phi, sigma), 3 SE3 (as above: these calls forward to devo_se3_*), 4 Sim3 (X [n,8] = t, q, s; tangent [n,7] = tau, phi,
 * sigma).  Same argument lists as devo_se3_* with the group id in front; gradients of group elements (N slots) hold a tangent in the
 * first K = N - 1 slots and 0 in the last.  Points: [n,3] (act) and [n,4] (act4).  Any other group id: DEVO_ERR_ARG.
 * devo_lie_projector: P [n,N,N] row-major, d(embedded coordinates) / d(left perturbation), last column zero (lietorch.cpp:312).
 * ---------------------------------------------------------------------------------------------- */
int devo_lie_exp(int group, const void* a, void* X, int64_t n, int dtype, devo_stream_t s);
int devo_lie_exp_backward(int group, const void* grad, const void* a, void* da, int64_t n, int dtype, devo_stream_t s);
int devo_lie_log(int group, const void* X, void* a, int64_t n, int dtype, devo_stream_t s);
int devo_lie_log_backward(int group, const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s);
int devo_lie_inv(int group, const void* X, void* Y, int64_t n, int dtype, devo_stream_t s);
int devo_lie_inv_backward(int group, const void* grad, const void* X, void* dX, int64_t n, int dtype, devo_stream_t s);
int devo_lie_mul(int group, const void* X, const void* Y, void* Z, int64_t n, int dtype, devo_stream_t s);
int devo_lie_mul_backward(int group, const void* grad, const void* X, const void* Y, void* dX, void* dY, int64_t n,
                          int dtype, devo_stream_t s);
int devo_lie_adj(int group, const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s);
int devo_lie_adj_backward(int group, const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n,
                          int dtype, devo_stream_t s);
int devo_lie_adjT(int group, const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s);
int devo_lie_adjT_backward(int group, const void* grad, const void* X, const void* a, void* dX, void* da, int64_t n,
                           int dtype, devo_stream_t s);
int devo_lie_act(int group, const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s);
int devo_lie_act_backward(int group, const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n,
                          int dtype, devo_stream_t s);
int devo_lie_act4(int group, const void* X, const void* p, void* q, int64_t n, int dtype, devo_stream_t s);
int devo_lie_act4_backward(int group, const void* grad, const void* X, const void* p, void* dX, void* dp, int64_t n,
                           int dtype, devo_stream_t s);
int devo_lie_as_matrix(int group, const void* X, void* T44, int64_t n, int dtype, devo_stream_t s);
int devo_lie_jinv(int group, const void* X, const void* a, void* b, int64_t n, int dtype, devo_stream_t s);
int devo_lie_projector(int group, const void* X, void* P, int64_t n, int dtype, devo_stream_t s);

/* ------------------------------------------------------------------------------------------------
 * Update operator pieces (devo/enet.py:32-99, devo/blocks.py:15-48) — the reductions and
 * element-wise steps between the GEMMs (the dense layers are plain library GEMMs issued by the host side).
 * T = DEVO_F32 / DEVO_F16 storage, fp32 arithmetic; rows are contiguous [rows, dim].
 * ---------------------------------------------------------------------------------------------- */

/* out = LayerNorm(x + add1 + add2 + hy[group_of[row]] + sigmoid(gate) * res) * gamma + beta — nn.LayerNorm(dim, eps)
 * (enet.py:47,53-55,65) with the sums in front of it fused in: the residual sums of enet.py:82-83 (add1, add2), the
 * SoftAgg expand of blocks.py:46 (hy + group_of) and the GatedResidual of blocks.py:28-29 (gate with row stride
 * ld_gate, res); every term may be NULL.  Optionally followed by ReLU (enet.py:65-66).  dim <= 1024. */
/* InstanceNorm2d without affine parameters or running statistics (the encoders' norm: devo/extractor.py:27-38) on a CHANNELS-LAST activation
 * x [N, H, W, C] (HW pixels per image), fp32 / fp16, 16-byte aligned, C a multiple of 4 / 8:  y = (x - mean_nc) * rstd_nc, biased variance,
 * rounded to the storage type, then ReLU'd when `relu`; with `res` (same layout; needs relu) y = relu(res + relu(norm(x))) — the tail of a
 * residual block (extractor.py:48-54).  Two launches (partial sums in a fixed order, apply): deterministic.  workspace: devo_instnorm_workspace_bytes. */
size_t devo_instnorm_workspace_bytes(int N, int C);
int devo_instnorm_cl(const void* x, const void* res, void* y, int N, int HW, int C, float eps, int relu, void* workspace, size_t ws_bytes, int dtype,
                     devo_stream_t stream);
/* ... with the convolution's bias [C] (same dtype, 16-byte aligned; or NULL) added in front as ATen adds it behind a bias-free MIOpen call:
 * the norm sees round(x + bias) — the caller leaves the bias out of the convolution (one elementwise launch per convolution less). */
int devo_instnorm_bias_cl(const void* x, const void* bias, const void* res, void* y, int N, int HW, int C, float eps, int relu, void* workspace,
                          size_t ws_bytes, int dtype, devo_stream_t stream);
/* y = act(round(x + bias)) — act = ReLU when `relu` — and, with `res` (needs relu), relu(round(res + y)), on a channels-last activation of
 * `pixels` x C elements (fp32 / fp16, C a multiple of 4 / 8, 16-byte aligned; bias may be NULL): the bias add, ReLU, sum and ReLU behind a
 * convolution of the context encoder (extractor.py:27-54 with norm_fn = 'none') as one launch. */
int devo_bias_act_cl(const void* x, const void* bias, const void* res, void* y, int64_t pixels, int C, int relu, int dtype, devo_stream_t stream);
int devo_upd_layernorm(const void* x, const void* add1, const void* add2, const void* hy, const int* group_of,
                       const void* gate, int64_t ld_gate, const void* res, const void* gamma, const void* beta,
                       void* out, int64_t rows, int dim, float eps, int relu, int dtype, devo_stream_t stream);

/* The adjoint of devo_upd_layernorm without the hy / gate terms (training; the reference differentiates nn.LayerNorm through
 * torch.autograd, enet.py:44,52-56,62): fp32, dim == 384.  y = LN(x + add1 + add2) [ReLU'd], dout = dL/dy  ->  dx (the gradient of x and of
 * either addend) and dgamma += sum_rows dout xhat, dbeta += sum_rows dout (ADDED into buffers the caller has zeroed or is accumulating
 * in).  Mean and variance are recomputed from the inputs: the forward saves nothing but its inputs.
 * partials: NULL — the workgroups add their column sums with float atomics (order, hence the last bits, varies from run to run); or f32
 * [512 * 2 * dim] of scratch — they store them and a second small kernel adds them in workgroup order: bit-reproducible (what
 * torch.use_deterministic_algorithms(True) selects in devo_amd.update). */
int devo_upd_layernorm_backward(const float* x, const float* add1, const float* add2, const float* gamma, const float* beta,
                                const float* dout, float* dx, float* dgamma, float* dbeta, int64_t rows, int dim, float eps, int relu,
                                float* partials, devo_stream_t stream);

/* The graph tables of the Update operator (devo/enet.py:86-95) for one edge list, in one call:
 *   ws_kk  <- devo_ba_prepare(kk, bound, 0): the edges grouped by patch (the scatter_softmax / scatter_sum index of agg_kk, blocks.py:42-43)
 *   ix, jx <- cuda_ba.neighbors(kk, jj) (ba.cpp:104-149) read off those groups (NULL, NULL: skipped); kk must lie in [0, bound)
 *   ws_ij  <- devo_ba_prepare(pair, bound, 0) with pair = (ii - min ii) * (max jj - min jj + 1) + (jj - min jj): the groups of
 *             ii * 12345 + jj (enet.py:94) with keys inside (frames in the window)^2, which must stay below bound
 * ws_kk, ws_ij: devo_ba_workspace_bytes(E, bound, 0) bytes each, read through devo_ba_table_offsets(E, bound, 0); pair_key i64 [E + 2]
 * scratch (holds the keys afterwards).  DEVO's inference hands the operator new index tensors every frame: this is per-frame work. */
int devo_upd_graph_tables(const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int bound, void* ws_kk,
                          size_t ws_kk_bytes, void* ws_ij, size_t ws_ij_bytes, int64_t* pair_key, int64_t* ix, int64_t* jx,
                          devo_stream_t stream);

/* out[e] = idx[e] >= 0 ? src[idx[e]] : 0   — `mask * net[:, ix]` of enet.py:87-91 (idx from devo_ba_neighbors). */
int devo_upd_masked_gather(const void* src, const int64_t* idx, void* out, int64_t E, int dim, int dtype,
                           devo_stream_t stream);

/* SoftAgg reduction (blocks.py:42-43: torch_scatter.scatter_softmax + scatter_sum over dim 1): for every group s
 * (edges perm[seg_start[s] .. seg_start[s+1]), tables from devo_ba_prepare / devo_ba_prepared_tables on the group key,
 * *n_seg groups) y[s] = sum_e f[e] * softmax_over_group(g)[e], channel-wise.  group_of i32 [E] (optional) receives
 * the group index of every edge for devo_upd_expand_add.  f and g may be column blocks of one wider matrix (the two
 * Linear layers share their input: one GEMM): rows of stride ld_fg.  dim even, operands 8-byte aligned. */
int devo_upd_softagg(const void* f, const void* g, int64_t ld_fg /* row stride of f and g (>= dim) */, const int* perm,
                     const int* seg_start, const int* n_seg, void* y, int* group_of, int64_t E, int dim, int dtype,
                     devo_stream_t stream);
/* ... with the caller's estimate of the rows per group (E / groups; 0 = unknown): groups of >= 48 rows (DEVO's frame pairs) run on 16 waves per
 * workgroup instead of 4 (a wave's rows are a chain of dependent row latencies). */
int devo_upd_softagg_hint(const void* f, const void* g, int64_t ld_fg, const int* perm, const int* seg_start, const int* n_seg, void* y, int* group_of,
                          int64_t E, int dim, int dtype, int rows_per_group, devo_stream_t stream);

/* Adjoint of devo_upd_softagg for training (the backward of blocks.py:42-43's scatter_softmax * f -> scatter_sum): dy [n_seg, dim] ->
 * df, dg (rows of stride ld_d; every edge of every group is written):  d f_e = w_e dy,  d g_e = w_e dy (f_e - y),  w = softmax of g
 * over the edge's group, channel-wise.  Same tables and alignment rules as devo_upd_softagg. */
int devo_upd_softagg_backward(const void* f, const void* g, int64_t ld_fg, const int* perm, const int* seg_start, const int* n_seg,
                              const void* dy, void* df, void* dg, int64_t ld_d, int64_t E, int dim, int dtype, devo_stream_t stream);

/* net[e] += hy[group_of[e]]   — `net + h(y)[:, jx]` of blocks.py:46 / enet.py:93-94, in place. */
int devo_upd_expand_add(void* net, const void* hy, const int* group_of, int64_t E, int dim, int dtype,
                        devo_stream_t stream);

/* out = x + sigmoid(gate) * res   — GatedResidual (blocks.py:28-29) after its three Linear layers. */
int devo_upd_gated_residual(const void* x, const void* gate, int64_t ld_gate /* row stride of gate */, const void* res,
                            void* out, int64_t rows, int dim, int dtype, devo_stream_t stream);

/* Adjoint of devo_upd_gated_residual with respect to the gate pre-activation and res (d x = d out), training:
 * d gate = d out * res * s (1 - s),  d res = d out * s,  s = sigmoid(gate).  dgate / dres contiguous [rows, dim]. */
int devo_upd_gated_residual_backward(const void* gate, int64_t ld_gate, const void* res, const void* dout, void* dgate, void* dres,
                                     int64_t rows, int dim, int dtype, devo_stream_t stream);

/* net[e] = x[e] + sigmoid(gate[e]) * res[e] -> net_out (the last GatedResidual; gate == NULL: net = x, nothing stored),
 * then delta[e] = Wd relu(net[e]) + bd;  weight[e] = sigmoid(Ww relu(net[e]) + bw)   (Wd, Ww [2, dim]; enet.py:68-78). */
int devo_upd_heads(const void* x, const void* gate, int64_t ld_gate, const void* res, void* net_out, const void* Wd,
                   const void* bd, const void* Ww, const void* bw, void* delta, void* weight, int64_t E, int dim,
                   int dtype, devo_stream_t stream);

/* The Update operator's dense layers in fp32 storage on the fp16 matrix cores (csrc/linear.hip): y[M, N] = act(x[M, K] W^T + bias) [+ residual]
 * with every fp32 value split into fp16 hi + lo (2^-22 relative per factor, fp32 accumulation) — the 18 000 / 21 600-row Linear layers of
 * the update operator (enet.py:41-78, blocks.py:15-48) at half the fp32 library GEMM's time.  Both operands are scaled by exact powers
 * of two before the split (weight columns once per version; activation rows by a running scale inside the kernel), so gradient-sized
 * rows (1e-7) keep their 22 bits.  Any N and K (the corr MLP's first layer has K = 882, its dX 882 outputs, the heads 2): the kernel works
 * on column blocks of 96 and K steps of 32, the weight image carries zeros behind N and K.
 *   devo_upd_split_weight: the weight, element (n, k) at W[n * s_n + k * s_k] (s_n = K, s_k = 1: a Linear's [N, K] weight for the forward;
 *     s_n = 1, s_k = N_in: the same storage read as its transpose for dX = dY W), -> wsplit (devo_upd_split_weight_bytes(N, K) =
 *     ceil96(N) ceil32(K) 4 + ceil96(N) 4 bytes — the operand image over whole column blocks of 96, then the inverse column scales —,
 *     16-byte aligned; ALLOCATE WITH THE QUERY, the call takes no size): once per version of the weight.
 *   devo_upd_linear_split: x fp32, rows ldx >= K elements apart (any alignment of 4 bytes); y fp32, rows ldy >= N apart (16-byte pieces when
 *     ldy is a multiple of 4 and y / residual are 16-byte aligned, single values otherwise); bias fp32 [N] or NULL; residual NULL or fp32 with y's row pitch, added after the activation (it may be y itself:
 *     x.add_(linear(t)) in one launch); columns >= relu_from get max(., 0) (0: all of them, >= N: none — a gate | res pair of a
 *     GatedResidual in one launch); gate NULL or fp32 with y's row pitch: the result is kept where gate > 0 and zeroed elsewhere, before
 *     the residual — dX = (dY W) masked by the ReLU output it passes back through (threshold_backward in the epilogue). */
/* The update operator's Linear layers in fp16 storage, second structure (csrc/gemm_rs.hip; enet.py:41-78): a workgroup's rows live in LDS once,
 * the weights go from the L2 into the registers of the wave that multiplies them.  y[M, N] = act(x W^T + bias) [+ residual]; the ReLU applies from
 * column relu_from on (N: none); residual may be y.  N a multiple of 384, K in (352, 384] (devo_upd_rs_supported); x rows 4-byte aligned, y /
 * residual rows 16-byte aligned.  Weight image:
 * devo_upd_rs_pack_weight_f16 (devo_upd_rs_weight_bytes(N, K) bytes, 16-byte aligned), once per weight version. */
size_t devo_upd_rs_weight_bytes(int N, int K);
int devo_upd_rs_supported(int N, int K);
int devo_upd_rs_pack_weight_f16(const void* W /* f16, element (n, k) at W[n * s_n + k * s_k] */, int64_t s_n, int64_t s_k, int N, int K, void* wimage, void* stream);
int devo_upd_rs_linear_f16(const void* x, int64_t ldx, const void* wimage, const void* bias, const void* residual, void* y, int64_t ldy, int M, int N, int K,
                           int relu_from, void* stream);
/* What follows the frame-pair aggregation in the update operator as ONE launch, fp16 storage (enet.py:52-57, 96-99; blocks.py:29-48) — the rows
 * stay in LDS between the layers:  net = LN0(x + hy[group_of]);  net = LN2(net + sigmoid(gate1(net)) res1(net));
 * net_out = net + sigmoid(gate3(net)) res3(net);  delta = d(relu(net_out)), weight = sigmoid(w(relu(net_out))).
 * x, net_out [E, 384] contiguous, hy [groups, 384], delta / weight [E, 2]; wgr*: the [gate[0] | res[0]] weights concatenated to [768, 384], wr2_*:
 * res[2] [384, 384], both as devo_upd_rs_pack_weight_f16 images; bgr* [768], br2_* [384]; Wd / Ww [2, 384]; everything fp16, 16-byte aligned.
 * Every layer output and LayerNorm output is rounded to fp16 where the layer-by-layer path stores it. */
/* fp32 storage in the row-resident structure (csrc/gemm_rs.hip): devo_upd_linear_split's contract and arithmetic (fp32 in and out, every value an
 * exact fp16 hi + lo pair, power-of-two scales per row — the row's own largest magnitude — and per weight column), N a multiple of 384, K a multiple
 * of 4 in (352, 384] (devo_upd_rs_split_supported); x, y, residual, gate rows 16-byte aligned.  Weight image: devo_upd_rs_split_weight
 * (devo_upd_rs_split_weight_bytes(N, K) bytes, 16-byte aligned; element (n, k) at W[n * s_n + k * s_k]: the weight or its transpose view). */
size_t devo_upd_rs_split_weight_bytes(int N, int K);
int devo_upd_rs_split_supported(int N, int K);
int devo_upd_rs_split_weight(const float* W, int64_t s_n, int64_t s_k, int N, int K, void* wimage, void* stream);
int devo_upd_rs_linear_split(const float* x, int64_t ldx, const void* wimage, const float* bias, const float* residual, const float* gate, float* y, int64_t ldy,
                             int M, int N, int K, int relu_from, void* stream);
/* l2(relu(l1(x[gather]))) [+ residual] as one launch with the rows resident in LDS, both layers 384 -> 384 (enet.py:46-50, 86-91: c1 / c2 with
 * their neighbour gather and the sum).  x rows 16-byte aligned (ldx a multiple of 8), residual / y [M, 384] contiguous; gather i64 [M] (negative or
 * >= x_rows: a zero row) or null; weight images of devo_upd_rs_pack_weight_f16; biases 8-byte aligned. */
int devo_upd_rs_mlp2_f16(const void* x, int64_t ldx, int x_rows, const int64_t* gather, const void* w1image, const void* b1, const void* w2image, const void* b2,
                         const void* residual, void* y, int M, void* stream);
/* ... and, on the result rows still in LDS, the 768-wide f | g layer of the SoftAgg that follows (blocks.py:36-40): fg [M, 768] = y [Wf | Wg]^T + [bf | bg]
 * (wfg: the image of the concatenated [768, 384] weight; wfg / bfg / fg all or none). */
int devo_upd_rs_mlp2_fg_f16(const void* x, int64_t ldx, int x_rows, const int64_t* gather, const void* w1image, const void* b1, const void* w2image, const void* b2,
                            const void* residual, void* y, int M, const void* wfg_image, const void* bfg, void* fg, void* stream);
/* x += hy[group_of] (the expand-add behind a SoftAgg, enet.py:93; in place, rounded to fp16 like devo_upd_expand_add) and the f | g layer of the
 * SoftAgg that follows on the same rows, one launch: x [M, 384] contiguous, hy [groups, 384], fg [M, 768]. */
int devo_upd_rs_expand_fg_f16(void* x, const void* hy, const int* group_of, const void* wfg_image, const void* bfg, void* fg, int M, void* stream);
/* The correlation branch and the first LayerNorm of the update operator as ONE launch, fp16 storage (enet.py:59-66, 82-83):
 *   c = l5(relu(LN3(l2(relu(l0(corr))))));  out = LN(net + inp + c).   corr [E, K0], 864 < K0 <= 896 (28 K steps of 32; DEVO: 882), rows 4-byte aligned; net / inp / out
 * [E, 384] contiguous; weight images of devo_upd_rs_pack_weight_f16 ([384, K0], [384, 384], [384, 384]); vectors fp16, 16-byte aligned. */
int devo_upd_rs_corr_f16(const void* corr, int64_t ldc, int K0, const void* w0image, const void* b0, const void* w2image, const void* b2, const void* ln3_w,
                         const void* ln3_b, float eps3, const void* w5image, const void* b5, const void* net, const void* inp, const void* ln_w, const void* ln_b,
                         float eps, void* out, int E, void* stream);
/* ... with `net` as fp32 [E, 384] (the recurrent state as autocast keeps it): it enters net + inp + c unrounded, no conversion pass in front. */
int devo_upd_rs_corr_f16_net32(const void* corr, int64_t ldc, int K0, const void* w0image, const void* b0, const void* w2image, const void* b2, const void* ln3_w,
                               const void* ln3_b, float eps3, const void* w5image, const void* b5, const float* net, const void* inp, const void* ln_w, const void* ln_b,
                               float eps, void* out, int E, void* stream);
int devo_upd_rs_gru_f16(const void* x, const void* hy, const int* group_of, const void* ln0_w, const void* ln0_b, float eps0, const void* wgr1_img,
                        const void* bgr1, const void* wr2_1_img, const void* br2_1, const void* ln2_w, const void* ln2_b, float eps2, const void* wgr3_img,
                        const void* bgr3, const void* wr2_3_img, const void* br2_3, const void* Wd, const void* bd, const void* Ww, const void* bw,
                        void* net_out, void* delta, void* weight, int E, void* stream);
/* ... with net_out as fp32 [E, 384]: the values the fp16 form stores, widened — what devo.py:311's call under autocast returns (the recurrent
 * state stays fp32 there), without a conversion pass behind the launch. */
int devo_upd_rs_gru_f16_out32(const void* x, const void* hy, const int* group_of, const void* ln0_w, const void* ln0_b, float eps0, const void* wgr1_img,
                              const void* bgr1, const void* wr2_1_img, const void* br2_1, const void* ln2_w, const void* ln2_b, float eps2, const void* wgr3_img,
                              const void* bgr3, const void* wr2_3_img, const void* br2_3, const void* Wd, const void* bd, const void* Ww, const void* bw,
                              float* net_out, void* delta, void* weight, int E, void* stream);

/* Linear - ReLU - Linear of the update operator as ONE launch, fp16 storage / fp32 accumulation (csrc/mlp2.hip; enet.py:46-50 c1 / c2,
 * :59-61 the corr MLP's first two layers): y[r] = (residual[r] +) W2 relu(W1 x[src(r)] + b1) + b2 with both layers 384 wide, any K1 (W1 is
 * [384, K1]); src(r) = r, or gather[r] (i64 [M]; negative = a zero row: `mask * net[:, ix]`).  The 384-wide intermediate stays in LDS, rounded
 * to fp16 like the two-launch form's.  Weight images: devo_upd_mlp2_pack_weight (devo_upd_mlp2_weight_bytes(K) bytes, 16-byte aligned), once per
 * version of a weight.  x: rows ldx elements apart (even), x_rows of them; y / residual: rows ldy apart (multiple of 8), 16-byte aligned; y must
 * not alias x when gather is given. */
size_t devo_upd_mlp2_weight_bytes(int K);
int devo_upd_mlp2_pack_weight(const void* W /* f16, element (n, k) at W[n * s_n + k * s_k], n < 384 */, int64_t s_n, int64_t s_k, int K, void* wimage,
                              devo_stream_t stream);
int devo_upd_mlp2_f16(const void* x, int64_t ldx, int x_rows, const int64_t* gather, const void* w1image, const void* b1, int K1, const void* w2image,
                      const void* b2, const void* residual, void* y, int64_t ldy, int M, devo_stream_t stream);

size_t devo_upd_split_weight_bytes(int N, int K);
int devo_upd_split_weight(const float* W, int64_t s_n, int64_t s_k, int N, int K, void* wsplit, devo_stream_t stream);
int devo_upd_linear_split(const float* x, int64_t ldx, const void* wsplit, const float* bias, const float* residual, const float* gate, float* y,
                          int64_t ldy, int M, int N, int K, int relu_from, devo_stream_t stream);

/* The same workgroup shape for fp16 storage — the update operator's inference precision (devo.py:71-77: autocast): y[M, N] (fp16) =
 * act(x[M, K] W^T + bias) [+ residual], fp32 accumulation, one MFMA per block (no split, no scales), K steps of 64.
 *   devo_upd_pack_weight_f16: W fp16, element (n, k) at W[n * s_n + k * s_k] -> wimage (devo_upd_pack_weight_f16_bytes(N, K) = N ceil64(K) 2
 *     bytes, 16-byte aligned): the B-operand image, once per version of the weight.
 *   devo_upd_linear_f16: x fp16 rows ldx >= K elements apart (a multiple of 2, 4-byte aligned), y / residual fp16 rows ldy apart (a
 *     multiple of 4, 8-byte aligned), bias fp16 [N] or NULL; relu_from / residual as devo_upd_linear_split.  N % 96 == 0, any K. */
size_t devo_upd_pack_weight_f16_bytes(int N, int K);
int devo_upd_pack_weight_f16(const void* W, int64_t s_n, int64_t s_k, int N, int K, void* wimage, devo_stream_t stream);
int devo_upd_linear_f16(const void* x, int64_t ldx, const void* wimage, const void* bias, const void* residual, void* y, int64_t ldy, int M,
                        int N, int K, int relu_from, devo_stream_t stream);

/* The third product of a Linear layer's training step (csrc/linear_dw.hip): dW[No, Ni] = dY[R, No]^T X[R, Ni] and db[No] = the column sums of
 * dY (db may be NULL), fp32 in and out on the fp16 matrix cores like devo_upd_linear_split (exact hi + lo splits, per-column running
 * power-of-two scales) — what torch.autograd computes for the reference's nn.Linear layers (enet.py:41-78, blocks.py:15-48) as
 * `grad_output.t() @ input` and `grad_output.sum(0)`.  Any No, Ni and row pitches (the kernel works on 128 x 128 blocks: the corr MLP's 882
 * inputs are 7 block columns, the last one masked); tensors 4-byte aligned, the workspace (devo_upd_dw_workspace_bytes(R, No, Ni) bytes:
 * the row slices' partial blocks — no atomics, reproducible) 16-byte aligned. */
size_t devo_upd_dw_workspace_bytes(int R, int No, int Ni);
int devo_upd_dw_split(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, int R, int No, int Ni, void* workspace, float* dW,
                      int64_t ld_dw, float* db, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Event voxelisation — the step in front of the encoders.
 * ---------------------------------------------------------------------------------------------- */

/* to_voxel_grid (utils/event_utils.py:180-232): N events (x, y f32 pixel coordinates, t f64 ascending timestamps,
 * p i8 polarity with 0 meaning -1) vote trilinearly into grid f32 [bins, H, W] (zeroed here; corners outside are
 * dropped).  Weights in fp64 like the reference, accumulation with fp32 atomics (order differs: fp32 rounding). */
int devo_voxelize(const float* xs, const float* ys, const double* ts, const signed char* ps, int64_t N, int H, int W,
                  int bins, float* grid, devo_stream_t stream);

/* std (utils/voxel_utils.py:6-28, devo/devo.py:438-452), in place: vox f32 [nseg, len] — nseg = b (sequence-wise) or
 * b*n (frame-wise); every segment's NON-ZERO entries are standardised with the mean / stddev of those entries; nothing
 * is changed if any segment has no non-zero entry.  ws: devo_voxel_std_workspace_bytes(nseg). */
size_t devo_voxel_std_workspace_bytes(int nseg);
int devo_voxel_std(float* vox, int nseg, int64_t len, void* ws, size_t ws_bytes, devo_stream_t stream);

/* The event front end of the loaders (utils/load_utils.py:47-76: EventSlicer.get_events -> rectify_map[y, x] -> to_voxel_grid
 * -> trafos) for S windows of ONE stream in one call.  Events: ts ascending, f64 (ts_i64 = 0) or int64 microseconds (ts_i64 = 1);
 * p i8 with 0 meaning -1.  Window s holds the events with t0[s] <= t < t1[s] (EventSlicer's rule; t0, t1 f64 device arrays
 * of S) and is voxelised into out[s] (f32 [S, bins, H, W], zeroed here) with its time axis normalised by its own first and
 * last event.  rectify_map f32 [H, W, 2] or NULL: when given, xs / ys are raw int32 sensor coordinates and the event votes
 * at map[y, x] (an event outside the sensor is dropped); when NULL, xs / ys are f32 coordinates.  counts (int64 [S], may be
 * NULL) receives every window's event count.  The window bounds are found on the device: no host synchronisation.
 * ws: devo_voxelize_windows_workspace_bytes(S). */
size_t devo_voxelize_windows_workspace_bytes(int S);
int devo_voxelize_windows(const void* xs, const void* ys, const void* ts, int ts_i64, const signed char* ps, int64_t N, const double* t0,
                          const double* t1, int S, const float* rectify_map, int H, int W, int bins, float* out, int64_t* counts, void* ws,
                          size_t ws_bytes, devo_stream_t stream);

/* RemoveHotPixelsVoxel(num_stds) (utils/event_utils.py:235-262), in place: vox f32 [nseg, len]; per segment the mean and the
 * unbiased std of ALL len entries (fp64), then every entry with |v| > mean + num_stds * std is set to 0.
 * ws: devo_voxel_hot_pixels_workspace_bytes(nseg). */
size_t devo_voxel_hot_pixels_workspace_bytes(int nseg);
int devo_voxel_hot_pixels(float* vox, int nseg, int64_t len, double num_stds, void* ws, size_t ws_bytes, devo_stream_t stream);

/* rescale (utils/voxel_utils.py:31-51): out = vox with positive entries divided by the largest positive entry and negative
 * entries divided by minus the smallest negative entry, both over all n entries; a sign with no entry is left unchanged.
 * out may equal vox.  ws: devo_voxel_rescale_workspace_bytes(). */
size_t devo_voxel_rescale_workspace_bytes(void);
int devo_voxel_rescale(const float* vox, float* out, int64_t n, void* ws, size_t ws_bytes, devo_stream_t stream);

/* voxel_augment / _augment (utils/voxel_utils.py:55-136) with torchvision 0.13's uint8 tensor ops: vox f32 [nseg, nimg, H, W]
 * (a sequence of nimg = n * bins images) -> out f32, same shape, a separate buffer.  rescale != 0: vox is rescaled first (as
 * devo_voxel_rescale, on the fly).  Every voxel becomes R = (uint8)(255 * max(-v, 0)), G = 0, B = (uint8)(255 * max(v, 0)), the op
 * is applied per image, and out = B' / 255 - R' / 255.  op: 0 adjust_brightness, 1 adjust_contrast, 2 invert, 3 posterize,
 * 4 adjust_saturation, 5 adjust_sharpness, 6 solarize; factor: the blend ratio (ops 0, 1, 4, 5), the bits (3), the threshold (6),
 * unused (2).  standardise != 0: std(out) sequence-wise (devo_voxel_std's rule; nothing changes if a segment has no non-zero
 * voxel), from exact integer statistics.  The result does not depend on the launch shape.  No host synchronisation; the
 * workspace is cleared by a kernel (graph capture safe).  ws: devo_voxel_augment_workspace_bytes(nseg, nimg). */
size_t devo_voxel_augment_workspace_bytes(int nseg, int nimg);
int devo_voxel_augment(const float* vox, float* out, int nseg, int nimg, int H, int W, int rescale, int op, double factor, int standardise,
                       void* ws, size_t ws_bytes, devo_stream_t stream);

/* The tail of a training sample (devo/data_readers/base.py:356-371): transform_rescale's resize and EVSDAugmentor's jitter, zoom and
 * centre crop, then the depth normalisation.  ATen's CPU arithmetic (torch 2.10), FMAs where its build contracts and nowhere else.
 * devo_voxel_resample: src f32 [B, C, H, W] -> dst f32 [B, C, Hc, Wc] (contiguous, separate buffers).  params: HOST int [B][4] =
 * (Hs, Ws, y0, x0): sample b is resized to Hs x Ws (mode DEVO_RESAMPLE_BILINEAR: upsample_bilinear2d, align_corners=False, no
 * explicit scale; DEVO_RESAMPLE_NEAREST: nearest_idx) and only rows y0 .. y0 + Hc - 1, columns x0 .. x0 + Wc - 1 of it are
 * computed (0 <= y0, y0 + Hc <= Hs, likewise x).  Jitter v + ((u - 0.5) * 2) * 1e-4 on every source tap before interpolation:
 * u = noise[same index as the tap] when noise (device, src's shape) is given, else, when seeds (HOST uint64 [B]) is given, a
 * 24-bit uniform hashed from (seeds[b], the tap's index within sample b); neither: no jitter.  Samples go DEVO_RESAMPLE_MAX_BATCH
 * to a launch, with their parameters as kernel arguments (nothing is copied to the device).  C * H * W < 2^32. */
#define DEVO_RESAMPLE_MAX_BATCH 64
enum { DEVO_RESAMPLE_BILINEAR = 0, DEVO_RESAMPLE_NEAREST = 1 };
int devo_voxel_resample(const float* src, float* dst, int B, int C, int H, int W, int Hc, int Wc, const int* params, int mode, const float* noise,
                        const uint64_t* seeds, devo_stream_t stream);

/* The depth normalisation of __getitem__ for B samples of n disparities each (disps f32 [B, n], in place): s = factor *
 * torch.quantile(disps[b], q) exactly as torch computes it for fp32 input (rank q * (n - 1) in fp32, the last index if a NaN is
 * present, ATen's lerp; NaN sorts last), then disps[b] /= s, poses[b, p, 0:3] *= s for poses f32 [B, P, pose_stride] (may be NULL)
 * and s_out[b] = s (may be NULL).  Exact radix select; no size limit below 2^31.  No host synchronisation; the workspace
 * (devo_depth_normalise_workspace_bytes(B)) is cleared by a kernel (graph capture safe). */
size_t devo_depth_normalise_workspace_bytes(int B);
int devo_depth_normalise(float* disps, int64_t n, int B, float* poses, int P, int pose_stride, float q, float factor, float* s_out, void* ws,
                         size_t ws_bytes, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The patch graph of DEVO's inference (devo/devo.py:225-239 append_factors / remove_factors, :258-265 motionmag, :267-306 keyframe):
 * edge lists ii (source frame), jj (target frame), kk (patch) i64 [E] and the recurrent state net T [1, E, dim] (fp16 or fp32, dim a
 * multiple of 8, 16-byte aligned: rows move as 16-byte words).  ws: devo_graph_workspace_bytes(capacity) serves every call on a
 * graph of up to `capacity` edges; calls that share a workspace must be enqueued on one stream.  `record` is a HOST-VISIBLE word
 * (pinned host memory, device-addressable at its own address) of DEVO_GRAPH_RECORD_BYTES = {i32 removed, i32 n_edges, f32 mean_ij,
 * f32 mean_ji}, written by the last kernel of the call; the caller records an event behind the call and waits for that.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_GRAPH_RECORD_BYTES 16
#define DEVO_GRAPH_SHIFT_MAX 8
size_t devo_graph_workspace_bytes(int capacity);

/* motionmag(i, j) and motionmag(j, i) (devo.py:258-265) in one pass over all edges: the mean of pops.flow_mag(beta) over the edges
 * with (ii, jj) == (i, j) -> record.mean_ij, over those with (ii, jj) == (j, i) -> record.mean_ji; NaN where there is no such edge.
 * poses f32 [n_poses, 7], patches f32 [n_patches, 3, P, P], intrinsics f32 [n_poses, 4]; an edge whose indices fall outside them
 * is skipped.  Reproducible from run to run (no float atomics).  record.removed = 0, record.n_edges = E. */
int devo_graph_motion(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                      int n_poses, int n_patches, int P, int i, int j, float beta, void* ws, size_t ws_bytes, void* record, devo_stream_t stream);

/* The graph half of DEVO.keyframe (devo.py:267-287, :305-306) with the decision taken on the device: k = n - keyframe_index,
 * m = double(motionmag(k - 1, k + 1)) + double(motionmag(k + 1, k - 1)); if m / 2 < thresh (false for NaN) the edges with ii == k or
 * jj == k are dropped, the survivors renumbered (kk -= M where ii > k, then ii -= 1; jj -= 1 where jj > k) and n' = n - 1, else
 * n' = n; then the edges with ix[kk] < n' - removal_window go (kk as renumbered; ix i64 [ix_len], a kk outside it keeps its edge).
 * Survivors keep their order (a stable compaction) and land in ii_out / jj_out / kk_out / net_out, which must hold E entries / rows
 * and must not alias the inputs.  record: {removed, number of survivors, mean_ij, mean_ji}. */
int devo_graph_keyframe(const float* poses, const float* patches, const float* intrinsics, const int64_t* ii, const int64_t* jj, const int64_t* kk,
                        const void* net, const int64_t* ix, int64_t* ii_out, int64_t* jj_out, int64_t* kk_out, void* net_out, int E, int n_poses,
                        int n_patches, int64_t ix_len, int P, int dim, int net_dtype, int M, int n, int keyframe_index, double thresh,
                        int removal_window, float beta, void* ws, size_t ws_bytes, void* record, devo_stream_t stream);

/* remove_factors(mask) (devo.py:235-239): the same stable compaction with a caller's mask (u8 / bool [E], non-zero = drop).
 * record: {0, number of survivors, 0, 0}. */
int devo_graph_remove(const int64_t* ii, const int64_t* jj, const int64_t* kk, const void* net, const unsigned char* mask, int64_t* ii_out,
                      int64_t* jj_out, int64_t* kk_out, void* net_out, int E, int dim, int net_dtype, void* ws, size_t ws_bytes, void* record,
                      devo_stream_t stream);

/* append_factors (devo.py:225-233), one launch: ii / jj / kk are buffers of `capacity` entries holding E edges; entries E .. E + n_new - 1
 * become ii = ix[patch_ids] (-1 for a patch outside ix), jj = frame_ids, kk = patch_ids; net_new [E + n_new, dim] = the E rows of
 * net_old followed by zero rows.  E + n_new > capacity is an error (nothing is launched). */
int devo_graph_append(int64_t* ii, int64_t* jj, int64_t* kk, const void* net_old, void* net_new, const int64_t* ix, int64_t ix_len,
                      const int64_t* patch_ids, const int64_t* frame_ids, int E, int n_new, int capacity, int dim, int net_dtype, devo_stream_t stream);

/* The window edges of a new frame (devo.py:366-380 followed by both append_factors calls of :541-542), ONE launch, for a state of n >= 1
 * frames of M patches (after the increment of :537), r = lifetime >= 1: first the forward edges, patches M max(n - r, 0) .. M (n - 1) - 1
 * -> frame n - 1, then the backward edges, patches M (n - 1) .. M n - 1 -> frames max(n - r, 0) .. n - 1 (patch-major: flatmeshgrid's
 * `ij` order); ii = ix[kk] (-1 for a patch outside ix); net_new as in devo_graph_append.  devo_odom_append_frame_edges: how many
 * edges that is (0 for arguments outside their ranges).  E + edges > capacity is an error (nothing is launched). */
int64_t devo_odom_append_frame_edges(int M, int n, int lifetime);
int devo_odom_append_frame(int64_t* ii, int64_t* jj, int64_t* kk, const void* net_old, void* net_new, const int64_t* ix, int64_t ix_len, int M, int n,
                            int lifetime, int E, int capacity, int dim, int net_dtype, devo_stream_t stream);

/* The frame shift of keyframe removal (devo.py:289-295) for up to DEVO_GRAPH_SHIFT_MAX tensors of any dtype in one launch: tensor s
 * is `tensors[s]` (HOST array of device pointers), contiguous, with rows of row_bytes[s] (HOST array) bytes; rows k + 1 .. n - 1 of
 * each move down by one (row r <- row r + 1 for r = k .. n - 2, in place). */
int devo_graph_shift_frames(void* const* tensors, const int64_t* row_bytes, int count, int k, int n, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The per-frame state of DEVO's inference between the update step, the Patchifier and the patch graph: the frame store with the
 * motion model and the depth initialisation (devo/devo.py:487-488, :502-520), the point cloud behind every update (:342-344) and
 * the relative-pose log with terminate() (:179-196, :276-280, :534).  poses f32 [N, 7], patches f32 [N, M, 3, P, P], intrinsics
 * f32 [N, 4], tstamps i64 [N]: the caller's frame buffers (devo.py:56-65).  `status` is a HOST-VISIBLE i32 (pinned host memory,
 * device-addressable at its own address): 0, or the DEVO_FRAME_STATUS_* code of the last error a kernel met; the caller clears it.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_FRAME_MEDIAN_MAX 32768      /* depth values the median of devo_frame_begin selects from: 3 M P P */
enum { DEVO_FRAME_COPY_LAST = 0, DEVO_FRAME_DAMPED_LINEAR = 1 };
enum { DEVO_FRAME_STATUS_BAD_ENTRY = 1,  /* a log entry whose frame lies outside the capacity or whose parent is not an earlier frame */
       DEVO_FRAME_STATUS_MISSING = 2,    /* a frame below `counter` that is no keyframe and that no chain of entries ties to one */
       DEVO_FRAME_STATUS_UNSORTED = 3 }; /* tstamps[:n] is not strictly increasing */

/* Row n of the four buffers, ONE launch; no other row is written.
 *   poses[n]      n > 1: Exp(damping * Log(P[n-1] P[n-2]^-1)) P[n-1] for DEVO_FRAME_DAMPED_LINEAR, a copy of row n - 1 for
 *                 DEVO_FRAME_COPY_LAST; n <= 1: untouched (devo.py:502-512).
 *   patches[n]    channels 0 and 1 from new_patches f32 [M, 3, P, P]; channel 2 = depth[patch] (depth f32 [M]) or, with depth == NULL,
 *                 the LOWER median of patches[n-3 : n, :, 2] — the value of rank (3 M P P - 1) / 2, what torch.median returns; an exact
 *                 selection (-0 orders below +0; NaN if there is one).  Needs n >= 3 and 3 M P P <= DEVO_FRAME_MEDIAN_MAX: beyond it
 *                 DEVO_ERR_UNSUPPORTED is returned and nothing is launched.
 *   intrinsics[n] new_intrinsics f32 [4] / res, a correctly rounded division;  tstamps[n] = counter. */
int devo_frame_begin(float* poses, float* patches, float* intrinsics, int64_t* tstamps, int N, int M, int P, int n, const float* new_patches,
                     const float* new_intrinsics, int64_t counter, float res, int motion_model, float damping, const float* depth,
                     devo_stream_t stream);

/* out f32 [>= m, 3], rows start_frame * M .. m - 1: the centre pixel (P/2, P/2) of patch k through X = G[ix[k]]^-1 ((x - cx) / fx,
 * (y - cy) / fy, 1, d), out[k] = X[:3] / X[3] (devo.py:342-344; NaN where ix[k] names no frame).  ONE launch; other rows are not touched. */
int devo_frame_point_cloud(const float* poses, const float* patches, const float* intrinsics, const int64_t* ix, int n_poses, int n_patches, int64_t ix_len,
                           int P, int M, int m, int start_frame, float* out, devo_stream_t stream);

/* The log of terminate(): parent i64 [capacity] (-1: no entry), rel f32 [capacity, 7].
 * record_removed (devo.py:276-280, BEFORE the frame buffers shift): t0 = tstamps[k-1], t1 = tstamps[k] read on the device,
 * parent[t1] = t0, rel[t1] = P[k] P[k-1]^-1.  record_skipped (devo.py:534): parent[t] = t0, rel[t] = identity.  One launch each. */
int devo_frame_record_removed(const float* poses, const int64_t* tstamps, int n_poses, int k, int64_t* parent, float* rel, int capacity, int* status,
                              devo_stream_t stream);
int devo_frame_record_skipped(int64_t t, int64_t t0, int64_t* parent, float* rel, int capacity, int* status, devo_stream_t stream);

/* terminate() (devo.py:186-196): out f32 [counter, 7] = the INVERSE of pose(t), pose(tstamps[i]) = poses[i] for i < n (a keyframe wins
 * over a log entry; tstamps[:n] strictly increasing, as the state machine keeps it), pose(t) = rel[t] pose(parent[t]) otherwise.
 * Parallel pointer jumping, 1 + ceil(log2(counter)) launches (devo_frame_complete_launches), no bound on the depth of a chain.
 * ws: devo_frame_complete_workspace_bytes(counter).  counter > capacity: DEVO_ERR_ARG. */
size_t devo_frame_complete_workspace_bytes(int counter);
int devo_frame_complete_launches(int counter);
int devo_frame_complete(const float* poses, const int64_t* tstamps, int n, int counter, const int64_t* parent, const float* rel, int capacity, float* out,
                        void* ws, size_t ws_bytes, int* status, devo_stream_t stream);

/* A new voxel grid on its way to the Patchifier (devo.py:406-467), TWO launches, no host wait.  vox: fp32 or fp16 [bins, H, W];
 * out: f32 [bins, H, W'], W' = W - 2 for W == DEVO_INPUT_CROP_WIDTH (columns 1 .. W - 2 are kept; the statistics are taken over all W
 * columns, as the reference normalises before it crops), else W.
 *   DEVO_INPUT_NONE     out = x.
 *   DEVO_INPUT_RESCALE  positives divided by the largest positive, negatives by minus the smallest negative (correctly rounded fp32
 *                       divisions); a polarity without entries changes nothing.
 *   DEVO_INPUT_STD      with nnz = #(x != 0) > 0: out = (x - mean) / sigma on the non-zero voxels and 0 elsewhere, mean = sum x / nnz and
 *                       sigma^2 = sum x^2 / nnz - mean^2 formed in fp64 and rounded to fp32 once, the difference and the quotient in fp32;
 *                       nnz == 0: out = x.  Where all non-zero voxels are equal the result is devo_voxel_std's for that grid.
 * record: 4 HOST-VISIBLE doubles (pinned host memory): {nnz, bins H W, c0, c1}, (c0, c1) = (mean, sigma) as fp32 values under STD, (largest
 * positive, largest -negative) under RESCALE, zeros under NONE; valid once the work enqueued on `stream` so far has run.  Sums are fp64 in
 * an order fixed by bins H W: the same bits from run to run.  ws: devo_odom_input_workspace_bytes(bins H W). */
enum { DEVO_INPUT_NONE = 0, DEVO_INPUT_RESCALE = 1, DEVO_INPUT_STD = 2 };
#define DEVO_INPUT_CROP_WIDTH 346
size_t devo_odom_input_workspace_bytes(int64_t numel);
int devo_odom_input(const void* vox, int dtype, int bins, int H, int W, int norm, float* out, void* ws, size_t ws_bytes, double* record,
                     devo_stream_t stream);

/* The motion probe's median (devo.py:256), ONE workgroup: out[0] = torch.quantile(delta.norm(dim=-1).float(), 0.5) for delta fp32 or fp16
 * [M, 2], 1 <= M <= DEVO_PROBE_MEDIAN_MAX (beyond it DEVO_ERR_UNSUPPORTED, nothing is launched).  The norms are formed in fp64 from the
 * exactly converted input and rounded to fp32; an exact selection; for even M the mean of the two middle values, formed in fp64 and rounded
 * once; NaN if there is one.  out: f32, device or host-visible memory. */
#define DEVO_PROBE_MEDIAN_MAX 1024
int devo_odom_probe_median(const void* delta, int dtype, int M, float* out, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The training loss of one update iteration (train.py:172-236 and the metrics of :254-266); T = fp32 or fp64 throughout.
 *   flow term   x, y T [Ec, P, P, 2] (p_ij and its ground truth over the close edges), v T [Ec]: the mean over the edges with v > 0.5
 *               of the smallest of the P x P residual norms (NaN when there is none); px1 = the share of ALL pixels below 0.25.
 *   pose term   Gs, Ps T [n, 7], 2 <= n <= DEVO_LOSS_MAX_POSES: both inverted, the prediction's translations scaled by
 *               s = min(Var(t2) / sum of the singular values of cov(t2, t1), 10) (kabsch_umeyama, :54-65; fp64, no reflection
 *               correction, a constant for the adjoint), e1 = log(dP dG^-1) over the n (n - 1) ordered pairs, tr / ro = mean norms.
 *   scorer term (scores != NULL; the last iteration) scores T [n_patches]; v_full T [Ef], x_full, y_full T [Ef, P, P, 2],
 *               ba_weights T [Ef, 2], kk i64 [Ef]: mean over the edges with v_full >= 0.5 of (-log(mean w) / 2 + 1) * scores[kk] * min
 *               residual + mean(-log(max(scores, 1e-6))).  deterministic != 0: the adjoint's scatter over kk in a fixed order, else atomics.
 * loss T [1] = flow_weight * flow + scores_weight * scorer (+ pose_weight * pose when use_pose != 0).
 * stats f32 [DEVO_LOSS_STATS] = {flow, pose, tr, ro, px1, r1, r2, t1, t2, scores, scale}.
 * state: devo_loss_state_bytes(Ec, n, Ef, n_patches, dtype) bytes (Ef = n_patches = 0 without the scorer term), 16-byte aligned;
 * the partial sums and the adjoints of the three terms for a unit incoming gradient.  It belongs to this call until its backward has run.
 * Launches: forward 2 (+ 2 with the scorer term), backward 1.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_LOSS_STATS 11
#define DEVO_LOSS_AUX 8
#define DEVO_LOSS_MAX_POSES 128
size_t devo_loss_state_bytes(int Ec, int n, int Ef, int n_patches, int dtype);
int devo_loss_forward(const void* x, const void* y, const void* v, int Ec, int P, const void* Gs, const void* Ps, int n, const void* scores, int n_patches,
                      const void* v_full, const void* x_full, const void* y_full, const void* ba_weights, const int64_t* kk, int Ef, int deterministic,
                      double flow_weight, double pose_weight, double scores_weight, int use_pose, void* loss, float* stats, void* state, size_t state_bytes,
                      int dtype, devo_stream_t stream);
/* g T [1] (the gradient arriving at loss) and the state of the forward call with the same sizes and weights (pose_weight = 0 where the
 * pose term was not weighted in) -> g_coords T [Ec, P, P, 2] (every element written), g_Gs T [n, 7] (lietorch's embedding: the tangent
 * in the first six), g_scores T [n_patches]; each may be NULL. */
int devo_loss_backward(const void* g, const void* state, size_t state_bytes, int Ec, int P, int n, int Ef, int n_patches, double flow_weight, double pose_weight,
                       double scores_weight, void* g_coords, void* g_Gs, void* g_scores, int dtype, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The growing patch graph of the training loop (devo/enet.py:297-339 and the edge selections of :359-369; csrc/train_graph.hip;
 * devo_amd/train_graph.py).  Patches are frame-major, M per frame.  An index buffer holds three rows of `cap` int64 each (ii, jj, kk),
 * a list buffer four (position in the edge list, ii, jj, kk): close = the edges with 0 < |ii - jj| <= 2, far = those with <= 16, in
 * edge order.  Every total is host arithmetic (the caller passes E_new); every store is guarded by its buffer's capacity.
 * ws: devo_train_graph_workspace_bytes(capacity in edges).  Nothing waits for the device.
 *   init   the graph flatmeshgrid(where(ix < init_frames), arange(init_frames)) in closed form and its lists.  2 launches.
 *   grow   the growth to frame n (1 <= n < N <= DEVO_TRAIN_GRAPH_MAX_FRAMES): dst = [(p, n) for patches p of frames < n] +
 *          [(p, j) for patches p of frame n, j in 0..n] + src, then (drop != 0) the stable compaction that keeps ii != n - 4 and
 *          jj != n - 4; net_new T [E_new, dim] = zero rows for the new edges, the old rows behind them, compacted alike (fp16 / fp32,
 *          dim a multiple of 8, 16-byte aligned); map i32 [E_old] (needed under a drop, else may be NULL): the new row of an old row
 *          or -1; poses_out f32 [N, 7] = poses_in with row n = row n - 1; patches_out f32 [N M, 3, P, P] = patches_in with channel 2
 *          of frame n = the lower median of channel 2 of frames n - 2 and n - 1 (2 M P P <= DEVO_FRAME_MEDIAN_MAX values; NaN if
 *          there is one); the lists of dst.  Outputs never alias inputs.  3 launches.
 *   net_backward   grad_old T [E_old, dim] = 0 + grad_new[map] (zero where map < 0; the sum turns -0 into +0, as the torch composition's
 *          index_put_(accumulate) does).  1 launch.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_TRAIN_GRAPH_MAX_FRAMES 64
size_t devo_train_graph_workspace_bytes(int capacity);
int devo_train_graph_init(int64_t* idx, int64_t idx_cap, int M, int init_frames, int64_t* close, int64_t close_cap, int64_t* far_, int64_t far_cap,
                          void* ws, size_t ws_bytes, devo_stream_t stream);
int devo_train_graph_grow(const int64_t* src_idx, int64_t src_cap, int E_old, int64_t* dst_idx, int64_t dst_cap, int E_new, int M, int n, int drop,
                          const void* net_old, void* net_new, int dim, int net_dtype, int* map, const float* poses_in, float* poses_out, int N,
                          const float* patches_in, float* patches_out, int P, int64_t* close, int64_t close_cap, int64_t* far_, int64_t far_cap, void* ws,
                          size_t ws_bytes, devo_stream_t stream);
int devo_train_graph_net_backward(const void* grad_new, const int* map, void* grad_old, int E_old, int E_new, int dim, int net_dtype, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The training frame graph of one scene (devo/data_readers/base.py:263-286 over rgbd_utils.py:104-141; csrc/frame_graph.hip;
 * devo_amd/frame_graph.py): the mean induced-flow magnitude between all pairs of N frames on subsampled h x w maps, and the neighbour
 * lists below a flow threshold.  All tensors fp32 unless stated, contiguous.  ws: devo_frame_graph_workspace_bytes of (N, h, w), the same
 * buffer for distances and lists (0 for sizes that are refused).  No atomics: every result is bit-reproducible.
 *   N <= DEVO_FRAME_GRAPH_MAX_FRAMES = 32768: the workspace holds two N x N arrays of 4-byte sums and the caller an N x N matrix; at
 *          32768 each is 4 GiB (12 GiB together), N^2 = 2^30 keeps every list length and degree sum far inside 32 + 64-bit
 *          arithmetic, and N / 64 target blocks stay inside the grid's second dimension.  Pair indices are 64-bit throughout.
 *   2 h w < DEVO_FRAME_GRAPH_MAX_POINTS = 2^20: below it the integer rule 10 (V_ij + V_ji) < 7 * 2 h w agrees with the reference's fp32
 *          `val.mean(-1) < 0.7` for every count (the tie V = 0.7 * 2 h w stays finite); larger maps: DEVO_ERR_UNSUPPORTED.
 *   disps      depths [N, h, w] (already subsampled) -> disps = 1 / depth, where every depth below 0.01 is first replaced by the mean of
 *              its frame (taken over all h w values before any replacement; fp64 partial sums in a fixed order).  1 launch.
 *   distances  poses [N, 7] camera-to-world (t, q = x y z w), disps [N, h, w], intrinsics [N, 4] (fx fy cx cy at the maps' resolution)
 *              -> matrix [N, N] = scale * (S_ij + S_ji) / (V_ij + V_ji), +inf where fewer than 70 % of the 2 h w points are valid
 *              (never NaN), bitwise symmetric.  S_ij = sum over the pixels of i of min(|flow|, 100) * valid, V_ij = sum valid, for
 *              G_ij = P_j P_i^-1 on the world-to-camera poses (i = j: translation (-0.1, 0, 0), no rotation): X1 = R (X, Y, 1) + t disp,
 *              Z = X1_z or 1 where X1_z < 0.1, projection with j's intrinsics, valid = X1_z > 0.2.  3 launches.
 *   lists      matrix [N, N] -> CSR lists of the entries < max_flow, columns ascending.  cols == dists == NULL: the degree count and
 *              the scan write rowptr i64 [N + 1] (2 launches); the caller reads rowptr[N], sizes cols i64 / dists f32 of `capacity`
 *              entries and calls again with them: the order-preserving compaction (1 launch; stores past `capacity` are dropped).
 * (The declarations keep a space in front of the parenthesis: tests/test_frames_cpu.py takes every `devo_frame_` name that is directly
 * followed by one for an entry point of csrc/frames.hip.)
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_FRAME_GRAPH_MAX_FRAMES 32768
#define DEVO_FRAME_GRAPH_MAX_POINTS (1 << 20)
size_t devo_frame_graph_workspace_bytes (int N, int h, int w);
int devo_frame_graph_disps (const float* depths, float* disps, int N, int h, int w, devo_stream_t stream);
int devo_frame_graph_distances (const float* poses, const float* disps, const float* intrinsics, int N, int h, int w, float scale, float* matrix, void* ws,
                               size_t ws_bytes, devo_stream_t stream);
int devo_frame_graph_lists (const float* matrix, int N, float max_flow, int64_t* rowptr, int64_t* cols, float* dists, int64_t capacity, void* ws, size_t ws_bytes,
                           devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Patch selection (devo/selector.py:50-287, PatchSelector.__call__, and what devo/enet.py:100-200 derives from the chosen centres;
 * csrc/select.hip; devo_amd/select.py): ONE launch, one workgroup per frame, no workspace.
 *   scores   f32 [n, h, w] with ELEMENT strides (s_n, s_h, s_w).  The map is zero-padded (never materialised) to whole cells of k x k —
 *            whole 2 x 2 grids of cells with `grid` — centred, the extra pixel of an odd padding at the bottom / right; pad = 0 (3xrandom
 *            only) runs on the map as it is.  k must be 4; at most DEVO_SELECT_MAX_CELLS cells per frame, m <= DEVO_SELECT_MAX_CELLS
 *            (3xrandom: 3 m): anything larger is DEVO_ERR_UNSUPPORTED.
 *   ranking  everywhere: the higher key first, on equal keys the lower flat cell index first.  Bit-reproducible, no atomics.
 *   TOPK     key = the cell's maximum; the m best cells (grid: m / 4 per quadrant, output k-major and quadrant-minor), pixel = the
 *            first maximum of the cell in row-major order.
 *   MULTI    noise f32 [n, C + 16 m] of Exp(1) draws, C = cells per frame (values <= 0 count as FLT_MIN).  Cell key
 *            (mean + 1e-7f) / noise[cell] with grid, mean / noise[cell] without; the largest keys in decreasing order.  The pixel of
 *            output slot s: offset o = first argmax_j (win[j] + 1e-7f) / noise[C + 16 s + j] over the 16 pixels that start one pixel
 *            up-left of the cell (0 outside the padded map), applied to the cell's origin (the reference's arithmetic).
 *   NMS      a 3 x 3 box at every cell's maximum (x1 = max(cx - 1.5, 0), x2 = x1 + 3), category = the frame, with grid the reference's
 *            quadrant test (box corner in pixels < half the pooled size), greedy suppression at IoU > 0.4 in rank order; the first m
 *            survivors, counts i32 [n] = survivors per frame; slots beyond the count repeat the frame's last survivor.  The suppression
 *            is iterated over the whole map until nothing changes: (longest suppression chain + 1) rounds of one barrier each, at most
 *            C + 1 (a monotonically decreasing chain of overlapping boxes through every cell): bounded, never a hang.
 *   3XRANDOM cand_x, cand_y i64 [n, 3 m] on the (padded) map; their scores (0 in the padding) sorted ascending and stable, the last m;
 *            out_scores = those scores, ascending; the winners leave as x + 1, y + 1 (the reference's _3xrandom).
 *   epilogue x = clamp(x - left, 0, w - 1) (y alike; without the clamp when pad = 0), out_scores = the map there (all modes but
 *            3XRANDOM), then x += offset, y += offset and, with `clamp`, x into [cx0, cx1], y into [cy0, cy1].
 *   outputs  x, y i64 [n, m]; xy f32 [n, m, 2]; out_scores f32 [n, m]; index i64 [n m] (the frame); patches f32 [n m, 3, P, P]:
 *            (x + j - P/2, y + i - P/2, 1) — with disps (f32 [n, H, W], element strides d_n, d_h, d_w) the depth there, and 0 in all
 *            three planes outside H x W.  disps must have the size of the FRAME the centres live in (the feature map, which the entry
 *            point does not see otherwise): H x W is both the gather's bound and the bound the coordinates are zeroed against.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_SELECT_MAX_CELLS 4096
enum { DEVO_SELECT_TOPK = 0, DEVO_SELECT_MULTI = 1, DEVO_SELECT_NMS = 2, DEVO_SELECT_3XRANDOM = 3 };
int devo_patch_select(const float* scores, int64_t s_n, int64_t s_h, int64_t s_w, int n, int h, int w, int m, int mode, int grid, int k, int pad,
                      const float* noise, const int64_t* cand_x, const int64_t* cand_y, int offset, int clamp, int cx0, int cx1, int cy0, int cy1,
                      const float* disps, int64_t d_n, int64_t d_h, int64_t d_w, int H, int W, int P, int64_t* x, int64_t* y, float* xy,
                      float* out_scores, float* patches, int64_t* index, int* counts, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Trajectory evaluation (what utils/eval_utils.py's ate / ate_real / log_results obtain from evo: association, Umeyama alignment,
 * ATE; csrc/traj_eval.hip; devo_amd/evaluation.py): ONE launch, one workgroup per pair of trajectories, all arithmetic fp64,
 * fixed-order reductions (bit-reproducible, independent of B), no host synchronisation.
 *   est, gt      poses [total_est, 7] / [total_gt, 7] as (t, q_xyzw), camera-to-world, contiguous, pose_dtype DEVO_F32 or DEVO_F64;
 *                quaternions are normalised on load.  Pair b owns rows est_off[b] .. est_off[b + 1] and gt_off[b] .. gt_off[b + 1]
 *                (int64 [B + 1] in DEVICE memory, checked against the totals by the kernel).
 *   stamps       [total_est] / [total_gt], int64 (stamps_f64 = 0) or fp64 (1), compared after conversion to fp64; a magnitude
 *                >= 2^53 or a non-finite stamp flags the pair (the conversion would not be exact).
 *   assoc        NEAREST: the shorter trajectory (the ground truth at equal length) is the short one; short pose i takes the long index
 *                j of the nearest stamp (the lowest j on equal distance, the leftmost of equal stamps) and is kept when the distance is
 *                <= max_diff; matches stay in short order.  INTERPOLATE: every estimated stamp inside [gt[0], gt[-1]] gets the ground
 *                truth interpolated between its bracketing poses (linear translation, shorter-arc slerp; a stamp that hits a ground-truth
 *                stamp takes that pose, the leftmost of equal ones); the estimate is the short one, matched = the lower bracket.
 *                The long stamps must be non-decreasing.
 *   align        NONE, SE3, SIM3 of the estimate onto the ground truth (Umeyama 1991) over the n matched positions: means, sigma_x^2 =
 *                mean |x - mean x|^2, Sigma = mean (y - mean y)(x - mean x)^T = U D V^T by a one-sided Jacobi iteration, S = diag(1, 1,
 *                sign(det U det V)), R = U S V^T, c = tr(D S) / sigma_x^2 (1 for SE3), t = mean y - c R mean x.  The third singular
 *                vectors are the cross products of the first two (a planar trajectory is valid).  n < 3 or sigma_2 <= 1e-10 sigma_1
 *                is degenerate.  NONE needs n >= 1.
 *   stats        fp64 [B, DEVO_TRAJ_EVAL_COLS], e_i = |y_i - (c R x_i + t)|:
 *                0 n; 1 rmse; 2 mean; 3 median (the mean of the two middle values for even n; NaN if an error is NaN); 4 std (population,
 *                two passes); 5 min; 6 max; 7 sse; 8 rot_rmse_deg, 9 rot_mean_deg (the angle of R_gt^T R R_est, 2 atan2(|q_v|, |q_w|));
 *                10 path_length (the whole ground-truth trajectory of the pair, before association); 11 MPE = 100 mean / path_length;
 *                12 scale c; 13 rpe_trans_rmse, 14 rpe_rot_rmse_deg over the matches k, k + rpe_delta (the estimate's translations scaled
 *                by c, error pose (Q_k^-1 Q_k+d)^-1 (P_k^-1 P_k+d); NaN for rpe_delta = 0 or >= n); 15 the number of RPE terms.
 *   transform    fp64 [B, 8] = (c, t, q_xyzw of R, w >= 0).
 *   status       i32 [B]: 0 or DEVO_TRAJ_* flags.  A flagged pair has columns 1 .. 15 and its transform NaN; column 0 stays the
 *                number of matches (0 when the association did not run).
 *   errors_out   fp64 [total_est] or NULL: e per SHORT pose at est_off[b] + i (the short trajectory is never longer than the estimate),
 *                NaN where unmatched and behind the short length.  matched_out i32 [total_est] or NULL: the long index, -1 likewise.
 *   ws           devo_traj_eval_workspace_bytes(total_est, assoc) bytes, 16-byte aligned.
 * At most DEVO_TRAJ_EVAL_MAX_MATCHES short poses per pair (more: the pair is flagged).
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_TRAJ_EVAL_COLS 16
#define DEVO_TRAJ_EVAL_MAX_MATCHES 131072
enum { DEVO_TRAJ_ALIGN_NONE = 0, DEVO_TRAJ_ALIGN_SE3 = 1, DEVO_TRAJ_ALIGN_SIM3 = 2 };
enum { DEVO_TRAJ_ASSOC_NEAREST = 0, DEVO_TRAJ_ASSOC_INTERPOLATE = 1 };
enum { DEVO_TRAJ_NO_MATCH = 1, DEVO_TRAJ_TOO_FEW = 2, DEVO_TRAJ_DEGENERATE = 4, DEVO_TRAJ_UNSORTED = 8, DEVO_TRAJ_TOO_LONG = 16, DEVO_TRAJ_STAMP_RANGE = 32,
       DEVO_TRAJ_BAD_OFFSETS = 64 };
size_t devo_traj_eval_workspace_bytes(int64_t total_est, int assoc);
int devo_traj_eval(const void* est, const void* est_stamps, const int64_t* est_off, int64_t total_est, const void* gt, const void* gt_stamps,
                   const int64_t* gt_off, int64_t total_gt, int B, int pose_dtype, int stamps_f64, int assoc, int align, double max_diff, int rpe_delta,
                   double* stats, double* transform, int* status, double* errors_out, int* matched_out, void* ws, size_t ws_bytes, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Relative pose error (the drift over sub-trajectories of a given length: what the reference's scripts/evaluate_rpe.py computes for a
 * fixed delta, and the "rel stats" of utils/eval_utils.py:log_results; csrc/traj_rel.hip; devo_amd/evaluation.py: relative_errors).
 * THREE launches on `stream`: devo_traj_eval's (association as above, align SIM3 when the scale is asked of it, NONE otherwise), prepare
 * (one workgroup per pair) and errors (one workgroup per (pair, delta)); fp64, fixed-order reductions, bit-reproducible, independent of
 * B and D, no host synchronisation.  est .. stamps_f64, assoc, max_diff: as for devo_traj_eval.  The n matches (x_k, y_k, s_k) of a pair
 * are in short order; s_k is the estimate's stamp.
 *   deltas       HOST fp64 [D], 1 <= D <= DEVO_TRAJ_REL_MAX_DELTAS, positive and finite; with relative != 0 fractions of u_{n-1} - u_0
 *                (resolved on the device).
 *   scale_mode   SIM3: c is the Umeyama scale of devo_traj_eval(align SIM3) (same bits; its rule of three matches and its degeneracy
 *                flag apply); VALUE: c = scale for every pair; PER_PAIR: c = scale_per_pair[b] (DEVICE fp64 [B]).  With a given scale
 *                two matches suffice (fewer: DEVO_TRAJ_TOO_FEW) and collinear matches are valid.
 *   unit         the index u_k: FRAMES k; STAMPS s_k (must not decrease: DEVO_TRAJ_UNSORTED); METRES the cumulative path length,
 *                RADIANS / DEGREES the cumulative rotation angle between consecutive matches, along the ground truth's matched poses
 *                (ALONG_GT) or the estimate's (ALONG_EST; its lengths times c).
 *   end          of the sub-trajectory that starts at match i.  REACH: the first j > i with u_j - u_i >= delta, none: no pair.  CLOSEST:
 *                the j in [0, n) whose u_j is nearest to u_i + delta, the lowest on a tie; dropped when j = n - 1 (j = i can occur).
 *   the error    E = (c . (X_i^-1 X_j))^-1 (Y_i^-1 Y_j), c multiplying the translation of the estimate's relative motion; |t_E| and the
 *                angle of R_E in degrees, 2 atan2(|q_v|, |q_w|).
 *   stats        fp64 [B, D, DEVO_TRAJ_REL_COLS]: 0 n (pose pairs); 1 trans_rmse, 2 trans_mean, 3 trans_median, 4 trans_std, 5 trans_min,
 *                6 trans_max; 7 .. 12 the same of the rotation error in degrees; 13 delta (resolved, in the unit); 14 span_mean, the mean
 *                of u_j - u_i; 15 scale c.  std and median as for devo_traj_eval.
 *   status       i32 [B, D]: devo_traj_eval's flags of the pair in each of its rows (and TOO_FEW / UNSORTED as above), or
 *                DEVO_TRAJ_REL_NO_PAIR for a (pair, delta) without a pair of poses.  A flagged row has n = 0 and NaN elsewhere.
 *   errors_out   fp64 [D, total_est, 2] or NULL: (|t_E|, angle) of the sub-trajectory starting at match i, at row est_off[b] + i; NaN where
 *                there is none.  ends_out i32 [D, total_est] or NULL: its end j (a match number), -1 likewise.
 *   ws           devo_traj_rel_workspace_bytes(total_est, assoc, B, D) bytes, 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_TRAJ_REL_COLS 16
#define DEVO_TRAJ_REL_MAX_DELTAS 16
enum { DEVO_TRAJ_REL_UNIT_FRAMES = 0, DEVO_TRAJ_REL_UNIT_STAMPS = 1, DEVO_TRAJ_REL_UNIT_METRES = 2, DEVO_TRAJ_REL_UNIT_RADIANS = 3, DEVO_TRAJ_REL_UNIT_DEGREES = 4 };
enum { DEVO_TRAJ_REL_ALONG_GT = 0, DEVO_TRAJ_REL_ALONG_EST = 1 };
enum { DEVO_TRAJ_REL_END_REACH = 0, DEVO_TRAJ_REL_END_CLOSEST = 1 };
enum { DEVO_TRAJ_REL_SCALE_SIM3 = 0, DEVO_TRAJ_REL_SCALE_VALUE = 1, DEVO_TRAJ_REL_SCALE_PER_PAIR = 2 };
enum { DEVO_TRAJ_REL_NO_PAIR = 128 }; /* joins the DEVO_TRAJ_* status bits */
size_t devo_traj_rel_workspace_bytes(int64_t total_est, int assoc, int B, int D);
int devo_traj_rel_eval(const void* est, const void* est_stamps, const int64_t* est_off, int64_t total_est, const void* gt, const void* gt_stamps,
                       const int64_t* gt_off, int64_t total_gt, int B, int pose_dtype, int stamps_f64, int assoc, double max_diff, const double* deltas,
                       int D, int unit, int relative, int along, int end, int scale_mode, double scale, const double* scale_per_pair, double* stats,
                       int* status, double* errors_out, int* ends_out, void* ws, size_t ws_bytes, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Camera models (what the reference obtains from OpenCV: utils/load_utils.py:675-702, :1041-1058, scripts/pp_*.py, devo/stream.py:26,74;
 * csrc/camera.hip; devo_amd/camera.py).  K, dist, R, K_new are HOST pointers to small fp64 arrays; they travel as kernel arguments (no
 * device copy, no workspace, one launch per call).
 *   model, dist  PINHOLE (n_dist 0), RADTAN (OpenCV's k1 k2 p1 p2 [k3]: n_dist 4 or 5), EQUIDISTANT (Kannala-Brandt / OpenCV fisheye
 *                k1..k4: n_dist 4).  Any other count is refused.
 *   K, K_new     (fx, fy, cx, cy), finite, focal lengths non-zero.  R: 3 x 3 row-major or NULL (identity).
 *   points       DEVICE [n, 2] of in_dtype (DEVO_F32 / DEVO_F64), or NULL: the pixel grid x = 0 .. W - 1, y = 0 .. H - 1 in row-major
 *                order, generated in the kernel (n must be H * W).  With points, H and W are not read.
 *   out          DEVICE [n, 2] of out_dtype (DEVO_F32 / DEVO_F64); all arithmetic is fp64.  An invalid point is (NaN, NaN).
 *   invalid_count  DEVICE int32 or NULL: the number of invalid points is ADDED (the caller zeroes it); one atomic per wave that has any.
 * devo_camera_undistort_points: raw pixel -> ideal pixel.  x_d = K^-1 p; x = model^-1(x_d); x <- R x (divided by its third component);
 *   out = K_new x, or x itself (normalised coordinates) when K_new is NULL.
 *   RADTAN: Newton on the two-dimensional forward model with its analytic Jacobian J, from x = x_d, at most 30 iterations, until
 *   |dx| + |dy| < 1e-12.  Valid iff it converges and det J > 0 at every iterate: the principal branch, which never crosses the fold of a
 *   strongly distorted model.
 *   EQUIDISTANT: theta_d = |x_d|; theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = theta_d is solved on [0, theta_lim] by
 *   Newton safeguarded by bisection, x = x_d tan(theta) / theta_d.  theta_lim = the smallest positive root of the left side's derivative
 *   in (0, pi / 2], or pi / 2 (found on the host in fp64).  Valid iff theta_d < theta_d,max = the left side at theta_lim; theta_d = 0 -> 0.
 * devo_camera_distort_points: ideal pixel in K_new (required) -> raw pixel.  x = K_new^-1 p; v = R^T (x, 1); invalid when v.z <= 0
 *   (behind the camera); x = v / v.z; the forward model (closed form); out = K x_d.  EQUIDISTANT: theta = atan |x| > theta_lim is invalid.
 * devo_image_remap: out[b, yo, xo, :] = the bilinear sample of images[b] at map[yo, xo] = (x, y) source coordinates.
 *   images       DEVICE [B, H, W, C] channels-last, contiguous, in_dtype DEVO_U8 or DEVO_F32, C in 1 .. 4.  map fp32 [Ho, Wo, 2].
 *   out          DEVICE [B, Ho, Wo, C], out_dtype DEVO_U8 or DEVO_F32.  fp32 weights from the fp32 coordinates (x - floor x: exact); a tap
 *                outside the image contributes 0 (OpenCV's BORDER_CONSTANT), a NaN coordinate gives 0.  DEVO_U8 output rounds to
 *                nearest even and saturates.  One thread per output pixel serves all channels and all B images.
 * ---------------------------------------------------------------------------------------------- */
enum { DEVO_CAM_PINHOLE = 0, DEVO_CAM_RADTAN = 1, DEVO_CAM_EQUIDISTANT = 2 };
enum { DEVO_U8 = 3 }; /* image dtype code of devo_image_remap, beside DEVO_F32 */
int devo_camera_undistort_points(const void* points, int64_t n, int H, int W, int in_dtype, int model, const double* K, const double* dist, int n_dist,
                                 const double* R, const double* K_new, void* out, int out_dtype, int* invalid_count, devo_stream_t stream);
int devo_camera_distort_points(const void* points, int64_t n, int H, int W, int in_dtype, int model, const double* K, const double* dist, int n_dist,
                               const double* R, const double* K_new, void* out, int out_dtype, int* invalid_count, devo_stream_t stream);
int devo_image_remap(const void* images, int B, int H, int W, int C, int in_dtype, const float* map, int Ho, int Wo, void* out, int out_dtype,
                     devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Event simulation: contrast-threshold events from consecutive log-intensity frames (what the reference's scripts/convert_tartan.py:198-297
 * obtains from esim_torch.ESIM; csrc/esim.hip; devo_amd/simulate.py).  All pointers are DEVICE pointers.
 * State per pixel: ref (fp64 reference level) and last_t (int64 stamp of its last emitted event, DEVO_ESIM_NO_EVENT before the first).
 * One frame pair with fp32 log-intensities i0, i1 (widened to fp64) and int64 nanosecond stamps t0 < t1, dt = t1 - t0:
 *   d = i1 - ref;  d >= 0: pol = +1, C = c_pos, n = floor(d / C);  otherwise pol = -1, C = c_neg, n = floor(-d / C)
 *   k = 1 .. n:  L_k = ref + pol * (k * C)   (the product rounded, then the sum);
 *                f = (L_k - i0) / (i1 - i0) clamped to [0, 1], f = 1 when i1 == i0;   t_k = t0 + (int64) floor(f * (double) dt);
 *                the event is emitted iff last_t is DEVO_ESIM_NO_EVENT or t_k - last_t >= refractory_ns, and then last_t = t_k
 *   ref = L_n when n > 0 (a suppressed event still moves the reference).
 * fp64 with one rounding per operation in this order, nothing contracted: the output is bit-comparable with a host restatement.
 * A call covers T pairs: (prev, frames[0]), (frames[0], frames[1]), ...; prev_stamp [1] and stamps [T] are the frames' stamps.
 *   devo_esim_count   walks every pixel over the T pairs WITHOUT writing events or state.  counts [H * W] int64: emitted events per pixel;
 *                     status_span [2] int64 (zeroed by the call): [0] DEVO_ESIM_* status bits, [1] the call's span stamps[T - 1] - *prev_stamp.
 *                     With a status bit set the rest means nothing and devo_esim_emit must not follow.
 *   devo_esim_emit    the same walk from the same state.  offsets [H * W] = the INCLUSIVE scan of counts, total = its last entry; event e of
 *                     pixel i goes to keys[offsets[i - 1] + e] (never outside [offsets[i - 1], min(offsets[i], total))) as
 *                     key = (t - *prev_stamp) << (b + 1) | i << 1 | (pol > 0),  b = the bits of H * W - 1 (at least 1), i = y * W + x:
 *                     the keys' integer order is the events' total order (t, i, pol) with -1 before +1.  The new state goes to ref_out /
 *                     last_t_out, which must not alias the old one.
 *   devo_esim_sort_keys  keys [n] -> sorted [n] (not in place): rocPRIM's keys-only radix sort over bits 0 .. b + 1 + the bits of span_ns,
 *                     where span_ns >= the largest stamp of a key (the count pass reports the call's span); ws of at least
 *                     devo_esim_sort_workspace_bytes(n, H, W, span_ns) bytes (0: refused arguments, or no device to ask), else
 *                     DEVO_ERR_WORKSPACE.
 *   devo_esim_decode  sorted keys -> x, y int16, t int64 (= *first_stamp + the key's stamp), p int8 in {-1, +1}.
 *   devo_esim_max_span_ns  the limit of the key: stamps[T - 1] - *prev_stamp must be below 2^(62 - b) ns (0 for a refused frame size).
 * Limits, refused with DEVO_ERR_ARG before any launch: 1 <= H, W <= DEVO_ESIM_MAX_SIDE (int16 coordinates); thresholds finite and
 * >= DEVO_ESIM_MIN_THRESHOLD; refractory_ns >= 0.  Found on the device and reported in the status word: a non-finite intensity
 * (NONFINITE), stamps not strictly increasing (STAMPS), a span at or above the key's limit (SPAN), more than DEVO_ESIM_MAX_CROSSINGS levels
 * crossed by one pixel in one pair (CROSSINGS; log_intensity frames with the smallest threshold cross 11 513).
 * devo_log_intensity: out[i] = table[images[i]], table fp32 [256] (the host's np.log(v / 255 + 1e-5) in fp32: convert_tartan.py:244).
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_ESIM_NO_EVENT INT64_MIN
#define DEVO_ESIM_MAX_SIDE 32767
#define DEVO_ESIM_MAX_CROSSINGS 1048576
#define DEVO_ESIM_MIN_THRESHOLD 1e-3
enum { DEVO_ESIM_NONFINITE = 1, DEVO_ESIM_STAMPS = 2, DEVO_ESIM_SPAN = 4, DEVO_ESIM_CROSSINGS = 8 };
int64_t devo_esim_max_span_ns(int H, int W);
int devo_esim_count(const float* prev, const float* frames, const int64_t* prev_stamp, const int64_t* stamps, int T, int H, int W, const double* ref,
                    const int64_t* last_t, double c_neg, double c_pos, int64_t refractory_ns, int64_t* counts, int64_t* status_span, devo_stream_t stream);
int devo_esim_emit(const float* prev, const float* frames, const int64_t* prev_stamp, const int64_t* stamps, int T, int H, int W, const double* ref,
                   const int64_t* last_t, double c_neg, double c_pos, int64_t refractory_ns, const int64_t* offsets, int64_t total, int64_t* keys,
                   double* ref_out, int64_t* last_t_out, devo_stream_t stream);
size_t devo_esim_sort_workspace_bytes(int64_t n, int H, int W, int64_t span_ns);
int devo_esim_sort_keys(const int64_t* keys, int64_t* sorted, int64_t n, int H, int W, int64_t span_ns, void* ws, size_t ws_bytes, devo_stream_t stream);
int devo_esim_decode(const int64_t* keys, int64_t n, int H, int W, const int64_t* first_stamp, int16_t* x, int16_t* y, int64_t* t, signed char* p,
                     devo_stream_t stream);
int devo_log_intensity(const unsigned char* images, int64_t n, const float* table, float* out, devo_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser step: gradient-norm clip + AdamW over a list of fp32 tensors (what the reference's train.py:248-249 does with clip_grad_norm_(10)
 * and torch.optim.AdamW.step(); csrc/optim.hip; devo_amd/optim.py).  Tensor t has numel[t] elements that lie DENSE in memory from its address
 * on (any permutation of a contiguous layout; parameter and gradient in the same one), 1 <= numel[t] < 2^31, at most DEVO_OPTIM_MAX_TENSORS
 * tensors.  Every tensor is cut into chunks of DEVO_OPTIM_CHUNK elements.
 *   devo_optim_chunks         the number of chunks of the list (0: refused sizes).
 *   devo_optim_moment_elems   the elements of each of the two flat moment buffers: every tensor's slice is padded to a multiple of 4 elements,
 *                             so each starts on a 16-byte boundary (0: refused sizes).
 *   devo_optim_plan           HOST outputs, built once: chunk_table [chunks, 4] int32 = (tensor, element offset (uint32), length, 0) in tensor
 *                             order, and moment_offsets [n_tensors] = the element offset of every tensor's slice in the moment buffers.
 *   devo_optim_workspace_bytes  the bytes of the step's workspace (the norm's partial sums).
 *   devo_optim_step           one step.  DEVICE pointers: chunk_table (the plan's, uploaded), tensor_table [n_tensors, 2] int64 = (parameter
 *                             address, moment offset), exp_avg, exp_avg_sq, counters, grad_norm, workspace.  HOST pointers: grads [n_tensors]
 *                             (this step's gradient addresses; NULL: the tensor has no gradient and is skipped whole, parameter and moments
 *                             untouched) and numel [n_tensors].  The gradient addresses travel as kernel arguments, DEVO_OPTIM_GROUP tensors
 *                             per launch, so a step may be enqueued before the one before it has run; nothing is synchronised or copied.
 *     launch 1   sum of g^2 in fp64 (every g widened first), one partial per workgroup, no atomics: bit-reproducible.
 *     launch 2   every workgroup sums the partials in one fixed order; norm = sqrt(sum) -> *grad_norm (fp64, BEFORE clipping);
 *                coef = max_norm < 0 ? 1 : min(1, max_norm / (norm + 1e-6)); then per element in fp32, one rounding per operation:
 *                  g = g coef;  p = p (1 - lr wd);  m = m + (g - m)(1 - beta1);  v = v beta2 + ((1 - beta2) g) g;
 *                  p = p + (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps)
 *                (torch.optim.AdamW's single-tensor form; lr / bc1, sqrt(bc2), 1 - lr wd, 1 - beta formed in fp64 and rounded to fp32).
 *                Gradients are read, never written.  bc1 = 1 - beta1^t and bc2 = 1 - beta2^t are the caller's.
 *     skip_nonfinite = 1   a step whose norm is inf or NaN writes nothing to p, m, v; a third launch then adds 1 to counters[0] (applied)
 *                or counters[1] (skipped), int64 [2]; bc1 and bc2 are formed on the device from t = counters[0] + 1 and the arguments are ignored.
 *                With 0, non-finite values propagate as in torch and counters may be NULL.
 * Refused with DEVO_ERR_ARG before any launch: null or misaligned pointers (16 bytes for tables, moments and gradients), sizes outside the
 * limits, n_chunks that is not the list's, lr / eps / weight_decay negative or not finite, betas outside [0, 1), a NaN max_norm, bias
 * corrections outside (0, 1], a workspace that is too small.
 * ---------------------------------------------------------------------------------------------- */
#define DEVO_OPTIM_CHUNK 2048
#define DEVO_OPTIM_GROUP 256
#define DEVO_OPTIM_MAX_TENSORS 4096
#define DEVO_OPTIM_MAX_PARTIALS 2048
int64_t devo_optim_chunks(const int64_t* numel, int n_tensors);
int64_t devo_optim_moment_elems(const int64_t* numel, int n_tensors);
size_t devo_optim_workspace_bytes(void);
int devo_optim_plan(const int64_t* numel, int n_tensors, int32_t* chunk_table, int64_t* moment_offsets);
int devo_optim_step(const int32_t* chunk_table, int64_t n_chunks, const int64_t* tensor_table, const void* const* grads, const int64_t* numel, int n_tensors,
                    float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double bc1,
                    double bc2, int skip_nonfinite, int64_t* counters, double* grad_norm, void* workspace, size_t workspace_bytes, devo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEVO_HIP_H */
