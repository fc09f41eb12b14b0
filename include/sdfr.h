/*
 * sdfr.h -- C ABI of libsdfr_hip.so: the MI355X (gfx950) implementation of
 * sdfest's differentiable-renderer hot path.
 *
 * This is the drop-in boundary.  It replaces the two entry points of the
 * reference's pybind module `sdf_renderer_cpp`
 *     forward (sdfest/differentiable_renderer/csrc/sdf_renderer.cpp:42-61)
 *     backward(sdfest/differentiable_renderer/csrc/sdf_renderer.cpp:63-86)
 * and, for the render-and-compare loop around them, the torch-op
 * implementations of
 *     losses.pc_loss          (sdfest/estimation/losses.py:32-135)
 *     SDFDecoder.forward      (sdfest/vae/sdf_vae.py:217-259)
 *
 * Rules of the boundary
 *   - plain C, no torch types.  Every pointer is a DEVICE pointer owned by the
 *     caller unless its name starts with `h_`.  All tensors are fp32,
 *     C-contiguous.
 *   - the library allocates nothing and never synchronises the host: all work
 *     is enqueued on `stream` (a hipStream_t; NULL = the default stream), so a
 *     call sequence can be captured into a hipGraph.  Scratch memory comes from
 *     the caller (`*_workspace_bytes`).
 *   - re-entrant and thread-safe: the reference's backward runs on a PyTorch
 *     autograd worker thread; every call does hipSetDevice(device) itself
 *     (reference: OptionalCUDAGuard, sdf_renderer.cpp:57-58, :82).
 *   - return 0 on success, a negative SDFR_E_* for argument errors, or a
 *     positive hipError_t.  sdfr_last_error() gives the thread's last message.
 *
 * Data layout
 *   sdf      [R][R][R]   index order sdf[x][y][z]
 *   pos      [B][3]      object position in the camera frame (OpenGL: -z forward)
 *   quat     [B][4]      object orientation, (x, y, z, w) scalar-last, unit norm
 *   inv_scale[B]         1 / half-width of the SDF volume
 *   depth    [B][H][W]   row 0 = top; 0 = no hit
 *   cx, cy               principal point in the pixel-centre-0.5 convention
 *                        (Camera.get_pinhole_camera_parameters(0.5),
 *                        sdf_renderer.py:116-133)
 *   B views share one SDF (sdf_view_stride = 0) or have one each
 *   (sdf_view_stride = R*R*R elements).
 *
 * STABILITY -- group 1 below is the boundary: its signatures and semantics are what a binding relies on and do not change
 * without SDFR_VERSION's major number changing.  Groups 2 - 9 are UNSTABLE: they exist for this repository's own host
 * code (the Python modules under sdfest_amd/), follow its needs from round to round (arguments were added in every round so far), and are
 * exported only because that host code is Python over ctypes; bind to them at your own risk, pinned to one SDFR_VERSION.
 *
 * CONTENTS -- the groups; a binding from another language needs group 1 only
 *   1. CORE: the reference boundary (what sdf_renderer_cpp, losses.pc_loss and SDFDecoder.forward are replaced by)
 *        sdfr_version, sdfr_last_error
 *        sdfr_render_forward[_workspace_bytes], sdfr_render_backward[_workspace_bytes]
 *        sdfr_pc_loss_forward, sdfr_pc_loss_backward[_workspace_bytes]
 *        sdfr_decoder_create / _destroy / _forward / _workspace_bytes / _tape_bytes,
 *        sdfr_decoder_backward_latent[_workspace_bytes], sdfr_decoder_set_option, sdfr_decoder_fc_one_wave
 *   2. [unstable] BATCHED / STEP forms of the same arithmetic (fewer launches, fewer bytes; same results)
 *        sdfr_render_step_forward[_counted|_resident] / _step_backward / _step_workspace_bytes, sdfr_render_sync_offset,
 *        sdfr_render_forward_resident, sdfr_render_resident_state_bytes,
 *        sdfr_render_partials_offset, sdfr_render_fixed_volume_offset, sdfr_fixed_to_float
 *        sdfr_render_forward_l1[_workspace_bytes], sdfr_render_backward_l1, sdfr_render_step_forward_l1,
 *        sdfr_render_step_backward_l1, sdfr_render_backward_l1_pc, sdfr_render_step_backward_l1_pc,
 *        sdfr_render_step_fused_l1_pc, sdfr_render_fused_view_count_offset, sdfr_render_fused_tile_loss_offset
 *        sdfr_pc_l1_backward[_accumulate]
 *        sdfr_decoder_launch_plan
 *   3. [unstable] LOOP: one render-and-compare iteration (SDFPipeline.__call__) as a fixed launch sequence
 *        sdfr_preprocess_depth, sdfr_depth_to_points_resident, sdfr_depth_count[_ordered|_centroid],
 *        sdfr_depth_to_points[_ordered|_shifted], sdfr_depth_points_workspace_bytes, sdfr_depth_centroid_workspace_bytes
 *        sdfr_pose_to_views[_objects], sdfr_views_to_pose_grad[_deferred], sdfr_decoder_backward_latent_deferred[_batch|_scaled], sdfr_decoder_forward_stage,
 *        sdfr_loop_tail, sdfr_loop_tail_fused, sdfr_loop_tail_objects, sdfr_adam_step, sdfr_point_constraint, sdfr_add_inplace
 *        K objects with V views each: sdfr_volumes_replicate, sdfr_volumes_sum_views, sdfr_inlier_ratio_objects
 *        N hypotheses of one object, refined as N such rows: sdfr_select_row
 *        sdfr_depth_l1_loss[_workspace_bytes], sdfr_pc_l1_loss, sdfr_inlier_ratio, sdfr_nn_loss_forward / _backward
 *        sharded over ranks: sdfr_loop_view_records, sdfr_loop_tail_records, sdfr_inlier_counts_record,
 *        sdfr_inlier_update_record
 *   4. [unstable] GENERATOR / INITIALISATION (the forward-only callers around the loop)
 *        sdfr_affine_mask; sdfr_pointnet_layer[_counted], sdfr_linear_vec, sdfr_orientation_posterior,
 *        sdfr_init_estimate; N sets per launch and the trainer's validation numbers: sdfr_pointnet_layer_batch,
 *        sdfr_linear_rows, sdfr_pose_metrics[_workspace_bytes]
 *        the N most probable orientation cells as N starts of the loop: sdfr_orientation_topk, sdfr_init_hypotheses
 *   5. [unstable] MESH: marching cubes over N grids (SDFPipeline.generate_mesh, after the estimate)
 *        sdfr_mesh_tables, sdfr_mesh_workspace_bytes, sdfr_mesh_count, sdfr_mesh_emit
 *   6. [unstable] METRICS: surface sampling and exact neighbour search for reconstruction metrics (the evaluation)
 *        sdfr_sample_workspace_bytes, sdfr_sample_points, sdfr_nn_workspace_bytes, sdfr_nn_query, sdfr_nn_reduce
 *   7. [unstable] ENCODER: the VAE's encoder half (SDFVAE.encode / forward / sample / prepare_input)
 *        sdfr_encoder_create / _destroy / _workspace_bytes / _forward, sdfr_normal_sample, sdfr_clamp
 *   8. [unstable] MESH DEPTH: depth images of triangle meshes (the synthetic views of the evaluation)
 *        sdfr_mesh_depth_workspace_bytes, sdfr_mesh_depth
 *   9. [unstable] MESH TO SDF: the signed distance volume of a triangle mesh (what the VAE is trained on and encodes)
 *        sdfr_mesh_sdf_workspace_bytes, sdfr_mesh_sdf
 *  12. [unstable] NOCS ANNOTATION: pose and scale of a NOCS frame's objects (NOCSDataset's preprocessing)
 *        sdfr_nocs_workspace_bytes, sdfr_nocs_count, sdfr_nocs_correspondences,
 *        sdfr_similarity_ransac[_workspace_bytes], sdfr_nocs_sample_indices
 *  13. [unstable] FRAME ANNOTATION: the visibility mask of an annotated RGB-D frame (AnnotatedRedwoodDataset)
 *        sdfr_visible_mask
 *  14. [unstable] POSE INFORMATION: the Gauss-Newton normal matrix of the depth residual (SDFPipeline.pose_uncertainty)
 *        sdfr_render_information[_workspace_bytes]; jointly with the latent: sdfr_render_information_shape[_workspace_bytes]
 *  15. [unstable] BOXES: the oriented box of an estimate without its mesh, and the exact 3D IoU of oriented boxes
 *        sdfr_sdf_bounds, sdfr_box_iou
 *  16. [unstable] AVERAGE PRECISION: pose errors of pairs, detection matching and the AP integral (the evaluation's mAP)
 *        sdfr_pose_pair_errors, sdfr_ap_match, sdfr_ap_integrate
 *  17. [unstable] DECODER JVP: the Jacobian of the decoded volume w.r.t. the latent (SDFPipeline.shape_uncertainty)
 *        sdfr_decoder_jvp[_workspace_bytes], sdfr_sdf_std
 *  18. [unstable] LM REFINEMENT: a damped Gauss-Newton step of pose and latent from those Gram matrices (SDFPipeline.refine)
 *        sdfr_lm_step
 *  19. [unstable] POINT-CLOUD INFORMATION: the Gauss-Newton normal matrix of the point-cloud residual, and its sum with
 *      the depth term's for group 18 (LMRefiner(pc_weight=), SDFPipeline.refine(pc_weight=))
 *        sdfr_pc_information[_workspace_bytes], sdfr_information_combine
 * (Within the file the groups follow the order in which the reference's code runs; every declaration carries the
 * reference file:line it replaces.)
 */
#ifndef SDFR_H_
#define SDFR_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFR_VERSION 100 /* 0.1.0 */
#define SDFR_API __attribute__((visibility("default")))

#define SDFR_E_INVALID (-1)   /* bad shape / size / flag */
#define SDFR_E_NULL (-2)      /* required pointer is NULL */
#define SDFR_E_WORKSPACE (-3) /* workspace too small */

/* ray-march safety cap.  The reference loop (sdf_renderer_cuda.cu:283-293) is
 * unbounded and spins forever for threshold == 0 on an exactly-zero sample; a
 * ray that needs more evaluations than this is reported as a miss (depth 0). */
#define SDFR_MAX_MARCH_STEPS 4096

/* d depth / d sdf weight assignment */
#define SDFR_SDF_GRAD_EXACT 0       /* trilinear weights (simple_renderer.py:399-408) */
#define SDFR_SDF_GRAD_CUDA_COMPAT 1 /* the permutation in sdf_renderer_cuda.cu:373-388 */
/* Flag bit, OR-ed into either of the above: DETERMINISTIC d depth / d sdf.  The reference
 * sums the per-pixel contributions with float atomics (sdf_renderer_cuda.cu:373-388) and so does the default mode
 * here, one per touched voxel per tile: the result varies in the last bits from run to run.  With this flag every
 * contribution is rounded once, per pixel, to the fixed quantum 2^-SDFR_FIXED_QUANTUM_BITS and everything after
 * that is INTEGER addition into a 64-bit volume in the workspace, converted to float at the end: g_sdf is bitwise
 * identical from run to run and does not depend on tile shapes, batch composition or -- when the ranks of a
 * sharded batch add their 64-bit volumes (sdfr_render_fixed_volume_offset) and convert afterwards
 * (sdfr_fixed_to_float) -- on how the views are spread over GPUs.  For tests and reproducible runs: several
 * times slower than the default (64-bit LDS table, no dense box).  Shared gradient volume only
 * (g_sdf_view_stride = 0), R <= 128; every backward form takes it (the loss-fused ones and the sampler's blocks of
 * sdfr_render_backward_l1_pc add into the same 64-bit volume).  Representable range:
 * |sum| < 2^(63 - 40) = 8.4e6 per voxel; contributions that are not finite count as 0 (NaN) or saturate. */
#define SDFR_SDF_GRAD_DETERMINISTIC 0x100
#define SDFR_FIXED_QUANTUM_BITS 40
/* Flag bit, OR-ed into sdf_grad_mode: a PERFORMANCE HINT for batch launches of sdfr_render_backward /
 * sdfr_render_step_backward, "the views are close": (nearly) every object spans at least two pixels per voxel on
 * the screen,
 *     sqrt(|fx fy|) * (2 / (R - 1)) / (inv_scale * |pos|) >= 2.
 * The kernel picks each view's tile shape on the device (32 x 32 pixels for such views, 64 x 8 otherwise) and the
 * launch has to provide workgroups for the finer tiling although close views use half of them; with the hint the
 * grid has half the rows (backward of the benchmark 125 -> 112 us) and a view that is NOT close takes its tiles two
 * per workgroup, one after the other -- results are the same whether the hint is true or not, but such views are
 * slower with it (objects of ~1 pixel per voxel: 103 -> 174 us).  The poses live in device memory: a caller that
 * does not know them asks the forward to count the close views (sdfr_render_step_forward_counted) and sets the
 * hint from an earlier step's count.  Ignored for small calls, for the deterministic forms and where the sampler's
 * blocks share the launch (sdfr_render_*backward_l1_pc). */
#define SDFR_BWD_HALF_GRID 0x200
/* Flag bit, OR-ed into sdf_grad_mode: the backward always uses its 32 x 8 tiling, whatever the batch size.  A
 * view's pose gradients are fixed-order sums over ITS tiles, so with this flag they do not depend on how many
 * other views share the launch: a batch sharded over ranks (sdfest_amd.pipeline, the sharded render-and-compare
 * loop) then gets, together with SDFR_SDF_GRAD_DETERMINISTIC, bitwise the single-process gradients.  Slower for
 * large batches (more, smaller tiles).  Pass the same flag to sdfr_loop_view_records. */
#define SDFR_BWD_SMALL_TILES 0x400

SDFR_API int sdfr_version(void);
SDFR_API const char* sdfr_last_error(void);

/* ==== 1. CORE ================================================================================= */
/* ---- sphere-tracing depth render -------------------------------------------------------- */

/* Scratch for sdfr_render_forward (per-view set-up records + the re-packed grid, see
 * render.hip "cell records").
 * Every renderer workspace (forward, backward, step, depth-L1 forms) starts with the B view records and,
 * at byte sdfr_render_sync_offset(B), a small sync region that only the forward's prologue launch uses:
 *   word 0 (uint32)  epoch of the prologue's intra-launch hand-off of the grid's plane minima
 *   word 1 (uint32)  count of view set-ups that did NOT receive the plane minima in time and fell back to the
 *                    whole cube as their may-hit box (same depth, slower march); it only ever grows, so a caller
 *                    that zero-fills the workspace once can read "how often did that happen" at any time.
 *   words 6, 7       {SDFR_SYNC_POLLS_MAGIC, rounds}: the caller's bound of the prologue's wait for the plane minima,
 *                    in polling rounds, for the forwards on THIS workspace (default 65536; 0: every view set-up takes
 *                    the fall-back path -- tests reach it this way).  Any other word 6 -- a zero-filled or an
 *                    uninitialised workspace -- means the default.  The library only reads them.
 *   words 8, 9       the stamp of the grid whose face records the workspace holds (RESIDENT GRID, below)
 *   word 11          SDFR_SYNC_GRID_MISMATCH_WORD: records that SDFR_GRID_RESIDENT_VERIFY found changed; only grows
 * No call writes into another call's part of a shared workspace's sync region. */
#define SDFR_SYNC_POLLS_MAGIC 0x504F4C4Cu
SDFR_API size_t sdfr_render_forward_workspace_bytes(int R, int B, int W, int H);
SDFR_API size_t sdfr_render_sync_offset(int B);

/* Deterministic mode: byte offset, in the workspace of sdfr_render_backward (step_layout = 0) or of
 * sdfr_render_step_backward (1), of the int64 [R][R][R] volume the last deterministic backward left:
 * g_sdf = volume * 2^-SDFR_FIXED_QUANTUM_BITS.  sdfr_fixed_to_float converts n such words (after, e.g., an
 * integer all-reduce over the ranks of a sharded batch). */
SDFR_API size_t sdfr_render_fixed_volume_offset(int R, int B, int W, int H, int step_layout);
SDFR_API int sdfr_fixed_to_float(const long long* fixed, size_t n, float* out, int device, void* stream);

/* Replaces sdf_renderer_cpp.forward (sdf_renderer.cpp:42-61 ->
 * sdf_renderer_cuda.cu:472-510, kernel :241-298), extended by a leading batch
 * dimension: view b of the output equals one reference call with pose b.
 * `depth` is fully overwritten (the reference zero-fills with torch::zeros). */
SDFR_API int sdfr_render_forward(const float* sdf, int R, long long sdf_view_stride,
                        const float* pos, const float* quat, const float* inv_scale, int B,
                        int W, int H, float cx, float cy, float fx, float fy, float threshold,
                        float* depth, void* workspace, size_t workspace_bytes, int device,
                        void* stream);

/* Scratch for sdfr_render_backward (set-up records + per-tile partial sums). */
SDFR_API size_t sdfr_render_backward_workspace_bytes(int R, int B, int W, int H);

/* Replaces sdf_renderer_cpp.backward (sdf_renderer.cpp:63-86 ->
 * sdf_renderer_cuda.cu:512-556, kernel :300-468), batched like the forward.
 *   depth        the forward's output for the SAME poses (pixels with depth != 0
 *                are differentiated, :334)
 *   g_sdf        overwritten.  g_sdf_view_stride = 0: [R][R][R], the sum over
 *                the B views (what autograd would accumulate for a shared SDF);
 *                R*R*R: one gradient volume per view.
 *   g_pos [B][3], g_quat [B][4] (x,y,z,w), g_inv_scale [B]: overwritten.
 * Pose gradients are reduced in a fixed order (bitwise reproducible); g_sdf uses
 * float atomics across workgroups (last-bit run-to-run variation, as in the
 * reference) unless sdf_grad_mode carries SDFR_SDF_GRAD_DETERMINISTIC. */
SDFR_API int sdfr_render_backward(const float* grad_depth, const float* depth, const float* sdf, int R,
                         long long sdf_view_stride, const float* pos, const float* quat,
                         const float* inv_scale, int B, int W, int H, float cx, float cy,
                         float fx, float fy, int sdf_grad_mode, float* g_sdf,
                         long long g_sdf_view_stride, float* g_pos, float* g_quat,
                         float* g_inv_scale, void* workspace, size_t workspace_bytes, int device,
                         void* stream);

/* ==== 2. BATCHED / STEP forms ================================================================= */
/* ---- one step = forward + backward of the SAME views ---------------------------------------- */

/* The reference's render-and-compare loop always runs the two halves as a pair:
 * SDFRendererFunctionGPU.forward saves (image, sdf, pos, quat, inv_scale) and .backward gets them back
 * (sdf_renderer.py:311-331, :334-357).  As two independent calls the backward repeats work the forward
 * has done (its own view set-up, with the whole cube's screen rectangle because it does not know the
 * threshold) and opens with a launch of its own (zero fill of g_sdf + set-up).  A step keeps the pair's
 * state in ONE workspace:
 *   sdfr_render_step_forward   = sdfr_render_forward; its prologue launch also zero-fills `g_sdf`
 *                                (g_sdf_view_stride as in sdfr_render_backward);
 *   sdfr_render_step_backward  = sdfr_render_backward for the views, camera and image size of the
 *                                preceding sdfr_render_step_forward on the same workspace: no prologue
 *                                launch, tiles culled with the forward's may-hit rectangles.  `depth` must
 *                                be that forward's output (it is 0 outside those rectangles), g_sdf the
 *                                volume it zero-filled.  pos / quat / inv_scale are not passed again.
 * Results equal the two stand-alone calls: depth bit for bit; pose gradients up to the rounding of their
 * fixed-order tile sums (the order follows the view's rectangle; still bitwise reproducible run to run),
 * g_sdf up to the order of its float atomics.  Nothing else may use the workspace between the two calls. */
SDFR_API size_t sdfr_render_step_workspace_bytes(int R, int B, int W, int H);
SDFR_API int sdfr_render_step_forward(const float* sdf, int R, long long sdf_view_stride, const float* pos,
                             const float* quat, const float* inv_scale, int B, int W, int H, float cx,
                             float cy, float fx, float fy, float threshold, float* depth, float* g_sdf,
                             long long g_sdf_view_stride, void* workspace, size_t workspace_bytes,
                             int device, void* stream);
/* sdfr_render_step_forward that also REPORTS how many of its views are close -- the fact behind the
 * SDFR_BWD_HALF_GRID hint -- without anybody looking at the poses on the host: the forward counts, on the device,
 * the views whose set-up gave them 32 x 32 backward tiles and, when the last view has been counted, stores
 *     (forwards counted on this workspace << 32) | close views of this forward
 * into *close_views_word with one 64-bit store.  The word must be visible to the device AND readable by the host
 * without a synchronisation (pinned host memory: hipHostMalloc / a pinned torch tensor; 8-byte aligned; NULL: no
 * report).  The caller reads it whenever it likes -- it then holds the count of some earlier, complete forward --
 * and sets the hint of its next backward from it: stale by a step or more is fine for a hint that cannot change
 * results.  Counted by batch launches (the forward's macro-tile form: smaller calls have no batch backward to
 * hint) -- by the image kernel, one atomic per view, off the critical path; the workspace's sync region must have
 * been zero-filled once before its first use.
 * Sync header words 4 / 5 hold the same two numbers on the device. */
SDFR_API int sdfr_render_step_forward_counted(const float* sdf, int R, long long sdf_view_stride, const float* pos,
                                     const float* quat, const float* inv_scale, int B, int W, int H, float cx,
                                     float cy, float fx, float fy, float threshold, float* depth, float* g_sdf,
                                     long long g_sdf_view_stride, void* workspace, size_t workspace_bytes,
                                     unsigned long long* close_views_word, int device, void* stream);
/* RESIDENT DEPTH: sdfr_render_forward / sdfr_render_step_forward_counted for a depth buffer that the caller renders
 * into call after call (a render-and-compare loop: the poses move a little per iteration).  Most of a batch's pixels
 * lie outside every view's may-hit region, and the plain calls store those zeros again in every call -- 74 % of the
 * benchmark's 315 MB.  With a RESIDENT STATE the library remembers, per view and band of 8 rows, which columns its
 * last forward into the buffer may have left non-zero, and a culled tile stores zeros only where that reaches.
 *   resident_state  caller-owned device memory, sdfr_render_resident_state_bytes(B, H) bytes, 128-byte aligned, that
 *                   goes with ONE depth buffer and one (B, W, H).  It needs no initialisation (zero-filled, 0xff-filled
 *                   and random bytes all read as "no previous call").  Only these two calls read or write it: no other
 *                   call's workspace scratch can reach it.  NULL: exactly the plain call.
 *   depth_resident  non-zero: the caller vouches that `depth` holds, byte for byte, what the previous call WITH THIS
 *                   STATE left there (nothing else has written it since, through any API).  0: no promise -- every
 *                   pixel is stored, as by the plain call, and the state is brought up to date for the next call.
 * The hand-over from one call to the next happens on the device (a sequence number in the state that the image
 * kernel advances, and two tag words per row): a captured step can be replayed with changing poses and grids.  A row
 * that was not written by the immediately preceding call with this state does not validate, and every culled tile of
 * that view stores its zeros.  depth is bit for bit what the plain call writes.  Applies to the batch forms over the
 * packed grid (shared SDF, B >= 17, R <= 128, W <= 65535); elsewhere the call stores every pixel and only advances
 * the sequence number.  No launch more than the plain call. */
SDFR_API size_t sdfr_render_resident_state_bytes(int B, int H);
SDFR_API int sdfr_render_forward_resident(const float* sdf, int R, long long sdf_view_stride, const float* pos,
                                 const float* quat, const float* inv_scale, int B, int W, int H, float cx, float cy,
                                 float fx, float fy, float threshold, float* depth, void* workspace,
                                 size_t workspace_bytes, void* resident_state, size_t resident_state_bytes,
                                 int depth_resident, int device, void* stream);
SDFR_API int sdfr_render_step_forward_resident(const float* sdf, int R, long long sdf_view_stride, const float* pos,
                                      const float* quat, const float* inv_scale, int B, int W, int H, float cx,
                                      float cy, float fx, float fy, float threshold, float* depth, float* g_sdf,
                                      long long g_sdf_view_stride, void* workspace, size_t workspace_bytes,
                                      unsigned long long* close_views_word, void* resident_state,
                                      size_t resident_state_bytes, int depth_resident, int device, void* stream);
/* RESIDENT GRID: the two calls above for a caller that renders the SAME grid call after call while the poses move (a
 * pose-only fitting loop, the orientation hypotheses of one object, one shape seen from many views).  The batch forms
 * re-pack the grid into face records in the workspace and reduce its plane minima in every call; all of that depends
 * on the grid alone.  A call that packs now leaves the minima and a stamp in the workspace's sync region beside the
 * records, and
 *   grid_resident   non-zero: the caller vouches that the last call on THIS workspace that packed a grid (any batch
 *                   form over a shared grid: these two, sdfr_render_forward, the step and the depth-L1 forwards)
 *                   packed the very bytes `sdf` points to now, at this address, with the same R and B, and that
 *                   nothing has written the workspace's record region since, through any API (in the plain backward
 *                   layout the tile partials lie where the records do; a step's backward leaves them alone).  The
 *                   prologue launch then neither packs nor reduces nor waits: its view set-ups read the kept minima.
 *                   0: no promise -- exactly the call above.
 * The library cannot compare the bytes.  What it can check costs nothing and is checked on the device, by the launch
 * itself: the stamp of a completed pack with this R, in the packed form this call takes (sync header words 8 / 9).
 * Without it -- a workspace that never packed, another R -- the launch packs as if nobody had vouched: never an error.
 * The poses are not part of the promise: every call sets its views up.  Results are bit for bit the plain call's.
 * Forms without a packed grid ignore the flag (fewer than 17 views, one grid per view, R > 128); the depth-L1 forward
 * and the one-launch fused step have no such argument.
 * Do not vouch in a call that is captured into a graph: the replay would keep the promise over a changed grid.
 *   SDFR_GRID_RESIDENT_VERIFY  (tests) vouch, and let the launch compare every record it did not re-pack with the
 *                   grid, bit for bit: records that differ are counted into sync header word
 *                   SDFR_SYNC_GRID_MISMATCH_WORD (it only ever grows, like word 1).  A separate instantiation: the
 *                   plain and the vouched launch carry no instruction for it. */
#define SDFR_GRID_RESIDENT 1
#define SDFR_GRID_RESIDENT_VERIFY 2
#define SDFR_SYNC_GRID_MISMATCH_WORD 11
SDFR_API int sdfr_render_forward_grid_resident(const float* sdf, int R, long long sdf_view_stride, const float* pos,
                                      const float* quat, const float* inv_scale, int B, int W, int H, float cx,
                                      float cy, float fx, float fy, float threshold, float* depth, void* workspace,
                                      size_t workspace_bytes, void* resident_state, size_t resident_state_bytes,
                                      int depth_resident, int grid_resident, int device, void* stream);
SDFR_API int sdfr_render_step_forward_grid_resident(const float* sdf, int R, long long sdf_view_stride,
                                           const float* pos, const float* quat, const float* inv_scale, int B, int W,
                                           int H, float cx, float cy, float fx, float fy, float threshold,
                                           float* depth, float* g_sdf, long long g_sdf_view_stride, void* workspace,
                                           size_t workspace_bytes, unsigned long long* close_views_word,
                                           void* resident_state, size_t resident_state_bytes, int depth_resident,
                                           int grid_resident, int device, void* stream);
/* The same pair for the loss-fused forms (below): sdfr_render_step_forward_l1 = sdfr_render_forward_l1 that also
 * zero-fills g_sdf and leaves the view records; sdfr_render_step_backward_l1_pc = sdfr_render_backward_l1_pc without
 * its prologue launch.  For a few views of the plain grid the forward has no prologue launch either (every
 * workgroup derives its view's record): the captured loop's iteration loses two launches.  close_views_word
 * (nullable): as in sdfr_render_step_forward_counted -- the half-grid hint of sdfr_render_step_backward_l1. */
SDFR_API int sdfr_render_step_forward_l1(const float* sdf, int R, long long sdf_view_stride, const float* pos,
                                const float* quat, const float* inv_scale, int B, int W, int H, float cx, float cy,
                                float fx, float fy, float threshold, const float* target, float* depth, float* loss,
                                float* loss_stats, float* g_sdf, long long g_sdf_view_stride, void* workspace,
                                size_t workspace_bytes, unsigned long long* close_views_word, int device,
                                void* stream);
SDFR_API int sdfr_render_step_backward_l1_pc(
    const float* loss_grad, float loss_weight, const float* loss_stats, const float* target, const float* depth,
    const float* sdf, int R, long long sdf_view_stride, const float* pos, const float* quat, const float* inv_scale,
    int B, int W, int H, float cx, float cy, float fx, float fy, int sdf_grad_mode, float* g_sdf,
    long long g_sdf_view_stride, void* workspace, size_t workspace_bytes, float pc_weight, const float* points,
    const int* offsets, int max_view_points, const float* scale, void* pc_workspace, size_t pc_workspace_bytes,
    float* loss, float* loss_stats_out, int device, void* stream);
/* ONE LAUNCH for the whole loss-fused step of 1 .. 8 views of the plain grid (sdfr_render_step_forward_l1 with the
 * loss deferred + sdfr_render_step_backward_l1_pc): every image tile marches its rays and, while the depths are still
 * in registers, runs the backward of its hit pixels; the sampler's blocks run beside the tiles as before.  The depth
 * loss is a mean over a count that no tile knows before the launch ends, so the depth term is left UNSCALED, with
 * the bare sign of (estimate - observation) as its upstream gradient:
 *   g_depth  float [B][R^3]   d/dSDF of view b's depth term, unscaled, ADDED to (every view has its own k)
 *   g_sdf    float [R^3]      the point-cloud term of all views (its scale is known), ADDED to
 *     (both NULL: nobody wants d/dSDF -- the tiles and the sampler's blocks then skip it)
 *   workspace (sdfr_render_step_workspace_bytes; offsets by the functions named)
 *     sdfr_render_partials_offset(R, B, W, H, 1)       the tiles' pose sums, unscaled (32 x 8-pixel tiles)
 *     sdfr_render_fused_view_count_offset(B, H)        float [B]     the views' overlap counts, ADDED to (integers
 *                                                      below 2^24 held in floats: exact in any order)
 *     sdfr_render_fused_tile_loss_offset(R, B, W, H)   (sum |est - obs|, count) per tile, 8 floats apart
 * Nothing is zero-filled by this call: whoever consumes a sum clears it (sdfr_decoder_backward_latent_deferred_scaled
 * forms  g_sdf + sum_b k_b g_depth[b],  k_b = weight / count_b, and clears the volumes; sdfr_loop_tail_fused multiplies
 * the pose sums and resets the counts) -- the volumes and the counts must be zero before the FIRST call.
 * depth equals sdfr_render_step_forward_l1's bit for bit; the gradients equal the two launches' up to rounding (k
 * multiplies sums instead of terms).  A view whose observed point set is small (<= 6144 points, tuning.hpp) sends its
 * d/dSDF to the volumes by float atomics directly (no LDS pre-sum: what a small object costs is the depth of a tile's
 * chain of phases); larger ones, and the sampler's blocks of 3 and more views (they share one volume), pre-sum in their
 * LDS tables as the two-launch form does.  sdf_grad_mode: SDFR_SDF_GRAD_EXACT or _CUDA_COMPAT, no flags.  R <= 128.
 * pos / quat / inv_scale / scale: the views' poses (scale = 1 / inv_scale, what the sampler takes). */
SDFR_API size_t sdfr_render_fused_view_count_offset(int B, int H);
SDFR_API size_t sdfr_render_fused_tile_loss_offset(int R, int B, int W, int H);   /* the (sum, count) tile records */
SDFR_API int sdfr_render_step_fused_l1_pc(
    const float* sdf, int R, long long sdf_view_stride, const float* pos, const float* quat, const float* inv_scale,
    const float* scale, int B, int W, int H, float cx, float cy, float fx, float fy, float threshold,
    const float* target, float* depth, int sdf_grad_mode, float* g_sdf, float* g_depth, void* workspace,
    size_t workspace_bytes, float pc_weight, const float* points, const int* offsets, int max_view_points,
    void* pc_workspace, size_t pc_workspace_bytes, int device, void* stream);
/* sdfr_render_step_backward_l1 = sdfr_render_backward_l1 as the second half of a step begun by
 * sdfr_render_step_forward_l1 (no prologue launch, the forward's view records and rectangles; pos / quat / inv_scale
 * are not passed again) -- the loss-fused form of sdfr_render_step_backward.
 * DEFERRED LOSS (both step backward forms): a step's forward called with loss = loss_stats = NULL leaves its per-tile
 * (sum, count) records unreduced -- no reduce launch between the two image kernels -- and the step's backward is then
 * given loss_stats = NULL and the two OUTPUTS loss [B], loss_stats_out [B][2]: every backward tile with a hit pixel
 * sums its view's counts itself (integers: exact in any order, so the upstream gradient is the same bit for bit) and
 * one workgroup per view writes loss / loss_stats_out in the reduce launch's fixed order (the same bits too), valid
 * after this call.  loss = loss_stats_out = NULL: loss_stats comes from the forward, as before. */
SDFR_API int sdfr_render_step_backward_l1(const float* loss_grad, float loss_weight, const float* loss_stats,
                                 const float* target, const float* depth, const float* sdf, int R,
                                 long long sdf_view_stride, int B, int W, int H, float cx, float cy, float fx,
                                 float fy, int sdf_grad_mode, float* g_sdf, long long g_sdf_view_stride, float* g_pos,
                                 float* g_quat, float* g_inv_scale, void* workspace, size_t workspace_bytes,
                                 float* loss, float* loss_stats_out, int device, void* stream);
/* byte offset of the backward's tile partials in its workspace (step_layout: of a step's workspace) */
SDFR_API size_t sdfr_render_partials_offset(int R, int B, int W, int H, int step_layout);
SDFR_API int sdfr_render_step_backward(const float* grad_depth, const float* depth, const float* sdf, int R,
                              long long sdf_view_stride, int B, int W, int H, float cx, float cy,
                              float fx, float fy, int sdf_grad_mode, float* g_sdf,
                              long long g_sdf_view_stride, float* g_pos, float* g_quat,
                              float* g_inv_scale, void* workspace, size_t workspace_bytes, int device,
                              void* stream);

/* ---- render + masked depth-L1 in one pass ------------------------------------ */

/* The depth term of SDFPipeline._compute_view_losses (sdfest/estimation/simple_setup.py:129-135)
 * folded into the renderer, so that neither the loss kernel nor the gradient image exists:
 *     overlap = (target > 0) & (depth > 0);   loss[b] = mean |depth - target| over overlap
 * sdfr_render_forward_l1 = sdfr_render_forward + loss[b] (NaN for an empty overlap, like
 * torch.mean of an empty selection) + loss_stats[b] = {sum |depth - target|, count} (2 floats per
 * view, consumed by the backward).  Sums are reduced in a fixed order (bitwise reproducible).
 *   target [B][H][W]  the observed depth images (read at hit pixels only). */
SDFR_API size_t sdfr_render_forward_l1_workspace_bytes(int R, int B, int W, int H);
SDFR_API int sdfr_render_forward_l1(const float* sdf, int R, long long sdf_view_stride,
                           const float* pos, const float* quat, const float* inv_scale, int B,
                           int W, int H, float cx, float cy, float fx, float fy, float threshold,
                           const float* target, float* depth, float* loss, float* loss_stats,
                           void* workspace, size_t workspace_bytes, int device, void* stream);

/* sdfr_render_backward with the upstream gradient image formed in the kernel:
 *     grad_depth = k_b * sign(depth - target) on the overlap, 0 elsewhere,
 *     k_b = loss_weight * (loss_grad ? loss_grad[b] : 1) / count_b      (0 for an empty overlap)
 * i.e. the gradient of sum_b loss_weight * loss_grad[b] * loss[b].  Results are identical to
 * sdfr_depth_l1_loss followed by sdfr_render_backward.  Workspace: sdfr_render_backward_workspace_bytes.
 *   loss_grad [B] DEVICE array or NULL;  loss_stats [B][2] from sdfr_render_forward_l1. */
SDFR_API int sdfr_render_backward_l1(const float* loss_grad, float loss_weight, const float* loss_stats,
                            const float* target, const float* depth, const float* sdf, int R,
                            long long sdf_view_stride, const float* pos, const float* quat,
                            const float* inv_scale, int B, int W, int H, float cx, float cy,
                            float fx, float fy, int sdf_grad_mode, float* g_sdf,
                            long long g_sdf_view_stride, float* g_pos, float* g_quat,
                            float* g_inv_scale, void* workspace, size_t workspace_bytes, int device,
                            void* stream);

/* ==== 1. CORE (continued) ===================================================================== */
/* ---- trilinear SDF sampler of the point-cloud loss --------------------------------------- */

/* Replaces losses.pc_loss (sdfest/estimation/losses.py:32-135), for all views of a step at once.
 *   points  [N][3]   camera-frame points; view v owns [offsets[v], offsets[v+1])
 *   offsets [B+1]    DEVICE int array; NULL is allowed for B == 1 and means [0, max_view_points)
 *   max_view_points  host-side upper bound of the longest segment (sizes the grid)
 *   pos [B][3], quat [B][4] (need not be normalised: the kernel normalises like the reference,
 *   :58), scale [B] (half-width, NOT its inverse)
 *   out     [N]      interpolated distance * scale, 0 for points outside the volume (:92-94,:134) */
SDFR_API int sdfr_pc_loss_forward(const float* points, const int* offsets, int B, int max_view_points,
                         const float* pos, const float* quat, const float* scale,
                         const float* sdf, int R, long long sdf_view_stride, float* out,
                         int device, void* stream);

SDFR_API size_t sdfr_pc_loss_backward_workspace_bytes(int B, int max_view_points);

/* VJP of the above for upstream grad_out[N]; equals torch autograd through losses.py:32-135
 * (the q normalisation is differentiated through; outside points get no gradient).
 * g_sdf is overwritten (stride 0: summed over the views; R^3: per view); g_pos [B][3],
 * g_quat [B][4], g_scale [B] are overwritten, reduced in a fixed order. */
SDFR_API int sdfr_pc_loss_backward(const float* grad_out, const float* points, const int* offsets, int B,
                          int max_view_points, const float* pos, const float* quat,
                          const float* scale, const float* sdf, int R, long long sdf_view_stride,
                          float* g_sdf, long long g_sdf_view_stride, float* g_pos, float* g_quat,
                          float* g_scale, void* workspace, size_t workspace_bytes, int device,
                          void* stream);

/* sdfr_pc_loss_backward for the loss the loop really uses (simple_setup.py:137-144),
 *     loss[v] = mean |pc_loss values of view v|,   objective = weight * sum_v loss[v]:
 * the upstream gradient +-weight / M_v is formed from the sign of each point's value inside the
 * kernel and loss[v] (NaN for a view without points, as torch.mean of nothing) is a by-product, so
 * neither sdfr_pc_loss_forward nor sdfr_pc_l1_loss has to run.  Gradients are identical to
 * forward -> sdfr_pc_l1_loss -> sdfr_pc_loss_backward.  Workspace: sdfr_pc_loss_backward_workspace_bytes. */
SDFR_API int sdfr_pc_l1_backward(float weight, float* loss, const float* points, const int* offsets, int B,
                        int max_view_points, const float* pos, const float* quat, const float* scale,
                        const float* sdf, int R, long long sdf_view_stride, float* g_sdf,
                        long long g_sdf_view_stride, float* g_pos, float* g_quat, float* g_scale,
                        void* workspace, size_t workspace_bytes, int device, void* stream);
/* the same, ADDING the d/dSDF contributions to g_sdf instead of overwriting it: in the loop the sampler runs
 * after the renderer's backward and sums into its volume (one zero fill and one addition launch less). */
SDFR_API int sdfr_pc_l1_backward_accumulate(float weight, float* loss, const float* points, const int* offsets, int B,
                        int max_view_points, const float* pos, const float* quat, const float* scale,
                        const float* sdf, int R, long long sdf_view_stride, float* g_sdf,
                        long long g_sdf_view_stride, float* g_pos, float* g_quat, float* g_scale,
                        void* workspace, size_t workspace_bytes, int device, void* stream);


/* ---- VAE decoder forward ------------------------------------------------------------------ */

/* Replaces SDFDecoder.forward / SDFVAE.decode (sdfest/vae/sdf_vae.py:217-259, :79-87).
 * The handle owns a device copy of the weights (re-laid-out for the kernels); creation is the
 * only call of this library that allocates device memory and synchronises.
 *   h_params   HOST pointer: the decoder's tensors flattened in state_dict order
 *              (decoder._fc_layers.{i}.weight [out][in], .bias, ..., decoder._conv_layers.{i}
 *              .weight [cout][cin][k][k][k], .bias)
 *   the five conv_* arrays and fc_out are the yaml's decoder.conv_layers / fc_layers entries
 *   volume     sdf_size (64); tsdf: truncation value or 0 for "False" */
typedef struct sdfr_decoder sdfr_decoder;
SDFR_API int sdfr_decoder_create(const float* h_params, size_t n_params, int latent, int n_fc,
                        const int* fc_out, int n_conv, const int* conv_in_size,
                        const int* conv_cin, const int* conv_cout, const int* conv_k,
                        const int* conv_relu, int volume, float tsdf, int device,
                        sdfr_decoder** out_handle);
SDFR_API void sdfr_decoder_destroy(sdfr_decoder* decoder);
SDFR_API size_t sdfr_decoder_workspace_bytes(const sdfr_decoder* decoder, int N);
/* z [N][latent] -> out [N][volume^3] (the reference returns (N,1,D,D,D)); on the decoder's device.
 * tape: NULL for inference; otherwise sdfr_decoder_tape_bytes(decoder, N) bytes that receive the
 * post-ReLU layer outputs a later sdfr_decoder_backward_latent needs. */
SDFR_API size_t sdfr_decoder_tape_bytes(const sdfr_decoder* decoder, int N);
SDFR_API int sdfr_decoder_forward(const sdfr_decoder* decoder, const float* z, int N, int enforce_tsdf,
                         float* out, float* tape, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Which of two equivalent kernel forms the calls on ONE decoder handle take.  The defaults are the measured-faster forms;
 * the results are the same bit for bit either way (the tests compare the forms through this call).  Per handle: nothing
 * is process-wide.  Returns the option's old value (>= 0) or SDFR_E_INVALID / SDFR_E_NULL.
 *   SDFR_DECODER_OPT_FUSED_RESIZE  how batched forwards treat an up-sampling resize in front of a 3x3x3 layer: 1 (default)
 *                                  inside that layer's patch load where that is faster (fine sizes up to 16), 2 wherever
 *                                  the folded form exists (fine sizes 16, 32, 64), 0 always as its own launch
 *   SDFR_DECODER_OPT_TILED_VJP     1 (default): the transposed resizes of the VJP in one launch each (an LDS-staged block
 *                                  per workgroup); 0: the three single-axis launches it replaces
 *   SDFR_DECODER_OPT_FC_ONE_WAVE   1 (default): the backward of a NARROW Linear stack (every layer input <= 64 wide, e.g.
 *                                  the mug decoder's 8 -> 20 -> 50) runs as one wave out of LDS -- in
 *                                  sdfr_decoder_backward_latent and inside sdfr_loop_tail[_records]; 0: the one-workgroup
 *                                  form wider stacks take
 *   SDFR_DECODER_OPT_FUSED_SINGLE  few latents (the render-and-compare loop decodes ONE): layer pairs as one launch each,
 *                                  the producer recomputed under the consumer's tile.  Bits (default 5 = the pairs that
 *                                  measured faster on MI355X, C5 0.1200 -> 0.1120 ms per iteration):
 *                                  1 an up-sampling resize + the 3x3x3 convolution behind it (sdf_vae.py:235-246),
 *                                  2 the Linear stack + the first convolution (:223-238),
 *                                  4 in the VJP the first transposed resize (+ ReLU mask, swapped 1x1x1 layer, padding)
 *                                    + the transposed convolution that reads it,
 *                                  8 the VJP's following stages likewise, chained through a z-pass epilogue */
#define SDFR_DECODER_OPT_FUSED_RESIZE 0
#define SDFR_DECODER_OPT_TILED_VJP 1
#define SDFR_DECODER_OPT_FC_ONE_WAVE 2
#define SDFR_DECODER_OPT_FUSED_SINGLE 3
SDFR_API int sdfr_decoder_set_option(sdfr_decoder* decoder, int option, int value);
/* Read only: 1 if the calls on this handle take the one-wave form of the Linear stack's leading layers -- at most 8
 * layers, every layer input at most 64 wide, their weights and biases AS THEY LIE in the device image (64-float
 * alignment gaps between the blocks included) within 6144 floats, and SDFR_DECODER_OPT_FC_ONE_WAVE not switched off --,
 * 0 if not, SDFR_E_NULL without a handle.  The one statement of that criterion: what sdfr_loop_tail_fused(decoder_tape)
 * requires, so a caller asks here instead of repeating the arithmetic.  Changes nothing. */
SDFR_API int sdfr_decoder_fc_one_wave(const sdfr_decoder* decoder);
/* [unstable, group 2] Read only: the launches a pass over N latents would make on this handle, in order, one
 * SDFR_DECODER_STEP_* code per launch -- the answer of the planner the calls themselves launch from, for caller
 * buffers that are 256-byte aligned (a pointer that is not 16-byte aligned can cost a call its 16-byte load forms).
 * Launches nothing and takes no stream.  pass: SDFR_DECODER_PASS_FORWARD with flags PLAN_TAPE (a taped forward),
 * PLAN_CLAMP (enforce_tsdf), PLAN_STAGE_1 or PLAN_STAGE_2 (sdfr_decoder_forward_stage's stages 1 / 2; neither: both);
 * SDFR_DECODER_PASS_VJP with flags PLAN_DEFERRED (the _deferred forms: the last launch is the caller's), PLAN_SCALED_1
 * or PLAN_SCALED_N (the _deferred_scaled form with one / several views, N = 1).  Returns the number of steps and writes
 * the first `capacity` of them to steps; 0 for N = 0; SDFR_E_NULL without a handle, SDFR_E_INVALID for an unknown pass
 * or flags that are not that pass's. */
#define SDFR_DECODER_PASS_FORWARD 0
#define SDFR_DECODER_PASS_VJP 1
#define SDFR_DECODER_PLAN_TAPE 1
#define SDFR_DECODER_PLAN_CLAMP 2
#define SDFR_DECODER_PLAN_STAGE_1 4
#define SDFR_DECODER_PLAN_STAGE_2 8
#define SDFR_DECODER_PLAN_DEFERRED 16
#define SDFR_DECODER_PLAN_SCALED_1 32
#define SDFR_DECODER_PLAN_SCALED_N 64
/* forward: the Linear stack (NARROW: its one-wave form), alone or with the first convolution (FC_CONV) */
#define SDFR_DECODER_STEP_FC_STACK 1
#define SDFR_DECODER_STEP_FC_STACK_NARROW 2
#define SDFR_DECODER_STEP_FC_STACK_BATCH 3
#define SDFR_DECODER_STEP_FC_STACK_BATCH_NARROW 4
#define SDFR_DECODER_STEP_FC_CONV 5
/* a trilinear resize: gathered, tiled (batches), with a swapped 1x1x1 layer's channel mix */
#define SDFR_DECODER_STEP_RESIZE 6
#define SDFR_DECODER_STEP_RESIZE_TILED 7
#define SDFR_DECODER_STEP_RESIZE_MIX 8
/* a convolution (VJP: the transposed one): 1x1x1, direct (batches; UP: with the resize in front of it), on the matrix
 * cores (plain, split-K, z-grouped, input resident in LDS; UP: few latents, with the resize in front of it) */
#define SDFR_DECODER_STEP_CONV1X1 9
#define SDFR_DECODER_STEP_CONV1X1_VEC4 10
#define SDFR_DECODER_STEP_DIRECT 11
#define SDFR_DECODER_STEP_DIRECT_UP 12
#define SDFR_DECODER_STEP_MFMA 13
#define SDFR_DECODER_STEP_MFMA_SPLIT_K 14
#define SDFR_DECODER_STEP_MFMA_Z_GROUPED 15
#define SDFR_DECODER_STEP_MFMA_RESIDENT 16
#define SDFR_DECODER_STEP_MFMA_UP 17
#define SDFR_DECODER_STEP_COPY 18
#define SDFR_DECODER_STEP_CLAMP 19
/* VJP: the scaled form's sum, mask + padding, a transposed resize (tiled: one launch; else z + y, single axes, the x
 * pass with mask + padding, with the swapped 1x1x1 layer too), a fused stage (transposed resize + convolution), the
 * transposed Linear layers (the wide one; the leading ones, WAVE: their one-wave form) */
#define SDFR_DECODER_STEP_SCALED_COMBINE 20
#define SDFR_DECODER_STEP_PAD_MASK 21
#define SDFR_DECODER_STEP_RESIZE_T_TILED 22
#define SDFR_DECODER_STEP_RESIZE_T_ZY 23
#define SDFR_DECODER_STEP_RESIZE_T_AXIS 24
#define SDFR_DECODER_STEP_RESIZE_T_X_PAD 25
#define SDFR_DECODER_STEP_RESIZE_T_X_MIX_PAD 26
#define SDFR_DECODER_STEP_VJP_STAGE 27
#define SDFR_DECODER_STEP_FC_LAST_T 28
#define SDFR_DECODER_STEP_FC_LAST_T_BATCH 29
#define SDFR_DECODER_STEP_FC_STACK_T 30
#define SDFR_DECODER_STEP_FC_STACK_T_WAVE 31
SDFR_API int sdfr_decoder_launch_plan(const sdfr_decoder* decoder, int pass, int N, int flags, int* steps, int capacity);
/* Vector-Jacobian product of the decoder w.r.t. the latent, weights held constant: what
 * loss.backward() propagates to latent_shape in SDFPipeline.__call__
 * (sdfest/estimation/simple_setup.py:413-414, :456) through SDFDecoder.forward
 * (sdfest/vae/sdf_vae.py:217-259).  grad_out [N][volume^3] -> g_z [N][latent].
 * `tape` comes from the forward of the same z with enforce_tsdf = 0.  Deterministic (no atomics). */
SDFR_API size_t sdfr_decoder_backward_workspace_bytes(const sdfr_decoder* decoder, int N);
SDFR_API int sdfr_decoder_backward_latent(const sdfr_decoder* decoder, const float* z, const float* tape,
                                 const float* grad_out, int N, float* g_z, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* The same for ONE latent without its last launch (the backward of the small leading Linear layers, one workgroup):
 * *t_mid receives where, inside `workspace`, the gradient w.r.t. the wide layer's input lies; sdfr_loop_tail finishes
 * the product rule in its own launch.  Nothing else may use the workspace in between. */
SDFR_API int sdfr_decoder_backward_latent_deferred(const sdfr_decoder* decoder, const float* z, const float* tape,
                                          const float* grad_out, void* workspace, size_t workspace_bytes,
                                          void* stream, const float** t_mid);
/* sdfr_decoder_forward in two halves that meet in the tape (tape != NULL): stages = 1 the Linear stack only (z -> the
 * wide layer's output, in the tape's slot; out may be NULL), 2 the convolutional part from that slot (z is not read),
 * 3 both = sdfr_decoder_forward.  For the captured loop, whose tail launch leaves the NEXT iteration's Linear-stack
 * output in the tape (sdfr_loop_tail_fused, decoder_tape): its decode is then stage 2 alone, stage 1 runs once in
 * front of the first iteration.  Same kernels, same numbers. */
SDFR_API int sdfr_decoder_forward_stage(const sdfr_decoder* decoder, const float* z, int N, int enforce_tsdf,
                               float* out, float* tape, void* workspace, size_t workspace_bytes,
                               void* stream, int stages);
/* sdfr_decoder_backward_latent_deferred for an incoming gradient in 1 + n_scaled volumes, n_scaled of them not yet
 * normalised:
 *     grad = grad_out + sum_v k_v * grad_scaled[v],   k_v = count[v] > 0 ? weight / count[v] : 0   (count: device floats)
 * -- what sdfr_render_step_fused_l1_pc leaves: the point-cloud term, and every view's depth term before its division by
 * the view's overlap count.  With one scaled volume the first launch of the VJP forms the sum as it loads (decoders
 * whose first launch cannot, and n_scaled > 1, get it from one small launch in front), and ALL the volumes are
 * zero-filled once they have been read -- their producer adds into them.  volume^3 a multiple of 4, the volumes
 * 16-byte aligned, grad_scaled [n_scaled][volume^3], n_scaled <= 64. */
SDFR_API int sdfr_decoder_backward_latent_deferred_scaled(const sdfr_decoder* decoder, const float* z, const float* tape,
                                                 float* grad_out, float* grad_scaled, int n_scaled, const float* count,
                                                 float weight, void* workspace, size_t workspace_bytes, void* stream,
                                                 const float** t_mid);
/* ... and for N latents (the K objects of a frame): *t_mid is [N][width of the wide layer's input]; sdfr_loop_tail_objects
 * finishes object k's product rule from row k. */
SDFR_API int sdfr_decoder_backward_latent_deferred_batch(const sdfr_decoder* decoder, const float* z, const float* tape,
                                                const float* grad_out, int N, void* workspace, size_t workspace_bytes,
                                                void* stream, const float** t_mid);


/* ==== 3. LOOP ================================================================================= */
/* ---- glue of one render-and-compare iteration (SDFPipeline.__call__, simple_setup.py:408-470) --- */
/* Small kernels that replace the reference's per-iteration torch-op soup so that a whole
 * iteration is a fixed launch sequence (graph-capturable).  All pointers are device pointers. */

/* :411, :424-430 -- world-frame pose (position[3], orientation[4] un-normalised, scale[1]) to
 * the V camera frames: pos_c [V][3], quat_c [V][4], inv_scale [V] (= 1/scale), scale_v [V]. */
SDFR_API int sdfr_pose_to_views(const float* position, const float* orientation, const float* scale,
                       const float* cam_pos, const float* cam_quat, int V, float* pos_c,
                       float* quat_c, float* inv_scale, float* scale_v, int device, void* stream);

/* reverse of the above: per-view gradients from the renderer (ga_*: w.r.t. pos_c, quat_c,
 * inv_scale) and from the sampler (gb_*: w.r.t. pos_c, quat_c, scale), any of which may be NULL,
 * to g_position[3], g_orientation[4] (through the normalisation), g_scale[1]. */
SDFR_API int sdfr_views_to_pose_grad(const float* orientation, const float* scale, const float* cam_quat,
                            int V, const float* ga_pos, const float* ga_quat,
                            const float* ga_inv_scale, const float* gb_pos, const float* gb_quat,
                            const float* gb_scale, float* g_position, float* g_orientation,
                            float* g_scale, int device, void* stream);

/* The same chain with the two per-view reductions that precede it folded in: three launches of a
 * launch-bound loop in one.  Call sdfr_render_backward / _l1 with g_pos = g_quat = g_inv_scale = NULL and
 * sdfr_pc_loss_backward / sdfr_pc_l1_backward / _accumulate with g_pos = g_quat = g_scale = NULL ("deferred": they
 * then leave their per-tile / per-block partial sums in their workspaces and skip their reduce launch), then
 * pass those workspaces here, untouched in between, with the same V (= B), W, H, offsets, max_view_points and the
 * per-view quaternions quat_c the sampler was given.  Either workspace may be NULL (term absent).  pc_loss [V]:
 * the loss values of sdfr_pc_l1_backward* (which does not write them when deferred), NULL for the plain backward.
 * Same sums in the same order as the three separate launches (results agree to the last bit or two).  V <= 64. */
SDFR_API int sdfr_views_to_pose_grad_deferred(const float* orientation, const float* scale, const float* cam_quat,
                                     int V, const void* render_workspace, int W, int H,
                                     const void* pc_workspace, const int* offsets, int max_view_points,
                                     const float* quat_c, float* pc_loss, float* g_position,
                                     float* g_orientation, float* g_scale, int device, void* stream);

/* The tail of one iteration of the captured loop in ONE launch (one workgroup): sdfr_views_to_pose_grad_deferred (the
 * pose gradients go to grads[0..7]), sdfr_point_constraint (con_source NULL: none), sdfr_adam_step on params /
 * grads [position 3 | orientation 4 | scale 1 | latent n_params - 8] (grads[8..] must hold the latent gradient
 * already), and sdfr_pose_to_views for the NEXT iteration (pos_c / quat_c / inv_scale / scale_v are read by the
 * chain as this iteration's and then overwritten with the next one's).  Same arithmetic in the same order as the
 * four calls.  render_partials_offset: sdfr_render_partials_offset (the tile partials of a stand-alone or of a
 * step's backward).  decoder / decoder_t_mid (both or neither): the tail first runs the last stage of the decoder's
 * VJP that sdfr_decoder_backward_latent_deferred left out -- grads[8..] = d/d latent from decoder_t_mid, the latent
 * being params[8..] -- one launch less per iteration, same arithmetic. */
SDFR_API int sdfr_loop_tail(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int* step, int n_params,
                   float lr_position, float lr_orientation, float lr_scale, float lr_latent, int update_latent,
                   const float* cam_pos, const float* cam_quat, int V, const void* render_workspace,
                   size_t render_partials_offset, int W, int H, const void* pc_workspace, const int* offsets,
                   int max_view_points, float* pos_c, float* quat_c, float* inv_scale, float* scale_v, float* pc_loss,
                   const float* con_source, const float* con_target, float con_weight, float* con_loss,
                   const sdfr_decoder* decoder, const float* decoder_t_mid, int device, void* stream);

/* sdfr_loop_tail behind sdfr_render_step_fused_l1_pc (the render pair as ONE launch): the tiles' pose sums of the
 * depth term come unscaled, beside the views' overlap counts -- the per-view reduction multiplies them by
 * k = depth_weight / count (the expression of the two-launch form's tiles), writes depth_loss [V] (nullable) =
 * sum |est - obs| / count from the tiles' records, and RESETS the counts for the next step.  view_count_offset /
 * tile_loss_offset: sdfr_render_fused_view_count_offset / _tile_loss_offset.  Everything else as sdfr_loop_tail. */
SDFR_API int sdfr_loop_tail_fused(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int* step, int n_params,
                         float lr_position, float lr_orientation, float lr_scale, float lr_latent, int update_latent,
                         const float* cam_pos, const float* cam_quat, int V, void* render_workspace,
                         size_t render_partials_offset, size_t view_count_offset, size_t tile_loss_offset,
                         float depth_weight, float* depth_loss, int W, int H, const void* pc_workspace,
                         const int* offsets, int max_view_points, float* pos_c, float* quat_c, float* inv_scale,
                         float* scale_v, float* pc_loss, const float* con_source, const float* con_target,
                         float con_weight, float* con_loss, const sdfr_decoder* decoder, const float* decoder_t_mid,
                         float* decoder_tape, unsigned* arrivals, int device, void* stream);
/* decoder_tape / arrivals (both or neither; with decoder, update_latent and a Linear stack whose leading layers are
 * at most 64 wide): the launch ALSO runs the decoder's Linear stack for the parameters it has just updated and leaves
 * the wide layer's output in the tape's slot -- the next iteration's decode is sdfr_decoder_forward_stage(stages = 2),
 * one launch less per iteration.  The launch then has one workgroup per 256 outputs of the wide layer: every one
 * repeats the latent's share of the tail (its gradient, its Adam step -- same inputs, same arithmetic, same numbers;
 * nothing is handed from workgroup to workgroup) and forms its slice; workgroup 0 is the tail proper and stores the
 * state.  arrivals: one device word, zero before a run's first iteration -- the other workgroups count themselves in
 * once they have read the state, workgroup 0 stores the new state only when all have (a bounded wait). */

/* sdfr_loop_tail for SEVERAL estimates at once -- the K detected objects of one frame, each with its own pose, scale,
 * latent and Adam state, optimised side by side in one launch sequence (the reference runs its pipeline once per object,
 * one after the other: simple_setup.py:213-225; a single estimate's iteration is a chain of dependent launches that
 * leaves most of the chip idle).  Workgroup k is object k:
 *   params / grads / exp_avg / exp_avg_sq  [K][n_params];  step [K]  (one counter per object)
 *   the launch's views are object-major: object k owns views k V .. k V + V - 1 of the render / sampler launches
 *   (set-up records, tile partials, point blocks, quat_c, pc_loss, and the pos_c / quat_c / inv_scale / scale_v written
 *   for the next iteration: all [K V ...]); cam_pos [V][3], cam_quat [V][4] are ONE camera list, the same for every object
 *   decoder == NULL: grads[k][8..] must hold d loss / d latent of object k (sdfr_decoder_backward_latent with N = K);
 *   decoder + decoder_t_mid (sdfr_decoder_backward_latent_deferred_batch with N = K, row k = object k): workgroup k runs
 *   the last stage of object k's VJP itself, as sdfr_loop_tail does for the single estimate (one launch less, and no
 *   copy of the latent gradients into `grads`)
 *   latents (may be NULL): [K][n_params - 8], receives the UPDATED latents packed for the next iteration's batched
 *   decode (sdfr_decoder_forward with N = K reads z [N][latent]; `params` holds them with stride n_params)
 *   No point constraint.  Same arithmetic per object, in the same order, as sdfr_loop_tail. */
/* sdfr_pose_to_views for the K rows of `params` ([K][n_params]: position 3 | orientation 4 | scale 1 | ...) and one camera
 * list: view k V + v of the outputs is object k seen from camera v; latents (may be NULL): as above, the CURRENT ones. */
SDFR_API int sdfr_pose_to_views_objects(const float* params, int n_params, int n_objects, const float* cam_pos,
                               const float* cam_quat, int V, float* pos_c, float* quat_c, float* inv_scale,
                               float* scale_v, float* latents, int device, void* stream);
SDFR_API int sdfr_loop_tail_objects(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int* step, int n_params,
                           int n_objects, float lr_position, float lr_orientation, float lr_scale, float lr_latent,
                           int update_latent, const float* cam_pos, const float* cam_quat, int V,
                           const void* render_workspace, size_t render_partials_offset, int W, int H,
                           const void* pc_workspace, const int* offsets, int max_view_points, float* pos_c,
                           float* quat_c, float* inv_scale, float* scale_v, float* pc_loss,
                           const sdfr_decoder* decoder, const float* decoder_t_mid, float* latents, int device,
                           void* stream);

/* Around that tail once an object has V > 1 views (pipeline.MultiObjectRenderAndCompare(views=V)): the render and sampler
 * launches take one SDF volume per VIEW (sdf_view_stride) and leave one d/dSDF volume per view, the decoder and its VJP
 * work per OBJECT.  Rows of n floats (n = R^3), object-major:
 *   sdfr_volumes_replicate   src [K][n] -> dst [K V][n]:  dst[k V + v] = src[k]                      (bit copies)
 *   sdfr_volumes_sum_views   src [K V][n] -> dst [K][n]:  dst[k] = ((src[k V] + src[k V + 1]) + ...) in fp32, v
 *                            ascending: one fixed order per element, the same bits on every run
 * One launch each over (chunks of a row, K); 16-byte accesses for every row that starts on a 16-byte boundary (all of
 * them when n is a multiple of 4 and the buffers are aligned), float by float for the others.  K = 0 or n = 0: nothing is
 * launched.  V < 1, K < 0 or K > 65535: SDFR_E_INVALID. */
SDFR_API int sdfr_volumes_replicate(const float* src, float* dst, int K, int V, size_t n, int device, void* stream);
SDFR_API int sdfr_volumes_sum_views(const float* src, float* dst, int K, int V, size_t n, int device, void* stream);

/* sdfr_inlier_ratio (below) for the K objects of sdfr_loop_tail_objects, after it, in two launches whatever K is -- a
 * count grid over (chunks of 1024 pixels, K) and K update workgroups; integer atomics only:
 *   depth_input [K][H][W];  depth_estimate: image k starts at depth_estimate + k * estimate_stride floats (>= W H: with
 *   V views per object the caller passes the LAST view of the [K][V][H][W] estimates, stride V W H; :463-470)
 *   step [K], counts [K][2] (zero on the first call, left zero), history [K][max_history] (may be NULL),
 *   state [K][3], params / best_params [K][n_params]
 * Per object exactly sdfr_inlier_ratio: the same expression per pixel, integer counts, ratio = (float)inliers /
 * (float)valid (0 / 0 stays NaN), history[k][step[k] - 1] written only for 1 <= step[k] <= max_history, a strictly larger
 * ratio, or the first, copies row k of params.  K = 0: nothing is launched. */
SDFR_API int sdfr_inlier_ratio_objects(const float* depth_input, const float* depth_estimate, size_t estimate_stride,
                              int K, int W, int H, float relative_threshold, const int* step, int* counts,
                              float* history, int max_history, float* state, const float* params, int n_params,
                              float* best_params, int device, void* stream);

/* ---- N orientation hypotheses of ONE object (SDFPipeline.estimate_hypotheses; the reference has no counterpart: it
 * refines the one argmax cell, and "init_view: best" picks a view, not a cell) ---------------------------------------
 * The N most probable cells (sdfr_orientation_topk, sdfr_init_hypotheses: group 4) are N rows of the K-object loop on
 * N copies of the object's images; this is the way back from N rows to one answer, on the device. */
#define SDFR_MAX_HYPOTHESES 32

/* j* = argmax over j < N of score[j * score_stride]; out_row[0..n) = rows[j*][0..n) (rows [N][n], bit copies),
 * out_index[0] = j*, out_score[0] = the winning score's bits.  Equal scores: the smaller j (the more probable cell).
 * A NaN counts as -inf: never taken while a finite score is left; all NaN gives row 0.  The loop's scores: column
 * max_iterations - 1 of sdfr_inlier_ratio_objects' history (stride max_history), or its state's best ratios (stride 3).
 * One wave, one launch, no atomics, nothing allocated.  1 <= N <= SDFR_MAX_HYPOTHESES, score_stride >= 1, n >= 0. */
SDFR_API int sdfr_select_row(const float* score, int score_stride, int N, const float* rows, int n, float* out_row,
                             int* out_index, float* out_score, int device, void* stream);

/* ---- the loop sharded over ranks (one process per GPU) ------------------------------------------------
 * The reference's multi-view iteration is one Python loop over the views with ONE shared pose and ONE shared SDF
 * (simple_setup.py:420-446, update :456-462).  Sharded, every rank renders and samples a contiguous shard of the
 * views and the iteration has exactly one exchange, an all-reduce (sum) of one bucket
 *     [ d loss / d SDF, R^3 words ][ V_total view records of SDFR_VIEW_RECORD_FLOATS floats ]
 * after which every rank runs the same decoder VJP and the same Adam step on replicated state (no broadcast).
 * A view's record: [0..7] the renderer's pose sums (g_pos 3, g_quat 4, g_inv_scale), [8..15] the sampler's (g_pos 3,
 * g_quat 4 through the normalisation's Jacobian, g_scale), [16] its depth loss, [17] its point-cloud loss, rest 0.
 * Records instead of the 8 summed pose gradients: each is non-zero on exactly one rank, so the sum over ranks
 * reproduces it exactly, and the chain adds the views in one fixed order on every rank (thread t of the tail's
 * workgroup the views t, t + 256, ..., then a fixed tree: any number of views) -- the pose gradient does not
 * depend on how the views were spread (with SDFR_SDF_GRAD_DETERMINISTIC | SDFR_BWD_SMALL_TILES the whole iteration
 * is bitwise the single-process one; exchange the bucket as 64-bit integers then, the volume being the int64 one).
 *
 * sdfr_loop_view_records: one launch, one wave per view of the whole list: records[v] for this rank's views
 * [view_begin, view_begin + V_local) from the partials the deferred backward calls left (as
 * sdfr_views_to_pose_grad_deferred: render_workspace + sdfr_render_partials_offset, pc_workspace; either may be NULL;
 * with_pc_loss: the sampler ran in its L1 form and left loss partials), zeros for every other view.  loss_depth
 * [V_local] (or NULL): per-view depth losses to carry along.  sdf_grad_mode: the backward's (SDFR_BWD_SMALL_TILES). */
#define SDFR_VIEW_RECORD_FLOATS 20
SDFR_API int sdfr_loop_view_records(const void* render_workspace, size_t render_partials_offset, int W, int H,
                           int sdf_grad_mode, const void* pc_workspace, int with_pc_loss, const int* offsets,
                           int max_view_points, const float* quat_c, const float* loss_depth, int view_begin,
                           int V_local, int V_total, float* records, int device, void* stream);
/* sdfr_loop_tail working from the exchanged records of ALL views: (decoder VJP's last stage,) the chain over the
 * V_total records with cam_quat [V_total][4], the point constraint, Adam, and the next iteration's view poses for
 * this rank's shard (cam_pos / cam_quat are the whole lists; pos_c / quat_c / inv_scale / scale_v [V_local]). */
/* The inlier bookkeeping of sdfr_inlier_ratio split around the exchange: the rank that owns the LAST view counts
 * (sdfr_inlier_counts_record: the two counts, as floats -- exact below 2^24 pixels -- into words 18 and 19 of that
 * view's record, after sdfr_loop_view_records), every rank updates from the exchanged record after the tail
 * (sdfr_inlier_update_record: ratio, history, best-so-far state and parameters as sdfr_inlier_ratio). */
SDFR_API int sdfr_inlier_counts_record(const float* depth_input, const float* depth_estimate, int W, int H,
                              float relative_threshold, int* counts, float* record, int device, void* stream);
SDFR_API int sdfr_inlier_update_record(const float* record, const int* step, float* history, int max_history,
                              float* state, const float* params, int n_params, float* best_params, int device,
                              void* stream);
SDFR_API int sdfr_loop_tail_records(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int* step, int n_params,
                           float lr_position, float lr_orientation, float lr_scale, float lr_latent,
                           int update_latent, const float* cam_pos, const float* cam_quat, int V_total,
                           int view_begin, int V_local, const float* records, float* pos_c, float* quat_c,
                           float* inv_scale, float* scale_v, const float* con_source, const float* con_target,
                           float con_weight, float* con_loss, const sdfr_decoder* decoder,
                           const float* decoder_t_mid, int device, void* stream);

/* sdfr_render_backward_l1 and sdfr_pc_l1_backward_accumulate of one loop iteration in ONE launch (they are
 * independent and neither fills the chip for a handful of views): arguments as in those two calls -- the per-view
 * poses are pos / quat with inv_scale for the renderer and scale (= 1 / inv_scale) for the sampler -- and the same
 * results in g_sdf (zero-filled first, then both terms added).  The pose gradients are always left deferred in the
 * two workspaces: follow with sdfr_views_to_pose_grad_deferred, which also writes the point-cloud loss values. */
SDFR_API int sdfr_render_backward_l1_pc(
    const float* loss_grad, float loss_weight, const float* loss_stats, const float* target, const float* depth,
    const float* sdf, int R, long long sdf_view_stride, const float* pos, const float* quat, const float* inv_scale,
    int B, int W, int H, float cx, float cy, float fx, float fy, int sdf_grad_mode, float* g_sdf,
    long long g_sdf_view_stride, void* workspace, size_t workspace_bytes, float pc_weight, const float* points,
    const int* offsets, int max_view_points, const float* scale, void* pc_workspace, size_t pc_workspace_bytes,
    int device, void* stream);

/* :125-131 -- loss[v] = mean |estimate - target| over (target > 0) & (estimate > 0) (NaN when the
 * overlap is empty, like torch.mean of an empty selection); grad_estimate = weight * d loss / d
 * estimate.  Deterministic two-pass reduction. */
SDFR_API size_t sdfr_depth_l1_workspace_bytes(int V, int W, int H);
SDFR_API int sdfr_depth_l1_loss(const float* estimate, const float* target, int V, int W, int H,
                       float weight, float* loss, float* grad_estimate, void* workspace,
                       size_t workspace_bytes, int device, void* stream);

/* :144 -- loss[v] = mean |values| over view v's points, grad_values = weight * sign / M_v */
SDFR_API int sdfr_pc_l1_loss(const float* values, const int* offsets, int V, int max_view_points,
                    float weight, float* loss, float* grad_values, int device, void* stream);

/* pointset_utils.depth_to_pointcloud (sdfest/initialization/pointset_utils.py:57-77, convention "opengl",
 * no mask, no normalisation) for V images at once: the non-zero pixels, view-major and row-major,
 *     x = (col - cx0) * z * rfx,  y = -(row - cy0) * z * rfy,  z = -depth     (pixel-centre-0 intrinsics).
 * rfx, rfy are the reciprocal focal lengths: torch evaluates `t / scalar` on the GPU as
 * `t * float(1.0 / scalar)` (reciprocal in double, rounded once), and the caller that holds the double
 * computes exactly that -- the points are then bit-identical to the reference expression's.
 * Two calls because the caller sizes the output: sdfr_depth_count writes counts[v] (DEVICE ints) and
 * the per-block counts into `workspace`; the caller reads the counts, builds the exclusive prefix
 * `offsets` [V] (DEVICE ints) and allocates points [sum][3]; sdfr_depth_to_points fills them from the
 * SAME depth and workspace. */
SDFR_API size_t sdfr_depth_points_workspace_bytes(int V, int W, int H);
SDFR_API int sdfr_depth_count(const float* depth, int V, int W, int H, int* counts, void* workspace,
                     size_t workspace_bytes, int device, void* stream);
SDFR_API int sdfr_depth_to_points(const float* depth, int V, int W, int H, float rfx, float rfy, float cx0,
                         float cy0, const int* offsets, const void* workspace, float* points,
                         int device, void* stream);
/* The same with the ORDER of a view's points chosen by the caller.  SDFR_POINT_ORDER_ROW_MAJOR is the reference's
 * (torch.nonzero).  SDFR_POINT_ORDER_TILED enumerates the image in tiles of 64 x 16 pixels, a tile in four 16 x 16
 * sub-tiles, a sub-tile row-major: the same points, permuted within their view, so that 256 consecutive points are a
 * compact patch of the surface.  For consumers that only sum over a view's points -- the point-cloud loss and its
 * gradients (losses.py:32-135 has no order): the sampler's backward pre-sums the d/dSDF of 256 consecutive points
 * in LDS before its global atomics, and compact patches share more voxels (global atomics per point of
 * back-projected depth images: 0.55 row-major, ~0.3 tiled).  Use the same order in both calls. */
#define SDFR_POINT_ORDER_ROW_MAJOR 0
#define SDFR_POINT_ORDER_TILED 1
SDFR_API int sdfr_depth_count_ordered(const float* depth, int V, int W, int H, int order, int* counts, void* workspace,
                             size_t workspace_bytes, int device, void* stream);
SDFR_API int sdfr_depth_to_points_ordered(const float* depth, int V, int W, int H, int order, float rfx, float rfy,
                                 float cx0, float cy0, const int* offsets, const void* workspace, float* points,
                                 int device, void* stream);
/* The synthetic-view generator's point sets are normalised by their centroid (generated_dataset.py:318-326:
 * pointset -= mean(pointset), position -= mean; optionally + a noise vector).  Both passes over the images do that
 * on the way: sdfr_depth_count_centroid = sdfr_depth_count_ordered that also leaves centroid[v] = mean of view v's
 * back-projected points (fixed-order sums; 0 for an empty view) and, with `offsets` [V] (nullable), the exclusive
 * prefix of the counts that sdfr_depth_to_points_* takes -- the caller reads the counts (to size `points`) -- and
 * sdfr_depth_to_points_shifted writes (points - shift[v]) + noise[v]: two roundings, in the reference's order
 * (`pointset -= centroid`, then `pointset += noise`).  shift / noise [V][3], either may be NULL (that term is
 * skipped: shift = noise = NULL gives the plain points).  No pass over the packed points, no per-point owner index,
 * no atomics.
 * Workspace: sdfr_depth_centroid_workspace_bytes, 16-byte aligned, the same for both calls. */
SDFR_API size_t sdfr_depth_centroid_workspace_bytes(int V, int W, int H);
SDFR_API int sdfr_depth_count_centroid(const float* depth, int V, int W, int H, int order, float rfx, float rfy,
                              float cx0, float cy0, int* counts, int* offsets, float* centroid, void* workspace,
                              size_t workspace_bytes, int device, void* stream);
SDFR_API int sdfr_depth_to_points_shifted(const float* depth, int V, int W, int H, int order, float rfx, float rfy,
                                 float cx0, float cy0, const int* offsets, const void* workspace, const float* shift,
                                 const float* noise, float* points, int device, void* stream);

/* The same pair of passes WITHOUT the host in between, for a caller that re-uses its buffers from observation to
 * observation (the captured render-and-compare loop, rebound to new depth images): `points` has room for every pixel
 * (V * W * H points), so nobody has to read the counts to size it.  One call: block counts -> counts [V] and the
 * exclusive prefix offsets [V + 1] (offsets[V] = all points; the format sdfr_pc_* take) -> compaction.  Consumers are
 * then launched for `max_view_points` = W * H (an upper bound sizes their grids; blocks beyond a view's real count leave
 * at once).  Workspace: sdfr_depth_points_workspace_bytes.  Same points, bit for bit, as the two-call form. */
SDFR_API int sdfr_depth_to_points_resident(const float* depth, int V, int W, int H, int order, float rfx, float rfy,
                                  float cx0, float cy0, int* counts, int* offsets, void* workspace,
                                  size_t workspace_bytes, float* points, int device, void* stream);

/* SDFPipeline._preprocess_depth (sdfest/estimation/simple_setup.py:671-693), IN PLACE like the reference:
 *     depth[~mask] = 0;   if has_far_field: depth[depth > far_field] = 0
 * depth [V][H][W]; mask [V][H][W] bytes (a torch.bool tensor's storage: 0 = outside).  copy_to (nullable): the
 * preprocessed images are also written there (the loop's own target buffer: one pass instead of two). */
SDFR_API int sdfr_preprocess_depth(float* depth, const unsigned char* mask, int V, int W, int H, float far_field,
                          int has_far_field, float* copy_to, int device, void* stream);

/* a += b  (sums the renderer's and the sampler's d/dSDF) */
SDFR_API int sdfr_add_inplace(float* a, const float* b, size_t n, int device, void* stream);

/* :400-406, :458-462 -- one torch.optim.Adam step (default betas/eps) on params laid out
 * [position 3 | orientation 4 | scale 1 | latent ...], then orientation /= |orientation|.
 * step[0] (device int) is the number of steps taken so far and is incremented. */
SDFR_API int sdfr_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int* step, int n_params, float lr_position, float lr_orientation,
                   float lr_scale, float lr_latent, int update_latent, int device, void* stream);

/* :164-175 + losses.py:138-153 -- point constraint on the (un-normalised) orientation parameter:
 * loss[0] = weight * |q (source,0) conj(q) - target| (quaternion_apply, quaternion_utils.py:36-54);
 * its gradient w.r.t. q is ADDED to g_orientation[4].  loss / g_orientation may be NULL. */
SDFR_API int sdfr_point_constraint(const float* orientation, const float* source, const float* target,
                          float weight, float* loss, float* g_orientation, int device, void* stream);

/* :177-211 -- inlier ratio of one view (the reference passes the LAST view's loop variables,
 * :463-470) and the best-estimate bookkeeping: ratio = #(|in - est| / in < relative_threshold) /
 * #(in != 0); history[step[0] - 1] = ratio (if 1 <= step[0] <= max_history; step = sdfr_adam_step's
 * counter, call after it); a strictly larger ratio, or the first, copies params[n_params] to
 * best_params.  state[3] = {best ratio, its 1-based iteration, has_best}: zero it before a run.
 * counts[2] is integer scratch that must be zero on the first call (left zero by every call). */
SDFR_API int sdfr_inlier_ratio(const float* depth_input, const float* depth_estimate, int W, int H,
                      float relative_threshold, const int* step, int* counts, float* history,
                      int max_history, float* state, const float* params, int n_params,
                      float* best_params, int device, void* stream);

/* losses.py:8-29 -- nn_loss: dist[i] = min_j max(0, -2 a_i.b_j + |a_i|^2 + |b_j|^2), nearest[i] = the
 * first minimising j; points are (N,3) / (M,3).  The backward is the VJP autograd gives the
 * reference: through the selected pair, none for a clamped (zero) distance; g_to is overwritten. */
SDFR_API int sdfr_nn_loss_forward(const float* points_from, int N, const float* points_to, int M,
                         float* dist, int* nearest, int device, void* stream);
SDFR_API int sdfr_nn_loss_backward(const float* grad_dist, const float* points_from, int N,
                          const float* points_to, int M, const float* dist, const int* nearest,
                          float* g_from, float* g_to, int device, void* stream);

/* generated_dataset.py:234-245 -- perturbed mask of the view generator: mask[b][i][j] = 1 where the
 * input pixel nearest to M_b (j + 0.5 - W/2, i + 0.5 - H/2, 1) + (W/2 - 0.5, H/2 - 0.5) has depth != 0
 * (0 outside the image); matrices[B][6] = the row-major 2x3 INVERSE affine maps in pixels about the image
 * centre (what torchvision's RandomAffine hands to grid_sample(nearest, align_corners=False)). */
SDFR_API int sdfr_affine_mask(const float* depth, int B, int W, int H, const float* matrices,
                     unsigned char* mask, int device, void* stream);

/* ==== 4. GENERATOR / INITIALISATION (sdfr_affine_mask above; the network below) =============== */
/* ---- initialisation network forward: sdfest/initialization/pointnet.py:7-96,
 * sdf_pose_network.py:9-115, estimation/simple_setup.py:795-812 ------------------------------------ */

/* one per-point layer of VanillaPointNet on a set of M points, inference mode:
 *   Y = relu((X W[:, :cin]^T + cvec) * bn_scale + bn_shift);   y = resid ? resid + Y : Y  (y may be NULL);
 *   colmax[col] = max over the points of Y[:, col]  (written, cout floats).
 * x [M][ldx], w [cout][ldw] as torch stores nn.Linear.weight, y / resid [M][ldy].  bn_scale / bn_shift are
 * the folded BatchNorm1d (gamma / sqrt(var + eps), beta - mean * scale; 1 and 0 without batch norm).
 * A dense link's concatenated set maximum enters through cvec = bias + W[:, cin:] . max (sdfr_linear_vec). */
SDFR_API int sdfr_pointnet_layer(const float* x, int M, int cin, int ldx, const float* w, int ldw,
                        const float* cvec, const float* bn_scale, const float* bn_shift,
                        const float* resid, float* y, int ldy, int cout, float* colmax, int device,
                        void* stream);

/* The same with the number of points ON THE DEVICE (row_count[0], clamped to M_capacity = the rows x, y and resid have
 * room for): for a caller that never reads the count of a depth image's points back -- the initialisation network
 * inside a captured launch sequence (sdfest_amd.init_network.ResidentInit).  The grid strides over the real rows. */
SDFR_API int sdfr_pointnet_layer_counted(const float* x, const int* row_count, int M_capacity, int cin, int ldx,
                                const float* w, int ldw, const float* cvec, const float* bn_scale,
                                const float* bn_shift, const float* resid, float* y, int ldy, int cout,
                                float* colmax, int device, void* stream);

/* y[cout] = act((W[:, koff:koff+k] . x + bias) * bn_scale + bn_shift): the head's layers on the set feature
 * and the bias vectors of dense links.  bias, bn_scale / bn_shift may be NULL; relu = 0 / 1. */
SDFR_API int sdfr_linear_vec(const float* w, int ldw, int koff, const float* x, int k, const float* bias,
                    const float* bn_scale, const float* bn_shift, int relu, float* y, int cout,
                    int device, void* stream);

/* simple_setup.py:795-812, :978-1009 -- posterior[C] = softmax(logits), with a prior: posterior * prior /
 * train_prior (train_prior may be NULL), L1-normalised; out_index = argmax (first maximum), out_max = its
 * probability. */
SDFR_API int sdfr_orientation_posterior(const float* logits, int C, const float* prior, const float* train_prior,
                               float* posterior, int* out_index, float* out_max, int device, void* stream);

/* simple_setup.py:790-838 for one view, on the device: the head's output row -> the estimate in the WORLD frame, written
 * into params [position 3 | orientation 4 | scale 1 | latent] (the loop's parameter vector: sdfr_loop_tail).
 *   head          [latent + 4 + C] (discretised orientation: latent, position, scale, C logits) or [latent + 8]
 *   grid_quats    [C][4] with index = the argmax of sdfr_orientation_posterior (SO3Grid.index_to_quat of every cell,
 *                 uploaded once), or NULL: the head's quaternion, normalised (sdf_pose_network.py:97-101)
 *   centroid [3]  nullable: `position += centroid` (:793-794);  cam_pos [3], cam_quat [4]: camera -> world (:819-825)
 *   mean_shape    zero latent (:790-791)
 *   take_if_better 0: "first" -- always written; 1: "best" -- written only where posterior_max[0] > best[0], which
 *                 then takes its value (:829-838; the caller zeroes best[0] in front of the first view). */
SDFR_API int sdfr_init_estimate(const float* head, int latent, const float* grid_quats, const int* index,
                       const float* centroid, const float* cam_pos, const float* cam_quat, int mean_shape,
                       int take_if_better, const float* posterior_max, float* best, float* params, int device,
                       void* stream);

/* The N largest entries of posterior [C] (what sdfr_orientation_posterior left, prior-adjusted or not), descending:
 * out_index [N], out_prob [N] = posterior[out_index] (its bits).  Equal values: the smaller index first (-0 = +0).  A
 * NaN counts as -inf: it is never taken while a finite number is left -- the rule of sdfr_orientation_posterior's argmax
 * (`p > best` from best = -1), so entry 0 is that call's out_index / out_max.  One workgroup, N passes over the
 * posterior, which is only read; integer comparisons only: the same bits on every run.
 * 1 <= N <= SDFR_MAX_HYPOTHESES, N <= C <= 2^24. */
SDFR_API int sdfr_orientation_topk(const float* posterior, int C, int N, int* out_index, float* out_prob, int device,
                                   void* stream);

/* N starts of the loop from one estimate: params [N][n_params], row j = params_one [n_params] (the row
 * sdfr_init_estimate wrote: [position 3 | orientation 4 | scale 1 | latent], world frame) bit for bit, except
 * orientation = cam_quat (x) grid_quats[index[j]] -- sdfr_init_estimate's own product, rounding for rounding, so the row
 * of the argmax cell is params_one itself.  grid_quats [C][4]; index [N] on the device (sdfr_orientation_topk's
 * out_index), clamped to [0, C) there.  params must not overlap params_one.  8 <= n_params <= 8 + 1024. */
SDFR_API int sdfr_init_hypotheses(const float* params_one, int n_params, const float* grid_quats, int C,
                                  const int* index, int N, const float* cam_quat, float* params, int device,
                                  void* stream);

/* ---- the same network on N point sets per launch (eval() over a validation set: sdfest/initialization/scripts/
 * train.py:439-481) -- csrc/initnet_eval.hip.  Row n of every result has the bits of the single-set call on set n: the
 * same tile, the same k chunks, the same reductions; it depends neither on N nor on the other sets nor on M_capacity. */

/* sdfr_pointnet_layer for N sets: x [N][M_capacity][ldx], y / resid [N][M_capacity][ldy] (both nullable), colmax
 * [N][cout] (written).  counts: device int [N], the real rows of every set, clamped to [0, M_capacity]; NULL: every
 * set has M_capacity rows.  Rows past counts[n] are neither read into a result nor written; a set without rows gets 0
 * in every column of colmax.  cvec_stride = 0: cvec [cout] is shared; = cout: cvec [N][cout], one per set (a dense
 * link's bias + W[:, cin:] . max[n], sdfr_linear_rows).  bn_scale / bn_shift [cout] are shared.
 * pool_resid = 0: colmax = max over the rows of Y, and y = resid + Y needs y as in sdfr_pointnet_layer.
 * pool_resid = 1 (a residual link into the LAST layer, pointnet.py:88-96): colmax = max over the rows of resid + Y,
 * of any sign; y may be NULL.  With y == NULL nothing but colmax is stored.  1 <= N <= 65535, N M_capacity <= 2^30. */
SDFR_API int sdfr_pointnet_layer_batch(const float* x, const int* counts, int N, int M_capacity, int cin, int ldx,
                                       const float* w, int ldw, const float* cvec, int cvec_stride,
                                       const float* bn_scale, const float* bn_shift, const float* resid, float* y,
                                       int ldy, int cout, int pool_resid, float* colmax, int device, void* stream);

/* sdfr_linear_vec on N rows: y[n] = act((W[:, koff:koff+k] . x[n] + bias) * bn_scale + bn_shift), x [N][ldx],
 * y [N][ldy]; every (row, column) is summed in sdfr_linear_vec's order.  1 <= N <= 65535. */
SDFR_API int sdfr_linear_rows(const float* w, int ldw, int koff, const float* x, int ldx, int k, const float* bias,
                              const float* bn_scale, const float* bn_shift, int relu, float* y, int ldy, int cout, int N,
                              int device, void* stream);

/* The validation numbers of train.py:439-481 (and the "metric geodesic distance" of :344-374) for one batch, added to
 * record [5] (fp64, caller-owned, zeroed by the caller in front of a validation set):
 *   record[0] += sum |p - p*|_2          record[1] += sum |s - s*|
 *   record[2] += sum 2 acos(clip(|q . q*|, 0, 1))
 *   record[3] += sum (logsumexp(logits) - logits[orientation_index])   (n_cells > 0 and orientation_index != NULL)
 *   record[4] += N
 * out [N][ld_out]: the head's rows, latent [latent], position [3], scale [1], then n_cells logits or (n_cells = 0) the
 * quaternion before its normalisation.  q = grid_quats [n_cells][4] at the FIRST maximum of the logits
 * (sdfr_orientation_posterior's rule), or the row's quaternion normalised.  Targets: position [N][3], scale [N],
 * quat [N][4], orientation_index [N] (nullable; clamped to the table).  Per sample in fp64 by one wave, into
 * workspace (sdfr_pose_metrics_workspace_bytes(N), 8-byte aligned); then ONE thread adds the N samples to the record in
 * sample order: no atomics, the same batches in the same order give the same bits. */
SDFR_API size_t sdfr_pose_metrics_workspace_bytes(int N);   /* 0: N < 1 */
SDFR_API int sdfr_pose_metrics(const float* out, int N, int ld_out, int latent, int n_cells, const float* grid_quats,
                               const float* position, const float* scale, const float* quat,
                               const int* orientation_index, double* record, void* workspace, size_t workspace_bytes,
                               int device, void* stream);

/* ==== 5. MESH ================================================================================= */
/* ---- marching cubes: simple_setup.py:621-669 (generate_mesh: skimage.measure.marching_cubes) ----------------------
 * N grids sdf [N][R][R][R] (2 <= R <= 256), each its own mesh.  complete = 1: every grid inside a virtual border of
 * 1.0 (the reference's F.pad(sdf, (1,)*6, value=1.0); nothing is copied), side M = R + 2; else M = R.
 *   a corner is inside iff v < level; one vertex per crossed grid edge, shared by its triangles (a welded mesh)
 *   vertex order: grid point g = (i M + j) M + k ascending, then its edges along axis 0, 1, 2
 *   face order:   cell (minimum corner g) ascending, then the case table's triangle order
 *   position:     (a + t (b - a)) s - s (M - 1) / 2 per axis, t = (level - v_a) / (v_b - v_a), s = 2 / (R - 1)
 *   winding:      (b - a) x (c - a) points toward increasing SDF
 *   normals:      np.gradient of the (padded) grid at both edge ends, lerped by t, normalised (0 where it vanishes)
 * Integer scans only: the same bits every run, whatever N.  Two calls with the same arguments and workspace:
 *   sdfr_mesh_count  totals [N][4] (device int32) = {V, F, min, max} per grid (min / max of the padded volume as
 *                    float bits: skimage raises unless min <= level <= max); the caller reads them back, then
 *   sdfr_mesh_emit   vertices [sum V][3] float, normals [sum V][3] float (nullable), faces [sum F][3] int32 with the
 *                    grids one after the other; face indices are local to their grid's vertices.  `totals` is the
 *                    count's (still on the device); sdf, level, complete and the workspace are the count's too. */
/* host copies of the case tables (no GPU needed): edge_mask[256] (bit e = edge e crossed), tri_table[256][16] (up
 * to five edge triples, -1 terminated).  Corner c = dx + 2 dy + 4 dz; edge e = 4 a + (the other two offsets, the
 * lower axis first) along axis a. */
SDFR_API int sdfr_mesh_tables(unsigned short* h_edge_mask, signed char* h_tri_table);
SDFR_API size_t sdfr_mesh_workspace_bytes(int N, int R, int complete);   /* 0 for invalid arguments */
SDFR_API int sdfr_mesh_count(const float* sdf, int N, int R, int complete, float level, int* totals,
                             void* workspace, size_t workspace_bytes, int device, void* stream);
SDFR_API int sdfr_mesh_emit(const float* sdf, int N, int R, int complete, float level, const int* totals,
                            float* vertices, float* normals, int* faces, void* workspace, size_t workspace_bytes,
                            int device, void* stream);

/* ==== 6. METRICS ============================================================================== */
/* ---- uniform surface sampling: open3d's TriangleMesh.sample_points_uniformly (rendering_evaluation.py:290-295) -----
 * K meshes, n points each, one record per mesh in a device table (the meshes may be slices of shared buffers):
 *   triangle t is chosen with probability area_t / sum(area): u from a 53-bit double, t = the first face with
 *   cdf[t] > u cdf[F - 1] (cdf: the inclusive fp64 scan of |(b - a) x (c - a)| over the record's unscaled fp32
 *   vertices, in an order fixed by F; zero-area faces are never chosen); point = (1 - sqrt r1) a + sqrt r1 (1 - r2) b
 *   + sqrt r1 r2 c; then p := R(quat) (factor p) + position.
 *   random words: Philox-4x32-10, key = {seed & 0xffffffff, seed >> 32}, counter = {sample index i, 0, 0, 0};
 *   words x, y -> u = ((x >> 5) 2^26 + (y >> 6)) 2^-53, z -> r1 = (z >> 8) 2^-24, w -> r2 = (w >> 8) 2^-24.
 *   The mesh's position in the table is not part of the stream: a batch equals its single calls bit for bit.
 * Outputs points [K][n][3] float; normals [K][n][3] float (nullable: the barycentric blend of the record's vertex
 * normals, rotated, normalised; NaN for a record without normals); triangles [K][n] int32 (nullable).
 * A record whose faces leave [0, total_faces) of the workspace, or whose every face has zero area, gives NaN points
 * and triangle -1.  Requirements: 1 <= num_faces <= max_faces for every record, the records' CDF ranges
 * [cdf_offset, cdf_offset + num_faces) disjoint inside [0, total_faces). */
typedef struct sdfr_sample_mesh {
  const float* vertices;   /* [num_vertices][3], unscaled */
  const int* faces;        /* [num_faces][3] vertex indices */
  const float* normals;    /* [num_vertices][3] or NULL */
  long long cdf_offset;    /* the mesh's first element of the workspace's fp64 CDF */
  int num_vertices, num_faces;
  float factor;            /* uniform scale (the Mesh's _factor) */
  float quat[4];           /* (x, y, z, w) */
  float position[3];
} sdfr_sample_mesh;        /* 72 bytes; read on the device through csrc/mesh_record.hpp alone, written by mesh.py's
                            * _MeshTable alone */
SDFR_API size_t sdfr_sample_workspace_bytes(int K, long long total_faces, int max_faces);   /* 0: invalid */
SDFR_API int sdfr_sample_points(const sdfr_sample_mesh* meshes, int K, long long total_faces, int max_faces, int n,
                                unsigned long long seed, float* points, float* normals, int* triangles,
                                void* workspace, size_t workspace_bytes, int device, void* stream);

/* ---- exact neighbours: scipy.spatial.KDTree(refs).query(queries, p=p) (metrics.py), brute force, O(N M) ------------
 * K pairs: query set k = queries[q_offsets[k] .. q_offsets[k+1]) against reference set k = refs[r_offsets[k] ..
 * r_offsets[k+1]) (device int64 offsets, [K + 1]; max_q / max_r: host bounds of every pair's sizes, they shape the
 * grid; offsets are clamped to [0, total], so wrong ones give wrong answers, never out-of-bounds accesses).
 *   p in [1, inf] (p = 1, 2, inf specialised); the fp32 value sum |q_i - r_i|^p (max |q_i - r_i| for p = inf), from
 *   coordinate differences, decides; ties go to the lowest reference index; the winner's distance is then recomputed
 *   in fp64.  farthest = 1: the farthest reference point instead (with refs = queries, max over the queries of it is
 *   the set's diameter).  Per query: dist [total_q] double, index [total_q] int32 (nullable; local to its reference
 *   set).  A query with no reference point (empty set, NaN) gets NaN and -1.  The result is the same bits whatever the
 *   batch or the run: per-workgroup winners merge through integer atomics on (float bits << 32 | index). */
SDFR_API size_t sdfr_nn_workspace_bytes(int K, long long total_q, int max_q);   /* 0: invalid */
SDFR_API int sdfr_nn_query(const float* queries, const long long* q_offsets, long long total_q, int max_q,
                           const float* refs, const long long* r_offsets, long long total_r, int max_r, int K,
                           float p, int farthest, double* dist, int* index, void* workspace, size_t workspace_bytes,
                           int device, void* stream);
/* per pair k over dist[offsets[k] .. offsets[k+1]), fp64 in a fixed tree order (the same bits for a pair whatever K):
 * stats [K][SDFR_NN_STATS] = {sum d, max d, count, NaN count, count(d < t_j) for j < SDFR_NN_MAX_THRESHOLDS,
 * count(d / extent[k] < t_j) for j < SDFR_NN_MAX_THRESHOLDS}; NaN distances are left out of the sum, max and counts;
 * t_j = h_thresholds[j] for j < num_thresholds (0 in the rest); extent [K] device, nullable (then 1). */
#define SDFR_NN_MAX_THRESHOLDS 4
#define SDFR_NN_STATS (4 + 2 * SDFR_NN_MAX_THRESHOLDS)
SDFR_API int sdfr_nn_reduce(const double* dist, const long long* offsets, long long total, int K,
                            const double* h_thresholds, int num_thresholds, const double* extent, double* stats,
                            int device, void* stream);

/* ==== 7. ENCODER ============================================================================== */
/* ---- SDFEncoder.forward (sdf_vae.py:103-169) and the noise of SDFVAE.encode / sample (:60-77) ------------------------
 * N cubic grids x [N][1][D][D][D] -> means [N][L], log_var [N][L] and (z nullable) z = means + exp(0.5 log_var) eps.
 * The layers are h_ops [n_ops][SDFR_ENC_OP_INTS] = {type, a, b, kernel, stride, padding, relu, 0} over (C, S, S, S)
 * (C = 1, S = D at first; Flatten is no op, torch's (C, D, H, W) order is the flattened one):
 *   SDFR_ENC_CONV     Conv3d: a = in_channels (= C), b = out_channels, cubic kernel, stride, zero padding, with bias;
 *                     S -> (S + 2 padding - kernel) / stride + 1
 *   SDFR_ENC_MAXPOOL  MaxPool3d: kernel, stride, padding 0, floor (a, b unused)
 *   SDFR_ENC_LINEAR   Linear: a = in_features (= C S^3, or the previous Linear's b), b = out_features; the
 *                     activation is flat from here on, no 3-d op may follow
 *   SDFR_ENC_RELU     ReLU (all other fields 0); relu = 1 in any other op applies a ReLU to its output
 * h_params: for every CONV / LINEAR op in order its weight (torch's layout: [b][a][k][k][k] / [b][a]) and bias [b];
 * then linear_means.weight [L][F], .bias [L], linear_log_var.weight [L][F], .bias [L] (F = the flat feature count).
 * Anything else, or a size or parameter count that does not add up, is SDFR_E_INVALID at creation, naming the op.
 * Results: fixed summation orders, no atomics -- a row's means / log_var are the same bits whatever N, its position
 * in the batch, or the run.  eps[i][j]: Philox-4x32-10, key = {seed & 0xffffffff, seed >> 32}, counter = {i, j, 0,
 * 0x56414531}; words x, y -> u1 = ((x >> 5) 2^26 + (y >> 6)) 2^-53, z, w -> u2 likewise; eps = sqrt(-2 ln(1 - u1))
 * cos(2 pi u2) in fp64, rounded to fp32; z = eps * float(exp(0.5 log_var)) + means, two fp32 roundings.  eps depends on
 * (seed, i, j) only. */
#define SDFR_ENC_CONV 1
#define SDFR_ENC_MAXPOOL 2
#define SDFR_ENC_LINEAR 3
#define SDFR_ENC_RELU 4
#define SDFR_ENC_OP_INTS 8
typedef struct sdfr_encoder sdfr_encoder;
SDFR_API int sdfr_encoder_create(const float* h_params, size_t n_params, int volume, int latent, int n_ops,
                                 const int* h_ops, int device, sdfr_encoder** out_handle);
SDFR_API void sdfr_encoder_destroy(sdfr_encoder* encoder);
SDFR_API size_t sdfr_encoder_workspace_bytes(const sdfr_encoder* encoder, int N);   /* 0: NULL encoder or N < 1 */
SDFR_API int sdfr_encoder_forward(const sdfr_encoder* encoder, const float* x, int N, float* means, float* log_var,
                                  float* z, unsigned long long seed, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* out [n][L] = eps of rows 0 .. n-1 (the stream above: SDFVAE.sample, zero means and unit std) */
SDFR_API int sdfr_normal_sample(float* out, int n, int L, unsigned long long seed, int device, void* stream);
/* x[i] = min(max(x[i], -t), t) in place, t >= 0 (SDFEncoder.prepare_input: the tsdf clamp) */
SDFR_API int sdfr_clamp(float* x, size_t count, float t, int device, void* stream);

/* ==== 8. MESH DEPTH =========================================================================== */
/* ---- depth images of triangle meshes: the reference's synthetic.draw_depth_geometry (an off-screen Open3D window) ----
 * K images [K][H][W] in one call, image k of record k of a sdfr_sample_mesh table (the records sdfr_sample_points
 * takes; normals and cdf_offset are not read; K poses of one mesh and K different meshes are the same call).  A posed
 * vertex is R(quat) (factor * v) + position; the camera sits at the origin of that frame, `flags` says which frame:
 *   SDFR_MESH_DEPTH_OPENGL  x right, y up, looking along -z (this library's renderer): the ray of pixel (row, col) is
 *                           ((col + 0.5 - cx) / fx, -(row + 0.5 - cy) / fy, -1), depth = -z
 *   SDFR_MESH_DEPTH_OPEN3D  x right, y down, looking along +z (the reference's draw_depth_geometry): the ray is
 *                           ((col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy, 1), depth = z
 * (no skew; cx, cy as Camera.get_pinhole_camera_parameters(0.5) returns them).
 * depth = the smallest z-depth (not ray length) over the triangles the pixel-centre ray meets with depth > near
 * (near >= 0), 0 where it meets none; both faces of a triangle count; no far plane.  Coverage is decided per pixel by
 * the ray (three scalar triple products, inclusive), never by projected vertices: a triangle that crosses the camera
 * plane is drawn where it is in front.  The term of an edge is computed from its two vertices in one order (lower
 * vertex index first) and negated for the triangle that walks it the other way, so two triangles that share an edge
 * (by vertex indices) leave no pixel centre between them.  A triangle with a vertex index outside [0, num_vertices),
 * a repeated index, a non-finite posed vertex, zero area or seen edge-on covers nothing and reads nothing out of
 * bounds; so does a record with num_faces outside [1, max_faces] or a NULL vertices / faces pointer (an image of
 * zeros).  triangle [K][H][W] int32 (nullable): the face that gave the depth, -1 for none; among faces of bitwise
 * equal depth the lowest index.
 * Bitwise reproducible: no float atomics; a triangle's depth in a pixel depends on its own three vertices, the
 * record's pose and the pixel alone -- the same bits on every run, under any permutation of the faces, and for
 * image k alone or among K.
 * Workspace: 16 bytes per image (the screen rectangle of the posed mesh; tiles outside it store zeros and leave).
 * The triangle set-up is recomputed by every 32 x 8-pixel tile inside that rectangle rather than stored per
 * (image, triangle).  total_faces / max_faces: the sum / a bound of the records' face counts (max_faces shapes the
 * grid).  No allocation, no host synchronisation; kernels only, so the call can be captured into a graph. */
#define SDFR_MESH_DEPTH_OPENGL 0
#define SDFR_MESH_DEPTH_OPEN3D 1
SDFR_API size_t sdfr_mesh_depth_workspace_bytes(int K, long long total_faces, int max_faces, int W,
                                                int H);   /* 0: invalid */
SDFR_API int sdfr_mesh_depth(const sdfr_sample_mesh* meshes, int K, long long total_faces, int max_faces, int W, int H,
                             float cx, float cy, float fx, float fy, float near, int flags, float* depth,
                             int* triangle, void* workspace, size_t workspace_bytes, int device, void* stream);

/* ==== 9. MESH TO SDF ========================================================================== */
/* ---- the distance volume of a triangle mesh: the reference's vae/sdf_utils.py::mesh_to_sdf (the external mesh_to_sdf
 * package: distances to a scanned point cloud, signs from depth buffers), computed exactly ------------------------------
 * K volumes sdf [K][R][R][R] in one call, volume k of record k of a sdfr_sample_mesh table (normals and cdf_offset are
 * not read).  A posed vertex is R(quat) (factor * v) + position, as in sdfr_sample_points and sdfr_mesh_depth; grid
 * point (i, j, k) = sdf[i][j][k] sits at ((2 i - (R - 1)) / (R - 1), ...) in that frame: index idx of an axis at
 * (idx - (R - 1) / 2) * 2 / (R - 1), the corners at -1 and 1, the frame and axis order of sdfr_mesh_emit and of the
 * renderer.  2 <= R <= 256.
 *   |sdf|   the Euclidean distance to the closest point of any valid triangle -- in the face, on an edge or at a
 *           vertex (the closest point by Voronoi region, not a plane distance).  fp32, no contraction; a pair's squared
 *           distance depends on the grid point and the face's three posed vertices, taken in ascending INDEX order,
 *           alone; the minimum over the faces is exact, ties go to the lowest face, the square root is taken once.
 *   sign    w = (1 / 4 pi) sum_t Omega_t,  Omega_t = 2 atan2(A . (B x C), |A||B||C| + (A . B)|C| + (B . C)|A| + (C . A)|B|)
 *           with A, B, C the face's vertices minus the point: every term in fp32, the sum in fp64 in ascending face
 *           order.  A point is inside (sdf < 0) iff w > 0.5.  Faces are oriented as Mesh documents: (b - a) x (c - a)
 *           points out of the object.
 *   flags   SDFR_MESH_SDF_SIGNED, or SDFR_MESH_SDF_UNSIGNED: no winding work, the output is |signed output| bit for bit
 *           (winding must then be NULL).
 *   triangle [K][R^3] int32 (nullable): the closest face, -1 for none.  winding [K][R^3] float (nullable): w, for
 *           diagnosing meshes that are not closed (then w is neither 0 nor 1 and the sign near 0.5 means little).
 * A triangle with a vertex index outside [0, num_vertices), a repeated index, a non-finite posed vertex or zero area
 * contributes neither distance nor winding and reads nothing out of bounds.  A record without a valid face, with a NULL
 * vertices / faces pointer, with num_faces outside [1, max_faces], or whose faces do not fit into total_faces gives a
 * volume of NaN (winding NaN, triangle -1), as the sampler does.
 * Bitwise reproducible: no float atomics; volume k is the same bits on every run, alone or among K, at any position in
 * the table.  The unsigned field and `triangle` do not depend on the order of the faces (up to the permutation); the
 * signed field's sign is not promised to be so, its sum being ordered.
 * Workspace: 16 bytes per record (rounded up to 64) + 64 bytes per face of total_faces: every face is posed once.
 * total_faces / max_faces: the sum / a bound of the records' face counts (max_faces shapes the set-up's grid).  No
 * allocation, no host synchronisation; kernels only, so the call can be captured into a graph.  Work: K R^3 max_faces
 * point-triangle pairs, brute force. */
#define SDFR_MESH_SDF_SIGNED 0
#define SDFR_MESH_SDF_UNSIGNED 1
SDFR_API size_t sdfr_mesh_sdf_workspace_bytes(int K, long long total_faces, int max_faces, int R);   /* 0: invalid */
SDFR_API int sdfr_mesh_sdf(const sdfr_sample_mesh* meshes, int K, long long total_faces, int max_faces, int R, int flags,
                           float* sdf, int* triangle, float* winding, void* workspace, size_t workspace_bytes,
                           int device, void* stream);

/* ==== 10. VAE TRAINING ======================================================================== */
/* ---- one iteration of the reference's trainer (sdfest/vae/scripts/train.py:195-287): forward with a tape, the loss
 * and its gradient, the gradient of every parameter, Adam ------------------------------------------------------------
 * A trainer handle describes the network only: the decoder as sdfr_decoder_create takes it, the encoder's op list as
 * sdfr_encoder_create takes it (the same checks, the same messages).  It holds no parameters and no device memory;
 * creation makes no HIP call.
 * PARAMETERS live in one flat fp32 device buffer of sdfr_vae_trainer_param_count floats that the caller owns, in
 * state_dict order and torch's layouts: sdfr_encoder_create's h_params followed by sdfr_decoder_create's h_params.
 * The gradient and Adam's two moments are buffers of the same length and layout.
 *   forward   x [N][D^3] (clamped IN PLACE to +-tsdf when post != 0 and tsdf > 0: prepare_input) -> means, log_var,
 *             z [N][L] (z = eps * exp(0.5 log_var) + means, eps the stream of group 7: counter {i, j, 0, 0x56414531}),
 *             recon [N][D^3] = decoder(z) without the tsdf clamp, and in `tape` every layer output the backward reads.
 *   loss      train.py:208-229, :271-281.  post != 0 and tsdf > 0: recon is clamped to +-tsdf where |x| >= tsdf and
 *             |recon| >= tsdf.  e1 = |recon - x|, e2 = e1^2, small = |x| < 0.1; terms [6] = {l2_small, l2_large,
 *             l1_small, l1_large, kld, total} (sums, not means; kld = -0.5 sum(1 + log_var - means^2 - exp(log_var));
 *             total = the four weighted terms + kld * (post ? w_kld : 0)).  g_recon [N][D^3] = d total / d recon (0
 *             where the clamp cuts); g_means, g_log_var [N][L] = the KLD's direct share of d total / d means, log_var.
 *   backward  the gradient of `total` w.r.t. every parameter into grads (every element is written): through the
 *             decoder (Linear, ReLU, trilinear resize, Conv3d) to z, through z = eps exp(0.5 log_var) + means into the
 *             heads, through the encoder (Linear, MaxPool3d with its argmax recomputed: the first maximum of a window,
 *             ReLU, Conv3d; no gradient w.r.t. x).  Takes the x, seed, log_var, z, tape and recon of the forward.
 * Every output element has one owner and a fixed summation order, no float atomics: the same inputs give the same
 * bits on every run.  The long sums (the loss terms over N D^3 voxels, a convolution's weight and bias gradient over
 * N S^3 positions) are two-stage: partial sums per workgroup in the workspace, then a combine in fixed order (in fp64).
 * No allocation, no host synchronisation; kernels only, on the caller's stream.  1 <= N <= 65535. */
typedef struct sdfr_vae_trainer sdfr_vae_trainer;
SDFR_API int sdfr_vae_trainer_create(int latent, int n_fc, const int* fc_out, int n_conv, const int* conv_in_size,
                                     const int* conv_cin, const int* conv_cout, const int* conv_k,
                                     const int* conv_relu, int volume, float tsdf, int n_ops, const int* h_ops,
                                     int device, sdfr_vae_trainer** out_handle);
SDFR_API void sdfr_vae_trainer_destroy(sdfr_vae_trainer* trainer);
/* floats of the flat parameter buffer, and of its encoder part (the decoder's parameters start there); 0: NULL */
SDFR_API size_t sdfr_vae_trainer_param_count(const sdfr_vae_trainer* trainer);
SDFR_API size_t sdfr_vae_trainer_encoder_param_count(const sdfr_vae_trainer* trainer);
SDFR_API size_t sdfr_vae_trainer_tape_bytes(const sdfr_vae_trainer* trainer, int N);        /* 0: NULL or N < 1 */
SDFR_API size_t sdfr_vae_trainer_workspace_bytes(const sdfr_vae_trainer* trainer, int N);   /* loss and backward */
SDFR_API int sdfr_vae_trainer_forward(const sdfr_vae_trainer* trainer, const float* params, float* x, int N,
                                      unsigned long long seed, int post, float* means, float* log_var, float* z,
                                      float* recon, float* tape, size_t tape_bytes, void* stream);
SDFR_API int sdfr_vae_trainer_loss(const sdfr_vae_trainer* trainer, const float* recon, const float* x,
                                   const float* means, const float* log_var, int N, float w_l2_small,
                                   float w_l2_large, float w_l1_small, float w_l1_large, float w_kld, int post,
                                   float* terms, float* g_recon, float* g_means, float* g_log_var, void* workspace,
                                   size_t workspace_bytes, void* stream);
SDFR_API int sdfr_vae_trainer_backward(const sdfr_vae_trainer* trainer, const float* params, const float* x, int N,
                                       unsigned long long seed, const float* log_var, const float* z,
                                       const float* tape, const float* recon, const float* g_recon,
                                       const float* g_means, const float* g_log_var, float* grads, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* ---- the point cloud term of the same iteration: pc_weight * loss_pc (train.py:230-269, :278) -------------------------
 * Per sample b the reference renders the TARGET volume x_b at a random orientation (position (0, 0, -5), scale 1,
 * threshold 0.01: sdfr_render_forward with sdf_view_stride = D^3 does that for all N at once), lifts the non-zero depth
 * pixels to points (depth_to_pointcloud, pointset_utils.py:57-77, OpenGL frame) and adds
 *     loss_pc += sum over the points of v^2,
 * v = train.py's own pc_loss (:30-125; losses.pc_loss without its final * scale) of the RECONSTRUCTION the other terms
 * see: the trilinear value at o = R(q / |q|)^T (P - position) / scale, 0 where the point's base cell
 * floor((o + 1) (D - 1) / 2) lies outside [0, D - 2]^3.
 * sdfr_vae_trainer_pc_term goes between sdfr_vae_trainer_loss and sdfr_vae_trainer_backward, in ONE pass over the
 * depth pixels (lift -> object frame -> cell -> the eight corners -> v; no point buffer, nothing per point in memory):
 *   depth [N][H][W]   any depth images (a pixel != 0 is a point); cx, cy, fx, fy as sdfr_render_forward takes them
 *                     (pixel-centre-0.5 intrinsics; the lift uses cx - 0.5, cy - 0.5 with integer pixel indices)
 *   pos [N][3], quat [N][4] (x, y, z, w; normalised here), scale [N]   device, the pose the points are sampled at
 *   recon, x [N][D^3], post   the forward's raw output and its (clamped) input: post != 0 and tsdf > 0 make a corner read
 *                     clamp(recon, +-tsdf) where |x| >= tsdf and |recon| >= tsdf, exactly as sdfr_vae_trainer_loss does,
 *                     and a corner the clamp cuts (recon < -tsdf or recon > tsdf) receives gradient 0
 *   loss_pc [1]       device: the UNWEIGHTED sum, overwritten
 *   terms             the terms [6] of sdfr_vae_trainer_loss: terms[5] (total) += pc_weight * loss_pc
 *   g_recon [N][D^3]  += 2 pc_weight v (trilinear weight) per corner: ADDED to what sdfr_vae_trainer_loss wrote.  A voxel
 *                     no point touches keeps its bits (an all-zero depth image leaves g_recon untouched, loss_pc = 0).
 * The scatter is deterministic the way SDFR_SDF_GRAD_DETERMINISTIC is: every contribution is rounded once to the
 * quantum 2^-SDFR_FIXED_QUANTUM_BITS (2^-40 = 9.1e-13) and added as a 64-bit INTEGER into a volume in the workspace
 * (integer addition is associative: the same bits on every run, whatever the order), which is converted once and added
 * to g_recon in fp64.  Representable range: |sum| < 2^(63 - 40) = 8.4e6 per voxel; a contribution that is not finite
 * saturates (NaN counts as 0).  loss_pc is a two-stage sum in fixed order: a float record per workgroup, then the
 * records in fp64 by one workgroup.  Pixels outside a conservative screen rectangle of the volume's bounding sphere
 * (radius sqrt(3) |scale| around pos) are not read: their points lie outside the volume.
 * Group 10's contract holds: no float atomics, no allocation, no host synchronisation, kernels only, on the caller's
 * stream; 1 <= N <= 65535, 1 <= W, H <= 65535.  The workspace is the term's own (sdfr_vae_trainer_workspace_bytes
 * keeps its values) and must be 8-byte aligned. */
SDFR_API size_t sdfr_vae_trainer_pc_term_workspace_bytes(const sdfr_vae_trainer* trainer, int N);   /* 0: NULL or N < 1 */
SDFR_API int sdfr_vae_trainer_pc_term(const sdfr_vae_trainer* trainer, const float* depth, int N, int W, int H, float cx,
                                      float cy, float fx, float fy, const float* pos, const float* quat,
                                      const float* scale, const float* recon, const float* x, int post, float pc_weight,
                                      float* loss_pc, float* terms, float* g_recon, void* workspace,
                                      size_t workspace_bytes, void* stream);
/* The term's orientations, uniform on SO(3) as train.py:242-251 draws them, quat [N][4] (x, y, z, w) on the device:
 *     q_i = (sqrt(1 - u1) sin 2 pi u2, sqrt(1 - u1) cos 2 pi u2, sqrt(u1) sin 2 pi u3, sqrt(u1) cos 2 pi u3)
 * from the Philox-4x32-10 stream of group 7 with key = seed and counter {i, 0, 0, 0x56415043} ("VAPC", apart from the
 * noise's 0x56414531): u_k = (word k - 1 of the output >> 8) * 2^-24, in [0, 1) with 24 bits each; the expression is
 * evaluated in fp64 and rounded to fp32 once.  A function of (seed, i) alone: a resumed run draws what the
 * uninterrupted one would.  N = 0: nothing to do. */
SDFR_API int sdfr_vae_trainer_pc_orientations(unsigned long long seed, int N, float* quat, int device, void* stream);
/* One torch.optim.Adam step (default betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) over a flat buffer of n
 * floats: exp_avg += (g - exp_avg) (1 - b1); exp_avg_sq = b2 exp_avg_sq + (1 - b2) g g; p += -(lr / (1 - b1^t)) exp_avg
 * / (sqrt(exp_avg_sq) / sqrt(1 - b2^t) + eps), the bias corrections in fp64 as torch forms them.  step[0] (device int)
 * is the number of steps taken so far and is incremented.  None of sdfr_adam_step's pose handling. */
SDFR_API int sdfr_adam_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int* step, size_t n,
                            double lr, int device, void* stream);

/* ==== 11. INITIALISATION NETWORK TRAINING ===================================================== */
/* ---- one iteration of the reference's trainer of the single-shot network (sdfest/initialization/scripts/train.py
 * :130-150, _compute_loss :211-287): VanillaPointNet + SDFPoseHead under train(), the loss, every parameter's gradient.
 * The update is sdfr_adam_flat above. -----------------------------------------------------------------------------------
 * A trainer handle describes the network only (group 4 runs the same network in inference mode): in_size, the backbone's
 * widths and its batchnorm / dense / residual flags, the head's widths and its batchnorm, the latent size, and n_cells
 * orientation classes (discretized) or 0 (quaternion).  The head's output row has L + 4 + n_cells or L + 8 floats:
 * latent [L], position [3], scale [1], logits [n_cells] or the quaternion BEFORE its normalisation [4].  The handle holds
 * no parameters and no device memory; creation makes no HIP call.  Not implemented (SDFR_E_INVALID): a residual link
 * that adds per-point inputs to a dense link's broadcast columns (in_size = 2 x the first width, dense and residual).
 * PARAMETERS: one flat fp32 device buffer of sdfr_pose_trainer_param_count floats that the caller owns, in the
 * reference's parameters() order and torch's layouts: _backbone._linear_layers.i.{weight, bias} for every i, then
 * _backbone._bn_layers.i.{weight, bias}, _head._linear_layers.i.{weight, bias}, _head._bn_layers.i.{weight, bias},
 * _head._final_layer.{weight, bias}.  The gradient has the same length and layout.
 * STATISTICS: a second flat buffer of sdfr_pose_trainer_stat_count floats, {running_mean [c], running_var [c]} per
 * BatchNorm in the same order (backbone, then head); may be NULL when update_stats == 0.
 *   forward   points [N][M][in_size] -> out [N][row], and in `tape` what the backward reads (every per-point layer's
 *             linear output and activation, the batch statistics, the set maxima and their rows).  BatchNorm
 *             normalises with the batch's mean and BIASED variance (eps 1e-5) over all N M rows (backbone) or N rows
 *             (head); update_stats != 0: running <- 0.9 running + 0.1 {mean, UNBIASED variance}.
 *   loss      terms [5] = {latent, position, scale, orientation, total}: mse (mean over all elements) of the three,
 *             cross_entropy (mean over N) of the logits against orientation_index [N], or mean(1 - (q / |q| . t)^2)
 *             against orientation_quat [N][4]; total = the weighted sum.  g_out [N][row] = d total / d out.
 *   backward  the gradient of `total` w.r.t. every parameter into grads (every element is written).  The gradient of a
 *             set maximum goes to the FIRST row that attains it.  Takes the points and tape of the forward.
 * Every output element has one owner and a fixed summation order, no atomics: the same inputs give the same bits on
 * every run.  Sums over the N M rows are two-stage: an fp64 record per (sample, column) or per block of rows, then
 * the records in order; the batch variance is a centred second pass.  No allocation, no host synchronisation; kernels
 * only, on the caller's stream.  1 <= N <= 65535, N M <= 2^30; N >= 2 with a head BatchNorm.  The workspace must be
 * 8-byte aligned and is shared by the three calls (the loss accepts one sized for any M). */
typedef struct sdfr_pose_trainer sdfr_pose_trainer;
SDFR_API int sdfr_pose_trainer_create(int in_size, int n_backbone, const int* backbone_out, int batchnorm, int dense,
                                      int residual, int n_head, const int* head_out, int head_batchnorm, int latent,
                                      int n_cells, int device, sdfr_pose_trainer** out_handle);
SDFR_API void sdfr_pose_trainer_destroy(sdfr_pose_trainer* trainer);
SDFR_API size_t sdfr_pose_trainer_param_count(const sdfr_pose_trainer* trainer);   /* 0: NULL */
SDFR_API size_t sdfr_pose_trainer_stat_count(const sdfr_pose_trainer* trainer);
SDFR_API int sdfr_pose_trainer_output_size(const sdfr_pose_trainer* trainer);      /* floats of an output row */
SDFR_API size_t sdfr_pose_trainer_tape_bytes(const sdfr_pose_trainer* trainer, int N, int M);        /* 0: invalid */
SDFR_API size_t sdfr_pose_trainer_workspace_bytes(const sdfr_pose_trainer* trainer, int N, int M);   /* 0: invalid */
SDFR_API int sdfr_pose_trainer_forward(const sdfr_pose_trainer* trainer, const float* params, float* stats,
                                       const float* points, int N, int M, int update_stats, float* out, float* tape,
                                       size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);
SDFR_API int sdfr_pose_trainer_loss(const sdfr_pose_trainer* trainer, const float* out, const float* latent,
                                    const float* position, const float* scale, const int* orientation_index,
                                    const float* orientation_quat, int N, float w_latent, float w_position,
                                    float w_scale, float w_orientation, float* terms, float* g_out, void* workspace,
                                    size_t workspace_bytes, void* stream);
SDFR_API int sdfr_pose_trainer_backward(const sdfr_pose_trainer* trainer, const float* params, const float* points, int N,
                                        int M, const float* tape, const float* g_out, float* grads, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* ==== 12. NOCS ANNOTATION ===================================================================== */
/* ---- pose and scale of the annotated objects of a NOCS frame (sdfest/initialization/datasets/nocs_dataset.py:673-712,
 * nocs_utils.py:14-241): the NOCS-map points of an object are aligned to its back-projected depth points by a RANSAC
 * over 100 five-point similarity fits and a final fit over the winner's inliers.  K objects per call, ragged through
 * DEVICE offsets [K + 1] (long long) as sdfr_nn_query's.  Kernels only, on the caller's stream; no allocation, no host
 * synchronisation; every result is written with ordinary vector stores.
 *
 * CORRESPONDENCES (:673-698), for the K mask ids of ONE frame.  depth [H][W] fp32 metres, mask [H][W] bytes (the
 * instance ids), nocs [H][W][channels] bytes (channels 3 or 4; the first three are used), mask_ids [K] DEVICE ints.
 * The valid pixels of object k are those with `(mask == mask_ids[k]) * depth != 0`, in ROW-MAJOR order (the order is
 * part of the result: the RANSAC's samples index it).  For each,
 *     source = (float(c) / 255 - 0.5,  float(c) / 255 - 0.5,  (1 - float(c) / 255) - 0.5)      (fp32, each step rounded)
 *     target = ((col - cx0) * z * rfx,  (row - cy0) * z * rfy,  z)                              (OpenCV frame)
 * with the pixel-centre-0 principal point and reciprocal focal lengths of sdfr_depth_to_points (the same expressions,
 * y and z not negated).  Two calls because the caller sizes the output: sdfr_nocs_count writes counts [K] (DEVICE
 * ints), max_depth [K] (the largest valid depth; 0 for an empty object) and its block counts into `workspace`; the
 * caller forms offsets [K + 1] and passes the SAME inputs and workspace to sdfr_nocs_correspondences, which writes
 * source / target rows offsets[k] ... of [capacity][3] floats.  A row outside [0, min(offsets[k + 1], capacity)) is
 * not written.  The reference's rejections (:692-698: fewer than 30 points, a depth above 32) are the caller's, from
 * counts and max_depth.  W H < 2^31 - 1024, 0 <= K <= 65535. */
SDFR_API size_t sdfr_nocs_workspace_bytes(int W, int H, int K);   /* 0: invalid */
SDFR_API int sdfr_nocs_count(const float* depth, const unsigned char* mask, int W, int H, const int* mask_ids, int K,
                             int* counts, float* max_depth, void* workspace, size_t workspace_bytes, int device,
                             void* stream);
SDFR_API int sdfr_nocs_correspondences(const float* depth, const unsigned char* mask, const unsigned char* nocs,
                                       int channels, int W, int H, float rfx, float rfy, float cx0, float cy0,
                                       const int* mask_ids, int K, const long long* offsets, long long capacity,
                                       const void* workspace, float* source, float* target, int device, void* stream);

/* THE FIT: nocs_utils.estimate_similarity_transform for K correspondence sets.  source / target [total][3] of `dtype`
 * (SDFR_NOCS_F32 or SDFR_NOCS_F64; NOCS data is fp32, the reference's own test passes fp64); object k owns rows
 * offsets[k] ... offsets[k + 1] - 1, at most max_n of them.  offsets must be NON-DECREASING: the objects' rows may
 * not overlap (overlapping objects share per-row scratch, and their results are undefined).  Offsets outside
 * [0, total] are clamped, so nothing is read out of bounds whatever they hold; an object that has more than max_n rows
 * after clamping is not fitted from a part of its rows, it answers SDFR_NOCS_TRUNCATED.  ALL arithmetic is fp64, as numpy's is from the moment the reference appends the homogeneous ones --
 * the two thresholds included (numpy takes an fp32 input's norms in fp32; the difference is ~1e-7 relative).
 *   sample_indices [K][SDFR_NOCS_HYPOTHESES][5] DEVICE ints: the five correspondences of every hypothesis, an INPUT
 *   (the reference draws them with np.random.choice; sdfr_nocs_sample_indices below draws them on the device).
 *   pass_t = 0.01 max(t / s, s / t) from the mean norms of target and source, stop_t = pass_t / 100.
 *   Hypothesis i = the Umeyama fit of its five pairs; residual_i = sqrt(sum_n |target_n - T_i source_n|^2).
 *   Selection = the reference's sequential loop (:111-131) replayed: j = the first iteration whose residual is below
 *   stop_t (99 without one), the winner = the first strict minimum of residual_0..j starting from 1e10; only
 *   iterations 0..j "ran": a zero source variance or a NaN covariance among THEM fails the object, later ones do not.
 *   Inliers = the winner's |d_n| < pass_t (every point when no residual beat 1e10).  inlier_ratio keeps the
 *   reference's quirk: np.count_nonzero(inlier_idx) counts inlier INDICES that are non-zero, so point 0 never counts
 *   (:167-169); it is 0 when no residual beat 1e10.  Final fit = Umeyama over the inliers.
 * Outputs, per object (DEVICE): position [3], rotation [3][3], scale, transform [4][4] (doubles, row-major; NaN unless
 * status is SDFR_NOCS_OK), inlier_ratio (double), best_iteration (the winner, -1 without one), iterations_run (j + 1),
 * status; inlier_mask [total] bytes (nullable).  A valid rotation is a ROTATION (orthogonal, determinant +1) whatever
 * the covariance's rank: for exactly planar or collinear sources, where a rotation and its mirror image fit equally
 * well and the reference returns either by rounding, it is the rotation.
 *   SDFR_NOCS_OK          the four results are valid
 *   SDFR_NOCS_NONE        the reference returns four None: fewer than 5 points, or inlier_ratio < 0.1
 *   SDFR_NOCS_POSE_ERROR  the reference raises PoseEstimationError: zero source variance in a fit that ran (:226-229)
 *   SDFR_NOCS_NAN_INPUT   the reference raises RuntimeError: a NaN covariance in a fit that ran (:211-215)
 *   SDFR_NOCS_TRUNCATED   the object has more than max_n rows: the caller's max_n is too small (iterations_run 0)
 * Every sum has a fixed order that depends on the object's own point count only: an object's results are the same bits
 * alone, in any batch and at any place in it.  1 <= K <= 65535, 0 <= max_n <= total.  The workspace is 128-byte
 * aligned. */
#define SDFR_NOCS_HYPOTHESES 100
#define SDFR_NOCS_F32 0
#define SDFR_NOCS_F64 1
#define SDFR_NOCS_OK 0
#define SDFR_NOCS_NONE 1
#define SDFR_NOCS_POSE_ERROR 2
#define SDFR_NOCS_NAN_INPUT 3
#define SDFR_NOCS_TRUNCATED 4
SDFR_API size_t sdfr_similarity_ransac_workspace_bytes(int K, long long total, int max_n);   /* 0: invalid */
SDFR_API int sdfr_similarity_ransac(const void* source, const void* target, int dtype, const long long* offsets,
                                    long long total, int max_n, int K, const int* sample_indices, double* position,
                                    double* rotation, double* scale, double* transform, double* inlier_ratio,
                                    int* best_iteration, int* iterations_run, int* status, unsigned char* inlier_mask,
                                    void* workspace, size_t workspace_bytes, int device, void* stream);

/* sample_indices [K][SDFR_NOCS_HYPOTHESES][5]: five DISTINCT indices in [0, N_k), N_k = offsets[k + 1] - offsets[k],
 * per hypothesis.  A stream of this library's own -- numpy's global Mersenne Twister stream, which the reference
 * draws from, is NOT reproduced: Philox-4x32-10, key = the object's seed (object_seeds[k], DEVICE, or `seed` for every
 * object when object_seeds is NULL), counter = {iteration, draw, attempt, 0x4E4F4353}; index = floor(word0 * N / 2^32);
 * a draw equal to an earlier one of its row is drawn again with attempt + 1 (after 64 attempts: the smallest index
 * not yet in the row).  An object's place in the batch is not part of the stream: the same seed and N give the same
 * rows.  N_k < 5: the rows are zeros (the fit answers SDFR_NOCS_NONE without reading them).  N_k is taken from the
 * offsets as they are, not clamped to a buffer or to the fit's max_n: the fit clamps every index it reads into the
 * object's rows, and an object it truncates answers SDFR_NOCS_TRUNCATED, so such rows never reach a result. */
SDFR_API int sdfr_nocs_sample_indices(const long long* offsets, int K, unsigned long long seed,
                                      const unsigned long long* object_seeds, int* sample_indices, int device,
                                      void* stream);

/* ==== 13. FRAME ANNOTATION ==================================================================== */
/* ---- the instance mask of an annotated RGB-D frame (sdfest/initialization/datasets/redwood_dataset.py:262-275,
 * AnnotatedRedwoodDataset._compute_mask): where the ground-truth mesh, drawn at its annotated pose (sdfr_mesh_depth),
 * covers a pixel and the sensor did not see something in front of it.  B images per call; rendered, observed
 * [B][H][W] fp32 metres (0 = nothing drawn / no reading).  Per pixel
 *     mask   = rendered != 0 && !(observed != 0 && observed < rendered - margin)
 * with the subtraction rounded to fp32 and IEEE comparisons: a pixel at exactly fl(rendered - margin) stays visible
 * (the comparison is strict), and so does an observed NaN or infinity, as in torch.  margin >= 0 and finite (the
 * reference's is 0.01).
 *   mask    [B][H][W] bytes, 0 or 1 (a torch.bool buffer)
 *   masked  [B][H][W] fp32, nullable: mask ? observed : 0
 *   counts  [B][4] int32, nullable: covered (rendered != 0), visible (mask), occluded (covered && !mask), valid
 *           (mask && observed != 0: the points of the frame's masked point cloud).  OVERWRITTEN by every call.
 * Image b starts at pixel b H W of every buffer; the float pointers need 4-byte alignment only (a view into a larger
 * buffer, H W no multiple of 4): an image whose rendered, observed and masked pixels are equally far from a 16-byte
 * boundary, with the mask 4-byte aligned at the same pixel, moves 16 bytes per lane and access, any other one pixel.
 * Same results either way, and the same bits on every run (the counts are integer atomics).  H, W >= 1,
 * H W <= 2^31 - 1, 0 <= B <= 65535 (B = 0: nothing to do).  Kernels only, on the caller's stream; no workspace, no
 * allocation, no host synchronisation: the call can be captured into a graph. */
SDFR_API int sdfr_visible_mask(const float* rendered, const float* observed, int B, int H, int W, float margin,
                               unsigned char* mask, float* masked, int* counts, int device, void* stream);

/* ==== 14. POSE INFORMATION ==================================================================== */
/* ---- how well a depth image determines the pose it was rendered at.  The reference's estimator returns a point
 * estimate only and names an unobservable rotation in its metrics alone (rotational_symmetry_axis); this is the
 * quantity behind a covariance of (position, rotation, scale): per view, the Gram matrix of the per-pixel feature
 * vector f = (d0 .. d7, r, 1),
 *     d   d depth / d (px, py, pz, qx, qy, qz, qw, inv_scale) of the pixel -- the vector sdfr_render_backward
 *         multiplies by its upstream gradient and sums away, in the same arithmetic
 *     r   depth - target (fp32)
 * over the INCLUDED pixels: depth > 0 && target > 0 (the overlap of estimation/simple_setup.py:125), and, for
 * inlier_threshold > 0, fabsf(target - depth) / target < inlier_threshold (_compute_inlier_ratio, :183-184) with an
 * IEEE fp32 subtraction and division -- numpy float32 gives the same set.  inlier_threshold = 0: the whole overlap.
 *   depth   [B][H][W] the rendered estimate at (pos, quat, inv_scale); its non-zero pixels are the hit pixels
 *   target  [B][H][W] the observation
 *   gram    [B][10][10] doubles, overwritten: [:8][:8] = J^T J, [:8][8] = J^T r, [8][8] = sum r^2, [9][9] = the number
 *           of included pixels (exact), [:8][9] = sum d, [8][9] = sum r; exactly symmetric; all zeros for a view
 *           without an included pixel
 * Pixels outside the projection of the bounding sphere of the grid's cube (centre pos, radius sqrt(3) / inv_scale) are
 * not read: no ray hits the grid there, and the forward leaves them 0.
 * Pose, intrinsics and sdf_view_stride as in sdfr_render_backward.  Two launches on the caller's stream -- the image
 * tiles of all views, then a fixed-order sum of each view's tile records in double --, no allocation, no host
 * synchronisation.  Every sum has one order: two calls on the same inputs give the same bits, a view's matrix does not
 * depend on the other views of the call, and the workspace may hold anything on entry.
 * B, W, H >= 1 (B <= 65535, W H <= 2^31 - 1), 2 <= R <= 1023, inlier_threshold >= 0 and finite, the workspace 128-byte
 * and gram 8-byte aligned.  Every argument error -- a NULL pointer and a workspace that is too small included -- is
 * SDFR_E_INVALID with a message, before anything touches the GPU; _workspace_bytes answers 0 for sizes the call
 * refuses. */
SDFR_API size_t sdfr_render_information_workspace_bytes(int B, int W, int H);
SDFR_API int sdfr_render_information(const float* depth, const float* target, const float* sdf, int R,
                                     long long sdf_view_stride, const float* pos, const float* quat,
                                     const float* inv_scale, int B, int W, int H, float cx, float cy, float fx,
                                     float fy, float inlier_threshold, double* gram, void* workspace,
                                     size_t workspace_bytes, int device, void* stream);

/* ---- the same jointly with the latent: per view the F x F Gram matrix, F = 10 + T, of f = (d0 .. d7, s0 .. s_{T-1}, r, 1)
 * over the same included pixels -- d, r, the inclusion rule and the tile cull are sdfr_render_information's, instruction
 * for instruction --, with
 *     s_t = d depth / d (latent direction t) = f * trilerp(jac[.][t]) at the pixel's hit cell with the pixel's offsets,
 *           f = scale |d.z|: the EXACT d depth / d SDF weights of sdfr_render_backward (SDFR_SDF_GRAD_EXACT) contracted
 *           with the tangent volumes.  SDFR_SDF_GRAD_CUDA_COMPAT is a compatibility weighting (the reference's corner
 *           permutation), not a derivative, and has no counterpart here.
 *   jac     [R^3][Tp] floats, voxel-major as sdfr_decoder_jvp (group 17) writes it: the T tangent values of a grid corner
 *           in one row of Tp floats (Tp a multiple of 4, Tp >= T; columns T .. Tp - 1 are not read into the result);
 *           16-byte aligned.  jac_view_stride = 0: the views share it; otherwise >= R^3 Tp floats (a multiple of 4) from
 *           view to view -- with several views per object, pass the views' own pointers through the stride of a
 *           repeated buffer, as sdf_view_stride
 *   gram    [B][F][F] doubles, overwritten: [:8][:8] the pose block (what sdfr_render_information gives, up to the
 *           rounding of a different summation block), [8:8+T][8:8+T] the latent block, [:8+T][8+T] = J^T r,
 *           [8+T][8+T] = sum r^2, [9+T][9+T] the exact count; exactly symmetric; all zeros for a view without an included
 *           pixel
 * 1 <= T <= SDFR_INFO_MAX_TANGENTS: F <= 32 is one 32 x 32 block of the matrix cores.  Everything else -- the two launches, the fixed-order
 * sums, "a view does not depend on its batch", "the workspace may hold anything on entry", the limits and the argument
 * errors (all SDFR_E_INVALID before anything touches the GPU; T = 23, a Tp that is no multiple of 4 or below T, a
 * misaligned jac) -- as sdfr_render_information. */
#define SDFR_INFO_MAX_TANGENTS 22 /* 10 + T <= 32; the T of groups 17, 18 and 19 has the same limit */
SDFR_API size_t sdfr_render_information_shape_workspace_bytes(int B, int W, int H, int T);
SDFR_API int sdfr_render_information_shape(const float* depth, const float* target, const float* sdf, int R,
                                           long long sdf_view_stride, const float* jac, int Tp, int T,
                                           long long jac_view_stride, const float* pos, const float* quat,
                                           const float* inv_scale, int B, int W, int H, float cx, float cy, float fx,
                                           float fy, float inlier_threshold, double* gram, void* workspace,
                                           size_t workspace_bytes, int device, void* stream);

/* ==== 15. BOXES =============================================================================== */
/* ---- the bounds of a grid's iso-surface: what amin / amax of sdfr_mesh_emit's vertices give, without counting,
 * scanning or emitting a mesh.  Grids, `complete`, `level`, the inside rule (v < level), the axis order and the vertex
 * position are group 5's; per grid
 *   bounds  [N][6] float, overwritten: lo x, y, z, hi x, y, z = per axis the minimum and maximum, over ALL crossed edges
 *           of the (padded) volume, of the vertex sdfr_mesh_emit places on that edge -- the same bits (one statement of
 *           the arithmetic, csrc/mesh_grid.hpp); lo = +inf, hi = -inf for a grid without a crossed edge
 *   crossed [N] int32, overwritten: the number of crossed edges (the V of sdfr_mesh_count's totals)
 * Minima, maxima (atomics on an order-preserving integer image of the float) and an integer count: the same bits on
 * every call, and for a grid alone or among N.  The outputs may hold anything on entry.  Three launches on the caller's
 * stream, no workspace, no allocation, no host synchronisation: the call can be captured into a graph.
 * 2 <= R <= 256, 0 <= N <= 65535 (N = 0 does nothing), level finite, all pointers 4-byte aligned; every argument error is
 * SDFR_E_INVALID with a message, before anything touches the GPU.  Only finite grids are specified. */
SDFR_API int sdfr_sdf_bounds(const float* sdf, int N, int R, int complete, float level,
                             float* bounds /* [N][6]: lo xyz then hi xyz */, int* crossed /* [N] */,
                             int device, void* stream);

/* ---- the 3D IoU of oriented boxes (the reference leaves it a TODO: estimation/metrics.py:66-70), in fp64.
 * A box is 10 doubles: centre (3), quaternion x, y, z, w (4; normalised inside), full side lengths (3); it is the set
 * c + R(q) x, |x_i| <= e_i / 2.
 *   boxes_a [N][10], boxes_b [M][10]
 *   mode    SDFR_BOX_IOU_MATRIX: iou [N][M], every a against every b;  SDFR_BOX_IOU_PAIRED: N == M, iou [N]
 *   iou     V / (V_a + V_b - V), V = the volume of the intersection; intersection (nullable, same shape): V
 *   symmetry_axis 0 | 1 | 2 with symmetry_steps = S >= 1 (<= 65536): box b is also turned about ITS OWN axis by
 *           2 pi s / S, s = 0 .. S - 1, and the largest V (hence the largest IoU) is returned -- a category whose turn
 *           about that axis cannot be observed (correct_thresh's rotational_symmetry_axis); -1: one evaluation
 *           (symmetry_steps is not read); S = 1 gives the bits of -1
 * V is the sum over the 12 face planes of (plane distance x area of the clipped rectangle) / 3, with L = |e_a| + |e_b| +
 * |c_b - c_a|: a signed distance of at most 1e-12 L counts as zero, so coplanar faces -- fp32-rounded multiples of 90
 * degrees included -- are counted once; boxes whose bounding spheres are apart give exactly 0; 0 <= V <= min(V_a, V_b).
 * Accuracy: within 1e-12 L^3 of the exact volume for boxes in general position, for coplanar faces and for parallel
 * ones (identical boxes give 1, boxes that only touch 0, to that bound).  NOT for two faces that cross at an angle d
 * below about 1e-5 rad without being coplanar to 1e-12 L: each is cut by the other's plane, the cut line is placed by
 * the rounding of distances of about 1e-17 L / d, and the two cuts need not agree -- measured 1e-9 of the volume at d =
 * 1e-7, 1e-7 at d = 1e-8, more as d falls towards 1e-12 L / side.
 * A box with a non-finite entry, a non-positive side length or a quaternion whose squared norm is 0 or not finite gives
 * NaN in every entry it takes part in.  An entry depends on its own two boxes alone: MATRIX [i][j] is bitwise the
 * PAIRED result of (a_i, b_j), in any batch.  N = 0 or M = 0 does nothing.  One launch on the caller's stream, no
 * workspace, no allocation, no host synchronisation.  All pointers 8-byte aligned; every argument error is
 * SDFR_E_INVALID with a message, before anything touches the GPU. */
#define SDFR_BOX_IOU_MATRIX 0   /* iou [N][M] */
#define SDFR_BOX_IOU_PAIRED 1   /* N == M, iou [N] */
SDFR_API int sdfr_box_iou(const double* boxes_a, int N, const double* boxes_b, int M, int mode,
                          int symmetry_axis, int symmetry_steps,
                          double* iou, double* intersection /* nullable */, int device, void* stream);

/* ==== 16. AVERAGE PRECISION =================================================================== */
/* Detection matching and average precision over IoU thresholds and over (degrees, distance) thresholds, per class: the
 * number category-level pose estimation reports.  The reference has no such code; THE PROTOCOL below is this project's
 * own statement of it, after the published NOCS evaluation -- parity with a third-party script is not claimed.
 *   Groups.    Detections and ground truths carry a frame id and an integer class id; a GROUP is one (frame, class) and
 *              only detections and ground truths of one group can match.
 *   Order.     Inside a group the detections are processed by descending score, ties by the lower input index.
 *   Pairs.     Every (detection i, ground truth j) of a group has four doubles: 0 iou, 1 degrees, 2 distance (metres),
 *              3 key, the preference among ground truths.
 *   Criterion. (iou_min, degrees_max, distance_max); a pair is ADMISSIBLE iff iou >= iou_min && degrees <= degrees_max
 *              && distance <= distance_max.  -inf / +inf switch a test off; a pair with a NaN entry (the key included) is
 *              never admissible.
 *   Matching.  Criteria are independent of each other.  For one criterion, in detection order, a detection takes the
 *              admissible, still unmatched ground truth with the smallest key (ties: the lower ground-truth index), or
 *              stays unmatched.  key = -iou with (t, +inf, +inf) is the usual IoU matching; key = degrees + 100 distance
 *              with (-inf, d, s) the usual degree / cm matching; (0.1, 10, 0.05) says "10 degrees, 5 cm among boxes that
 *              overlap" directly.
 *   AP.        For one (class, criterion): all detections of the class over all frames by descending score (ties: the
 *              lower input index), tp_k = detection k is matched, n_gt = the class's ground truths;
 *                  precision_k = cumtp_k / (k + 1),  p^_k = max_{j >= k} precision_j,  AP = (sum_{k: tp_k} p^_k) / n_gt
 *              -- the sum first, then one division: all matched gives exactly 1.0, none matched exactly 0.0.  n_gt == 0:
 *              NaN; ground truths but no detections: 0.  mAP is the mean over the classes whose AP is not NaN.
 * All three calls are fp64, enqueue kernels on the caller's stream, allocate nothing, never synchronise the host, and sum
 * in one fixed order: two calls on the same inputs give the same bits.  Every argument error is SDFR_E_INVALID or (a
 * required pointer) SDFR_E_NULL with a message, before anything touches the GPU; doubles and long longs need 8-byte, ints
 * 4-byte alignment.  A count of 0 (N; G, T or P; T or C) does nothing. */

/* ---- rotation and position error of N pose pairs.  A pose is 7 doubles: position (3), quaternion x, y, z, w
 * (normalised inside).
 *   distance [N]  |p_a - p_b|
 *   degrees  [N]  2 atan2(|v|, |w|) of the relative unit quaternion (v, w) = q_a conj(q_b), in degrees: q and -q give the
 *                 same value, equal poses exactly 0; with symmetry_axis[n] = a in {0, 1, 2} instead
 *                 atan2(|a1 x a2|, a1 . a2) of the images a1 = R(q_a) e_a, a2 = R(q_b) e_a of that object axis (a turn
 *                 about it cannot be observed: correct_thresh's rotational_symmetry_axis).  atan2, not acos, which loses
 *                 half the digits near 0 and 180 degrees.
 *   symmetry_axis [N] int, nullable (= none); any value but 0, 1, 2 means none
 * A non-finite entry or a quaternion whose squared norm is 0 or not finite gives NaN in both outputs. */
SDFR_API int sdfr_pose_pair_errors(const double* pose_a /* [N][7] */, const double* pose_b /* [N][7] */,
                                   const int* symmetry_axis /* [N] nullable */, int N, double* degrees,
                                   double* distance, int device, void* stream);

/* ---- greedy matching of G groups under T criteria.
 *   table       [n_pairs][4] the pair tables of all groups, one after the other
 *   pred_offset [G + 1] int: the detections of group g are the columns pred_offset[g] .. pred_offset[g + 1] of `matched`,
 *               ALREADY in processing order (descending score)
 *   gt_offset   [G + 1] int: group g has ng = gt_offset[g + 1] - gt_offset[g] ground truths (only the differences are used)
 *   pair_offset [G + 1] long long: pair (i, j) of group g is row pair_offset[g] + i * ng + j of the table
 *   criteria    [T][3]  iou_min, degrees_max, distance_max
 *   matched     [T][P] bytes, P = the number of detections: the LOCAL index 0 .. 63 of the ground truth a detection took
 *               under criterion t, or SDFR_AP_UNMATCHED.  Columns no group covers are not written.
 *   status      nullable int, OVERWRITTEN: bit 0 = some group was refused
 * At most SDFR_AP_MAX_GT ground truths per group (the matched set is one 64-bit mask).  A group with more, or whose three
 * offsets disagree (negative or decreasing, detections beyond P, pairs beyond n_pairs, a pair count that is not nd x ng),
 * gets SDFR_AP_UNMATCHED in all its rows -- where its columns lie inside [0, P) -- and sets the status bit; the other
 * groups are not affected, nothing outside [0, n_pairs) is read and nothing outside [0, T P) written.
 * One thread per (group, criterion), a workgroup being one group and SDFR_AP_CRITERIA_BLOCK consecutive criteria; a
 * group's result does not depend on the other groups or on T.  0 <= G <= 2^24, 0 <= T <= 2^20. */
#define SDFR_AP_MAX_GT 64
#define SDFR_AP_UNMATCHED 255
#define SDFR_AP_CRITERIA_BLOCK 256
SDFR_API int sdfr_ap_match(const double* table, long long n_pairs, const int* pred_offset, const int* gt_offset,
                           const long long* pair_offset, int G, int P, const double* criteria, int T,
                           unsigned char* matched, int* status /* nullable */, int device, void* stream);

/* ---- the AP integral of T criteria x C classes.
 *   matched      [T][P] as sdfr_ap_match wrote it
 *   order        [P] int: the detections (columns of `matched`) class by class, each class's slice by descending score
 *   class_offset [C + 1] int: class c's slice of `order`
 *   n_gt         [C] int: the class's ground truths over all frames
 *   ap           [T][C] doubles, overwritten, by the formula above; NaN for n_gt <= 0 or a class_offset outside [0, P]
 * An entry of `order` outside [0, P) is not read and counts as unmatched.  One wave per (criterion, class): it counts the
 * matches, then walks the slice from its end in chunks of 64 with the running maximum of the precision; a lane adds
 * its terms in walk order and one xor butterfly adds the lanes.  0 <= T <= 2^20, T C <= 2^31 - 1. */
SDFR_API int sdfr_ap_integrate(const unsigned char* matched, int T, int P, const int* order, const int* class_offset,
                               const int* n_gt, int C, double* ap, int device, void* stream);

/* ==== 17. DECODER JVP ========================================================================= */
/* ---- the forward-mode derivative of sdfr_decoder_forward w.r.t. the latent: d SDF / d z is volume^3 x latent, that is
 * `latent` tangent volumes, which no number of VJP calls below volume^3 yields.  The decoder is Linear, ReLU, trilinear
 * resize and Conv3d; its derivative along a direction is the same chain WITHOUT the biases and with every ReLU replaced
 * by the mask [activation > 0] of the primal run (a ReLU on the last layer included).  The N T directions of a call are
 * rows of a batch through that network, row (n, t) masked by latent n.
 *   z        [N][latent]: the latents of the forward (the small leading Linear layers are not on the tape; they are
 *            recomputed with the forward's own fmaf chains, as sdfr_decoder_backward_latent does)
 *   tape     what a preceding sdfr_decoder_forward(decoder, z, N, ..., tape, ...) wrote; the forward is not touched
 *   out      that forward's output [N][volume^3]; read only with enforce_tsdf on a decoder that truncates (NULL otherwise):
 *            the result is zero where out sits on the clamp, !(|out| < tsdf)
 *   tangents [N][T][latent]; NULL: the identity basis (T == latent), row t = d / d z_t
 *   jac      [N][volume^3][Tp] floats, overwritten, VOXEL-major: jac[n][voxel][t] is the derivative of latent n's voxel
 *            along tangents[n][t]; Tp = T rounded up to a multiple of 4, columns T .. Tp - 1 are written as zeros (the
 *            tangents of a grid corner are Tp / 4 16-byte loads for sdfr_render_information_shape).  16-byte aligned.
 *            The layout is written by the last step itself (the final resize, or the last convolution), no transpose.
 * fp32 fmaf chains in a fixed order (channels, then taps ascending), no atomics: the same bits on every call, and
 * row (n, .) does not depend on the other latents of the call.  The swapped 1x1x1 layer and the resizes are linear and
 * pass unchanged.  Kernels only on `stream`, no allocation, no host synchronisation.  1 <= T <= SDFR_INFO_MAX_TANGENTS (group 14),
 * N T <= 65535.  Errors before anything touches the GPU: SDFR_E_NULL (a pointer), SDFR_E_INVALID (N, T, a NULL
 * `tangents` with T != latent, a misaligned jac), SDFR_E_WORKSPACE; _workspace_bytes answers 0 for what the call refuses. */
SDFR_API size_t sdfr_decoder_jvp_workspace_bytes(const sdfr_decoder* decoder, int N, int T);
SDFR_API int sdfr_decoder_jvp(const sdfr_decoder* decoder, const float* z, const float* tape,
                              const float* out /* NULL unless enforce_tsdf */,
                              const float* tangents /* nullable: the identity basis */, int N, int T, int enforce_tsdf,
                              float* jac, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the standard deviation of every voxel of K decoded volumes under a covariance of their latents (or of any T
 * directions): out[k][voxel] = sqrt(max(0, j^T S_k j)), j = jac[k][voxel][:T].
 *   jac        [K][voxels][Tp] as above; covariance [K][T][T] doubles; out [K][voxels] floats, overwritten
 * One thread per voxel, the covariance in LDS, fp64 sums in a fixed order.  1 <= K <= 65535, 1 <= voxels <= 2^31,
 * 1 <= T <= SDFR_INFO_MAX_TANGENTS, Tp >= T a multiple of 4, jac 16-byte and covariance 8-byte aligned; every argument error is
 * SDFR_E_INVALID before anything touches the GPU. */
SDFR_API int sdfr_sdf_std(const float* jac, int K, long long voxels, int Tp, int T, const double* covariance,
                          float* out, int device, void* stream);

/* ==== 18. LM REFINEMENT ======================================================================= */
/* ---- one Levenberg-Marquardt step of K estimates from the Gram matrices of groups 14 / 17.  The loop of group 3 is
 * first order and returns the iterate it stopped at; the reference has nothing else (and no Gram matrix to build it
 * from).  This is the bookkeeping-and-solve half of a damped Gauss-Newton iteration: the caller decodes and renders the
 * TRIAL rows and hands in their Gram matrices, the call decides whether the trial replaces the CURRENT iterate, forms
 * the normal equations at the current iterate in the world tangent, solves them and writes the next trial rows;
 * sdfr_pose_to_views_objects (group 3) then gives that trial's camera-frame poses and packed latents for the next render.
 *   gram_trial   [K V][F][F] doubles, F = 10 + T, object-major (view k V + v): what sdfr_render_information (T = 0) or
 *                sdfr_render_information_shape (T >= 1) wrote for the rows of params_trial; read only
 *   params_trial [K][n_params] floats: position 3 | orientation 4 (x, y, z, w) | scale 1 | latent ...; read as the rows
 *                the Gram matrices were evaluated at, overwritten with the NEXT trial (entries 8 + T .. are the current
 *                row's: with T = 0 the latent is never touched)
 *   params_cur   [K][n_params], gram_cur [K V][F][F]: the current iterate and its Gram matrices; the call's own
 *   state        [K][SDFR_LM_STATE_DOUBLES] doubles, indexed by the macros below
 *   step         [K][7 + T] doubles or NULL: the solved tangent step delta behind the new trial (zeros for a row
 *                that solved nothing in this call)
 *   cam_quat     [V][4]: the cameras' orientations in the world, ONE list for every object (as sdfr_pose_to_views_objects)
 * Per object, with rss = sum_v gram[v][8 + T][8 + T], cnt = sum_v gram[v][9 + T][9 + T] (views ascending), z the row's
 * entries 8 .. 8 + T - 1 and mu = latent_weight:
 *   cost     Phi = rss / cnt + mu |z|^2: the MEAN squared residual (the included pixels change from iterate to iterate; a
 *            sum would reward losing overlap).  Not finite where a Gram entry of the trial is not, or cnt = 0.
 *   accept   init != 0: always, and lambda = lambda0, the counters 0.  Otherwise iff Phi_trial is finite, cnt_trial >=
 *            min_overlap cnt_cur and Phi_trial < Phi_cur.  Accepted: the trial row and its V matrices are copied into
 *            the current ones, lambda <- max(lambda lambda_down, lambda_min).  Rejected: lambda <- lambda lambda_up.
 *            These are IEEE double operations in this order without contraction: a float64 restatement decides alike.
 *   system   at the current iterate, per view M = diag(T8, I_T) with T8 the 8 x 7 map d (px, py, pz, qx, qy, qz, qw,
 *            inv_scale) / d (world position, world rotation vector, log-scale) -- identity; 1/2 (e_k, 0) (x) q_c; -inv_scale;
 *            position and rotation columns through R_c^T -- at the view's camera-frame quaternion q_c = conj(cam_quat[v])
 *            (x) q / |q| and inv_scale = 1 / scale, recomputed here in double from the current row:
 *              H = sum_v M^T G_v[:8+T][:8+T] M / cnt + mu I_latent,   g = sum_v M^T G_v[:8+T][8+T] / cnt + mu z
 *            (views ascending, then the division), the model Phi(delta) ~ Phi + 2 g^T delta + delta^T H delta.
 *   solve    A = H + lambda diag(max(H_ii, 1e-12 max_j H_jj)) -- the floor keeps a direction nothing observes (a
 *            symmetric body's spin, a latent column of zeros) from a zero pivot; its step is exactly 0 --, A delta = -g by
 *            Cholesky in double.
 *   retract  position += delta[0:3]; q <- exp(delta[3:6] / 2) (x) q / |q|, normalised; scale <- scale exp(delta[6]);
 *            z += delta[7:]; rounded to float.
 *   status   SDFR_LM_RUNNING; SDFR_LM_CONVERGED: the rounded trial equals the current row bit for bit (entries
 *            0 .. 8 + T - 1), or the step behind a trial that has just been accepted had a scaled norm
 *            sqrt(delta^T diag(A) delta) < step_tol; SDFR_LM_STALLED: lambda > lambda_max after a rejection;
 *            SDFR_LM_NO_SYSTEM: cnt = 0, an input (a Gram entry, an entry 0 .. 8 + T - 1 of the row) or the retracted
 *            row is not finite, or a pivot is not positive even with the floor.
 *            A row whose status is not SDFR_LM_RUNNING is FROZEN: its trial row is set to its current row, and later calls
 *            (init = 0) leave its current row, its current matrices and its state bit for bit as they are.  No NaN is
 *            ever written to a parameter row.
 * One launch on the caller's stream: workgroup k is object k and is one wave; all arithmetic is double, the matrices
 * (n = 7 + T <= 29: 6.7 KB) live in LDS; no workspace, no allocation, no host synchronisation.  Every sum has one order:
 * two calls on the same inputs give the same bits, and row k depends neither on K nor on the other rows.  On init the
 * current buffers and the state may hold anything.
 * 1 <= K <= 65535, 1 <= V <= SDFR_LM_MAX_VIEWS, 0 <= T <= SDFR_INFO_MAX_TANGENTS (group 14), 8 + T <= n_params <= 65535; the
 * double buffers 8-byte aligned;
 * every scalar finite and >= 0.  Errors before anything touches the GPU: SDFR_E_NULL (a pointer other than step),
 * SDFR_E_INVALID (everything else), with a message. */
#define SDFR_LM_MAX_VIEWS 64 /* views per object, here and in sdfr_information_combine (group 19) */
#define SDFR_LM_STATE_DOUBLES 16
#define SDFR_LM_LAMBDA 0        /* the damping the NEXT solve uses (the last one used, once frozen) */
#define SDFR_LM_COST 1          /* Phi of the current iterate */
#define SDFR_LM_COUNT 2         /* its pixel count, summed over the views */
#define SDFR_LM_STATUS 3        /* SDFR_LM_RUNNING ... */
#define SDFR_LM_ACCEPTED 4      /* trials accepted since init (init itself is not one) */
#define SDFR_LM_REJECTED 5
#define SDFR_LM_STEP_NORM 6     /* sqrt(delta^T diag(A) delta) of the last solve */
#define SDFR_LM_PREDICTED 7     /* -(2 g^T delta + delta^T H delta) of the last solve */
#define SDFR_LM_ACTUAL 8        /* Phi_cur - Phi_trial of the last trial judged (0 at init) */
#define SDFR_LM_COST_INIT 9     /* Phi and count at init */
#define SDFR_LM_COUNT_INIT 10
#define SDFR_LM_LAST_ACCEPT 11  /* 1: the last call accepted its trial (init included), 0: it rejected it */
#define SDFR_LM_COST_TRIAL 12   /* Phi and count of the last trial judged, accepted or not */
#define SDFR_LM_COUNT_TRIAL 13  /* (14, 15: reserved, written as 0) */
#define SDFR_LM_RUNNING 0
#define SDFR_LM_CONVERGED 1
#define SDFR_LM_STALLED 2
#define SDFR_LM_NO_SYSTEM 3
SDFR_API int sdfr_lm_step(const double* gram_trial, float* params_trial, float* params_cur, double* gram_cur,
                          double* state, double* step /* nullable */, const float* cam_quat, int K, int V, int T,
                          int n_params, int init, double latent_weight, double min_overlap, double lambda0,
                          double lambda_up, double lambda_down, double lambda_min, double lambda_max, double step_tol,
                          int device, void* stream);

/* ==== 19. POINT-CLOUD INFORMATION ============================================================= */
/* ---- the Gauss-Newton information of the point-cloud residual.  The loop of group 3 minimises the depth L1 PLUS the
 * point-cloud loss (simple_setup.py:133-144: the observed points must lie on the zero set of the posed SDF); the Gram
 * matrices of groups 14 / 17, and so sdfr_lm_step, see the depth residual alone, which is summed over a pixel set that
 * changes with the iterate.  This is the matrix of the other half, summed over the FIXED set of observed points, in the
 * same 8 + T coordinates and the same layout.  The reference has neither.
 *   points, offsets, max_view_points, pos, quat, scale, sdf, R, sdf_view_stride: exactly sdfr_pc_loss_forward's (group 1;
 *       `scale`, not inv_scale, as the sampler takes it; offsets may be NULL for a single view of max_view_points points)
 *   jac, Tp, T, jac_view_stride: exactly sdfr_render_information_shape's (group 14).  T = 0: pose only, jac may be NULL
 *       and Tp is ignored; otherwise 1 <= T <= SDFR_INFO_MAX_TANGENTS, Tp a multiple of 4 and >= T.  F = 10 + T.
 *   gram    [B][F][F] doubles, overwritten: per view the Gram matrix over ALL M_v points of the view of
 *       f = (e0 .. e7, s0 .. s_{T-1}, r, 1):
 *         r        the point's value as sdfr_pc_loss_forward writes it (0 outside the volume)
 *         e0..e2   d r / d p;   e3..e6  d r / d q of the RAW quaternion, through the normalisation: with a = d r / d q^,
 *                  (a - q^ (q^ . a)) / |q|;   e7  d r / d inv_scale = -scale^2 d r / d scale -- group 14's coordinate, so
 *                  that the tangent map of sdfr_lm_step applies unchanged
 *         s_t      scale * trilerp(jac[.][t]) at the point's cell with the point's offsets
 *       A point outside the volume has f = (0, .., 0, 0, 1): it is a member of the reference's mean with residual 0
 *       (losses.py:134, simple_setup.py:144) and gets no gradient.
 *       [:8+T][:8+T] = J^T J, [:8+T][8+T] = J^T r, [8+T][8+T] = sum r^2, [9+T][9+T] = M_v exactly; symmetric bit for bit;
 *       all zeros for a view without points.
 *   inside  [B] ints or NULL: the number of the view's points inside the volume (exact)
 *   workspace: sdfr_pc_information_workspace_bytes(B, max_view_points, T) bytes = B min(nblk, G) F F floats with
 *       nblk = ceil(max_view_points / 256) and G = 64 (pc_information.hip), 128-byte aligned; it may hold anything on entry.
 * Two launches on `stream` (three with `inside`: its zero fill): workgroup g of a view takes the view's 256-point blocks
 * g, g + G, ... -- 32 v_mfma_f32_32x32x2_f32 per 64 points into accumulators that stay live across them (the longest
 * fp32 chain is 64 ceil(nb_v / G) points) --, the four waves are summed as (0 + 1) + (2 + 3) into one float record, and
 * the second launch sums a view's min(nb_v, G) records in record order in double.  Every sum has one order: the same
 * inputs give the same bits, and a view's matrix depends neither on B, nor on the other views, nor on max_view_points.
 * The per-point derivative expressions are those of the sampler's backward (sdfr_pc_loss_backward) with upstream
 * gradient 1.  B <= 65535, max_view_points <= 2^30, 2 <= R <= 1024; gram 8-byte, jac (and its stride) 16-byte aligned.
 * Every error is SDFR_E_INVALID with a message, before anything touches the GPU: a NULL pointer other than `inside`
 * (or jac at T = 0), a short or misaligned workspace.  Not an error, returns 0: B = 0 (nothing is written), and
 * max_view_points = 0 (gram and inside are zeroed).  _workspace_bytes returns 0 for sizes the call refuses. */
SDFR_API size_t sdfr_pc_information_workspace_bytes(int B, int max_view_points, int T);
SDFR_API int sdfr_pc_information(const float* points, const int* offsets /* nullable */, int B, int max_view_points,
                                 const float* pos, const float* quat, const float* scale, const float* sdf, int R,
                                 long long sdf_view_stride, const float* jac /* nullable with T = 0 */, int Tp, int T,
                                 long long jac_view_stride, double* gram, int* inside /* nullable */, void* workspace,
                                 size_t workspace_bytes, int device, void* stream);

/* ---- depth and point-cloud Gram matrices of K objects with V views each, added for sdfr_lm_step (which stays as it is:
 * its cost is rss / cnt).  The combined objective is
 *     Phi = sum_v rss_d / sum_v cnt_d + pc_weight sum_v rss_p / sum_v M_v + mu |z|^2
 * -- the squared counterpart of what the loop minimises.  Per object k, views ascending, IEEE double without contraction,
 * in this order (F = 10 + T; Gd, Gp the [K V][F][F] inputs, object-major):
 *     cd = sum_v Gd[k V + v][F-1][F-1];  cp = sum_v Gp[k V + v][F-1][F-1]
 *     alpha = (cd > 0 && cp > 0) ? (pc_weight cd) / cp : 0
 *     out[i][j] = Gd[i][j] + alpha Gp[i][j]  for i, j < F - 1 (the product is rounded, then the sum);
 *     row and column F - 1 are copied from Gd
 * Then out[8+T][8+T] / cd is Phi's data part and H, g of sdfr_lm_step are those of Phi; the count stays the depth term's,
 * so min_overlap means what it meant.  gram_out may be gram_depth (in place).  Entries that are not finite propagate (the
 * step then reports SDFR_LM_NO_SYSTEM).  One launch, no workspace; object k depends neither on K nor on the other
 * objects.  1 <= K <= 65535, 1 <= V <= SDFR_LM_MAX_VIEWS, 0 <= T <= SDFR_INFO_MAX_TANGENTS, pc_weight finite and >= 0, the
 * matrices 8-byte aligned; every error is SDFR_E_INVALID with a message before anything touches the GPU. */
SDFR_API int sdfr_information_combine(const double* gram_depth, const double* gram_pc, int K, int V, int T,
                                      double pc_weight, double* gram_out, int device, void* stream);

/* ---- looking at a render: surface normals, the range of a depth image, packed RGB8 frames (shade.hip).  Nothing here
 * is differentiated and nothing takes a workspace.
 *
 * sdfr_render_normals: `depth` [B][H][W] is sdfr_render_forward's output for the same grid(s), poses and intrinsics;
 * sdf, R, sdf_view_stride (0: one grid for all B views, otherwise >= R^3: one per view), pos, quat, inv_scale as the
 * forward takes them.  normals [B][H][W][3], every element written: for a pixel with depth != 0 the gradient of the
 * trilinear interpolant at the pixel's hit point -- the cell, the clamped base and the un-clamped offsets of
 * sdfr_render_backward, cells that extrapolate past the grid included -- normalised and rotated into the camera frame
 * (it points away from the object: the SDF is positive outside); three zeros where depth == 0, where the gradient
 * vanishes and where it is not finite.  One launch, no atomics; a view's result does not depend on its batch.
 *
 * sdfr_depth_range: range [B][2] (shared == 0) or [1][2] (shared != 0: one workgroup reads all B images -- meant for a
 * few images; for many, reduce the [B][2] rows with a second call that takes them as one 2B x 1 image) = the minimum
 * and the maximum over the pixels that are finite and non-zero, (0, 0) where there are none.  Exact; one launch.
 *
 * sdfr_shade_frames: one pass over B frames ordered (state, view) with V = views_per_state; frame f reads grid f / V
 * when sdf_view_stride != 0, pose f and target image f % V.  Outputs [B][H][W][3] bytes R, G, B; a NULL output is
 * skipped (not all three).  A pixel with depth == 0 gets `background` (0xRRGGBB) in every image.  Otherwise
 *   depth_rgb   (needs range: device memory, {vmin, vmax} at range + f * range_stride, range_stride 0 or 2)
 *               viridis[clamp(floor((z - vmin) / (vmax - vmin) * 256), 0, 255)], entry 0 when vmax == vmin
 *   error_rgb   (needs target [V][H][W]) background where the target is 0, else
 *               viridis[clamp(floor(|z - target| / error_max * 256), 0, 255)]
 *   shaded_rgb  (needs sdf, pos, quat, inv_scale) with n the normal of sdfr_render_normals and l = light / |light| (camera
 *               frame, towards the light): s = ambient + (1 - ambient) max(0, n . l), channel c =
 *               round(255 clamp(base_c s, 0, 1))
 * The table is matplotlib's viridis at 256 entries (colormap_table.hpp).  A frame's bytes depend on that frame's inputs
 * alone, and the same inputs give the same bytes.
 *
 * All three: 1 <= B <= 65535, W, H >= 1, W H <= 2^30, 2 <= R <= 1024, float buffers 4-byte aligned.  Every error is
 * SDFR_E_INVALID with a message, before anything touches the GPU: a NULL required pointer, B, W or H <= 0, R < 2, V < 1 or
 * B not a multiple of V, error_max <= 0, range_stride not 0 or 2, a zero focal length or light, background beyond 0xffffff. */
SDFR_API int sdfr_render_normals(const float* depth, const float* sdf, int R, long long sdf_view_stride,
                                 const float* pos, const float* quat, const float* inv_scale, int B, int W, int H,
                                 float cx, float cy, float fx, float fy, float* normals, int device, void* stream);
SDFR_API int sdfr_depth_range(const float* depth, int B, int W, int H, int shared, float* range, int device,
                              void* stream);
SDFR_API int sdfr_shade_frames(const float* depth, const float* sdf, int R, long long sdf_view_stride,
                               const float* pos, const float* quat, const float* inv_scale, int B, int W, int H,
                               float cx, float cy, float fx, float fy, int views_per_state,
                               const float* target /* nullable */, const float* range /* nullable */, int range_stride,
                               float error_max, float light_x, float light_y, float light_z, float ambient,
                               float base_r, float base_g, float base_b, int background,
                               unsigned char* depth_rgb /* nullable */, unsigned char* error_rgb /* nullable */,
                               unsigned char* shaded_rgb /* nullable */, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFR_H_ */
