/*
 * sfm_hip.h — C ABI of the MI355X-native two-view SfM hot path
 * (libsfm_hip.so, built from deep-sfm-revisited_amd/csrc for gfx950).
 *
 * Drop-in boundary for jytime/Deep-SfM-Revisited:
 *   - the `essential_matrix` PyTorch extension (RANSAC_FiveP/essential_matrix/
 *     essential_matrix_wrapper.cpp:102-108) — initialise / computeP / optimise /
 *     decompose / decomposeUV;
 *   - the plane-sweep cost volume of models/PSNet.py:144-158 and the per-plane
 *     warp models/inverse_warp.py:121-153;
 *   - the dense correspondence build of models/SFMnet.py:176-263 (flow2coord
 *     298-318) feeding the RANSAC.
 *
 * Conventions
 *   - Every pointer marked [dev] is device memory on the current HIP device;
 *     [host] is host memory.  No torch types cross this boundary.
 *   - Device work is stream-ordered on `stream` (a hipStream_t, NULL = default
 *     stream).  Functions return before the work completes unless stated.
 *   - Return value: SFM_OK (0) or an SFM_ERR_* code; sfm_last_error() gives a
 *     message (thread-local).  Nothing calls exit() (the reference's
 *     CudaErrorCheck exit()s the process: essential_matrix.cu:17-24).
 *   - Scratch memory is caller-provided (`workspace`), sized by the matching
 *     *_workspace_bytes() query; no call allocates device memory, so every
 *     device entry point is hipGraph-capturable.
 */
#ifndef SFM_HIP_H
#define SFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SFM_OK = 0,
  SFM_ERR_ARG = 1,        /* invalid argument (shape, size, range)          */
  SFM_ERR_HIP = 2,        /* HIP runtime / launch error                     */
  SFM_ERR_WORKSPACE = 3   /* workspace missing or too small                 */
};

#define SFM_ABI_VERSION 1
#define SFM_RANSAC_CHAINS 512   /* reference: 8 blocks x 64 threads (essential_matrix.cu:201-203) */
#define SFM_MAX_BATCH 64        /* pairs per device launch (larger batches are chunked) */

int sfm_abi_version(void);
const char* sfm_last_error(void);

/* ------------------------------------------------------------------------
 * RANSAC five-point essential matrix
 * ------------------------------------------------------------------------
 * Hypotheses: H = SFM_RANSAC_CHAINS * iters; hypothesis h = t*iters + i is
 * iteration i of chain t (reference thread t).  Sampling: Philox4x32-10 keyed
 * by `seed`, counter {h, draw/4, 0, 0}, curand_uniform-style (0,1] floats
 * turned into indices by the reference's RandomInt arithmetic, clamped to n-1.
 * Selection: per hypothesis the best candidate on the first num_test points
 * (first strict max, default candidate 0), rescored on the first
 * num_ransac_test points; the winner is the first hypothesis (in h order)
 * with the maximal rescored count — exactly the reference's per-thread
 * strict-> update followed by the host max_element (kernel_functions.cu:
 * 141-226, essential_matrix.cu:248-265).  If no hypothesis has an inlier,
 * E = P = 0, inliers = 0, winner = -1 (the reference returns uninitialised
 * memory there).
 */

/* Workspace for up to `batch` pairs of at most n_max points and `iters`
 * RANSAC iterations per chain. */
size_t sfm_ransac5_workspace_bytes(int batch, int64_t n_max, int iters);

/* Single pair, reference layout.  Replaces ProjectionMatrixRansac
 * (essential_matrix.cu:190-280, cheirality=1) and EssentialMatrixInitialise
 * (essential_matrix.cu:110-184, cheirality=0).
 *   q, qp          [dev] n x 2 float64, row-major (x, y) — input1 / input2
 *   E_out          [dev] 3x3 float64; P_out [dev] 3x4 float64 (may be NULL
 *                  when cheirality == 0); inliers_out [dev] int32[1];
 *   winner_out     [dev] int32[1] or NULL.
 * Requires 1 <= num_test, num_ransac_test <= n (the reference reads out of
 * bounds otherwise), iters >= 1, thr > 0. */
int sfm_ransac5(const double* q, const double* qp, int64_t n,
                int num_test, int num_ransac_test, int iters, double thr,
                uint64_t seed, int cheirality,
                void* workspace, size_t workspace_bytes,
                double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out,
                void* stream);

/* Batched pairs on packed correspondences.
 *   pts            [dev] batch x n_stride x 4 float64: (x, y, x', y') per point
 *   n              [host] batch int64: points of each pair (<= n_stride)
 *   num_test, num_ransac_test: per-call; values <= 0 mean "all n[b] points"
 *   E_out [dev] batch x 9, P_out [dev] batch x 12 (or NULL), inliers_out
 *   [dev] batch int32, winner_out [dev] batch int32 or NULL,
 *   hyp_score_out  [dev] batch x H int32 rescored count per hypothesis, or NULL.
 */
int sfm_ransac5_packed(const double* pts, int64_t n_stride, const int64_t* n, int batch,
                       int num_test, int num_ransac_test, int iters, double thr,
                       uint64_t seed, int cheirality,
                       void* workspace, size_t workspace_bytes,
                       double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out,
                       int32_t* hyp_score_out, void* stream);

/* Fused dense path: RANSAC straight from the flow
 * field, no correspondence buffer.  Point k of each pair is pixel
 * (u, v) = (m + k % (w_side-2m), m + k / (w_side-2m)) of the crop, with the
 * values of sfm_flow_to_points (bit-identical results to
 * sfm_flow_to_points + sfm_ransac5_packed).
 *   flow [dev] batch x 2 x H x W float32; Kinv [dev] batch x 3 x 3 float32;
 *   other arguments and outputs as sfm_ransac5_packed. */
int sfm_ransac5_flow(const float* flow, int batch, int H, int W, int h_side, int w_side, int margin,
                     const float* Kinv, int num_test, int num_ransac_test, int iters, double thr,
                     uint64_t seed, int cheirality, void* workspace, size_t workspace_bytes,
                     double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out,
                     int32_t* hyp_score_out, void* stream);

/* Inlier counts of given essential matrices over packed correspondences:
 * counts[b][c] = #{k < n[b] : e(E[b][c], point k) <= thr} with e the
 * reference's ComputeError<double> Sampson-style error
 * (kernel_functions.cu:232-264), through the same scorer the RANSAC uses
 * (split-f16 matrix-core decisions exact by bound + float64 re-test; the
 * float32 / float64 VALU scorers outside its threshold range), bit-exact.
 * The reference's scoring loop over a candidate set (kernel_functions.cu:
 * 187-214) without the sampling.
 *   pts [dev] batch x n_stride x 4 float64; n [host] batch;
 *   E [dev] batch x ncand x 9 float64; counts [dev] batch x ncand int32;
 *   workspace [dev] sfm_score_essentials_workspace_bytes(batch, ncand). */
size_t sfm_score_essentials_workspace_bytes(int batch, int ncand);
int sfm_score_essentials(const double* pts, int64_t n_stride, const int64_t* n, int batch, const double* E,
                         int ncand, double thr, int32_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Exact inlier mask of E (reference ComputeError + `<= thr`) for each point.
 *   pts [dev] batch x n_stride x 4; n [host] batch; E [dev] batch x 9;
 *   mask [dev] batch x n_stride uint8 (entries >= n[b] are written 0). */
int sfm_ransac5_inlier_mask(const double* pts, int64_t n_stride, const int64_t* n, int batch,
                            const double* E, double thr, uint8_t* mask, void* stream);

/* Dense flow -> packed normalised correspondences (models/SFMnet.py:179-263,
 * flow2coord 298-318): crop flow to h_side x w_side, drop a `margin` border,
 * q = (K^-1 (u, v, 1))[:2], qp = (K^-1 (u+fu, v+fv, 1))[:2] in float32 rows
 * (k0*x + k1*y) + k2, widened to float64.  Point k = (v-m)*(w_side-2m)+(u-m).
 *   flow [dev] batch x 2 x H x W float32; Kinv [dev] batch x 3 x 3 float32;
 *   pts_out [dev] batch x N x 4 float64, N = (h_side-2m)(w_side-2m). */
int sfm_flow_to_points(const float* flow, int batch, int H, int W, int h_side, int w_side,
                       int margin, const float* Kinv, double* pts_out, void* stream);

/* Sparse correspondences of SFMnet.pose_by_ransac (models/SFMnet.py:218-258),
 * for keypoints from any matcher (the reference uses cv2 SIFT/SURF + FLANN):
 *   mode 0: flow at np.round(kp1) (round half to even; caller validates the
 *           range — the reference's indexing raises), cfg default;
 *   mode 1: cfg.SAMPLE_SP — grid_sample (align_corners=True, zeros) of the
 *           coordinate grids at kp1;
 *   mode 2: cfg.SIFT_POSE — the matched keypoints kp1 / kp2 themselves;
 * then K^-1 (float32, 3 rows) and f64 widening.
 *   flow [dev] batch x 2 x H x W float32 (unused for mode 2), cropped to
 *   h_side x w_side; kp1, kp2 [dev] batch x kp_stride x 2 float32 pixel (x, y);
 *   n [host] batch int64 keypoints per pair; Kinv [dev] batch x 3 x 3 float32;
 *   pts_out [dev] batch x n_stride x 4 float64 (rows >= n[b] untouched). */
int sfm_keypoints_to_points(const float* flow, int batch, int H, int W, int h_side, int w_side,
                            const float* kp1, const float* kp2, int64_t kp_stride, const int64_t* n, int mode,
                            const float* Kinv, double* pts_out, int64_t n_stride, void* stream);

/* Scored candidate E's per pair of the last sfm_ransac5_packed call made with
 * this workspace (the last <= SFM_MAX_BATCH chunk), copied to the host
 * (synchronous).  Work accounting: the score kernel evaluates
 * counts[b] x max(num_test, num_ransac_test) correspondences for pair b. */
int sfm_ransac5_candidate_counts(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                 int32_t* counts_host);

/* Per hypothesis of the last sfm_ransac5_packed / _flow call made with this
 * workspace (laid out for `batch` pairs; the last <= SFM_MAX_BATCH chunk): the
 * five-point solver's real-root count (<= 0: no valid root) and the candidates
 * it kept (roots that pass cheirality; every valid root, at most 10, when
 * cheirality == 0), copied to the host (synchronous).
 *   nroots_host, ncand_host [host] batch x H int32, H = SFM_RANSAC_CHAINS * iters. */
int sfm_ransac5_hypothesis_counts(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                  int32_t* nroots_host, int32_t* ncand_host);

/* Evaluations the last RANSAC call with this workspace skipped by exact
 * bound pruning (tuning key score_prune; on when num_test == num_ransac_test
 * and hyp_score_out is NULL), copied to the host (synchronous).  The score
 * kernel performed sum(counts) x max(num_test, num_ransac_test) minus this
 * many evaluations.  Pruning never changes E, P, the inlier count or the
 * winner (ransac_common.h, PruneState). */
int sfm_ransac5_skipped_evaluations(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                    unsigned long long* skipped_host);
/* Diagnostics of the last pruned k_score_mf2 call on the workspace
 * (sfm_last_scorer() "k_score_mf2+prune"): per pair, the candidates the
 * count bound kept (scored to their exact counts); every other candidate was
 * dropped after the pruning point; points_host (optional): per pair, the
 * pruning point in points (a multiple of the 1024-point span: clamp at the
 * pair's N).  Undefined after an unpruned call.  Synchronises. */
int sfm_ransac5_kept_candidates(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                int32_t* kept_host, int32_t* points_host);

/* Pack reference-layout q, qp (n x 2 each) into pts (n x 4). */
int sfm_pack_points(const double* q, const double* qp, int64_t n, double* pts_out, void* stream);

/* ------------------------------------------------------------------------
 * Host-side E utilities (the reference runs these on CPU tensors too)
 * ------------------------------------------------------------------------ */
/* EssentialMatrixOptimise -> polish_E_robust_parametric (essential_matrix.cu:
 * 76-105, polish_E.cu:1470-1577).  All pointers [host]; q, qp n x 2. */
int sfm_essential_optimise(const double* q, const double* qp, int64_t n, const double* E_init,
                           double delta, double alpha, int max_reps, double* E_out);
/* Batched GPU form of the same IRLS.  The sums are
 * reassociated (parallel reduction), so E agrees with the host version to
 * rounding level, not bit for bit.
 *   pts [dev] batch x n_stride x 4 float64 (x, y, x', y'); n [host] batch;
 *   E_init, E_out [dev] batch x 9 float64. */
size_t sfm_essential_optimise_workspace_bytes(int batch, int64_t n_max);
int sfm_essential_optimise_batched(const double* pts, int64_t n_stride, const int64_t* n, int batch,
                                   const double* E_init, double delta, double alpha, int max_reps,
                                   double* E_out, void* workspace, size_t workspace_bytes, void* stream);
/* EssentialMatrixDecompose -> Edecomp(E, params) (essential_matrix.cu:29-43). */
int sfm_essential_decompose(const double* E, double* params5);
/* EssentialMatrixDecomposeUV -> Edecomp(E, U, V) (essential_matrix.cu:48-70). */
int sfm_essential_decompose_uv(const double* E, double* U, double* V);

/* ------------------------------------------------------------------------
 * Plane sweep
 * ------------------------------------------------------------------------ */
/* Scratch for the plane sweep: the target features re-laid out as channel
 * quads [B][ceil(C/4)][h*w][4] float32. */
size_t sfm_plane_sweep_workspace_bytes(int batch, int channels, int h, int w);

/* Cost volume of models/PSNet.py:144-157 for one target view:
 *   cost[b, c,   i] = ref[b, c]                     (c < C)
 *   cost[b, C+c, i] = inverse_warp(tgt, d_i)[b, c]
 * with d_i = (min_depth * nlabel) / (i + 1) in float32.
 *   ref, tgt [dev] batch x C x h x w float32
 *   pose     [dev] batch x 3 x 4 float32 (already RESCALE_DEPTH-scaled)
 *   K4, K4inv [dev] batch x 3 x 3 float32 (feature-resolution intrinsics)
 *   out_dtype 0: float32, 1: bfloat16 (round-to-nearest-even)
 *   cost     [dev] batch x 2C x nlabel x h x w */
int sfm_plane_sweep(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                    const float* pose, const float* K4, const float* K4inv,
                    int nlabel, float min_depth, int out_dtype, void* cost,
                    void* workspace, size_t workspace_bytes, void* stream);

/* General form.  ref == NULL: warped half only, out batch x C x nlabel x h x w.
 *   depth_mode 0: d_i = (min_depth * nlabel) / (i + 1)   (disp2depth, default)
 *   depth_mode 1: d_i = (i + 1) * min_depth               (cfg.PREDICT_BY_DEPTH,
 *                                                          PSNet.py:150-151) */
int sfm_plane_sweep_ex(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                       const float* pose, const float* K4, const float* K4inv,
                       int nlabel, float min_depth, int depth_mode, int out_dtype, void* cost,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same cost volume (models/PSNet.py:144-157) written channels-last, in the
 * layout and activation type its consumer, the regularisation stack
 * (PSNet.py:159; sfm_conv3_*), reads: what sfm_plane_sweep_ex into a float32
 * volume followed by sfm_to_channels_last_{f32,bf16,f16} produce, bit for
 * bit, without the planar [batch, 2C, nlabel, h, w] volume in between.
 *   out[b, i, y, x, c]     = ref[b, c, y, x]                     (c < C)
 *   out[b, i, y, x, C + c] = inverse_warp(tgt, d_i)[b, c, y, x]
 * Arguments as sfm_plane_sweep_ex (ref is required; predict_by_depth is its
 * depth_mode), and
 *   out_dtype 0: float32, 1: bfloat16, 2: float16 (both round to nearest even,
 *             the conversion of sfm_to_channels_last_*)
 *   out       [dev] batch x nlabel x h x w x 2C, 16-byte aligned
 *   workspace sfm_plane_sweep_workspace_bytes(batch, channels, h, w).
 * nlabel * h * w < 2^31.  channels a multiple of 4 (float32) or 8 (16-bit)
 * with every pair's tensors below 4 GiB take the wide-store kernel, any other
 * shape an element-wise one: the same values.  The switch "sweep_fused_cl"
 * (sfm_tune_set; 0, 1; default 1; not enumerated by sfm_tune_key) is not read
 * here: it tells a caller that owns both routes (sfm_amd.regularize) which one
 * to take. */
int sfm_plane_sweep_cl(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                       const float* pose, const float* K4, const float* K4inv,
                       int nlabel, float min_depth, int predict_by_depth,
                       int out_dtype /* 0 fp32, 1 bf16, 2 f16 */,
                       void* out, void* workspace, size_t workspace_bytes, void* stream);

/* sfm_plane_sweep_cl for float16 features, read as they come (the feature CNN's
 * output under cfg.MIXED_PREC autocast, models/SFMnet.py:80, 119): no float32
 * copy of either map, and the target is re-laid out as 16-byte channel octets,
 * so a tap gather brings eight channels where a float32 quad brings four.
 *   ref, tgt [dev] batch x C x h x w IEEE half, 2-byte aligned
 * Every other argument, every check and error code as sfm_plane_sweep_cl.
 * Contract: the result equals sfm_plane_sweep_cl on the same features widened
 * to float32, bit for bit, for every finite or infinite feature value (half to
 * float32 is exact, subnormals included; the tap sum and the rounding are the
 * same float32 operations).  channels a multiple of 8, for every out_dtype,
 * with every pair's tensors below 4 GiB take the wide-store kernel, any other
 * shape an element-wise one: the same values.
 *   workspace sfm_plane_sweep_workspace_bytes(batch, channels, h, w): the
 *             octets, [B][ceil(C/8)][h*w] x 16 bytes, fit the quads' region
 *             ([B][ceil(C/4)][h*w] x 16 bytes), so there is no query of its own.
 * Stream-ordered, no allocation.  The switch "sweep_f16_feat" (sfm_tune_set;
 * 0, 1; default 1; not enumerated by sfm_tune_key) is not read here: like
 * "sweep_fused_cl" it tells the Python depth stage (sfm_amd.psnet,
 * sfm_amd.regularize), which holds float16 features under MIXED_PREC, whether
 * to pass them here or to widen them for sfm_plane_sweep_cl. */
int sfm_plane_sweep_cl_f16(const void* ref, const void* tgt, int batch, int channels, int h, int w,
                           const float* pose, const float* K4, const float* K4inv,
                           int nlabel, float min_depth, int predict_by_depth,
                           int out_dtype /* 0 fp32, 1 bf16, 2 f16 */,
                           void* out, void* workspace, size_t workspace_bytes, void* stream);

/* The sweep section of PSNet.forward from the pose stage's outputs, in one
 * call (models/PSNet.py:130-157): the reference's tensor preparation runs in a
 * one-thread-per-pair kernel instead of ~10 ATen launches, bit for bit:
 *   pose      [dev] batch x 3 x 4, pose_dtype 0: float32, 1: float64 (P.float())
 *   K, Kinv   [dev] batch x 3 x 3 float32, full resolution; K4 = K with rows
 *             0-1 / 4, K4inv = Kinv with [:2,:2] * 4 (PSNet.py:130-133)
 *   t_scale   > 0: translation column * t_scale in float32 (cfg.RESCALE_DEPTH);
 *             <= 0: unscaled
 * then as sfm_plane_sweep_ex (ref == NULL: warped half only). */
int sfm_plane_sweep_psnet(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                          const void* pose, int pose_dtype, const float* K, const float* Kinv, float t_scale,
                          int nlabel, float min_depth, int depth_mode, int out_dtype, void* cost,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The two halves of sfm_plane_sweep_psnet's volume separately, so that the
 * pose-independent reference half (cost[:, :C, i] = ref, PSNet.py:155) can be
 * written on a second stream while RANSAC runs (round 4; the scorer is
 * compute-bound and leaves HBM idle):
 *   sfm_plane_sweep_ref_planes         rows 0..C-1 of every pair's
 *       [2C, nlabel, h, w] volume: a copy of ref per plane (bf16: RNE), in one
 *       wave per SIMD with 8 VGPRs, which fits beside the scorer's waves.
 *       workspace: sfm_plane_sweep_ref_planes_workspace_bytes (a padded copy
 *       of ref); shapes off its fast path use a generic kernel.
 *   sfm_plane_sweep_psnet_warped_half  sfm_plane_sweep_psnet without those rows
 *       (windows off the sweep's fast path still write them from ref: the
 *       same values).
 * Together they write exactly sfm_plane_sweep_psnet's volume. */
size_t sfm_plane_sweep_ref_planes_workspace_bytes(int batch, int channels, int h, int w);
/* Score fence: while enabled, every RANSAC call records a library-owned
 * event on its stream right before its scoring phase; sfm_score_fence_wait
 * makes `stream` wait for the last one recorded on that stream's device (so
 * the reference half can run beside the compute-bound scorer rather than the
 * latency-bound solve).  One event per device, created on the device of the
 * stream (not the caller's current device).  enable(1) / enable(0) are
 * reference-counted: recording stays on until every enable(1) has been
 * matched by an enable(0) (TwoViewHotPath enables it for its lifetime).
 * Every RANSAC call on a device records the same fence, so two hot paths
 * sharing a device wait on whichever scoring phase was enqueued last. */
int sfm_score_fence_enable(int on);
int sfm_score_fence_wait(void* stream);

/* Score gate (round 5; scoped to a waiting stream in round 6).  arm = 1:
 * record a library-owned event on `stream` and arm it for `waiter`: the next
 * RANSAC call (sfm_ransac5 / _packed / _flow) issued on the stream `waiter`
 * (on stream's device) makes `waiter` wait for the event right before its
 * scoring phase, and disarms the gate (one-shot).  RANSAC calls on any other
 * stream neither wait for nor consume it, so a second hot path or a plain
 * computeP on the same device is unaffected.  Re-arming for the same waiter
 * replaces the previous gate; arm = 0 disarms the waiter's gate.  At most 32
 * gates are armed at once (SFM_ERR_ARG beyond).  A pipelined caller arms it on
 * the side stream right after the previous step's sweep, for its own main
 * stream, so that sweep overlaps this step's correspondence build and
 * five-point solve but not the scorer
 * (sfm_amd.pipeline.TwoViewHotPath.step_pipelined).  No reference
 * counterpart: the reference's steps are serial (essential_matrix.cu:190-280
 * then PSNet.py:130-158). */
int sfm_score_gate(void* stream, void* waiter, int arm);

/* Reference-half job.  Arms a one-shot job for the next RANSAC call
 * (sfm_ransac5 / _packed / _flow) issued on `stream`: that call also writes
 * the pose-independent reference half of the cost volume `cost` [batch,
 * 2 * channels, nlabel, h, w] (cost_dtype 0 float32, 1 bfloat16), cost[b, c, l]
 * = ref[b, c] for every plane l (PSNet.py:155), from `ref` [batch, channels,
 * h, w] float32 -- the same bytes sfm_plane_sweep_ref_planes writes -- on the
 * same stream, so that the sweep after it can be the warped half alone
 * (sfm_plane_sweep_psnet_warped_half).  When the call's scorer is the pruned
 * matrix-core scorer (dense pairs of >= 32 spans of 1024 points, num_test ==
 * num_ransac_test, no per-hypothesis scores, "score_mf_prune_upper" = 1) and
 * h * w is even (with nlabel even when h * w % 4 == 2), ref 8-byte and cost
 * 16-byte aligned, the scorer's first launch issues the stores from its own
 * waves while it leaves HBM idle (the store rider, csrc/score_mf2.h); in
 * every other case, and with the switch "score_ref_rider" (sfm_tune_set; 0,
 * 1; default 1; not enumerated by sfm_tune_key) at 0, the call runs
 * sfm_plane_sweep_ref_planes' kernels on the stream instead.  Either way the
 * half is complete, in stream order, when the call's own outputs are.
 * The job is scoped to (device, stream): RANSAC calls on other streams
 * neither see nor consume it.  It is consumed by the next call on the stream
 * whatever path that call takes; arming again for the stream replaces it;
 * ref == NULL and cost == NULL disarms.  A slot holds no HIP object and no
 * call waits on it; of more than 32 armed streams the oldest job is dropped,
 * so jobs that are never consumed cannot exhaust the slots.  ref and cost
 * must stay valid until the consuming call's work on the stream is done.
 * sfm_score_ref_jobs_armed returns the number of armed jobs. */
int sfm_score_ref_job(void* stream, const float* ref, void* cost, int batch, int channels, int nlabel, int h, int w,
                      int cost_dtype);
int sfm_score_ref_jobs_armed(void);
int sfm_plane_sweep_ref_planes(const float* ref, int batch, int channels, int h, int w, int nlabel, int out_dtype,
                               void* cost, void* workspace, size_t workspace_bytes, void* stream);
int sfm_plane_sweep_psnet_warped_half(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                                      const void* pose, int pose_dtype, const float* K, const float* Kinv,
                                      float t_scale, int nlabel, float min_depth, int depth_mode, int out_dtype,
                                      void* cost, void* workspace, size_t workspace_bytes, void* stream);

/* Warped half only (cost[b, c, i] = inverse_warp(tgt, d_i)), batch x C x nlabel x h x w. */
int sfm_plane_sweep_warped(const float* tgt, int batch, int channels, int h, int w,
                           const float* pose, const float* K4, const float* K4inv,
                           int nlabel, float min_depth, int out_dtype, void* out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the cost volume of models/PSNet.py:144-157 into the features:
 * what autograd computes in the reference's training loop through
 * cost[:, :C, i] = ref (PSNet.py:155) and through F.grid_sample inside
 * inverse_warp (models/inverse_warp.py:151) into the target features.
 *   grad_ref[b, c, p] = sum_i grad_cost[b, c, i, p]
 *   grad_tgt[b, c, t] = sum_i sum_p sum_k [tap_k(b, i, p) == t] weight_k(b, i, p) grad_cost[b, C + c, i, p]
 * with the taps and weights of the forward (the same float32 bits), so the
 * result is the exact transpose of sfm_plane_sweep_ex's warped half.  No
 * gradient is formed for pose, K4, K4inv or the plane depths.
 *   grad_cost  [dev] batch x 2C x nlabel x h x w float32 (planar), or
 *              batch x C x nlabel x h x w with warped_only = 1
 *   grad_ref   [dev] batch x C x h x w float32, or NULL (not wanted); must be
 *              NULL with warped_only
 *   grad_tgt   [dev] batch x C x h x w float32; zeroed inside the call
 *   pose, K4, K4inv, nlabel, min_depth as sfm_plane_sweep_ex; predict_by_depth
 *              is its depth_mode
 *   workspace  sfm_plane_sweep_backward_workspace_bytes(batch, channels, h, w, nlabel)
 * Every buffer 4-byte aligned.  nlabel * h < 2^31, w < 2^23.
 * grad_tgt is accumulated with float atomics and may differ in its last bits
 * between two calls on the same inputs (as torch's grid_sample backward on the
 * GPU); grad_ref is reproducible bit for bit. */
size_t sfm_plane_sweep_backward_workspace_bytes(int batch, int channels, int h, int w, int nlabel);
int sfm_plane_sweep_backward(const float* grad_cost, int warped_only, int batch, int channels, int h, int w,
                             const float* pose, const float* K4, const float* K4inv, int nlabel, float min_depth,
                             int predict_by_depth, float* grad_ref /* may be null */, float* grad_tgt,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Depth stage after the sweep
 * ------------------------------------------------------------------------ */
/* Scratch for sfm_plane_sweep_correlation: channel quads of ref and tgt. */
size_t sfm_correlation_workspace_bytes(int batch, int channels, int h, int w);

/* Correlation cost of REG2D.py:103-109 without the warped volume:
 *   cost[b, i] = mean_c(ref[b, c] * inverse_warp(tgt, d_i)[b, c])
 *   ref, tgt [dev] batch x C x h x w float32; pose/K4/K4inv as sfm_plane_sweep;
 *   depth_mode as sfm_plane_sweep_ex; cost [dev] batch x nlabel x h x w float32. */
int sfm_plane_sweep_correlation(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                                const float* pose, const float* K4, const float* K4inv, int nlabel,
                                float min_depth, int depth_mode, float* cost,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Soft-argmin depth head of PSNet.py:191-213 (submodule.py:57-93):
 * F.interpolate(cost, [L, H, W], 'trilinear', align_corners=False) -> softmax
 * over planes -> depth_mode 0: depth = min_depth*L / (sum p_i (i+1) + 1e-16)
 *                depth_mode 1: depth = min_depth * sum p_i (i+1) depth_step
 *                              (cfg.PREDICT_BY_DEPTH; depth_step = int(MIN_DEPTH))
 *   cost [dev] batch x nlabel x h x w float32; depth [dev] batch x H x W float32. */
int sfm_depth_head(const float* cost, int batch, int nlabel, int h, int w, int H, int W, int depth_mode,
                   float min_depth, float depth_step, float* depth, void* stream);

/* Backward of sfm_depth_head into the cost: the gradient autograd forms in the
 * reference's training loop through F.interpolate(trilinear), F.softmax and
 * disparityregression / depthregression (models/PSNet.py:194-216,
 * models/submodule.py:57-93), whose outputs its loss reads (main.py:387-389).
 * With v_l the forward's interpolated logit at an output pixel, p = softmax(v),
 * val_l = (l + 1) step, reg = sum_l p_l val_l and d = grad_depth * dout/dreg
 * (min_depth in depth mode, -(min_depth L) / (reg + 1e-16)^2 in disparity mode):
 *   grad_cost[b, l, y, x] = sum over the output pixels whose taps include (y, x)
 *                           of d p_l (val_l - reg) wy wx
 * with the forward's own taps, weights and exponentials (the same bits): the
 * exact transpose of sfm_depth_head.
 *   cost, batch ... depth_step   exactly what the forward call was given
 *              (min_depth is its multiplier argument)
 *   grad_depth [dev] batch x H x W float32
 *   grad_cost  [dev] batch x nlabel x h x w float32, every element written;
 *              must not alias cost
 *   workspace  [dev] sfm_depth_head_backward_workspace_bytes(batch, H, W) bytes
 *              (24 per output pixel), 8-byte aligned; SFM_ERR_WORKSPACE with the
 *              needed size in the message when it is missing or too small
 * sfm_depth_head's shape limits, and nlabel <= 8 * 65535.  A gather without
 * atomics: one thread owns an element and sums its contributors in a fixed
 * order, so the result is reproducible bit for bit from call to call; a cell no
 * output pixel reads (downsampling) gets exactly 0. */
size_t sfm_depth_head_backward_workspace_bytes(int batch, int H, int W);
int sfm_depth_head_backward(const float* cost, const float* grad_depth, int batch, int nlabel, int h, int w, int H,
                            int W, int depth_mode, float min_depth, float depth_step, float* grad_cost,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The transpose of the head's interpolation along one axis (host only, no
 * device work): the output indices of F.interpolate(align_corners=False) from
 * in_size to out_size (PSNet.py:194-197) whose taps include `cell`.
 * [*first0, *first0 + *count0) read it as tap 0, [*first1, *first1 + *count1)
 * as tap 1; both are contiguous runs because the source index is monotone in
 * the output index.  Tap 1 is the cell after tap 0, or the same cell at the
 * last index, or the output's own cell when the sizes match.  An empty run
 * has count 0.  This is the function sfm_depth_head_backward's gather walks. */
int sfm_depth_head_contributors(int in_size, int out_size, int cell, int* first0, int* count0, int* first1,
                                int* count1);

/* K^-1 of a batch of 3x3 matrices, as models/SFMnet.py:104 forms it
 * (intrinsic_inv_gpu = torch.inverse(intrinsic_gpu)): bit for bit what
 * torch.linalg.inv_ex returns on ROCm (rocsolver getrf + getrs order), in one
 * launch.  K, Kinv [dev] batch x 3 x 3 float32 row-major.  Singular K gives
 * inf / NaN entries (torch raises). */
int sfm_kinv3x3(const float* K, int batch, float* Kinv, void* stream);

/* models/inverse_warp.py:121-153 for an arbitrary depth map:
 *   feat [dev] B x C x h x w; depth [dev] B x h x w; pose [dev] B x 3 x 4;
 *   K, Kinv [dev] B x 3 x 3; out [dev] B x C x h x w (float32). */
int sfm_inverse_warp(const float* feat, int batch, int channels, int h, int w,
                     const float* depth, const float* pose, const float* K, const float* Kinv,
                     float* out, void* stream);

/* Backward of sfm_inverse_warp into feat: the gradient autograd forms through
 * F.grid_sample at models/inverse_warp.py:151 (the reference's per-plane callers:
 * PSNet.py:155, PANet.py:129, REGNet.py:177, REG2D.py:108,139), as the exact
 * transpose of the forward's taps and weights.  No gradient for depth, pose, K.
 *   grad_out [dev] B x C x h x w float32; depth, pose, K, Kinv as sfm_inverse_warp;
 *   grad_feat [dev] B x C x h x w float32, zeroed inside the call.
 * Float atomics: last bits may differ from call to call (sfm_plane_sweep_backward). */
int sfm_inverse_warp_backward(const float* grad_out, int batch, int channels, int h, int w, const float* depth,
                              const float* pose, const float* K, const float* Kinv, float* grad_feat, void* stream);

/* Flow2Depth, models/flow2depth.py:7-41 (dead code in the reference):
 *   KR = K.R [dev] B x 3 x 3, KT = K.T [dev] B x 3, Kinv [dev] B x 3 x 3
 *   (float32, numpy's inverse of K as the reference takes it);
 *   out [dev] B x H x W float32 = channel 2 of the [B, H*W, 3] result viewed
 *   as [B, 3, H, W], exactly as the reference returns it. */
int sfm_flow2depth(const float* KR, const float* KT, const float* Kinv, int batch, int H, int W, float* out,
                   void* stream);

/* ------------------------------------------------------------------------
 * Validation depth metrics (main.py:565-593 and evaluate_metric,
 * main.py:727-747 with demon_metrics.py:63 l1_inverse, :130 scale_invariant)
 * ------------------------------------------------------------------------ */
/* Scratch for sfm_depth_metrics: selection state, radix histograms and the
 * per-chunk partial sums (0 for an invalid shape). */
size_t sfm_depth_metrics_workspace_bytes(int batch, int H, int W);

/* One row of sums per pair, replacing the per-pair loop of main.py:565-593
 * (mask, median scale, clamp) and evaluate_metric's numpy reductions
 * (main.py:727-747), stream-ordered and without a host synchronisation:
 *   pred [dev] float32, pair b's pixel (y, x) at pred[b * pred_batch_stride +
 *     y * pred_row_stride + x]: the top-left H x W crop of the padded
 *     prediction is read in place (main.py:495-499, 543);
 *   gt [dev] batch x H x W float32;
 *   rescale [dev] batch float32 or NULL: p0 = pred * rescale[b] (main.py:536-541);
 *   mask_mode 0 (KITTI, main.py:568-574): gt > 0 && gt < 80 inside
 *     [y0, y1) x [x0, x1), the Eigen crop the host computes;
 *   mask_mode 1 (DeMoN, main.py:566): 0.5 <= gt <= 10; the rectangle is ignored;
 *   scale = median(gt[mask]) / median(p0[mask]) with torch's lower median,
 *     over the whole image when the mask is empty (main.py:580-582);
 *   p = p0 * scale, p <= min_depth -> min_depth, p > max_depth -> max_depth
 *     (main.py:588-590; max_depth = MIN_DEPTH * nlabel);
 *   rows [dev] batch x 16 float64: 0 n, 1 med_gt, 2 med_p, 3 scale, then over
 *     the masked pixels with d = gt - p: 4 sum |d|/gt, 5 sum d*d/gt, 6 sum d*d,
 *     7 sum l*l, 8 sum l (l = log gt - log p, float64), 9-11 the counts of
 *     max(gt/p, p/gt) < 1.25, 1.25^2, 1.25^3, 12 sum |1/gt - 1/p|, 13-15 zero.
 *     Terms are formed in float32 as numpy forms them and summed in float64 in
 *     a fixed order: a pair's row does not depend on the batch around it;
 *   depth_out [dev] batch x H x W float32 (p at every pixel) or NULL. */
int sfm_depth_metrics(const float* pred, int64_t pred_batch_stride, int pred_row_stride,
                      const float* gt, int batch, int H, int W, const float* rescale,
                      int mask_mode, int y0, int y1, int x0, int x1,
                      float min_depth, float max_depth,
                      double* rows, float* depth_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* 3-D cost regularisation layer of PSNet (models/PSNet.py:79-102, applied at
 * PSNet.py:159-165; convbn_3d = Conv3d(3, stride 1, pad 1, no bias) +
 * BatchNorm3d, models/submodule.py:17-20), on the matrix cores in bf16 with
 * fp32 accumulation:
 *   out = [relu](conv3x3x3(in) * scale[co] + bias[co]) [+ residual]
 *   in [dev] batch x depth x h x w x cin bf16 (channels-last), cin 32 or 64;
 *   weights [dev] 27 x 32 x cin bf16, tap = (kd*3 + kh)*3 + kw, cout
 *     zero-padded to 32 when cout == 1;
 *   scale, bias [dev] 32 float32 (BatchNorm folded; 1 / 0 for a plain conv);
 *   residual [dev] like out or NULL (cout 32 only), added after the ReLU;
 *   out [dev] batch x depth x h x w x 32 bf16 (cout 32), or
 *       batch x depth x h x w float32 (cout 1: the classify output). */
int sfm_conv3_bf16(const void* in, int batch, int cin, int depth, int h, int w, const void* weights,
                   const float* scale, const float* bias, const void* residual, int relu, int cout, void* out,
                   void* stream);

/* [batch][channels][plane] float32 (in_dtype 0) or bfloat16 (1) ->
 * [batch][plane][channels] bfloat16 (channels a multiple of 8): the
 * sweep's cost volume [B, 2C, L, h, w] into sfm_conv3_bf16's layout. */
int sfm_to_channels_last_bf16(const void* in, int in_dtype, int batch, int channels, int64_t plane, void* out,
                              void* stream);

/* The same layer with float16 activations and weights (11-bit mantissa,
 * fp32 accumulation on v_mfma_f32_32x32x16_f16): the precision the
 * reference's Conv3d layers run at under cfg.MIXED_PREC autocast
 * (models/SFMnet.py:164, cfgs/kitti.yml:10).  Arguments and layouts as
 * sfm_conv3_bf16, every 16-bit operand IEEE half. */
int sfm_conv3_f16(const void* in, int batch, int cin, int depth, int h, int w, const void* weights,
                  const float* scale, const float* bias, const void* residual, int relu, int cout, void* out,
                  void* stream);

/* [batch][channels][plane] float32 (in_dtype 0) or bfloat16 (1) ->
 * [batch][plane][channels] float16 (round to nearest even), sfm_conv3_f16's
 * layout. */
int sfm_to_channels_last_f16(const void* in, int in_dtype, int batch, int channels, int64_t plane, void* out,
                             void* stream);

/* Training the same layers in float16 (the reference trains under float16
 * autocast, cfgs/kitti.yml:10 MIXED_PREC): the weight gradient of one raw
 * Conv3d of the stack (models/PSNet.py:79-102, applied at PSNet.py:159-165),
 * on v_mfma_f32_32x32x16_f16 with fp32 accumulation:
 *   grad_weights[tap][co][ci] = sum over b, p of grad_out[b, p, co] in[b, p + tap - 1, ci]
 * (p + tap - 1 per axis, zero outside the volume; tap = (kd*3 + kh)*3 + kw).
 *   in           [dev] batch x depth x h x w x cin float16, cin 32 or 64: the
 *                layer's input, as sfm_conv3_f16 read it;
 *   grad_out     [dev] batch x depth x h x w x 32 float16: the gradient of the raw
 *                convolution's output.  cout must be 32: a cout 1 layer
 *                (classify's last) passes its gradient as channel 0 of a
 *                zero-padded 32-channel tensor and reads row co = 0;
 *   grad_weights [dev] 27 x 32 x cin float32, sfm_conv3_f16's pack layout;
 *   workspace    [dev] sfm_conv3_wgrad_f16_workspace_bytes(batch, cin, depth, h, w)
 *                bytes, 16-byte aligned: one 27 x 32 x 32 float32 partial sum per
 *                accumulating block and 32-channel half of cin.
 * Every pointer 16-byte aligned; grad_weights and workspace overlap neither
 * each other nor an input.  A fixed grid of accumulating blocks walks the
 * volume and a second launch adds their partial sums in block order: no float
 * atomics, so the result is reproducible bit for bit from run to run.  The
 * number of blocks is min(tiles, 512) (a tile: one plane, 4 rows, 64 columns),
 * or the tuning key conv_wgrad_blocks (1..4096; 0, default: as above) -- launch
 * shape only, read by both functions, and like sweep_fused_cl taken by
 * sfm_tune_set / sfm_tune_get without being enumerated by sfm_tune_key: it is
 * the tests' handle on few blocks, many blocks and more blocks than tiles.
 * Profile name "conv3_wgrad".
 *
 * The data gradient needs no kernel of its own.  With W[co][ci][tap] the
 * layer's weights,
 *   grad_in[p, ci] = sum over tap, co of W[co][ci][tap] grad_out[p - (tap - 1), co]
 * is sfm_conv3_f16 (scale 1, bias 0, relu 0, no residual, cout 32) on
 * grad_out with the flipped, transposed weights Wd[t][ci][co] = W[co][ci][26 - t]
 * as its 27 x 32 x 32 `weights`: one call for cin 32; for cin 64 one call per
 * 32-channel half of ci, the two outputs joined along the channel axis; for
 * cout 1, grad_out zero-padded to 32 channels as above. */
size_t sfm_conv3_wgrad_f16_workspace_bytes(int batch, int cin, int depth, int h, int w);
int sfm_conv3_wgrad_f16(const void* in, const void* grad_out, int batch, int cin, int cout, int depth, int h, int w,
                        float* grad_weights, void* workspace, size_t workspace_bytes, void* stream);

/* What stands between two such layers in a training step: the BatchNorm3d of
 * convbn_3d (models/submodule.py:17-20), the ReLU and the residual add of the
 * stack (models/PSNet.py:79-102, applied at 159-165), in float16, forward and
 * backward.  x is the raw convolution's output, voxels x 32 float16 channels
 * last (voxels = batch x depth x h x w, an int64_t: every offset is 64-bit).
 * Every pointer is 16-byte aligned and no output overlaps an input.  Nothing
 * is allocated; all launches go to `stream`.
 *
 * sfm_bn3_stats_f16 writes stats [dev] 5 x 32 float32: mean, biased variance,
 * invstd = 1 / sqrt(var + eps), a = gamma invstd, b = beta - mean a.
 *   gamma, beta  [dev] 32 float32: the module's weight and bias;
 *   training 1:  one pass over x: sum x and sum x^2 per channel in float64 (the
 *                product of two float16 values is exact there) by a fixed grid
 *                of blocks, each over a contiguous voxel range, each writing one
 *                2 x 32 double partial into `workspace`
 *                (sfm_bn3_stats_f16_workspace_bytes(voxels, 1) bytes); a second
 *                launch adds the partials in block order and derives the five
 *                rows in float64, each rounded once to float32.  No atomics: two
 *                calls give the same bits.  running_mean / running_var [dev] 32
 *                float32, each NULL or updated in place by torch's rule,
 *                (1 - momentum) r + momentum batch with the unbiased variance
 *                var voxels / (voxels - 1).  voxels >= 2;
 *   training 0:  no pass over x (which is not read), no workspace: the rows come
 *                from running_mean / running_var, which are required and left
 *                untouched.
 * The number of reducing blocks is min(ceil(voxels / 128), 512), or the tuning
 * key bn_blocks (1..4096; 0, default: as above) -- launch shape only, read by
 * the workspace queries too, and like conv_wgrad_blocks taken by sfm_tune_set /
 * sfm_tune_get without being enumerated by sfm_tune_key: the tests' handle on
 * one block, few blocks and more blocks than voxels.  Profile name "bn3_stats". */
size_t sfm_bn3_stats_f16_workspace_bytes(int64_t voxels, int training);
int sfm_bn3_stats_f16(const void* x, int64_t voxels, const float* gamma, const float* beta, double eps,
                      float* running_mean, float* running_var, double momentum, int training, float* stats,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The normalisation, activation and residual add of one layer of the same
 * stack (models/submodule.py:17-20; models/PSNet.py:79-102, 159-165) in one
 * pass: out = f16(relu(fma(a, x, b)) + residual), a and b rows 3 and 4 of
 * `stats`, the ReLU only with relu = 1, residual [dev] like x or NULL.  The
 * arithmetic is float32 and the result is rounded once (the modules round
 * after the BatchNorm and again after the add).  Profile name "bn3_apply". */
int sfm_bn3_apply_f16(const void* x, int64_t voxels, const float* stats, const void* residual, int relu, void* out,
                      void* stream);

/* The backward of sfm_bn3_apply_f16 on sfm_bn3_stats_f16's statistics (the
 * gradient of models/submodule.py:17-20 with the ReLU of models/PSNet.py:79-102,
 * 159-165), from x and `stats` alone: no output and no mask is saved.
 *   dy = grad_out, or with relu = 1 grad_out where the recomputed fma(a, x, b) > 0
 *   (the forward's float32 expression, hence the forward's mask);
 *   grad_gamma_beta [dev] 2 x 32 float32: dgamma = (sum dy x - mean sum dy) invstd,
 *   then dbeta = sum dy, the sums in float64 by the grid of sfm_bn3_stats_f16,
 *   partials in `workspace` (sfm_bn3_backward_f16_workspace_bytes(voxels) bytes)
 *   added in block order;
 *   grad_x [dev] like x, or NULL for the parameter gradients alone:
 *   training 1: a (dy - dbeta / N - xhat dgamma / N), xhat = (x - mean) invstd,
 *   N = voxels >= 2; training 0: a dy.  float32, rounded once.
 * Two launches, no atomics: two calls give the same bits.  The residual's
 * gradient is grad_out itself.  Profile name "bn3_bwd". */
size_t sfm_bn3_backward_f16_workspace_bytes(int64_t voxels);
int sfm_bn3_backward_f16(const void* x, const void* grad_out, int64_t voxels, const float* stats, int relu, int training,
                         void* grad_x, float* grad_gamma_beta, void* workspace, size_t workspace_bytes, void* stream);

/* The same three entries for the feature CNN (and context_net under
 * IND_CONTEXT): the BatchNorm2d of convbn (models/submodule.py:11-14), the ReLU
 * and the "+ x" of BasicBlock (models/submodule.py:22-44), in float16, forward
 * and backward -- what stands between two sfm_conv2x_f16 layers of a training
 * step.  x is what sfm_conv2x_f16 writes: pixels x channels float16 channels
 * last (pixels = images x h x w, an int64_t: every offset is 64-bit), channels
 * 32, 64 or 128 (anything else is refused: "channels must be 32, 64 or 128").
 * The kernels are the ones sfm_bn3_* runs, instantiated per channel count
 * (csrc/bn_act.h): the same arithmetic, order of additions, alignment and
 * aliasing rules, refusals and reproducibility; gamma, beta and the running
 * statistics hold `channels` float32, stats 5 x channels.
 *
 * sfm_bn2_stats_f16: as sfm_bn3_stats_f16; training 1 needs pixels >= 2.  The
 * number of reducing blocks is min(ceil(pixels / (4096 / channels)), 512), or
 * the tuning key bn_blocks; a partial is 2 x channels doubles, so the workspace
 * is blocks x 2 x channels x 8 bytes.  Profile name "bn2_stats". */
size_t sfm_bn2_stats_f16_workspace_bytes(int64_t pixels, int channels, int training);
int sfm_bn2_stats_f16(const void* x, int64_t pixels, int channels, const float* gamma, const float* beta, double eps,
                      float* running_mean, float* running_var, double momentum, int training, float* stats,
                      void* workspace, size_t workspace_bytes, void* stream);

/* One BatchNorm2d with its activation and residual (models/submodule.py:11-14;
 * the BasicBlock of models/submodule.py:22-44) in one pass: out =
 * f16(relu(fma(a, x, b)) + residual), the ReLU first and then the add, a and b
 * rows 3 and 4 of `stats` [dev] 5 x channels, residual [dev] like x or NULL.
 * float32, rounded once.  Profile name "bn2_apply". */
int sfm_bn2_apply_f16(const void* x, int64_t pixels, int channels, const float* stats, const void* residual, int relu,
                      void* out, void* stream);

/* The backward of sfm_bn2_apply_f16 on sfm_bn2_stats_f16's statistics (the
 * gradient of models/submodule.py:11-14 inside models/submodule.py:22-44), from
 * x and `stats` alone, as sfm_bn3_backward_f16: grad_gamma_beta [dev]
 * 2 x channels float32 (dgamma, then dbeta), grad_x [dev] like x or NULL, the
 * workspace sfm_bn2_backward_f16_workspace_bytes(pixels, channels) bytes.  Two
 * launches, no atomics.  Profile name "bn2_bwd". */
size_t sfm_bn2_backward_f16_workspace_bytes(int64_t pixels, int channels);
int sfm_bn2_backward_f16(const void* x, const void* grad_out, int64_t pixels, int channels, const float* stats, int relu,
                         int training, void* grad_x, float* grad_gamma_beta, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same layer at the reference's precision (conv_precision "fp32"):
 * float32 operands on v_mfma_f32_32x32x2_f32 (an exact fmaf chain: products
 * and sums round as float32 arithmetic; only the summation order differs from
 * PSNet's own Conv3d, models/PSNet.py:79-102).
 *   in [dev] batch x depth x h x w x cin float32 (channels-last), cin 32 or 64;
 *   weights [dev] 27 x 32 x cin float32 (layout as sfm_conv3_bf16);
 *   scale, bias [dev] 32 float32; residual [dev] like out or NULL;
 *   out [dev] batch x depth x h x w x 32 float32 (cout 32), or
 *       batch x depth x h x w float32 (cout 1).  All 16-byte aligned. */
int sfm_conv3_f32(const float* in, int batch, int cin, int depth, int h, int w, const float* weights,
                  const float* scale, const float* bias, const float* residual, int relu, int cout, float* out,
                  void* stream);

/* sfm_conv3_f32's layer with fp32 products formed on the f16 matrix cores
 * (conv_precision "fp32x3", round 5): both operands split in two f16 terms
 * (x = x_hi + x_lo; the weights first scaled by 2^wexp so their lo terms stay
 * normal, the scale folded back in the epilogue) and
 * w x ~ w_hi x_hi + w_hi x_lo + w_lo x_hi, three v_mfma_f32_32x32x16_f16 per
 * k = 16 into fp32 accumulators (~2^-21 relative per product).  Same layouts
 * and arguments as sfm_conv3_f32, plus wexp in [-24, 24] (the caller picks it
 * so that 2^wexp max|w| < 2^15).  Replaces the same Conv3d layers
 * (models/PSNet.py:79-102, applied at 159-165).
 * The split is valid while every input activation is within the f16 range
 * (|x| <= 65504; the reference's fp32 Conv3d has no such limit), and it is
 * as precise as stated while x_lo = f16(x - f16(x)), ~2^-11 |x|, is a normal
 * f16: for |x| >= 2^-3.  Below 2^-3 x_lo is subnormal and the product keeps an
 * absolute error of 2^-25 |w| per term, not a relative one: the layer's error
 * doubles with every halving of the activations' scale.  range_flag [dev] two
 * int32 words (8 bytes, 4-byte aligned) or NULL: when given, the call zeroes
 * both, the kernel sets word 0 to 1 if any input activation exceeds 65504 (or
 * is infinite) and raises word 1 to the bit pattern of the layer's largest
 * finite-or-infinite |activation| (NaNs are skipped), and a second,
 * stream-ordered launch of the sfm_conv3_f32 layer overwrites out when word 0
 * is set or that maximum is below 2^-3 (its blocks exit at once otherwise) --
 * the layer's result is then exactly sfm_conv3_f32's, at any activation scale.
 * The maximum is the layer's: a layer of tiny activations with a few large
 * ones is not re-run, and its error stays small relative to its largest
 * outputs only.  NULL: no check (the caller guarantees both sides). */
int sfm_conv3_f32x3(const float* in, int batch, int cin, int depth, int h, int w, const float* weights, int wexp,
                    const float* scale, const float* bias, const float* residual, int relu, int cout, float* out,
                    int* range_flag, void* stream);

/* [batch][channels][plane] float32 (in_dtype 0) or bfloat16 (1) ->
 * [batch][plane][channels] float32 (channels a multiple of 4): the sweep's
 * cost volume into sfm_conv3_f32's layout. */
int sfm_to_channels_last_f32(const void* in, int in_dtype, int batch, int channels, int64_t plane, float* out,
                             void* stream);

/* One stage of PSNet's per-plane context stack (convtext,
 * models/PSNet.py:17-26; the seven stages 64-71; applied at 190): a 3 x 3,
 * stride 1, dilated Conv2d with "same" zero padding (pad = dilation), its
 * optional BatchNorm2d folded (eval mode), on v_mfma_f32_32x32x16_f16 with
 * fp32 accumulation:
 *   out = [relu](conv3x3(in) * scale[co] + bias[co])
 *   in [dev] images x h x w x cin float16 (channels-last), cin 32, 64, 96 or 128;
 *   weights [dev] 9 x cout_pad x cin float16, tap = kh*3 + kw, cout_pad = cout
 *     rounded up to 32 (rows beyond cout zero);
 *   dilation 1..16;
 *   scale, bias [dev] cout_pad float32 (BatchNorm folded; 1 / 0 for a plain conv);
 *   cout 32, 64, 96 or 128: out [dev] images x h x w x cout float16, rounded
 *     once (to nearest even) after the ReLU; residual1 must be NULL;
 *   cout 1: out [dev] images x h x w float32 =
 *     f16round([relu](acc * scale + bias)) + residual1[pixel] -- the float16
 *     value torch's autocast gives convs(x), then the float32 "+ plane" of
 *     PSNet.py:190; residual1 [dev] images x h x w float32 or NULL.
 * Every pointer 16-byte aligned; out aliases no input. */
int sfm_conv2_f16(const void* in, int images, int cin, int h, int w, const void* weights, int cout, int dilation,
                  const float* scale, const float* bias, int relu, const float* residual1, void* out, void* stream);

/* sfm_conv2_f16 with every 16-bit operand bfloat16 (v_mfma_f32_32x32x16_bf16),
 * the cout 1 value rounded to bfloat16 before the add: the same context stage
 * (models/PSNet.py:17-26, 64-71, 190) as the opt-in 8-bit-mantissa path. */
int sfm_conv2_bf16(const void* in, int images, int cin, int h, int w, const void* weights, int cout, int dilation,
                   const float* scale, const float* bias, int relu, const float* residual1, void* out, void* stream);

/* The context stack's first-stage input (models/PSNet.py:17-26, 64-71, 190:
 * cat(ref features, cost plane) per plane) for planes l0 .. l0+nl-1 of every
 * pair, channels-last and padded to 64 channels:
 *   ctx [dev] batch x channels x h x w float32, channels == 32;
 *   planes [dev] batch x nlabel x h x w float32;
 *   out [dev] batch x nl x h x w x 64 float16 (round to nearest even):
 *     channels 0..31 ctx[b] (the same for every plane), channel 32
 *     planes[b][l0 + l], channels 33..63 zero.  Images are b-major, so the
 *     cout 1 stage's output is batch x nl x h x w, sfm_depth_head's layout. */
int sfm_context_pack_f16(const float* ctx, const float* planes, int batch, int nlabel, int l0, int nl, int channels,
                         int h, int w, void* out, void* stream);

/* sfm_context_pack_f16 writing bfloat16 (models/PSNet.py:17-26, 64-71, 190). */
int sfm_context_pack_bf16(const float* ctx, const float* planes, int batch, int nlabel, int l0, int nl, int channels,
                          int h, int w, void* out, void* stream);

/* Training the context stack in float16 (the reference trains under float16
 * autocast, cfgs/kitti.yml:10 MIXED_PREC): the weight gradient of one raw
 * stage of the stack (convtext, models/PSNet.py:17-26; the seven stages 64-71;
 * applied per plane at 175-190), on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation:
 *   grad_weights[tap][co][ci] = sum over image, y, x of
 *       grad_out[img, y, x, co] in[img, y + (kh-1) dil, x + (kw-1) dil, ci]
 * (zero outside the image; tap = kh*3 + kw).
 *   in           [dev] images x h x w x cin float16, cin 32, 64, 96 or 128: the
 *                stage's input, as sfm_conv2_f16 read it;
 *   grad_out     [dev] images x h x w x cout_pad float16, cout_pad 32, 64, 96 or
 *                128: the gradient of the raw convolution's output.  The cout 1
 *                stage passes its gradient as channel 0 of a zero-padded
 *                32-channel tensor and reads row co = 0;
 *   dilation     1..16;
 *   grad_weights [dev] 9 x cout_pad x cin float32, sfm_conv2_f16's pack layout;
 *   workspace    [dev] sfm_conv2_wgrad_f16_workspace_bytes(images, cin, cout_pad,
 *                h, w) bytes, 16-byte aligned: one 9 x cout_pad x cin float32
 *                partial sum per accumulating block.
 * Every pointer 16-byte aligned; grad_weights and workspace overlap neither
 * each other nor an input.  A fixed grid of accumulating blocks walks
 * contiguous ranges of tiles (4 rows x 64 columns of one image), each block
 * writing one partial, and a second launch adds the partials in block order: no
 * float atomics, so two calls give the same bits.  The number of blocks is
 * min(tiles, 512), or the tuning key conv2_wgrad_blocks (1..4096; 0, default:
 * as above) -- launch shape only, read by both functions, and like
 * conv_wgrad_blocks taken by sfm_tune_set / sfm_tune_get without being
 * enumerated by sfm_tune_key.  Profile name "conv2_wgrad". */
size_t sfm_conv2_wgrad_f16_workspace_bytes(int images, int cin, int cout_pad, int h, int w);
int sfm_conv2_wgrad_f16(const void* in, const void* grad_out, int images, int cin, int cout_pad, int h, int w,
                        int dilation, float* grad_weights, void* workspace, size_t workspace_bytes, void* stream);

/* The data gradient of the same stage (models/PSNet.py:17-26, 64-71, 175-190)
 * through the previous stage's ReLU.  With W[co][ci][tap] the stage's weights,
 *   grad_in[p, ci] = sum over tap, co of W[co][ci][tap] grad_out[p - (tap - 1) dil, co]
 * is sfm_conv2_f16's kernel on grad_out with the flipped, transposed weights
 * Wd[t][ci][co] = W[co][ci][8 - t] at the same dilation, and the epilogue
 *   grad_in[p, c] = act[p, c] > 0 ? f16(acc) : 0
 * a select, not a product: a non-finite gradient under a zero activation gives
 * +0, one under a positive activation comes through (a GradScaler sees it).
 *   grad_out [dev] images x h x w x cout_pad float16, cout_pad 32, 64, 96 or 128
 *            (the cout 1 stage: zero-padded to 32 channels, as above);
 *   weights  [dev] 9 x cin_pad x cout_pad float16: Wd, rows beyond cin and
 *            columns beyond cout zero;
 *   act      [dev] images x h x w x cin_pad float16: the stage's saved input,
 *            which is the previous stage's ReLU output; NULL (the first stage):
 *            nothing is masked;
 *   grad_in  [dev] images x h x w x cin_pad float16, cin_pad 32, 64, 96 or 128.
 * Every pointer 16-byte aligned; grad_in aliases no input.  Profile name
 * "conv2_dgrad". */
int sfm_conv2_dgrad_f16(const void* grad_out, int images, int cout_pad, int h, int w, const void* weights, int cin_pad,
                        int dilation, const void* act, void* grad_in, void* stream);

/* The first stage's data gradient back to PSNet's tensors: the backward of
 * sfm_context_pack_f16 and of the "+ plane" of models/PSNet.py:190 (the stack
 * of 17-26, 64-71, applied at 175-190), for planes l0 .. l0+nl-1 of every pair.
 *   grad_in0    [dev] batch x nl x h x w x 64 float16, 16-byte aligned: channels
 *               0..31 the feature gradient per plane, channel 32 the plane's,
 *               33..63 ignored;
 *   grad_out    [dev] batch x nlabel x h x w float32: the gradient of the stack's
 *               output;
 *   grad_ctx    [dev] batch x 32 x h x w float32: the planes' feature gradients
 *               added in ascending plane order in float32, onto the value
 *               already there, or onto zero with first != 0;
 *   grad_planes [dev] batch x nlabel x h x w float32:
 *               [b][l0 + l] = f32(grad_in0[b][l][.., 32]) + grad_out[b][l0 + l].
 * Called chunk after chunk in ascending plane order (first != 0 for the first)
 * the result has the same bits for any chunking.  Profile name
 * "context_unpack_grad". */
int sfm_context_unpack_grad_f16(const void* grad_in0, const float* grad_out, int batch, int nlabel, int l0, int nl,
                                int h, int w, int first, float* grad_ctx, float* grad_planes, void* stream);

/* The first-stage input of the full-resolution depth refinement stack
 * dep_convs (models/PSNet.py:218-221: up_feat = interpolate(refimg_fea,
 * [H, W], bilinear, align_corners=True); cat((depth, up_feat, ref))) for
 * pairs b0 .. b0+nb-1, channels-last and padded to 64 channels, the
 * upsample fused in:
 *   depth [dev] batch x H x W float32;
 *   feat [dev] batch x channels x h x w, channels == 32, float32
 *     (feat_dtype 0), bfloat16 (1) or float16 (2), read as it is;
 *   image [dev] batch x 3 x H x W float32;
 *   out [dev] nb x H x W x 64 float16 (round to nearest even), 16-byte
 *     aligned: channel 0 depth, 1..32 the features at
 *     src = dst * (in - 1) / (out - 1) (0 when out == 1), interpolated in
 *     torch's order of operations in float64 and rounded once (a float32
 *     evaluation is several float16 steps off where the terms cancel), 33..35
 *     the image, 36..63 zero.  dep_convs.0.0.weight packs without a
 *     permutation.
 * sfm_conv2_f16 runs the stack on it (cin 64); its cout 1 stage takes depth
 * as residual1 (PSNet.py:221 "+ depth"). */
int sfm_dep_context_pack_f16(const float* depth, const void* feat, int feat_dtype, const float* image, int batch,
                             int b0, int nb, int channels, int h, int w, int H, int W, void* out, void* stream);

/* sfm_dep_context_pack_f16 writing bfloat16 (models/PSNet.py:218-221). */
int sfm_dep_context_pack_bf16(const float* depth, const void* feat, int feat_dtype, const float* image, int batch,
                              int b0, int nb, int channels, int h, int w, int H, int W, void* out, void* stream);

/* The first stage's data gradient of dep_convs back to the features: the
 * backward of sfm_dep_context_pack_f16's bilinear upsample (models/PSNet.py:218-221:
 * up_feat = interpolate(refimg_fea, [H, W], bilinear, align_corners=True)) for
 * pairs b0 .. b0+nb-1.
 *   grad_in0  [dev] nb x H x W x 64 float16, 16-byte aligned: the gradient
 *             sfm_conv2_dgrad_f16(..., act = NULL) writes for the stack's first
 *             stage.  Channels 1..32 are the upsampled features' gradient;
 *             channel 0 (the reference feeds depth.detach()) and 33..63 (the
 *             image and the padding) are ignored;
 *   grad_feat [dev] batch x channels x h x w float32, channels == 32: pairs
 *             b0 .. b0+nb-1 are written (not added to), the others left as
 *             they are.
 * The exact adjoint of the forward with the forward's own weights: with
 * sy = (h - 1) / (H - 1) (0 when H == 1), fy = sy y, y0 = min((int)fy, h - 1),
 * y1 = y0 + (y0 < h - 1), ly1 = fy - y0, ly0 = 1 - ly1 in float64, and the same
 * in x,
 *   grad_feat[c][i][j] = sum over y, x of wy(i, y) wx(j, x) grad_in0[y][x][1 + c],
 *   wy(i, y) = ly0 [y0 == i] + ly1 [y1 == i].
 * A gather: every source pixel finds the destination rows and columns that read
 * it by evaluating that index expression (no inverted formula), weights them in
 * float64 and adds them rows ascending, then columns ascending, in float64,
 * rounded once to float32.  No float atomics: two calls give the same bits, and
 * a pair's result depends on that pair alone, so on no chunking.  Any ratio:
 * H == 1 or W == 1 (every destination on source 0), and H < h, where a source
 * pixel nothing reads is written as +0.  A zero weight still multiplies its
 * gradient, as torch's backward does, and nothing is filtered: a non-finite
 * gradient comes through (a GradScaler sees it).  Profile name
 * "dep_context_unpack_grad". */
int sfm_dep_context_unpack_grad_f16(const void* grad_in0, int batch, int b0, int nb, int channels, int h, int w, int H,
                                    int W, float* grad_feat, void* stream);

/* One Conv2d of PSNet's feature CNN (models/submodule.py:11-15 convbn, 22-44
 * BasicBlock with its downsample and "+= x", 108-184 feature_extraction), its
 * BatchNorm2d folded (eval mode): sfm_conv2_f16 generalised to that layer set,
 * on v_mfma_f32_32x32x16_f16 with fp32 accumulation:
 *   out = f16round([relu](conv(in) * scale[co] + bias[co]) + residual)
 *   in [dev] images x hin x win x cin float16 (channels-last), cin a multiple
 *     of 32 from 32 to 320 (the image's 3 channels padded to 32, sfm_image_pack_f16);
 *   ksize 3 or 1; stride 1 or 2; dilation 1..16, and 1 only for ksize 1 or
 *     stride 2; zero padding of dilation (3 x 3) or 0 (1 x 1), so
 *     hout = (hin - 1) / stride + 1 and wout = (win - 1) / stride + 1;
 *   weights [dev] ksize^2 x cout x cin float16, tap = kh*ksize + kw;
 *   cout 32, 64, 96 or 128; scale, bias [dev] cout float32;
 *   residual [dev] images x hout x wout x cout float16 or NULL, added in fp32
 *     before the one rounding (to nearest even); relu with a residual is refused;
 *   out [dev] images x hout x wout x cout float16.
 * At ksize 3, stride 1, residual NULL the result is sfm_conv2_f16's, bit for
 * bit.  Every pointer 16-byte aligned; out aliases no input. */
int sfm_conv2x_f16(const void* in, int images, int cin, int hin, int win, const void* weights, int cout, int ksize,
                   int stride, int dilation, const float* scale, const float* bias, int relu, const void* residual,
                   void* out, void* stream);

/* Training the feature CNN in float16 (the reference trains under float16
 * autocast, cfgs/kitti.yml:10 MIXED_PREC, in model.train()): the weight
 * gradient of one raw Conv2d of sfm_conv2x_f16's layer set (models/submodule.py:11-15
 * convbn, 22-44 BasicBlock and its downsample, 108-184 feature_extraction), on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation:
 *   grad_weights[tap][co][ci] = sum over image, y, x of
 *       grad_out[img, y, x, co] in[img, y stride + (kh - pad) dil, x stride + (kw - pad) dil, ci]
 * (zero outside the image; tap = kh*ksize + kw; pad = 1 at 3 x 3, 0 at 1 x 1).
 *   in           [dev] images x hin x win x cin float16, cin a multiple of 32
 *                from 32 to 320: the layer's input, as sfm_conv2x_f16 read it;
 *   grad_out     [dev] images x hout x wout x cout float16, cout 32, 64, 96 or
 *                128, hout = (hin - 1) / stride + 1, wout = (win - 1) / stride + 1:
 *                the gradient of the raw convolution's output;
 *   ksize 3 or 1; stride 1 or 2; dilation 1..16, and 1 only for ksize 1 or
 *                stride 2;
 *   grad_weights [dev] ksize^2 x cout x cin float32, sfm_conv2x_f16's pack layout;
 *   workspace    [dev] sfm_conv2x_wgrad_f16_workspace_bytes(images, cin, cout,
 *                hin, win, ksize, stride) bytes, 16-byte aligned: one ksize^2 x
 *                cout x cin float32 partial sum per accumulating block.
 * Every pointer 16-byte aligned; grad_weights and workspace overlap neither
 * each other nor an input.  Refused: hin * win * max(cin, 128) >= 2^31 (32-bit
 * in-image offsets; offsets across images are 64-bit).  sfm_conv2_wgrad_f16's
 * scheme: a fixed grid of accumulating blocks walks contiguous ranges of tiles
 * (4 rows x 64 columns of grad_out), each block writing one partial, and a
 * second launch adds the partials in block order: no float atomics, so two
 * calls give the same bits.  The number of blocks is min(tiles, 512), or the
 * tuning key conv2_wgrad_blocks (launch shape only, read by both functions).
 * At ksize 3, stride 1, cin <= 128 the call runs sfm_conv2_wgrad_f16 and the
 * result is its, bit for bit.  Profile name "conv2x_wgrad" (that case is
 * recorded under "conv2_wgrad" as well). */
size_t sfm_conv2x_wgrad_f16_workspace_bytes(int images, int cin, int cout, int hin, int win, int ksize, int stride);
int sfm_conv2x_wgrad_f16(const void* in, const void* grad_out, int images, int cin, int cout, int hin, int win,
                         int ksize, int stride, int dilation, float* grad_weights, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The data gradient of the same layer (models/submodule.py:11-15, 22-44,
 * 108-184).  With W[co][ci][tap] the layer's weights,
 *   grad_in[img, p, ci] = sum over tap, co and every output pixel q with
 *       q stride + (tap - pad) dil = p of W[co][ci][tap] grad_out[img, q, co],
 * accumulated in fp32 and rounded once to float16 (to nearest even).  No mask
 * and no fused add: on the training route BatchNorm2d sits between a
 * convolution and its ReLU, and autograd sums the residual fork.
 *   grad_out [dev] images x hout x wout x cout float16, cout 32, 64, 96 or 128;
 *   weights  [dev] ksize^2 x cin x cout float16: the dgrad pack
 *            Wd[t][ci][co] = W[co][ci][ksize^2 - 1 - t], rows beyond the
 *            layer's cin and columns beyond its cout zero;
 *   hin, win the input's size: at stride 2 both 2 hout - 1 and 2 hout are
 *            inputs of hout rows, so hout == (hin - 1) / stride + 1 is
 *            required, and the same for win;
 *   grad_in  [dev] images x hin x win x cin float16, cin a multiple of 32 from
 *            32 to 320, written in one call (at most 128 channels per launch).
 * ksize, stride and dilation as above.  A gather, no atomics: two calls give
 * the same bits.  At stride 1 it is sfm_conv2x_f16's implicit GEMM on grad_out
 * with Wd at the same dilation.  At stride 2 an input pixel of row parity a and
 * column parity b reads the kernel rows with a + pad - kh even and the kernel
 * columns with b + pad - kw even: 1, 2, 2 or 4 live taps per parity class at
 * 3 x 3.  Every pixel of grad_in is written.  At 3 x 3 with pad 1 every input
 * pixel is read by an output: p odd by tap 2 of q = (p - 1) / 2 <= hout - 1, p
 * even by tap 1 of q = p / 2, so no pixel is without a term.  At 1 x 1 / stride
 * 2 the pixels of an odd row or column are read by no output and are written
 * as +0, their gradient.  At ksize 3, stride 1, cin <= 128 the call runs
 * sfm_conv2_dgrad_f16(act = NULL) and the result is its, bit for bit.  Every
 * pointer 16-byte aligned; grad_in overlaps no input; the same size refusal as
 * above.  Profile name "conv2x_dgrad". */
int sfm_conv2x_dgrad_f16(const void* grad_out, int images, int cout, int hout, int wout, const void* weights, int cin,
                         int hin, int win, int ksize, int stride, int dilation, void* grad_in, void* stream);

/* The feature CNN's first input (models/submodule.py:112 firstconv's 3-channel
 * convbn): image [dev] batch x 3 x h x w float32 -> out [dev] batch x h x w x 32
 * float16, channels 0..2 the image (round to nearest even), 3..31 zero.
 * Both pointers 16-byte aligned. */
int sfm_image_pack_f16(const float* image, int batch, int h, int w, void* out, void* stream);

/* The AvgPool2d of the feature CNN's pyramid branches (models/submodule.py:
 * 125-139 branch1..4: kernel = stride = pool): in [dev] images x h x w x
 * channels float16 (channels a multiple of 8, at most 2048) -> out [dev]
 * images x h/pool x w/pool x channels float16 (both divisions floor; h, w >=
 * pool), pool 4, 8, 16 or 32: the window summed in fp32, times 1 / pool^2,
 * rounded once.  Both pointers 16-byte aligned. */
int sfm_avgpool_f16(const void* in, int images, int h, int w, int channels, int pool, void* out, void* stream);

/* lastconv's input (models/submodule.py:169-181: the four branches upsampled
 * to the skip map's size, bilinear, align_corners=True, and
 * cat((output_raw, output_skip, branch4, branch3, branch2, branch1), 1)):
 *   raw [dev] images x h x w x 64, skip [dev] images x h x w x 128 float16;
 *   branches [host] 4 device pointers in cat order (branch4, branch3, branch2,
 *     branch1), map b images x branch_h[b] x branch_w[b] x 32 float16;
 *     branch_h, branch_w [host] 4 ints, each >= 1 (a 1 x 1 map has scale 0);
 *   out [dev] images x h x w x 320 float16: channels 0..63 raw, 64..191 skip,
 *     192 + 32 b .. the branch b map at src = dst * (in - 1) / (out - 1),
 *     interpolated in torch's order of operations in float64 and rounded once,
 *     as sfm_dep_context_pack_f16 does.
 * Every device pointer 16-byte aligned; out aliases no input. */
int sfm_spp_pack_f16(const void* raw, const void* skip, const void* const* branches, const int* branch_h,
                     const int* branch_w, int images, int h, int w, void* out, void* stream);

/* Tuning knobs (process-wide; every key, its accepted values and default):
 *
 *   launch shape only -- outputs are bit-identical for every value:
 *     "solve_lanes"           1..16   lanes per wave in k_solve_front (16)
 *     "solve_coop"            0, 1    k_solve_front's equations and reduction and
 *                                     k_solve_back on DPP quads, 4 lanes per
 *                                     hypothesis (1); 0: one lane each
 *     "roots_lanes"           1..32   lanes per wave in k_roots (32)
 *     "sweep_lane_pixels"     0..2    pixel-to-lane mapping of the per-row sweep (0)
 *     "sweep_items_per_block" 1,2,4,8 work items per block of the per-row sweep (4)
 *     "sweep_nj"              1,2,4   pixels per lane of k_sweep_tile (1; bf16 uses 2)
 *     "sweep_buffer"          0, 1    buffer-addressed interior path of k_sweep_tile (1)
 *     "sweep_share"           0, 1    k_sweep_tile interior path: right-hand bilinear taps
 *                                     from the next lane where the offsets match (0)
 *     "sweep_store_nt"        0,1,2   k_sweep_tile's volume stores non-temporal (sc0 nt)
 *                                     so they do not evict the re-read operands
 *                                     (2, default: bf16 volumes, and fp32 volumes
 *                                     whose channel slab L*h*w*4 is <= 6 MiB --
 *                                     measured per shape, e.g. on for the indoor
 *                                     120x160 L=64 volume, off for KITTI 94x311)
 *     "sweep_store_wt"        -1..3   cache policy of k_sweep_tile's 16-byte stores:
 *                                     0 by sweep_store_nt, 1 sc1 (write-through:
 *                                     the line is not kept in the XCD's L2), 2 sc0
 *                                     sc1, 3 nt sc1; -1 (default): fp32 volumes 3,
 *                                     bf16 volumes 0; same bits
 *     "sweep_store_px"        -1,0,1, 16-byte lane stores of k_sweep_tile (8 bf16 / 4
 *                             2,4,8   fp32 consecutive pixels through a per-wave LDS
 *                                     stage) with that many pixels per lane for the
 *                                     taps; 0: plain 4-byte lane stores; -1 (default):
 *                                     bf16 2, fp32 1; same bits
 *     "sweep_run"             1..1024 planes per block of k_sweep_band (16)
 *     "sweep_band_rows"       2..64   target rows k_sweep_band stages in LDS (16,
 *                                     clipped to 80 KB per block)
 *     "score_blocks_per_cu"   1..64   persistent k_score32 blocks per CU (32)
 *     "score_mf_blocks_per_cu" 1..8   persistent k_score_mf blocks per CU (1)
 *     "score_prune"           0, 1    exact bound pruning in k_score32 (1; winner,
 *                                     count, E, P unchanged -- losing hypotheses'
 *                                     scores become lower bounds, so it is off
 *                                     whenever per-hypothesis scores are requested)
 *     "score_interleave"      0, 1    pair-interleaved k_score32 items (0)
 *     "score_fp32"            0, 1    float32 pre-decision level of k_score32 (1; exact by proof)
 *     "score_mf"              0..2    split-f16 matrix-core scorers (2: span-major
 *                                     k_score_mf2, 1: k_score_mf, 0: VALU scorers;
 *                                     2 by default; exact by proof, same counts)
 *     "score_mf_chunk"        1..4096 k_score_mf2's smallest claimed unit range, in
 *                                     (span, 32-candidate tile) units (64)
 *     "score_mf_chunk2"       0..4096 the same for the pruned sequence's last launch (0: as
 *                                     score_mf_chunk)
 *     "score_mf_prune"        0, 500..990  count-bound pruning in k_score_mf2 (880):
 *                                     every candidate scored on the first N per
 *                                     mille of each pair's 1024-point spans, then
 *                                     up to the pair's pruning point 1 - (inlier
 *                                     ratio estimated from them) + margin
 *                                     (k_mf2_split), then only candidates whose
 *                                     bound can still reach the leader's exact
 *                                     count (k_mf2_lead / _keep); 0 = one launch.
 *                                     Winner, count, E, P unchanged; only with
 *                                     num_test == num_ransac_test, no per-
 *                                     hypothesis scores, >= 32 spans per pair
 *     "score_mf_prune_margin" 0..200  that margin, per mille (10)
 *     "score_mf_prune_upper"  0, 1    1 (default, round 6): every candidate on
 *                                     every point with the one-sided test (counts
 *                                     of the points not certainly outliers: upper
 *                                     bounds), the leader counted exactly, and only
 *                                     the candidates whose upper count reaches it
 *                                     counted exactly (float64, or the two-sided
 *                                     matrix-core pass past 256 per pair); 0: the
 *                                     round-5 two-sided passes with the pruning
 *                                     point above.  Winner, count, E, P unchanged
 *     "score_mf_exact_max"    0..256  with score_mf_prune_upper: pairs with at most
 *                                     this many kept candidates count them in
 *                                     float64 (k_mf2_exact), the others on the
 *                                     matrix cores (256; same counts either way)
 *     "roots_split"           0, 1, 2 k_roots_split: falsi nodes shared by the wave's
 *                                     64 lanes (1, default), or by the four waves of
 *                                     a block (2, measured 2-6 % slower), speculated
 *                                     fallback bisection; same bits as k_roots (0)
 *     "conv_rolling"          0, 1    rolling-plane Conv3d for cin 32 (1; same bits)
 *     "conv_planes"           0,4,8,  output planes per block of the rolling-plane
 *                             16,32   Conv3d (0, default: by grid size; same bits)
 *
 *   results MAY change (sweep outputs by FMA rounding only):
 *     "sweep_flat"            0..3    2 (default): k_sweep_tile, 1: k_sweep_flat,
 *                                     3: k_sweep_band (plane runs, target band in
 *                                     LDS; measured slower); 1-3 are bit-identical
 *                                     to each other; they sum the
 *                                     four bilinear taps with FMA, which differs
 *                                     from 0, the per-row kernel in the
 *                                     reference's mul/add order, by <= 7.2e-7
 *                                     absolute on N(0,1) features
 *     "sweep_group"           4, 8    channels per sweep window (8); the channel
 *                                     group changes nothing but the launch shape
 *     "score_precision"       64, 32, 16  64 (default): the reference's float64
 *                                     ComputeError decision, exact; 32 / 16:
 *                                     ComputeError<float> / <half> semantics
 *                                     (approximate inlier sets, BASELINE C5)
 *     "score_lowp_template"   0, 1    32 / 16 only: 0 (default) E and every
 *                                     operation held in T; 1 the literal
 *                                     ComputeError<T> with the reference's
 *                                     double Ematrix (double products, sums
 *                                     rounded to T; kernel_functions.cu:231-264,
 *                                     common.h:26) */
int sfm_tune_set(const char* key, int value);
/* The current value of a tuning key. */
int sfm_tune_get(const char* key, int* value);
/* The name of tuning key `index` (0, 1, ...), NULL past the last one: lets a
 * caller snapshot and restore every knob (tests/conftest.py does, around
 * each GPU test). */
const char* sfm_tune_key(int index);
/* The score kernel the most recent RANSAC / score call of this process
 * dispatched ("k_score_mf2", "k_score_mf", "k_score32", ...; "" before any),
 * followed by "+prune" when k_score_mf2 ran with count-bound pruning (two
 * launches and k_mf2_lead / k_mf2_keep between them).  A dispatch check for tests. */
const char* sfm_last_scorer(void);
/* The kernel form the most recent plane-sweep call of this thread launched
 * ("" before any), taken from the call's launch plan.  A dispatch check for
 * tests.  The planar entries (sfm_plane_sweep, _ex, _warped, _psnet,
 * _psnet_warped_half):
 *   "k_sweep_tile+wide"  k_sweep_tile whose interior windows use 16-byte stores (the default)
 *   "k_sweep_tile"       k_sweep_tile with 4-byte stores (odd slab, unaligned
 *                        output, sweep_share, sweep_store_px = 0, sweep_buffer = 0)
 *   "k_sweep_flat"       sweep_flat = 1, and sweep_flat = 3 whose band does not fit
 *   "k_sweep_band"       sweep_flat = 3
 *   "k_sweep+vec"        the per-row form with 16-byte row stores (sweep_flat = 0,
 *                        or a shape outside the other forms' range)
 *   "k_sweep"            the per-row form with element stores
 * sfm_plane_sweep_cl, _cl_f16: "k_sweep_cl" (the fast path) or "k_sweep_cl_any";
 * sfm_plane_sweep_ref_planes: "k_ref_planes" or "k_ref_planes_generic";
 * sfm_plane_sweep_backward, sfm_inverse_warp_backward: "k_sweep_bwd" (an LDS
 * window of target rows per workgroup, flushed with row-contiguous atomics) or
 * "k_sweep_bwd+global" (rows too long for a window: every tap a global atomic). */
const char* sfm_last_sweep(void);

/* ------------------------------------------------------------------------
 * Per-kernel timing (HIP events recorded around every launch on the
 * launching stream while enabled).
 * ------------------------------------------------------------------------ */
int sfm_profile_enable(int on);
/* Restrict the recording to the comma-separated kernel names in `names`
 * (NULL or "" = every profiled kernel).  Each recorded launch adds two event
 * records to its stream (~3.5 us per step per kernel on MI355X between
 * dependent launches), so bench.py records only the roofline kernels inside
 * its timed region. */
int sfm_profile_select(const char* names);
int sfm_profile_reset(void);
/* Synchronises the recorded events; total milliseconds and launch count of
 * kernel `name` ("ransac_solve", "ransac_chain", "ransac_score",
 * "ransac_select", "flow_to_points", "plane_sweep", "sweep_tgt_quads",
 * "depth_metrics", ...). */
int sfm_profile_read(const char* name, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif

#endif /* SFM_HIP_H */
