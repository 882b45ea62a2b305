// RANSAC five-point essential matrix on CDNA4 (gfx950): the driver.
//
// Replaces the reference's essential_matrix extension hot path
// (RANSAC_FiveP/essential_matrix/essential_matrix.cu:110-280 host drivers,
// kernel_functions.cu:53-226 kernels).  The reference runs 512 threads, each
// looping over `ransac_iter` hypotheses and scoring every candidate E against
// all N correspondences serially.  Here the same semantics are split into
// data-parallel phases, each profiled under its own name:
//
//   ransac_solve   (ransac_solve.hip) one hypothesis per lane or DPP quad:
//                  k_solve_front (Philox sample, E basis, equations, det
//                  poly), k_roots / k_roots_split (Sturm root isolation),
//                  k_solve_back (E per root, cheirality, compaction).
//                                                           (latency-bound)
//   ransac_chain   (ransac_solve.hip) k_chain, one lane per reference thread
//                  ("chain"): resolves the stale slot-0 E/P state a chain
//                  carries across its iterations; k_cand emits the dense
//                  candidate records (prefix sum per pair).
//   ransac_score   (ransac_score.hip) the Sampson-style inlier test of every
//                  (candidate, point): on the matrix cores with split-f16
//                  operands (k_score_mf2, span-major, with count-bound
//                  pruning; k_score_mf) or on the vector ALUs (k_score32,
//                  k_score), as make_score_plan chooses.  Right before it the
//                  stream coordination of score_sync.cpp: score fence, score
//                  gate; a reference-half job may ride on its first launch.
//   ransac_select  (ransac_solve.hip) k_select, per pair: preselect / rescore
//                  per hypothesis, first-max argmax.
//
// Inlier decisions are bit-identical to the reference's IEEE evaluation
// e = |x'^T E x| / sqrt(Ex0^2+Ex1^2+xE0^2+xE1^2) <= thr (ComputeError,
// kernel_functions.cu:232-264).  Every scorer decides most (candidate, point)
// pairs on a cheaper evaluation with a proven error bound and re-evaluates
// the rare undecided ones in the reference's exact operation order.
#include <string>
#include <vector>
#include "ransac_common.h"

namespace sfm {

template <class Src>
static int run_chunk(const Src& src, const int64_t* n, int bc, int num_test,
                     int num_ransac_test, int iters, double thr, uint64_t seed, int cheir,
                     const Workspace& w, int ws_batch, double* E_out, double* P_out, int32_t* inliers_out,
                     int32_t* winner_out, int32_t* score_out, hipStream_t s, bool first_chunk,
                     const RefJob* ref_job = nullptr, bool* rode = nullptr) {
  const int H = kChains * iters;
  const int cmax = H * kMaxSlots;
  PairParams pp{};
  for (int b = 0; b < bc; ++b) {
    pp.n[b] = n[b];
    pp.test[b] = (int32_t)(num_test > 0 ? num_test : n[b]);
    pp.rtest[b] = (int32_t)(num_ransac_test > 0 ? num_ransac_test : n[b]);
    const int M = std::max(pp.test[b], pp.rtest[b]);
    pp.splits[b] = (M + kPtsPerItem - 1) / kPtsPerItem;
  }
  const ScorePlan plan = make_score_plan(thr, pp, bc, cmax, ws_batch, score_out != nullptr, true);
  launch_solve(src, pp, bc, H, seed, cheir, w, s);
  SFM_LAUNCHED();
  launch_chain(bc, H, iters, cheir, thr, plan, w, first_chunk, s);
  SFM_LAUNCHED();
  SFM_REQUIRE(prune_state(w.cntR, ws_batch, cmax).skipped == w.skipped, "internal: pruning state layout");
  if (plan.kc.prune) {
    SFM_HIP(hipMemsetAsync(w.cov, 0, (size_t)bc * cmax * 8, s));
    SFM_HIP(hipMemsetAsync(w.best_lb, 0, SFM_MAX_BATCH * kBestStride * 4, s));
  }
  if (int rc = record_score_fence(s)) return rc;
  if (int rc = wait_score_gate(s)) return rc;
  {
    ProfScope ps("ransac_score", s);
    ScoreBufs sb{w.cand_total, w.candE, w.candF, w.cntT, w.cntR, w.claim};
    sb.cmap = w.cmap;
    sb.cmap2 = w.cmap2;
    sb.lead = w.lead;
    sb.bnd = w.bnd;
    sb.skipped = w.skipped;
    launch_score(src, pp, sb, plan, s, ref_job, rode);
  }
  SFM_LAUNCHED();
  launch_select(bc, H, cheir, plan, w, score_out, E_out, P_out, inliers_out, winner_out, s);
  SFM_LAUNCHED();
  return SFM_OK;
}

static int check_common(int iters, double thr, int batch) {
  SFM_REQUIRE(batch >= 1, "batch must be >= 1");
  SFM_REQUIRE(iters >= 1 && iters <= 4096, "iters must be in [1, 4096]");
  SFM_REQUIRE(thr > 0.0, "inlier threshold must be > 0");
  return SFM_OK;
}

template <class Src>
static int run_src(const Src& src, const int64_t* n, int batch, int num_test, int num_ransac_test, int iters,
                   double thr, uint64_t seed, int cheir, void* ws, size_t ws_bytes, double* E_out, double* P_out,
                   int32_t* inliers_out, int32_t* winner_out, int32_t* score_out, hipStream_t s) {
  const int bc = std::min(batch, SFM_MAX_BATCH);
  const size_t need = layout(nullptr, bc, 0, iters, nullptr);
  if (!ws || ws_bytes < need) {
    set_error("workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  Workspace w;
  layout((char*)ws, bc, 0, iters, &w);
  const int H = kChains * iters;
  // a reference-half job armed for this stream (sfm_score_ref_job): consumed
  // here; the first chunk's scorer writes it when its first launch is the
  // one-sided pass and the shape is in the rider's range, else the reference
  // kernels do, on this stream, before the call returns
  RefJob job;
  const bool have_job = take_ref_job(s, &job);
  bool rode = false;
  for (int b0 = 0; b0 < batch; b0 += bc) {
    const int nb = std::min(bc, batch - b0);
    const int rc = run_chunk(src.shifted(b0), n + b0, nb, num_test, num_ransac_test, iters, thr, seed, cheir, w, bc,
                             E_out + (size_t)b0 * 9, P_out ? P_out + (size_t)b0 * 12 : nullptr, inliers_out + b0,
                             winner_out ? winner_out + b0 : nullptr,
                             score_out ? score_out + (size_t)b0 * H : nullptr, s, b0 == 0,
                             have_job && b0 == 0 ? &job : nullptr, &rode);
    if (have_job && b0 == 0 && !rode)
      if (int rc2 = sfm_plane_sweep_ref_planes(job.ref, job.batch, job.channels, job.h, job.w, job.nlabel, job.dtype,
                                               job.cost, nullptr, 0, s))
        return rc2;
    if (rc) return rc;
  }
  return SFM_OK;
}

static int run_packed(const double* pts, int64_t n_stride, const int64_t* n, int batch, int num_test,
                      int num_ransac_test, int iters, double thr, uint64_t seed, int cheir, void* ws,
                      size_t ws_bytes, double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out,
                      int32_t* score_out, hipStream_t s) {
  if (int rc = check_common(iters, thr, batch)) return rc;
  SFM_REQUIRE(pts && n && E_out && inliers_out, "null pointer argument");
  SFM_REQUIRE(cheir == 0 || P_out, "P_out required when cheirality is on");
  SFM_REQUIRE(n_stride >= 1 && n_stride <= (int64_t)INT32_MAX, "n_stride out of range");
  for (int b = 0; b < batch; ++b) {
    SFM_REQUIRE(n[b] >= 1 && n[b] <= n_stride, "each n[b] must be in [1, n_stride]");
    SFM_REQUIRE(num_test <= n[b] && num_ransac_test <= n[b],
                "num_test_points / num_ransac_test_points must not exceed the number of points");
  }
  return run_src(PackedSrc{pts, n_stride}, n, batch, num_test, num_ransac_test, iters, thr, seed, cheir, ws,
                 ws_bytes, E_out, P_out, inliers_out, winner_out, score_out, s);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_ransac5_workspace_bytes(int batch, int64_t n_max, int iters) {
  if (batch < 1 || iters < 1) return 0;
  return layout(nullptr, std::min(batch, SFM_MAX_BATCH), n_max, iters, nullptr);
}

int sfm_ransac5(const double* q, const double* qp, int64_t n, int num_test, int num_ransac_test, int iters,
                double thr, uint64_t seed, int cheirality, void* workspace, size_t workspace_bytes,
                double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out, void* stream) {
  SFM_REQUIRE(q && qp, "null point arrays");
  SFM_REQUIRE(n >= 1, "need at least one correspondence");
  SFM_REQUIRE(num_test >= 1 && num_ransac_test >= 1, "num_test_points and num_ransac_test_points must be >= 1");
  const size_t need = layout(nullptr, 1, n, iters < 1 ? 1 : iters, nullptr);
  if (!workspace || workspace_bytes < need) {
    set_error("workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  Workspace w;
  layout((char*)workspace, 1, n, iters < 1 ? 1 : iters, &w);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = sfm_pack_points(q, qp, n, w.pack, s)) return rc;
  const int64_t nn[1] = {n};
  return run_packed(w.pack, n, nn, 1, num_test, num_ransac_test, iters, thr, seed, cheirality, workspace,
                    workspace_bytes, E_out, P_out, inliers_out, winner_out, nullptr, s);
}

int sfm_ransac5_packed(const double* pts, int64_t n_stride, const int64_t* n, int batch, int num_test,
                       int num_ransac_test, int iters, double thr, uint64_t seed, int cheirality,
                       void* workspace, size_t workspace_bytes, double* E_out, double* P_out,
                       int32_t* inliers_out, int32_t* winner_out, int32_t* hyp_score_out, void* stream) {
  return run_packed(pts, n_stride, n, batch, num_test, num_ransac_test, iters, thr, seed, cheirality, workspace,
                    workspace_bytes, E_out, P_out, inliers_out, winner_out, hyp_score_out, (hipStream_t)stream);
}

int sfm_ransac5_flow(const float* flow, int batch, int H, int W, int h_side, int w_side, int margin,
                     const float* Kinv, int num_test, int num_ransac_test, int iters, double thr, uint64_t seed,
                     int cheirality, void* workspace, size_t workspace_bytes, double* E_out, double* P_out,
                     int32_t* inliers_out, int32_t* winner_out, int32_t* hyp_score_out, void* stream) {
  if (int rc = check_common(iters, thr, batch)) return rc;
  SFM_REQUIRE(flow && Kinv && E_out && inliers_out, "null pointer argument");
  SFM_REQUIRE(cheirality == 0 || P_out, "P_out required when cheirality is on");
  SFM_REQUIRE(H >= 1 && W >= 1 && h_side >= 1 && h_side <= H && w_side >= 1 && w_side <= W,
              "h_side/w_side out of range");
  SFM_REQUIRE(margin >= 0 && 2 * margin < h_side && 2 * margin < w_side, "margin leaves no pixels");
  const int64_t N = (int64_t)(h_side - 2 * margin) * (w_side - 2 * margin);
  SFM_REQUIRE(N >= 5 && N <= (int64_t)INT32_MAX, "point count out of range");
  SFM_REQUIRE(num_test <= N && num_ransac_test <= N,
              "num_test_points / num_ransac_test_points must not exceed the number of points");
  std::vector<int64_t> n((size_t)batch, N);
  const FlowSrc src{flow, Kinv, H, W, w_side - 2 * margin, margin, 1.0 / (double)(w_side - 2 * margin)};
  return run_src(src, n.data(), batch, num_test, num_ransac_test, iters, thr, seed, cheirality, workspace,
                 workspace_bytes, E_out, P_out, inliers_out, winner_out, hyp_score_out, (hipStream_t)stream);
}

size_t sfm_score_essentials_workspace_bytes(int batch, int ncand) {
  if (batch < 1 || batch > SFM_MAX_BATCH || ncand < 1) return 0;
  const size_t c = (size_t)batch * ncand;
  return align_up(SFM_MAX_BATCH * 4) + align_up(c * kCandStride * 8) + align_up(c * kMfRec * 2) + align_up(c * 4) +
         align_up(kMf2ClaimBytes);
}

int sfm_score_essentials(const double* pts, int64_t n_stride, const int64_t* n, int batch, const double* E,
                         int ncand, double thr, int32_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream) {
  SFM_REQUIRE(pts && n && E && counts, "null pointer argument");
  SFM_REQUIRE(batch >= 1 && batch <= SFM_MAX_BATCH, "batch must be in [1, 64]");
  SFM_REQUIRE(ncand >= 1 && ncand <= (1 << 20), "ncand must be in [1, 2^20]");
  SFM_REQUIRE(thr > 0.0, "inlier threshold must be > 0");
  SFM_REQUIRE(n_stride >= 1 && n_stride <= (int64_t)INT32_MAX, "n_stride out of range");
  for (int b = 0; b < batch; ++b) SFM_REQUIRE(n[b] >= 1 && n[b] <= n_stride, "each n[b] must be in [1, n_stride]");
  const size_t need = sfm_score_essentials_workspace_bytes(batch, ncand);
  if (!workspace || workspace_bytes < need) {
    set_error("workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* p = (char*)workspace;
  const size_t c = (size_t)batch * ncand;
  ScoreBufs w;
  w.cand_total = (int32_t*)p;
  p += align_up(SFM_MAX_BATCH * 4);
  w.candE = (double*)p;
  p += align_up(c * kCandStride * 8);
  w.candF = (_Float16*)p;
  p += align_up(c * kMfRec * 2);
  w.cntR = (int32_t*)p;
  p += align_up(c * 4);
  w.claim = (unsigned long long*)p;
  w.cntT = counts;
  PairParams pp{};
  for (int b = 0; b < batch; ++b) {
    pp.n[b] = n[b];
    pp.test[b] = pp.rtest[b] = (int32_t)n[b];
    pp.splits[b] = (int32_t)((n[b] + kPtsPerItem - 1) / kPtsPerItem);
  }
  const ScorePlan plan = make_score_plan(thr, pp, batch, ncand, batch, false, false);
  SFM_HIP(hipMemsetAsync(w.cntT, 0, c * 4, s));
  SFM_HIP(hipMemsetAsync(w.cntR, 0, c * 4, s));
  launch_fill_cands(E, batch, ncand, thr, plan, w, s);
  ProfScope ps("score_essentials", s);
  launch_score(PackedSrc{pts, n_stride}, pp, w, plan, s);
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_ransac5_candidate_counts(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                 int32_t* counts_host) {
  SFM_REQUIRE(workspace && counts_host && batch >= 1 && batch <= SFM_MAX_BATCH && iters >= 1, "invalid arguments");
  const int bc = batch;
  SFM_REQUIRE(workspace_bytes >= layout(nullptr, bc, 0, iters, nullptr), "workspace too small");
  Workspace w;
  layout((char*)workspace, bc, 0, iters, &w);
  SFM_HIP(hipMemcpy(counts_host, w.cand_total, sizeof(int32_t) * batch, hipMemcpyDeviceToHost));
  return SFM_OK;
}

int sfm_ransac5_hypothesis_counts(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                  int32_t* nroots_host, int32_t* ncand_host) {
  SFM_REQUIRE(workspace && nroots_host && ncand_host && batch >= 1 && batch <= SFM_MAX_BATCH && iters >= 1,
              "invalid arguments");
  const int bc = batch;
  SFM_REQUIRE(workspace_bytes >= layout(nullptr, bc, 0, iters, nullptr), "workspace too small");
  Workspace w;
  layout((char*)workspace, bc, 0, iters, &w);
  const size_t bytes = sizeof(int32_t) * (size_t)batch * kChains * iters;
  SFM_HIP(hipMemcpy(nroots_host, w.nroots, bytes, hipMemcpyDeviceToHost));
  SFM_HIP(hipMemcpy(ncand_host, w.ncand, bytes, hipMemcpyDeviceToHost));
  return SFM_OK;
}

int sfm_ransac5_skipped_evaluations(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                    unsigned long long* skipped_host) {
  SFM_REQUIRE(workspace && skipped_host && batch >= 1 && iters >= 1, "invalid arguments");
  const int bc = std::min(batch, SFM_MAX_BATCH);
  SFM_REQUIRE(workspace_bytes >= layout(nullptr, bc, 0, iters, nullptr), "workspace too small");
  Workspace w;
  layout((char*)workspace, bc, 0, iters, &w);
  SFM_HIP(hipMemcpy(skipped_host, w.skipped, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return SFM_OK;
}

int sfm_ransac5_kept_candidates(const void* workspace, size_t workspace_bytes, int batch, int iters,
                                int32_t* kept_host, int32_t* points_host) {
  SFM_REQUIRE(workspace && kept_host && batch >= 1 && batch <= SFM_MAX_BATCH && iters >= 1, "invalid arguments");
  SFM_REQUIRE(workspace_bytes >= layout(nullptr, batch, 0, iters, nullptr), "workspace too small");
  Workspace w;
  layout((char*)workspace, batch, 0, iters, &w);
  SFM_HIP(hipMemcpy(kept_host, w.lead + 3 * SFM_MAX_BATCH, sizeof(int32_t) * batch, hipMemcpyDeviceToHost));
  if (points_host) {
    SFM_HIP(hipMemcpy(points_host, w.bnd + 2 * SFM_MAX_BATCH, sizeof(int32_t) * batch, hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b) points_host[b] *= kMf2Span;   // spans -> points (the caller clamps at N)
  }
  return SFM_OK;
}

}  // extern "C"
