// Shared by the RANSAC translation units (ransac5.hip the driver,
// ransac_solve.hip, ransac_score.hip, ransac_points.hip, score_sync.cpp):
// the constants, the workspace layout, the correspondence sources, the
// scorers' argument structs and the functions the units call across each
// other.  No device code crosses a unit: what is shared here is inline.
#pragma once
#include <algorithm>
#include "common.h"

namespace sfm {

constexpr int kChains = SFM_RANSAC_CHAINS;
constexpr int kMaxSlots = 10;
constexpr size_t kMf2ClaimBytes = 9 * sizeof(unsigned long long);   // k_score_mf2's per-XCD claim counters + done
constexpr int kCandStride = 18;   // per candidate: E f64[9], Kg, then float[14] (E f32[9], A1, B1, A2, B2, ok32)
// solve state fields: E basis (36), the 3x3 blocks of the reduced equations
// that compute_E_matrix reads (39), the five samples (20), det poly (11), roots (10)
constexpr int kStEb = 0, kStA = 36, kStQ = 75, kStPoly = 95, kStRoots = 106, kStateFields = 116;
constexpr int kKC = 32;           // candidates per score tile
constexpr int kPPL = 8;           // points per lane per chunk
constexpr int kScoreThreads = 256;
constexpr int kChunk = kScoreThreads * kPPL;
constexpr int kPPL32 = 8;          // points per lane per chunk in k_score32 (6, 10, 12 measured slower)
constexpr int kPtsPerItem = 8192;  // points per k_score item (a whole number of chunks)
static_assert(kPtsPerItem % kChunk == 0, "item = whole chunks");
constexpr int kMfRec = 64;         // f16 per candidate of the matrix-core scorers: 4 A rows of K = 16 (score_mf.h)
constexpr int kMf2Span = 1024;     // points per staged span of k_score_mf2 (score_mf2.h)
constexpr int kBestStride = 64;    // best_lb[b * kBestStride]: one 256-byte line per pair (PruneState)

struct PairParams {
  int64_t n[SFM_MAX_BATCH];
  int32_t test[SFM_MAX_BATCH];     // num_test_points
  int32_t rtest[SFM_MAX_BATCH];    // num_ransac_test_points
  int32_t splits[SFM_MAX_BATCH];   // point splits of max(test, rtest)
};

struct Workspace {
  int32_t* nroots;     // [B][H]
  int32_t* ncand;      // [B][H]
  double* hypE;        // [B][H][10][9]
  double* hypP;        // [B][H][10][12]
  double* hypP0;       // [B][H][12]
  double* sstate;      // [kStateFields][B][H]: solve state between k_solve_front, k_roots, k_solve_back
  int32_t* cand_off;   // [B][H]
  int32_t* chain_ref;  // [B][H] (latest k <= i with a root) + 1 | (latest k < i with a candidate) + 1 << 16
  int32_t* cand_total; // [64]
  double* candE;       // [B][Cmax][kCandStride]
  int32_t* cntT;       // [B][Cmax]
  int32_t* cntR;       // [B][Cmax]
  int32_t* score;      // [B][H]
  _Float16* candF;     // [B][Cmax][kMfRec] split-f16 A rows of k_score_mf (k_mf_cands)
  unsigned long long* cov;      // [B][Cmax] pruning bound state: count | points covered << 32
  int32_t* best_lb;             // [64][kBestStride] largest partial count seen (a lower bound on the winning score)
  unsigned long long* skipped;  // [1] evaluations skipped by pruning (whole call)
  unsigned long long* claim;    // [9] k_score_mf2's range-claim counters and finished-block count (zero between launches)
  int32_t* cmap;       // [B][Cmax] k_mf2_keep: the kept candidates of each pair
  int32_t* cmap2;      // [B][Cmax] k_mf2_keep_map: those kept again at the end (one-sided pruning)
  int32_t* lead;       // [5][64] k_mf2_lead / _keep: leader count, index, rest count, kept candidates,
                       // kept candidates left to the matrix-core pass (one-sided pruning)
  int32_t* bnd;        // [4][64] k_mf2_split: span boundaries of the pruned launches per pair
  double* pack;        // [n_max][4] (last: its size is the only n_max-dependent one)
};

__host__ __device__ inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// Lay out the workspace; returns the byte count (ptrs filled when base != nullptr).
inline size_t layout(char* base, int bc, int64_t n_max, int iters, Workspace* w) {
  const size_t H = (size_t)kChains * iters, C = H * kMaxSlots;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align_up(bytes); return p; };
  Workspace t;
  t.nroots = (int32_t*)take(bc * H * 4);
  t.ncand = (int32_t*)take(bc * H * 4);
  t.hypE = (double*)take(bc * H * kMaxSlots * 9 * 8);
  t.hypP = (double*)take(bc * H * kMaxSlots * 12 * 8);
  t.hypP0 = (double*)take(bc * H * 12 * 8);
  t.sstate = (double*)take((size_t)kStateFields * bc * H * 8);
  t.cand_off = (int32_t*)take(bc * H * 4);
  t.chain_ref = (int32_t*)take(bc * H * 4);
  t.cand_total = (int32_t*)take(SFM_MAX_BATCH * 4);
  t.candE = (double*)take(bc * C * kCandStride * 8);
  t.cntT = (int32_t*)take(bc * C * 4);
  t.cntR = (int32_t*)take(bc * C * 4);
  t.cov = (unsigned long long*)take(bc * C * 8);     // must follow cntR (prune_state)
  t.best_lb = (int32_t*)take(SFM_MAX_BATCH * kBestStride * 4);
  t.skipped = (unsigned long long*)take(8);
  t.score = (int32_t*)take(bc * H * 4);
  t.candF = (_Float16*)take(bc * C * kMfRec * 2);
  // before pack: run_packed re-lays the workspace out with n_max = 0, so every
  // field it uses must sit at an offset independent of n_max
  t.claim = (unsigned long long*)take(kMf2ClaimBytes);
  t.cmap = (int32_t*)take(bc * C * 4);
  t.cmap2 = (int32_t*)take(bc * C * 4);
  t.lead = (int32_t*)take(SFM_MAX_BATCH * 5 * 4);
  t.bnd = (int32_t*)take(SFM_MAX_BATCH * 4 * 4);
  t.pack = (double*)take((size_t)std::max<int64_t>(n_max, 0) * 4 * 8);
  if (w) *w = t;
  return off;
}

// ---------------------------------------------------------------------------
// Correspondence sources.  The kernels read point k of pair b through one of
//   PackedSrc  packed (x, y, x', y') float64 rows (sfm_ransac5_packed)
//   FlowSrc    the dense flow itself: pixel (u, v) of the margin crop, q =
//              K^-1 (u, v, 1), qp = K^-1 (u + fu, v + fv, 1) in float32 rows
//              (k0*x + k1*y) + k2, widened (SFMnet.py:179-263, flow2coord
//              298-318) -- the fused path of SURVEY §8(f) row 2: no staging
//              buffer, 8 bytes of flow per point instead of 32.
// Both yield bit-identical values (k_flow_points uses FlowSrc).
// ---------------------------------------------------------------------------
struct PackedSrc {
  const double* pts;
  int64_t n_stride;
  __device__ __forceinline__ double4 load(int b, int64_t k) const {
    return *reinterpret_cast<const double4*>(pts + ((size_t)b * n_stride + k) * 4);
  }
  PackedSrc shifted(int b0) const { return PackedSrc{pts + (size_t)b0 * n_stride * 4, n_stride}; }
};

struct FlowSrc {
  const float* flow;   // [B][2][H][W]
  const float* Kinv;   // [B][3][3]
  int H, W, wn, margin;
  double inv_wn;       // 1 / wn: k / wn by one multiply and one exact correction (k < 2^31)
  __device__ __forceinline__ double4 load(int b, int64_t k64) const {
    const int k = (int)k64;
    int row = (int)((double)k * inv_wn);
    int col = k - row * wn;
    if (col < 0) { --row; col += wn; } else if (col >= wn) { ++row; col -= wn; }
    const int v = row + margin, u = col + margin;
    const float* Ki = Kinv + b * 9;
    const float* F = flow + (size_t)b * 2 * H * W;
    const float fu = F[(size_t)v * W + u], fv = F[(size_t)H * W + (size_t)v * W + u];
    const float u1 = (float)u, v1 = (float)v;
    const float u2 = u1 + fu, v2 = v1 + fv;
    const float x1 = (Ki[0] * u1 + Ki[1] * v1) + Ki[2];
    const float y1 = (Ki[3] * u1 + Ki[4] * v1) + Ki[5];
    const float x2 = (Ki[0] * u2 + Ki[1] * v2) + Ki[2];
    const float y2 = (Ki[3] * u2 + Ki[4] * v2) + Ki[5];
    return make_double4(x1, y1, x2, y2);
  }
  FlowSrc shifted(int b0) const {
    return FlowSrc{flow + (size_t)b0 * 2 * H * W, Kinv + (size_t)b0 * 9, H, W, wn, margin, inv_wn};
  }
};

// The score kernels' thresholds and switches (make_score_plan).
struct ScoreConsts {
  double thr, t2lo, t2hi;
  float t2lo32, t2hi32;
  int fast32;
  int prune;      // exact bound pruning on (PruneState)
  int interleave; // k_score32 item order: pairs interleaved (1) or one after another (0)
  int ws_batch;   // pairs the workspace was laid out for (locates PruneState)
};

// Exact bound pruning in k_score32 (tuning key score_prune; only when
// num_test == num_ransac_test, SFMnet's case, and no per-hypothesis scores
// are requested).  A candidate's final count is at most its count so far plus
// the points not yet scored for it.  Once that bound is below the largest
// count any candidate of the pair has reached so far, the candidate can be
// neither the winner nor decide it, so its remaining spans are skipped:
//   * best_lb only ever holds partial counts, each <= its candidate's final
//     count <= the winning score.
//   * a pruned candidate's true count is < best_lb.  If it loses its
//     hypothesis's preselection because its partial count is lower, that
//     hypothesis's true best is < best_lb too, so it cannot win.  Any
//     hypothesis or chain reaching the winning score has only unpruned, exact
//     counts (ties included).
//   * cov packs (count, points covered) in one 64-bit atomic, so every read
//     is a consistent snapshot.  Updates only lower count + (T - covered), and
//     only raise best_lb, so stale reads only prune less.
// The winner, its count, E and P are therefore identical with pruning on or
// off.  The per-hypothesis scores of losing hypotheses are lower bounds.
constexpr uint32_t kPrunedFlag = 0xBF800000u;   // record slot 10+13 (ok32) of a pruned candidate: -1.0f

// The pruning state follows cntR in the workspace (layout): cov [B][cmax]
// (count | points covered << 32), best_lb [64], skipped.  The score kernel
// derives it from cntR where it is used: its SGPRs are at the limit, and
// three more live pointers spill the hot loop.
struct PruneState {
  unsigned long long* cov;
  int32_t* best_lb;
  unsigned long long* skipped;
};
__host__ __device__ inline PruneState prune_state(int32_t* cntR, int ws_batch, int cmax) {
  char* p = reinterpret_cast<char*>(cntR) + align_up((size_t)ws_batch * cmax * 4);
  PruneState st;
  st.cov = reinterpret_cast<unsigned long long*>(p);
  p += align_up((size_t)ws_batch * cmax * 8);
  st.best_lb = reinterpret_cast<int32_t*>(p);
  p += align_up((size_t)SFM_MAX_BATCH * kBestStride * 4);
  st.skipped = reinterpret_cast<unsigned long long*>(p);
  return st;
}

// Exact reference evaluation (ComputeError, kernel_functions.cu:232-264).
__device__ __forceinline__ bool inlier_exact(double a, double D, double thr) {
  double e = a / sqrt(D);
  if (e < 0.0) e = -e;
  return e <= thr;
}

// Reference operation order, no contraction (ComputeError).
__device__ __forceinline__ bool inlier_reference(const double* E, double x, double y, double xp, double yp,
                                                 double thr) {
  const double ex0 = (E[0] * x + E[1] * y) + E[2];
  const double ex1 = (E[3] * x + E[4] * y) + E[5];
  const double ex2 = (E[6] * x + E[7] * y) + E[8];
  const double xe0 = (xp * E[0] + yp * E[3]) + E[6];
  const double xe1 = (xp * E[1] + yp * E[4]) + E[7];
  const double a = (xp * ex0 + yp * ex1) + ex2;
  const double D = ((ex0 * ex0 + ex1 * ex1) + xe0 * xe0) + xe1 * xe1;
  return inlier_exact(a, D, thr);
}

// The buffers the scorers read and write: the RANSAC workspace's, or those of
// sfm_score_essentials (no pruning: the trailing fields stay null).
struct ScoreBufs {
  int32_t* cand_total;
  double* candE;
  _Float16* candF;
  int32_t* cntT;
  int32_t* cntR;
  unsigned long long* claim;   // [9] k_score_mf2's range-claim counters and finished-block count
  int32_t* cmap2 = nullptr;    // the one-sided pruning's second keep (k_mf2_keep_map)
  int32_t* cmap = nullptr;     // count-bound pruning (k_mf2_lead / _keep): kept candidates, the
  int32_t* lead = nullptr;     // leader records (their [3] = kept candidates), the evaluations skipped,
  unsigned long long* skipped = nullptr;
  int32_t* bnd = nullptr;      // the launches' span boundaries per pair (k_mf2_split)
};

// The matrix-core scorers' threshold scaling (score_mf.h: mf_params).
struct MfParams {
  int k;                 // a' = 2^k a
  double t_lo, t_hi;     // scaled thresholds thr^2 4^k with the slack factors of score_mf.h
};

// The score-kernel choice and its launch shape, made once per call by
// make_score_plan for the RANSAC driver and sfm_score_essentials alike: the
// split-f16 matrix-core scorers when the threshold and precision allow, else
// the float32 / float64 VALU scorers.
enum class Scorer {
  kMf2Prune,   // k_score_mf2 with count-bound pruning (mf2_pm > 0)
  kMf2,        // k_score_mf2, one launch
  kMf,         // k_score_mf (num_test != num_ransac_test somewhere, or score_mf = 1)
  kLowp,       // k_score<false, Src, prec>: reduced precision, no exactness guards
  kScore32,    // k_score32: float32 pre-decision
  kFma,        // k_score<true>: float64 FMA pre-decision
  kRef         // k_score<false>: the reference order alone
};
struct ScorePlan {
  Scorer scorer;
  int bc, cmax;
  bool same;         // num_test == num_ransac_test for every pair
  int prec;          // kLowp: 32 / 16 (held in T), 33 / 17 (the literal template form)
  ScoreConsts kc;
  MfParams mp;
  double guard_g;    // k_cand / k_fill_cands: the float64 guard's G (0: no fast path)
  bool fast32;       // k_cand / k_fill_cands: write the float32 constants
  int cus;           // k_score_mf2's grid; k_score_mf's is cus * score_mf_blocks_per_cu
  int grid;          // the VALU scorers' persistent grid
  int mf2_pm;        // kMf2Prune: the first launch's share of each pair's spans, per mille
  bool one_cnt;      // k_select reads cntT for both counts (k_score_mf2 publishes one array)
};
// (the functions the units call across each other stay out of the library's
// exported symbols)
#pragma GCC visibility push(hidden)
// want_scores: per-hypothesis scores are requested (pruning leaves the losers'
// as lower bounds, so it is off); allow_prune: the buffers hold pruning state.
ScorePlan make_score_plan(double thr, const PairParams& pp, int bc, int cmax, int ws_batch, bool want_scores,
                          bool allow_prune);
// Launches the plan's scorer (ransac_score.hip; instantiated for PackedSrc and
// FlowSrc).  ref_job: a reference-half job the first one-sided launch may
// write (*rode set when it did).
template <class Src>
void launch_score(const Src& src, const PairParams& pp, const ScoreBufs& w, const ScorePlan& plan, hipStream_t s,
                  const RefJob* ref_job = nullptr, bool* rode = nullptr);

// One launcher per profiled phase (ransac_solve.hip; launch_solve instantiated
// for PackedSrc and FlowSrc).
template <class Src>
void launch_solve(const Src& src, const PairParams& pp, int bc, int H, uint64_t seed, int cheir, const Workspace& w,
                  hipStream_t s);
void launch_chain(int bc, int H, int iters, int cheir, double thr, const ScorePlan& plan, const Workspace& w,
                  bool first_chunk, hipStream_t s);
void launch_select(int bc, int H, int cheir, const ScorePlan& plan, const Workspace& w, int32_t* score_out,
                   double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out, hipStream_t s);
// candidate records of given essential matrices (sfm_score_essentials), as k_cand writes them
void launch_fill_cands(const double* E, int batch, int ncand, double thr, const ScorePlan& plan, const ScoreBufs& w,
                       hipStream_t s);
#pragma GCC visibility pop

}  // namespace sfm
