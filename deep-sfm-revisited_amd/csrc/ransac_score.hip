// RANSAC phase 3, scoring: every score kernel (score_valu.h, score_mf.h,
// score_mf2.h) and the two things the drivers use -- make_score_plan picks the
// scorer and its launch shape from the threshold, the pairs and the tuning;
// launch_score launches it for a correspondence source.
#include "score_mf2.h"

namespace sfm {

// The rider's launch parameters for a job, or false when the shape is outside
// its fast path (the caller then writes the reference half with
// sfm_plane_sweep_ref_planes): rows of even length whose periods start
// 16-byte aligned, 32-bit slab offsets, piece and run counts below 2^31.
template <int kFmt>
static bool make_rider(const RefJob& j, long long max_runs, RefRider<kFmt>* r) {
  const long long hw = (long long)j.h * j.w, L = j.nlabel;
  const long long esz = kFmt == 1 ? 4 : 2;
  if (hw < 4 || hw % 2 != 0 || (hw % 4 != 0 && L % 2 != 0)) return false;
  const long long P = hw % 4 == 0 ? hw : 2 * hw, np = L * hw / P;
  const long long slab_bytes = L * hw * esz;
  if (slab_bytes >= (1ll << 32) || (uintptr_t)j.ref % 8 != 0 || (uintptr_t)j.cost % 16 != 0) return false;
  const long long rows = (long long)j.batch * j.channels;
  const long long cpp = (P + 255) / 256, gpp = (np + kRiderStores - 1) / kRiderStores;
  const long long T = rows * cpp * gpp;
  if (T >= (1ll << 31) || max_runs >= (1ll << 31)) return false;
  r->ref = j.ref;
  r->cost = j.cost;
  r->T = (unsigned)T;
  r->C = (unsigned)j.channels;
  r->hw = (unsigned)hw;
  r->P = (unsigned)P;
  r->cpp = (unsigned)cpp;
  r->np = (unsigned)np;
  r->gpp = (unsigned)gpp;
  r->slab_bytes = (unsigned)slab_bytes;
  r->mcpp = make_magic((unsigned)cpp);
  r->mgpp = make_magic((unsigned)gpp);
  r->mC = make_magic((unsigned)j.channels);
  return true;
}

// score_precision with the low-precision form folded in: 64, 32 / 16 (held in
// T), 33 / 17 (the literal template form, score_lowp_template)
static int lowp_prec() {
  const int p = tuning().score_precision;
  return (p != 64 && tuning().score_lowp_template) ? p + 1 : p;
}

ScorePlan make_score_plan(double thr, const PairParams& pp, int bc, int cmax, int ws_batch, bool want_scores,
                          bool allow_prune) {
  ScorePlan p{};
  p.bc = bc;
  p.cmax = cmax;
  p.prec = lowp_prec();
  // reduced precision: no exactness guards; the plain ComputeError<T> kernel
  const bool fast = p.prec == 64 && thr >= 0x1p-40 && thr < 1.0;
  p.guard_g = fast ? 0x1p24 * (11.0 + 11.0 / thr) : 0.0;
  p.fast32 = fast && thr >= 0x1p-20 && tuning().score_fp32;
  ScoreConsts& kc = p.kc;
  kc.thr = thr;
  kc.t2lo = (thr * thr) * (1.0 - 0x1p-22);
  kc.t2hi = (thr * thr) * (1.0 + 0x1p-22);
  // float32 thresholds with directed slack (see fp32_constants)
  kc.t2lo32 = (float)((thr * thr) * (1.0 - 0x1p-6 - 0x1p-19));
  kc.t2hi32 = (float)((thr * thr) * (1.0 + 0x1p-7) / (1.0 - 0x1p-7) * (1.0 + 0x1p-19));
  kc.fast32 = p.fast32 ? 1 : 0;
  kc.ws_batch = ws_batch;
  kc.interleave = tuning().score_interleave;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  p.cus = std::max(1, cus);
  p.grid = p.cus * tuning().score_blocks_per_cu;
  p.same = true;
  int min_spans = INT32_MAX;
  for (int b = 0; b < bc; ++b) {
    p.same = p.same && pp.test[b] == pp.rtest[b];
    min_spans = std::min(min_spans, mf2_spans(std::max(pp.test[b], pp.rtest[b])));
  }
  const bool use_mf = p.fast32 && tuning().score_mf && mf_params(thr, &p.mp);
  const bool mf2 = use_mf && p.same && tuning().score_mf == 2;
  // exact bound pruning: SFMnet's num_test == num_ransac_test, no per-hypothesis scores requested
  const bool may_prune = allow_prune && p.same && !want_scores;
  kc.prune = (p.fast32 && !use_mf && may_prune && tuning().score_prune) ? 1 : 0;
  // count-bound pruning in k_score_mf2 (k_mf2_lead / _keep): same condition, and
  // every pair long enough that the second launch has spans to skip
  p.mf2_pm = (mf2 && may_prune && min_spans >= kMf2PruneMinSpans) ? tuning().score_mf_prune : 0;
  p.one_cnt = mf2;
  const bool lowp = p.prec == 32 || p.prec == 16 || p.prec == 33 || p.prec == 17;
  p.scorer = mf2 ? (p.mf2_pm > 0 ? Scorer::kMf2Prune : Scorer::kMf2)
             : use_mf ? Scorer::kMf
             : lowp ? Scorer::kLowp
             : p.fast32 ? Scorer::kScore32
             : fast ? Scorer::kFma
                    : Scorer::kRef;
  return p;
}

// One k_score_mf2 launch: the candidates it runs over and its spans of each pair.
struct Mf2Launch {
  const int32_t* cand_total;   // candidates per pair (through cmap: of the map)
  const int32_t* cmap;         // kMapped: the compacted candidates' index map
  int sp_lo, sp_hi;            // the spans, in per mille of the pair's, or
  const int32_t* bnd;          // from boundary row `phase` to the next (k_mf2_split)
  int phase;
  int chunk;                   // smallest unit range a block claims
};
static Mf2Launch spans_pm(const int32_t* cand_total, int lo, int hi, int chunk, const int32_t* cmap = nullptr) {
  return Mf2Launch{cand_total, cmap, lo, hi, nullptr, 0, chunk};
}
static Mf2Launch spans_bnd(const int32_t* cand_total, const int32_t* bnd, int phase, int chunk,
                           const int32_t* cmap = nullptr) {
  return Mf2Launch{cand_total, cmap, 0, 0, bnd, phase, chunk};
}

template <class Src, bool kMapped, bool kUpper, class... Rider>
static void launch_mf2(const Src& src, const PairParams& pp, const ScoreBufs& w, const ScorePlan& plan, hipStream_t s,
                       const Mf2Launch& a, const Rider&... rider) {
  hipLaunchKernelGGL((k_score_mf2<Src, kMapped, kUpper, Rider...>), dim3(plan.cus), dim3(mf2_waves<kUpper>() * 64), 0,
                     s, src, pp, plan.bc, plan.cmax, a.cand_total, w.candE, w.candF, w.cntT, plan.kc, w.claim, a.cmap,
                     a.sp_lo, a.sp_hi, a.bnd, a.phase, a.chunk, rider...);
}

// Launch `a` one-sided with the job's store rider (kFmt 1: a float32 volume, 2:
// bfloat16), when there is a job of that format inside the rider's fast path.
template <int kFmt, class Src>
static bool try_ride(const Src& src, const PairParams& pp, const ScoreBufs& w, const ScorePlan& plan, hipStream_t s,
                     const Mf2Launch& a, const RefJob* job, long long max_runs) {
  RefRider<kFmt> r;
  if (!job || !tuning().score_ref_rider || job->dtype != kFmt - 1 || !make_rider(*job, max_runs, &r)) return false;
  launch_mf2<Src, false, true>(src, pp, w, plan, s, a, r);
  return true;
}

// Count-bound pruning:
//   A every candidate on the first mf2_pm per mille of each pair's spans;
//   k_mf2_split picks the pair's pruning point sB from its inlier ratio;
//   B every candidate up to sB; k_mf2_lead + k_mf2_keep;
//   C the kept candidates on the rest.
// kUpper, the one-sided pruning (round 6): A, B and C count the points not
// certainly outliers (upper bounds), k_mf2_split also names the leader (the
// first max), k_mf2_lead counts it exactly over every point (lb), k_mf2_keep
// keeps the candidates whose upper bound (count + points left) reaches lb, and
// after C
//   k_mf2_keep_map keeps those whose full upper count still reaches lb;
//   their counts are zeroed, then counted exactly: float64 (k_mf2_exact) for
//   pairs with at most score_mf_exact_max of them, the two-sided matrix-core
//   pass through the index map for the others (lead row 4).
// With a reference-half job inside the rider's fast path, the one-sided A also
// writes that half (the store rider of score_mf2.h).
template <class Src, bool kUpper>
static void launch_mf2_pruned(const Src& src, const PairParams& pp, const ScoreBufs& w, const ScorePlan& plan,
                              hipStream_t s, const RefJob* ref_job, bool* rode) {
  const int bc = plan.bc, cmax = plan.cmax;
  const int ch = tuning().score_mf_chunk;
  const int ch2 = tuning().score_mf_chunk2 ? tuning().score_mf_chunk2 : ch;
  const int32_t* kept = w.lead + 3 * SFM_MAX_BATCH;
  const Mf2Launch A = spans_pm(w.cand_total, 0, plan.mf2_pm, ch);
  bool ride = false;
  if constexpr (kUpper) {
    long long max_runs = 0;
    for (int b = 0; b < bc; ++b)
      max_runs += (long long)mf2_spans(std::max(pp.test[b], pp.rtest[b])) * ((cmax + kKC - 1) / kKC);
    ride = try_ride<1>(src, pp, w, plan, s, A, ref_job, max_runs) ||
           try_ride<2>(src, pp, w, plan, s, A, ref_job, max_runs);
    if (ride) *rode = true;
  }
  if (!ride) launch_mf2<Src, false, kUpper>(src, pp, w, plan, s, A);
  hipLaunchKernelGGL(k_mf2_split, dim3(bc), dim3(1024), 0, s, pp, cmax, plan.mf2_pm, tuning().score_mf_prune_margin,
                     w.cand_total, w.cntT, w.bnd, kUpper ? w.lead : nullptr);
  launch_mf2<Src, false, kUpper>(src, pp, w, plan, s, spans_bnd(w.cand_total, w.bnd, 1, ch));
  hipLaunchKernelGGL(k_mf2_lead<Src>, dim3(kUpper ? 4 * kLeadBlocks : kLeadBlocks, bc), dim3(1024), 0, s, src, pp,
                     cmax, w.bnd, w.cand_total, w.candE, w.cntT, plan.kc, w.lead, kUpper ? 2 : 0);
  hipLaunchKernelGGL(k_mf2_keep, dim3((cmax + 1023) / 1024, bc), dim3(1024), 0, s, pp, cmax, w.bnd, w.cand_total,
                     w.cntT, w.lead, w.cmap, w.skipped, 0);
  launch_mf2<Src, true, kUpper>(src, pp, w, plan, s, spans_bnd(kept, w.bnd, 2, ch2, w.cmap));
  if constexpr (kUpper) {
    const int exact_max = tuning().score_mf_exact_max;
    hipLaunchKernelGGL(k_mf2_keep_map, dim3(bc), dim3(1024), 0, s, cmax, w.cntT, w.lead, w.cmap, w.cmap2, exact_max);
    hipLaunchKernelGGL(k_mf2_zero_kept, dim3((cmax + 255) / 256, bc), dim3(256), 0, s, cmax, w.lead, w.cmap2, w.cntT);
    hipLaunchKernelGGL(k_mf2_exact<Src>, dim3(kExactBlocks, bc), dim3(kExactThreads), 0, s, src, pp, cmax, w.lead,
                       w.cmap2, w.candE, plan.kc, w.cntT, exact_max);
    launch_mf2<Src, true, false>(src, pp, w, plan, s, spans_pm(w.lead + 4 * SFM_MAX_BATCH, 0, 1000, ch2, w.cmap2));
  }
}

template <bool FAST, int PREC, class Src>
static void launch_valu(const Src& src, const PairParams& pp, const ScoreBufs& w, const ScorePlan& plan,
                        hipStream_t s, const char* name) {
  hipLaunchKernelGGL((k_score<FAST, Src, PREC>), dim3(plan.grid), dim3(kScoreThreads), 0, s, src, pp, plan.bc,
                     plan.cmax, w.cand_total, w.candE, w.cntT, w.cntR, plan.kc);
  set_last_scorer(name);
}

template <class Src>
void launch_score(const Src& src, const PairParams& pp, const ScoreBufs& w, const ScorePlan& plan, hipStream_t s,
                  const RefJob* ref_job, bool* rode) {
  const int bc = plan.bc, cmax = plan.cmax;
  if (plan.scorer <= Scorer::kMf)
    hipLaunchKernelGGL(k_mf_cands, dim3((cmax + 255) / 256, bc), dim3(256), 0, s, cmax, w.cand_total, w.candE, w.candF,
                       plan.mp, w.claim, plan.mf2_pm > 0 ? w.lead : nullptr);
  const dim3 gmf(plan.cus * tuning().score_mf_blocks_per_cu);
  switch (plan.scorer) {
    case Scorer::kMf2Prune:
      if (tuning().score_mf_prune_upper) launch_mf2_pruned<Src, true>(src, pp, w, plan, s, ref_job, rode);
      else launch_mf2_pruned<Src, false>(src, pp, w, plan, s, ref_job, rode);
      set_last_scorer("k_score_mf2+prune");
      break;
    case Scorer::kMf2:
      launch_mf2<Src, false, false>(src, pp, w, plan, s, spans_pm(w.cand_total, 0, 1000, tuning().score_mf_chunk));
      set_last_scorer("k_score_mf2");
      break;
    case Scorer::kMf:
      if (plan.same)
        hipLaunchKernelGGL((k_score_mf<Src, true>), gmf, dim3(kMfWaves * 64), 0, s, src, pp, bc, cmax, w.cand_total,
                           w.candE, w.candF, w.cntT, w.cntR, plan.kc);
      else
        hipLaunchKernelGGL((k_score_mf<Src, false>), gmf, dim3(kMfWaves * 64), 0, s, src, pp, bc, cmax, w.cand_total,
                           w.candE, w.candF, w.cntT, w.cntR, plan.kc);
      set_last_scorer("k_score_mf");
      break;
    case Scorer::kLowp:
      if (plan.prec == 32) launch_valu<false, 32>(src, pp, w, plan, s, "k_score<32>");
      else if (plan.prec == 16) launch_valu<false, 16>(src, pp, w, plan, s, "k_score<16>");
      else if (plan.prec == 33) launch_valu<false, 33>(src, pp, w, plan, s, "k_score<33>");
      else launch_valu<false, 17>(src, pp, w, plan, s, "k_score<17>");
      break;
    case Scorer::kScore32:
      hipLaunchKernelGGL(k_score32<Src>, dim3(plan.grid), dim3(kScoreThreads), 0, s, src, pp, bc, cmax, w.cand_total,
                         w.candE, w.cntT, w.cntR, plan.kc);
      set_last_scorer(plan.kc.prune ? "k_score32+prune" : "k_score32");
      break;
    case Scorer::kFma:
      launch_valu<true, 64>(src, pp, w, plan, s, "k_score<fma>");
      break;
    case Scorer::kRef:
      launch_valu<false, 64>(src, pp, w, plan, s, "k_score<ref>");
      break;
  }
}

template void launch_score<PackedSrc>(const PackedSrc&, const PairParams&, const ScoreBufs&, const ScorePlan&,
                                      hipStream_t, const RefJob*, bool*);
template void launch_score<FlowSrc>(const FlowSrc&, const PairParams&, const ScoreBufs&, const ScorePlan&,
                                    hipStream_t, const RefJob*, bool*);

}  // namespace sfm
