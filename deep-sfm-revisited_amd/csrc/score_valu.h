// Phase 3 of the RANSAC on the vector ALUs (included by ransac_score.hip):
//   k_score    persistent, tiles of 32 candidates x 8192 points: the float64
//              FMA pre-decision behind a proven guard (k_score<true>), the
//              reference order alone (k_score<false>), or the reduced-precision
//              forms (k_score<false, Src, 32 / 16 / 33 / 17>)
//   k_score32  the float32 pre-decision with a float64 re-test of the
//              undecided evaluations, and exact bound pruning (PruneState)
// The error bounds behind the guards stand with the constants that
// ransac_solve.hip writes into the candidate records (guard_constant,
// fp32_constants).  inlier_f64v, lane_prefix and wave_sync also serve the
// matrix-core scorers (score_mf.h, score_mf2.h).
#pragma once
#include "ransac_common.h"

namespace sfm {

// mm2 = M^4 for the fast-path guard (NaN for non-finite / huge coordinates)
__device__ __forceinline__ double point_scale(double x, double y, double xp, double yp) {
  double M = fmax(fmax(fabs(x), fabs(y)), fmax(fabs(xp), fabs(yp)));
  M = fmax(M, 1.0);
  if (!(M <= 0x1p100)) return __builtin_nan("");
  const double M2 = M * M;
  return M2 * M2;
}

// Wave-uniform value copied into a VGPR: one VALU op may read only one SGPR,
// so the FMA-chain addends are broadcast once per candidate instead of being
// re-materialised for every point.
__device__ __forceinline__ double to_vgpr(double s) {
  double v;
  asm("v_mov_b64 %0, %1" : "=v"(v) : "s"(s));
  return v;
}

struct Addends { double e2, e5, e8, e6, e7; };

// UNITM: every point of the chunk has M = 1 (mm2 = 1), so the guard is D >= Kg
template <bool FAST, bool UNITM>
__device__ __forceinline__ bool inlier_test(const double* E, const Addends& ad, double Kg, double x, double y,
                                            double xp, double yp, double mm2, const ScoreConsts& k) {
  if (!FAST) return inlier_reference(E, x, y, xp, yp, k.thr);
  const double ex0 = fma(E[0], x, fma(E[1], y, ad.e2));
  const double ex1 = fma(E[3], x, fma(E[4], y, ad.e5));
  const double ex2 = fma(E[6], x, fma(E[7], y, ad.e8));
  const double xe0 = fma(xp, E[0], fma(yp, E[3], ad.e6));
  const double xe1 = fma(xp, E[1], fma(yp, E[4], ad.e7));
  const double a = fma(xp, ex0, fma(yp, ex1, ex2));
  const double D = fma(xe1, xe1, fma(xe0, xe0, fma(ex1, ex1, ex0 * ex0)));
  const double lhs = a * a;
  const bool g = UNITM ? (D >= Kg) : (D >= Kg * mm2);
  const bool fin = g && (lhs < k.t2lo * D);
  const bool fout = g && (lhs > k.t2hi * D);
  bool in = fin;
  if (!(fin || fout)) in = inlier_reference(E, x, y, xp, yp, k.thr);
  return in;
}

// Reduced-precision scoring (tuning key score_precision; BASELINE C5's fp32 vs
// fp16 inlier-set sweep).  Two forms; the reference itself only ever
// instantiates ComputeError<double> (kernel_functions.cu:193, 210), so neither
// has a reference output and both are pinned only to this build's oracle
// restatement (parity unpinned against the reference):
//   * "held in T" (score_precision 32 / 16, inlier_lowp below): this build's
//     own variant, NOT the reference's template.  E, q, qp and every
//     operation of ComputeError's expression tree in T (RNE, source order, no
//     contraction), sqrt and division correctly rounded in T.  E is first
//     scaled by a power of two (exact; the error is invariant to the scale of
//     E).  Inputs reach T through float32 (float64 -> float32 -> T).  For T =
//     half the sqrt and the division run in float32 and round once to half:
//     float32 carries 24 >= 2*11 + 2 bits, so that double rounding is exact.
//     oracle/ransac5_oracle.cpp:is_inlier_lp restates it.
//   * "template" (score_lowp_template 1, inlier_lowp_tpl): what a literal
//     ComputeError<T> instantiation computes with the reference's Ematrix =
//     double[3][3] (common.h:26).  q, qp are T; each E[k][l] * q[l] is a
//     double product (T widened exactly), `sum += ...` adds in double and
//     rounds the sum to T; xEx, D, sqrt and the division are T arithmetic.
//     No scaling of E.  oracle/ransac5_oracle.cpp:is_inlier_lp_tpl restates it.
// Both end with the call site's `error <= c_inlier_threshold` against the
// float64 threshold (kernel_functions.cu:193-194).
template <int PREC>
struct LowP { using T = float; };
template <>
struct LowP<16> { using T = _Float16; };
template <>
struct LowP<17> { using T = _Float16; };

// float64 -> binary16, rounded once (ties to even; subnormals; overflow to
// inf): the conversion of `T q_test[3] = {qs[..], ...}` for T = half.  The
// quantum arithmetic is exact in float64 (oracle: h16d).
__device__ __forceinline__ _Float16 h16_of_double(double v) {
  if (!(fabs(v) < 65520.0)) return (_Float16)(float)v;       // inf / nan / past max + half an ulp
  const double a = fabs(v);
  double q;
  if (a < 0x1p-14) {
    q = 0x1p-24;
  } else {
    int e;
    (void)frexp(a, &e);
    q = ldexp(1.0, e - 1 - 10);
  }
  return (_Float16)(float)copysign(rint(a / q) * q, v);      // representable: the conversions are exact
}
__device__ __forceinline__ float lowp_of_double(double v, float) { return (float)v; }
__device__ __forceinline__ _Float16 lowp_of_double(double v, _Float16) { return h16_of_double(v); }

// the literal template form (PREC 33 = float, 17 = half; see above)
template <int PREC>
__device__ __forceinline__ bool inlier_lowp_tpl(const double* E, double xd, double yd, double xpd, double ypd,
                                                double thr) {
  using T = typename LowP<PREC>::T;
  const T q[3] = {lowp_of_double(xd, T()), lowp_of_double(yd, T()), (T)1.0f};
  const T qp[3] = {lowp_of_double(xpd, T()), lowp_of_double(ypd, T()), (T)1.0f};
  T Ex[3], xE[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    T sum = (T)0.0f;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const double p = E[3 * k + l] * (double)q[l];
      const double t = (double)sum + p;
      sum = lowp_of_double(t, T());
    }
    Ex[k] = sum;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    T sum = (T)0.0f;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const double p = (double)qp[l] * E[3 * l + k];
      const double t = (double)sum + p;
      sum = lowp_of_double(t, T());
    }
    xE[k] = sum;
  }
  T xEx = (T)0.0f, m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m = qp[k] * Ex[k];
    xEx = xEx + m;
  }
  T D, m0, m1;
  m0 = Ex[0] * Ex[0]; m1 = Ex[1] * Ex[1]; D = m0 + m1;
  m0 = xE[0] * xE[0]; D = D + m0;
  m0 = xE[1] * xE[1]; D = D + m0;
  const T d = (T)sqrtf((float)D);
  T err = (T)((float)xEx / (float)d);
  if (err < (T)0.0f) err = -err;
  return (double)(float)err <= thr;
}

template <int PREC>
__device__ __forceinline__ bool inlier_lowp(const double* E, double xd, double yd, double xpd, double ypd,
                                            double thr) {
  using T = typename LowP<PREC>::T;
  // E scaled by a power of two to max |E_ij| in [0.5, 1): exact in float64,
  // and the Sampson error is invariant to the scale of E; without it a
  // five-point E of small norm underflows in half
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) m = fmax(m, fabs(E[i]));
  int ex = 0;
  if (m > 0.0 && m < 0x1p1000) (void)frexp(m, &ex);
  T e[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) e[i] = (T)(float)ldexp(E[i], -ex);
  const T x = (T)(float)xd, y = (T)(float)yd, xp = (T)(float)xpd, yp = (T)(float)ypd;
  // every intermediate is a named T: assignment rounds each operation to T
  T m0, m1, s;
  m0 = e[0] * x; m1 = e[1] * y; s = m0 + m1; const T ex0 = s + e[2];
  m0 = e[3] * x; m1 = e[4] * y; s = m0 + m1; const T ex1 = s + e[5];
  m0 = e[6] * x; m1 = e[7] * y; s = m0 + m1; const T ex2 = s + e[8];
  m0 = xp * e[0]; m1 = yp * e[3]; s = m0 + m1; const T xe0 = s + e[6];
  m0 = xp * e[1]; m1 = yp * e[4]; s = m0 + m1; const T xe1 = s + e[7];
  m0 = xp * ex0; m1 = yp * ex1; s = m0 + m1; const T a = s + ex2;
  T D;
  m0 = ex0 * ex0; m1 = ex1 * ex1; D = m0 + m1;
  m0 = xe0 * xe0; D = D + m0;
  m0 = xe1 * xe1; D = D + m0;
  const T d = (T)sqrtf((float)D);
  T err = (T)((float)a / (float)d);
  if (err < (T)0.0f) err = -err;
  return (double)(float)err <= thr;
}

// Level-3 test (reference order), kept as a named call site for the drain.
__device__ __forceinline__
bool inlier_reference_call(const double* E, double x, double y, double xp, double yp,
                                                   double thr) {
  return inlier_reference(E, x, y, xp, yp, thr);
}

// One chunk (kPPL points per lane) against the tile's nc candidates.  One
// ballot per (candidate, point); the num_test / num_ransac_test prefixes are
// applied as precomputed wave masks (SAME: both prefixes equal, one count).
template <bool FAST, bool UNITM, bool SAME, int PREC>
__device__ __forceinline__ void score_chunk(const double* __restrict__ CE, int nc, const double (&x)[kPPL],
                                            const double (&y)[kPPL], const double (&xp)[kPPL],
                                            const double (&yp)[kPPL], const double (&mm2)[kPPL],
                                            const uint64_t (&mT)[kPPL], const uint64_t (&mR)[kPPL],
                                            const ScoreConsts& kc, int lane, int32_t (*cnt)[2]) {
  for (int c = 0; c < nc; ++c) {
    double E[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = CE[(size_t)c * kCandStride + e];
    const double Kg = CE[(size_t)c * kCandStride + 9];
    Addends ad;
    if (FAST) ad = Addends{to_vgpr(E[2]), to_vgpr(E[5]), to_vgpr(E[8]), to_vgpr(E[6]), to_vgpr(E[7])};
    int sT = 0, sR = 0;
#pragma unroll
    for (int k = 0; k < kPPL; ++k) {
      const bool in = PREC == 64 ? inlier_test<FAST, UNITM>(E, ad, Kg, x[k], y[k], xp[k], yp[k], mm2[k], kc)
                      : (PREC & 1) ? inlier_lowp_tpl<PREC>(E, x[k], y[k], xp[k], yp[k], kc.thr)
                                   : inlier_lowp<PREC>(E, x[k], y[k], xp[k], yp[k], kc.thr);
      const uint64_t m = __ballot(in);
      sT += __popcll(m & mT[k]);
      if (!SAME) sR += __popcll(m & mR[k]);
    }
    if (SAME) sR = sT;
    if (lane == 0) {
      cnt[c][0] += sT;
      cnt[c][1] += sR;
    }
  }
}

template <bool FAST, class Src, int PREC = 64>
__global__ __launch_bounds__(kScoreThreads) void k_score(const Src src, PairParams pp, int batch, int cmax,
                                                         const int32_t* __restrict__ cand_total,
                                                         const double* __restrict__ candE,
                                                         int32_t* __restrict__ cntT, int32_t* __restrict__ cntR,
                                                         ScoreConsts kc) {
  __shared__ int32_t s_cnt[kScoreThreads / 64][kKC][2];
  __shared__ int32_t s_items[SFM_MAX_BATCH + 1];
  __shared__ int32_t s_tiles[SFM_MAX_BATCH];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    int acc = 0;
    for (int b = 0; b < batch; ++b) {
      const int tiles = (cand_total[b] + kKC - 1) / kKC;
      s_tiles[b] = tiles;
      s_items[b] = acc;
      acc += tiles * pp.splits[b];
    }
    s_items[batch] = acc;
  }
  for (int i = tid; i < (kScoreThreads / 64) * kKC * 2; i += kScoreThreads) (&s_cnt[0][0][0])[i] = 0;
  __syncthreads();
  const int total = s_items[batch];
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    int b = 0;
    while (item >= s_items[b + 1]) ++b;
    const int local = item - s_items[b];
    const int tiles = s_tiles[b];
    const int split = local / tiles, tile = local - split * tiles;
    const int ctot = cand_total[b];
    const int c0 = tile * kKC;
    const int nc = min(kKC, ctot - c0);
    const int T = pp.test[b], R = pp.rtest[b];
    const int M = max(T, R);
    const int p0 = split * kPtsPerItem;
    const int p1 = min(M, p0 + kPtsPerItem);
    const double* CE = candE + ((size_t)b * cmax + c0) * kCandStride;
    for (int cb = p0; cb < p1; cb += kChunk) {
      double x[kPPL], y[kPPL], xp[kPPL], yp[kPPL], mm2[kPPL];
      uint64_t mT[kPPL], mR[kPPL];
      bool unit = true;
#pragma unroll
      for (int k = 0; k < kPPL; ++k) {
        const int p = cb + k * kScoreThreads + tid;
        const bool ok = p < p1;
        const double4 v = src.load(b, ok ? p : p0);
        x[k] = v.x; y[k] = v.y; xp[k] = v.z; yp[k] = v.w;
        mm2[k] = point_scale(v.x, v.y, v.z, v.w);
        unit = unit && (mm2[k] == 1.0);
        mT[k] = __ballot(ok && p < T);
        mR[k] = __ballot(ok && p < R);
      }
      const bool all_unit = __all(unit);
      if (T == R) {
        if (all_unit) score_chunk<FAST, true, true, PREC>(CE, nc, x, y, xp, yp, mm2, mT, mR, kc, lane, s_cnt[wv]);
        else score_chunk<FAST, false, true, PREC>(CE, nc, x, y, xp, yp, mm2, mT, mR, kc, lane, s_cnt[wv]);
      } else {
        if (all_unit) score_chunk<FAST, true, false, PREC>(CE, nc, x, y, xp, yp, mm2, mT, mR, kc, lane, s_cnt[wv]);
        else score_chunk<FAST, false, false, PREC>(CE, nc, x, y, xp, yp, mm2, mT, mR, kc, lane, s_cnt[wv]);
      }
    }
    __syncthreads();
    if (tid < nc * 2) {
      const int c = tid >> 1, which = tid & 1;
      int s = 0;
#pragma unroll
      for (int w = 0; w < kScoreThreads / 64; ++w) { s += s_cnt[w][c][which]; s_cnt[w][c][which] = 0; }
      if (s) atomicAdd((which ? cntR : cntT) + (size_t)b * cmax + c0 + c, s);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Phase 3b: scoring with the float32 pre-decision (fp32_constants).
// Only float32 copies of the points stay in registers.  (Plain v_fma_f32
// issues at twice the fp64 rate on gfx950; packed v_pk_fma_f32 measured no
// faster.)  The kernel sits at the measured VALU issue ceiling
// (git-history scripts/probe_vgpr_bank.hip: ~1.15-1.3 ns per wave-FMA per SIMD at 4-8
// waves), so its cost is its VALU count: 21 per evaluation in the common
// path.  Undecided evaluations and lanes with a coordinate beyond 2^12 are
// queued and re-tested in float64.
// ---------------------------------------------------------------------------

#ifdef SFM_SCORE_STATS
// experiment builds only (git-history scripts/score_experiment.py): (candidate, point
// slot) wave iterations, those with an undecided lane, undecided evaluations
__device__ unsigned long long g_score_stats[3];
extern "C" int sfm_experiment_score_stats(unsigned long long* out3) {
  return hipMemcpyFromSymbol(out3, HIP_SYMBOL(g_score_stats), 24) == hipSuccess ? 0 : 2;
}
#endif

// float64 decision of one (reloaded) point; guard per point (any scale)
__device__ __forceinline__ bool inlier_f64v(const double* __restrict__ Ec, const double4 v, const ScoreConsts& kc) {
  double E[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = Ec[e];
  const double x = v.x, y = v.y, xp = v.z, yp = v.w;
  const double ex0 = fma(E[0], x, fma(E[1], y, E[2]));
  const double ex1 = fma(E[3], x, fma(E[4], y, E[5]));
  const double ex2 = fma(E[6], x, fma(E[7], y, E[8]));
  const double xe0 = fma(xp, E[0], fma(yp, E[3], E[6]));
  const double xe1 = fma(xp, E[1], fma(yp, E[4], E[7]));
  const double a = fma(xp, ex0, fma(yp, ex1, ex2));
  const double D = fma(xe1, xe1, fma(xe0, xe0, fma(ex1, ex1, ex0 * ex0)));
  const double lhs = a * a;
  const bool g = D >= Ec[9] * point_scale(x, y, xp, yp);
  const bool fin = g && (lhs < kc.t2lo * D);
  const bool fout = g && (lhs > kc.t2hi * D);
  if (fin || fout) return fin;
  return inlier_reference_call(E, x, y, xp, yp, kc.thr);
}

// Float32 pass.  Every decision is a wave mask straight out of one compare
// (inlier: din < -eps1, outlier: dout > eps2; all finite here since the
// lane's coordinates are within 2^12 and the candidate passed ok32), so the
// bookkeeping is scalar: counts by popcount, undecided = ~(in | out) per
// point.  Undecided points are queued and re-tested in float64.

// Lanes [0, n) of a wave (n may lie outside [0, 64]).
__device__ __forceinline__ uint64_t lane_prefix(int n) {
  return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
}

constexpr int kQueue = 1024;        // undecided (candidate, point) entries per wave (LDS)
static_assert(kQueue >= 64 * kPPL32, "the queue takes one candidate's undecided points past its low mark");

// Append the wave's undecided lanes (mask und) of one point slot to the queue.
__device__ __forceinline__ void enqueue_undecided(uint64_t und, int c, int p, int lane, uint32_t* q, int& qn) {
#ifdef SFM_SCORE_STATS
  if (lane == 0) {
    atomicAdd(&g_score_stats[0], 1ull);
    if (und) atomicAdd(&g_score_stats[1], 1ull);
    atomicAdd(&g_score_stats[2], (unsigned long long)__popcll(und));
  }
#endif
  if (!und) return;                                     // wave-uniform
  if ((und >> lane) & 1ull) {
    const int pos = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(und >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)und, 0));
    q[pos] = ((uint32_t)c << 24) | (uint32_t)p;
  }
  qn += __popcll(und);
}

// One float32 pass of a wave over candidates [c, nc) of its chunk (lane l
// holds points cb + 64k + l).  Returns the first candidate not processed: nc,
// or one met with the queue past its low mark (the caller drains the queue,
// reloads the chunk and resumes there).  The float64 test stays out of this
// loop so that its registers stay out of the hot loop's footprint.
//   MASKED: the chunk crosses the num_test (nT) or num_ransac_test (nR)
//   prefix, counted from the chunk base; SAME: both prefixes are equal.
//   GEN: some lane has M != 1 or is bad; otherwise eps are the records'
//   precomputed M = 1 values.
template <bool SAME, bool MASKED, bool GEN>
__device__ __forceinline__ int score32_pass(const double* __restrict__ CE, int c, int nc, int pl, int nT, int nR,
                                            const float (&x)[kPPL32], const float (&y)[kPPL32],
                                            const float (&xp)[kPPL32], const float (&yp)[kPPL32], float M2,
                                            uint64_t bad, const ScoreConsts& kc, int lane, int32_t (*cnt)[2],
                                            uint32_t* q, int& qn) {
  const float nt2lo = -kc.t2lo32, nt2hi = -kc.t2hi32;
  const float M4 = M2 * M2;
  for (; c < nc; ++c) {
    if (qn > kQueue - 64 * kPPL32) break;               // drain first
    const float* F = reinterpret_cast<const float*>(CE + (size_t)c * kCandStride + 10);
    int sT = 0, sR = 0;
    uint64_t undk[kPPL32];
    const uint32_t ok32 = __builtin_amdgcn_readfirstlane(__float_as_uint(F[13]));   // 1.0f, 0.0f or pruned
    if (ok32 == kPrunedFlag) continue;                  // exact bound pruning (PruneState)
    if (ok32 != 0u) {
      const float e0 = F[0], e1 = F[1], e2 = F[2], e3 = F[3], e4 = F[4], e5 = F[5], e6 = F[6], e7 = F[7], e8 = F[8];
      float neps1, eps2;
      if (GEN) {
        neps1 = -__builtin_fmaf(F[9], M4, F[10] * M2);               // per lane: its points' M
        eps2 = __builtin_fmaf(F[11], M4, F[12] * M2);
      } else {
        neps1 = F[14];
        eps2 = F[15];
      }
      // stage by stage across the kPPL32 points: independent FMA chains
      float ex0[kPPL32], ex1[kPPL32], ex2[kPPL32], xe0[kPPL32], xe1[kPPL32], a[kPPL32], D[kPPL32], aa[kPPL32];
      float din[kPPL32], dout[kPPL32];
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) ex0[k] = __builtin_fmaf(e0, x[k], __builtin_fmaf(e1, y[k], e2));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) ex1[k] = __builtin_fmaf(e3, x[k], __builtin_fmaf(e4, y[k], e5));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) ex2[k] = __builtin_fmaf(e6, x[k], __builtin_fmaf(e7, y[k], e8));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) xe0[k] = __builtin_fmaf(xp[k], e0, __builtin_fmaf(yp[k], e3, e6));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) xe1[k] = __builtin_fmaf(xp[k], e1, __builtin_fmaf(yp[k], e4, e7));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) a[k] = __builtin_fmaf(xp[k], ex0[k], __builtin_fmaf(yp[k], ex1[k], ex2[k]));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k)
        D[k] = __builtin_fmaf(xe1[k], xe1[k], __builtin_fmaf(xe0[k], xe0[k], __builtin_fmaf(ex1[k], ex1[k], ex0[k] * ex0[k])));
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) aa[k] = a[k] * a[k];
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) din[k] = __builtin_fmaf(nt2lo, D[k], aa[k]);
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) dout[k] = __builtin_fmaf(nt2hi, D[k], aa[k]);
#pragma unroll
      for (int k = 0; k < kPPL32; ++k) {
        uint64_t mi = __ballot(din[k] < neps1);
        const uint64_t mo = __ballot(dout[k] > eps2);
        uint64_t und = ~(mi | mo);
        if (GEN) {
          mi &= ~bad;
          und |= bad;
        }
        if (MASKED) {
          const uint64_t mT = lane_prefix(nT - 64 * k), mR = lane_prefix(nR - 64 * k);
          und &= mT | mR;
          sT += __popcll(mi & mT);
          if (!SAME) sR += __popcll(mi & mR);
        } else {
          sT += __popcll(mi);
        }
        undk[k] = und;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kPPL32; ++k)                  // candidate outside the float32 range
        undk[k] = MASKED ? (lane_prefix(nT - 64 * k) | lane_prefix(nR - 64 * k)) : ~0ull;
    }
    // enqueue after the unrolled compares (enqueueing inside them splits the
    // FMA block per point and costs SGPRs)
#pragma unroll
    for (int k = 0; k < kPPL32; ++k) enqueue_undecided(undk[k], c, pl + 64 * k, lane, q, qn);   // pl: relative to the item
    if (SAME || !MASKED) sR = sT;
    if (lane == 0) {
      cnt[c][0] += sT;
      cnt[c][1] += sR;
    }
  }
  return c;
}

// Compacted float64 pass over the queued evaluations: 64 lanes x kDrainBatch
// entries per round, the point loads of a round issued together.
constexpr int kDrainBatch = 4;

template <class Src>
__device__ __forceinline__ void score32_drain(const double* __restrict__ CE, const Src& src, int b, int p0, int T,
                                              int R, const ScoreConsts& kc, int lane, int32_t (*cnt)[2],
                                              const uint32_t* q, int qn) {
#pragma unroll 1
  for (int i0 = 0; i0 < qn; i0 += 64 * kDrainBatch) {
    uint32_t e[kDrainBatch];
    double4 v[kDrainBatch];
#pragma unroll
    for (int j = 0; j < kDrainBatch; ++j) {
      const int i = i0 + 64 * j + lane;
      e[j] = i < qn ? q[i] : 0xffffffffu;
      v[j] = src.load(b, p0 + (e[j] != 0xffffffffu ? (int)(e[j] & 0xffffffu) : 0));
    }
#pragma unroll
    for (int j = 0; j < kDrainBatch; ++j) {
      if (e[j] == 0xffffffffu) continue;
      const int c = (int)(e[j] >> 24), p = p0 + (int)(e[j] & 0xffffffu);
      if (inlier_f64v(CE + (size_t)c * kCandStride, v[j], kc)) {
        if (p < T) atomicAdd(&cnt[c][0], 1);
        if (p < R) atomicAdd(&cnt[c][1], 1);
      }
    }
  }
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Work unit: one wave scores one (pair, 32-candidate tile, kPtsPerWave-point
// span) item on its own -- its own LDS copy of the tile's records, counts and
// queue, no block barrier -- so a wave that drains a long queue never holds up
// the other waves of its block.  The queue collects the whole item's
// undecided evaluations (drained at the item's end, or earlier when past its
// low mark), so drains run in full 64-lane rounds.
constexpr int kPtsPerWave = kPPL32 * 64 * 4;

template <class Src>
__global__ __launch_bounds__(kScoreThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_score32(const Src src, PairParams pp, int batch, int cmax, const int32_t* __restrict__ cand_total,
               const double* __restrict__ candE, int32_t* __restrict__ cntT, int32_t* __restrict__ cntR,
               ScoreConsts kc) {
  constexpr int kWaves = kScoreThreads / 64;
  __shared__ int32_t s_cnt[kWaves][kKC][2];
  __shared__ int32_t s_items[SFM_MAX_BATCH + 1];   // items per pair; [batch] = total
  __shared__ int32_t s_first[SFM_MAX_BATCH + 1];   // pair-major order: first item of each pair
  __shared__ int32_t s_tiles[SFM_MAX_BATCH];
  __shared__ double2 s_cand[kWaves][kKC * kCandStride / 2];
  __shared__ uint32_t s_queue[kWaves][kQueue];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    int most = 0, acc = 0;
    for (int b = 0; b < batch; ++b) {
      const int tiles = (cand_total[b] + kKC - 1) / kKC;
      const int splits = (max(pp.test[b], pp.rtest[b]) + kPtsPerWave - 1) / kPtsPerWave;
      s_tiles[b] = tiles;
      s_items[b] = tiles * splits;
      s_first[b] = acc;
      acc += tiles * splits;
      most = max(most, tiles * splits);
    }
    s_first[batch] = acc;
    s_items[batch] = kc.interleave ? most * batch : acc;
  }
  for (int i = tid; i < kWaves * kKC * 2; i += kScoreThreads) (&s_cnt[0][0][0])[i] = 0;
  __syncthreads();
  int32_t(*cnt)[2] = s_cnt[wv];
  uint32_t* queue = s_queue[wv];
  const double* CE = reinterpret_cast<const double*>(s_cand[wv]);
  const int total = __builtin_amdgcn_readfirstlane(s_items[batch]);
  const int gw = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wv);
  // Items run split-major within a pair (every candidate of a pair advances
  // through its points together), pairs one after another, or interleaved
  // (item % batch, tuning key score_interleave).
  unsigned long long skipped = 0;                               // evaluations pruned by this wave
  for (int item = gw; item < total; item += gridDim.x * kWaves) {
    int b, local;
    if (kc.interleave) {
      b = __builtin_amdgcn_readfirstlane(item % batch);
      local = item / batch;
      if (local >= __builtin_amdgcn_readfirstlane(s_items[b])) continue;   // ragged batch: this pair is done
    } else {
      b = 0;
      while (item >= s_first[b + 1]) ++b;
      b = __builtin_amdgcn_readfirstlane(b);                    // wave-uniform (LDS-derived)
      local = item - __builtin_amdgcn_readfirstlane(s_first[b]);
    }
    const int tiles = __builtin_amdgcn_readfirstlane(s_tiles[b]);
    const int split = local / tiles, tile = local - split * tiles;
    const int ctot = cand_total[b];
    const int c0 = tile * kKC;
    const int nc = min(kKC, ctot - c0);
    const int T = pp.test[b], R = pp.rtest[b];
    const int M = max(T, R);
    const int p0 = split * kPtsPerWave;
    const int p1 = min(M, p0 + kPtsPerWave);
    {
      // this wave's copy of the tile's candidate records (nc x 144 B)
      const double2* srcc = reinterpret_cast<const double2*>(candE + ((size_t)b * cmax + c0) * kCandStride);
      for (int i = lane; i < nc * (kCandStride / 2); i += 64) s_cand[wv][i] = srcc[i];
    }
    wave_sync();
    // candidates whose bound count + (T - covered) is below the pair's best
    // count so far: flagged in this wave's LDS record (score32_pass skips them)
    bool all_pruned = false;
    int lb = 0;
    if (kc.prune) {
      const PruneState st = prune_state(cntR, kc.ws_batch, cmax);
      lb = __hip_atomic_load(st.best_lb + (size_t)b * kBestStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bool pr = false;
      if (lane < nc) {
        const unsigned long long v = __hip_atomic_load(st.cov + (size_t)b * cmax + c0 + lane, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        pr = (long long)(uint32_t)v + (long long)T - (long long)(v >> 32) < (long long)lb;
        if (pr) reinterpret_cast<float*>(s_cand[wv])[(lane * kCandStride + 10) * 2 + 13] = __uint_as_float(kPrunedFlag);
      }
      all_pruned = __ballot(pr) == lane_prefix(nc);
      wave_sync();
    }
    int qn = 0;
    for (int cb = all_pruned ? p1 : p0; cb < p1; cb += 64 * kPPL32) {
      int c = 0;
      for (;;) {
        // (re)load the chunk: the points are dead while the queue drains
        float x[kPPL32], y[kPPL32], xp[kPPL32], yp[kPPL32];
        double Mx = 1.0;
        const int pl = cb + lane;
#pragma unroll
        for (int k = 0; k < kPPL32; ++k) {
          const double4 v = src.load(b, min(pl + 64 * k, p1 - 1));
          Mx = fmax(Mx, fmax(fmax(fabs(v.x), fabs(v.y)), fmax(fabs(v.z), fabs(v.w))));
          x[k] = (float)v.x; y[k] = (float)v.y; xp[k] = (float)v.z; yp[k] = (float)v.w;
        }
        // lanes with a coordinate beyond 2^12 (or NaN) take the float64 test for all their points
        const bool lane_bad = !(Mx <= 0x1p12);
        const uint64_t bad = __ballot(lane_bad);
        const bool unit = __ballot(Mx != 1.0) == 0;                  // every lane M = 1, none bad
        const float Mf = lane_bad ? 1.0f : (float)Mx;
        const float M2 = Mf * Mf;
        const int nT = min(p1, T) - cb, nR = min(p1, R) - cb;
        if (min(nT, nR) >= 64 * kPPL32) {                           // no prefix masking needed
          if (unit) c = score32_pass<true, false, false>(CE, c, nc, pl - p0, nT, nR, x, y, xp, yp, M2, bad, kc, lane, cnt, queue, qn);
          else c = score32_pass<true, false, true>(CE, c, nc, pl - p0, nT, nR, x, y, xp, yp, M2, bad, kc, lane, cnt, queue, qn);
        } else if (T == R) {
          c = score32_pass<true, true, true>(CE, c, nc, pl - p0, nT, nR, x, y, xp, yp, M2, bad, kc, lane, cnt, queue, qn);
        } else {
          c = score32_pass<false, true, true>(CE, c, nc, pl - p0, nT, nR, x, y, xp, yp, M2, bad, kc, lane, cnt, queue, qn);
        }
        c = __builtin_amdgcn_readfirstlane(c);
        if (c >= nc) break;
        wave_sync();                                      // queue past its low mark: drain, resume at c
        score32_drain(CE, src, b, p0, T, R, kc, lane, cnt, queue, qn);
        qn = 0;
        wave_sync();
      }
    }
    wave_sync();
    score32_drain(CE, src, b, p0, T, R, kc, lane, cnt, queue, qn);
    wave_sync();
    if (kc.prune) {
      // publish (count, covered) of the span; raise the pair's best count so far
      const PruneState st = prune_state(cntR, kc.ws_batch, cmax);
      int reached = 0, skip = 0;
      if (lane < nc) {
        const float* F = reinterpret_cast<const float*>(CE + (size_t)lane * kCandStride + 10);
        if (__float_as_uint(F[13]) == kPrunedFlag) {
          skip = p1 - p0;
        } else {
          const int sc = cnt[lane][0];
          const unsigned long long old = atomicAdd(st.cov + (size_t)b * cmax + c0 + lane,
                                                   ((unsigned long long)(p1 - p0) << 32) | (unsigned)sc);
          reached = (int)(uint32_t)old + sc;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        reached = max(reached, __shfl_xor(reached, d, 64));
        skip += __shfl_xor(skip, d, 64);
      }
      // only raise the shared bound when this item beat the value it read:
      // one hot line per pair, updated by few items
      if (lane == 0 && reached > lb) atomicMax(st.best_lb + (size_t)b * kBestStride, reached);
      skipped += (unsigned long long)skip;
    }
    {
      const int c = lane >> 1, which = lane & 1;
      if (c < nc) {
        const int s = cnt[c][which];
        cnt[c][which] = 0;
        if (s) atomicAdd((which ? cntR : cntT) + (size_t)b * cmax + c0 + c, s);
      }
    }
    wave_sync();
  }
  if (kc.prune && lane == 0 && skipped) atomicAdd(prune_state(cntR, kc.ws_batch, cmax).skipped, skipped);
}

}  // namespace sfm
