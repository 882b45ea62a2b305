// RANSAC phases 1, 2 and 4: the five-point solve (k_solve_front, k_roots /
// k_roots_split, k_solve_back), the chains and the dense candidate list
// (k_chain, k_cand; k_fill_cands for given essential matrices) and the
// selection (k_select), with one launcher per profiled phase.
#include "ransac_common.h"
#include "five_point.h"

namespace sfm {

// ---------------------------------------------------------------------------
// Phase 1: one lane per hypothesis
// ---------------------------------------------------------------------------
// The solve is latency-bound (scratch-resident polynomial state, data-dependent
// Sturm iterations): only `lanes` lanes of each wave carry a hypothesis, so a
// pair's 4096 hypotheses occupy 4096 / lanes waves and every CU has several
// independent instruction streams to hide the scratch latency.
// The solve runs as three kernels so that each keeps a small live state:
//   k_solve_front  sample, E basis, constraint equations, reduction, det poly
//   k_roots        Sturm root isolation on a register-resident sequence
//                  (88 % of the former single kernel's time was spent here,
//                  waiting on scratch-resident coefficients)
//   k_solve_back   E per root, cheirality, compaction
// The state in between (116 doubles per hypothesis) is stored field-major.
__device__ __forceinline__ double& st_at(double* st, size_t stride, int f, size_t hb) { return st[f * stride + hb]; }

constexpr int kFrontLanes = 16;   // upper bound of the solve_lanes key

#ifdef SFM_FRONT_STATS
// experiment builds only: per wave (lane 0 of each block), the s_memtime
// stamps at the end of each phase of k_solve_front relative to its start:
// sample+load, basis, equations, reduction, determinant, state stores
__device__ unsigned long long g_front_cycles[6][1 << 15];
#define FRONT_STAMP(i)                                                                          \
  do {                                                                                          \
    __builtin_amdgcn_s_waitcnt(0);                                                              \
    if (threadIdx.x == 0)                                                                       \
      g_front_cycles[i][(size_t)blockIdx.y * gridDim.x + blockIdx.x] = __builtin_amdgcn_s_memtime() - t_front; \
  } while (0)
extern "C" int sfm_experiment_front_stats(unsigned long long* cycles, int n) {
  return hipMemcpyFromSymbol(cycles, HIP_SYMBOL(g_front_cycles), (size_t)6 * n * 8) == hipSuccess ? 0 : 2;
}
#else
#define FRONT_STAMP(i) do { } while (0)
#endif

// COOP (tuning key solve_coop, default): the reduction runs on DPP quads,
// four lanes per hypothesis (quad_reduce in five_point.h), so all 64 lanes of
// the wave work on the 16 hypotheses' reductions instead of 16 of them.
template <class Src, bool COOP>
__global__ __launch_bounds__(64) void k_solve_front(const Src src, PairParams pp, int H, uint64_t seed, int lanes,
                                                    double* __restrict__ st, size_t stride) {
#ifdef SFM_FRONT_STATS
  const unsigned long long t_front = __builtin_amdgcn_s_memtime();
#endif
  const int b = blockIdx.y;
  // COOP: quad g = lane / 4 carries hypothesis g; its four lanes draw the same
  // sample and build the same basis (the wave issues those instructions once
  // either way), then share the equations and the reduction
  const int g = COOP ? (int)threadIdx.x >> 2 : (int)threadIdx.x;
  const int qs = (int)threadIdx.x & 3;
  const int h = blockIdx.x * lanes + g;
  const bool act = g < lanes && h < H;
  if (!COOP && !act) return;
  // The equation set (1784 B) lives in LDS, one record per hypothesis: the
  // reduction's pivoting indexes rows dynamically, which put it in scratch
  // (0.30 -> 0.13 ms per 32,768 hypotheses).  A 1784-B lane stride is 446
  // dwords, so the 16 lanes' doubles fall in distinct bank pairs.
  __shared__ Eqs s_eqs[kFrontLanes];
  Eqs& A = s_eqs[g];
  double q[5][2], qp[5][2];
  Lin Eb[9];
  if (act) {
    const int64_t n = pp.n[b];
    int64_t idx[5];
    sample5(seed, (uint32_t)h, n, idx);
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const double4 v = src.load(b, idx[d]);
      q[d][0] = v.x; q[d][1] = v.y; qp[d][0] = v.z; qp[d][1] = v.w;
    }
    FRONT_STAMP(0);
    essential_basis(q, qp, Eb);
    FRONT_STAMP(1);
    if (COOP) {
      build_equations_quad(Eb, A, qs);
    } else {
      build_equations(Eb, A);
      FRONT_STAMP(2);
      reduce_equations(A);
    }
  }
  if (COOP) {
    __syncthreads();                           // the 16 records are written
    FRONT_STAMP(2);
    if (act) quad_reduce(A, qs);               // act is uniform per quad: its DPP exchanges stay within it
    __syncthreads();
    if (!act || qs != 0) return;
    raise_degree(A);
  }
  FRONT_STAMP(3);
  double poly[11];
  determinant_poly(A, poly);
  FRONT_STAMP(4);
  const size_t hb = (size_t)b * H + h;
#pragma unroll
  for (int e = 0; e < 9; ++e)
#pragma unroll
    for (int k = 0; k < 4; ++k) st_at(st, stride, kStEb + e * 4 + k, hb) = Eb[e].c[k];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      st_at(st, stride, kStA + i * 3 + j, hb) = A.e0[i][j];
      st_at(st, stride, kStA + 9 + i * 3 + j, hb) = A.e1[i][j];
      st_at(st, stride, kStA + 18 + i * 3 + j, hb) = A.e2[i][j];
      st_at(st, stride, kStA + 27 + i * 3 + j, hb) = A.e3[i][j];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) st_at(st, stride, kStA + 36 + i, hb) = A.e4[i];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    st_at(st, stride, kStQ + 4 * d + 0, hb) = q[d][0];
    st_at(st, stride, kStQ + 4 * d + 1, hb) = q[d][1];
    st_at(st, stride, kStQ + 4 * d + 2, hb) = qp[d][0];
    st_at(st, stride, kStQ + 4 * d + 3, hb) = qp[d][1];
  }
#pragma unroll
  for (int i = 0; i <= 10; ++i) st_at(st, stride, kStPoly + i, hb) = poly[i];
  FRONT_STAMP(5);
}

#ifdef SFM_ROOTS_STATS
__device__ unsigned long long g_roots_cycles[1 << 17];
extern "C" int sfm_experiment_roots_stats(unsigned int* evals, unsigned int* falsi, unsigned long long* cycles,
                                          unsigned long long* phases, int n, int reset) {
  if (reset) {
    static unsigned int z4[1 << 17];
    static unsigned long long z8[1 << 17];
    static unsigned long long zp[4][1 << 17];
    return (hipMemcpyToSymbol(HIP_SYMBOL(g_roots_evals), z4, sizeof(z4)) == hipSuccess &&
            hipMemcpyToSymbol(HIP_SYMBOL(g_roots_falsi), z4, sizeof(z4)) == hipSuccess &&
            hipMemcpyToSymbol(HIP_SYMBOL(g_roots_phase), zp, sizeof(zp)) == hipSuccess &&
            hipMemcpyToSymbol(HIP_SYMBOL(g_roots_cycles), z8, sizeof(z8)) == hipSuccess) ? 0 : 2;
  }
  return (hipMemcpyFromSymbol(evals, HIP_SYMBOL(g_roots_evals), n * 4) == hipSuccess &&
          hipMemcpyFromSymbol(falsi, HIP_SYMBOL(g_roots_falsi), n * 4) == hipSuccess &&
          hipMemcpyFromSymbol(phases, HIP_SYMBOL(g_roots_phase), 4 * (1 << 17) * 8) == hipSuccess &&
          hipMemcpyFromSymbol(cycles, HIP_SYMBOL(g_roots_cycles), n * 8) == hipSuccess) ? 0 : 2;
}
#endif

__global__ __launch_bounds__(64) void k_roots(int H, int lanes, double* __restrict__ st, size_t stride,
                                              int32_t* __restrict__ out_nroots) {
  const int b = blockIdx.y;
  if ((int)threadIdx.x >= lanes) return;
  const int h = blockIdx.x * lanes + threadIdx.x;
  if (h >= H) return;
#ifdef SFM_ROOTS_STATS
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  const size_t hb = (size_t)b * H + h;
  double poly[11];
#pragma unroll
  for (int i = 0; i <= 10; ++i) poly[i] = st_at(st, stride, kStPoly + i, hb);
#ifdef SFM_ROOTS_STATS
  __builtin_amdgcn_s_waitcnt(0);
  const unsigned long long tl = __builtin_amdgcn_s_memtime();
  g_roots_cycles[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x + (1 << 16)] = tl - t0;
#endif
  double roots[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) roots[i] = 0.0;
  __shared__ double s_lohi[kStkDepth * 2 * kStkLanes];
  __shared__ int s_ints[kStkDepth * 4 * kStkLanes];
  const IsoStack stk{s_lohi + threadIdx.x, s_ints + threadIdx.x};
  const int nr = real_roots_r(poly, roots, stk);
#pragma unroll
  for (int i = 0; i < 10; ++i) st_at(st, stride, kStRoots + i, hb) = roots[i];
  out_nroots[hb] = nr;
#ifdef SFM_ROOTS_STATS
  g_roots_cycles[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x] =
      __builtin_amdgcn_s_memtime() - t0;
#endif
}

// SOLVE_COOP (tuning key solve_coop, default): one DPP quad per hypothesis,
// lane s taking roots s, s + 4, s + 8; the accepted roots' slots come from a
// quad-wide mask of the cheirality results, so the writes are the one-lane
// loop's (accepted E / P in root order; slot 0 = root 0's E when no root is
// accepted).  Four times the waves of the one-lane kernel, whose 512 waves
// left half the SIMDs idle and followed each wave's most-rooted hypothesis.
template <bool COOP>
__global__ __launch_bounds__(64) void k_solve_back(int H, int cheir, const double* __restrict__ st, size_t stride,
                                                   const int32_t* __restrict__ nroots,
                                                   int32_t* __restrict__ out_ncand, double* __restrict__ hypE,
                                                   double* __restrict__ hypP) {
  const int b = blockIdx.y;
  const int qs = COOP ? (int)threadIdx.x & 3 : 0;
  const int h = COOP ? blockIdx.x * 16 + ((int)threadIdx.x >> 2) : blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = h < H;
  if (!COOP && !act) return;
  const size_t hb = (size_t)b * H + (act ? h : 0);
  const int nr = act ? nroots[hb] : 0;
  const int nv = nr > 0 ? (nr < 10 ? nr : 10) : 0;
  Lin Eb[9];
  Eqs A;   // only the blocks compute_E_matrix reads
  double q[5][2], qp[5][2];
  if (act) {
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
      for (int k = 0; k < 4; ++k) Eb[e].c[k] = st[(kStEb + e * 4 + k) * stride + hb];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        A.e0[i][j] = st[(kStA + i * 3 + j) * stride + hb];
        A.e1[i][j] = st[(kStA + 9 + i * 3 + j) * stride + hb];
        A.e2[i][j] = st[(kStA + 18 + i * 3 + j) * stride + hb];
        A.e3[i][j] = st[(kStA + 27 + i * 3 + j) * stride + hb];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i) A.e4[i] = st[(kStA + 36 + i) * stride + hb];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      q[d][0] = st[(kStQ + 4 * d + 0) * stride + hb];
      q[d][1] = st[(kStQ + 4 * d + 1) * stride + hb];
      qp[d][0] = st[(kStQ + 4 * d + 2) * stride + hb];
      qp[d][1] = st[(kStQ + 4 * d + 3) * stride + hb];
    }
  }
  double* Eo = hypE + hb * kMaxSlots * 9;
  double* Po = hypP + hb * kMaxSlots * 12;
  if (!COOP) {
    int nc = 0;
    for (int m = 0; m < nv; ++m) {
      const double w = st[(kStRoots + m) * stride + hb];
      double E[9];
      essential_at_root(Eb, A, w, E);
      if (!cheir) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Eo[m * 9 + e] = E[e];
        ++nc;
        continue;
      }
      double Pm[12];
      const bool ok = cheirality_P(E, q, qp, Pm);
      // compaction (cheirality.cu:142-146): accepted E's move to the front; if
      // none is accepted slot 0 keeps root 0's E.
      if (ok) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Eo[nc * 9 + e] = E[e];
#pragma unroll
        for (int e = 0; e < 12; ++e) Po[nc * 12 + e] = Pm[e];
        ++nc;
      } else if (m == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Eo[e] = E[e];
      }
    }
    out_ncand[hb] = nc;
    return;
  }
  // quad: roots m = qs + 4t
  double E[3][9], Pm[3][12];
  int okbits = 0;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int m = qs + 4 * t;
    if (m < nv) {
      const double w = st[(kStRoots + m) * stride + hb];
      essential_at_root(Eb, A, w, E[t]);
      const bool ok = !cheir || cheirality_P(E[t], q, qp, Pm[t]);
      if (ok) okbits |= 1 << m;
    }
  }
  // the quad's accepted-root mask (roots 0..9), OR-reduced over the four lanes
  okbits |= __builtin_amdgcn_update_dpp(0, okbits, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
  okbits |= __builtin_amdgcn_update_dpp(0, okbits, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
  if (!act) return;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int m = qs + 4 * t;
    if (m < nv) {
      if ((okbits >> m) & 1) {
        const int slot = __popc(okbits & ((1 << m) - 1));
#pragma unroll
        for (int e = 0; e < 9; ++e) Eo[slot * 9 + e] = E[t][e];
        if (cheir)
#pragma unroll
          for (int e = 0; e < 12; ++e) Po[slot * 12 + e] = Pm[t][e];
      } else if (m == 0 && okbits == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Eo[e] = E[t][e];
      }
    }
  }
  if (qs == 0) out_ncand[hb] = __popc(okbits);
}

// k_roots with the split isolation (five_point.h, isolate_p1 / falsi_tasks /
// bisect_deferred): lanes [0, lanes) of each wave own one hypothesis each
// through phase 1; phases 2 and 3 run over a task list on every lane.  NW = 1
// (roots_split 1, the default): one wave per block and its own list, so the
// launch lasts as long as its busiest wave (profiles/r03_roots_split_stats.txt:
// 245 k cycles per wave on average, 313-325 k at most).  NW = 4 (roots_split
// 2, opt-in): the block's four waves append to and claim from one pool (LDS
// counters), so the tail averages over four waves' tasks -- measured 2-6 %
// slower (profiles/r04_roots_pool_ab.txt).  Phase 1 stays per hypothesis, and
// every node's root goes to its fixed slot: the workspace is byte-identical.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_roots_split(int H, int lanes, double* __restrict__ st, size_t stride,
                                                         int32_t* __restrict__ out_nroots) {
  const int b = blockIdx.y;
  const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
  const int h = (blockIdx.x * NW + wv) * lanes + lane;
  const bool own = lane < lanes && h < H;
  const int owner = wv * kStkLanes + lane;                  // the hypothesis' slot in the pool
  __shared__ double s_lohi[NW][kStkDepth * 2 * kStkLanes];
  __shared__ int s_meta[NW][kStkDepth * kStkLanes];
  __shared__ RootsSharedT<kStkLanes * NW> sh;
  if (lane < kStkLanes) {
#pragma unroll
    for (int i = 0; i < 10; ++i) sh.roots[i][owner] = 0.0;
  }
  if (threadIdx.x == 0) { sh.ntask = 0; sh.ndl = 0; sh.next2 = 0; sh.next3 = 0; }
  __syncthreads();
#ifdef SFM_ROOTS_STATS
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  const size_t hb = (size_t)b * H + h;
  int nr = 0;
  double fac = 1.0;
  if (own) {
    double poly[11];
#pragma unroll
    for (int i = 0; i <= 10; ++i) poly[i] = st_at(st, stride, kStPoly + i, hb);
    double roots[10];
    SturmR R;
    const IsoStack stk{nullptr, nullptr};
    const IsoStackP stkp{s_lohi[wv] + lane, s_meta[wv] + lane};
    nr = real_roots_t<true>(poly, roots, stk, R, &sh, &stkp, owner, &fac);
  }
#ifdef SFM_ROOTS_STATS
  // split stats: cycles at the end of phase 1 / phase 2 in the second half of g_roots_cycles / g_roots_phase[0]
  const size_t si = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
  if (own) g_roots_cycles[si + (1 << 16)] = __builtin_amdgcn_s_memtime() - t0;
#endif
  __syncthreads();
  falsi_tasks<(NW > 1)>(sh, lane);
  __syncthreads();
#ifdef SFM_ROOTS_STATS
  if (own) g_roots_phase[0][si] = __builtin_amdgcn_s_memtime() - t0;
#endif
  bisect_deferred<(NW > 1)>(sh, lane);
  __syncthreads();
  if (own) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      double r = sh.roots[i][owner];
      if (i < nr) r /= fac;
      st_at(st, stride, kStRoots + i, hb) = r;
    }
    out_nroots[hb] = nr;
  }
#ifdef SFM_ROOTS_STATS
  if (own) g_roots_cycles[si] = __builtin_amdgcn_s_memtime() - t0;
#endif
}

// ---------------------------------------------------------------------------
// Fast inlier decision: error bound (derivation in DESIGN.md, "Scoring").
//
// With u = 2^-53, R = sum |E_ij| and M = max(1, |x|, |y|, |x'|, |y'|), the
// FMA-evaluated quantities used below differ from the values the reference's
// operation order produces by at most
//     |a_f - a_r| <= 11 u M^2 R,   ||v_f - v_r|| <= 10.0002 u R M
// (v = (Ex0, Ex1, xE0, xE1), a = x'^T E x, D = ||v||^2).  Deciding
//     inlier  if a_f^2 < thr^2 (1 - 2^-22) D_f,
//     outlier if a_f^2 > thr^2 (1 + 2^-22) D_f
// is then provably identical to the reference's IEEE test whenever
//     D_f >= (u R M^2 G)^2,   G = 2^24 (11 + 11/thr),
// and 2^-40 <= thr < 1, 2^-100 <= R <= 2^100, M <= 2^100.  Every other
// (candidate, point) pair takes the exact path.  Per candidate the constant
// Kg = (u R G)^2 is stored in candE[9] (NaN disables the fast path); per
// point mm2 = M^4, so the guard is D_f >= Kg * mm2.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double guard_constant(const double* E, double g) {
  double R = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) R += fabs(E[e]);
  if (!(R >= 0x1p-100 && R <= 0x1p100) || !(g > 0.0)) return __builtin_nan("");
  const double k = 0x1p-53 * R * g;
  return k * k;
}

// ---------------------------------------------------------------------------
// Float32 pre-decision (k_score32).  With u = 2^-24, M = max(1, |x|, |y|,
// |x'|, |y'|) <= 2^12 and R = sum|E_ij| in [2^-30, 2^30], the float32 FMA
// evaluation (inputs rounded to float32) satisfies
//     |a_s - a*| <= alpha = 8 u R M^2,   ||v_s - v*|| <= beta = 8.1 u R M
// against the exact values a*, v* of the float64 inputs (7.1 u R M^2 and
// 8.02 u R M by the standard bounds; the reference's own float64 error is far
// below the slack).  Bounding the cross terms 2|a|alpha and 2 sqrt(D) beta by
// AM-GM with weight 2^7 turns the reference test into two sign tests:
//     inlier  if fma(-t2lo, D, a*a) < -eps1
//     outlier if fma(-t2hi, D, a*a) >  eps2
//     eps1 = 129 alpha^2 + 128 thr^2 beta^2           = A1 M^4 + B1 M^2
//     eps2 = (128 alpha^2 + 129 thr^2 beta^2)/(1-2^-7) = A2 M^4 + B2 M^2
//     t2lo = thr^2 (1 - 2^-6 - 2^-19),  t2hi = thr^2 (1 + 2^-7)/(1 - 2^-7) (1 + 2^-19)
// (rounding is monotone and +-eps are floats, so each compare implies the
// exact inequality on aa = fl(a^2); aa is within u of a^2, the same loss as
// rounding a^2 + eps once; derivation in DESIGN.md, "Scoring").  Anything else
// is undecided and re-evaluated by the float64 path.  A*, B* carry a 2^-20
// upward slack that covers their float32 rounding and the float32 operations
// forming eps; slots 14/15 hold -eps1 and eps2 at M = 1 (the common case).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fp32_constants(const double* E, double thr, bool enable, float* out) {
  double R = 0.0;
  bool finite = true;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    R += fabs(E[e]);
    finite = finite && isfinite(E[e]);
  }
  const bool ok = enable && finite && R >= 0x1p-30 && R <= 0x1p30;
#pragma unroll
  for (int e = 0; e < 9; ++e) out[e] = ok ? (float)E[e] : 0.0f;
  const double al = 8.0 * 0x1p-24 * R * (1.0 + 0x1p-20) + 0x1p-120;
  const double be = 8.1 * 0x1p-24 * R * (1.0 + 0x1p-20) + 0x1p-120;
  const double t2 = thr * thr, up = 1.0 + 0x1p-20;
  const double A1 = 129.0 * al * al * up, B1 = 128.0 * t2 * be * be * up;
  const double A2 = 128.0 * al * al / (1.0 - 0x1p-7) * up, B2 = 129.0 * t2 * be * be / (1.0 - 0x1p-7) * up;
  out[9] = ok ? (float)A1 : 0.0f;
  out[10] = ok ? (float)B1 : 0.0f;
  out[11] = ok ? (float)A2 : 0.0f;
  out[12] = ok ? (float)B2 : 0.0f;
  out[13] = ok ? 1.0f : 0.0f;
  out[14] = ok ? -(float)((A1 + B1) * up) : 0.0f;
  out[15] = ok ? (float)((A2 + B2) * up) : 0.0f;
}

// ---------------------------------------------------------------------------
// Phase 2: chains and the dense candidate list
//   k_chain  one block of 512 per pair: exclusive scan of the candidate counts
//            over chains (chain t owns hypotheses t*iters .. t*iters+iters-1)
//   k_cand   one thread per (hypothesis, slot): the candidate records
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kChains) void k_chain(int H, int iters, const int32_t* __restrict__ nroots,
                                                   const int32_t* __restrict__ ncand, int32_t* __restrict__ cand_off,
                                                   int32_t* __restrict__ chain_ref, int32_t* __restrict__ cand_total,
                                                   unsigned long long* __restrict__ skipped) {
  __shared__ int32_t s_sum[kChains / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  // the call's pruning counter (first chunk only; it accumulates over chunks),
  // zeroed here rather than by a memset launch of its own
  if (skipped && b == 0 && t == 0) *skipped = 0ull;
  const size_t hb0 = (size_t)b * H + (size_t)t * iters;
  int cnt = 0;
  for (int i = 0; i < iters; ++i) {
    const int nc = ncand[hb0 + i];
    cnt += nc > 0 ? nc : 1;
  }
  const int lane = t & 63, wv = t >> 6;
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  if (lane == 63) s_sum[wv] = incl;
  __syncthreads();
  int off = incl - cnt;
  for (int w = 0; w < wv; ++w) off += s_sum[w];
  if (t == kChains - 1) cand_total[b] = off + cnt;
  // the same walk records, per hypothesis, the slot-0 state the reference
  // thread holds (kernel_functions.cu:154, 179): the chain's latest hypothesis
  // with a root (E) up to i, and with an accepted candidate (P) before i, so
  // that k_cand reads them in O(1) instead of looking back along the chain
  int ke = -1, kp = -1;
  for (int i = 0; i < iters; ++i) {
    const int nc = ncand[hb0 + i];
    if (nroots[hb0 + i] > 0) ke = i;
    cand_off[hb0 + i] = off;
    chain_ref[hb0 + i] = (ke + 1) | ((kp + 1) << 16);
    off += nc > 0 ? nc : 1;
    if (nc > 0) kp = i;
  }
}

// A hypothesis with no candidate rescores slot 0 as the reference thread
// holds it (kernel_functions.cu:154, 179-214): E of the chain's latest
// hypothesis with a root, P of its latest with an accepted candidate (zeros
// before any), as k_chain recorded them (chain_ref).
__global__ __launch_bounds__(256) void k_cand(int H, int iters, int cheir, const int32_t* __restrict__ chain_ref,
                                              const int32_t* __restrict__ ncand, const double* __restrict__ hypE,
                                              const double* __restrict__ hypP, double* __restrict__ hypP0,
                                              const int32_t* __restrict__ cand_off, double* __restrict__ candE,
                                              int cmax, double guard_g, double thr, int fast32,
                                              int32_t* __restrict__ cntT, int32_t* __restrict__ cntR) {
  const int b = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int h = g / kMaxSlots, j = g - h * kMaxSlots;
  if (h >= H) return;
  const size_t hb0 = (size_t)b * H;
  const size_t hb = hb0 + h;
  const int nc = ncand[hb];
  if (j >= (nc > 0 ? nc : 1)) return;
  const size_t ci = (size_t)b * cmax + cand_off[hb] + j;
  double* dst = candE + ci * kCandStride;
  // the scorers add into the counts of candidates < cand_total only: zeroing
  // them with their records replaces two memset launches per call
  cntT[ci] = 0;
  cntR[ci] = 0;
  if (nc > 0) {
    const double* Eh = hypE + (hb * kMaxSlots + j) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) dst[e] = Eh[e];
  } else {
    const int i = h % iters;
    const size_t c0 = hb - i;   // the chain's first hypothesis
    const int ref = chain_ref[hb];
    const int ke = (ref & 0xffff) - 1, kp = cheir ? (ref >> 16) - 1 : -1;
#pragma unroll
    for (int e = 0; e < 9; ++e) dst[e] = ke >= 0 ? hypE[(c0 + ke) * kMaxSlots * 9 + e] : 0.0;
#pragma unroll
    for (int e = 0; e < 12; ++e) hypP0[hb * 12 + e] = kp >= 0 ? hypP[(c0 + kp) * kMaxSlots * 12 + e] : 0.0;
  }
  dst[9] = guard_constant(dst, guard_g);
  fp32_constants(dst, thr, fast32 != 0, reinterpret_cast<float*>(dst + 10));
}

// Candidate records of given essential matrices (sfm_score_essentials): E,
// the float64 guard constant and the float32 constants, as k_cand writes them.
__global__ __launch_bounds__(256) void k_fill_cands(const double* __restrict__ E, int ncand, int cmax,
                                                    double guard_g, double thr, int fast32,
                                                    double* __restrict__ candE, int32_t* __restrict__ cand_total) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0) cand_total[b] = ncand;
  if (c >= ncand) return;
  double* dst = candE + ((size_t)b * cmax + c) * kCandStride;
  const double* src = E + ((size_t)b * ncand + c) * 9;
#pragma unroll
  for (int e = 0; e < 9; ++e) dst[e] = src[e];
  dst[9] = guard_constant(dst, guard_g);
  fp32_constants(dst, thr, fast32 != 0, reinterpret_cast<float*>(dst + 10));
}

// ---------------------------------------------------------------------------
// Phase 4: selection (one block per pair)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_select(int H, int cmax, int cheir,
                                                 const int32_t* __restrict__ ncand,
                                                 const int32_t* __restrict__ cand_off,
                                                 const int32_t* __restrict__ cntT,
                                                 const int32_t* __restrict__ cntR,
                                                 const double* __restrict__ candE,
                                                 const double* __restrict__ hypP,
                                                 const double* __restrict__ hypP0,
                                                 int32_t* __restrict__ score_out,
                                                 double* __restrict__ E_out, double* __restrict__ P_out,
                                                 int32_t* __restrict__ inliers_out, int32_t* __restrict__ winner_out) {
  __shared__ unsigned long long s_best[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t hb0 = (size_t)b * H;
  const int32_t* cT = cntT + (size_t)b * cmax;
  const int32_t* cR = cntR + (size_t)b * cmax;
  unsigned long long best = 0ull;
  for (int h = tid; h < H; h += blockDim.x) {
    const int nc = ncand[hb0 + h], off = cand_off[hb0 + h];
    int bi = 0, bc = 0;
    for (int j = 0; j < nc; ++j) {
      const int c = cT[off + j];
      if (c > bc) { bc = c; bi = j; }
    }
    const int s = cR[off + bi];
    score_out[hb0 + h] = s;
    const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)h);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d, 64);
    best = o > best ? o : best;
  }
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) best = s_best[w] > best ? s_best[w] : best;
  const int s = (int)(best >> 32);
  double* Eo = E_out + (size_t)b * 9;
  double* Po = P_out ? P_out + (size_t)b * 12 : nullptr;
  if (s <= 0) {
    for (int e = 0; e < 9; ++e) Eo[e] = 0.0;
    if (Po) for (int e = 0; e < 12; ++e) Po[e] = 0.0;
    inliers_out[b] = 0;
    if (winner_out) winner_out[b] = -1;
    return;
  }
  const int h = (int)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull));
  const int nc = ncand[hb0 + h], off = cand_off[hb0 + h];
  int bi = 0, bc = 0;
  for (int j = 0; j < nc; ++j) {
    const int c = cT[off + j];
    if (c > bc) { bc = c; bi = j; }
  }
  const double* Ew = candE + ((size_t)b * cmax + off + bi) * kCandStride;
  for (int e = 0; e < 9; ++e) Eo[e] = Ew[e];
  if (Po) {
    const double* Pw = nc > 0 ? hypP + ((hb0 + h) * kMaxSlots + bi) * 12 : hypP0 + (hb0 + h) * 12;
    for (int e = 0; e < 12; ++e) Po[e] = cheir ? Pw[e] : 0.0;
  }
  inliers_out[b] = s;
  if (winner_out) winner_out[b] = h;
}

// ---------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------
template <class Src>
void launch_solve(const Src& src, const PairParams& pp, int bc, int H, uint64_t seed, int cheir, const Workspace& w,
                  hipStream_t s) {
  ProfScope ps("ransac_solve", s);
  // lane counts bounded by the kernels' per-lane LDS records (the key validators enforce it too)
  const int lanes = std::min(tuning().solve_lanes, kFrontLanes);
  const int rlanes = std::min(tuning().roots_lanes, kStkLanes);
  const size_t stride = (size_t)bc * H;
  if (tuning().solve_coop)
    hipLaunchKernelGGL((k_solve_front<Src, true>), dim3((H + lanes - 1) / lanes, bc), dim3(64), 0, s, src, pp, H,
                       seed, lanes, w.sstate, stride);
  else
    hipLaunchKernelGGL((k_solve_front<Src, false>), dim3((H + lanes - 1) / lanes, bc), dim3(64), 0, s, src, pp, H,
                       seed, lanes, w.sstate, stride);
  if (tuning().roots_split == 2)
    hipLaunchKernelGGL(k_roots_split<4>, dim3((H + 4 * rlanes - 1) / (4 * rlanes), bc), dim3(256), 0, s, H, rlanes,
                       w.sstate, stride, w.nroots);
  else if (tuning().roots_split)
    hipLaunchKernelGGL(k_roots_split<1>, dim3((H + rlanes - 1) / rlanes, bc), dim3(64), 0, s, H, rlanes, w.sstate,
                       stride, w.nroots);
  else
    hipLaunchKernelGGL(k_roots, dim3((H + rlanes - 1) / rlanes, bc), dim3(64), 0, s, H, rlanes, w.sstate, stride,
                       w.nroots);
  if (tuning().solve_coop)
    hipLaunchKernelGGL(k_solve_back<true>, dim3((H + 15) / 16, bc), dim3(64), 0, s, H, cheir, w.sstate, stride,
                       w.nroots, w.ncand, w.hypE, w.hypP);
  else
    hipLaunchKernelGGL(k_solve_back<false>, dim3((H + 63) / 64, bc), dim3(64), 0, s, H, cheir, w.sstate, stride,
                       w.nroots, w.ncand, w.hypE, w.hypP);
}
template void launch_solve<PackedSrc>(const PackedSrc&, const PairParams&, int, int, uint64_t, int, const Workspace&,
                                      hipStream_t);
template void launch_solve<FlowSrc>(const FlowSrc&, const PairParams&, int, int, uint64_t, int, const Workspace&,
                                    hipStream_t);

void launch_chain(int bc, int H, int iters, int cheir, double thr, const ScorePlan& plan, const Workspace& w,
                  bool first_chunk, hipStream_t s) {
  ProfScope ps("ransac_chain", s);
  hipLaunchKernelGGL(k_chain, dim3(bc), dim3(kChains), 0, s, H, iters, w.nroots, w.ncand, w.cand_off, w.chain_ref,
                     w.cand_total, first_chunk ? w.skipped : nullptr);
  hipLaunchKernelGGL(k_cand, dim3((H * kMaxSlots + 255) / 256, bc), dim3(256), 0, s, H, iters, cheir, w.chain_ref,
                     w.ncand, w.hypE, w.hypP, w.hypP0, w.cand_off, w.candE, plan.cmax, plan.guard_g, thr,
                     plan.fast32 ? 1 : 0, w.cntT, w.cntR);
}

void launch_select(int bc, int H, int cheir, const ScorePlan& plan, const Workspace& w, int32_t* score_out,
                   double* E_out, double* P_out, int32_t* inliers_out, int32_t* winner_out, hipStream_t s) {
  ProfScope ps("ransac_select", s);
  hipLaunchKernelGGL(k_select, dim3(bc), dim3(1024), 0, s, H, plan.cmax, cheir, w.ncand, w.cand_off, w.cntT,
                     plan.one_cnt ? w.cntT : w.cntR, w.candE, w.hypP, w.hypP0, score_out ? score_out : w.score, E_out,
                     P_out, inliers_out, winner_out);
}

void launch_fill_cands(const double* E, int batch, int ncand, double thr, const ScorePlan& plan, const ScoreBufs& w,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_fill_cands, dim3((ncand + 255) / 256, batch), dim3(256), 0, s, E, ncand, ncand, plan.guard_g,
                     thr, plan.fast32 ? 1 : 0, w.candE, w.cand_total);
}

}  // namespace sfm
