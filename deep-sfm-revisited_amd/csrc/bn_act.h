// BatchNorm, ReLU and the residual add on channels-last float16, forward and
// backward: the one definition of the five kernels, templated on the channel
// count C (32, 64 or 128), and the checked launchers that sfm_bn3_* (bn3.hip,
// C = 32: the 3-D regularisation stack) and sfm_bn2_* (bn2.hip: the feature
// CNN's three widths) instantiate.
//
// x is [rows][C] float16: a row (a voxel or a pixel) is 2 C bytes and a lane
// owns one 8-channel group of it, so every load and store is 16 bytes, C / 8
// lanes cover a row and a wave covers 16, 8 or 4 consecutive rows (1 KiB, fully
// coalesced).  Every row index and byte offset is 64-bit.
//
//   k_bn3_stats       one pass over x: per channel sum x and sum x^2 in float64
//                     (the square of a float16 value is exact there).  A fixed
//                     grid; block k walks the contiguous row range
//                     [k N / n, (k + 1) N / n) and writes one [2][C] double
//                     partial -- zeros when its range is empty.
//   k_bn3_finalize    one block: adds the partials in block order (combine())
//                     and derives mean, biased variance, invstd, a = gamma invstd
//                     and b = beta - mean a in float64, each rounded once to
//                     float32; updates the running statistics as torch does.  In
//                     eval mode it is the only launch and reads the running
//                     statistics instead.
//   k_bn3_apply       out = f16(relu(fma(a, x, b)) + residual): float32, one
//                     rounding.
//   k_bn3_bwd_reduce  sum dy and sum dy x per channel in float64, dy = grad_out
//                     masked by the recomputed fma(a, x, b) > 0 (the forward's
//                     float32 expression, so the forward's mask); same grid and
//                     partials as k_bn3_stats.
//   k_bn3_bwd_apply   every block adds the partials in block order itself (they
//                     sit in L2), so the backward is two launches; block 0 writes
//                     dgamma and dbeta; then dx in float32, one rounding.
//
// No atomics anywhere: a thread's, a wave's, a block's and the grid's sums are
// each added in a fixed order, so two calls give the same bits.  At C = 32 the
// order is the one csrc/bn3.hip had before the template: the same bits.
#pragma once
#include <string>
#include "common.h"

namespace sfm {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kBnThreads = 512;                   // 8 waves
constexpr int kBnWaves = kBnThreads / 64;
constexpr int kBnDefaultBlocks = 512;             // reducing blocks: 2 per CU on MI355X (256 CUs)
constexpr int kBnApplyBlocks = 1024;              // most blocks of the grid-stride apply kernels
constexpr int kBnBwdApplyBlocks = 512;            // each of these re-adds the partials: fewer of them

// the layout at C channels
template <int C>
struct BnShape {
  static_assert(C == 32 || C == 64 || C == 128, "channel counts of the batch-norm kernels");
  static constexpr int kLanes = C / 8;                     // lanes that cover a row: 4, 8, 16
  static constexpr int kRows = kBnThreads / kLanes;        // rows a block covers per load: 128, 64, 32
  static constexpr int kEntries = 2 * C;                   // doubles per partial: [2][C]
};

__device__ __forceinline__ f16x8 ld8(const unsigned short* p) {
  return __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(p));
}
__device__ __forceinline__ void st8(unsigned short* p, f16x8 v) {
  *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, v);
}

// first row of block k's range
__device__ __forceinline__ int64_t range_begin(int64_t rows, int64_t k, int64_t nb) { return rows * k / nb; }

// The block's sums of acc[0..7] (first row of the partial) and acc[8..15]
// (second row), the thread's values for channels 8 g + j of its group
// g = tid & (C / 8 - 1), written as one [2][C] partial: a butterfly over the
// lanes of a wave that share g (16, 8 or 4 of them), then the 8 waves in order.
template <int C>
__device__ __forceinline__ void block_partial(double (&acc)[16], double* __restrict__ out) {
  constexpr int L = BnShape<C>::kLanes, E = BnShape<C>::kEntries;
  __shared__ double sh[kBnWaves][E];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = tid & (L - 1);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    double v = acc[i];
#pragma unroll
    for (int m = L; m < 64; m *= 2) v = v + __shfl_xor(v, m);
    acc[i] = v;
  }
  if (lane < L) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sh[wv][(i >> 3) * C + g * 8 + (i & 7)] = acc[i];
  }
  __syncthreads();
  if (tid < E) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kBnWaves; ++w) s = s + sh[w][tid];
    out[tid] = s;
  }
}

// tot[e] = the partials of blocks 0, 1, ... nb - 1 added in block order: wave r
// adds the r-th of eight contiguous runs of blocks in order (a lane holds
// entries lane, lane + 64, ...), the eight sums are then added in order.
// Called by every thread of a block; tot is LDS, 2 C entries.
template <int C>
__device__ __forceinline__ void combine(const double* __restrict__ partial, int nb, double* tot) {
  constexpr int E = BnShape<C>::kEntries, Q = E / 64;
  __shared__ double run[kBnWaves][E];
  const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int k0 = nb * r / kBnWaves, k1 = nb * (r + 1) / kBnWaves;
  double s[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) s[q] = 0.0;
#pragma unroll 8
  for (int k = k0; k < k1; ++k) {
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = s[q] + partial[(int64_t)k * E + q * 64 + lane];
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) run[r][q * 64 + lane] = s[q];
  __syncthreads();
  if (threadIdx.x < E) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < kBnWaves; ++q) t = t + run[q][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
}

__device__ __forceinline__ void stats_accum(double (&acc)[16], f16x8 v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const double d = (double)(float)v[j];
    acc[j] = acc[j] + d;
    acc[8 + j] = __builtin_fma(d, d, acc[8 + j]);          // d d is exact: one rounding, the sum's
  }
}

template <int C>
__global__ __launch_bounds__(kBnThreads) void k_bn3_stats(const unsigned short* __restrict__ x, int64_t rows,
                                                         double* __restrict__ partial) {
  constexpr int L = BnShape<C>::kLanes, R = BnShape<C>::kRows;
  const int tid = threadIdx.x, g = tid & (L - 1);
  const int64_t v1 = range_begin(rows, (int64_t)blockIdx.x + 1, gridDim.x);
  int64_t v = range_begin(rows, blockIdx.x, gridDim.x) + tid / L;
  const unsigned short* xg = x + g * 8;
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0;
  for (; v + 3 * R < v1; v += 4 * R) {                     // four loads in flight
    const f16x8 a0 = ld8(xg + v * C), a1 = ld8(xg + (v + R) * C);
    const f16x8 a2 = ld8(xg + (v + 2 * R) * C), a3 = ld8(xg + (v + 3 * R) * C);
    stats_accum(acc, a0);
    stats_accum(acc, a1);
    stats_accum(acc, a2);
    stats_accum(acc, a3);
  }
  for (; v < v1; v += R) stats_accum(acc, ld8(xg + v * C));
  block_partial<C>(acc, partial + (int64_t)blockIdx.x * BnShape<C>::kEntries);
}

template <int C>
__global__ __launch_bounds__(kBnThreads) void k_bn3_finalize(const double* __restrict__ partial, int nb, int64_t rows,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, double eps,
                                                            float* running_mean, float* running_var, double momentum,
                                                            int training, float* __restrict__ stats) {
  __shared__ double tot[BnShape<C>::kEntries];
  if (training) combine<C>(partial, nb, tot);              // block-uniform
  const int c = threadIdx.x;
  if (c >= C) return;
  double mean, var;
  if (training) {
    const double n = (double)rows;
    mean = tot[c] / n;
    var = tot[C + c] / n - mean * mean;
    if (var < 0.0) var = 0.0;
    // torch's rule: (1 - m) r + m batch, the batch variance unbiased
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * n / (n - 1.0)));
  } else {
    mean = (double)running_mean[c];
    var = (double)running_var[c];
  }
  const double invstd = 1.0 / sqrt(var + eps);
  const double a = (double)gamma[c] * invstd;
  const double b = (double)beta[c] - mean * a;
  stats[c] = (float)mean;
  stats[C + c] = (float)var;
  stats[2 * C + c] = (float)invstd;
  stats[3 * C + c] = (float)a;
  stats[4 * C + c] = (float)b;
}

// the forward's pre-activation: one float32 fused multiply-add, here and in the backward's mask
__device__ __forceinline__ float pre_act(float a, float x, float b) { return __builtin_fmaf(a, x, b); }

template <bool RELU, bool RES>
__device__ __forceinline__ f16x8 apply8(f16x8 xv, f16x8 rv, const float (&a)[8], const float (&b)[8]) {
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float z = pre_act(a[j], (float)xv[j], b[j]);
    if (RELU) z = (z > 0.0f || z != z) ? z : 0.0f;         // a NaN stays a NaN, as torch's relu keeps it
    if (RES) z = z + (float)rv[j];
    o[j] = (_Float16)z;                                     // the one rounding (nearest even)
  }
  return o;
}

// items: 16-byte groups, C / 8 per row.  The grid's stride is a multiple of C / 8, so a thread keeps its group.
template <int C, bool RELU, bool RES>
__global__ __launch_bounds__(kBnThreads) void k_bn3_apply(const unsigned short* __restrict__ x, int64_t items,
                                                         const float* __restrict__ stats,
                                                         const unsigned short* __restrict__ res,
                                                         unsigned short* __restrict__ out) {
  const int g = threadIdx.x & (BnShape<C>::kLanes - 1);
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = stats[3 * C + g * 8 + j];
    b[j] = stats[4 * C + g * 8 + j];
  }
  const int64_t stride = (int64_t)gridDim.x * kBnThreads;
  int64_t i = (int64_t)blockIdx.x * kBnThreads + threadIdx.x;
  const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (; i + stride < items; i += 2 * stride) {            // two groups in flight
    const int64_t i1 = i + stride;
    const f16x8 x0 = ld8(x + i * 8), x1 = ld8(x + i1 * 8);
    const f16x8 r0 = RES ? ld8(res + i * 8) : zero, r1 = RES ? ld8(res + i1 * 8) : zero;
    st8(out + i * 8, apply8<RELU, RES>(x0, r0, a, b));
    st8(out + i1 * 8, apply8<RELU, RES>(x1, r1, a, b));
  }
  for (; i < items; i += stride)
    st8(out + i * 8, apply8<RELU, RES>(ld8(x + i * 8), RES ? ld8(res + i * 8) : zero, a, b));
}

template <bool RELU>
__device__ __forceinline__ void bwd_accum(double (&acc)[16], f16x8 xv, f16x8 gv, const float (&a)[8],
                                          const float (&b)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xf = (float)xv[j];
    float dy = (float)gv[j];
    if (RELU && !(pre_act(a[j], xf, b[j]) > 0.0f)) dy = 0.0f;
    const double d = (double)dy;
    acc[j] = acc[j] + d;
    acc[8 + j] = __builtin_fma(d, (double)xf, acc[8 + j]);  // the product of two float16 values is exact
  }
}

template <int C, bool RELU>
__global__ __launch_bounds__(kBnThreads) void k_bn3_bwd_reduce(const unsigned short* __restrict__ x,
                                                              const unsigned short* __restrict__ gy, int64_t rows,
                                                              const float* __restrict__ stats,
                                                              double* __restrict__ partial) {
  constexpr int L = BnShape<C>::kLanes, R = BnShape<C>::kRows;
  const int tid = threadIdx.x, g = tid & (L - 1);
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = stats[3 * C + g * 8 + j];
    b[j] = stats[4 * C + g * 8 + j];
  }
  const int64_t v1 = range_begin(rows, (int64_t)blockIdx.x + 1, gridDim.x);
  int64_t v = range_begin(rows, blockIdx.x, gridDim.x) + tid / L;
  const unsigned short* xg = x + g * 8;
  const unsigned short* gg = gy + g * 8;
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0;
  for (; v + R < v1; v += 2 * R) {                         // four loads in flight
    const f16x8 x0 = ld8(xg + v * C), x1 = ld8(xg + (v + R) * C);
    const f16x8 g0 = ld8(gg + v * C), g1 = ld8(gg + (v + R) * C);
    bwd_accum<RELU>(acc, x0, g0, a, b);
    bwd_accum<RELU>(acc, x1, g1, a, b);
  }
  for (; v < v1; v += R) bwd_accum<RELU>(acc, ld8(xg + v * C), ld8(gg + v * C), a, b);
  block_partial<C>(acc, partial + (int64_t)blockIdx.x * BnShape<C>::kEntries);
}

template <bool RELU, bool TRAIN>
__device__ __forceinline__ f16x8 bwd8(f16x8 xv, f16x8 gv, const float (&a)[8], const float (&b)[8],
                                      const float (&mean)[8], const float (&invstd)[8], const float (&k1)[8],
                                      const float (&k2)[8]) {
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xf = (float)xv[j];
    float dy = (float)gv[j];
    if (RELU && !(pre_act(a[j], xf, b[j]) > 0.0f)) dy = 0.0f;
    float t = dy;
    if (TRAIN) {
      const float xh = (xf - mean[j]) * invstd[j];
      t = (dy - k1[j]) - xh * k2[j];
    }
    o[j] = (_Float16)(a[j] * t);
  }
  return o;
}

template <int C, bool RELU, bool TRAIN>
__global__ __launch_bounds__(kBnThreads) void k_bn3_bwd_apply(const unsigned short* __restrict__ x,
                                                             const unsigned short* __restrict__ gy, int64_t rows,
                                                             const float* __restrict__ stats,
                                                             const double* __restrict__ partial, int nb,
                                                             unsigned short* __restrict__ gx,
                                                             float* __restrict__ grad_gamma_beta) {
  __shared__ double tot[BnShape<C>::kEntries];
  __shared__ float coef[2][C];
  const int tid = threadIdx.x, g = tid & (BnShape<C>::kLanes - 1);
  if (TRAIN || blockIdx.x == 0) {                          // block-uniform: eval mode needs the sums for block 0 alone
    combine<C>(partial, nb, tot);
    if (tid < C) {
      const double mean = (double)stats[tid], invstd = (double)stats[2 * C + tid];
      const double dbeta = tot[tid];
      const double dgamma = (tot[C + tid] - mean * dbeta) * invstd;
      if (blockIdx.x == 0) {
        grad_gamma_beta[tid] = (float)dgamma;
        grad_gamma_beta[C + tid] = (float)dbeta;
      }
      const double n = (double)rows;
      coef[0][tid] = (float)(dbeta / n);
      coef[1][tid] = (float)(dgamma / n);
    }
    __syncthreads();
  }
  if (!gx) return;
  float a[8], b[8], mean[8], invstd[8], k1[8], k2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = g * 8 + j;
    a[j] = stats[3 * C + c];
    b[j] = stats[4 * C + c];
    mean[j] = stats[c];
    invstd[j] = stats[2 * C + c];
    k1[j] = TRAIN ? coef[0][c] : 0.0f;
    k2[j] = TRAIN ? coef[1][c] : 0.0f;
  }
  const int64_t items = rows * BnShape<C>::kLanes;
  const int64_t stride = (int64_t)gridDim.x * kBnThreads;
  int64_t i = (int64_t)blockIdx.x * kBnThreads + tid;
  for (; i + stride < items; i += 2 * stride) {            // four loads in flight
    const int64_t i1 = i + stride;
    const f16x8 x0 = ld8(x + i * 8), x1 = ld8(x + i1 * 8);
    const f16x8 g0 = ld8(gy + i * 8), g1 = ld8(gy + i1 * 8);
    st8(gx + i * 8, bwd8<RELU, TRAIN>(x0, g0, a, b, mean, invstd, k1, k2));
    st8(gx + i1 * 8, bwd8<RELU, TRAIN>(x1, g1, a, b, mean, invstd, k1, k2));
  }
  for (; i < items; i += stride)
    st8(gx + i * 8, bwd8<RELU, TRAIN>(ld8(x + i * 8), ld8(gy + i * 8), a, b, mean, invstd, k1, k2));
}

constexpr int64_t kBnMaxRows = (int64_t)1 << 40;          // rows x 4096 blocks stays far inside int64

// bn_blocks: a given number of reducing blocks (launch shape only; more blocks than rows is allowed: the
// spare ones write zero partials)
template <int C>
int bn_blocks(int64_t rows) {
  const int forced = tuning().bn_blocks;
  if (forced > 0) return forced;
  const int64_t steps = (rows + BnShape<C>::kRows - 1) / BnShape<C>::kRows;
  return (int)(steps < kBnDefaultBlocks ? steps : kBnDefaultBlocks);
}

template <int C>
size_t bn_ws_bytes(int64_t rows) {
  return (size_t)bn_blocks<C>(rows) * BnShape<C>::kEntries * sizeof(double);
}

inline unsigned apply_grid(int64_t items, int most) {
  const int64_t blocks = (items + kBnThreads - 1) / kBnThreads;
  return (unsigned)(blocks < most ? blocks : most);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what an entry-point family calls a row, and its profile scopes
struct BnWords {
  const char* bad_count;       // "invalid voxel count"
  const char* need_two;        // the training-mode refusal of a single row
  const char* stats;           // profile scopes
  const char* apply;
  const char* bwd;
};

// The three checked launchers: every refusal before any pointer is read.
template <int C>
int bn_stats(const BnWords& wd, const void* x, int64_t rows, const float* gamma, const float* beta, double eps,
             float* running_mean, float* running_var, double momentum, int training, float* stats, void* workspace,
             size_t workspace_bytes, void* stream) {
  constexpr size_t kStatsBytes = 5 * C * sizeof(float), kRowBytes = C * sizeof(float);
  SFM_REQUIRE(x && gamma && beta && stats, "null pointer argument");
  SFM_REQUIRE(training == 0 || training == 1, "training must be 0 or 1");
  SFM_REQUIRE(rows >= 1 && rows <= kBnMaxRows, wd.bad_count);
  SFM_REQUIRE(!training || rows >= 2, wd.need_two);
  SFM_REQUIRE(training || (running_mean && running_var), "eval mode needs the running statistics (null pointer argument)");
  SFM_REQUIRE(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "eps must be >= 0 and momentum in [0, 1]");
  SFM_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(stats) && aligned16(running_mean) &&
                  aligned16(running_var),
              "batch-norm operands must be 16-byte aligned");
  const size_t need = training ? bn_ws_bytes<C>(rows) : 0;
  if (need && (!workspace || workspace_bytes < need)) {
    set_error("batch-norm statistics workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  SFM_REQUIRE(!need || aligned16(workspace), "workspace must be 16-byte aligned");
  const size_t xb = (size_t)rows * 2 * C;
  const void* ws = need ? workspace : nullptr;
  SFM_REQUIRE(!overlap(stats, kStatsBytes, x, xb) && !overlap(stats, kStatsBytes, gamma, kRowBytes) &&
                  !overlap(stats, kStatsBytes, beta, kRowBytes) && !overlap(stats, kStatsBytes, running_mean, kRowBytes) &&
                  !overlap(stats, kStatsBytes, running_var, kRowBytes) && !overlap(stats, kStatsBytes, ws, need) &&
                  !overlap(ws, need, x, xb) && !overlap(ws, need, gamma, kRowBytes) && !overlap(ws, need, beta, kRowBytes) &&
                  !overlap(ws, need, running_mean, kRowBytes) && !overlap(ws, need, running_var, kRowBytes) &&
                  !overlap(running_mean, kRowBytes, x, xb) && !overlap(running_var, kRowBytes, x, xb) &&
                  !overlap(running_mean, kRowBytes, running_var, kRowBytes) &&
                  !overlap(running_mean, kRowBytes, gamma, kRowBytes) && !overlap(running_mean, kRowBytes, beta, kRowBytes) &&
                  !overlap(running_var, kRowBytes, gamma, kRowBytes) && !overlap(running_var, kRowBytes, beta, kRowBytes),
              "batch-norm statistics outputs must not alias its inputs");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(wd.stats, s);
  int nb = 0;
  if (training) {
    nb = bn_blocks<C>(rows);
    hipLaunchKernelGGL(k_bn3_stats<C>, dim3((unsigned)nb), dim3(kBnThreads), 0, s, (const unsigned short*)x, rows,
                       (double*)workspace);
    SFM_LAUNCHED();
  }
  hipLaunchKernelGGL(k_bn3_finalize<C>, dim3(1), dim3(kBnThreads), 0, s, (const double*)workspace, nb, rows, gamma, beta,
                     eps, running_mean, running_var, momentum, training, stats);
  SFM_LAUNCHED();
  return SFM_OK;
}

template <int C>
int bn_apply(const BnWords& wd, const void* x, int64_t rows, const float* stats, const void* residual, int relu,
             void* out, void* stream) {
  constexpr size_t kStatsBytes = 5 * C * sizeof(float);
  SFM_REQUIRE(x && stats && out, "null pointer argument");
  SFM_REQUIRE(relu == 0 || relu == 1, "relu must be 0 or 1");
  SFM_REQUIRE(rows >= 1 && rows <= kBnMaxRows, wd.bad_count);
  SFM_REQUIRE(aligned16(x) && aligned16(stats) && aligned16(residual) && aligned16(out),
              "batch-norm operands must be 16-byte aligned");
  const size_t xb = (size_t)rows * 2 * C;
  SFM_REQUIRE(!overlap(out, xb, x, xb) && !overlap(out, xb, residual, xb) && !overlap(out, xb, stats, kStatsBytes),
              "batch-norm output must not alias its inputs");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(wd.apply, s);
  const int64_t items = rows * BnShape<C>::kLanes;
  const dim3 grid(apply_grid(items, kBnApplyBlocks)), block(kBnThreads);
  const unsigned short* xp = (const unsigned short*)x;
  const unsigned short* rp = (const unsigned short*)residual;
  unsigned short* op = (unsigned short*)out;
  if (relu && rp) hipLaunchKernelGGL((k_bn3_apply<C, true, true>), grid, block, 0, s, xp, items, stats, rp, op);
  else if (relu) hipLaunchKernelGGL((k_bn3_apply<C, true, false>), grid, block, 0, s, xp, items, stats, rp, op);
  else if (rp) hipLaunchKernelGGL((k_bn3_apply<C, false, true>), grid, block, 0, s, xp, items, stats, rp, op);
  else hipLaunchKernelGGL((k_bn3_apply<C, false, false>), grid, block, 0, s, xp, items, stats, rp, op);
  SFM_LAUNCHED();
  return SFM_OK;
}

template <int C>
int bn_backward(const BnWords& wd, const void* x, const void* grad_out, int64_t rows, const float* stats, int relu,
                int training, void* grad_x, float* grad_gamma_beta, void* workspace, size_t workspace_bytes,
                void* stream) {
  constexpr size_t kStatsBytes = 5 * C * sizeof(float), kRowBytes = C * sizeof(float);
  SFM_REQUIRE(x && grad_out && stats && grad_gamma_beta, "null pointer argument");
  SFM_REQUIRE((relu == 0 || relu == 1) && (training == 0 || training == 1), "relu and training must be 0 or 1");
  SFM_REQUIRE(rows >= 1 && rows <= kBnMaxRows, wd.bad_count);
  SFM_REQUIRE(!training || rows >= 2, wd.need_two);
  SFM_REQUIRE(aligned16(x) && aligned16(grad_out) && aligned16(stats) && aligned16(grad_x) && aligned16(grad_gamma_beta),
              "batch-norm operands must be 16-byte aligned");
  const size_t need = bn_ws_bytes<C>(rows);
  if (!workspace || workspace_bytes < need) {
    set_error("batch-norm backward workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  SFM_REQUIRE(aligned16(workspace), "workspace must be 16-byte aligned");
  const size_t xb = (size_t)rows * 2 * C, gb = 2 * kRowBytes;
  SFM_REQUIRE(!overlap(grad_x, xb, x, xb) && !overlap(grad_x, xb, grad_out, xb) && !overlap(grad_x, xb, stats, kStatsBytes) &&
                  !overlap(grad_x, xb, grad_gamma_beta, gb) && !overlap(grad_x, xb, workspace, need) &&
                  !overlap(grad_gamma_beta, gb, x, xb) && !overlap(grad_gamma_beta, gb, grad_out, xb) &&
                  !overlap(grad_gamma_beta, gb, stats, kStatsBytes) && !overlap(grad_gamma_beta, gb, workspace, need) &&
                  !overlap(workspace, need, x, xb) && !overlap(workspace, need, grad_out, xb) &&
                  !overlap(workspace, need, stats, kStatsBytes),
              "batch-norm backward outputs must not alias its inputs");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(wd.bwd, s);
  const int nb = bn_blocks<C>(rows);
  const unsigned short* xp = (const unsigned short*)x;
  const unsigned short* gp = (const unsigned short*)grad_out;
  double* part = (double*)workspace;
  if (relu) hipLaunchKernelGGL((k_bn3_bwd_reduce<C, true>), dim3((unsigned)nb), dim3(kBnThreads), 0, s, xp, gp, rows, stats, part);
  else hipLaunchKernelGGL((k_bn3_bwd_reduce<C, false>), dim3((unsigned)nb), dim3(kBnThreads), 0, s, xp, gp, rows, stats, part);
  SFM_LAUNCHED();
  // without grad_x one block: the ordered sum and the two parameter gradients
  const dim3 grid(grad_x ? apply_grid(rows * BnShape<C>::kLanes, kBnBwdApplyBlocks) : 1u), block(kBnThreads);
  unsigned short* gx = (unsigned short*)grad_x;
  if (relu && training)
    hipLaunchKernelGGL((k_bn3_bwd_apply<C, true, true>), grid, block, 0, s, xp, gp, rows, stats, part, nb, gx, grad_gamma_beta);
  else if (relu)
    hipLaunchKernelGGL((k_bn3_bwd_apply<C, true, false>), grid, block, 0, s, xp, gp, rows, stats, part, nb, gx, grad_gamma_beta);
  else if (training)
    hipLaunchKernelGGL((k_bn3_bwd_apply<C, false, true>), grid, block, 0, s, xp, gp, rows, stats, part, nb, gx, grad_gamma_beta);
  else
    hipLaunchKernelGGL((k_bn3_bwd_apply<C, false, false>), grid, block, 0, s, xp, gp, rows, stats, part, nb, gx, grad_gamma_beta);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace
}  // namespace sfm
