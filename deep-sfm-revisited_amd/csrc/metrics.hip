// Validation depth metrics on CDNA4 (gfx950): main.py:565-593 (mask, median
// scale, clamp) and evaluate_metric (main.py:727-747, demon_metrics.py:63,130)
// as one small row of sums per pair, with no host synchronisation.
//
//   k_metrics_hist    one radix-select pass: a histogram of one digit of the
//                     order-preserving u32 keys of gt and p0 = pred * rescale
//                     over the pair's selected pixels (digits of 11 + 11 + 10
//                     bits, most significant first).  Pass 0 also counts the
//                     masked pixels and the NaNs.  Integer atomics only.
//   k_metrics_select  picks the bin that holds the lower median's rank
//                     ((n - 1) / 2) and narrows the key prefix.
//   k_metrics_accum   p = clamp(p0 * (med_gt / med_p)); per-chunk partial sums
//                     of the metric terms (float64) and counts; depth_out.
//   k_metrics_final   sums the chunk partials in chunk order, writes the row.
//
// A pair with an empty mask takes the reference's `except` branch
// (main.py:582): its medians run over the whole image.  Its masked count is
// known only after pass 0, so pass 0 is launched a second time for the
// "whole image" selection; those blocks leave at once unless the count is 0.
//
// A chunk is kChunk consecutive pixels of one pair, whatever the batch or the
// grid, and every reduction runs in a fixed order, so a pair's row depends on
// that pair's pixels, H and W alone.
//
// Loads are 4-byte and coalesced (a wave reads 256 contiguous bytes): neither
// a pair's base (H*W odd) nor a row of the strided pred view is 16-byte
// aligned in general.
#include <string>
#include "common.h"

namespace sfm {

constexpr int kMetThreads = 256;
constexpr int kMetPerThread = 16;
constexpr int kChunk = kMetThreads * kMetPerThread;   // pixels per block: a compile-time constant
constexpr int kBins = 2048;
constexpr int kPartial = 9;        // doubles per chunk: six sums, three counts
constexpr int kAggRounds = 6;      // wave-aggregated rounds before plain LDS atomics

// per-pair selection state (u32 words)
enum {
  ST_N = 0,          // masked count
  ST_NAN_GT = 1,     // NaNs among the selected gt / p0
  ST_NAN_P = 2,
  ST_PREFIX_GT = 3,  // key prefix found so far
  ST_PREFIX_P = 4,
  ST_RANK_GT = 5,    // rank still to find inside the prefix
  ST_RANK_P = 6,
  ST_WORDS = 8
};

struct MetArgs {
  const float* pred;
  int64_t pred_bs;
  int pred_rs;
  const float* gt;
  int H, W;
  const float* rescale;
  int mode, y0, y1, x0, x1;
};

__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ bool in_mask(const MetArgs& a, float g, int y, int x) {
  if (a.mode == 0) return g > 0.0f && g < 80.0f && y >= a.y0 && y < a.y1 && x >= a.x0 && x < a.x1;
  return g >= 0.5f && g <= 10.0f;
}

// One pixel of pair b: gt and p0 (main.py:541), and whether the mask holds.
__device__ __forceinline__ void load_pixel(const MetArgs& a, int b, int i, float& g, float& p0, bool& m) {
  const int y = i / a.W, x = i - y * a.W;
  g = a.gt[(size_t)b * a.H * a.W + i];
  p0 = a.pred[(size_t)b * a.pred_bs + (size_t)y * a.pred_rs + x];
  if (a.rescale) p0 = p0 * a.rescale[b];
  m = in_mask(a, g, y, x);
}

// Add one to hist[bin] for every lane with `on`.  Lanes of a wave that share a
// bin (nearby pixels mostly do in the top-digit pass) are counted by one lane.
__device__ __forceinline__ void hist_add(uint32_t* hist, bool on, uint32_t bin, bool aggregate) {
  if (aggregate) {
    for (int r = 0; r < kAggRounds; ++r) {
      const unsigned long long live = __ballot(on);
      if (live == 0ull) return;
      const int lead = __ffsll((long long)live) - 1;
      const uint32_t lb = (uint32_t)__shfl((int)bin, lead);
      const bool same = on && bin == lb;
      const unsigned long long grp = __ballot(same);
      if ((int)(threadIdx.x & 63) == lead) atomicAdd(&hist[lb], (uint32_t)__popcll(grp));
      on = on && !same;
    }
  }
  if (on) atomicAdd(&hist[bin], 1u);
}

// grid (chunks, B).  pass 0..2; whole = 1: the launch for pairs with an empty mask.
__global__ __launch_bounds__(kMetThreads) void k_metrics_hist(MetArgs a, int pass, int whole, uint32_t* __restrict__ state,
                                                              uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[2][kBins];
  __shared__ uint32_t lcount[3];
  const int b = blockIdx.y;
  uint32_t* st = state + (size_t)b * ST_WORDS;
  const bool first = pass == 0 && !whole;
  const bool all = first ? false : st[ST_N] == 0u;      // written by the launches before this one
  if (whole && !all) return;
  const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
  const uint32_t digit_mask = pass == 2 ? 1023u : 2047u;
  const uint32_t pre_gt = st[ST_PREFIX_GT], pre_p = st[ST_PREFIX_P];
  for (int i = threadIdx.x; i < kBins; i += kMetThreads) { lh[0][i] = 0u; lh[1][i] = 0u; }
  if (threadIdx.x < 3) lcount[threadIdx.x] = 0u;
  __syncthreads();
  const int hw = a.H * a.W;
  const int base = blockIdx.x * kChunk;
  uint32_t n = 0, nan_g = 0, nan_p = 0;
  for (int j = 0; j < kMetPerThread; ++j) {
    const int i = base + j * kMetThreads + threadIdx.x;
    bool sel = false;
    float g = 0.0f, p0 = 0.0f;
    if (i < hw) {
      bool m;
      load_pixel(a, b, i, g, p0, m);
      sel = all || m;
    }
    const uint32_t kg = order_key(g), kp = order_key(p0);
    bool on_g = sel, on_p = sel;
    if (pass > 0) {            // only keys inside the prefix found so far
      on_g = on_g && (kg >> (shift + (pass == 1 ? 11 : 10))) == pre_gt;
      on_p = on_p && (kp >> (shift + (pass == 1 ? 11 : 10))) == pre_p;
    } else if (sel) {
      n += 1u;
      nan_g += g != g ? 1u : 0u;
      nan_p += p0 != p0 ? 1u : 0u;
    }
    hist_add(lh[0], on_g, (kg >> shift) & digit_mask, pass == 0);
    hist_add(lh[1], on_p, (kp >> shift) & digit_mask, pass == 0);
  }
  if (pass == 0) {
    if (n) atomicAdd(&lcount[0], n);
    if (nan_g) atomicAdd(&lcount[1], nan_g);
    if (nan_p) atomicAdd(&lcount[2], nan_p);
  }
  __syncthreads();
  uint32_t* gh = hist + ((size_t)b * 3 + pass) * 2 * kBins;
  for (int i = threadIdx.x; i < 2 * kBins; i += kMetThreads) {
    const uint32_t v = lh[i / kBins][i % kBins];
    if (v) atomicAdd(&gh[i], v);
  }
  if (pass == 0 && threadIdx.x < 3 && lcount[threadIdx.x]) {
    // the masked count only from the masked launch (it decides `all`); NaN counts from whichever ran
    if (threadIdx.x > 0 || first) atomicAdd(&st[threadIdx.x == 0 ? ST_N : threadIdx.x], lcount[threadIdx.x]);
  }
}

// grid (2, B): x = 0 gt, 1 p0.  One block scans the 2048 bins of this pass.
__global__ __launch_bounds__(kMetThreads) void k_metrics_select(int pass, int hw, uint32_t* __restrict__ state,
                                                                const uint32_t* __restrict__ hist) {
  __shared__ uint32_t part[kMetThreads];
  const int b = blockIdx.y, which = blockIdx.x;
  uint32_t* st = state + (size_t)b * ST_WORDS;
  const uint32_t* h = hist + (((size_t)b * 3 + pass) * 2 + which) * kBins;
  constexpr int kPer = kBins / kMetThreads;
  uint32_t mine[kPer];
  uint32_t s = 0;
  for (int k = 0; k < kPer; ++k) {
    mine[k] = h[threadIdx.x * kPer + k];
    s += mine[k];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  uint32_t rank;
  if (pass == 0) {
    const uint32_t n = st[ST_N];
    rank = ((n ? n : (uint32_t)hw) - 1u) / 2u;        // torch's lower median
  } else {
    rank = st[ST_RANK_GT + which];
  }
  uint32_t before = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
  __syncthreads();                                     // every thread has read the old rank
  if (rank >= before && rank < before + s) {           // exactly one thread
    uint32_t cum = before;
    int k = 0;
    while (k < kPer - 1 && rank >= cum + mine[k]) { cum += mine[k]; ++k; }
    const uint32_t bin = (uint32_t)(threadIdx.x * kPer + k);
    const uint32_t pre = pass == 0 ? 0u : st[ST_PREFIX_GT + which];
    st[ST_PREFIX_GT + which] = (pre << (pass == 2 ? 10 : 11)) | bin;
    st[ST_RANK_GT + which] = rank - cum;
  }
}

__device__ __forceinline__ void pair_scale(const uint32_t* st, float& med_gt, float& med_p, float& scale) {
  const float nanf_ = __uint_as_float(0x7fc00000u);
  med_gt = st[ST_NAN_GT] ? nanf_ : key_value(st[ST_PREFIX_GT]);
  med_p = st[ST_NAN_P] ? nanf_ : key_value(st[ST_PREFIX_P]);
  scale = med_gt / med_p;                               // main.py:580 / 582
}

// Fixed-order block sum: lane pairs at halving distances through LDS.
__device__ __forceinline__ double block_sum(double v, double* buf) {
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int d = kMetThreads / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) buf[threadIdx.x] = buf[threadIdx.x] + buf[threadIdx.x + d];
    __syncthreads();
  }
  const double r = buf[0];
  __syncthreads();
  return r;
}

// grid (chunks, B)
__global__ __launch_bounds__(kMetThreads) void k_metrics_accum(MetArgs a, float min_depth, float max_depth,
                                                               const uint32_t* __restrict__ state,
                                                               double* __restrict__ partial,
                                                               float* __restrict__ depth_out) {
  __shared__ double buf[kMetThreads];
  const int b = blockIdx.y;
  float med_gt, med_p, scale;
  pair_scale(state + (size_t)b * ST_WORDS, med_gt, med_p, scale);
  const int hw = a.H * a.W;
  const int base = blockIdx.x * kChunk;
  double acc[kPartial];
  for (int k = 0; k < kPartial; ++k) acc[k] = 0.0;
  for (int j = 0; j < kMetPerThread; ++j) {
    const int i = base + j * kMetThreads + threadIdx.x;
    if (i >= hw) break;
    float g, p0;
    bool m;
    load_pixel(a, b, i, g, p0, m);
    float p = p0 * scale;                               // main.py:585
    if (p <= min_depth) p = min_depth;                  // main.py:589-590; NaN fails both
    if (p > max_depth) p = max_depth;
    if (depth_out) depth_out[(size_t)b * hw + i] = p;
    if (!m) continue;
    const float d = g - p;
    const float ad = fabsf(d);
    const float dd = d * d;
    acc[0] += (double)(ad / g);
    acc[1] += (double)(dd / g);
    acc[2] += (double)dd;
    const double l = log((double)g) - log((double)p);
    acc[3] += l * l;
    acc[4] += l;
    const float q0 = g / p, q1 = p / g;                 // max(q0, q1) < t: both below t (NaN: neither)
    acc[5] += (q0 < 1.25f && q1 < 1.25f) ? 1.0 : 0.0;
    acc[6] += (q0 < 1.5625f && q1 < 1.5625f) ? 1.0 : 0.0;
    acc[7] += (q0 < 1.953125f && q1 < 1.953125f) ? 1.0 : 0.0;
    const float ig = 1.0f / g, ip = 1.0f / p;
    acc[8] += (double)fabsf(ig - ip);
  }
  double* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * kPartial;
  for (int k = 0; k < kPartial; ++k) {
    const double r = block_sum(acc[k], buf);
    if (threadIdx.x == 0) out[k] = r;
  }
}

// grid (B), 64 threads: lane k < 9 sums slot k over the chunks in chunk order.
__global__ __launch_bounds__(64) void k_metrics_final(int chunks, const uint32_t* __restrict__ state,
                                                      const double* __restrict__ partial, double* __restrict__ rows) {
  const int b = blockIdx.x;
  const uint32_t* st = state + (size_t)b * ST_WORDS;
  double* row = rows + (size_t)b * 16;
  const int k = threadIdx.x;
  if (k < kPartial) {
    double s = 0.0;
    const double* p = partial + (size_t)b * chunks * kPartial + k;
    for (int c = 0; c < chunks; ++c) s += p[(size_t)c * kPartial];
    row[4 + k] = s;
  } else if (k < 12) {
    row[4 + k] = 0.0;                                   // slots 13..15
  } else if (k == 12) {
    float med_gt, med_p, scale;
    pair_scale(st, med_gt, med_p, scale);
    row[0] = (double)st[ST_N];
    row[1] = (double)med_gt;
    row[2] = (double)med_p;
    row[3] = (double)scale;
  }
}

static int met_chunks(int H, int W) { return (int)(((int64_t)H * W + kChunk - 1) / kChunk); }

static size_t met_head_bytes(int B) {        // state + histograms: zeroed by every call
  return (size_t)B * (ST_WORDS + 3 * 2 * kBins) * sizeof(uint32_t);
}

static size_t met_ws_bytes(int B, int H, int W) {
  const size_t head = (met_head_bytes(B) + 255) & ~(size_t)255;
  return head + (size_t)B * met_chunks(H, W) * kPartial * sizeof(double);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_depth_metrics_workspace_bytes(int batch, int H, int W) {
  if (batch < 1 || H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30)) return 0;
  return met_ws_bytes(batch, H, W);
}

int sfm_depth_metrics(const float* pred, int64_t pred_batch_stride, int pred_row_stride, const float* gt, int batch,
                      int H, int W, const float* rescale, int mask_mode, int y0, int y1, int x0, int x1,
                      float min_depth, float max_depth, double* rows, float* depth_out, void* workspace,
                      size_t workspace_bytes, void* stream) {
  SFM_REQUIRE(pred && gt && rows, "null pointer argument (pred, gt, rows)");
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 30),
              "invalid depth-metrics shape");
  SFM_REQUIRE(pred_row_stride >= W, "pred_row_stride is smaller than W");
  SFM_REQUIRE(pred_batch_stride >= (int64_t)H * pred_row_stride, "pred_batch_stride is smaller than H * pred_row_stride");
  SFM_REQUIRE(mask_mode == 0 || mask_mode == 1, "mask_mode must be 0 (KITTI) or 1 (DeMoN)");
  SFM_REQUIRE(mask_mode == 1 || (y0 >= 0 && y0 <= y1 && y1 <= H && x0 >= 0 && x0 <= x1 && x1 <= W),
              "crop rectangle outside the image");
  SFM_REQUIRE(min_depth > 0.0f && max_depth >= min_depth, "depth range: need 0 < min_depth <= max_depth");
  const size_t need = met_ws_bytes(batch, H, W);
  if (!workspace || workspace_bytes < need) {
    set_error("depth-metrics workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("depth_metrics", s);
  const int chunks = met_chunks(H, W);
  const size_t head = met_head_bytes(batch);
  uint32_t* state = (uint32_t*)workspace;
  uint32_t* hist = state + (size_t)batch * ST_WORDS;
  double* partial = (double*)((char*)workspace + ((head + 255) & ~(size_t)255));
  SFM_HIP(hipMemsetAsync(workspace, 0, head, s));
  MetArgs a{pred, pred_batch_stride, pred_row_stride, gt, H, W, rescale, mask_mode, y0, y1, x0, x1};
  const dim3 grid(chunks, batch), block(kMetThreads);
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(k_metrics_hist, grid, block, 0, s, a, pass, 0, state, hist);
    if (pass == 0) hipLaunchKernelGGL(k_metrics_hist, grid, block, 0, s, a, 0, 1, state, hist);
    hipLaunchKernelGGL(k_metrics_select, dim3(2, batch), block, 0, s, pass, H * W, state, hist);
  }
  hipLaunchKernelGGL(k_metrics_accum, grid, block, 0, s, a, min_depth, max_depth, state, partial, depth_out);
  hipLaunchKernelGGL(k_metrics_final, dim3(batch), dim3(64), 0, s, chunks, state, partial, rows);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
