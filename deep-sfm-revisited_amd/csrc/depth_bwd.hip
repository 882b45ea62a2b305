// Backward of the soft-argmin depth head into the cost volume (gfx950):
// the gradient autograd forms in the reference's training loop through
// F.interpolate(trilinear), F.softmax and disparityregression /
// depthregression (models/PSNet.py:194-216, models/submodule.py:57-93).
//
// With v_l the forward's interpolated logit of plane l at the output pixel
// (b, Y, X) (depth_head.h: float32 taps combined in float64 with axis_weights'
// weights in head_value's nesting), m = max_l v_l, e_l = expf((float)(v_l - m)),
// s = sum_l e_l, p_l = e_l / s, val_l = (float)(l + 1) step, reg = sum_l p_l val_l
// and d = grad_depth dout/dreg (min_depth in depth mode,
// -(min_depth L) / (reg + 1e-16)^2 in disparity mode):
//
//   grad_cost[b, l, y, x] = sum over (Y, X) whose taps include (y, x) of
//                           d p_l (val_l - reg) wy wx
//
// where wy (wx) is the weight the forward gave row y (column x) at Y (X): l0
// as tap 0, l1 as tap 1, l0 + l1 where both taps are the cell (the clamped last
// index).  The helpers are the forward's own, so p_l has the forward's bits and
// the result is the exact transpose of k_depth_head.
//
// A gather in two launches, no atomics:
//   k_depth_head_stats   one thread per output pixel repeats the forward's two
//                        passes and writes (m, reg, d / s) as float64 into the
//                        workspace (24 bytes per pixel).
//   k_depth_head_bwd     one thread per low-resolution cell and chunk of
//                        kHeadBwdPlanes planes.  The output indices that read a
//                        cell along one axis are a contiguous run
//                        (head_contributors: the source index is monotone in the
//                        output index), about 2 H/h x 2 W/w pixels.  The thread
//                        walks them row by row in ascending order, recomputes
//                        v_l and e_l from the four taps (neighbouring threads
//                        read neighbouring taps: L1 / L2), accumulates in
//                        float64 and stores one float per plane.
// One thread owns an element and sums in a fixed order, so the result is
// reproducible bit for bit from run to run.  A cell no output pixel reads
// (downsampling) gets exactly 0.
#include <string>
#include "common.h"
#include "depth_head.h"

namespace sfm {

constexpr int kHeadBwdThreads = 256;
// planes per thread, sized as kCorrPlanes (depth.hip): a contributor's weights, taps and workspace record
// are formed once and serve this many planes
constexpr int kHeadBwdPlanes = 8;

static size_t head_bwd_ws_bytes(int B, int H, int W) {
  const size_t plane = ((size_t)B * H * W * sizeof(double) + 255) & ~(size_t)255;
  return 3 * plane;
}

// grid (ceil(W / 256), H, B); thread = output pixel.  The two passes are k_depth_head's.
__global__ __launch_bounds__(kHeadBwdThreads) void k_depth_head_stats(
    const float* __restrict__ cost, const float* __restrict__ grad_depth, int L, int h, int w, int H, int W,
    double ratio_h, double ratio_w, int depth_mode, float min_depth, float step, double* __restrict__ ws_m,
    double* __restrict__ ws_reg, double* __restrict__ ws_k) {
  const int b = blockIdx.z, Y = blockIdx.y;
  const int X = blockIdx.x * kHeadBwdThreads + threadIdx.x;
  if (X >= W) return;
  HeadTaps t;
  int y0, y1, x0, x1;
  axis_weights(Y, h, H, ratio_h, y0, y1, t.wy0, t.wy1);
  axis_weights(X, w, W, ratio_w, x0, x1, t.wx0, t.wx1);
  t.o00 = y0 * w + x0; t.o01 = y0 * w + x1;
  t.o10 = y1 * w + x0; t.o11 = y1 * w + x1;
  const size_t hw = (size_t)h * w;
  const float* cb = cost + (size_t)b * L * hw;
  double m = -INFINITY;
  for (int l = 0; l < L; ++l) m = fmax(m, head_value(cb + l * hw, t));
  double s = 0.0, ws = 0.0;
  for (int l = 0; l < L; ++l) {
    const double e = (double)expf((float)(head_value(cb + l * hw, t) - m));
    s = s + e;
    ws = ws + e * (double)((float)(l + 1) * step);
  }
  const double reg = ws / s;
  const size_t o = ((size_t)b * H + Y) * W + X;
  const double g = (double)grad_depth[o];
  double d;
  if (depth_mode) {
    d = g * (double)min_depth;                                                   // out = reg min_depth
  } else {
    const double q = reg + 1e-16;                                                // out = min_depth L / (reg + 1e-16)
    d = g * (-((double)min_depth * (double)L) / (q * q));
  }
  ws_m[o] = m;
  ws_reg[o] = reg;
  ws_k[o] = d / s;
}

// the weight axis_weights gave `cell` at output index dst: l0 as tap 0 plus l1 as tap 1
__device__ __forceinline__ double cell_weight(int cell, int i0, int i1, double l0, double l1) {
  return (i0 == cell ? l0 : 0.0) + (i1 == cell ? l1 : 0.0);
}

// the union of a cell's two contributor runs (adjacent or nested, depth_head.h): [first, end)
__device__ __forceinline__ void contributor_span(int in_size, int out_size, int cell, int& first, int& end) {
  int f0, c0, f1, c1;
  head_contributors(in_size, out_size, cell, f0, c0, f1, c1);
  first = out_size;
  end = 0;
  if (c0 > 0) { first = min(first, f0); end = max(end, f0 + c0); }
  if (c1 > 0) { first = min(first, f1); end = max(end, f1 + c1); }
}

// grid (ceil(h w / 256), ceil(L / kHeadBwdPlanes), B); thread = low-resolution cell, x fastest
__global__ __launch_bounds__(kHeadBwdThreads) void k_depth_head_bwd(
    const float* __restrict__ cost, int L, int h, int w, int H, int W, double ratio_h, double ratio_w, float step,
    const double* __restrict__ ws_m, const double* __restrict__ ws_reg, const double* __restrict__ ws_k,
    float* __restrict__ grad_cost) {
  const int b = blockIdx.z;
  const int hw = h * w;
  const int p = blockIdx.x * kHeadBwdThreads + threadIdx.x;
  if (p >= hw) return;
  const int y = p / w, x = p - y * w;
  const int l0 = blockIdx.y * kHeadBwdPlanes;
  const int nl = min(L - l0, kHeadBwdPlanes);
  const float* cb = cost + ((size_t)b * L + l0) * hw;
  int Y0, Y1, X0, X1;
  contributor_span(h, H, y, Y0, Y1);
  contributor_span(w, W, x, X0, X1);
  double acc[kHeadBwdPlanes];
#pragma unroll
  for (int j = 0; j < kHeadBwdPlanes; ++j) acc[j] = 0.0;
  for (int Y = Y0; Y < Y1; ++Y) {
    HeadTaps t;
    int ya, yb;
    axis_weights(Y, h, H, ratio_h, ya, yb, t.wy0, t.wy1);
    const double wy = cell_weight(y, ya, yb, t.wy0, t.wy1);
    const size_t row = ((size_t)b * H + Y) * W;
    for (int X = X0; X < X1; ++X) {
      int xa, xb;
      axis_weights(X, w, W, ratio_w, xa, xb, t.wx0, t.wx1);
      const double wx = cell_weight(x, xa, xb, t.wx0, t.wx1);
      t.o00 = ya * w + xa; t.o01 = ya * w + xb;
      t.o10 = yb * w + xa; t.o11 = yb * w + xb;
      const double m = ws_m[row + X], reg = ws_reg[row + X];
      const double k = ws_k[row + X] * (wy * wx);
#pragma unroll
      for (int j = 0; j < kHeadBwdPlanes; ++j) {
        if (j < nl) {
          const double e = (double)expf((float)(head_value(cb + (size_t)j * hw, t) - m));
          const double val = (double)((float)(l0 + j + 1) * step);
          acc[j] = acc[j] + (k * e) * (val - reg);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kHeadBwdPlanes; ++j)
    if (j < nl) grad_cost[((size_t)b * L + l0 + j) * hw + p] = (float)acc[j];
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_depth_head_backward_workspace_bytes(int batch, int H, int W) {
  if (batch < 1 || H < 1 || W < 1) return 0;
  return head_bwd_ws_bytes(batch, H, W);
}

int sfm_depth_head_contributors(int in_size, int out_size, int cell, int* first0, int* count0, int* first1,
                                int* count1) {
  SFM_REQUIRE(first0 && count0 && first1 && count1, "null pointer argument");
  SFM_REQUIRE(in_size >= 1 && out_size >= 1 && cell >= 0 && cell < in_size, "invalid axis sizes or cell");
  head_contributors(in_size, out_size, cell, *first0, *count0, *first1, *count1);
  return SFM_OK;
}

int sfm_depth_head_backward(const float* cost, const float* grad_depth, int batch, int nlabel, int h, int w, int H,
                            int W, int depth_mode, float min_depth, float depth_step, float* grad_cost,
                            void* workspace, size_t workspace_bytes, void* stream) {
  SFM_REQUIRE(cost && grad_depth && grad_cost, "null pointer argument");
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && nlabel >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && H <= 65535,
              "invalid depth-head shape");
  SFM_REQUIRE(depth_mode == 0 || depth_mode == 1, "depth_mode must be 0 (disparity) or 1 (depth)");
  SFM_REQUIRE(depth_mode == 0 || depth_step > 0.0f, "depth regression needs a positive step");
  SFM_REQUIRE((int64_t)nlabel * h * w < ((int64_t)1 << 31), "cost volume too large");
  // the grid's y counts chunks of planes
  SFM_REQUIRE((nlabel + kHeadBwdPlanes - 1) / kHeadBwdPlanes <= 65535, "too many planes");
  SFM_REQUIRE((const float*)grad_cost != cost, "grad_cost must not alias cost");
  const size_t need = head_bwd_ws_bytes(batch, H, W);
  if (!workspace || workspace_bytes < need) {
    set_error("depth-head backward workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  SFM_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* ws_m = (double*)workspace;
  double* ws_reg = (double*)((char*)workspace + need / 3);
  double* ws_k = (double*)((char*)workspace + 2 * (need / 3));
  const double ratio_h = (double)h / (double)H, ratio_w = (double)w / (double)W;   // as sfm_depth_head
  const float step = depth_mode ? depth_step : 1.0f;
  {
    ProfScope ps("depth_head_bwd_stats", s);
    hipLaunchKernelGGL(k_depth_head_stats, dim3((W + kHeadBwdThreads - 1) / kHeadBwdThreads, H, batch),
                       dim3(kHeadBwdThreads), 0, s, cost, grad_depth, nlabel, h, w, H, W, ratio_h, ratio_w, depth_mode,
                       min_depth, step, ws_m, ws_reg, ws_k);
    SFM_LAUNCHED();
  }
  ProfScope ps("depth_head_bwd", s);
  const int hw = h * w;
  hipLaunchKernelGGL(k_depth_head_bwd,
                     dim3((hw + kHeadBwdThreads - 1) / kHeadBwdThreads, (nlabel + kHeadBwdPlanes - 1) / kHeadBwdPlanes,
                          batch),
                     dim3(kHeadBwdThreads), 0, s, cost, nlabel, h, w, H, W, ratio_h, ratio_w, step, ws_m, ws_reg, ws_k,
                     grad_cost);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
