// Interpolation helpers of the soft-argmin depth head, shared by its forward
// (depth.hip, k_depth_head) and its backward (depth_bwd.hip): the backward
// recomputes the forward's interpolated logits from these, so its softmax has
// the forward's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace sfm {

struct HeadTaps {
  int o00, o01, o10, o11;
  double wx0, wx1, wy0, wy1;
};

// F.interpolate(..., mode='trilinear', align_corners=False) source index and
// weights along one axis (PyTorch's area_pixel_compute_source_index with
// guard_index_and_lambda; identity when the sizes match).  In float64: a
// float32 weight is off by about 1e-6, and the classify logits differ by
// O(100) between neighbouring taps, which moved the soft-argmin by up to 2e-4
// of the depth against the exact interpolation (tests/test_gpu_depth.py).
__device__ __forceinline__ void axis_weights(int dst, int in_size, int out_size, double ratio, int& i0, int& i1,
                                             double& l0, double& l1) {
  if (in_size == out_size) {
    i0 = i1 = dst;
    l0 = 1.0;
    l1 = 0.0;
    return;
  }
  double src = ratio * ((double)dst + 0.5) - 0.5;
  if (src < 0.0) src = 0.0;
  i0 = min((int)floor(src), in_size - 1);
  l1 = fmin(fmax(src - (double)i0, 0.0), 1.0);
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l0 = 1.0 - l1;
}

// interpolated cost of plane l (PyTorch's nested order: ((x00 wx0 + x01 wx1) wy0 + (x10 wx0 + x11 wx1) wy1)),
// float32 taps combined in float64
__device__ __forceinline__ double head_value(const float* __restrict__ plane, const HeadTaps& t) {
  const double r0 = (double)plane[t.o00] * t.wx0 + (double)plane[t.o01] * t.wx1;
  const double r1 = (double)plane[t.o10] * t.wx0 + (double)plane[t.o11] * t.wx1;
  return r0 * t.wy0 + r1 * t.wy1;
}

// axis_weights' i0 for in_size != out_size, on the host too (the same double operations)
__host__ __device__ inline int head_tap0(int dst, int in_size, double ratio) {
  double src = ratio * ((double)dst + 0.5) - 0.5;
  if (src < 0.0) src = 0.0;
  const int f = (int)floor(src);
  return f < in_size - 1 ? f : in_size - 1;
}

// The first output index whose tap 0 is `cell` or beyond (out_size if none).  head_tap0 is monotone in dst, so
// the estimate from the inverse map is walked to the exact boundary of the forward's own rounding.
__host__ __device__ inline int head_first_at_or_beyond(int cell, int in_size, int out_size, double ratio) {
  if (cell <= 0) return 0;
  if (cell >= in_size) return out_size;
  const double t = ceil(((double)cell + 0.5) / ratio - 0.5);
  int d = t < 0.0 ? 0 : (t > (double)out_size ? out_size : (int)t);
  while (d > 0 && head_tap0(d - 1, in_size, ratio) >= cell) --d;
  while (d < out_size && head_tap0(d, in_size, ratio) < cell) ++d;
  return d;
}

// The output indices along one axis whose taps include `cell` (the transpose of axis_weights): the run
// [first0, first0 + count0) has it as tap 0 (weight l0), the run [first1, first1 + count1) as tap 1 (weight
// l1).  Tap 1 of an output index is the cell after its tap 0, or the same cell at the last index (where the
// cell receives l0 + l1), and its own cell when the sizes match.  An empty run has count 0 (downsampling).
__host__ __device__ inline void head_contributors(int in_size, int out_size, int cell, int& first0, int& count0,
                                                  int& first1, int& count1) {
  if (in_size == out_size) {
    first0 = first1 = cell;
    count0 = count1 = 1;
    return;
  }
  const double ratio = (double)in_size / (double)out_size;
  const int a = head_first_at_or_beyond(cell - 1, in_size, out_size, ratio);
  const int b = head_first_at_or_beyond(cell, in_size, out_size, ratio);
  const int c = head_first_at_or_beyond(cell + 1, in_size, out_size, ratio);
  first0 = b;
  count0 = c - b;
  // tap 1: the indices whose tap 0 is the cell before, and at the last cell its own as well
  first1 = cell > 0 ? a : b;
  count1 = (cell == in_size - 1 ? out_size : b) - first1;
}

}  // namespace sfm
