// The float16 weight gradient of a 2-D convolution (conv2_wgrad.hip): the
// launch plan, the workspace size and the launcher that sfm_conv2_wgrad_f16
// (context_bwd.hip) and sfm_conv2x_wgrad_f16 (feature_bwd.hip) share.  The
// entry points check their own arguments; nothing here does.
#pragma once
#include "common.h"

namespace sfm {

// the channel counts of the 2-D backward kernels: an output (and the context stack's input) of one to four
// 32-channel groups; the feature CNN's input up to lastconv.0's 320
inline bool chan_ok(int c) { return c == 32 || c == 64 || c == 96 || c == 128; }
inline bool cin_ok(int c) { return c >= 32 && c <= 320 && c % 32 == 0; }

struct XwPlan {
  int hout, wout, ntx, nty, blocks, ng;
  int64_t ntiles;
};

#pragma GCC visibility push(hidden)
// ksize 3 or 1, stride 1 or 2; reads the conv2_wgrad_blocks tuning key
XwPlan xw_plan(int images, int cout, int hin, int win, int ksize, int stride);
size_t xw_ws_bytes(const XwPlan& p, int cin, int cout, int ksize);
// k_conv2_wgrad's partials into `workspace` (xw_ws_bytes), then k_conv2_wgrad_reduce into grad_weights
// [ksize^2][cout][cin]: two launches on s.  dil is 1 unless ksize 3 and stride 1.
int launch_conv2_wgrad(hipStream_t s, const XwPlan& p, const void* in, const void* grad_out, int cin, int cout,
                       int hin, int win, int ksize, int stride, int dil, void* workspace, float* grad_weights);
#pragma GCC visibility pop

}  // namespace sfm
