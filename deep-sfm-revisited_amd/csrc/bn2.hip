// BatchNorm2d, ReLU and the residual add of the feature CNN in float16, forward
// and backward (models/submodule.py:11-14 convbn; the BasicBlock of :22-44):
// what stands between two sfm_conv2x_f16 layers of a training step.
//
// x is [pixels][channels] float16, channels last, channels 32, 64 or 128.  The
// entry points only: the kernels and the checked launchers are bn_act.h's, the
// ones sfm_bn3_* runs at 32 channels.
#include "bn_act.h"

using namespace sfm;

namespace {
const BnWords kWords = {"invalid pixel count",
                        "training-mode batch statistics need more than one value per channel (pixels >= 2)",
                        "bn2_stats", "bn2_apply", "bn2_bwd"};

bool channels_ok(int c) { return c == 32 || c == 64 || c == 128; }

size_t ws_bytes(int64_t pixels, int channels) {
  return channels == 32 ? bn_ws_bytes<32>(pixels) : channels == 64 ? bn_ws_bytes<64>(pixels) : bn_ws_bytes<128>(pixels);
}
}  // namespace

extern "C" {

size_t sfm_bn2_stats_f16_workspace_bytes(int64_t pixels, int channels, int training) {
  if (pixels < 1 || pixels > kBnMaxRows || !channels_ok(channels) || !training) return 0;
  return ws_bytes(pixels, channels);
}

int sfm_bn2_stats_f16(const void* x, int64_t pixels, int channels, const float* gamma, const float* beta, double eps,
                      float* running_mean, float* running_var, double momentum, int training, float* stats,
                      void* workspace, size_t workspace_bytes, void* stream) {
  SFM_REQUIRE(channels_ok(channels), "channels must be 32, 64 or 128");
  if (channels == 32)
    return bn_stats<32>(kWords, x, pixels, gamma, beta, eps, running_mean, running_var, momentum, training, stats,
                        workspace, workspace_bytes, stream);
  if (channels == 64)
    return bn_stats<64>(kWords, x, pixels, gamma, beta, eps, running_mean, running_var, momentum, training, stats,
                        workspace, workspace_bytes, stream);
  return bn_stats<128>(kWords, x, pixels, gamma, beta, eps, running_mean, running_var, momentum, training, stats,
                       workspace, workspace_bytes, stream);
}

int sfm_bn2_apply_f16(const void* x, int64_t pixels, int channels, const float* stats, const void* residual, int relu,
                      void* out, void* stream) {
  SFM_REQUIRE(channels_ok(channels), "channels must be 32, 64 or 128");
  if (channels == 32) return bn_apply<32>(kWords, x, pixels, stats, residual, relu, out, stream);
  if (channels == 64) return bn_apply<64>(kWords, x, pixels, stats, residual, relu, out, stream);
  return bn_apply<128>(kWords, x, pixels, stats, residual, relu, out, stream);
}

size_t sfm_bn2_backward_f16_workspace_bytes(int64_t pixels, int channels) {
  if (pixels < 1 || pixels > kBnMaxRows || !channels_ok(channels)) return 0;
  return ws_bytes(pixels, channels);
}

int sfm_bn2_backward_f16(const void* x, const void* grad_out, int64_t pixels, int channels, const float* stats, int relu,
                         int training, void* grad_x, float* grad_gamma_beta, void* workspace, size_t workspace_bytes,
                         void* stream) {
  SFM_REQUIRE(channels_ok(channels), "channels must be 32, 64 or 128");
  if (channels == 32)
    return bn_backward<32>(kWords, x, grad_out, pixels, stats, relu, training, grad_x, grad_gamma_beta, workspace,
                           workspace_bytes, stream);
  if (channels == 64)
    return bn_backward<64>(kWords, x, grad_out, pixels, stats, relu, training, grad_x, grad_gamma_beta, workspace,
                           workspace_bytes, stream);
  return bn_backward<128>(kWords, x, grad_out, pixels, stats, relu, training, grad_x, grad_gamma_beta, workspace,
                          workspace_bytes, stream);
}

}  // extern "C"
