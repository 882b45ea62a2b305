// BatchNorm3d, ReLU and the residual add of PSNet's cost regularisation in
// float16, forward and backward (models/submodule.py:17-20 convbn_3d; the
// stack of models/PSNet.py:79-102 as applied at 159-165): what stands between
// two sfm_conv3_f16 layers of a training step.
//
// x is [voxels][32] float16, channels last.  The entry points only: the kernels
// and the checked launchers are bn_act.h's, at C = 32 (four lanes cover a voxel,
// a wave covers 16 consecutive voxels).
#include "bn_act.h"

using namespace sfm;

namespace {
const BnWords kWords = {"invalid voxel count",
                        "training-mode batch statistics need more than one value per channel (voxels >= 2)",
                        "bn3_stats", "bn3_apply", "bn3_bwd"};
}

extern "C" {

size_t sfm_bn3_stats_f16_workspace_bytes(int64_t voxels, int training) {
  if (voxels < 1 || voxels > kBnMaxRows || !training) return 0;
  return bn_ws_bytes<32>(voxels);
}

int sfm_bn3_stats_f16(const void* x, int64_t voxels, const float* gamma, const float* beta, double eps,
                      float* running_mean, float* running_var, double momentum, int training, float* stats,
                      void* workspace, size_t workspace_bytes, void* stream) {
  return bn_stats<32>(kWords, x, voxels, gamma, beta, eps, running_mean, running_var, momentum, training, stats,
                      workspace, workspace_bytes, stream);
}

int sfm_bn3_apply_f16(const void* x, int64_t voxels, const float* stats, const void* residual, int relu, void* out,
                      void* stream) {
  return bn_apply<32>(kWords, x, voxels, stats, residual, relu, out, stream);
}

size_t sfm_bn3_backward_f16_workspace_bytes(int64_t voxels) {
  if (voxels < 1 || voxels > kBnMaxRows) return 0;
  return bn_ws_bytes<32>(voxels);
}

int sfm_bn3_backward_f16(const void* x, const void* grad_out, int64_t voxels, const float* stats, int relu, int training,
                         void* grad_x, float* grad_gamma_beta, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_backward<32>(kWords, x, grad_out, voxels, stats, relu, training, grad_x, grad_gamma_beta, workspace,
                         workspace_bytes, stream);
}

}  // extern "C"
