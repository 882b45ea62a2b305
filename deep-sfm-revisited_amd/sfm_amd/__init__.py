"""sfm_amd — MI355X-native hot path of two-view deep SfM (jytime/Deep-SfM-Revisited).

Host-side mirror of the reference's operator interfaces over the C ABI of
libsfm_hip.so (include/sfm_hip.h):
  ransac   batched RANSAC five-point (essential_matrix extension), flow -> points
  sweep    plane-sweep cost volume (planar, or channels-last for the regulariser), inverse_warp,
           PSNet sweep section; plane_sweep_cost_autograd / inverse_warp_autograd with a gradient into the features
  regularize  PSNet 3-D cost regularisation (dres0..classify) on the matrix cores; conv3_autograd with a float16
           backward (data and weight gradient) for training, batchnorm3_act_autograd (BatchNorm3d + ReLU + residual
           in float16, forward and backward)
  context  PSNet's per-plane context stack and the full-resolution refinement stack on the matrix cores;
           context_refine_autograd and dep_context_refine_autograd with a float16 backward (data and weight
           gradient of every stage; dep_context_unpack_grad, the bilinear upsample's backward)
  feature  PSNet's feature CNN on the matrix cores; conv2x_autograd, one Conv2d with a float16
           backward (conv2x_wgrad_f16 / conv2x_dgrad_f16: strided, 1 x 1 and 320-channel layers);
           batchnorm2_act_autograd (BatchNorm2d + ReLU + residual in float16, forward and backward),
           convbn2_autograd and basic_block_autograd (one convbn, one BasicBlock) on them
  depth    correlation cost and the soft-argmin depth head; depth_head_autograd with a gradient into the cost
  synth    seeded synthetic KITTI-shaped inputs
  dist     one-process-per-GPU pair sharding and RCCL metric gather
  validate the validation loop and its fused depth-metric rows (main.py:477-601)
"""
from . import _lib  # noqa: F401

__all__ = ["ransac", "sweep", "regularize", "synth", "dist", "config", "validate", "plane_sweep_cost_autograd",
           "inverse_warp_autograd", "depth_head_autograd", "conv3_autograd", "batchnorm3_act_autograd",
           "context_refine_autograd", "dep_context_refine_autograd", "dep_context_unpack_grad",
           "conv2x_autograd", "conv2x_wgrad_f16", "conv2x_dgrad_f16",
           "pack_dgrad_weights2x", "unpack_wgrad2x", "batchnorm2_act_autograd", "convbn2_autograd",
           "basic_block_autograd"]


def __getattr__(name):
    # the differentiable entries, imported on first use (sfm_amd.sweep and sfm_amd.depth need torch)
    if name in ("plane_sweep_cost_autograd", "inverse_warp_autograd"):
        from . import sweep
        return getattr(sweep, name)
    if name == "depth_head_autograd":
        from . import depth
        return depth.depth_head_autograd
    if name in ("conv3_autograd", "batchnorm3_act_autograd"):
        from . import regularize
        return getattr(regularize, name)
    if name in ("context_refine_autograd", "dep_context_refine_autograd", "dep_context_unpack_grad"):
        from . import context
        return getattr(context, name)
    if name in ("conv2x_autograd", "conv2x_wgrad_f16", "conv2x_dgrad_f16",
                "pack_dgrad_weights2x", "unpack_wgrad2x", "batchnorm2_act_autograd", "convbn2_autograd",
                "basic_block_autograd"):
        from . import feature
        return getattr(feature, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
