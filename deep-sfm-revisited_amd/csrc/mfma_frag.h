// The 32x32x16 float16 MFMA's vector types, and the transposing LDS read that
// builds an operand whose K axis is the slow axis of the staged image: the
// weight-gradient kernels (regularize_bwd.hip, conv2_wgrad.hip), where K is
// the voxel / pixel axis of both operands.
#pragma once
#include <hip/hip_runtime.h>

namespace sfm {
namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// One 32x32x16 MFMA operand from a [voxel][32 channels] f16 image (64-byte
// rows): rows = 32 channels, k = 16 consecutive voxels from `voxel0`.  Lane l
// gets channel l % 32 of voxels voxel0 + 8 (l / 32) + 0..7.  Per 16-lane group
// g, lane 4 q + p supplies the address of voxel row q, channels 16 (g & 1) +
// 4 p .. + 3; the second read is 4 voxel rows on.  Every lane takes part
// (ds_read_b64_tr_b16 needs EXEC all ones), and A and B read through this one
// function agree in their k order by construction.
__device__ __forceinline__ f16x8 tr_frag(const unsigned char* img, int voxel0, int lane) {
  const int v = voxel0 + 8 * (lane >> 5) + ((lane >> 2) & 3);
  const unsigned char* a = img + v * 64 + 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  typedef short i16x4 __attribute__((vector_size(8)));
  typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
  const f16x4 lo = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)a));
  const f16x4 hi = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(a + 4 * 64)));
  return f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace
}  // namespace sfm
