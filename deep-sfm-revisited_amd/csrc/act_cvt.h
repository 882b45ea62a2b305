// float32 <-> 16-bit activation conversions of the regularisation stack, shared
// by its kernels (regularize.hip: Act<F16>, k_to_channels_last*) and by the
// plane sweep that writes the stack's channels-last input itself (sweep_cl.hip:
// k_sweep_cl), so that both round a float32 cost value with the same function.
#pragma once
#include <hip/hip_runtime.h>

namespace sfm {

__device__ __forceinline__ float bf2f(unsigned short b) { return __uint_as_float((unsigned int)b << 16); }

__device__ __forceinline__ unsigned short f2bf(float f) {  // RNE (v_cvt_pk_bf16_f32)
  const __bf16 v = (__bf16)f;
  return __builtin_bit_cast(unsigned short, v);
}

// bf16 (F16 = false) or IEEE half (F16 = true), as raw 16-bit patterns
template <bool F16> struct ActCvt;
template <> struct ActCvt<false> {
  static __device__ __forceinline__ float to_f(unsigned short b) { return bf2f(b); }
  static __device__ __forceinline__ unsigned short from_f(float f) { return f2bf(f); }
};
template <> struct ActCvt<true> {
  static __device__ __forceinline__ float to_f(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ unsigned short from_f(float f) {   // RNE (v_cvt_f16_f32)
    return __builtin_bit_cast(unsigned short, (_Float16)f);
  }
};

}  // namespace sfm
