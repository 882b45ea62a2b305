// The 3x3 / stride 1 / pad = dilation 2-D convolution tile on the gfx950 matrix
// cores, shared by PSNet's context stacks (context.hip: sfm_conv2_f16 /
// sfm_conv2_bf16) and its feature CNN (feature.hip: sfm_conv2x_f16).
//
// k_conv2: implicit GEMM, D[cout][pixels] = W[cout][K] . X[K][pixels], K = 9
// taps x cin, weights as the A operand.  One block = 4 waves = R output rows x
// 64 output columns of one image; a wave owns R/2 rows x 32 columns and all
// NG = cout_pad / 32 output-channel groups (NG x R/2 32x32 accumulators: R = 8
// for NG <= 2, R = 4 for NG = 3, 4, so at most 8 accumulators = 128 registers
// per lane).  The K loop is staged through LDS one (kernel row dy, 32-channel
// chunk) at a time: input rows y0 + (dy-1) dil + 0..R-1, columns x0 - dil ..
// x0 + 63 + dil (the three dx taps read the same rows at column offsets 0,
// dil, 2 dil, so no row halo is staged) and that (dy, chunk)'s 3 x cout_pad x
// 32 weights.  16-byte chunks are XOR-swizzled as in regularize.hip.  Taps
// outside the image are zeros written at staging time.  The next stage is
// prefetched into VGPRs during the current one's MFMAs.
#pragma once
#include "common.h"
#include "act_cvt.h"
#include "mfma_frag.h"

namespace sfm {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kTileX = 64;     // output columns per block
constexpr int kMaxDil = 16;
constexpr int kThreads = 256;  // 4 waves: 2 row groups x 2 column halves

__device__ __forceinline__ int swz(int chunk, int row) { return chunk ^ ((row >> 2) & 3); }

template <bool F16> struct Act;
template <> struct Act<false> : ActCvt<false> {
  using v8 = bf16x8;
  static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Act<true> : ActCvt<true> {
  using v8 = f16x8;
  static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

constexpr int rows_of(int ng) { return ng <= 2 ? 8 : 4; }
constexpr int w_bytes(int ng) { return 3 * ng * 32 * 64; }                       // one (dy, chunk): 3 taps
constexpr int in_bytes(int ng, int dil) { return rows_of(ng) * (kTileX + 2 * dil) * 64; }

// The 16-bit epilogue of one wave's accumulators: D[row = cout][col = pixel];
// the lane holds pixel (y0 + o, x) and couts 32g + 8q + 4h + (0..3) in
// acc[g][o][4q .. 4q+3].  v = fma(acc, scale, bias), ReLU if asked, then with
// RES16 "+ residual" (16-bit, the output's layout; may be null) and one
// rounding to the 16-bit type.
template <typename A, int NG, int PB, bool RES16>
__device__ __forceinline__ void conv2_store16(const f32x16 (&acc)[NG][PB], const float* __restrict__ scale,
                                              const float* __restrict__ bias, int relu,
                                              const unsigned short* __restrict__ res16,
                                              unsigned short* __restrict__ out, int cout, int img, int y0, int x, int h,
                                              int H, int W) {
#pragma unroll
  for (int o = 0; o < PB; ++o) {
    const int y = y0 + o;
    if (y >= H) break;
    const int64_t pix = ((int64_t)img * H + y) * W + x;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = 32 * g + 8 * q + 4 * h;
        const float4 sc = *reinterpret_cast<const float4*>(scale + co);
        const float4 bi = *reinterpret_cast<const float4*>(bias + co);
        float v[4] = {__builtin_fmaf(acc[g][o][4 * q + 0], sc.x, bi.x), __builtin_fmaf(acc[g][o][4 * q + 1], sc.y, bi.y),
                      __builtin_fmaf(acc[g][o][4 * q + 2], sc.z, bi.z), __builtin_fmaf(acc[g][o][4 * q + 3], sc.w, bi.w)};
        if (relu)
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.0f);
        if (RES16 && res16) {
          const uint2 rv = *reinterpret_cast<const uint2*>(res16 + pix * cout + co);
          v[0] += A::to_f((unsigned short)(rv.x & 0xffffu));
          v[1] += A::to_f((unsigned short)(rv.x >> 16));
          v[2] += A::to_f((unsigned short)(rv.y & 0xffffu));
          v[3] += A::to_f((unsigned short)(rv.y >> 16));
        }
        uint2 st;
        st.x = (unsigned)A::from_f(v[0]) | ((unsigned)A::from_f(v[1]) << 16);
        st.y = (unsigned)A::from_f(v[2]) | ((unsigned)A::from_f(v[3]) << 16);
        *reinterpret_cast<uint2*>(out + pix * cout + co) = st;
      }
    }
  }
}

// The data-gradient epilogue (MASK): out[p, c] = act[p, c] > 0 ? 16-bit(acc) : +0,
// act the 16-bit activation the gradient passes the ReLU of (the output's
// layout; null: no mask).  A select, so a non-finite accumulator under a zero
// activation gives 0 and one under a positive activation comes through.
template <typename A, int NG, int PB>
__device__ __forceinline__ void conv2_store_mask(const f32x16 (&acc)[NG][PB], const unsigned short* __restrict__ act,
                                                 unsigned short* __restrict__ out, int cout, int img, int y0, int x,
                                                 int h, int H, int W) {
#pragma unroll
  for (int o = 0; o < PB; ++o) {
    const int y = y0 + o;
    if (y >= H) break;
    const int64_t pix = ((int64_t)img * H + y) * W + x;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = 32 * g + 8 * q + 4 * h;
        unsigned short v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = A::from_f(acc[g][o][4 * q + j]);
        if (act) {
          const uint2 av = *reinterpret_cast<const uint2*>(act + pix * cout + co);
          const unsigned short a[4] = {(unsigned short)(av.x & 0xffffu), (unsigned short)(av.x >> 16),
                                       (unsigned short)(av.y & 0xffffu), (unsigned short)(av.y >> 16)};
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = A::to_f(a[j]) > 0.0f ? v[j] : (unsigned short)0;
        }
        uint2 st;
        st.x = (unsigned)v[0] | ((unsigned)v[1] << 16);
        st.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
        *reinterpret_cast<uint2*>(out + pix * cout + co) = st;
      }
    }
  }
}

// res: with RES16 the 16-bit residual of the 16-bit output (or null); without,
// the fp32 residual of the cout 1 form (or null); with MASK the 16-bit
// activation of conv2_store_mask (or null), scale / bias / relu unread.
template <bool F16, int NG, bool RES16, bool MASK = false>
__global__ __launch_bounds__(kThreads, 2) void k_conv2(
    const unsigned short* __restrict__ in, int cin, const unsigned short* __restrict__ wpk,
    const float* __restrict__ scale, const float* __restrict__ bias, int relu, const void* __restrict__ res,
    unsigned short* __restrict__ out, float* __restrict__ out1, int cout, int dil, int H, int W, int ntx, int nty) {
  using A = Act<F16>;
  using v8 = typename A::v8;
  constexpr int R = rows_of(NG);        // output rows per block
  constexpr int PB = R / 2;             // output rows (32-pixel blocks) per wave
  constexpr int NX = R / 2;             // extra-column loads per thread
  constexpr int WROWS = 3 * NG * 32;    // weight rows per stage
  constexpr int NW = (WROWS + 63) / 64; // weight loads per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* lds_w = lds;
  unsigned char* lds_in = lds + w_bytes(NG);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int rest = blockIdx.x;
  const int tx = rest % ntx;
  rest /= ntx;
  const int ty = rest % nty, img = rest / nty;
  const int x0 = tx * kTileX, y0 = ty * R;
  const int r = lane & 31, h = lane >> 5;
  const int wrow = (wave >> 1) * PB, wcol = (wave & 1) * 32;
  const int SW = kTileX + 2 * dil;  // staged columns
  const int nchunk = cin >> 5;
  const int nstage = 3 * nchunk;    // stage s: dy = s / nchunk, channel chunk cc = s % nchunk
  const int rowstride = W * cin;
  const unsigned short* img_in = in + (int64_t)img * H * W * cin;

  // Register prefetch of one stage.  Thread t stages chunk t&3 of staged
  // column t>>2 (0..63) in all R rows; columns 64 .. SW-1 (2 dil of them, at
  // most 32) go 128 threads to a row, two rows at a time; weights 64 rows at
  // a time.  Per-thread address parts are hoisted out of the stage loop.
  const int mc = tid & 3, mpx = tid >> 2;
  const int mgx = x0 - dil + mpx;
  const bool mvx = mgx >= 0 && mgx < W;
  const int moff = mgx * cin + mc * 8;
  const int mlds = mpx * 64 + swz(mc, mpx) * 16;
  const int ecol = kTileX + ((tid & 127) >> 2), erow = tid >> 7;
  const bool eact = ecol < SW;
  const int egx = x0 - dil + ecol;
  const bool evx = eact && egx >= 0 && egx < W;
  const int eoff = egx * cin + mc * 8;
  const int elds = ecol * 64 + swz(mc, ecol) * 16;
  const int woff = mpx * cin + mc * 8;
  const int wlds = mpx * 64 + swz(mc, mpx) * 16;
  uint4 pin[R + NX], pw[NW];
  auto fetch = [&](int s) {
    const int dy = s / nchunk, cc = s - dy * nchunk;
    const int gy0 = y0 + (dy - 1) * dil;
    const unsigned short* pl = img_in + cc * 32;
#pragma unroll
    for (int ry = 0; ry < R; ++ry) {
      const int gy = gy0 + ry;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gy >= 0 && gy < H && mvx) v = *reinterpret_cast<const uint4*>(pl + gy * rowstride + moff);
      pin[ry] = v;
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int gy = gy0 + 2 * k + erow;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gy >= 0 && gy < H && evx) v = *reinterpret_cast<const uint4*>(pl + gy * rowstride + eoff);
      pin[R + k] = v;
    }
    const unsigned short* wb = wpk + (int64_t)dy * WROWS * cin + cc * 32;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (mpx + 64 * k < WROWS) v = *reinterpret_cast<const uint4*>(wb + woff + k * 64 * cin);
      pw[k] = v;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int ry = 0; ry < R; ++ry) *reinterpret_cast<uint4*>(lds_in + ry * SW * 64 + mlds) = pin[ry];
    if (eact) {
#pragma unroll
      for (int k = 0; k < NX; ++k) *reinterpret_cast<uint4*>(lds_in + (2 * k + erow) * SW * 64 + elds) = pin[R + k];
    }
#pragma unroll
    for (int k = 0; k < NW; ++k)
      if (mpx + 64 * k < WROWS) *reinterpret_cast<uint4*>(lds_w + wlds + k * 64 * 64) = pw[k];
  };

  f32x16 acc[NG][PB];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int o = 0; o < PB; ++o)
      for (int i = 0; i < 16; ++i) acc[g][o][i] = 0.0f;

  fetch(0);
  for (int s = 0; s < nstage; ++s) {
    __syncthreads();  // the previous stage's operand reads are done
    commit();
    __syncthreads();
    if (s + 1 < nstage) fetch(s + 1);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int c = kb * 2 + h;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        v8 wf[NG], xf[PB];
#pragma unroll
        for (int g = 0; g < NG; ++g)
          wf[g] = *reinterpret_cast<const v8*>(lds_w + ((dx * NG + g) * 32 + r) * 64 + swz(c, r) * 16);
        const int p = wcol + r + dx * dil;
#pragma unroll
        for (int o = 0; o < PB; ++o)
          xf[o] = *reinterpret_cast<const v8*>(lds_in + ((wrow + o) * SW + p) * 64 + swz(c, p) * 16);
        // consecutive MFMAs update different accumulators
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int o = 0; o < PB; ++o) acc[g][o] = A::mfma(wf[g], xf[o], acc[g][o]);
      }
    }
  }

  const int x = x0 + wcol + r;
  if (x >= W) return;
  if constexpr (MASK) {
    conv2_store_mask<A, NG, PB>(acc, reinterpret_cast<const unsigned short*>(res), out, cout, img, y0 + wrow, x, h, H, W);
    return;
  }
  if (!RES16 && out1) {  // cout == 1: the 16-bit rounding torch's autocast output has, then the fp32 "+ plane"
    const float* res1 = reinterpret_cast<const float*>(res);
#pragma unroll
    for (int o = 0; o < PB; ++o) {
      const int y = y0 + wrow + o;
      if (y >= H) break;
      const int64_t pix = ((int64_t)img * H + y) * W + x;
      if (h == 0) {
        float v = __builtin_fmaf(acc[0][o][0], scale[0], bias[0]);
        if (relu) v = fmaxf(v, 0.0f);
        v = A::to_f(A::from_f(v));
        if (res1) v += res1[pix];
        out1[pix] = v;
      }
    }
    return;
  }
  conv2_store16<A, NG, PB, RES16>(acc, scale, bias, relu, RES16 ? reinterpret_cast<const unsigned short*>(res) : nullptr,
                                  out, cout, img, y0 + wrow, x, h, H, W);
}

template <bool F16, int NG, bool RES16, bool MASK = false>
void launch_conv2(hipStream_t s, const void* in, int images, int cin, int h, int w, const void* weights, int cout,
                  int dilation, const float* scale, const float* bias, int relu, const void* residual, void* out) {
  constexpr int R = rows_of(NG);
  const int ntx = (w + kTileX - 1) / kTileX, nty = (h + R - 1) / R;
  const unsigned lds = (unsigned)(w_bytes(NG) + in_bytes(NG, dilation));
  hipLaunchKernelGGL((k_conv2<F16, NG, RES16, MASK>), dim3((unsigned)(ntx * nty * images)), dim3(kThreads), lds, s,
                     (const unsigned short*)in, cin, (const unsigned short*)weights, scale, bias, relu, residual,
                     cout == 1 ? nullptr : (unsigned short*)out, cout == 1 ? (float*)out : nullptr, cout, dilation, h,
                     w, ntx, nty);
}
static_assert(w_bytes(2) + in_bytes(2, kMaxDil) <= 64 * 1024 && w_bytes(4) + in_bytes(4, kMaxDil) <= 64 * 1024,
              "a stage fits the default 64 KB of dynamic LDS, two blocks per CU");

}  // namespace
}  // namespace sfm
