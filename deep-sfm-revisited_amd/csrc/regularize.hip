// 3-D cost regularisation of PSNet on the gfx950 matrix
// cores: the dres0..dres4 / classify stack of models/PSNet.py:79-102 applied
// at PSNet.py:159-165, each layer a 3x3x3 / stride 1 / pad 1 Conv3d with its
// BatchNorm3d folded into a per-channel affine (eval mode), optional ReLU and
// optional residual add.
//
// Layout in HBM: activations are channels-last bf16, [B][D=nlabel][H][W][C]
// with C = 32 (64 for the first layer's input, the [ref | warped] cost
// volume).  Weights are packed per layer as [27 taps][32 cout][Cin] bf16
// (cout zero-padded to 32 for the final 32 -> 1 conv).
//
// k_conv3: implicit GEMM, D[32 cout][pixels] = W[cout][K] . X[K][pixels],
// K = 27 taps x Cin.  One block = 4 waves = one depth slice d, 8 output rows
// and 64 output columns; a wave owns 4 rows x 32 columns (four 32x32
// accumulators).  The K loop is staged through LDS one (dz, 32-channel chunk)
// at a time: the 10 x 66 input halo of depth plane d+dz-1 and the 9 (dy, dx)
// weight taps, 16-byte chunks XOR-swizzled so the ds_read_b128 operand reads
// of a 16-lane group hit distinct bank slots.  The next stage is prefetched
// into VGPRs while the current one computes.  Per stage and wave: 2 k-steps x
// 3 dx x 12 = 72 v_mfma_f32_32x32x16_bf16 against 36 input-row and 18 weight
// fragment reads.  The epilogue applies scale/bias, ReLU and the residual in
// fp32 and stores bf16 four channels at a time (or, for the last layer, the
// single output channel as fp32 [B][D][H][W], the layout the depth head reads).
#include "common.h"
#include "act_cvt.h"
#include <type_traits>

namespace sfm {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileX = 64;          // output columns per block
constexpr int kXcds = 8;            // MI355X: 8 XCDs, each with its own L2
#ifndef SFM_CONV_MINW
#define SFM_CONV_MINW 2
#endif
constexpr int kTileY = 8;           // output rows per block
constexpr int kHaloX = kTileX + 2;  // 66
constexpr int kHaloY = kTileY + 2;  // 10
constexpr int kInBytes = kHaloY * kHaloX * 64;  // one 32-channel chunk: 64 B per pixel
constexpr int kWBytes = 9 * 32 * 64;            // 9 taps x 32 cout x 32 cin bf16
constexpr int kConvThreads = 256;               // 4 waves: 2 row groups x 2 column halves
static_assert(kConvThreads == 4 * kTileX && kHaloY * 8 <= kConvThreads, "staging map: 4 chunks x 64 columns");

__device__ __forceinline__ int swz(int chunk, int row) { return chunk ^ ((row >> 2) & 3); }

// (bf2f / f2bf and the per-type conversions ActCvt<F16>: act_cvt.h, shared with the sweep)

// 16-bit activation type of the low-precision stack: bf16 (8-bit mantissa,
// the fast opt-in) or f16 (11-bit mantissa: what the reference's Conv3d
// layers compute in under cfg.MIXED_PREC autocast, SFMnet.py:164 with
// cfgs/kitti.yml:10).  Same tiling; the MFMA and the conversions differ.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
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

// D = W . X: rows = 32 output channels (weights as the A operand), columns =
// 32 pixels of one output row (the input as the B operand).  A wave owns 4
// output rows x 32 pixels (4 accumulators); each input row fragment it reads
// from LDS feeds up to 3 of them (dy = 0, 1, 2), so an MFMA costs 0.5 input
// and 0.25 weight ds_read_b128.
template <bool F16>
__global__ __launch_bounds__(kConvThreads, SFM_CONV_MINW) void k_conv3(
    const unsigned short* __restrict__ in, int cin, const unsigned short* __restrict__ wpk,
    const float* __restrict__ scale, const float* __restrict__ bias, const unsigned short* __restrict__ res, int relu,
    unsigned short* __restrict__ out, float* __restrict__ out1, int D, int H, int W, int ntx, int nty, int nblk,
    int per_xcd) {
  using A = Act<F16>;
  using v8 = typename A::v8;
  __shared__ __attribute__((aligned(16))) unsigned char lds_in[kInBytes];
  __shared__ __attribute__((aligned(16))) unsigned char lds_w[kWBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  // XCD-aware order: the dispatcher deals workgroup ids round-robin over the
  // 8 XCDs, so id % 8 picks the XCD and id / 8 the slot on it.  Logical
  // blocks are d-fastest, and each XCD owns a contiguous logical range: the
  // blocks resident on one XCD at a time are consecutive depth slices of one
  // (x, y) tile, which stage the same input planes (d-1, d, d+1) and so hit
  // each other's lines in that XCD's L2 instead of re-reading HBM 3 times.
  const int logical = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
  if (logical >= nblk) return;  // whole block, before any barrier
  const int d = logical % D;
  int rest = logical / D;
  const int tx = rest % ntx;
  rest /= ntx;
  const int ty = rest % nty, b = rest / nty;
  const int x0 = tx * kTileX, y0 = ty * kTileY;
  const int r = lane & 31, h = lane >> 5;
  const int wrow = (wave >> 1) * 4, wcol = (wave & 1) * 32;
  const int nchunk = cin >> 5;
  const int nstage = 3 * nchunk;  // stage s: dz = s / nchunk, channel chunk cc = s % nchunk
  const int64_t plane = (int64_t)H * W;

  // Register prefetch of one stage (global -> VGPRs during the previous
  // stage's MFMAs).  Thread t stages chunk t&3 of halo column t>>2 (0..63)
  // in all 10 halo rows, threads < 80 also one chunk of columns 64/65, and
  // 4-5 weight chunks.  Every per-thread address part is hoisted out of the
  // stage loop; a stage only moves scalar plane / row / chunk bases.
  const int mc = tid & 3, mpx = tid >> 2;
  const int mgx = x0 - 1 + mpx;
  const bool mvx = mgx >= 0 && mgx < W;
  const int moff = mgx * cin + mc * 8;
  const int mlds = mpx * 64 + swz(mc, mpx) * 16;
  const bool hasx = tid < kHaloY * 8;
  const int epx = 64 + ((tid >> 2) & 1), ery = tid >> 3;
  const int egx = x0 - 1 + epx, egy = y0 - 1 + ery;
  const bool evalid = hasx && egx < W && egy >= 0 && egy < H;
  const int eoff = egy * W * cin + egx * cin + mc * 8;
  const int elds = (ery * kHaloX + epx) * 64 + swz(mc, epx) * 16;
  const int wco = (tid >> 2) & 31, wt0 = tid >> 7;
  const int woff = (wt0 * 32 + wco) * cin + mc * 8;
  const int wlds = (wt0 * 32 + wco) * 64 + swz(mc, wco) * 16;
  const int rowstride = W * cin;
  uint4 pin[kHaloY + 1], pw[5];
  auto fetch = [&](int s) {
    const int dz = s / nchunk, cc = s - dz * nchunk;
    const int zd = d + dz - 1;
    const bool zin = zd >= 0 && zd < D;
    const unsigned short* pl = in + (((int64_t)b * D + (zin ? zd : 0)) * plane) * cin + cc * 32;
#pragma unroll
    for (int ry = 0; ry < kHaloY; ++ry) {
      const int gy = y0 - 1 + ry;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (zin && gy >= 0 && gy < H && mvx) v = *reinterpret_cast<const uint4*>(pl + gy * rowstride + moff);
      pin[ry] = v;
    }
    {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (zin && evalid) v = *reinterpret_cast<const uint4*>(pl + eoff);
      pin[kHaloY] = v;
    }
    const unsigned short* wb = wpk + (int64_t)dz * 9 * 32 * cin + cc * 32;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (wt0 + 2 * k < 9) v = *reinterpret_cast<const uint4*>(wb + woff + k * 2 * 32 * cin);
      pw[k] = v;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int ry = 0; ry < kHaloY; ++ry)
      *reinterpret_cast<uint4*>(lds_in + ry * kHaloX * 64 + mlds) = pin[ry];
    if (hasx) *reinterpret_cast<uint4*>(lds_in + elds) = pin[kHaloY];
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (wt0 + 2 * k < 9) *reinterpret_cast<uint4*>(lds_w + wlds + k * 2 * 32 * 64) = pw[k];
  };

  f32x16 acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
    for (int i = 0; i < 16; ++i) acc[o][i] = 0.0f;

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
        v8 wf[3], xf[6];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
          wf[dy] = *reinterpret_cast<const v8*>(lds_w + ((dy * 3 + dx) * 32 + r) * 64 + swz(c, r) * 16);
        const int p = wcol + r + dx;
#pragma unroll
        for (int ir = 0; ir < 6; ++ir)  // input rows wrow .. wrow + 5 of the halo
          xf[ir] = *reinterpret_cast<const v8*>(lds_in + ((wrow + ir) * kHaloX + p) * 64 + swz(c, p) * 16);
        // dy-major: consecutive MFMAs update different accumulators
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int o = 0; o < 4; ++o) acc[o] = A::mfma(wf[dy], xf[o + dy], acc[o]);
      }
    }
  }

  // epilogue: D[row = cout][col = pixel]; lane holds pixel r and couts 8q + 4h + (0..3) in acc[.][4q .. 4q+3]
  const int x = x0 + wcol + r;
  if (x >= W) return;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = y0 + wrow + o;
    if (y >= H) break;
    const int64_t pix = ((int64_t)b * D + d) * plane + (int64_t)y * W + x;
    if (out1) {
      if (h == 0) out1[pix] = __builtin_fmaf(acc[o][0], scale[0], bias[0]);
      continue;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 8 * q + 4 * h;
      const float4 sc = *reinterpret_cast<const float4*>(scale + co);
      const float4 bi = *reinterpret_cast<const float4*>(bias + co);
      float v[4] = {__builtin_fmaf(acc[o][4 * q + 0], sc.x, bi.x), __builtin_fmaf(acc[o][4 * q + 1], sc.y, bi.y),
                    __builtin_fmaf(acc[o][4 * q + 2], sc.z, bi.z), __builtin_fmaf(acc[o][4 * q + 3], sc.w, bi.w)};
      if (relu)
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.0f);
      if (res) {
        const uint2 rv = *reinterpret_cast<const uint2*>(res + pix * 32 + co);
        v[0] += A::to_f(rv.x & 0xffff);
        v[1] += A::to_f(rv.x >> 16);
        v[2] += A::to_f(rv.y & 0xffff);
        v[3] += A::to_f(rv.y >> 16);
      }
      uint2 st;
      st.x = (unsigned)A::from_f(v[0]) | ((unsigned)A::from_f(v[1]) << 16);
      st.y = (unsigned)A::from_f(v[2]) | ((unsigned)A::from_f(v[3]) << 16);
      *reinterpret_cast<uint2*>(out + pix * 32 + co) = st;
    }
  }
}

// k_conv3r: the cin = 32 layers, rolling along the depth (plane) axis.  A
// block owns a 4-row x 64-column tile for nplanes consecutive output planes (chosen per launch).
// All 27 weight taps stay resident in LDS (54 KB, staged once per block) and
// every input plane of the range is staged ONCE (6 x 66 halo, 25 KB): plane
// z feeds output planes z+1, z and z-1 (dz = 0, 1, 2) from three rotating
// accumulator sets, and plane z-1 is complete (stored) after plane z.  This
// cuts the bytes a CU pulls from L2/HBM per MFMA ~3.6x against k_conv3,
// whose per-CU load rate (~8 B/cycle) was the binding limit (PMC).
// A wave owns 2 rows x 32 columns: 3 planes x 2 rows = six 32x32 accumulators.
constexpr int kRTileY = 4;                          // output rows per block
constexpr int kRHaloY = kRTileY + 2;                // 6
constexpr int kRInBytes = kRHaloY * kHaloX * 64;    // 25,344
constexpr int kRWBytes = 27 * 32 * 64;              // 55,296
constexpr int kRLds = kRInBytes + kRWBytes;         // 80,640: two blocks per CU

template <bool F16>
__global__ __launch_bounds__(256, 2) void k_conv3r(const unsigned short* __restrict__ in,
                                                   const unsigned short* __restrict__ wpk,
                                                   const float* __restrict__ scale, const float* __restrict__ bias,
                                                   const unsigned short* __restrict__ res, int relu,
                                                   unsigned short* __restrict__ out, float* __restrict__ out1, int D,
                                                   int H, int W, int ntx, int nty, int ndc, int nplanes, int nblk,
                                                   int per_xcd) {
  using A = Act<F16>;
  using v8 = typename A::v8;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* lds_w = lds;
  unsigned char* lds_in = lds + kRWBytes;
  const int logical = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
  if (logical >= nblk) return;  // whole block, before any barrier
  int rest = logical;
  const int dc = rest % ndc;
  rest /= ndc;
  const int tx = rest % ntx;
  rest /= ntx;
  const int ty = rest % nty, b = rest / nty;
  const int x0 = tx * kTileX, y0 = ty * kRTileY, d0 = dc * nplanes;
  const int nd = min(nplanes, D - d0);  // output planes of this block
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wrow = (wave >> 1) * 2, wcol = (wave & 1) * 32;
  const int64_t plane = (int64_t)H * W;
  constexpr int cin = 32;

  // all 27 taps of the weights, once: [tap][cout][32 cin] swizzled
  for (int i = tid; i < 27 * 32 * 4; i += 256) {
    const int c = i & 3, co = (i >> 2) & 31, t = i >> 7;
    const uint4 v = *reinterpret_cast<const uint4*>(wpk + (t * 32 + co) * cin + c * 8);
    *reinterpret_cast<uint4*>(lds_w + (t * 32 + co) * 64 + swz(c, co) * 16) = v;
  }

  // input staging map (hoisted): chunk t&3 of halo column t>>2 in all 6 rows;
  // threads < 48 also one chunk of columns 64/65
  const int mc = tid & 3, mpx = tid >> 2;
  const int mgx = x0 - 1 + mpx;
  const bool mvx = mgx >= 0 && mgx < W;
  const int moff = mgx * cin + mc * 8;
  const int mlds = mpx * 64 + swz(mc, mpx) * 16;
  const bool hasx = tid < kRHaloY * 8;
  const int epx = 64 + ((tid >> 2) & 1), ery = tid >> 3;
  const int egx = x0 - 1 + epx, egy = y0 - 1 + ery;
  const bool evalid = hasx && egx < W && egy >= 0 && egy < H;
  const int eoff = egy * W * cin + egx * cin + mc * 8;
  const int elds = (ery * kHaloX + epx) * 64 + swz(mc, epx) * 16;
  const int rowstride = W * cin;
  uint4 pin[kRHaloY + 1];
  auto fetch = [&](int z) {
    const bool zin = z >= 0 && z < D;
    const unsigned short* pl = in + (((int64_t)b * D + (zin ? z : 0)) * plane) * cin;
#pragma unroll
    for (int ry = 0; ry < kRHaloY; ++ry) {
      const int gy = y0 - 1 + ry;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (zin && gy >= 0 && gy < H && mvx) v = *reinterpret_cast<const uint4*>(pl + gy * rowstride + moff);
      pin[ry] = v;
    }
    uint4 v = make_uint4(0, 0, 0, 0);
    if (zin && evalid) v = *reinterpret_cast<const uint4*>(pl + eoff);
    pin[kRHaloY] = v;
  };
  auto commit = [&]() {
#pragma unroll
    for (int ry = 0; ry < kRHaloY; ++ry) *reinterpret_cast<uint4*>(lds_in + ry * kHaloX * 64 + mlds) = pin[ry];
    if (hasx) *reinterpret_cast<uint4*>(lds_in + elds) = pin[kRHaloY];
  };

  f32x16 acc[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int o = 0; o < 2; ++o)
      for (int i = 0; i < 16; ++i) acc[k][o][i] = 0.0f;

  auto store = [&](f32x16* a, int d) {  // epilogue of output plane d (rows wrow, wrow+1)
    const int x = x0 + wcol + r;
    if (x >= W) return;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int y = y0 + wrow + o;
      if (y >= H) break;
      const int64_t pix = ((int64_t)b * D + d) * plane + (int64_t)y * W + x;
      if (out1) {
        if (h == 0) out1[pix] = __builtin_fmaf(a[o][0], scale[0], bias[0]);
        continue;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = 8 * q + 4 * h;
        const float4 sc = *reinterpret_cast<const float4*>(scale + co);
        const float4 bi = *reinterpret_cast<const float4*>(bias + co);
        float v[4] = {__builtin_fmaf(a[o][4 * q + 0], sc.x, bi.x), __builtin_fmaf(a[o][4 * q + 1], sc.y, bi.y),
                      __builtin_fmaf(a[o][4 * q + 2], sc.z, bi.z), __builtin_fmaf(a[o][4 * q + 3], sc.w, bi.w)};
        if (relu)
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.0f);
        if (res) {
          const uint2 rv = *reinterpret_cast<const uint2*>(res + pix * 32 + co);
          v[0] += A::to_f(rv.x & 0xffff);
          v[1] += A::to_f(rv.x >> 16);
          v[2] += A::to_f(rv.y & 0xffff);
          v[3] += A::to_f(rv.y >> 16);
        }
        uint2 st;
        st.x = (unsigned)A::from_f(v[0]) | ((unsigned)A::from_f(v[1]) << 16);
        st.y = (unsigned)A::from_f(v[2]) | ((unsigned)A::from_f(v[3]) << 16);
        *reinterpret_cast<uint2*>(out + pix * 32 + co) = st;
      }
    }
  };

  // Channels-last epilogue through LDS (the staged plane is dead once every
  // wave has left the MFMA loop): scale/bias/ReLU in the accumulator layout
  // (lane = pixel, 16 channels), one row at a time into a padded [32 px][36]
  // fp32 tile per wave, then read back as lane = (pixel, 16 consecutive
  // channels) so the residual loads and bf16 stores are 32-byte contiguous
  // per lane and a wave covers its row's 2 KB in one pass.
  auto store_cl = [&](f32x16* a, int d) {
    float* T = reinterpret_cast<float*>(lds_in) + wave * (32 * 36);
    const int px = lane >> 1, half = lane & 1;
    const int x = x0 + wcol + px;
    __syncthreads();  // every wave is done with the plane (T overlaps other waves' halo rows)
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      // T is private to the wave: LDS ops of one wave complete in order, so
      // only the compiler must keep row o's writes after row o-1's reads
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = 8 * q + 4 * h;
        const float4 sc = *reinterpret_cast<const float4*>(scale + co);
        const float4 bi = *reinterpret_cast<const float4*>(bias + co);
        float4 v = make_float4(__builtin_fmaf(a[o][4 * q + 0], sc.x, bi.x), __builtin_fmaf(a[o][4 * q + 1], sc.y, bi.y),
                               __builtin_fmaf(a[o][4 * q + 2], sc.z, bi.z), __builtin_fmaf(a[o][4 * q + 3], sc.w, bi.w));
        if (relu) {
          v.x = fmaxf(v.x, 0.0f);
          v.y = fmaxf(v.y, 0.0f);
          v.z = fmaxf(v.z, 0.0f);
          v.w = fmaxf(v.w, 0.0f);
        }
        *reinterpret_cast<float4*>(T + r * 36 + co) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int y = y0 + wrow + o;
      if (y < H && x < W) {
        const int64_t pix = ((int64_t)b * D + d) * plane + (int64_t)y * W + x;
        float v[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float4 t = *reinterpret_cast<const float4*>(T + px * 36 + half * 16 + 4 * k);
          v[4 * k] = t.x;
          v[4 * k + 1] = t.y;
          v[4 * k + 2] = t.z;
          v[4 * k + 3] = t.w;
        }
        if (res) {
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const uint4 rv = *reinterpret_cast<const uint4*>(res + pix * 32 + half * 16 + 8 * k);
            const unsigned int w4[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              v[8 * k + 2 * e] += A::to_f(w4[e] & 0xffff);
              v[8 * k + 2 * e + 1] += A::to_f(w4[e] >> 16);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          uint4 st;
          st.x = (unsigned)A::from_f(v[8 * k + 0]) | ((unsigned)A::from_f(v[8 * k + 1]) << 16);
          st.y = (unsigned)A::from_f(v[8 * k + 2]) | ((unsigned)A::from_f(v[8 * k + 3]) << 16);
          st.z = (unsigned)A::from_f(v[8 * k + 4]) | ((unsigned)A::from_f(v[8 * k + 5]) << 16);
          st.w = (unsigned)A::from_f(v[8 * k + 6]) | ((unsigned)A::from_f(v[8 * k + 7]) << 16);
          *reinterpret_cast<uint4*>(out + pix * 32 + half * 16 + 8 * k) = st;
        }
      }
    }
  };

  // step j stages plane z = d0 - 1 + j and feeds output planes m = j - dz
  // (m in [0, nd)); ring slot of output m is m % 3, i.e. (PH - dz) mod 3.
  const int nsteps = nd + 2;
  auto step = [&](auto ph, int j) {
    constexpr int PH = decltype(ph)::value;
    __syncthreads();  // previous plane's operand reads are done
    commit();
    __syncthreads();
    if (j + 1 < nsteps) fetch(d0 + j);  // plane of step j + 1
    const bool v0 = j < nd, v1 = j >= 1 && j - 1 < nd, v2 = j >= 2;
#pragma unroll
    for (int g = 0; g < 6; ++g) {
      const int kb = g / 3, dx = g - 3 * (g / 3);
      const int c = kb * 2 + h;
      v8 wf[3][3], xf[4];
#pragma unroll
      for (int dz = 0; dz < 3; ++dz)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
          wf[dz][dy] = *reinterpret_cast<const v8*>(lds_w + (((dz * 3 + dy) * 3 + dx) * 32 + r) * 64 + swz(c, r) * 16);
      const int p = wcol + r + dx;
#pragma unroll
      for (int ir = 0; ir < 4; ++ir)
        xf[ir] = *reinterpret_cast<const v8*>(lds_in + ((wrow + ir) * kHaloX + p) * 64 + swz(c, p) * 16);
      if (v0) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int o = 0; o < 2; ++o)
            acc[PH][o] = A::mfma(wf[0][dy], xf[o + dy], acc[PH][o]);
      }
      if (v1) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int o = 0; o < 2; ++o)
            acc[(PH + 2) % 3][o] = A::mfma(wf[1][dy], xf[o + dy], acc[(PH + 2) % 3][o]);
      }
      if (v2) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int o = 0; o < 2; ++o)
            acc[(PH + 1) % 3][o] = A::mfma(wf[2][dy], xf[o + dy], acc[(PH + 1) % 3][o]);
      }
    }
    if (v2) {  // output plane m = j - 2 is complete
      if (out1) store(acc[(PH + 1) % 3], d0 + j - 2);
      else store_cl(acc[(PH + 1) % 3], d0 + j - 2);
#pragma unroll
      for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 16; ++i) acc[(PH + 1) % 3][o][i] = 0.0f;
    }
  };

  fetch(d0 - 1);
  for (int j0 = 0; j0 < nsteps; j0 += 3) {
    step(std::integral_constant<int, 0>{}, j0);
    if (j0 + 1 < nsteps) step(std::integral_constant<int, 1>{}, j0 + 1);
    if (j0 + 2 < nsteps) step(std::integral_constant<int, 2>{}, j0 + 2);
  }
}

// [B][C][P] (fp32 or bf16) -> [B][P][C] bf16, P = D*H*W.  A 64-pixel x C tile
// through LDS: coalesced reads along P per channel, coalesced 16-byte writes.
template <typename T, bool F16>
__global__ __launch_bounds__(256) void k_to_channels_last(const T* __restrict__ in, int C, int64_t P,
                                                          unsigned short* __restrict__ out) {
  __shared__ float tile[64][65];
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const int tid = threadIdx.x;
  for (int c0 = 0; c0 < C; c0 += 64) {
    __syncthreads();
    for (int i = tid; i < 64 * 64; i += 256) {
      const int px = i & 63, c = i >> 6;
      const int64_t p = p0 + px;
      float v = 0.0f;
      if (p < P && c0 + c < C) {
        if constexpr (sizeof(T) == 4) v = in[((int64_t)b * C + c0 + c) * P + p];
        else v = bf2f(in[((int64_t)b * C + c0 + c) * P + p]);
      }
      tile[c][px] = v;
    }
    __syncthreads();
    const int cw = min(64, C - c0);
    for (int i = tid; i < 64 * (cw / 8); i += 256) {
      const int g = i % (cw / 8), px = i / (cw / 8);
      const int64_t p = p0 + px;
      if (p >= P) continue;
      unsigned short s[8];
      for (int j = 0; j < 8; ++j) s[j] = Act<F16>::from_f(tile[g * 8 + j][px]);
      uint4 v;
      v.x = s[0] | ((unsigned)s[1] << 16);
      v.y = s[2] | ((unsigned)s[3] << 16);
      v.z = s[4] | ((unsigned)s[5] << 16);
      v.w = s[6] | ((unsigned)s[7] << 16);
      *reinterpret_cast<uint4*>(out + ((int64_t)b * P + p) * C + c0 + g * 8) = v;
    }
  }
}

// Fast path for float32 input with P % 4 == 0 and C % 8 == 0, C <= 64:
// 256 pixels per block, one float4 (4 pixels) per thread-load so a wave reads
// 1 KB contiguous per channel row; values are rounded to bf16 on the way into
// a [C][256 + 8] LDS tile; each thread then gathers 8 channels of one pixel
// and writes 16 contiguous bytes.
template <bool F16>
__global__ __launch_bounds__(256) void k_to_channels_last_f4(const float* __restrict__ in, int C, int64_t P,
                                                             unsigned short* __restrict__ out) {
  __shared__ unsigned short tile[64][256 + 8];
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * 256;
  const int tid = threadIdx.x;
  const int q = tid & 63;  // float4 index within the 256-pixel window
  for (int c = tid >> 6; c < C; c += 4) {
    const int64_t p = p0 + 4 * q;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p < P) v = *reinterpret_cast<const float4*>(in + ((int64_t)b * C + c) * P + p);  // P % 4 == 0: all 4 valid
    unsigned short* t = &tile[c][4 * q];
    t[0] = Act<F16>::from_f(v.x);
    t[1] = Act<F16>::from_f(v.y);
    t[2] = Act<F16>::from_f(v.z);
    t[3] = Act<F16>::from_f(v.w);
  }
  __syncthreads();
  const int ng = C / 8;
  for (int i = tid; i < 256 * ng; i += 256) {
    const int g = i % ng, px = i / ng;
    const int64_t p = p0 + px;
    if (p >= P) continue;
    uint4 v;
    v.x = tile[g * 8 + 0][px] | ((unsigned)tile[g * 8 + 1][px] << 16);
    v.y = tile[g * 8 + 2][px] | ((unsigned)tile[g * 8 + 3][px] << 16);
    v.z = tile[g * 8 + 4][px] | ((unsigned)tile[g * 8 + 5][px] << 16);
    v.w = tile[g * 8 + 6][px] | ((unsigned)tile[g * 8 + 7][px] << 16);
    *reinterpret_cast<uint4*>(out + ((int64_t)b * P + p) * C + g * 8) = v;
  }
}


// ---------------------------------------------------------------------------
// fp32 path (conv_precision = "fp32"): the same Conv3d layers at the
// reference's precision, on v_mfma_f32_32x32x2_f32 (f32 operands, f32
// accumulation; gfx950's f32 MFMA is an exact fmaf chain, so every product and
// sum rounds as float32 arithmetic does -- only the summation order differs
// from a CPU conv).  Activations are channels-last fp32 [B][D][H][W][C] (128 B
// per voxel at C = 32), weights [27 taps][32 cout][Cin] fp32.
//
// k_conv3_f32: a block (4 waves) owns one depth slice d, 8 output rows x 64
// columns; a wave owns 4 rows x 32 columns (four 32x32 accumulators).  K = 27
// taps x Cin is staged per (dz, 16-channel quarter of a 32-channel chunk):
// the 10 x 66 halo of plane d+dz-1 (64 B per pixel) and the 9 (dy, dx) weight
// taps, 60.7 KB, two blocks per CU so one block's staging overlaps the other's
// MFMAs.  An MFMA consumes k = 2 (lane half kh supplies channel 8 kh + j of
// the quarter at k-step j); each lane reads its 8 channels of a pixel (or of a
// cout row) as two ds_read_b128, 16-byte chunks XOR-swizzled by (p >> 2) & 3
// so a 16-lane group of ds_read_b128 hits 16 distinct bank slots.  Per stage
// and wave: 3 dx x 8 k-steps x 3 dy x 4 rows = 288 MFMAs (64 cycles each at
// one wave per SIMD) against 3 x 6 input and 3 x 3 weight fragment pairs.
// Out-of-range planes (dz at the volume's ends) contribute zeros and are not
// staged at all.  The epilogue is k_conv3's in fp32: scale/bias, ReLU,
// residual, float4 stores (or the single output channel as fp32 [B][D][H][W]).
constexpr int kF32Ch = 16;                                   // channels per stage
constexpr int kF32Pix = kF32Ch * 4;                          // 64 B per staged pixel
constexpr int kF32InBytes = kHaloY * kHaloX * kF32Pix;       // 42,240
constexpr int kF32WBytes = 9 * 32 * kF32Pix;                 // 18,432
// The low side of the fp32x3 split (k_conv3_x3): x_lo = f16(x - f16(x)) is
// ~2^-11 |x|, subnormal (below 2^-14) once |x| < 2^-3, and then carries an
// absolute error of 2^-25 instead of a relative one.  A layer whose largest
// activation is below this is re-run by k_conv3_f32.
constexpr float kX3AmaxMin = 0.125f;
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz4(int chunk, int p) { return chunk ^ ((p >> 2) & 3); }

__global__ __launch_bounds__(kConvThreads, 2) void k_conv3_f32(
    const float* __restrict__ in, int cin, const float* __restrict__ wpk, const float* __restrict__ scale,
    const float* __restrict__ bias, const float* __restrict__ res, int relu, float* __restrict__ out,
    float* __restrict__ out1, int D, int H, int W, int ntx, int nty, int nblk, int per_xcd,
    const int* __restrict__ only_if) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_in[kF32InBytes];
  __shared__ __attribute__((aligned(16))) unsigned char lds_w[kF32WBytes];
  // the fp32x3 layer's re-run: nothing to do unless an activation left the
  // f16 range (word 0) or the layer's largest one is below kX3AmaxMin (word 1)
  if (only_if && only_if[0] == 0 && __int_as_float(only_if[1]) >= kX3AmaxMin) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int logical = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);   // XCD-aware, d-fastest
  if (logical >= nblk) return;
  const int d = logical % D;
  int rest = logical / D;
  const int tx = rest % ntx;
  rest /= ntx;
  const int ty = rest % nty, b = rest / nty;
  const int x0 = tx * kTileX, y0 = ty * kTileY;
  const int r = lane & 31, kh = lane >> 5;
  const int wrow = (wave >> 1) * 4, wcol = (wave & 1) * 32;
  const int nq = cin / kF32Ch;
  const int64_t plane = (int64_t)H * W;

  f32x16 acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
    for (int i = 0; i < 16; ++i) acc[o][i] = 0.0f;

  for (int dz = 0; dz < 3; ++dz) {
    const int zd = d + dz - 1;
    if (zd < 0 || zd >= D) continue;                         // zero padding: no contribution (block-uniform)
    const float* pl = in + ((int64_t)b * D + zd) * plane * cin;
    for (int q = 0; q < nq; ++q) {
      __syncthreads();                                       // the previous stage's operand reads are done
      // input halo: 10 rows x 66 pixels x 4 chunks of 16 B
      for (int i = tid; i < kHaloY * kHaloX * 4; i += kConvThreads) {
        const int c = i & 3, px = (i >> 2) % kHaloX, ry = (i >> 2) / kHaloX;
        const int gx = x0 - 1 + px, gy = y0 - 1 + ry;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H)
          v = *reinterpret_cast<const float4*>(pl + ((int64_t)gy * W + gx) * cin + q * kF32Ch + c * 4);
        *reinterpret_cast<float4*>(lds_in + (ry * kHaloX + px) * kF32Pix + swz4(c, px) * 16) = v;
      }
      // weights: 9 (dy, dx) taps x 32 cout x 4 chunks
      for (int i = tid; i < 9 * 32 * 4; i += kConvThreads) {
        const int c = i & 3, co = (i >> 2) & 31, t = i >> 7;
        const float4 v = *reinterpret_cast<const float4*>(wpk + ((int64_t)(dz * 9 + t) * 32 + co) * cin + q * kF32Ch + c * 4);
        *reinterpret_cast<float4*>(lds_w + (t * 32 + co) * kF32Pix + swz4(c, co) * 16) = v;
      }
      __syncthreads();
#pragma unroll 1
      for (int dx = 0; dx < 3; ++dx) {
        const int p = wcol + r + dx;
#pragma unroll
        for (int e = 0; e < 2; ++e) {                        // channels 8 kh + 4 e .. + 3
          const int ch = 2 * kh + e;
          f32x4 wf[3], xf[6];
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
            wf[dy] = *reinterpret_cast<const f32x4*>(lds_w + ((dy * 3 + dx) * 32 + r) * kF32Pix + swz4(ch, r) * 16);
#pragma unroll
          for (int ir = 0; ir < 6; ++ir)
            xf[ir] = *reinterpret_cast<const f32x4*>(lds_in + ((wrow + ir) * kHaloX + p) * kF32Pix + swz4(ch, p) * 16);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int o = 0; o < 4; ++o)
                acc[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[dy][j], xf[o + dy][j], acc[o], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: lane holds pixel r, couts 8q + 4kh + (0..3) in acc[.][4q .. 4q+3]
  const int x = x0 + wcol + r;
  if (x >= W) return;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = y0 + wrow + o;
    if (y >= H) break;
    const int64_t pix = ((int64_t)b * D + d) * plane + (int64_t)y * W + x;
    if (out1) {
      if (kh == 0) out1[pix] = __builtin_fmaf(acc[o][0], scale[0], bias[0]);
      continue;
    }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int co = 8 * qq + 4 * kh;
      const float4 sc = *reinterpret_cast<const float4*>(scale + co);
      const float4 bi = *reinterpret_cast<const float4*>(bias + co);
      float4 v = make_float4(__builtin_fmaf(acc[o][4 * qq + 0], sc.x, bi.x), __builtin_fmaf(acc[o][4 * qq + 1], sc.y, bi.y),
                             __builtin_fmaf(acc[o][4 * qq + 2], sc.z, bi.z), __builtin_fmaf(acc[o][4 * qq + 3], sc.w, bi.w));
      if (relu) {
        v.x = fmaxf(v.x, 0.0f);
        v.y = fmaxf(v.y, 0.0f);
        v.z = fmaxf(v.z, 0.0f);
        v.w = fmaxf(v.w, 0.0f);
      }
      if (res) {
        const float4 rv = *reinterpret_cast<const float4*>(res + pix * 32 + co);
        v.x += rv.x;
        v.y += rv.y;
        v.z += rv.z;
        v.w += rv.w;
      }
      *reinterpret_cast<float4*>(out + pix * 32 + co) = v;
    }
  }
}

// ---------------------------------------------------------------------------
// fp32 via split f16 (round 5, conv_precision "fp32x3"): the fp32 layers of
// k_conv3_f32 -- same fp32 channels-last activations, weights, epilogue and
// tiling -- with each product formed on the f16 matrix cores from a two-term
// split of both operands, x = x_hi + x_lo, w = w_hi + w_lo (x_hi = f16(x),
// x_lo = f16(x - x_hi); weights pre-scaled by 2^wexp so that w_lo stays in
// the f16 normal range):
//   w x ~ w_hi x_hi + w_hi x_lo + w_lo x_hi      (w_lo x_lo, ~2^-22 |w x|, dropped)
// three v_mfma_f32_32x32x16_f16 per k = 16 into the fp32 accumulators, every
// f16 product exact in f32.  Per product ~2^-21 relative (against 2^-24 for
// the f32 MFMA) at 5x fewer matrix-core cycles per stage (108 x 32-cycle
// MFMAs vs 288 x 64-cycle ones).  Emulated on the float64 PSNet fixture
// before it was written: depth median 2.8e-7 / max 3.6e-6 relative (the f32
// path 2.3e-7 / 3.1e-6; bars 1e-5 / 1e-4).  Valid while every activation
// and 2^wexp w is below the f16 maximum (65504).
// A stage is (dz, 16-channel quarter), as in k_conv3_f32; a staged pixel (or
// weight row) is 64 B: chunks 0-1 the hi halves of channels 0-7 / 8-15,
// chunks 2-3 the lo halves, XOR-swizzled by (p >> 2) & 3.  The next stage's
// fp32 operands load into registers under the current stage's MFMAs (as in
// k_conv3) and are split on their way into LDS (one float4 -> 8 B hi + 8 B lo).
// ---------------------------------------------------------------------------
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
constexpr float kF16Max = 65504.0f;                          // the largest finite f16

__device__ __forceinline__ void split_f16x4(const float4 v, uint2& hi, uint2& lo) {
  const f16x4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
  const f16x4 l = {(_Float16)(v.x - (float)h[0]), (_Float16)(v.y - (float)h[1]), (_Float16)(v.z - (float)h[2]),
                   (_Float16)(v.w - (float)h[3])};
  hi = __builtin_bit_cast(uint2, h);
  lo = __builtin_bit_cast(uint2, l);
}

__global__ __launch_bounds__(kConvThreads, 2) void k_conv3_x3(
    const float* __restrict__ in, int cin, const float* __restrict__ wpk, int wexp, const float* __restrict__ scale,
    const float* __restrict__ bias, const float* __restrict__ res, int relu, float* __restrict__ out,
    float* __restrict__ out1, int D, int H, int W, int ntx, int nty, int nblk, int per_xcd,
    int* __restrict__ range_flag) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_in[kF32InBytes];
  __shared__ __attribute__((aligned(16))) unsigned char lds_w[kF32WBytes];
  __shared__ int lds_amax;                                    // the block's largest activation, as its bit pattern
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int logical = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);   // XCD-aware, d-fastest
  if (logical >= nblk) return;
  if (tid == 0) lds_amax = 0;                                 // ordered before its use by the stage loop's barriers
  const int d = logical % D;
  int rest = logical / D;
  const int tx = rest % ntx;
  rest /= ntx;
  const int ty = rest % nty, b = rest / nty;
  const int x0 = tx * kTileX, y0 = ty * kTileY;
  const int r = lane & 31, kh = lane >> 5;
  const int wrow = (wave >> 1) * 4, wcol = (wave & 1) * 32;
  const int nq = cin / kF32Ch;
  const int64_t plane = (int64_t)H * W;
  const float wmul = __builtin_ldexpf(1.0f, wexp);
  // the stages: (dz, quarter q) over the planes inside the volume (zero
  // padding contributes nothing), staged through registers one ahead
  const int dz0 = d == 0 ? 1 : 0, dz1 = d == D - 1 ? 2 : 3;
  const int nstage = (dz1 - dz0) * nq;

  // staging map (hoisted, as k_conv3's): thread t loads float4 t&3 of halo
  // column t>>2 (0..63) in all 10 rows, threads < 80 one float4 of columns
  // 64/65, and weight float4 t&3 of cout (t>>2)&31 for taps t>>7 + 2k
  const int mc = tid & 3, mpx = tid >> 2;
  const int mgx = x0 - 1 + mpx;
  const bool mvx = mgx >= 0 && mgx < W;
  const bool hasx = tid < kHaloY * 8;
  const int epx = 64 + ((tid >> 2) & 1), ery = tid >> 3;
  const int egx = x0 - 1 + epx, egy = y0 - 1 + ery;
  const bool evalid = hasx && egx < W && egy >= 0 && egy < H;
  const int wco = (tid >> 2) & 31, wt0 = tid >> 7;
  float4 pin[kHaloY + 1], pw[5];
  auto fetch = [&](int s) {
    const int dz = dz0 + s / nq, q = s - (s / nq) * nq;
    const float* pl = in + ((int64_t)b * D + (d + dz - 1)) * plane * cin + q * kF32Ch + mc * 4;
#pragma unroll
    for (int ry = 0; ry < kHaloY; ++ry) {
      const int gy = y0 - 1 + ry;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (gy >= 0 && gy < H && mvx) v = *reinterpret_cast<const float4*>(pl + ((int64_t)gy * W + mgx) * cin);
      pin[ry] = v;
    }
    {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (evalid) v = *reinterpret_cast<const float4*>(pl + ((int64_t)egy * W + egx) * cin);
      pin[kHaloY] = v;
    }
    const float* wb = wpk + (int64_t)dz * 9 * 32 * cin + q * kF32Ch + mc * 4;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (wt0 + 2 * k < 9) v = *reinterpret_cast<const float4*>(wb + ((wt0 + 2 * k) * 32 + wco) * cin);
      pw[k] = v;
    }
  };
  // one float4 (4 channels, mc) -> 8 B of hi halves in chunk mc >> 1 and 8 B
  // of lo halves in chunk 2 + (mc >> 1) of a 64-byte LDS row
  auto put = [&](unsigned char* row, int sw, float4 v) {
    uint2 hi, lo;
    split_f16x4(v, hi, lo);
    *reinterpret_cast<uint2*>(row + (mc & 1) * 8 + swz4(mc >> 1, sw) * 16) = hi;
    *reinterpret_cast<uint2*>(row + (mc & 1) * 8 + swz4(2 + (mc >> 1), sw) * 16) = lo;
  };
  // the largest staged activation magnitude: past the f16 maximum x_hi would
  // be infinite (NaNs drop out of fmaxf, and propagate alike on both paths)
  float amax = 0.0f;
  auto track = [&](const float4 v) {
    amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  };
  auto commit = [&]() {
#pragma unroll
    for (int ry = 0; ry < kHaloY; ++ry) {
      track(pin[ry]);
      put(lds_in + (ry * kHaloX + mpx) * kF32Pix, mpx, pin[ry]);
    }
    if (hasx) {
      track(pin[kHaloY]);
      put(lds_in + (ery * kHaloX + epx) * kF32Pix, epx, pin[kHaloY]);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (wt0 + 2 * k < 9) {
        float4 v = pw[k];
        v.x *= wmul; v.y *= wmul; v.z *= wmul; v.w *= wmul;
        put(lds_w + ((wt0 + 2 * k) * 32 + wco) * kF32Pix, wco, v);
      }
  };

  f32x16 acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
    for (int i = 0; i < 16; ++i) acc[o][i] = 0.0f;

  fetch(0);
  for (int s = 0; s < nstage; ++s) {
    __syncthreads();                                         // the previous stage's operand reads are done
    commit();
    __syncthreads();
    if (s + 1 < nstage) fetch(s + 1);                        // global loads in flight under the MFMAs
#pragma unroll 1
    for (int dx = 0; dx < 3; ++dx) {
      const int p = wcol + r + dx;
      f16x8 wh[3], wl[3], xh[6], xl[6];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const unsigned char* wrowp = lds_w + ((dy * 3 + dx) * 32 + r) * kF32Pix;
        wh[dy] = *reinterpret_cast<const f16x8*>(wrowp + swz4(kh, r) * 16);
        wl[dy] = *reinterpret_cast<const f16x8*>(wrowp + swz4(2 + kh, r) * 16);
      }
#pragma unroll
      for (int ir = 0; ir < 6; ++ir) {
        const unsigned char* px = lds_in + ((wrow + ir) * kHaloX + p) * kF32Pix;
        xh[ir] = *reinterpret_cast<const f16x8*>(px + swz4(kh, p) * 16);
        xl[ir] = *reinterpret_cast<const f16x8*>(px + swz4(2 + kh, p) * 16);
      }
      // hi x hi first into each accumulator, then the two cross terms
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          acc[o] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[dy], xh[o + dy], acc[o], 0, 0, 0);
          acc[o] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[dy], xl[o + dy], acc[o], 0, 0, 0);
          acc[o] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[dy], xh[o + dy], acc[o], 0, 0, 0);
        }
    }
  }

  // an activation outside the f16 range: flag the layer for its fp32 re-run
  // (sfm_conv3_f32x3 with a range flag; a plain vector store, idempotent).
  // The low side: the layer's largest activation into word 1, one atomicMax
  // per block (amax >= 0 and never NaN, so its bit pattern orders as an int).
  if (range_flag) {
    if (amax > kF16Max) range_flag[0] = 1;
    atomicMax(&lds_amax, __float_as_int(amax));
    __syncthreads();
    if (tid == 0) atomicMax(range_flag + 1, lds_amax);
  }
  // epilogue: k_conv3_f32's, with the weights' 2^wexp folded into the scale
  // (exact: a power of two)
  const float unscale = __builtin_ldexpf(1.0f, -wexp);
  const int x = x0 + wcol + r;
  if (x >= W) return;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = y0 + wrow + o;
    if (y >= H) break;
    const int64_t pix = ((int64_t)b * D + d) * plane + (int64_t)y * W + x;
    if (out1) {
      if (kh == 0) out1[pix] = __builtin_fmaf(acc[o][0], scale[0] * unscale, bias[0]);
      continue;
    }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int co = 8 * qq + 4 * kh;
      float4 sc = *reinterpret_cast<const float4*>(scale + co);
      sc.x *= unscale; sc.y *= unscale; sc.z *= unscale; sc.w *= unscale;
      const float4 bi = *reinterpret_cast<const float4*>(bias + co);
      float4 v = make_float4(__builtin_fmaf(acc[o][4 * qq + 0], sc.x, bi.x), __builtin_fmaf(acc[o][4 * qq + 1], sc.y, bi.y),
                             __builtin_fmaf(acc[o][4 * qq + 2], sc.z, bi.z), __builtin_fmaf(acc[o][4 * qq + 3], sc.w, bi.w));
      if (relu) {
        v.x = fmaxf(v.x, 0.0f);
        v.y = fmaxf(v.y, 0.0f);
        v.z = fmaxf(v.z, 0.0f);
        v.w = fmaxf(v.w, 0.0f);
      }
      if (res) {
        const float4 rv = *reinterpret_cast<const float4*>(res + pix * 32 + co);
        v.x += rv.x;
        v.y += rv.y;
        v.z += rv.z;
        v.w += rv.w;
      }
      *reinterpret_cast<float4*>(out + pix * 32 + co) = v;
    }
  }
}

// [B][C][P] (fp32 or bf16) -> [B][P][C] fp32 through a 64-pixel x 64-channel
// LDS tile: coalesced reads along P per channel, 16-byte writes along C.
template <typename T>
__global__ __launch_bounds__(256) void k_to_channels_last_f32(const T* __restrict__ in, int C, int64_t P,
                                                              float* __restrict__ out) {
  __shared__ float tile[64][65];
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const int tid = threadIdx.x;
  for (int c0 = 0; c0 < C; c0 += 64) {
    __syncthreads();
    for (int i = tid; i < 64 * 64; i += 256) {
      const int px = i & 63, c = i >> 6;
      const int64_t p = p0 + px;
      float v = 0.0f;
      if (p < P && c0 + c < C) {
        if constexpr (sizeof(T) == 4) v = in[((int64_t)b * C + c0 + c) * P + p];
        else v = bf2f(in[((int64_t)b * C + c0 + c) * P + p]);
      }
      tile[c][px] = v;
    }
    __syncthreads();
    const int cw = min(64, C - c0);
    for (int i = tid; i < 64 * (cw / 4); i += 256) {
      const int g = i % (cw / 4), px = i / (cw / 4);
      const int64_t p = p0 + px;
      if (p >= P) continue;
      *reinterpret_cast<float4*>(out + ((int64_t)b * P + p) * C + c0 + g * 4) =
          make_float4(tile[g * 4][px], tile[g * 4 + 1][px], tile[g * 4 + 2][px], tile[g * 4 + 3][px]);
    }
  }
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

}  // extern "C"

template <bool F16>
static int conv3_lp(const void* in, int batch, int cin, int depth, int h, int w, const void* weights,
                    const float* scale, const float* bias, const void* residual, int relu, int cout, void* out,
                    void* stream) {
  SFM_REQUIRE(in && weights && scale && bias && out, "null pointer argument");
  SFM_REQUIRE(cin == 32 || cin == 64, "cin must be 32 or 64");
  SFM_REQUIRE(cout == 32 || cout == 1, "cout must be 32 or 1");
  SFM_REQUIRE(cout == 32 || residual == nullptr, "residual needs cout 32");
  SFM_REQUIRE(batch >= 1 && depth >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)h * w * cin < ((int64_t)1 << 31), "conv plane too large (32-bit in-plane offsets)");
  SFM_REQUIRE(in != out && (residual == nullptr || residual != out), "conv output must not alias its inputs");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)weights & 15) == 0, "conv operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(F16 ? "conv3_f16" : "conv3", s);
  const int ntx = (w + kTileX - 1) / kTileX;
  if (cin == 32 && tuning().conv_rolling) {
    // > 64 KB of dynamic LDS must be opted into; set on every launch (cheap,
    // and correct for whichever device is current and from any host thread)
    SFM_HIP(hipFuncSetAttribute((const void*)k_conv3r<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, kRLds));
    // Longest plane run that still gives ~one full round of 2 blocks per CU
    // (fewer halo planes and weight stagings per output plane; measured at
    // C2: 8 -> 16 -> 32 planes = 748 -> 772 -> 798 TFLOP/s).
    const int nty = (h + kRTileY - 1) / kRTileY;
    int nplanes = 4;
    for (int cand : {32, 16, 8}) {
      if ((int64_t)ntx * nty * batch * ((depth + cand - 1) / cand) >= 480) {
        nplanes = cand;
        break;
      }
    }
    // conv_planes: a given run length instead (launch shape only: the tests' handle on the long runs)
    if (tuning().conv_planes) nplanes = tuning().conv_planes;
    const int ndc = (depth + nplanes - 1) / nplanes;
    const int64_t nblk = (int64_t)ntx * nty * ndc * batch;
    SFM_REQUIRE(nblk < ((int64_t)1 << 31) - 8, "conv grid too large");
    const int per_xcd = (int)((nblk + kXcds - 1) / kXcds);
    hipLaunchKernelGGL(k_conv3r<F16>, dim3((unsigned)(per_xcd * kXcds)), dim3(256), kRLds, s, (const unsigned short*)in,
                       (const unsigned short*)weights, scale, bias, (const unsigned short*)residual, relu,
                       cout == 32 ? (unsigned short*)out : nullptr, cout == 1 ? (float*)out : nullptr, depth, h, w,
                       ntx, nty, ndc, nplanes, (int)nblk, per_xcd);
  } else {
    const int nty = (h + kTileY - 1) / kTileY;
    const int64_t nblk = (int64_t)ntx * nty * batch * depth;
    SFM_REQUIRE(nblk < ((int64_t)1 << 31) - 8, "conv grid too large");
    const int per_xcd = (int)((nblk + kXcds - 1) / kXcds);
    hipLaunchKernelGGL(k_conv3<F16>, dim3((unsigned)(per_xcd * kXcds)), dim3(kConvThreads), 0, s, (const unsigned short*)in,
                       cin, (const unsigned short*)weights, scale, bias, (const unsigned short*)residual, relu,
                       cout == 32 ? (unsigned short*)out : nullptr, cout == 1 ? (float*)out : nullptr, depth, h, w,
                       ntx, nty, (int)nblk, per_xcd);
  }
  SFM_LAUNCHED();
  return SFM_OK;
}

extern "C" {

int sfm_conv3_bf16(const void* in, int batch, int cin, int depth, int h, int w, const void* weights,
                   const float* scale, const float* bias, const void* residual, int relu, int cout, void* out,
                   void* stream) {
  return conv3_lp<false>(in, batch, cin, depth, h, w, weights, scale, bias, residual, relu, cout, out, stream);
}

int sfm_conv3_f16(const void* in, int batch, int cin, int depth, int h, int w, const void* weights,
                  const float* scale, const float* bias, const void* residual, int relu, int cout, void* out,
                  void* stream) {
  return conv3_lp<true>(in, batch, cin, depth, h, w, weights, scale, bias, residual, relu, cout, out, stream);
}

}  // extern "C"

template <bool F16>
static int to_channels_last_lp(const void* in, int in_dtype, int batch, int channels, int64_t plane, void* out,
                               void* stream) {
  SFM_REQUIRE(in && out, "null pointer argument");
  SFM_REQUIRE(in_dtype == 0 || in_dtype == 1, "in_dtype must be 0 (float32) or 1 (bfloat16)");
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 8 && channels % 8 == 0 && plane >= 1,
              "invalid channels-last shape (channels must be a multiple of 8)");
  SFM_REQUIRE(((uintptr_t)out & 15) == 0, "output must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("to_channels_last", s);
  dim3 grid((unsigned)((plane + 63) / 64), batch);
  if (in_dtype == 0 && plane % 4 == 0 && channels <= 64 && ((uintptr_t)in & 15) == 0)
    hipLaunchKernelGGL(k_to_channels_last_f4<F16>, dim3((unsigned)((plane + 255) / 256), batch), dim3(256), 0, s,
                       (const float*)in, channels, plane, (unsigned short*)out);
  else if (in_dtype == 0)
    hipLaunchKernelGGL((k_to_channels_last<float, F16>), grid, dim3(256), 0, s, (const float*)in, channels, plane,
                       (unsigned short*)out);
  else
    hipLaunchKernelGGL((k_to_channels_last<unsigned short, F16>), grid, dim3(256), 0, s, (const unsigned short*)in, channels,
                       plane, (unsigned short*)out);
  SFM_LAUNCHED();
  return SFM_OK;
}

extern "C" {

int sfm_to_channels_last_bf16(const void* in, int in_dtype, int batch, int channels, int64_t plane, void* out,
                              void* stream) {
  return to_channels_last_lp<false>(in, in_dtype, batch, channels, plane, out, stream);
}

int sfm_to_channels_last_f16(const void* in, int in_dtype, int batch, int channels, int64_t plane, void* out,
                             void* stream) {
  return to_channels_last_lp<true>(in, in_dtype, batch, channels, plane, out, stream);
}

int sfm_conv3_f32(const float* in, int batch, int cin, int depth, int h, int w, const float* weights,
                  const float* scale, const float* bias, const float* residual, int relu, int cout, float* out,
                  void* stream) {
  SFM_REQUIRE(in && weights && scale && bias && out, "null pointer argument");
  SFM_REQUIRE(cin == 32 || cin == 64, "cin must be 32 or 64");
  SFM_REQUIRE(cout == 32 || cout == 1, "cout must be 32 or 1");
  SFM_REQUIRE(cout == 32 || residual == nullptr, "residual needs cout 32");
  SFM_REQUIRE(batch >= 1 && depth >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE(in != out && (residual == nullptr || residual != out), "conv output must not alias its inputs");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)weights & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                  ((uintptr_t)residual & 15) == 0,
              "conv operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv3_f32", s);
  const int ntx = (w + kTileX - 1) / kTileX;
  const int nty = (h + kTileY - 1) / kTileY;
  const int64_t nblk = (int64_t)ntx * nty * batch * depth;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31) - 8, "conv grid too large");
  const int per_xcd = (int)((nblk + kXcds - 1) / kXcds);
  hipLaunchKernelGGL(k_conv3_f32, dim3((unsigned)(per_xcd * kXcds)), dim3(kConvThreads), 0, s, in, cin, weights,
                     scale, bias, residual, relu, cout == 32 ? out : nullptr, cout == 1 ? out : nullptr, depth, h, w,
                     ntx, nty, (int)nblk, per_xcd, (const int*)nullptr);
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_conv3_f32x3(const float* in, int batch, int cin, int depth, int h, int w, const float* weights, int wexp,
                    const float* scale, const float* bias, const float* residual, int relu, int cout, float* out,
                    int* range_flag, void* stream) {
  SFM_REQUIRE(in && weights && scale && bias && out, "null pointer argument");
  SFM_REQUIRE(cin == 32 || cin == 64, "cin must be 32 or 64");
  SFM_REQUIRE(cout == 32 || cout == 1, "cout must be 32 or 1");
  SFM_REQUIRE(cout == 32 || residual == nullptr, "residual needs cout 32");
  SFM_REQUIRE(wexp >= -24 && wexp <= 24, "wexp must be in [-24, 24]");
  SFM_REQUIRE(batch >= 1 && depth >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE(in != out && (residual == nullptr || residual != out), "conv output must not alias its inputs");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)weights & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                  ((uintptr_t)residual & 15) == 0,
              "conv operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv3_f32x3", s);
  const int ntx = (w + kTileX - 1) / kTileX;
  const int nty = (h + kTileY - 1) / kTileY;
  const int64_t nblk = (int64_t)ntx * nty * batch * depth;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31) - 8, "conv grid too large");
  const int per_xcd = (int)((nblk + kXcds - 1) / kXcds);
  SFM_REQUIRE(range_flag == nullptr || ((uintptr_t)range_flag & 3) == 0, "range_flag must be 4-byte aligned");
  if (range_flag) SFM_HIP(hipMemsetAsync(range_flag, 0, 2 * sizeof(int), s));
  hipLaunchKernelGGL(k_conv3_x3, dim3((unsigned)(per_xcd * kXcds)), dim3(kConvThreads), 0, s, in, cin, weights, wexp,
                     scale, bias, residual, relu, cout == 32 ? out : nullptr, cout == 1 ? out : nullptr, depth, h, w,
                     ntx, nty, (int)nblk, per_xcd, range_flag);
  SFM_LAUNCHED();
  if (range_flag) {
    // stream-ordered fallback: the same layer on the f32 matrix cores (the
    // same weights: k_conv3_x3 applies 2^wexp itself) re-writes out, its
    // blocks returning at once unless an activation left the f16 range or
    // the layer's largest one is below kX3AmaxMin
    hipLaunchKernelGGL(k_conv3_f32, dim3((unsigned)(per_xcd * kXcds)), dim3(kConvThreads), 0, s, in, cin, weights,
                       scale, bias, residual, relu, cout == 32 ? out : nullptr, cout == 1 ? out : nullptr, depth, h,
                       w, ntx, nty, (int)nblk, per_xcd, (const int*)range_flag);
    SFM_LAUNCHED();
  }
  return SFM_OK;
}

int sfm_to_channels_last_f32(const void* in, int in_dtype, int batch, int channels, int64_t plane, float* out,
                             void* stream) {
  SFM_REQUIRE(in && out, "null pointer argument");
  SFM_REQUIRE(in_dtype == 0 || in_dtype == 1, "in_dtype must be 0 (float32) or 1 (bfloat16)");
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 4 && channels % 4 == 0 && plane >= 1,
              "invalid channels-last shape (channels must be a multiple of 4)");
  SFM_REQUIRE(((uintptr_t)out & 15) == 0, "output must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("to_channels_last", s);
  dim3 grid((unsigned)((plane + 63) / 64), batch);
  if (in_dtype == 0)
    hipLaunchKernelGGL(k_to_channels_last_f32<float>, grid, dim3(256), 0, s, (const float*)in, channels, plane, out);
  else
    hipLaunchKernelGGL(k_to_channels_last_f32<unsigned short>, grid, dim3(256), 0, s, (const unsigned short*)in,
                       channels, plane, out);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
