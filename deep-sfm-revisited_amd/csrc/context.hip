// PSNet's per-plane context stack (models/PSNet.py:17-26 convtext, 64-71 the
// seven dilated stages 33 -> 128 -> 128 -> 128 -> 96 -> 64 -> 32 -> 1, applied
// per plane at 175-190) on the gfx950 matrix cores: each stage a 3x3 /
// stride 1 / pad = dilation Conv2d with its optional BatchNorm2d folded into a
// per-channel affine (eval mode) and a ReLU, the last one followed by the
// fp32 "+ plane" of PSNet.py:190.
//
// Layout in HBM: activations are channels-last 16-bit, [images][H][W][C] with
// C in {32, 64, 96, 128}; weights are packed per layer as [9 taps][cout_pad]
// [cin], tap = kh*3 + kw, cout_pad = cout rounded up to 32.
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
#include "common.h"
#include "act_cvt.h"

namespace sfm {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

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

template <bool F16, int NG>
__global__ __launch_bounds__(kThreads, 2) void k_conv2(
    const unsigned short* __restrict__ in, int cin, const unsigned short* __restrict__ wpk,
    const float* __restrict__ scale, const float* __restrict__ bias, int relu, const float* __restrict__ res1,
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

  // epilogue: D[row = cout][col = pixel]; lane holds pixel r and couts 32g + 8q + 4h + (0..3) in acc[g][.][4q .. 4q+3]
  const int x = x0 + wcol + r;
  if (x >= W) return;
#pragma unroll
  for (int o = 0; o < PB; ++o) {
    const int y = y0 + wrow + o;
    if (y >= H) break;
    const int64_t pix = ((int64_t)img * H + y) * W + x;
    if (out1) {  // cout == 1: the 16-bit rounding torch's autocast output has, then the fp32 "+ plane"
      if (h == 0) {
        float v = __builtin_fmaf(acc[0][o][0], scale[0], bias[0]);
        if (relu) v = fmaxf(v, 0.0f);
        v = A::to_f(A::from_f(v));
        if (res1) v += res1[pix];
        out1[pix] = v;
      }
      continue;
    }
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
        uint2 st;
        st.x = (unsigned)A::from_f(v[0]) | ((unsigned)A::from_f(v[1]) << 16);
        st.y = (unsigned)A::from_f(v[2]) | ((unsigned)A::from_f(v[3]) << 16);
        *reinterpret_cast<uint2*>(out + pix * cout + co) = st;
      }
    }
  }
}

// The first layer's input for planes l0 .. l0+nl-1 of every pair:
// [batch][nl][h][w][64], channels 0..31 ctx[b] (the same for every plane),
// channel 32 planes[b][l], 33..63 zero.  One thread per (pixel, 8-channel
// chunk): 16-byte stores, 128 contiguous bytes per pixel.
template <bool F16>
__global__ __launch_bounds__(256) void k_context_pack(const float* __restrict__ ctx, const float* __restrict__ planes,
                                                      int nlabel, int l0, int nl, int channels, int hw, int64_t total,
                                                      unsigned short* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int chunk = (int)(i & 7);
  const int64_t pixel = i >> 3;  // (b * nl + l) * hw + p
  const int p = (int)(pixel % hw);
  const int64_t bl = pixel / hw;
  const int l = (int)(bl % nl), b = (int)(bl / nl);
  unsigned short s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (chunk * 8 < channels) {
    const float* c = ctx + ((int64_t)b * channels + chunk * 8) * hw + p;
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = ActCvt<F16>::from_f(c[(int64_t)j * hw]);
  } else if (chunk * 8 == channels) {
    s[0] = ActCvt<F16>::from_f(planes[((int64_t)b * nlabel + l0 + l) * hw + p]);
  }
  uint4 v;
  v.x = s[0] | ((unsigned)s[1] << 16);
  v.y = s[2] | ((unsigned)s[3] << 16);
  v.z = s[4] | ((unsigned)s[5] << 16);
  v.w = s[6] | ((unsigned)s[7] << 16);
  *reinterpret_cast<uint4*>(out + pixel * 64 + chunk * 8) = v;
}

// The first input of the full-resolution refinement stack dep_convs
// (models/PSNet.py:218-221) for pairs b0 .. b0+nb-1: [nb][H][W][64], channel 0
// depth, 1..32 the [h][w] features upsampled bilinearly to H x W
// (align_corners=True), 33..35 the image, 36..63 zero -- the order of the
// reference's cat((depth, up_feat, ref)).  One thread per (pixel, 8-channel
// chunk) as in k_context_pack: 16-byte stores, 128 contiguous bytes per pixel.
// Chunk 0 holds the depth and features 0..6, chunks 1..3 features 8k-1 ..
// 8k+6, chunk 4 feature 31 and the image, chunks 5..7 zeros.  The features are
// read in their own type T; the low-resolution map is re-read from cache.
// The interpolation is torch's upsample_bilinear2d term by term (no
// contraction: the file is built with -ffp-contract=off), evaluated in
// float64: in fp32 the rounding of src = scale * dst alone (2^-24 src, 1e-6 at
// the right edge of a KITTI row) is several float16 steps wherever the four
// terms cancel to a small value.  In float64 the sum is the exact one to 1e-16,
// so the single rounding to the 16-bit type (through float32, as torch converts
// a float64 tensor) is the only one.
template <typename T> __device__ __forceinline__ double feat_to_d(T v);
template <> __device__ __forceinline__ double feat_to_d<float>(float v) { return (double)v; }
template <> __device__ __forceinline__ double feat_to_d<_Float16>(_Float16 v) { return (double)(float)v; }
template <> __device__ __forceinline__ double feat_to_d<__bf16>(__bf16 v) { return (double)(float)v; }

template <bool F16, typename T>
__global__ __launch_bounds__(256) void k_dep_pack(const float* __restrict__ depth, const T* __restrict__ feat,
                                                  const float* __restrict__ image, int b0, int h, int w, int H, int W,
                                                  double sy, double sx, int nbx, unsigned short* __restrict__ out) {
  const int img = blockIdx.x / nbx;
  const int i = (blockIdx.x - img * nbx) * 256 + threadIdx.x;
  const int HW = H * W;
  if (i >= HW * 8) return;
  const int chunk = i & 7, p = i >> 3;
  const int y = p / W, x = p - y * W;
  const int b = b0 + img;
  unsigned short s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (chunk < 5) {
    const double fy = sy * (double)y, fx = sx * (double)x;
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
    const double ly1 = fy - (double)y0, lx1 = fx - (double)x0;
    const double ly0 = 1.0 - ly1, lx0 = 1.0 - lx1;
    const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
    const int hw = h * w;
    const T* f = feat + (int64_t)b * 32 * hw;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = chunk * 8 + j - 1;   // slot j of this chunk is feature c
      if (c >= 0 && c < 32) {
        const T* fc = f + (int64_t)c * hw;
        const double v = ly0 * (lx0 * feat_to_d<T>(fc[o00]) + lx1 * feat_to_d<T>(fc[o01])) +
                         ly1 * (lx0 * feat_to_d<T>(fc[o10]) + lx1 * feat_to_d<T>(fc[o11]));
        s[j] = ActCvt<F16>::from_f((float)v);
      }
    }
    if (chunk == 0) s[0] = ActCvt<F16>::from_f(depth[(int64_t)b * HW + p]);
    if (chunk == 4) {
      const float* im = image + (int64_t)b * 3 * HW + p;
#pragma unroll
      for (int k = 0; k < 3; ++k) s[1 + k] = ActCvt<F16>::from_f(im[(int64_t)k * HW]);
    }
  }
  uint4 v;
  v.x = s[0] | ((unsigned)s[1] << 16);
  v.y = s[2] | ((unsigned)s[3] << 16);
  v.z = s[4] | ((unsigned)s[5] << 16);
  v.w = s[6] | ((unsigned)s[7] << 16);
  *reinterpret_cast<uint4*>(out + ((int64_t)img * HW + p) * 64 + chunk * 8) = v;
}

template <bool F16, int NG>
void launch_conv2(hipStream_t s, const void* in, int images, int cin, int h, int w, const void* weights, int cout,
                  int dilation, const float* scale, const float* bias, int relu, const float* residual1, void* out) {
  constexpr int R = rows_of(NG);
  const int ntx = (w + kTileX - 1) / kTileX, nty = (h + R - 1) / R;
  const unsigned lds = (unsigned)(w_bytes(NG) + in_bytes(NG, dilation));
  hipLaunchKernelGGL((k_conv2<F16, NG>), dim3((unsigned)(ntx * nty * images)), dim3(kThreads), lds, s,
                     (const unsigned short*)in, cin, (const unsigned short*)weights, scale, bias, relu, residual1,
                     cout == 1 ? nullptr : (unsigned short*)out, cout == 1 ? (float*)out : nullptr, cout, dilation, h,
                     w, ntx, nty);
}
static_assert(w_bytes(2) + in_bytes(2, kMaxDil) <= 64 * 1024 && w_bytes(4) + in_bytes(4, kMaxDil) <= 64 * 1024,
              "a stage fits the default 64 KB of dynamic LDS, two blocks per CU");

template <bool F16>
int conv2_lp(const void* in, int images, int cin, int h, int w, const void* weights, int cout, int dilation,
             const float* scale, const float* bias, int relu, const float* residual1, void* out, void* stream) {
  SFM_REQUIRE(in && weights && scale && bias && out, "null pointer argument");
  SFM_REQUIRE(cin == 32 || cin == 64 || cin == 96 || cin == 128, "cin must be 32, 64, 96 or 128");
  SFM_REQUIRE(cout == 1 || cout == 32 || cout == 64 || cout == 96 || cout == 128, "cout must be 1, 32, 64, 96 or 128");
  SFM_REQUIRE(dilation >= 1 && dilation <= kMaxDil, "dilation must be 1..16");
  SFM_REQUIRE(cout == 1 || residual1 == nullptr, "residual1 needs cout 1");
  SFM_REQUIRE(images >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)h * w * cin < ((int64_t)1 << 31), "conv image too large (32-bit in-image offsets)");
  SFM_REQUIRE(in != out && (const void*)residual1 != out, "conv output must not alias its inputs");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)weights & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                  ((uintptr_t)scale & 15) == 0 && ((uintptr_t)bias & 15) == 0,
              "conv operands must be 16-byte aligned");
  const int ng = cout == 1 ? 1 : cout / 32;
  const int64_t nblk = (int64_t)((w + kTileX - 1) / kTileX) * ((h + rows_of(ng) - 1) / rows_of(ng)) * images;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "conv grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("context_conv2", s);
  switch (ng) {
    case 1: launch_conv2<F16, 1>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
    case 2: launch_conv2<F16, 2>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
    case 3: launch_conv2<F16, 3>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
    default: launch_conv2<F16, 4>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
  }
  SFM_LAUNCHED();
  return SFM_OK;
}

template <bool F16>
int context_pack(const float* ctx, const float* planes, int batch, int nlabel, int l0, int nl, int channels, int h,
                 int w, void* out, void* stream) {
  SFM_REQUIRE(ctx && planes && out, "null pointer argument");
  SFM_REQUIRE(channels == 32, "the context stack's first layer takes 32 feature channels + 1 plane");
  SFM_REQUIRE(batch >= 1 && nlabel >= 1 && h >= 1 && w >= 1, "invalid context shape");
  SFM_REQUIRE(l0 >= 0 && nl >= 1 && l0 <= nlabel - nl, "plane range outside the volume");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 28), "context map too large");
  SFM_REQUIRE(((uintptr_t)out & 15) == 0, "output must be 16-byte aligned");
  const int64_t total = (int64_t)batch * nl * h * w * 8;
  const int64_t nblk = (total + 255) / 256;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "context pack grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("context_pack", s);
  hipLaunchKernelGGL(k_context_pack<F16>, dim3((unsigned)nblk), dim3(256), 0, s, ctx, planes, nlabel, l0, nl, channels,
                     h * w, total, (unsigned short*)out);
  SFM_LAUNCHED();
  return SFM_OK;
}

template <bool F16>
int dep_context_pack(const float* depth, const void* feat, int feat_dtype, const float* image, int batch, int b0,
                     int nb, int channels, int h, int w, int H, int W, void* out, void* stream) {
  SFM_REQUIRE(depth && feat && image && out, "null pointer argument");
  SFM_REQUIRE(feat_dtype >= 0 && feat_dtype <= 2, "feat_dtype must be 0 (float32), 1 (bfloat16) or 2 (float16)");
  SFM_REQUIRE(channels == 32, "the refinement stack's first layer takes 1 depth + 32 feature + 3 image channels");
  SFM_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "invalid refinement shape");
  SFM_REQUIRE(b0 >= 0 && nb >= 1 && b0 <= batch - nb, "pair range outside the batch");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 28), "feature map too large");
  SFM_REQUIRE((int64_t)H * W < ((int64_t)1 << 28), "image too large");
  SFM_REQUIRE(((uintptr_t)out & 15) == 0, "output must be 16-byte aligned");
  const int nbx = (int)(((int64_t)H * W * 8 + 255) / 256);
  SFM_REQUIRE((int64_t)nbx * nb < ((int64_t)1 << 31), "refinement pack grid too large");
  // torch's area_pixel_compute_scale for align_corners=True, in float64
  const double sy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
  const double sx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("dep_context_pack", s);
  const dim3 grid((unsigned)(nbx * nb)), block(256);
  unsigned short* o = (unsigned short*)out;
  if (feat_dtype == 0)
    hipLaunchKernelGGL((k_dep_pack<F16, float>), grid, block, 0, s, depth, (const float*)feat, image, b0, h, w, H, W,
                       sy, sx, nbx, o);
  else if (feat_dtype == 1)
    hipLaunchKernelGGL((k_dep_pack<F16, __bf16>), grid, block, 0, s, depth, (const __bf16*)feat, image, b0, h, w, H,
                       W, sy, sx, nbx, o);
  else
    hipLaunchKernelGGL((k_dep_pack<F16, _Float16>), grid, block, 0, s, depth, (const _Float16*)feat, image, b0, h, w,
                       H, W, sy, sx, nbx, o);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_conv2_f16(const void* in, int images, int cin, int h, int w, const void* weights, int cout, int dilation,
                  const float* scale, const float* bias, int relu, const float* residual1, void* out, void* stream) {
  return conv2_lp<true>(in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out, stream);
}

int sfm_conv2_bf16(const void* in, int images, int cin, int h, int w, const void* weights, int cout, int dilation,
                   const float* scale, const float* bias, int relu, const float* residual1, void* out, void* stream) {
  return conv2_lp<false>(in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out, stream);
}

int sfm_context_pack_f16(const float* ctx, const float* planes, int batch, int nlabel, int l0, int nl, int channels,
                         int h, int w, void* out, void* stream) {
  return context_pack<true>(ctx, planes, batch, nlabel, l0, nl, channels, h, w, out, stream);
}

int sfm_context_pack_bf16(const float* ctx, const float* planes, int batch, int nlabel, int l0, int nl, int channels,
                          int h, int w, void* out, void* stream) {
  return context_pack<false>(ctx, planes, batch, nlabel, l0, nl, channels, h, w, out, stream);
}

int sfm_dep_context_pack_f16(const float* depth, const void* feat, int feat_dtype, const float* image, int batch,
                             int b0, int nb, int channels, int h, int w, int H, int W, void* out, void* stream) {
  return dep_context_pack<true>(depth, feat, feat_dtype, image, batch, b0, nb, channels, h, w, H, W, out, stream);
}

int sfm_dep_context_pack_bf16(const float* depth, const void* feat, int feat_dtype, const float* image, int batch,
                              int b0, int nb, int channels, int h, int w, int H, int W, void* out, void* stream) {
  return dep_context_pack<false>(depth, feat, feat_dtype, image, batch, b0, nb, channels, h, w, H, W, out, stream);
}

}  // extern "C"
