// PSNet's per-plane context stack (models/PSNet.py:17-26 convtext, 64-71 the
// seven dilated stages 33 -> 128 -> 128 -> 128 -> 96 -> 64 -> 32 -> 1, applied
// per plane at 175-190) on the gfx950 matrix cores: each stage a 3x3 /
// stride 1 / pad = dilation Conv2d with its optional BatchNorm2d folded into a
// per-channel affine (eval mode) and a ReLU, the last one followed by the
// fp32 "+ plane" of PSNet.py:190.
//
// Layout in HBM: activations are channels-last 16-bit, [images][H][W][C] with
// C in {32, 64, 96, 128}; weights are packed per layer as [9 taps][cout_pad]
// [cin], tap = kh*3 + kw, cout_pad = cout rounded up to 32.  The convolution
// tile itself (k_conv2) is conv2_tile.h, shared with the feature CNN (feature.hip).
#include "conv2_tile.h"

namespace sfm {
namespace {

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
    case 1: launch_conv2<F16, 1, false>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
    case 2: launch_conv2<F16, 2, false>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
    case 3: launch_conv2<F16, 3, false>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
    default: launch_conv2<F16, 4, false>(s, in, images, cin, h, w, weights, cout, dilation, scale, bias, relu, residual1, out); break;
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
