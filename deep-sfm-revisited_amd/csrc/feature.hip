// PSNet's feature CNN (models/submodule.py:108-184 feature_extraction; its
// BasicBlock 22-44, convbn 11-15) on the gfx950 matrix cores, float16:
//
//   sfm_image_pack_f16   the image, channels-last and padded to 32 channels
//   sfm_conv2x_f16       every Conv2d + folded BatchNorm2d [+ ReLU] [+ residual]
//   sfm_avgpool_f16      branch1..4's AvgPool2d
//   sfm_spp_pack_f16     cat(raw, skip, upsampled branches), lastconv's input
//
// Activations are channels-last float16, [images][H][W][C]; weights
// [ksize^2][cout_pad][cin], tap = kh*ksize + kw (context.hip's layout).
//
// sfm_conv2x_f16 runs the 3 x 3 / stride 1 layers -- 98 % of the arithmetic --
// on k_conv2 (conv2_tile.h), the context stack's tile, with the BasicBlock's
// "+ x" as a 16-bit residual in its epilogue.  The two stride-2 layers and the
// 1 x 1 layers run on k_conv2s below, the same implicit GEMM without the
// register prefetch: one block = 4 waves = 4 output rows x 64 output columns,
// a wave 2 rows x 32 columns and all NG output-channel groups; a stage is one
// (kernel row, 32-channel chunk): 4 input rows x SW columns and KS x cout_pad
// x 32 weights in LDS, SW = 63 stride + KS (129 columns at 3 x 3 / stride 2).
#include "conv2_tile.h"

namespace sfm {
namespace {

constexpr int kRowsS = 4;  // output rows per block of k_conv2s
constexpr int sw_of(int ks, int stride) { return (kTileX - 1) * stride + ks; }
constexpr int lds_bytes_s(int ng, int ks, int stride) { return ks * ng * 32 * 64 + kRowsS * sw_of(ks, stride) * 64; }
static_assert(lds_bytes_s(4, 3, 2) <= 64 * 1024, "the largest stage fits the default 64 KB of dynamic LDS");

template <int NG, int KS, int STRIDE>
__global__ __launch_bounds__(kThreads) void k_conv2s(
    const unsigned short* __restrict__ in, int cin, const unsigned short* __restrict__ wpk,
    const float* __restrict__ scale, const float* __restrict__ bias, int relu, const unsigned short* __restrict__ res,
    unsigned short* __restrict__ out, int cout, int Hin, int Win, int Hout, int Wout, int ntx, int nty) {
  using A = Act<true>;
  using v8 = typename A::v8;
  constexpr int R = kRowsS, PB = R / 2;
  constexpr int SW = sw_of(KS, STRIDE);   // staged input columns
  constexpr int PAD = KS == 3 ? 1 : 0;
  constexpr int WROWS = KS * NG * 32;     // weight rows per stage
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* lds_w = lds;
  unsigned char* lds_in = lds + WROWS * 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int rest = blockIdx.x;
  const int tx = rest % ntx;
  rest /= ntx;
  const int ty = rest % nty, img = rest / nty;
  const int x0 = tx * kTileX, y0 = ty * R;
  const int r = lane & 31, h = lane >> 5;
  const int wrow = (wave >> 1) * PB, wcol = (wave & 1) * 32;
  const int nchunk = cin >> 5;
  const int rowstride = Win * cin;
  const unsigned short* img_in = in + (int64_t)img * Hin * Win * cin;
  const int gx0 = x0 * STRIDE - PAD;
  const int mc = tid & 3;

  f32x16 acc[NG][PB];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int o = 0; o < PB; ++o)
      for (int i = 0; i < 16; ++i) acc[g][o][i] = 0.0f;

  for (int s = 0; s < KS * nchunk; ++s) {  // stage s: dy = s / nchunk, channel chunk cc = s % nchunk
    const int dy = s / nchunk, cc = s - dy * nchunk;
    __syncthreads();  // the previous stage's operand reads are done
    const unsigned short* pl = img_in + cc * 32 + mc * 8;
    for (int i = tid >> 2; i < R * SW; i += kThreads / 4) {
      const int ry = i / SW, sc = i - ry * SW;
      const int gy = (y0 + ry) * STRIDE + dy - PAD, gx = gx0 + sc;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gy >= 0 && gy < Hin && gx >= 0 && gx < Win) v = *reinterpret_cast<const uint4*>(pl + gy * rowstride + gx * cin);
      *reinterpret_cast<uint4*>(lds_in + i * 64 + swz(mc, sc) * 16) = v;
    }
    const unsigned short* wb = wpk + (int64_t)dy * WROWS * cin + cc * 32 + mc * 8;
    for (int i = tid >> 2; i < WROWS; i += kThreads / 4)
      *reinterpret_cast<uint4*>(lds_w + i * 64 + swz(mc, i) * 16) = *reinterpret_cast<const uint4*>(wb + i * cin);
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int c = kb * 2 + h;
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) {
        v8 wf[NG], xf[PB];
#pragma unroll
        for (int g = 0; g < NG; ++g)
          wf[g] = *reinterpret_cast<const v8*>(lds_w + ((dx * NG + g) * 32 + r) * 64 + swz(c, r) * 16);
        const int p = (wcol + r) * STRIDE + dx;
#pragma unroll
        for (int o = 0; o < PB; ++o)
          xf[o] = *reinterpret_cast<const v8*>(lds_in + ((wrow + o) * SW + p) * 64 + swz(c, p) * 16);
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int o = 0; o < PB; ++o) acc[g][o] = A::mfma(wf[g], xf[o], acc[g][o]);
      }
    }
  }

  const int x = x0 + wcol + r;
  if (x >= Wout) return;
  conv2_store16<A, NG, PB, true>(acc, scale, bias, relu, res, out, cout, img, y0 + wrow, x, h, Hout, Wout);
}

// [B][3][H][W] float32 -> [B][H][W][32] float16: one thread per (pixel,
// 8-channel chunk), 16-byte stores; chunk 0 holds the image, 1..3 zeros.
__global__ __launch_bounds__(256) void k_image_pack(const float* __restrict__ image, int hw, int64_t total,
                                                    unsigned short* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  uint4 v = make_uint4(0, 0, 0, 0);
  if ((i & 3) == 0) {
    const int64_t pixel = i >> 2;
    const int64_t b = pixel / hw;
    const float* im = image + b * 3 * hw + (pixel - b * hw);
    v.x = (unsigned)ActCvt<true>::from_f(im[0]) | ((unsigned)ActCvt<true>::from_f(im[hw]) << 16);
    v.y = (unsigned)ActCvt<true>::from_f(im[2 * (int64_t)hw]);
  }
  *reinterpret_cast<uint4*>(out + i * 8) = v;
}

// AvgPool2d(p, stride p): one block per output pixel.  Thread t sums chunk
// t % (C/8) (8 channels) over every (256 / (C/8))-th pixel of the p x p window
// in fp32; the slices are then added in order, times 1 / (p p), rounded once.
// The order of the sum depends on C and p alone.
__global__ __launch_bounds__(256) void k_avgpool(const unsigned short* __restrict__ in, int h, int w, int C, int p,
                                                 int ho, int wo, unsigned short* __restrict__ out) {
  __shared__ float part[256][8];
  const int nch = C >> 3, nsl = 256 / nch;
  const int tid = threadIdx.x;
  const int chunk = tid % nch, slice = tid / nch;
  int rest = blockIdx.x;
  const int ox = rest % wo;
  rest /= wo;
  const int oy = rest % ho, img = rest / ho;
  float s[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (slice < nsl) {
    const unsigned short* base = in + (((int64_t)img * h + (int64_t)oy * p) * w + (int64_t)ox * p) * C + chunk * 8;
    for (int k = slice; k < p * p; k += nsl) {
      const int iy = k / p, ix = k - iy * p;
      const uint4 v = *reinterpret_cast<const uint4*>(base + ((int64_t)iy * w + ix) * C);
      const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[2 * j] += ActCvt<true>::to_f((unsigned short)(u[j] & 0xffffu));
        s[2 * j + 1] += ActCvt<true>::to_f((unsigned short)(u[j] >> 16));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[tid][j] = s[j];
  __syncthreads();
  if (tid >= nch) return;
  for (int k = 1; k < nsl; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += part[k * nch + tid][j];
  const float inv = 1.0f / (float)(p * p);
  uint4 v;
  v.x = (unsigned)ActCvt<true>::from_f(s[0] * inv) | ((unsigned)ActCvt<true>::from_f(s[1] * inv) << 16);
  v.y = (unsigned)ActCvt<true>::from_f(s[2] * inv) | ((unsigned)ActCvt<true>::from_f(s[3] * inv) << 16);
  v.z = (unsigned)ActCvt<true>::from_f(s[4] * inv) | ((unsigned)ActCvt<true>::from_f(s[5] * inv) << 16);
  v.w = (unsigned)ActCvt<true>::from_f(s[6] * inv) | ((unsigned)ActCvt<true>::from_f(s[7] * inv) << 16);
  *reinterpret_cast<uint4*>(out + (((int64_t)img * ho + oy) * wo + ox) * C + tid * 8) = v;
}

// lastconv's input [images][h][w][320] = cat(raw 64, skip 128, up(branch4),
// up(branch3), up(branch2), up(branch1)) (submodule.py:181).  blockIdx.y is
// the segment: 0 raw, 1 skip, 2..5 the four 32-channel branch maps in that
// order, each [images][bh][bw][32], upsampled bilinearly (align_corners=True)
// as k_dep_pack (context.hip) does: torch's upsample_bilinear2d term by term
// in float64, rounded once (through float32, as torch converts a float64
// tensor).  One thread per (pixel, 8-channel chunk), 16-byte loads and stores.
struct SppBranches {
  const unsigned short* map[4];
  int bh[4], bw[4];
  double sy[4], sx[4];
};

__global__ __launch_bounds__(256) void k_spp_pack(const unsigned short* __restrict__ raw,
                                                  const unsigned short* __restrict__ skip, SppBranches br, int h, int w,
                                                  int nbx, unsigned short* __restrict__ out) {
  const int seg = blockIdx.y;
  const int nck = seg == 0 ? 8 : seg == 1 ? 16 : 4;            // 16-byte chunks of this segment
  const int cbase = seg == 0 ? 0 : seg == 1 ? 64 : 192 + 32 * (seg - 2);
  const int img = blockIdx.x / nbx;
  const int i = (blockIdx.x - img * nbx) * 256 + threadIdx.x;
  const int hw = h * w;
  if (i >= hw * nck) return;
  const int p = i / nck, chunk = i - p * nck;
  const int64_t pix = (int64_t)img * hw + p;
  uint4 v;
  if (seg < 2) {
    const unsigned short* src = seg == 0 ? raw + pix * 64 : skip + pix * 128;
    v = *reinterpret_cast<const uint4*>(src + chunk * 8);
  } else {
    const int b = seg - 2;
    const int bh = br.bh[b], bw = br.bw[b];
    const int y = p / w, x = p - y * w;
    const double fy = br.sy[b] * (double)y, fx = br.sx[b] * (double)x;
    const int y0 = min((int)fy, bh - 1), x0 = min((int)fx, bw - 1);
    const int y1 = y0 + (y0 < bh - 1), x1 = x0 + (x0 < bw - 1);
    const double ly1 = fy - (double)y0, lx1 = fx - (double)x0;
    const double ly0 = 1.0 - ly1, lx0 = 1.0 - lx1;
    const unsigned short* m = br.map[b] + (int64_t)img * bh * bw * 32 + chunk * 8;
    const uint4 q00 = *reinterpret_cast<const uint4*>(m + (y0 * bw + x0) * 32);
    const uint4 q01 = *reinterpret_cast<const uint4*>(m + (y0 * bw + x1) * 32);
    const uint4 q10 = *reinterpret_cast<const uint4*>(m + (y1 * bw + x0) * 32);
    const uint4 q11 = *reinterpret_cast<const uint4*>(m + (y1 * bw + x1) * 32);
    const unsigned u00[4] = {q00.x, q00.y, q00.z, q00.w}, u01[4] = {q01.x, q01.y, q01.z, q01.w};
    const unsigned u10[4] = {q10.x, q10.y, q10.z, q10.w}, u11[4] = {q11.x, q11.y, q11.z, q11.w};
    unsigned s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = j >> 1, sh = (j & 1) * 16;
      const double v00 = (double)ActCvt<true>::to_f((unsigned short)((u00[k] >> sh) & 0xffffu));
      const double v01 = (double)ActCvt<true>::to_f((unsigned short)((u01[k] >> sh) & 0xffffu));
      const double v10 = (double)ActCvt<true>::to_f((unsigned short)((u10[k] >> sh) & 0xffffu));
      const double v11 = (double)ActCvt<true>::to_f((unsigned short)((u11[k] >> sh) & 0xffffu));
      const double val = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
      s[j] = ActCvt<true>::from_f((float)val);
    }
    v.x = s[0] | (s[1] << 16);
    v.y = s[2] | (s[3] << 16);
    v.z = s[4] | (s[5] << 16);
    v.w = s[6] | (s[7] << 16);
  }
  *reinterpret_cast<uint4*>(out + pix * 320 + cbase + chunk * 8) = v;
}

template <int NG, int KS, int STRIDE>
void launch_conv2s(hipStream_t s, const void* in, int images, int cin, int hin, int win, int hout, int wout,
                   const void* weights, int cout, const float* scale, const float* bias, int relu, const void* residual,
                   void* out) {
  const int ntx = (wout + kTileX - 1) / kTileX, nty = (hout + kRowsS - 1) / kRowsS;
  hipLaunchKernelGGL((k_conv2s<NG, KS, STRIDE>), dim3((unsigned)(ntx * nty * images)), dim3(kThreads),
                     (unsigned)lds_bytes_s(NG, KS, STRIDE), s, (const unsigned short*)in, cin,
                     (const unsigned short*)weights, scale, bias, relu, (const unsigned short*)residual,
                     (unsigned short*)out, cout, hin, win, hout, wout, ntx, nty);
}

template <int KS, int STRIDE>
void launch_conv2s_ng(int ng, hipStream_t s, const void* in, int images, int cin, int hin, int win, int hout, int wout,
                      const void* weights, int cout, const float* scale, const float* bias, int relu,
                      const void* residual, void* out) {
  switch (ng) {
    case 1: launch_conv2s<1, KS, STRIDE>(s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out); break;
    case 2: launch_conv2s<2, KS, STRIDE>(s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out); break;
    case 3: launch_conv2s<3, KS, STRIDE>(s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out); break;
    default: launch_conv2s<4, KS, STRIDE>(s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out); break;
  }
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_conv2x_f16(const void* in, int images, int cin, int hin, int win, const void* weights, int cout, int ksize,
                   int stride, int dilation, const float* scale, const float* bias, int relu, const void* residual,
                   void* out, void* stream) {
  SFM_REQUIRE(in && weights && scale && bias && out, "null pointer argument");
  SFM_REQUIRE(cin >= 32 && cin <= 320 && cin % 32 == 0, "cin must be a multiple of 32 from 32 to 320");
  SFM_REQUIRE(cout == 32 || cout == 64 || cout == 96 || cout == 128, "cout must be 32, 64, 96 or 128");
  SFM_REQUIRE(ksize == 3 || ksize == 1, "ksize must be 3 or 1");
  SFM_REQUIRE(stride == 1 || stride == 2, "stride must be 1 or 2");
  SFM_REQUIRE(dilation >= 1 && dilation <= kMaxDil, "dilation must be 1..16");
  SFM_REQUIRE(dilation == 1 || (ksize == 3 && stride == 1), "a 1 x 1 or stride 2 conv takes dilation 1 only");
  SFM_REQUIRE(!(relu && residual), "relu with a residual is not built (BasicBlock adds after a plain conv-BN)");
  SFM_REQUIRE(images >= 1 && hin >= 1 && win >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)hin * win * cin < ((int64_t)1 << 31), "conv image too large (32-bit in-image offsets)");
  SFM_REQUIRE(in != out && residual != out, "conv output must not alias its inputs");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)weights & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                  ((uintptr_t)scale & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)residual & 15) == 0,
              "conv operands must be 16-byte aligned");
  // pad = dilation (3 x 3) or 0 (1 x 1): Hout = (Hin + 2 pad - dilation (ksize - 1) - 1) / stride + 1
  const int hout = (hin - 1) / stride + 1, wout = (win - 1) / stride + 1;
  const int ng = cout / 32;
  const bool tile = ksize == 3 && stride == 1;
  const int rows = tile ? rows_of(ng) : kRowsS;
  const int64_t nblk = (int64_t)((wout + kTileX - 1) / kTileX) * ((hout + rows - 1) / rows) * images;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "conv grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("feature_conv2x", s);
  if (tile) {
    switch (ng) {
      case 1: launch_conv2<true, 1, true>(s, in, images, cin, hin, win, weights, cout, dilation, scale, bias, relu, residual, out); break;
      case 2: launch_conv2<true, 2, true>(s, in, images, cin, hin, win, weights, cout, dilation, scale, bias, relu, residual, out); break;
      case 3: launch_conv2<true, 3, true>(s, in, images, cin, hin, win, weights, cout, dilation, scale, bias, relu, residual, out); break;
      default: launch_conv2<true, 4, true>(s, in, images, cin, hin, win, weights, cout, dilation, scale, bias, relu, residual, out); break;
    }
  } else if (ksize == 3) {
    launch_conv2s_ng<3, 2>(ng, s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out);
  } else if (stride == 2) {
    launch_conv2s_ng<1, 2>(ng, s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out);
  } else {
    launch_conv2s_ng<1, 1>(ng, s, in, images, cin, hin, win, hout, wout, weights, cout, scale, bias, relu, residual, out);
  }
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_image_pack_f16(const float* image, int batch, int h, int w, void* out, void* stream) {
  SFM_REQUIRE(image && out, "null pointer argument");
  SFM_REQUIRE(batch >= 1 && h >= 1 && w >= 1, "invalid image shape");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 28), "image too large");
  SFM_REQUIRE(((uintptr_t)image & 15) == 0 && ((uintptr_t)out & 15) == 0, "image pack operands must be 16-byte aligned");
  const int64_t total = (int64_t)batch * h * w * 4;
  const int64_t nblk = (total + 255) / 256;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "image pack grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("feature_image_pack", s);
  hipLaunchKernelGGL(k_image_pack, dim3((unsigned)nblk), dim3(256), 0, s, image, h * w, total, (unsigned short*)out);
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_avgpool_f16(const void* in, int images, int h, int w, int channels, int pool, void* out, void* stream) {
  SFM_REQUIRE(in && out, "null pointer argument");
  SFM_REQUIRE(pool == 4 || pool == 8 || pool == 16 || pool == 32, "pool size must be 4, 8, 16 or 32");
  SFM_REQUIRE(channels >= 8 && channels <= 2048 && channels % 8 == 0, "channels must be a multiple of 8, at most 2048");
  SFM_REQUIRE(images >= 1 && h >= pool && w >= pool, "invalid pool shape (the map must hold one window)");
  SFM_REQUIRE(in != out, "pool output must not alias its input");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0, "pool operands must be 16-byte aligned");
  const int ho = h / pool, wo = w / pool;
  const int64_t nblk = (int64_t)images * ho * wo;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "pool grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("feature_avgpool", s);
  hipLaunchKernelGGL(k_avgpool, dim3((unsigned)nblk), dim3(256), 0, s, (const unsigned short*)in, h, w, channels, pool,
                     ho, wo, (unsigned short*)out);
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_spp_pack_f16(const void* raw, const void* skip, const void* const* branches, const int* branch_h,
                     const int* branch_w, int images, int h, int w, void* out, void* stream) {
  SFM_REQUIRE(raw && skip && branches && branch_h && branch_w && out, "null pointer argument");
  SFM_REQUIRE(images >= 1 && h >= 1 && w >= 1, "invalid feature map shape");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 24), "feature map too large");
  SFM_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)skip & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "spp pack operands must be 16-byte aligned");
  SppBranches br;
  for (int b = 0; b < 4; ++b) {
    SFM_REQUIRE(branches[b], "null pointer argument");
    SFM_REQUIRE(((uintptr_t)branches[b] & 15) == 0, "spp pack operands must be 16-byte aligned");
    SFM_REQUIRE(branch_h[b] >= 1 && branch_w[b] >= 1 && (int64_t)branch_h[b] * branch_w[b] < ((int64_t)1 << 24),
                "invalid branch map shape");
    SFM_REQUIRE(branches[b] != out, "spp pack output must not alias its inputs");
    br.map[b] = (const unsigned short*)branches[b];
    br.bh[b] = branch_h[b];
    br.bw[b] = branch_w[b];
    // torch's area_pixel_compute_scale for align_corners=True, in float64
    br.sy[b] = h > 1 ? (double)(branch_h[b] - 1) / (double)(h - 1) : 0.0;
    br.sx[b] = w > 1 ? (double)(branch_w[b] - 1) / (double)(w - 1) : 0.0;
  }
  SFM_REQUIRE(raw != out && skip != out, "spp pack output must not alias its inputs");
  const int nbx = (int)(((int64_t)h * w * 16 + 255) / 256);
  SFM_REQUIRE((int64_t)nbx * images < ((int64_t)1 << 31), "spp pack grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("feature_spp_pack", s);
  hipLaunchKernelGGL(k_spp_pack, dim3((unsigned)(nbx * images), 6), dim3(256), 0, s, (const unsigned short*)raw,
                     (const unsigned short*)skip, br, h, w, nbx, (unsigned short*)out);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
