// The backward of PSNet's per-plane context stack (models/PSNet.py:17-26
// convtext, 64-71 the seven dilated stages, applied per plane at 175-190) in
// float16 on the gfx950 matrix cores: the three products a training step needs
// beside the forward (context.hip).
//
// The weight gradient of a 3x3 / stride 1 / pad = dilation stage is
// k_conv2_wgrad<NG, 3, 1> (conv2_wgrad.hip), the kernel the feature CNN's
// layers run too: sfm_conv2_wgrad_f16 checks its arguments and calls that
// file's launcher.
//
// The data gradient is k_conv2 itself (conv2_tile.h) on flipped weights with
// the MASK epilogue; k_context_unpack_grad carries the first stage's gradient
// back to PSNet's tensors.  The full-resolution refinement stack dep_convs
// (PSNet.py:218-221) runs the same two products; k_dep_unpack_grad is the
// backward of its pack's bilinear upsample into the features.
#include <string>
#include "conv2_tile.h"
#include "conv2_wgrad.h"

namespace sfm {
namespace {

// The first stage's data gradient g [batch][nl][h][w][64] (channels 0..31 the
// features', 32 the plane's, the rest ignored) back to PSNet's tensors.  One
// thread per (pair, pixel, 8-channel chunk), as k_context_pack: chunks 0..3 add
// the planes' feature gradients in ascending plane order in float32, onto
// grad_ctx's value unless `first`; chunk 4 writes every plane's gradient plus
// grad_out's, the gradient of the "+ plane" residual.
__global__ __launch_bounds__(256) void k_context_unpack_grad(const unsigned short* __restrict__ g,
                                                             const float* __restrict__ grad_out, int nlabel, int l0,
                                                             int nl, int hw, int64_t total, int first,
                                                             float* __restrict__ grad_ctx,
                                                             float* __restrict__ grad_planes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int chunk = (int)(i & 7);
  const int64_t bp = i >> 3;                      // b * hw + p
  const int p = (int)(bp % hw), b = (int)(bp / hw);
  if (chunk > 4) return;
  const unsigned short* gp = g + ((int64_t)b * nl * hw + p) * 64 + chunk * 8;
  if (chunk == 4) {
    for (int l = 0; l < nl; ++l) {
      const int64_t o = ((int64_t)b * nlabel + l0 + l) * hw + p;
      grad_planes[o] = ActCvt<true>::to_f(gp[(int64_t)l * hw * 64]) + grad_out[o];
    }
    return;
  }
  float* c = grad_ctx + ((int64_t)b * 32 + chunk * 8) * hw + p;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = first ? 0.0f : c[(int64_t)j * hw];
  for (int l = 0; l < nl; ++l) {
    const uint4 v = *reinterpret_cast<const uint4*>(gp + (int64_t)l * hw * 64);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[2 * j] = s[2 * j] + ActCvt<true>::to_f((unsigned short)(w[j] & 0xffffu));
      s[2 * j + 1] = s[2 * j + 1] + ActCvt<true>::to_f((unsigned short)(w[j] >> 16));
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) c[(int64_t)j * hw] = s[j];
}

// The first destination index d in [0, n_dst) whose forward source index
// min((int)(scale d), n_src - 1) -- k_dep_pack's expression (context.hip) -- is
// at least t, or n_dst: a bisection over the forward's own expression, which
// is monotone in d (a rounded product by a non-negative constant, a
// truncation, a min).
__device__ __forceinline__ int dep_first_at_least(double scale, int n_src, int n_dst, int t) {
  int lo = 0, hi = n_dst;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (min((int)(scale * (double)mid), n_src - 1) >= t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The backward of k_dep_pack's bilinear upsample (models/PSNet.py:218-221) into
// the features: g [nb][H][W][64] is the first stage's data gradient, channels
// 1..32 the upsampled features'.  A gather: one thread per (pair, source pixel
// (i, j), 16-byte chunk 0..4 of g).  The destination rows that read source row
// i are those whose y0 is i - 1 or i (y1 = y0 + (y0 < h - 1)), a contiguous
// range found by bisection on the forward's index expression; every row and
// column of the range is then weighted with the forward's own y0, y1, ly0, ly1
// in float64,
//   wy = ly0 [y0 == i] + ly1 [y1 == i],
// so no inverted formula can disagree with k_dep_pack at a rounding boundary.
// Rows ascending, then columns ascending, summed in float64 and rounded once to
// float32: no atomics, the same bits from call to call and for any chunking.
// Slot s of chunk k is feature 8 k + s - 1 (k_dep_pack's layout): chunk 0 writes
// features 0..6, chunks 1..3 eight each, chunk 4 feature 31.  A source pixel
// that no destination reads is written as +0.
__global__ __launch_bounds__(256) void k_dep_unpack_grad(const unsigned short* __restrict__ g, int b0, int h, int w,
                                                         int H, int W, double sy, double sx, int64_t total,
                                                         float* __restrict__ grad_feat) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int chunk = (int)(t % 5);
  const int64_t sp = t / 5;                       // img * h * w + i * w + j
  const int hw = h * w;
  const int p = (int)(sp % hw), img = (int)(sp / hw);
  const int i = p / w, j = p - i * w;
  const int ya = dep_first_at_least(sy, h, H, i - 1), yb = dep_first_at_least(sy, h, H, i + 1);
  const int xa = dep_first_at_least(sx, w, W, j - 1), xb = dep_first_at_least(sx, w, W, j + 1);
  const unsigned short* gp = g + (int64_t)img * H * W * 64 + chunk * 8;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int y = ya; y < yb; ++y) {
    const double fy = sy * (double)y;
    const int y0 = min((int)fy, h - 1);
    const int y1 = y0 + (y0 < h - 1);
    const double ly1 = fy - (double)y0, ly0 = 1.0 - ly1;
    const double wy = (y0 == i ? ly0 : 0.0) + (y1 == i ? ly1 : 0.0);
    const unsigned short* row = gp + (int64_t)y * W * 64;
    for (int x = xa; x < xb; ++x) {
      const double fx = sx * (double)x;
      const int x0 = min((int)fx, w - 1);
      const int x1 = x0 + (x0 < w - 1);
      const double lx1 = fx - (double)x0, lx0 = 1.0 - lx1;
      const double wx = (x0 == j ? lx0 : 0.0) + (x1 == j ? lx1 : 0.0);
      const double wt = wy * wx;
      const uint4 v = *reinterpret_cast<const uint4*>(row + (int64_t)x * 64);
      const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s[2 * k] = s[2 * k] + wt * (double)ActCvt<true>::to_f((unsigned short)(u[k] & 0xffffu));
        s[2 * k + 1] = s[2 * k + 1] + wt * (double)ActCvt<true>::to_f((unsigned short)(u[k] >> 16));
      }
    }
  }
  float* out = grad_feat + (int64_t)(b0 + img) * 32 * hw + p;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = chunk * 8 + k - 1;              // slot k of this chunk is feature c
    if (c >= 0 && c < 32) out[(int64_t)c * hw] = (float)s[k];
  }
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_conv2_wgrad_f16_workspace_bytes(int images, int cin, int cout_pad, int h, int w) {
  if (images < 1 || h < 1 || w < 1 || !chan_ok(cin) || !chan_ok(cout_pad)) return 0;
  return xw_ws_bytes(xw_plan(images, cout_pad, h, w, 3, 1), cin, cout_pad, 3);
}

int sfm_conv2_wgrad_f16(const void* in, const void* grad_out, int images, int cin, int cout_pad, int h, int w,
                        int dilation, float* grad_weights, void* workspace, size_t workspace_bytes, void* stream) {
  SFM_REQUIRE(in && grad_out && grad_weights, "null pointer argument");
  SFM_REQUIRE(chan_ok(cin), "cin must be 32, 64, 96 or 128");
  SFM_REQUIRE(chan_ok(cout_pad),
              "cout_pad must be 32, 64, 96 or 128 (a cout 1 stage passes its gradient zero-padded to 32 channels)");
  SFM_REQUIRE(dilation >= 1 && dilation <= kMaxDil, "dilation must be 1..16");
  SFM_REQUIRE(images >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)h * w * 128 < ((int64_t)1 << 31), "conv image too large (32-bit in-image offsets)");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)grad_weights & 15) == 0,
              "conv operands must be 16-byte aligned");
  const XwPlan p = xw_plan(images, cout_pad, h, w, 3, 1);
  const size_t need = xw_ws_bytes(p, cin, cout_pad, 3);
  if (!workspace || workspace_bytes < need) {
    set_error("conv2 weight-gradient workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  SFM_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  const size_t pix = (size_t)images * h * w;
  const size_t in_bytes = pix * cin * 2, go_bytes = pix * cout_pad * 2;
  const size_t gw_bytes = (size_t)9 * cout_pad * cin * sizeof(float);
  SFM_REQUIRE(!overlap(grad_weights, gw_bytes, in, in_bytes) && !overlap(grad_weights, gw_bytes, grad_out, go_bytes) &&
                  !overlap(grad_weights, gw_bytes, workspace, need) && !overlap(workspace, need, in, in_bytes) &&
                  !overlap(workspace, need, grad_out, go_bytes),
              "conv weight-gradient outputs must not alias its inputs");
  const int64_t slices = (int64_t)3 * (cin / 32) * (cout_pad / 32 / p.ng);
  SFM_REQUIRE(slices <= 65535, "conv weight-gradient grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv2_wgrad", s);
  return launch_conv2_wgrad(s, p, in, grad_out, cin, cout_pad, h, w, 3, 1, dilation, workspace, grad_weights);
}

int sfm_conv2_dgrad_f16(const void* grad_out, int images, int cout_pad, int h, int w, const void* weights, int cin_pad,
                        int dilation, const void* act, void* grad_in, void* stream) {
  SFM_REQUIRE(grad_out && weights && grad_in, "null pointer argument");
  SFM_REQUIRE(chan_ok(cout_pad),
              "cout_pad must be 32, 64, 96 or 128 (a cout 1 stage passes its gradient zero-padded to 32 channels)");
  SFM_REQUIRE(chan_ok(cin_pad), "cin_pad must be 32, 64, 96 or 128");
  SFM_REQUIRE(dilation >= 1 && dilation <= kMaxDil, "dilation must be 1..16");
  SFM_REQUIRE(images >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)h * w * cout_pad < ((int64_t)1 << 31), "conv image too large (32-bit in-image offsets)");
  SFM_REQUIRE(grad_out != grad_in && act != grad_in, "conv output must not alias its inputs");
  SFM_REQUIRE(((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)weights & 15) == 0 && ((uintptr_t)grad_in & 15) == 0 &&
                  ((uintptr_t)act & 15) == 0,
              "conv operands must be 16-byte aligned");
  const int ng = cin_pad / 32;
  const int64_t nblk = (int64_t)((w + kTileX - 1) / kTileX) * ((h + rows_of(ng) - 1) / rows_of(ng)) * images;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "conv grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv2_dgrad", s);
  // k_conv2 on the gradient: its cin is the forward stage's cout_pad, its cout the forward's cin_pad
  switch (ng) {
    case 1: launch_conv2<true, 1, true, true>(s, grad_out, images, cout_pad, h, w, weights, cin_pad, dilation, nullptr, nullptr, 0, act, grad_in); break;
    case 2: launch_conv2<true, 2, true, true>(s, grad_out, images, cout_pad, h, w, weights, cin_pad, dilation, nullptr, nullptr, 0, act, grad_in); break;
    case 3: launch_conv2<true, 3, true, true>(s, grad_out, images, cout_pad, h, w, weights, cin_pad, dilation, nullptr, nullptr, 0, act, grad_in); break;
    default: launch_conv2<true, 4, true, true>(s, grad_out, images, cout_pad, h, w, weights, cin_pad, dilation, nullptr, nullptr, 0, act, grad_in); break;
  }
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_context_unpack_grad_f16(const void* grad_in0, const float* grad_out, int batch, int nlabel, int l0, int nl,
                                int h, int w, int first, float* grad_ctx, float* grad_planes, void* stream) {
  SFM_REQUIRE(grad_in0 && grad_out && grad_ctx && grad_planes, "null pointer argument");
  SFM_REQUIRE(batch >= 1 && nlabel >= 1 && h >= 1 && w >= 1, "invalid context shape");
  SFM_REQUIRE(l0 >= 0 && nl >= 1 && l0 <= nlabel - nl, "plane range outside the volume");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 28), "context map too large");
  SFM_REQUIRE(((uintptr_t)grad_in0 & 15) == 0, "the stage gradient must be 16-byte aligned");
  SFM_REQUIRE(((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)grad_ctx & 3) == 0 && ((uintptr_t)grad_planes & 3) == 0,
              "float operands must be 4-byte aligned");
  SFM_REQUIRE((const void*)grad_ctx != (const void*)grad_planes && (const void*)grad_planes != (const void*)grad_out &&
                  (const void*)grad_ctx != (const void*)grad_out,
              "context gradient outputs must not alias each other or grad_out");
  const int64_t total = (int64_t)batch * h * w * 8;
  const int64_t nblk = (total + 255) / 256;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "context unpack grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("context_unpack_grad", s);
  hipLaunchKernelGGL(k_context_unpack_grad, dim3((unsigned)nblk), dim3(256), 0, s, (const unsigned short*)grad_in0,
                     grad_out, nlabel, l0, nl, h * w, total, first ? 1 : 0, grad_ctx, grad_planes);
  SFM_LAUNCHED();
  return SFM_OK;
}

int sfm_dep_context_unpack_grad_f16(const void* grad_in0, int batch, int b0, int nb, int channels, int h, int w, int H,
                                    int W, float* grad_feat, void* stream) {
  SFM_REQUIRE(grad_in0 && grad_feat, "null pointer argument");
  SFM_REQUIRE(channels == 32, "the refinement stack's first layer takes 1 depth + 32 feature + 3 image channels");
  SFM_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "invalid refinement shape");
  SFM_REQUIRE(b0 >= 0 && nb >= 1 && b0 <= batch - nb, "pair range outside the batch");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 28), "feature map too large");
  SFM_REQUIRE((int64_t)H * W < ((int64_t)1 << 28), "image too large");
  SFM_REQUIRE(((uintptr_t)grad_in0 & 15) == 0, "the stage gradient must be 16-byte aligned");
  SFM_REQUIRE(((uintptr_t)grad_feat & 3) == 0, "float operands must be 4-byte aligned");
  const int64_t total = (int64_t)nb * h * w * 5;
  const int64_t nblk = (total + 255) / 256;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "refinement unpack grid too large");
  // k_dep_pack's scales: torch's area_pixel_compute_scale for align_corners=True, in float64
  const double sy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
  const double sx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("dep_context_unpack_grad", s);
  hipLaunchKernelGGL(k_dep_unpack_grad, dim3((unsigned)nblk), dim3(256), 0, s, (const unsigned short*)grad_in0, b0, h, w,
                     H, W, sy, sx, total, grad_feat);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
