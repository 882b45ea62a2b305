// The backward of one Conv2d of PSNet's feature CNN (models/submodule.py:11-15
// convbn, 22-44 BasicBlock with its downsample, 108-184 feature_extraction) in
// float16 on the gfx950 matrix cores, over sfm_conv2x_f16's layer set (feature.hip):
// 3 x 3 or 1 x 1, stride 1 or 2, 32..320 input channels.
//
// The weight gradient is k_conv2_wgrad<NG, KS, STRIDE> (conv2_wgrad.hip), the
// context stack's kernel; sfm_conv2x_wgrad_f16 checks its arguments and calls
// that file's launcher.  What this CNN's layers add to it is the stride 2 x
// stage: consecutive gy pixels read x pixels two apart, which the transposing
// read's 16-consecutive-pixel K axis cannot do, so a staged row holds x's
// columns split by parity and the three kw taps read three consecutive
// positions of the odd, even and odd images.
//
// The data gradient is a gather, rounded once to float16:
//   k_conv2x_dgrad1<NG, KS>  stride 1: k_conv2s' implicit GEMM (feature.hip) on gy
//     with the flipped, transposed weights Wd, dilated, for the NG groups of
//     input channels from ci0 of a cin-wide result (lastconv.0's 320 channels
//     are three launches into one tensor);
//   k_conv2x_dgrad2<NG, KS>  stride 2: one grad_in row per block; wave (b, half)
//     owns the 32 columns 2 j + b of one column parity, so that every pixel of
//     an MFMA has the same live taps: at 3 x 3 a row of parity a reads kernel
//     rows {1} or {0, 2} and a column of parity b kernel columns {1} or {0, 2}
//     -- 1, 2, 2 or 4 taps per parity class; at 1 x 1 the even-even class alone
//     has a tap and the other pixels are written as +0.
// At 3 x 3 / stride 1 / cin <= 128 both entry points run sfm_conv2_wgrad_f16 /
// sfm_conv2_dgrad_f16 (context_bwd.hip) and return their bits.
#include <string>
#include "conv2_tile.h"
#include "conv2_wgrad.h"

namespace sfm {
namespace {

// One wave's accumulators of a data-gradient tile rounded to float16: D[row = ci][col = pixel]; the lane holds
// pixel `pix` and channels co0 + 32 g + 8 q + 4 h + (0..3) in acc[g][4 q .. 4 q + 3]; `cin` is the channel stride.
template <int NG>
__device__ __forceinline__ void dgrad_store(const f32x16 (&acc)[NG], unsigned short* __restrict__ out, int64_t pix,
                                            int cin, int co0, int h) {
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned short v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ActCvt<true>::from_f(acc[g][4 * q + j]);
      uint2 st;
      st.x = (unsigned)v[0] | ((unsigned)v[1] << 16);
      st.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
      *reinterpret_cast<uint2*>(out + pix * cin + co0 + 32 * g + 8 * q + 4 * h) = st;
    }
}

constexpr int kDgRows = 4;  // grad_in rows per block of k_conv2x_dgrad1
constexpr int dg1_lds(int ng, int ks, int dil) { return ks * ng * 32 * 64 + kDgRows * (kTileX + (ks - 1) * dil) * 64; }
constexpr int dg2_lds(int ng, int ks) { return ks * ng * 32 * 64 + (kTileX + 1) * 64; }
static_assert(dg1_lds(4, 3, kMaxDil) <= 64 * 1024, "the largest stage fits the default 64 KB of dynamic LDS");

// grad_in[p, ci0 + c] = sum over t, co of Wd[t][ci0 + c][co] gy[p + (t - pad) dil, co], c < 32 NG: k_conv2s at
// stride 1 with a dilation, gy as the input and rows ci0 .. of every tap of Wd [KS^2][cin][cout] as the weights.
template <int NG, int KS>
__global__ __launch_bounds__(kThreads) void k_conv2x_dgrad1(
    const unsigned short* __restrict__ gy, int cout, const unsigned short* __restrict__ wd, int cin, int ci0, int dil,
    unsigned short* __restrict__ out, int H, int W, int ntx, int nty) {
  using A = Act<true>;
  using v8 = typename A::v8;
  constexpr int R = kDgRows, PB = R / 2;
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
  const int SW = kTileX + (KS - 1) * dil;  // staged columns
  const int nchunk = cout >> 5;
  const int rowstride = W * cout;
  const unsigned short* img_in = gy + (int64_t)img * H * W * cout;
  const int gx0 = x0 - PAD * dil;
  const int mc = tid & 3;

  f32x16 acc[PB][NG];
#pragma unroll
  for (int o = 0; o < PB; ++o)
#pragma unroll
    for (int g = 0; g < NG; ++g)
      for (int i = 0; i < 16; ++i) acc[o][g][i] = 0.0f;

  for (int s = 0; s < KS * nchunk; ++s) {  // stage s: dy = s / nchunk, channel chunk cc = s % nchunk
    const int dy = s / nchunk, cc = s - dy * nchunk;
    __syncthreads();  // the previous stage's operand reads are done
    const unsigned short* pl = img_in + cc * 32 + mc * 8;
    for (int i = tid >> 2; i < R * SW; i += kThreads / 4) {
      const int ry = i / SW, sc = i - ry * SW;
      const int gyy = y0 + ry + (dy - PAD) * dil, gx = gx0 + sc;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gyy >= 0 && gyy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const uint4*>(pl + gyy * rowstride + gx * cout);
      *reinterpret_cast<uint4*>(lds_in + i * 64 + swz(mc, sc) * 16) = v;
    }
    for (int i = tid >> 2; i < WROWS; i += kThreads / 4) {
      const int dx = i / (NG * 32), row = i - dx * (NG * 32);
      const unsigned short* wb = wd + ((int64_t)(dy * KS + dx) * cin + ci0 + row) * cout + cc * 32 + mc * 8;
      *reinterpret_cast<uint4*>(lds_w + i * 64 + swz(mc, i) * 16) = *reinterpret_cast<const uint4*>(wb);
    }
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
        const int p = wcol + r + dx * dil;
#pragma unroll
        for (int o = 0; o < PB; ++o)
          xf[o] = *reinterpret_cast<const v8*>(lds_in + ((wrow + o) * SW + p) * 64 + swz(c, p) * 16);
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int o = 0; o < PB; ++o) acc[o][g] = A::mfma(wf[g], xf[o], acc[o][g]);
      }
    }
  }

  const int x = x0 + wcol + r;
  if (x >= W) return;
#pragma unroll
  for (int o = 0; o < PB; ++o) {
    const int y = y0 + wrow + o;
    if (y >= H) break;
    dgrad_store<NG>(acc[o], out, ((int64_t)img * H + y) * W + x, cin, ci0, h);
  }
}

// Stride 2: block = (image, grad_in row py, 64 column pairs from j0); wave (b, half) owns columns 2 j + b,
// j = j0 + 32 half + 0..31.  Output row q and kernel row kh meet at py when py + pad - kh = 2 q, and likewise in
// x, so a stage is (live kh, 32-channel chunk of co): gy's row q, columns j0 .. j0 + 64, and the KS taps
// Wd[KS^2 - 1 - (kh KS + kw)]; a wave multiplies the kw with b + pad - kw even, at column offset (b + pad - kw) / 2.
template <int NG, int KS>
__global__ __launch_bounds__(kThreads) void k_conv2x_dgrad2(
    const unsigned short* __restrict__ gy, int cout, const unsigned short* __restrict__ wd, int cin, int ci0,
    unsigned short* __restrict__ out, int Hin, int Win, int Hout, int Wout, int ntx) {
  using A = Act<true>;
  using v8 = typename A::v8;
  constexpr int PAD = KS == 3 ? 1 : 0;
  constexpr int WROWS = KS * NG * 32;
  constexpr int SW = kTileX + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* lds_w = lds;
  unsigned char* lds_in = lds + WROWS * 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int rest = blockIdx.x;
  const int tx = rest % ntx;
  rest /= ntx;
  const int py = rest % Hin, img = rest / Hin;
  const int j0 = tx * kTileX;
  const int r = lane & 31, h = lane >> 5;
  const int b = wave & 1, jw = (wave >> 1) * 32;
  const int nchunk = cout >> 5;
  const unsigned short* img_g = gy + (int64_t)img * Hout * Wout * cout;
  const int mc = tid & 3;

  f32x16 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g)
    for (int i = 0; i < 16; ++i) acc[g][i] = 0.0f;

  for (int kh = 0; kh < KS; ++kh) {
    const int t = py + PAD - kh;                    // block-uniform: every barrier is reached by all
    if (t < 0 || (t & 1) || (t >> 1) >= Hout) continue;
    const unsigned short* grow = img_g + (t >> 1) * (Wout * cout);
    for (int cc = 0; cc < nchunk; ++cc) {
      __syncthreads();  // the previous stage's operand reads are done
      for (int i = tid >> 2; i < SW; i += kThreads / 4) {
        const int qx = j0 + i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (qx < Wout) v = *reinterpret_cast<const uint4*>(grow + qx * cout + cc * 32 + mc * 8);
        *reinterpret_cast<uint4*>(lds_in + i * 64 + swz(mc, i) * 16) = v;
      }
      for (int i = tid >> 2; i < WROWS; i += kThreads / 4) {
        const int kw = i / (NG * 32), row = i - kw * (NG * 32);
        const int tap = KS * KS - 1 - (kh * KS + kw);
        const unsigned short* wb = wd + ((int64_t)tap * cin + ci0 + row) * cout + cc * 32 + mc * 8;
        *reinterpret_cast<uint4*>(lds_w + i * 64 + swz(mc, i) * 16) = *reinterpret_cast<const uint4*>(wb);
      }
      __syncthreads();
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int u = b + PAD - kw;                 // wave-uniform
        if (u & 1) continue;
        const int p = jw + r + (u >> 1);            // u is 0 or 2: at most column 64 of the stage
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const int c = kb * 2 + h;
          const v8 xf = *reinterpret_cast<const v8*>(lds_in + p * 64 + swz(c, p) * 16);
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const v8 wf = *reinterpret_cast<const v8*>(lds_w + ((kw * NG + g) * 32 + r) * 64 + swz(c, r) * 16);
            acc[g] = A::mfma(wf, xf, acc[g]);
          }
        }
      }
    }
  }

  const int px = 2 * (j0 + jw + r) + b;
  if (px >= Win) return;
  dgrad_store<NG>(acc, out, ((int64_t)img * Hin + py) * Win + px, cin, ci0, h);
}

template <int NG, int KS>
void launch_dg(hipStream_t s, int stride, const void* grad_out, int images, int cout, int hout, int wout,
               const void* weights, int cin, int ci0, int hin, int win, int dil, void* grad_in) {
  if (stride == 1) {
    const int ntx = (win + kTileX - 1) / kTileX, nty = (hin + kDgRows - 1) / kDgRows;
    hipLaunchKernelGGL((k_conv2x_dgrad1<NG, KS>), dim3((unsigned)(ntx * nty * images)), dim3(kThreads),
                       (unsigned)dg1_lds(NG, KS, dil), s, (const unsigned short*)grad_out, cout,
                       (const unsigned short*)weights, cin, ci0, dil, (unsigned short*)grad_in, hin, win, ntx, nty);
  } else {
    const int ntx = ((win + 1) / 2 + kTileX - 1) / kTileX;
    hipLaunchKernelGGL((k_conv2x_dgrad2<NG, KS>), dim3((unsigned)(ntx * hin * images)), dim3(kThreads),
                       (unsigned)dg2_lds(NG, KS), s, (const unsigned short*)grad_out, cout,
                       (const unsigned short*)weights, cin, ci0, (unsigned short*)grad_in, hin, win, hout, wout, ntx);
  }
}

template <int KS>
void launch_dg_ng(int ng, hipStream_t s, int stride, const void* grad_out, int images, int cout, int hout, int wout,
                  const void* weights, int cin, int ci0, int hin, int win, int dil, void* grad_in) {
  switch (ng) {
    case 1: launch_dg<1, KS>(s, stride, grad_out, images, cout, hout, wout, weights, cin, ci0, hin, win, dil, grad_in); break;
    case 2: launch_dg<2, KS>(s, stride, grad_out, images, cout, hout, wout, weights, cin, ci0, hin, win, dil, grad_in); break;
    case 3: launch_dg<3, KS>(s, stride, grad_out, images, cout, hout, wout, weights, cin, ci0, hin, win, dil, grad_in); break;
    default: launch_dg<4, KS>(s, stride, grad_out, images, cout, hout, wout, weights, cin, ci0, hin, win, dil, grad_in); break;
  }
}

// the checks both entry points share; 0 or the error code
int check_layer(int images, int cin, int cout, int hin, int win, int ksize, int stride, int dilation) {
  SFM_REQUIRE(cin_ok(cin), "cin must be a multiple of 32 from 32 to 320");
  SFM_REQUIRE(chan_ok(cout), "cout must be 32, 64, 96 or 128");
  SFM_REQUIRE(ksize == 3 || ksize == 1, "ksize must be 3 or 1");
  SFM_REQUIRE(stride == 1 || stride == 2, "stride must be 1 or 2");
  SFM_REQUIRE(dilation >= 1 && dilation <= kMaxDil, "dilation must be 1..16");
  SFM_REQUIRE(dilation == 1 || (ksize == 3 && stride == 1), "a 1 x 1 or stride 2 conv takes dilation 1 only");
  SFM_REQUIRE(images >= 1 && hin >= 1 && win >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)hin * win * (cin > 128 ? cin : 128) < ((int64_t)1 << 31),
              "conv image too large (32-bit in-image offsets)");
  return SFM_OK;
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_conv2x_wgrad_f16_workspace_bytes(int images, int cin, int cout, int hin, int win, int ksize, int stride) {
  if (images < 1 || hin < 1 || win < 1 || !cin_ok(cin) || !chan_ok(cout) || (ksize != 3 && ksize != 1) ||
      (stride != 1 && stride != 2))
    return 0;
  return xw_ws_bytes(xw_plan(images, cout, hin, win, ksize, stride), cin, cout, ksize);
}

int sfm_conv2x_wgrad_f16(const void* in, const void* grad_out, int images, int cin, int cout, int hin, int win,
                         int ksize, int stride, int dilation, float* grad_weights, void* workspace,
                         size_t workspace_bytes, void* stream) {
  SFM_REQUIRE(in && grad_out && grad_weights, "null pointer argument");
  if (const int rc = check_layer(images, cin, cout, hin, win, ksize, stride, dilation)) return rc;
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)grad_weights & 15) == 0,
              "conv operands must be 16-byte aligned");
  const XwPlan p = xw_plan(images, cout, hin, win, ksize, stride);
  const size_t need = xw_ws_bytes(p, cin, cout, ksize);
  if (!workspace || workspace_bytes < need) {
    set_error("conv2x weight-gradient workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  SFM_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  const size_t in_bytes = (size_t)images * hin * win * cin * 2, go_bytes = (size_t)images * p.hout * p.wout * cout * 2;
  const size_t gw_bytes = (size_t)ksize * ksize * cout * cin * sizeof(float);
  SFM_REQUIRE(!overlap(grad_weights, gw_bytes, in, in_bytes) && !overlap(grad_weights, gw_bytes, grad_out, go_bytes) &&
                  !overlap(grad_weights, gw_bytes, workspace, need) && !overlap(workspace, need, in, in_bytes) &&
                  !overlap(workspace, need, grad_out, go_bytes),
              "conv weight-gradient outputs must not alias its inputs");
  const int64_t slices = (int64_t)ksize * (cin / 32) * (cout / 32 / p.ng);
  SFM_REQUIRE(slices <= 65535, "conv weight-gradient grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv2x_wgrad", s);
  // the context stack's layer set goes through its entry point: the same kernel, under its "conv2_wgrad" scope too
  if (ksize == 3 && stride == 1 && cin <= 128)
    return sfm_conv2_wgrad_f16(in, grad_out, images, cin, cout, hin, win, dilation, grad_weights, workspace,
                               workspace_bytes, stream);
  return launch_conv2_wgrad(s, p, in, grad_out, cin, cout, hin, win, ksize, stride, dilation, workspace, grad_weights);
}

int sfm_conv2x_dgrad_f16(const void* grad_out, int images, int cout, int hout, int wout, const void* weights, int cin,
                         int hin, int win, int ksize, int stride, int dilation, void* grad_in, void* stream) {
  SFM_REQUIRE(grad_out && weights && grad_in, "null pointer argument");
  if (const int rc = check_layer(images, cin, cout, hin, win, ksize, stride, dilation)) return rc;
  SFM_REQUIRE(hout == (hin - 1) / stride + 1 && wout == (win - 1) / stride + 1,
              "grad_in's hin x win is not an input size of grad_out's hout x wout at this stride");
  SFM_REQUIRE(((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)weights & 15) == 0 && ((uintptr_t)grad_in & 15) == 0,
              "conv operands must be 16-byte aligned");
  const size_t go_bytes = (size_t)images * hout * wout * cout * 2, gi_bytes = (size_t)images * hin * win * cin * 2;
  const size_t w_bytes_all = (size_t)ksize * ksize * cin * cout * 2;
  SFM_REQUIRE(!overlap(grad_in, gi_bytes, grad_out, go_bytes) && !overlap(grad_in, gi_bytes, weights, w_bytes_all),
              "conv output must not alias its inputs");
  const int rows = stride == 1 ? kDgRows : 1;
  const int cols = stride == 1 ? win : (win + 1) / 2;
  const int64_t nblk = (int64_t)((cols + kTileX - 1) / kTileX) * ((hin + rows - 1) / rows) * images;
  SFM_REQUIRE(nblk < ((int64_t)1 << 31), "conv grid too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv2x_dgrad", s);
  // the context stack's layer set: its kernel, its bits
  if (ksize == 3 && stride == 1 && cin <= 128)
    return sfm_conv2_dgrad_f16(grad_out, images, cout, hin, win, weights, cin, dilation, nullptr, grad_in, stream);
  for (int ci0 = 0; ci0 < cin; ci0 += 128) {       // at most 128 input channels per launch, into the one tensor
    const int ng = (cin - ci0 < 128 ? cin - ci0 : 128) / 32;
    if (ksize == 3)
      launch_dg_ng<3>(ng, s, stride, grad_out, images, cout, hout, wout, weights, cin, ci0, hin, win, dilation, grad_in);
    else
      launch_dg_ng<1>(ng, s, stride, grad_out, images, cout, hout, wout, weights, cin, ci0, hin, win, dilation, grad_in);
    SFM_LAUNCHED();
  }
  return SFM_OK;
}

}  // extern "C"
