// The weight gradient of one Conv2d in float16 on the gfx950 matrix cores, for
// PSNet's context stacks (sfm_conv2_wgrad_f16, context_bwd.hip) and its feature
// CNN (sfm_conv2x_wgrad_f16, feature_bwd.hip): 3 x 3 (pad = dilation) or 1 x 1,
// stride 1 or 2, 32..320 input channels,
//
//   gW[tap][co][ci] = sum over img, y, x of gy[img, y, x, co] in[img, y S + (kh - pad) dil, x S + (kw - pad) dil, ci]
//
// k_conv2_wgrad<NG, KS, STRIDE>: a GEMM per tap whose K axis is the pixel axis,
// the slow axis of both operands.  Both tiles are staged in LDS as they lie in
// memory ([pixel][32 channels], 64-byte rows per 32-channel chunk) and both
// MFMA operands are read with ds_read_b64_tr_b16 through one address function
// (tr_frag, mfma_frag.h), so a tap's column shift is a row offset of the x
// image.  Pixels outside the image are staged as zeros; EXEC is all ones at
// every read.
//
// The full result is up to 144 32x32 accumulators, so the grid splits it:
// blockIdx.y = (kernel row dy, 32-channel chunk of ci, set of NG co groups).  A
// wave holds the KS kw taps of its NG groups: at 3 x 3 NG = 1, 2, 3 for cout 32,
// 64 | 128, 96 (3 NG <= 9 accumulators), at 1 x 1 every group.  A tile is 4 rows
// x 64 columns of gy; per tile the block stages gy's NG chunks and, as k_conv2
// does per kernel row, x's rows (y0 + 0..3) S + (dy - pad) dil (a stage whose
// rows are all outside the image is skipped).  Wave r owns tile row r: per
// 16-pixel chunk it reads NG gy fragments and KS x fragments for KS NG MFMAs (at
// 3 x 3 2 (3 + NG) / (3 NG) transposing reads per MFMA: 2.7, 1.7, 1.3).  The
// grid is a fixed number of blocks; block k walks the contiguous tile range
// [k T / n, (k + 1) T / n), accumulates in registers, adds its four waves'
// accumulators through LDS in wave order and writes one partial -- zeros when
// its range is empty.  k_conv2_wgrad_reduce adds the partials in block order:
// no float atomics, the same bits from run to run.
//
// The x stage.  At stride 1 it is columns x0 - pad dil .. x0 + 63 + pad dil and
// tap kw reads at row offset kw dil.  At stride 2 consecutive gy pixels read x
// pixels two apart, which tr_frag's 16-consecutive-pixel K axis cannot do, so a
// staged row holds x's columns split by parity: positions 0..64 the odd
// columns 2 (x0 + p) - 1, positions 65..128 the even columns 2 (x0 + p - 65).
// Tap kw = 0 (column 2 x - 1) then reads the odd image at x - x0, kw = 2
// (column 2 x + 1) the odd image at x - x0 + 1 and kw = 1 (column 2 x) the
// even image at x - x0: three reads at consecutive positions.  The 1 x 1 /
// stride 2 stage holds the even columns alone.
#include "conv2_wgrad.h"
#include "conv2_tile.h"

namespace sfm {
namespace {

constexpr int kXwTileX = 64;            // gy columns per tile
constexpr int kXwRows = 4;              // gy rows per tile: one per wave
constexpr int kXwThreads = 256;
constexpr int kXwDefaultBlocks = 512;   // 2 per CU on MI355X (256 CUs)
constexpr int kXwOdd = kXwTileX + 1;    // stride 2, 3 x 3: staged odd columns; the even ones follow
constexpr int xw_g_bytes(int ng) { return ng * kXwRows * kXwTileX * 64; }
constexpr int xw_sw(int ks, int stride, int dil) {
  return stride == 2 ? (ks == 3 ? kXwOdd + kXwTileX : kXwTileX) : kXwTileX + (ks - 1) * dil;
}
constexpr int xw_x_bytes(int ks, int stride, int dil) { return kXwRows * xw_sw(ks, stride, dil) * 64; }
constexpr int xw_partial(int ks, int ng) { return ks * ng * 32 * 32; }   // floats per block and slice
// co groups per wave: all of them at 1 x 1 (one tap); 1, 2, 3 at 3 x 3 -- but 1 for 96 channels at stride 2, whose
// x stage is 129 columns wide
constexpr int xw_ng(int cout, int ks, int stride) {
  return ks == 1 ? cout / 32 : cout == 32 ? 1 : cout == 96 ? (stride == 2 ? 1 : 3) : 2;
}
constexpr int kXwMaxLds = 80 * 1024;
static_assert(xw_g_bytes(3) + xw_x_bytes(3, 1, kMaxDil) <= kXwMaxLds && xw_g_bytes(2) + xw_x_bytes(3, 2, 1) <= kXwMaxLds &&
                  xw_g_bytes(4) + xw_x_bytes(1, 2, 1) <= kXwMaxLds,
              "two blocks per CU (160 KB of LDS)");
static_assert(xw_partial(3, 3) * 4 <= xw_g_bytes(3) && xw_partial(3, 1) * 4 <= xw_g_bytes(1) &&
                  xw_partial(1, 4) * 4 <= xw_g_bytes(4),
              "the block's reduction image fits the gy stage");

template <int NG, int KS, int STRIDE>
__global__ __launch_bounds__(kXwThreads, 2) void k_conv2_wgrad(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ gy, int cin, int cop, int dil, int Hin,
    int Win, int Hout, int Wout, int ntx, int nty, int64_t ntiles, float* __restrict__ partial) {
  constexpr int PAD = KS == 3 ? 1 : 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* lds_g = lds;
  unsigned char* lds_x = lds + xw_g_bytes(NG);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int nci = cin >> 5, nset = (cop >> 5) / NG;
  int sl = blockIdx.y;                            // slice = (dy * nci + cc) * nset + set
  const int set = sl % nset;
  sl /= nset;
  const int cc = sl % nci, dy = sl / nci;
  const int nb = gridDim.x;
  const int64_t t0 = ntiles * blockIdx.x / nb, t1 = ntiles * (blockIdx.x + 1) / nb;
  const int SW = xw_sw(KS, STRIDE, dil);          // staged x positions per row
  const int64_t plane_in = (int64_t)Hin * Win, plane_out = (int64_t)Hout * Wout;

  f32x16 acc[KS][NG];                             // [kw][co group]
#pragma unroll
  for (int a = 0; a < KS; ++a)
#pragma unroll
    for (int g = 0; g < NG; ++g)
      for (int i = 0; i < 16; ++i) acc[a][g][i] = 0.0f;

  for (int64_t t = t0; t < t1; ++t) {             // block-uniform bounds: every barrier is reached by all
    const int tx = (int)(t % ntx);
    int64_t rest = t / ntx;
    const int ty = (int)(rest % nty), img = (int)(rest / nty);
    const int x0 = tx * kXwTileX, y0 = ty * kXwRows;
    const int iy0 = y0 * STRIDE + (dy - PAD) * dil;   // x's first staged row; row r is iy0 + r STRIDE
    if (iy0 >= Hin || iy0 + (kXwRows - 1) * STRIDE < 0) continue;   // zero padding: no contribution (block-uniform)
    __syncthreads();                              // the previous tile's reads are done
    {
      const unsigned short* gp = gy + (int64_t)img * plane_out * cop + set * NG * 32;
      for (int i = tid; i < NG * kXwRows * kXwTileX * 4; i += kXwThreads) {
        const int c = i & 3, col = (i >> 2) & (kXwTileX - 1), r = (i >> 8) & (kXwRows - 1), grp = i >> 10;
        const int gx = x0 + col, gyy = y0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gx < Wout && gyy < Hout)
          v = *reinterpret_cast<const uint4*>(gp + ((int64_t)gyy * Wout + gx) * cop + grp * 32 + c * 8);
        *reinterpret_cast<uint4*>(lds_g + ((grp * kXwRows + r) * kXwTileX + col) * 64 + c * 16) = v;
      }
      const unsigned short* xp = x + (int64_t)img * plane_in * cin + cc * 32;
      for (int i = tid; i < kXwRows * SW * 4; i += kXwThreads) {
        const int c = i & 3, p = i >> 2;
        const int ry = p / SW, px = p - ry * SW;
        int gx;
        if (STRIDE == 1) gx = x0 - PAD * dil + px;
        else if (KS == 3) gx = px < kXwOdd ? 2 * (x0 + px) - 1 : 2 * (x0 + px - kXwOdd);
        else gx = 2 * (x0 + px);
        const int gyy = iy0 + ry * STRIDE;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gx >= 0 && gx < Win && gyy >= 0 && gyy < Hin)
          v = *reinterpret_cast<const uint4*>(xp + ((int64_t)gyy * Win + gx) * cin + c * 8);
        *reinterpret_cast<uint4*>(lds_x + p * 64 + c * 16) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kXwTileX / 16; ++c) {
      f16x8 gf[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) gf[g] = tr_frag(lds_g + g * (kXwRows * kXwTileX * 64), wave * kXwTileX + c * 16, lane);
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        // stride 1: the last chunk at kw = 2 ends at column 48 + 2 dil + 15 < SW; stride 2: the odd image at 0 or 1
        // (ends at 64 < 65), the even image from 65 (ends at 128 < SW)
        const int off = STRIDE == 1 ? kw * dil : KS == 1 ? 0 : kw == 1 ? kXwOdd : kw >> 1;
        const f16x8 xf = tr_frag(lds_x, wave * SW + c * 16 + off, lane);
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[kw][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gf[g], xf, acc[kw][g], 0, 0, 0);
      }
    }
  }

  // The four waves' accumulators added in wave order through LDS, then one partial per block.
  // D[row = co][col = ci]: the lane holds ci = lane % 32 and co = 8 q + 4 (lane / 32) + j in acc[4 q + j].
  float* red = reinterpret_cast<float*>(lds);     // [kw][group][32 co][32 ci]
  const int ci = lane & 31, h = lane >> 5;
#pragma unroll
  for (int wv = 0; wv < kXwThreads / 64; ++wv) {
    __syncthreads();                              // the operand reads, then the waves before this one, are done
    if (wave == wv) {
#pragma unroll
      for (int kw = 0; kw < KS; ++kw)
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float* e = red + ((kw * NG + g) * 32 + 8 * q + 4 * h + j) * 32 + ci;
              *e = wv == 0 ? acc[kw][g][4 * q + j] : *e + acc[kw][g][4 * q + j];
            }
    }
  }
  __syncthreads();
  float* out = partial + ((int64_t)blockIdx.y * nb + blockIdx.x) * xw_partial(KS, NG);
  for (int i = tid; i < xw_partial(KS, NG); i += kXwThreads) out[i] = red[i];
}

// gW[tap][co][ci] = the partials of blocks 0, 1, ... nb - 1 of the element's slice, added in that order
__global__ __launch_bounds__(256) void k_conv2_wgrad_reduce(const float* __restrict__ partial, int nb, int cin, int cop,
                                                            int ks, int ng, float* __restrict__ gw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= ks * ks * cop * cin) return;
  const int ci = e % cin, co = (e / cin) % cop, tap = e / (cin * cop);
  const int dy = tap / ks, kw = tap - dy * ks;
  const int cog = co >> 5, set = cog / ng, grp = cog - set * ng;
  const int slice = (dy * (cin >> 5) + (ci >> 5)) * ((cop >> 5) / ng) + set;
  const int ps = xw_partial(ks, ng);
  const float* p = partial + (int64_t)slice * nb * ps + ((kw * ng + grp) * 32 + (co & 31)) * 32 + (ci & 31);
  float s = 0.0f;
  for (int k = 0; k < nb; ++k) s = s + p[(int64_t)k * ps];
  gw[e] = s;
}

template <int NG, int KS, int STRIDE>
int launch_xw(hipStream_t s, const XwPlan& p, const void* in, const void* grad_out, int cin, int cout, int dil, int hin,
              int win, void* workspace) {
  const unsigned lds = (unsigned)(xw_g_bytes(NG) + xw_x_bytes(KS, STRIDE, dil));
  // > 64 KB of dynamic LDS must be opted into; set on every such launch (cheap, and correct for whichever
  // device is current and from any host thread, as conv3_lp does)
  if (lds > 64 * 1024)
    SFM_HIP(hipFuncSetAttribute((const void*)k_conv2_wgrad<NG, KS, STRIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                kXwMaxLds));
  const unsigned slices = (unsigned)KS * (unsigned)(cin / 32) * (unsigned)(cout / 32 / NG);
  hipLaunchKernelGGL((k_conv2_wgrad<NG, KS, STRIDE>), dim3((unsigned)p.blocks, slices), dim3(kXwThreads), lds, s,
                     (const unsigned short*)in, (const unsigned short*)grad_out, cin, cout, dil, hin, win, p.hout,
                     p.wout, p.ntx, p.nty, p.ntiles, (float*)workspace);
  SFM_LAUNCHED();
  return SFM_OK;
}

template <int KS, int STRIDE>
int launch_xw_ng(int ng, hipStream_t s, const XwPlan& p, const void* in, const void* grad_out, int cin, int cout,
                 int dil, int hin, int win, void* workspace) {
  switch (ng) {
    case 1: return launch_xw<1, KS, STRIDE>(s, p, in, grad_out, cin, cout, dil, hin, win, workspace);
    case 2: return launch_xw<2, KS, STRIDE>(s, p, in, grad_out, cin, cout, dil, hin, win, workspace);
    case 3: return launch_xw<3, KS, STRIDE>(s, p, in, grad_out, cin, cout, dil, hin, win, workspace);
    default:
      if constexpr (KS == 1) return launch_xw<4, KS, STRIDE>(s, p, in, grad_out, cin, cout, dil, hin, win, workspace);
      set_error("conv weight-gradient: no kernel for this channel grouping");
      return SFM_ERR_ARG;
  }
}

}  // namespace

XwPlan xw_plan(int images, int cout, int hin, int win, int ksize, int stride) {
  XwPlan p;
  p.hout = (hin - 1) / stride + 1;
  p.wout = (win - 1) / stride + 1;
  p.ntx = (p.wout + kXwTileX - 1) / kXwTileX;
  p.nty = (p.hout + kXwRows - 1) / kXwRows;
  p.ntiles = (int64_t)p.ntx * p.nty * images;
  p.ng = xw_ng(cout, ksize, stride);
  // conv2_wgrad_blocks: a given number of accumulating blocks (launch shape only; more blocks than tiles is
  // allowed: the spare ones write zero partials)
  const int forced = tuning().conv2_wgrad_blocks;
  p.blocks = forced > 0 ? forced : (int)(p.ntiles < kXwDefaultBlocks ? p.ntiles : kXwDefaultBlocks);
  return p;
}

size_t xw_ws_bytes(const XwPlan& p, int cin, int cout, int ksize) {
  return (size_t)p.blocks * ksize * ksize * cout * cin * sizeof(float);
}

int launch_conv2_wgrad(hipStream_t s, const XwPlan& p, const void* in, const void* grad_out, int cin, int cout,
                       int hin, int win, int ksize, int stride, int dil, void* workspace, float* grad_weights) {
  int rc;
  if (ksize == 3 && stride == 1) rc = launch_xw_ng<3, 1>(p.ng, s, p, in, grad_out, cin, cout, dil, hin, win, workspace);
  else if (ksize == 3) rc = launch_xw_ng<3, 2>(p.ng, s, p, in, grad_out, cin, cout, 1, hin, win, workspace);
  else if (stride == 2) rc = launch_xw_ng<1, 2>(p.ng, s, p, in, grad_out, cin, cout, 1, hin, win, workspace);
  else rc = launch_xw_ng<1, 1>(p.ng, s, p, in, grad_out, cin, cout, 1, hin, win, workspace);
  if (rc != SFM_OK) return rc;
  hipLaunchKernelGGL(k_conv2_wgrad_reduce, dim3((unsigned)((ksize * ksize * cout * cin + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, p.blocks, cin, cout, ksize, p.ng, grad_weights);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace sfm
