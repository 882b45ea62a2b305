// The backward of PSNet's per-plane context stack (models/PSNet.py:17-26
// convtext, 64-71 the seven dilated stages, applied per plane at 175-190) in
// float16 on the gfx950 matrix cores: the three products a training step needs
// beside the forward (context.hip).
//
// k_conv2_wgrad: the weight gradient of one 3x3 / stride 1 / pad = dilation
// stage,
//
//   gW[tap][co][ci] = sum over img, y, x of gy[img, y, x, co] x[img, y + (kh-1) dil, x + (kw-1) dil, ci]
//
// a GEMM per tap whose K axis is the pixel axis, the slow axis of both operands.
// Both tiles are staged in LDS as they lie in memory ([pixel][32 channels],
// 64-byte rows per 32-channel chunk) and both MFMA operands are read with
// ds_read_b64_tr_b16 through one address function (tr_frag, as in
// regularize_bwd.hip), so a tap's column shift kw dil is a row offset of the x
// image.  Pixels outside the image are staged as zeros; EXEC is all ones at
// every read.
//
// The full result is up to 144 32x32 accumulators, so the grid splits it:
// blockIdx.y = (kernel row dy, 32-channel chunk of ci, set of NG co groups),
// NG = 1, 2, 3 for cout_pad 32, 64 | 128, 96.  A wave holds the three kw taps
// of its NG groups: 3 NG <= 9 accumulators.  A tile is 4 rows x 64 columns of
// gy; per tile the block stages gy's NG chunks and, as k_conv2 does per kernel
// row, x's rows y0 + (dy-1) dil + 0..3, columns x0 - dil .. x0 + 63 + dil (a
// stage whose rows are all outside the image is skipped).  Wave r owns tile row
// r: per 16-pixel chunk it reads NG gy fragments and 3 x fragments for 3 NG
// MFMAs (2 (3 + NG) / (3 NG) transposing reads per MFMA: 2.7, 1.7, 1.3).  The
// grid is a fixed number of blocks; block k walks the contiguous tile range
// [k T / n, (k + 1) T / n), accumulates in registers, adds its four waves'
// accumulators through LDS in wave order and writes one partial -- zeros when
// its range is empty.  k_conv2_wgrad_reduce adds the partials in block order:
// no float atomics, the same bits from run to run.
//
// The data gradient is k_conv2 itself (conv2_tile.h) on flipped weights with
// the MASK epilogue; k_context_unpack_grad carries the first stage's gradient
// back to PSNet's tensors.  The full-resolution refinement stack dep_convs
// (PSNet.py:218-221) runs the same two products; k_dep_unpack_grad is the
// backward of its pack's bilinear upsample into the features.
#include <string>
#include "conv2_tile.h"

namespace sfm {
namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kW2TileX = 64;            // gy columns per tile
constexpr int kW2Rows = 4;              // gy rows per tile: one per wave
constexpr int kW2Threads = 256;
constexpr int kW2DefaultBlocks = 512;   // 2 per CU on MI355X (256 CUs)
constexpr int w2_g_bytes(int ng) { return ng * kW2Rows * kW2TileX * 64; }
constexpr int w2_x_bytes(int dil) { return kW2Rows * (kW2TileX + 2 * dil) * 64; }
constexpr int w2_partial(int ng) { return 3 * ng * 32 * 32; }   // floats per block and slice
constexpr int w2_ng(int cout_pad) { return cout_pad == 96 ? 3 : cout_pad == 32 ? 1 : 2; }
static_assert(w2_g_bytes(3) + w2_x_bytes(kMaxDil) <= 80 * 1024, "two blocks per CU (160 KB of LDS)");
static_assert(w2_partial(3) * 4 <= w2_g_bytes(3) && w2_partial(1) * 4 <= w2_g_bytes(1),
              "the block's reduction image fits the gy stage");

// One 32x32x16 MFMA operand from a [pixel][32 channels] f16 image (64-byte
// rows): rows = 32 channels, k = 16 consecutive pixels from `pixel0`
// (regularize_bwd.hip's tr_frag: lane l gets channel l % 32 of pixels pixel0 +
// 8 (l / 32) + 0..7).
__device__ __forceinline__ f16x8 tr_frag(const unsigned char* img, int pixel0, int lane) {
  const int v = pixel0 + 8 * (lane >> 5) + ((lane >> 2) & 3);
  const unsigned char* a = img + v * 64 + 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
  typedef short i16x4 __attribute__((vector_size(8)));
  typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
  const f16x4 lo = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)a));
  const f16x4 hi = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(a + 4 * 64)));
  return f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int NG>
__global__ __launch_bounds__(kW2Threads, 2) void k_conv2_wgrad(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ gy, int cin, int cop, int dil, int H, int W,
    int ntx, int nty, int64_t ntiles, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* lds_g = lds;
  unsigned char* lds_x = lds + w2_g_bytes(NG);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int nci = cin >> 5, nset = (cop >> 5) / NG;
  int sl = blockIdx.y;                            // slice = (dy * nci + cc) * nset + set
  const int set = sl % nset;
  sl /= nset;
  const int cc = sl % nci, dy = sl / nci;
  const int nb = gridDim.x;
  const int64_t t0 = ntiles * blockIdx.x / nb, t1 = ntiles * (blockIdx.x + 1) / nb;
  const int SW = kW2TileX + 2 * dil;              // staged x columns
  const int64_t plane = (int64_t)H * W;

  f32x16 acc[3][NG];                              // [kw][co group]
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int g = 0; g < NG; ++g)
      for (int i = 0; i < 16; ++i) acc[a][g][i] = 0.0f;

  for (int64_t t = t0; t < t1; ++t) {             // block-uniform bounds: every barrier is reached by all
    const int tx = (int)(t % ntx);
    int64_t rest = t / ntx;
    const int ty = (int)(rest % nty), img = (int)(rest / nty);
    const int x0 = tx * kW2TileX, y0 = ty * kW2Rows;
    const int iy0 = y0 + (dy - 1) * dil;          // x's first staged row
    if (iy0 >= H || iy0 + kW2Rows <= 0) continue; // zero padding: no contribution (block-uniform)
    __syncthreads();                              // the previous tile's reads are done
    {
      const unsigned short* gp = gy + (int64_t)img * plane * cop + set * NG * 32;
      for (int i = tid; i < NG * kW2Rows * kW2TileX * 4; i += kW2Threads) {
        const int c = i & 3, col = (i >> 2) & (kW2TileX - 1), r = (i >> 8) & (kW2Rows - 1), grp = i >> 10;
        const int gx = x0 + col, gyy = y0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gx < W && gyy < H) v = *reinterpret_cast<const uint4*>(gp + ((int64_t)gyy * W + gx) * cop + grp * 32 + c * 8);
        *reinterpret_cast<uint4*>(lds_g + ((grp * kW2Rows + r) * kW2TileX + col) * 64 + c * 16) = v;
      }
      const unsigned short* xp = x + (int64_t)img * plane * cin + cc * 32;
      for (int i = tid; i < kW2Rows * SW * 4; i += kW2Threads) {
        const int c = i & 3, p = i >> 2;
        const int ry = p / SW, px = p - ry * SW;
        const int gx = x0 - dil + px, gyy = iy0 + ry;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gx >= 0 && gx < W && gyy >= 0 && gyy < H)
          v = *reinterpret_cast<const uint4*>(xp + ((int64_t)gyy * W + gx) * cin + c * 8);
        *reinterpret_cast<uint4*>(lds_x + p * 64 + c * 16) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kW2TileX / 16; ++c) {
      f16x8 gf[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) gf[g] = tr_frag(lds_g + g * (kW2Rows * kW2TileX * 64), wave * kW2TileX + c * 16, lane);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {            // the last chunk at kw = 2 ends at column 48 + 2 dil + 15 < SW
        const f16x8 xf = tr_frag(lds_x, wave * SW + c * 16 + kw * dil, lane);
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
  for (int wv = 0; wv < kW2Threads / 64; ++wv) {
    __syncthreads();                              // the operand reads, then the waves before this one, are done
    if (wave == wv) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
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
  float* out = partial + ((int64_t)blockIdx.y * nb + blockIdx.x) * w2_partial(NG);
  for (int i = tid; i < w2_partial(NG); i += kW2Threads) out[i] = red[i];
}

// gW[tap][co][ci] = the partials of blocks 0, 1, ... nb - 1 of the element's slice, added in that order
__global__ __launch_bounds__(256) void k_conv2_wgrad_reduce(const float* __restrict__ partial, int nb, int cin, int cop,
                                                            int ng, float* __restrict__ gw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 9 * cop * cin) return;
  const int ci = e % cin, co = (e / cin) % cop, tap = e / (cin * cop);
  const int dy = tap / 3, kw = tap - dy * 3;
  const int cog = co >> 5, set = cog / ng, grp = cog - set * ng;
  const int slice = (dy * (cin >> 5) + (ci >> 5)) * ((cop >> 5) / ng) + set;
  const int ps = w2_partial(ng);
  const float* p = partial + (int64_t)slice * nb * ps + ((kw * ng + grp) * 32 + (co & 31)) * 32 + (ci & 31);
  float s = 0.0f;
  for (int k = 0; k < nb; ++k) s = s + p[(int64_t)k * ps];
  gw[e] = s;
}

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

struct Wgrad2Plan {
  int ntx, nty, blocks, ng;
  int64_t ntiles;
};

Wgrad2Plan wgrad2_plan(int images, int cout_pad, int h, int w) {
  Wgrad2Plan p;
  p.ntx = (w + kW2TileX - 1) / kW2TileX;
  p.nty = (h + kW2Rows - 1) / kW2Rows;
  p.ntiles = (int64_t)p.ntx * p.nty * images;
  p.ng = w2_ng(cout_pad);
  // conv2_wgrad_blocks: a given number of accumulating blocks (launch shape only; more blocks than tiles is
  // allowed: the spare ones write zero partials)
  const int forced = tuning().conv2_wgrad_blocks;
  p.blocks = forced > 0 ? forced : (int)(p.ntiles < kW2DefaultBlocks ? p.ntiles : kW2DefaultBlocks);
  return p;
}

size_t wgrad2_ws_bytes(const Wgrad2Plan& p, int cin, int cout_pad) {
  return (size_t)p.blocks * 9 * cout_pad * cin * sizeof(float);
}

bool chan_ok(int c) { return c == 32 || c == 64 || c == 96 || c == 128; }

bool overlap(const void* a, size_t na, const void* b, size_t nbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nbytes && b0 < a0 + na;
}

template <int NG>
int launch_wgrad2(hipStream_t s, const Wgrad2Plan& p, const void* in, const void* grad_out, int cin, int cop, int dil,
                  int h, int w, void* workspace) {
  const unsigned lds = (unsigned)(w2_g_bytes(NG) + w2_x_bytes(dil));
  // > 64 KB of dynamic LDS must be opted into; set on every such launch (cheap, and correct for whichever
  // device is current and from any host thread, as conv3_lp does)
  if (lds > 64 * 1024)
    SFM_HIP(hipFuncSetAttribute((const void*)k_conv2_wgrad<NG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                w2_g_bytes(NG) + w2_x_bytes(kMaxDil)));
  const unsigned slices = 3u * (unsigned)(cin / 32) * (unsigned)(cop / 32 / NG);
  hipLaunchKernelGGL(k_conv2_wgrad<NG>, dim3((unsigned)p.blocks, slices), dim3(kW2Threads), lds, s,
                     (const unsigned short*)in, (const unsigned short*)grad_out, cin, cop, dil, h, w, p.ntx, p.nty,
                     p.ntiles, (float*)workspace);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_conv2_wgrad_f16_workspace_bytes(int images, int cin, int cout_pad, int h, int w) {
  if (images < 1 || h < 1 || w < 1 || !chan_ok(cin) || !chan_ok(cout_pad)) return 0;
  return wgrad2_ws_bytes(wgrad2_plan(images, cout_pad, h, w), cin, cout_pad);
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
  const Wgrad2Plan p = wgrad2_plan(images, cout_pad, h, w);
  const size_t need = wgrad2_ws_bytes(p, cin, cout_pad);
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
  int rc;
  switch (p.ng) {
    case 1: rc = launch_wgrad2<1>(s, p, in, grad_out, cin, cout_pad, dilation, h, w, workspace); break;
    case 2: rc = launch_wgrad2<2>(s, p, in, grad_out, cin, cout_pad, dilation, h, w, workspace); break;
    default: rc = launch_wgrad2<3>(s, p, in, grad_out, cin, cout_pad, dilation, h, w, workspace); break;
  }
  if (rc != SFM_OK) return rc;
  hipLaunchKernelGGL(k_conv2_wgrad_reduce, dim3((unsigned)((9 * cout_pad * cin + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, p.blocks, cin, cout_pad, p.ng, grad_weights);
  SFM_LAUNCHED();
  return SFM_OK;
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
