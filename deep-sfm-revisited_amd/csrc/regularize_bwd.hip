// Weight gradient of one 3x3x3 / stride 1 / pad 1 Conv3d layer of PSNet's
// cost regularisation (models/PSNet.py:79-102, applied at 159-165) on the
// gfx950 matrix cores, float16 operands and float32 accumulation: the third
// product of a training step (the forward and the data gradient are both
// sfm_conv3_f16, see sfm_hip.h).
//
//   gW[tap][co][ci] = sum over b, p of gy[b, p, co] x[b, p + tap - 1, ci]
//
// (p + tap - 1 per axis, zero outside the volume), x [B][D][H][W][cin] and gy
// [B][D][H][W][32] channels-last float16, gW [27][32][cin] float32 in
// sfm_conv3_f16's pack layout.
//
// A GEMM per tap, D[32 co][32 ci] = G^T[co][voxels] . X[voxels][ci], whose K
// axis is the voxel axis: the slow axis of both operands in memory.  Both
// tiles are staged in LDS as they lie in memory ([voxel][32 channels], 64-byte
// rows) and both MFMA operands are read with ds_read_b64_tr_b16, the hardware
// transpose read: a 16-lane group reads a block of 4 voxels x 16 channels and
// each lane receives one channel of the four voxels.  A and B are read by the
// same address function (tr_frag, mfma_frag.h), so the k order of the two operands agrees by
// construction.  A tap's shift is a row offset of the X image (64 dx bytes),
// so it costs nothing.  Every lane takes part in every read (EXEC all ones):
// voxels outside the volume are staged as zeros, never masked.
//
// k_conv3_wgrad: a block is 3 waves; wave dx owns the nine taps (dz, dy, dx)
// as nine 32x32 float32 accumulators (144 registers).  A tile is one plane z,
// 4 rows and 64 columns of gy; per dz the 6 x 66 halo of x's plane z + dz - 1
// is staged (a plane outside the volume is skipped).  Per 16-voxel chunk a
// wave reads 4 gy fragments and 6 x fragments for 12 MFMAs.  The grid is a
// fixed number of blocks (sized to the machine, or the conv_wgrad_blocks
// tuning key); block k walks the contiguous tile range [k T / n, (k + 1) T / n),
// z fastest, so consecutive tiles re-read the same x planes from L2, and
// accumulates in registers.  It writes one [27][32][32] partial into the
// caller's workspace -- all of it, zeros included, when its range is empty.
// k_conv3_wgrad_reduce then sums the partials in block order, one thread per
// element: no float atomics anywhere, so the result is reproducible bit for
// bit from run to run.  cin = 64 runs the two 32-channel halves as grid.y.
#include <string>
#include "common.h"
#include "mfma_frag.h"

namespace sfm {
namespace {

constexpr int kWgTileX = 64;                      // gy columns per tile
constexpr int kWgTileY = 4;                       // gy rows per tile
constexpr int kWgHaloX = kWgTileX + 2;            // 66
constexpr int kWgHaloY = kWgTileY + 2;            // 6
constexpr int kWgThreads = 192;                   // 3 waves: dx = 0, 1, 2
constexpr int kWgGyBytes = kWgTileY * kWgTileX * 64;     // 16,384
// the last chunk's reads at dx = 2 end at halo column 48 + 2 + 15 = 65: inside the row
constexpr int kWgXBytes = kWgHaloY * kWgHaloX * 64;      // 25,344
constexpr int kWgPartial = 27 * 32 * 32;          // floats per block and 32-channel half
constexpr int kWgDefaultBlocks = 512;             // 2 per CU on MI355X (256 CUs)

__global__ __launch_bounds__(kWgThreads, 2) void k_conv3_wgrad(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ gy, int cin, int B, int D, int H, int W,
    int ntx, int nty, int64_t ntiles, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_g[kWgGyBytes];
  __shared__ __attribute__((aligned(16))) unsigned char lds_x[kWgXBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63, dx = tid >> 6;
  const int half = blockIdx.y;                    // 32-channel half of cin
  const int nb = gridDim.x;
  const int64_t t0 = ntiles * blockIdx.x / nb, t1 = ntiles * (blockIdx.x + 1) / nb;
  const int64_t plane = (int64_t)H * W;

  f32x16 acc[3][3];                               // [dz][dy]
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 16; ++i) acc[a][c][i] = 0.0f;

  for (int64_t t = t0; t < t1; ++t) {             // block-uniform bounds: every barrier is reached by all
    const int z = (int)(t % D);
    int64_t rest = t / D;
    const int tx = (int)(rest % ntx);
    rest /= ntx;
    const int ty = (int)(rest % nty), b = (int)(rest / nty);
    const int x0 = tx * kWgTileX, y0 = ty * kWgTileY;
    __syncthreads();                              // the previous tile's reads of lds_g are done
    {
      const unsigned short* gp = gy + (((int64_t)b * D + z) * plane) * 32;
      for (int i = tid; i < kWgTileY * kWgTileX * 4; i += kWgThreads) {
        const int c = i & 3, col = (i >> 2) & (kWgTileX - 1), r = i >> 8;
        const int gx = x0 + col, gyy = y0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gx < W && gyy < H) v = *reinterpret_cast<const uint4*>(gp + ((int64_t)gyy * W + gx) * 32 + c * 8);
        *reinterpret_cast<uint4*>(lds_g + (r * kWgTileX + col) * 64 + c * 16) = v;
      }
    }
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
      const int zz = z + dz - 1;
      if (zz < 0 || zz >= D) continue;            // zero padding: no contribution (block-uniform)
      __syncthreads();                            // the previous stage's reads of lds_x are done
      {
        const unsigned short* xp = x + (((int64_t)b * D + zz) * plane) * cin + half * 32;
        for (int i = tid; i < kWgHaloY * kWgHaloX * 4; i += kWgThreads) {
          const int c = i & 3, px = (i >> 2) % kWgHaloX, ry = (i >> 2) / kWgHaloX;
          const int gx = x0 - 1 + px, gyy = y0 - 1 + ry;
          uint4 v = make_uint4(0, 0, 0, 0);
          if (gx >= 0 && gx < W && gyy >= 0 && gyy < H)
            v = *reinterpret_cast<const uint4*>(xp + ((int64_t)gyy * W + gx) * cin + c * 8);
          *reinterpret_cast<uint4*>(lds_x + (ry * kWgHaloX + px) * 64 + c * 16) = v;
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < kWgTileX / 16; ++c) {
        f16x8 gf[kWgTileY];
#pragma unroll
        for (int r = 0; r < kWgTileY; ++r) gf[r] = tr_frag(lds_g, r * kWgTileX + c * 16, lane);
#pragma unroll
        for (int hr = 0; hr < kWgHaloY; ++hr) {   // halo row hr feeds output row hr - dy
          const f16x8 xf = tr_frag(lds_x, hr * kWgHaloX + c * 16 + dx, lane);
#pragma unroll
          for (int dy = 0; dy < 3; ++dy) {
            const int r = hr - dy;
            if (r >= 0 && r < kWgTileY)
              acc[dz][dy] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gf[r], xf, acc[dz][dy], 0, 0, 0);
          }
        }
      }
    }
  }

  // D[row = co][col = ci]: lane holds ci = lane % 32 and co = 8 q + 4 (lane / 32) + j in acc[4 q + j]
  float* out = partial + ((int64_t)half * nb + blockIdx.x) * kWgPartial;
  const int ci = lane & 31, h = lane >> 5;
#pragma unroll
  for (int dz = 0; dz < 3; ++dz)
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int tap = (dz * 3 + dy) * 3 + dx;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(tap * 32 + 8 * q + 4 * h + j) * 32 + ci] = acc[dz][dy][4 * q + j];
    }
}

// gW[tap][co][half * 32 + ci] = the partials of blocks 0, 1, ... nb - 1, added in that order
__global__ __launch_bounds__(256) void k_conv3_wgrad_reduce(const float* __restrict__ partial, int nb, int cin,
                                                            float* __restrict__ gw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int half = blockIdx.y;
  if (e >= kWgPartial) return;
  const float* p = partial + (int64_t)half * nb * kWgPartial + e;
  float s = 0.0f;
  for (int k = 0; k < nb; ++k) s = s + p[(int64_t)k * kWgPartial];
  gw[(e >> 5) * cin + half * 32 + (e & 31)] = s;
}

struct WgradPlan {
  int ntx, nty, blocks;
  int64_t ntiles;
};

WgradPlan wgrad_plan(int batch, int depth, int h, int w) {
  WgradPlan p;
  p.ntx = (w + kWgTileX - 1) / kWgTileX;
  p.nty = (h + kWgTileY - 1) / kWgTileY;
  p.ntiles = (int64_t)p.ntx * p.nty * depth * batch;
  // conv_wgrad_blocks: a given number of accumulating blocks (launch shape only; more blocks than tiles is
  // allowed: the spare ones write zero partials)
  const int forced = tuning().conv_wgrad_blocks;
  p.blocks = forced > 0 ? forced : (int)(p.ntiles < kWgDefaultBlocks ? p.ntiles : kWgDefaultBlocks);
  return p;
}

size_t wgrad_ws_bytes(const WgradPlan& p, int cin) {
  return (size_t)(cin / 32) * p.blocks * kWgPartial * sizeof(float);
}

}  // namespace
}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_conv3_wgrad_f16_workspace_bytes(int batch, int cin, int depth, int h, int w) {
  if (batch < 1 || depth < 1 || h < 1 || w < 1 || (cin != 32 && cin != 64)) return 0;
  return wgrad_ws_bytes(wgrad_plan(batch, depth, h, w), cin);
}

int sfm_conv3_wgrad_f16(const void* in, const void* grad_out, int batch, int cin, int cout, int depth, int h, int w,
                        float* grad_weights, void* workspace, size_t workspace_bytes, void* stream) {
  SFM_REQUIRE(in && grad_out && grad_weights, "null pointer argument");
  SFM_REQUIRE(cin == 32 || cin == 64, "cin must be 32 or 64");
  SFM_REQUIRE(cout == 32, "cout must be 32 (a cout 1 layer passes its gradient zero-padded to 32 channels)");
  SFM_REQUIRE(batch >= 1 && depth >= 1 && h >= 1 && w >= 1, "invalid conv shape");
  SFM_REQUIRE((int64_t)h * w * cin < ((int64_t)1 << 31), "conv plane too large (32-bit in-plane offsets)");
  SFM_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)grad_weights & 15) == 0,
              "conv operands must be 16-byte aligned");
  const WgradPlan p = wgrad_plan(batch, depth, h, w);
  const size_t need = wgrad_ws_bytes(p, cin);
  if (!workspace || workspace_bytes < need) {
    set_error("conv3 weight-gradient workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  SFM_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  const size_t vox = (size_t)batch * depth * h * w;
  const size_t gw_bytes = (size_t)27 * 32 * cin * sizeof(float);
  SFM_REQUIRE(!overlap(grad_weights, gw_bytes, in, vox * cin * 2) && !overlap(grad_weights, gw_bytes, grad_out, vox * 64) &&
                  !overlap(grad_weights, gw_bytes, workspace, need) && !overlap(workspace, need, in, vox * cin * 2) &&
                  !overlap(workspace, need, grad_out, vox * 64),
              "conv weight-gradient outputs must not alias its inputs");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("conv3_wgrad", s);
  hipLaunchKernelGGL(k_conv3_wgrad, dim3((unsigned)p.blocks, (unsigned)(cin / 32)), dim3(kWgThreads), 0, s,
                     (const unsigned short*)in, (const unsigned short*)grad_out, cin, batch, depth, h, w, p.ntx, p.nty,
                     p.ntiles, (float*)workspace);
  SFM_LAUNCHED();
  hipLaunchKernelGGL(k_conv3_wgrad_reduce, dim3((kWgPartial + 255) / 256, (unsigned)(cin / 32)), dim3(256), 0, s,
                     (const float*)workspace, p.blocks, cin, grad_weights);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
