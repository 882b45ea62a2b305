// Backward of the plane sweep and of inverse_warp into the features (gfx950).
//
// The reference back-propagates through grid_sample into the target features
// (models/PSNet.py:155, models/inverse_warp.py:151).  With g the gradient of
// the planar float32 volume, d_i the forward's plane depths and off_k, wt_k
// the four taps make_taps gives at the position sample_pos gives (warp.h):
//
//   grad_tgt[b, c, t] = sum_i sum_p sum_{k<4} [off_k(b,i,p) == t] wt_k(b,i,p) g[b, C + c, i, p]
//   grad_ref[b, c, p] = sum_i g[b, c, i, p]
//
// Positions and weights are warp.h's own (load_proj, sample_pos_nr, make_taps,
// plane_depth): the backward is the exact transpose of the forward because both
// see the same float32 bits.  A pixel the forward zero-samples contributes
// nothing; a tap of weight 0 (an invalid tap included) adds nothing.
//
// k_sweep_bwd.  A workgroup owns (pair, group of up to 8 channels, band of
// reference rows, chunk of planes) and sums into a float32 LDS window of
// `wr` whole target rows per channel: within a plane neighbouring pixels hit
// neighbouring taps, across planes the taps slide along the epipolar line, so
// what shares a destination is summed on chip (LDS float adds) and leaves as
// one row-contiguous atomicAdd per window element that is not zero: 256-byte
// wave instructions spread over the window's rows.  The window's first row is
// placed where the band's centre pixel samples on the chunk's middle plane.
// A tap outside the window goes straight to a global atomicAdd: under a large
// rotation that is most of them, slower and still correct.  A row too long
// for any window (wr = 0) takes that path for every tap ("k_sweep_bwd+global").
//
// sfm_inverse_warp_backward is the same kernel with a per-pixel depth map and
// one "plane".
//
// Reproducibility: grad_tgt is accumulated with float atomics, whose order of
// arrival varies, so it may differ in its last bits from run to run (as
// torch's grid_sample backward on the GPU does); sums of exactly representable
// terms (the exact-lattice tests) do not.  grad_ref is summed by one thread per
// element in plane order and is reproducible bit for bit.
#include <algorithm>
#include "sweep_common.h"

namespace sfm {

constexpr int kBwdThreads = 256;
constexpr int kBwdCG = 8;                 // channels per group: one position and four taps serve this many
constexpr int kBwdMaxRows = 8;            // reference rows per band, at most
constexpr size_t kBwdLds = 64 * 1024;     // window bytes per block, at most (two blocks per CU)

struct BwdGeom {
  int B, C, h, w, hw, L;
  int rows;        // gradient rows per plane: C (warped half only) or 2C
  int row0;        // first warped row: 0 or C
  int cg;          // channels per group: min(C, kBwdCG)
  int rb, nbands;  // reference rows per band, bands per image
  int lp, nchunks; // planes per chunk, chunks
  int wr;          // target rows of the LDS window (0: none, every tap a global atomic)
  float dmax, dstep;
};

// grad_tgt = 0 and, for the sweep, its tables: each pair's Proj (load_proj) and
// the plane depths (plane_depth), as the forward's relayout writes them.
__global__ __launch_bounds__(256) void k_sweep_bwd_prep(float* __restrict__ grad_tgt, size_t n, int B,
                                                        const float* __restrict__ pose, const float* __restrict__ K,
                                                        const float* __restrict__ Kinv, Proj* __restrict__ projs,
                                                        int L, float dmax, float dstep, float* __restrict__ depths) {
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (projs) {
    if (t0 < (size_t)B) {
      Proj pr;
      load_proj(pose, K, Kinv, (int)t0, pr);
      projs[t0] = pr;
    }
    for (size_t i = t0; i < (size_t)L; i += (size_t)gridDim.x * 256) depths[i] = plane_depth(dmax, dstep, (int)i);
  }
  for (size_t i = t0; i < n; i += (size_t)gridDim.x * 256) grad_tgt[i] = 0.0f;
}

// g: the volume's gradient [B][q.rows][L][hw]; depth_map [B][hw] or null (then
// the plane depths: `depths`, or plane_depth when that is null); projs [B] or
// null (then load_proj here).  grid (bands * chunks, channel groups, pairs).
__global__ __launch_bounds__(kBwdThreads) void k_sweep_bwd(const float* __restrict__ g,
                                                           const float* __restrict__ depth_map,
                                                           const float* __restrict__ pose,
                                                           const float* __restrict__ K,
                                                           const float* __restrict__ Kinv,
                                                           const Proj* __restrict__ projs,
                                                           const float* __restrict__ depths, BwdGeom q,
                                                           float* __restrict__ grad_tgt) {
  extern __shared__ float win[];   // [nc][wr][w]
  const int tid = (int)threadIdx.x;
  const int b = (int)blockIdx.z;
  const int c0 = (int)blockIdx.y * kBwdCG;
  const int nc = min(kBwdCG, q.C - c0);
  const int chunk = (int)(blockIdx.x / (unsigned)q.nbands);
  const int band = (int)blockIdx.x - chunk * q.nbands;
  const int y0 = band * q.rb, nrow = min(q.rb, q.h - y0);
  const int p0 = y0 * q.w, npix = nrow * q.w;
  const int l0 = chunk * q.lp, nl = min(q.lp, q.L - l0);
  const int wsz = q.wr * q.w;      // window elements per channel

  Proj pr;
  if (projs) pr = projs[b];
  else load_proj(pose, K, Kinv, b, pr);
  const SampleK sk = sample_consts(q.h, q.w);
  auto depth_at = [&](int l, int p) {
    if (depth_map) return depth_map[(size_t)b * q.hw + p];
    return depths ? depths[l] : plane_depth(q.dmax, q.dstep, l);
  };
  auto position = [&](int l, int p, float& ix, float& iy) {
    const int yy = p / q.w;
    const float xf = (float)(p - yy * q.w), yf = (float)yy;
    float ray[3];
    ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
    ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
    ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
    return sample_pos_nr(pr, ray, depth_at(l, p), sk, ix, iy);
  };

  int wy0 = 0;
  if (wsz > 0) {
    // where the band's centre samples on the chunk's middle plane (uniform); any choice is correct
    int cy = y0 + nrow / 2;
    float ix, iy;
    if (position(l0 + nl / 2, cy * q.w + q.w / 2, ix, iy)) cy = (int)floorf(iy);
    wy0 = min(max(cy - nrow / 2 - (q.wr - nrow - 1) / 2, 0), q.h - q.wr);
    for (int i = tid; i < nc * wsz; i += kBwdThreads) win[i] = 0.0f;
    __syncthreads();
  }

  float* G = grad_tgt + ((size_t)b * q.C + c0) * q.hw;
  const size_t cstride = (size_t)q.L * q.hw;
  const int items = nl * npix;
  for (int t = tid; t < items; t += kBwdThreads) {
    const int li = t / npix;
    const int l = l0 + li, p = p0 + (t - li * npix);
    float ix, iy;
    if (!position(l, p, ix, iy)) continue;
    Taps tp;
    make_taps(ix, iy, q.h, q.w, tp);
    const float* gp = g + (((size_t)b * q.rows + q.row0 + c0) * q.L + l) * q.hw + p;
    float gv[kBwdCG];
#pragma unroll
    for (int k = 0; k < kBwdCG; ++k) gv[k] = k < nc ? gp[k * cstride] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float wt = tp.wt[j];
      if (wt == 0.0f) continue;
      const int off = tp.off[j];
      const int rel = off - wy0 * q.w;
      if ((unsigned)rel < (unsigned)wsz) {
#pragma unroll
        for (int k = 0; k < kBwdCG; ++k)
          if (k < nc) atomicAdd(&win[k * wsz + rel], wt * gv[k]);
      } else {
#pragma unroll
        for (int k = 0; k < kBwdCG; ++k)
          if (k < nc) atomicAdd(&G[(size_t)k * q.hw + off], wt * gv[k]);
      }
    }
  }

  if (wsz > 0) {
    __syncthreads();
    const int base = wy0 * q.w;
    for (int i = tid; i < nc * wsz; i += kBwdThreads) {
      const float v = win[i];
      if (v == 0.0f) continue;
      const int c = i / wsz;
      atomicAdd(&G[(size_t)c * q.hw + base + (i - c * wsz)], v);
    }
  }
}

// grad_ref[b, c, p] = sum_i g[b, c, i, p], planes in index order, one thread per element
__global__ __launch_bounds__(256) void k_sweep_bwd_ref(const float* __restrict__ g, int C, int L, int hw, size_t n,
                                                       float* __restrict__ grad_ref) {
  const size_t chw = (size_t)C * hw;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const size_t b = e / chw, r = e - b * chw;
    const size_t c = r / hw, p = r - c * hw;
    const float* gp = g + ((b * 2 * C + c) * L) * hw + p;
    float acc = gp[0];
    for (int i = 1; i < L; ++i) acc = acc + gp[(size_t)i * hw];
    grad_ref[e] = acc;
  }
}

static unsigned bwd_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 16); }

static size_t bwd_ws_bytes(int B, int L) { return sweep_proj_bytes(B) + (((size_t)L * sizeof(float) + 255) & ~(size_t)255); }

// The launch shape: channel groups, row bands and plane chunks, and the LDS window that fits.
static BwdGeom bwd_geom(int B, int C, int h, int w, int L, int rows, int row0, float dmax, float dstep) {
  BwdGeom q;
  q.B = B; q.C = C; q.h = h; q.w = w; q.hw = h * w; q.L = L;
  q.rows = rows; q.row0 = row0; q.dmax = dmax; q.dstep = dstep;
  q.cg = std::min(C, kBwdCG);
  const size_t row_bytes = (size_t)q.cg * w * sizeof(float);
  q.wr = (int)std::min<size_t>((size_t)h, kBwdLds / row_bytes);
  if (q.wr < 2) q.wr = 0;                              // a window of one row holds no pixel's four taps
  q.wr = std::min(q.wr, kBwdMaxRows + 2);
  q.rb = q.wr ? std::max(1, q.wr - 2) : std::min(h, 4);   // the band's taps span rb + 1 rows when the rows do not drift
  q.nbands = (h + q.rb - 1) / q.rb;
  // planes per chunk: 16, fewer while the grid is under ~4 blocks per CU (a chunk's window flush is per chunk)
  const int64_t per_chunk = (int64_t)B * ((C + kBwdCG - 1) / kBwdCG) * q.nbands;
  q.lp = std::min(16, L);
  while (q.lp > 1 && per_chunk * ((L + q.lp - 1) / q.lp) < 1024) q.lp = (q.lp + 1) / 2;
  q.nchunks = (L + q.lp - 1) / q.lp;
  return q;
}

static int launch_sweep_bwd(const BwdGeom& q, const float* g, const float* depth_map, const float* pose,
                            const float* K, const float* Kinv, const Proj* projs, const float* depths,
                            float* grad_tgt, hipStream_t s) {
  const dim3 grid((unsigned)(q.nbands * q.nchunks), (unsigned)((q.C + kBwdCG - 1) / kBwdCG), (unsigned)q.B);
  const size_t lds = (size_t)q.cg * q.wr * q.w * sizeof(float);
  hipLaunchKernelGGL(k_sweep_bwd, grid, dim3(kBwdThreads), lds, s, g, depth_map, pose, K, Kinv, projs, depths, q,
                     grad_tgt);
  SFM_LAUNCHED();
  set_last_sweep(q.wr ? "k_sweep_bwd" : "k_sweep_bwd+global");
  return SFM_OK;
}

static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_plane_sweep_backward_workspace_bytes(int batch, int channels, int h, int w, int nlabel) {
  if (batch < 1 || channels < 1 || h < 1 || w < 1 || nlabel < 1) return 0;
  return bwd_ws_bytes(batch, nlabel);
}

int sfm_plane_sweep_backward(const float* grad_cost, int warped_only, int batch, int channels, int h, int w,
                             const float* pose, const float* K4, const float* K4inv, int nlabel, float min_depth,
                             int predict_by_depth, float* grad_ref, float* grad_tgt, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const int B = batch, C = channels, L = nlabel;
  SFM_REQUIRE(grad_cost && pose && K4 && K4inv && grad_tgt && workspace, "null pointer argument");
  SFM_REQUIRE(warped_only == 0 || warped_only == 1, "warped_only must be 0 or 1");
  SFM_REQUIRE(!(warped_only && grad_ref), "grad_ref must be null with warped_only (the volume has no reference rows)");
  SFM_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 4 * 65535 && h >= 2 && w >= 2 && L >= 1, "invalid sweep shape");
  SFM_REQUIRE(predict_by_depth == 0 || predict_by_depth == 1, "predict_by_depth must be 0 (inverse depth) or 1 (depth)");
  SFM_REQUIRE(min_depth > 0.0f, "min_depth must be positive");
  // a block's items (planes of a chunk x pixels of a band) and the grid's x (bands x chunks) are ints
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 30) && w < (1 << 23), "feature map too large");
  SFM_REQUIRE((int64_t)L * h < ((int64_t)1 << 31), "sweep too large: nlabel * h must be below 2^31");
  SFM_REQUIRE(aligned4(grad_cost) && aligned4(grad_ref) && aligned4(grad_tgt) && aligned4(pose) && aligned4(K4) &&
                  aligned4(K4inv) && aligned4(workspace),
              "buffers must be 4-byte aligned");
  if (int rc = check_sweep_workspace(workspace, workspace_bytes, bwd_ws_bytes(B, L))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float dmax = min_depth * (float)L;   // disp2depth = ones * MIN_DEPTH * nlabel (fp32)
  const float dstep = predict_by_depth ? min_depth : 0.0f;
  Proj* projs = (Proj*)workspace;
  float* depths = reinterpret_cast<float*>((char*)workspace + sweep_proj_bytes(B));
  const size_t n = (size_t)B * C * h * w;
  {
    ProfScope ps("sweep_bwd_prep", s);
    hipLaunchKernelGGL(k_sweep_bwd_prep, dim3(bwd_grid(std::max(n, (size_t)std::max(B, L)))), dim3(256), 0, s, grad_tgt,
                       n, B, pose, K4, K4inv, projs, L, dmax, dstep, depths);
    SFM_LAUNCHED();
  }
  if (grad_ref) {
    ProfScope ps("sweep_bwd_ref", s);
    hipLaunchKernelGGL(k_sweep_bwd_ref, dim3(bwd_grid(n)), dim3(256), 0, s, grad_cost, C, L, h * w, n, grad_ref);
    SFM_LAUNCHED();
  }
  const BwdGeom q = bwd_geom(B, C, h, w, L, warped_only ? C : 2 * C, warped_only ? 0 : C, dmax, dstep);
  ProfScope ps("sweep_bwd", s);
  return launch_sweep_bwd(q, grad_cost, nullptr, pose, K4, K4inv, projs, depths, grad_tgt, s);
}

int sfm_inverse_warp_backward(const float* grad_out, int batch, int channels, int h, int w, const float* depth,
                              const float* pose, const float* K, const float* Kinv, float* grad_feat, void* stream) {
  SFM_REQUIRE(grad_out && depth && pose && K && Kinv && grad_feat, "null pointer argument");
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 1 && channels <= 4 * 65535 && h >= 2 && w >= 2,
              "invalid warp shape");
  SFM_REQUIRE((int64_t)h * w < ((int64_t)1 << 30) && w < (1 << 23), "feature map too large");
  SFM_REQUIRE(aligned4(grad_out) && aligned4(depth) && aligned4(pose) && aligned4(K) && aligned4(Kinv) &&
                  aligned4(grad_feat),
              "buffers must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)batch * channels * h * w;
  {
    ProfScope ps("sweep_bwd_prep", s);
    hipLaunchKernelGGL(k_sweep_bwd_prep, dim3(bwd_grid(n)), dim3(256), 0, s, grad_feat, n, batch, pose, K, Kinv,
                       (Proj*)nullptr, 0, 0.0f, 0.0f, (float*)nullptr);
    SFM_LAUNCHED();
  }
  const BwdGeom q = bwd_geom(batch, channels, h, w, 1, channels, 0, 0.0f, 0.0f);
  ProfScope ps("inverse_warp_bwd", s);
  return launch_sweep_bwd(q, grad_out, depth, pose, K, Kinv, nullptr, nullptr, grad_feat, s);
}

}  // extern "C"
