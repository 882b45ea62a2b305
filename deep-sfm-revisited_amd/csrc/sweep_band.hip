// Plane-sweep cost volume, plane-run form with the target band in LDS (tuning
// key sweep_flat = 3): k_sweep_band and its launcher.
#include "sweep_common.h"

namespace sfm {

// ---------------------------------------------------------------------------
// Cost volume, plane-run form with the target band in LDS (sweep_flat = 3).
//
// k_sweep_tile is bound by the texture address/data units, not by HBM: per
// pixel and channel quad a lane issues four 16-byte tap gathers (64 B through
// the L1 path for 16 B of output), and re-reads the same target pixels at
// every plane (PMC: 1.8 GB of reads per launch against 0.06 GB algorithmic).
// Here one block produces a run of R consecutive planes of one 256*NJ-pixel
// tile for one channel quad:
//   * the source rows every tap of the run touches are found first (the same
//     sample positions, computed twice), and that band of full target rows --
//     contiguous in tq -- is copied once into LDS; the taps are then ds_read
//     from it (lanes whose taps fall outside a band clipped to the LDS budget
//     gather from global memory, same values);
//   * the tile's reference pixels (the same at every plane) are staged once
//     and stored R times;
//   * the windows stay 256-byte aligned per plane: at plane l the tile covers
//     pixels [WIN n - ph_l, WIN n - ph_l + WIN), ph_l the row's misalignment
//     at that plane, so every full wave store is one aligned segment.
// On KITTI (94x311 features, |t| 0.6) the band of a 16-plane run is 6 rows at
// the median, 14 at p99: ~15 B of staged reads per 4 channels of a pixel
// and plane instead of 64 B of gathers.  Same arithmetic as k_sweep_tile
// (bit-identical volumes).
// ---------------------------------------------------------------------------
template <int NJ>
__device__ __forceinline__ int band_pixel(int ws, int wave, int lane, int j) {
  return ws + 64 * NJ * wave + 64 * j + lane;
}

template <typename OutT, int NJ>
__global__ __launch_bounds__(kBandThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_sweep_band(const float* __restrict__ ref,
                                                             const f32x4* __restrict__ tq,
                                                             const float* __restrict__ pose,
                                                             const float* __restrict__ K4,
                                                             const float* __restrict__ K4inv, BandGeom g,
                                                             OutT* __restrict__ out) {
  constexpr bool BF = sizeof(OutT) == 2;
  static_assert(!BF || NJ % 2 == 0, "bf16 windows pack register pairs");
  constexpr int WIN = 256 * NJ;
  extern __shared__ f32x4 s_band[];            // cap_rows * w quads, then the reference tile
  __shared__ int s_ylo, s_yhi;
  const unsigned item = blockIdx.x;            // ((b * C4 + k) * nruns + run) * ntiles + n
  const unsigned r1 = magic_div(item, g.mtile);
  const int n = (int)(item - r1 * (unsigned)g.ntiles);
  const unsigned r2 = magic_div(r1, g.mrun);
  const int run = (int)(r1 - r2 * (unsigned)g.nruns);
  const int b = (int)magic_div(r2, g.mgrp);
  const int k = (int)(r2 - (unsigned)b * (unsigned)g.C4);
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = (tid >> 6) & 3, grp = tid >> 8;   // wave group grp takes planes l0 + grp + 4 i
  const int A = g.amask + 1;
  const int l0 = run * g.run, l1 = min(g.L, l0 + g.run);
  const int nc = min(4, g.C - 4 * k);
  const size_t wrow = ((size_t)b * g.rows + g.ref_rows + 4 * k) * (size_t)g.slab;   // first warped row
  const int wmis = (int)((wrow + (size_t)g.out_mis) & (size_t)g.amask);
  auto phase = [&](int l) { return (wmis + (int)(((unsigned)l * (unsigned)g.hwmod) & (unsigned)g.amask)) & g.amask; };
  const int rbase = WIN * n - A;               // reference tile: pixels [rbase, rbase + WIN + A)
  const int RW = WIN + A;                      // <= 640 < kBandThreads
  float* s_ref = reinterpret_cast<float*>(s_band + g.cap_rows * g.w);

  if (tid == 0) { s_ylo = 0x7fffffff; s_yhi = -1; }
  // reference tile loads first: in flight during the band estimate
  float rv[4];
  if (g.ref_rows) {
    const int p = rbase + tid;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* R = ref + ((size_t)b * g.C + 4 * k + min(c, nc - 1)) * g.hw;
      rv[c] = (tid < RW && p >= 0 && p < g.hw) ? R[p] : 0.0f;
    }
  }
  Proj pr;
  load_proj(pose, K4, K4inv, b, pr);
  const SampleK sk = sample_consts(g.h, g.w);
  auto pixel_ray = [&](int p, float (&ray)[3]) {
    int y = (int)((float)p * g.inv_w);
    int x = p - y * g.w;
    if (x < 0) { --y; x += g.w; }
    if (x >= g.w) { ++y; x -= g.w; }
    const float xf = (float)x, yf = (float)y;
    ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
    ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
    ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
  };

  // Band estimate: the tap rows of the tile at four planes of the run (its
  // first and last, and two between; one per wave group).  A pixel's sample
  // moves monotonically along its epipolar line with the plane, so the run's
  // taps lie between the end planes' almost everywhere; the exceptions (and
  // bands clipped to cap_rows) take the global path below, so the estimate
  // changes only speed, never values.
  int ylo = 0x7fffffff, yhi = -1;
  {
    const int l = l0 + (grp * (l1 - 1 - l0) + 1) / 3;
    const float d = plane_depth(g.dmax, g.dstep, l);
    const int ws = WIN * n - phase(l);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int p = band_pixel<NJ>(ws, wave, lane, j);
      if (p >= 0 && p < g.hw) {
        float ray[3], ix, iy;
        pixel_ray(p, ray);
        if (sample_pos_nr(pr, ray, d, sk, ix, iy)) {
          const int y0 = (int)floorf(iy);
          ylo = min(ylo, y0);
          yhi = max(yhi, y0 + (y0 < g.h - 1 ? 1 : 0));
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    ylo = min(ylo, __shfl_xor(ylo, o));
    yhi = max(yhi, __shfl_xor(yhi, o));
  }
  __syncthreads();   // s_ylo / s_yhi initialised
  if (lane == 0) { atomicMin(&s_ylo, ylo); atomicMax(&s_yhi, yhi); }
  if (g.ref_rows && tid < RW) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s_ref[c * RW + tid] = rv[c];
  }
  __syncthreads();
  int by0 = s_ylo, nb = 0;
  if (s_yhi >= by0) {
    // a little slack around the estimate, inside the image and the LDS
    const int want_lo = max(by0 - 1, 0), want_hi = min(s_yhi + 1, g.h - 1);
    nb = min(want_hi - want_lo + 1, g.cap_rows);
    by0 = want_lo;
  } else {
    by0 = 0;
  }
  const f32x4* T = tq + ((size_t)b * g.C4 + k) * g.hw;   // this quad's target plane
  {
    const f32x4* src = T + (size_t)by0 * g.w;
    const int cnt = nb * g.w;
    int i = tid;
    for (; i + kBandThreads < cnt; i += 2 * kBandThreads) {
      const f32x4 a0 = src[i], a1 = src[i + kBandThreads];
      s_band[i] = a0; s_band[i + kBandThreads] = a1;
    }
    if (i < cnt) s_band[i] = src[i];
  }
  __syncthreads();
  const unsigned lo = (unsigned)(by0 * g.w), span = (unsigned)(nb * g.w);
  const bool odd = (lane & 1) != 0;

  for (int l = l0 + grp; l < l1; l += 4) {
    const float d = plane_depth(g.dmax, g.dstep, l);
    const int ws = WIN * n - phase(l);
    const int fl = l * g.hw;                   // slab index of the plane's pixel 0
    float acc[4][NJ], cp[4][NJ];
    bool ok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int p = band_pixel<NJ>(ws, wave, lane, j);
      ok[j] = p >= 0 && p < g.hw;
      const int pp = ok[j] ? p : max(rbase, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[c][j] = 0.0f;
        cp[c][j] = g.ref_rows ? s_ref[c * RW + (pp - rbase)] : 0.0f;
      }
      float ray[3], ix, iy;
      pixel_ray(pp, ray);
      if (ok[j] && sample_pos_nr(pr, ray, d, sk, ix, iy)) {
        TapsIn tp;
        make_taps_inside(ix, iy, g.h, g.w, tp);
        f32x4 t0, t1, t2, t3;
        if (tp.off[0] - lo < span && tp.off[3] - lo < span) {
          t0 = s_band[tp.off[0] - lo]; t1 = s_band[tp.off[1] - lo];
          t2 = s_band[tp.off[2] - lo]; t3 = s_band[tp.off[3] - lo];
        } else {
          t0 = *at_u32(T, tp.off[0] * 16u); t1 = *at_u32(T, tp.off[1] * 16u);
          t2 = *at_u32(T, tp.off[2] * 16u); t3 = *at_u32(T, tp.off[3] * 16u);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = tp.wt[0] * t0[e];
          v = __builtin_fmaf(tp.wt[1], t1[e], v);
          v = __builtin_fmaf(tp.wt[2], t2[e], v);
          acc[e][j] = __builtin_fmaf(tp.wt[3], t3[e], v);
        }
      }
    }
    auto store_row = [&](OutT* row, const float* v) {
      if (!BF) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int p = band_pixel<NJ>(ws, wave, lane, j);
          if (ok[j]) store1(at_u32(row, (unsigned)(fl + p) * 4u), v[j]);
        }
      } else {
#pragma unroll
        for (int s = 0; s < NJ / 2; ++s) {
          const unsigned a = to_bf16(v[2 * s]), bb = to_bf16(v[2 * s + 1]);
          const unsigned u = bf16_pair_swap(a, bb, odd);
          // even lane 2m: pixels 128 s + 2m, +1; odd lane 2m+1: 128 s + 64 + 2m, +1
          const int p = ws + 64 * NJ * wave + 128 * s + lane + (odd ? 63 : 0);
          const bool okl = p >= 0 && p < g.hw, okh = p + 1 >= 0 && p + 1 < g.hw;
          if (g.pair_ok && okl && okh) {
            *reinterpret_cast<unsigned int*>(at_u32(row, (unsigned)(fl + p) * 2u)) = u;
          } else {
            if (okl) row[fl + p] = (unsigned short)(u & 0xffffu);
            if (okh) row[fl + p + 1] = (unsigned short)(u >> 16);
          }
        }
      }
    };
    if (g.ref_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= nc) break;
        store_row(out + ((size_t)b * g.rows + 4 * k + c) * (size_t)g.slab, cp[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= nc) break;
      store_row(out + wrow + (size_t)c * g.slab, acc[c]);
    }
  }
}

int launch_sweep_band(const SweepPlan& p, const SweepOperands& op, hipStream_t s) {
  // plan.lds (band_lds_bytes) is above the default limit of dynamic LDS
  if (p.out_dtype == 0) {
    SFM_HIP(hipFuncSetAttribute((const void*)k_sweep_band<float, 1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds));
    hipLaunchKernelGGL((k_sweep_band<float, 1>), dim3(p.blocks), dim3(kBandThreads), p.lds, s, op.ref, op.tq, op.pose,
                       op.K4, op.K4inv, p.band, (float*)op.out);
  } else {
    SFM_HIP(hipFuncSetAttribute((const void*)k_sweep_band<unsigned short, 2>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL((k_sweep_band<unsigned short, 2>), dim3(p.blocks), dim3(kBandThreads), p.lds, s, op.ref,
                       op.tq, op.pose, op.K4, op.K4inv, p.band, (unsigned short*)op.out);
  }
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace sfm
