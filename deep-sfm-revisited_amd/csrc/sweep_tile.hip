// Plane-sweep cost volume, the two aligned-slab-window forms: k_sweep_flat
// (tuning key sweep_flat = 1) and k_sweep_tile (sweep_flat = 2, the default),
// which share FlatGeom and the in-image taps, with their launchers.
#include "sweep_common.h"

namespace sfm {

// ---------------------------------------------------------------------------
// Cost volume, aligned-slab form (tuning key sweep_flat = 1).
//
// Each output row (b, r) of the [B, rows, L, h, w] volume is one contiguous
// slab of L*h*w elements.  A work item is a 1024-element window of the slabs
// of one channel group: G = 4*NQ warped rows (channels 4*NQ*k ..) and, for
// the full volume, the G reference rows of the same channels.  Window starts
// are 256-byte aligned in absolute address (a window may straddle two
// planes), so every wave store is one aligned 256-byte segment.
//   * git-history scripts/probe_store_bw2.hip (profiles/r01_probe_store_bw2.txt): stores
//     of this shape run at 6.3-7.0 TB/s on MI355X for 1-8 rows per item, the
//     per-row windows of k_sweep at 4.0-5.0 (their 256-byte wave segments straddle
//     cache lines: rows start at arbitrary 4-byte offsets).
//   * Pairing the copy rows with the warped rows in one item keeps every
//     block half store-bound, half VALU-bound, so the two overlap on every
//     CU instead of alternating between all-copy and all-warp phases.
//   * One item per block, items in address order (window fastest): the
//     resident blocks sweep a narrow front of the 2G slabs.
//   * Every vector-memory byte passes the CU's 64 B/clk L1 path: per 4-byte
//     output ~8 B of tap gathers (16 B per warped output), 2 B of reference
//     loads and the 4 B store.  Rays K^-1 (x, y, 1) are therefore recomputed
//     (18 VALU) rather than read from a per-pixel table (16 B per pixel and
//     plane; measured 1.36 vs 1.32 ms at KITTI B=8, L=128).
// Arithmetic: the reference's float32 expression order (warp.h
// sample_pos_nr: the same bits as sample_pos with Newton-Raphson divisions),
// the bilinear taps in the in-image form (make_taps_inside), and FMA in the
// 4-tap sum (within 1 ulp of the per-row kernel's mul/add chain).  Uniform
// integer divisions use magic numbers.
// ---------------------------------------------------------------------------
template <typename OutT> struct FlatLanes;   // pixels per lane per store, stores per lane per row
template <> struct FlatLanes<float> { static constexpr int PXL = 1, NS = 4; };
template <> struct FlatLanes<unsigned short> { static constexpr int PXL = 2, NS = 2; };

template <typename OutT, int PXL>
__device__ __forceinline__ void store_px(OutT* row, int f0, int slab, bool pair_ok, const float* v) {
  if (PXL == 1) {
    if (f0 >= 0 && f0 < slab) store1(row + f0, v[0]);
  } else {
    if (pair_ok && f0 >= 0 && f0 + 1 < slab) {
      const unsigned int u = (unsigned int)to_bf16(v[0]) | ((unsigned int)to_bf16(v[1]) << 16);
      *reinterpret_cast<unsigned int*>(row + f0) = u;
    } else {
#pragma unroll
      for (int k = 0; k < PXL; ++k)
        if (f0 + k >= 0 && f0 + k < slab) store1(row + f0 + k, v[k]);
    }
  }
}

// One item's body.  INTERIOR: the window lies inside the slab (every lane
// pixel valid; unguarded stores), else edge windows with per-pixel guards.
template <typename OutT, int NQ, bool INTERIOR>
__device__ __forceinline__ void sweep_flat_item(const float* __restrict__ ref, const f32x4* __restrict__ tq,
                                                const float* __restrict__ pose,
                                                const float* __restrict__ K4, const float* __restrict__ K4inv,
                                                const FlatGeom& g, OutT* __restrict__ out, int b, int k,
                                                int start, size_t wbase) {
  constexpr int PXL = FlatLanes<OutT>::PXL, NS = FlatLanes<OutT>::NS, NPX = PXL * NS;
  constexpr int G = 4 * NQ;
  const int c0 = k * G;
  const int l0 = (int)magic_div((unsigned)max(start, 0), g.mhw);
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  // lane pixels: slab index f = start + 256 wave + 64 PXL s + PXL lane + e
  int fs[NS], ps[NPX], ls[NPX];
  const int pbase = start - l0 * g.hw;         // in-plane index of the window start (< 0 only at an edge)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    fs[s] = start + 256 * wave + 64 * PXL * s + PXL * lane;
#pragma unroll
    for (int e = 0; e < PXL; ++e) {
      int p = pbase + 256 * wave + 64 * PXL * s + PXL * lane + e, l = l0;
      if (!INTERIOR) {
        const int f = fs[s] + e;
        if (f < 0 || f >= g.slab) p = 0;
      }
      while (p >= g.hw) { p -= g.hw; ++l; }
      ps[s * PXL + e] = p;
      ls[s * PXL + e] = l;
    }
  }
  const int nc = min(G, g.C - c0);
  // reference rows of the group: loads first (in flight during the warp)
  float cp[G][NPX];
  if (g.ref_rows) {
#pragma unroll
    for (int c = 0; c < G; ++c) {
      if (c >= nc) break;
      const float* R = ref + ((size_t)b * g.C + c0 + c) * g.hw;
#pragma unroll
      for (int j = 0; j < NPX; ++j) cp[c][j] = *at_u32(R, (unsigned)ps[j] * 4u);
    }
  }
  Proj pr;
  load_proj(pose, K4, K4inv, b, pr);
  const SampleK sk = sample_consts(g.h, g.w);
  const float dA = plane_depth(g.dmax, g.dstep, l0), dB = plane_depth(g.dmax, g.dstep, l0 + 1);
  const f32x4* Tb = tq + ((size_t)b * g.C4 + k * NQ) * g.hw;
  f32x4 acc[NQ][NPX];
#pragma unroll
  for (int j = 0; j < NPX; ++j) {
    const int p = ps[j], l = ls[j];
    float d = l == l0 ? dA : dB;
    if (l > l0 + 1) d = plane_depth(g.dmax, g.dstep, l);   // feature maps under 1024 pixels
    // pixel (x, y) = (p % w, p / w): float reciprocal and one correction (p < 2^24),
    // then the ray K^-1 (x, y, 1) in the reference's order (pixel2cam)
    int y = (int)((float)p * g.inv_w);
    int x = p - y * g.w;
    if (x < 0) { --y; x += g.w; }
    if (x >= g.w) { ++y; x -= g.w; }
    const float xf = (float)x, yf = (float)y;
    float ray[3];
    ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
    ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
    ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
    float ix, iy;
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc[n][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (sample_pos_nr(pr, ray, d, sk, ix, iy)) {
      TapsIn tp;
      make_taps_inside(ix, iy, g.h, g.w, tp);
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        if (4 * n >= nc) break;
        const f32x4* T = Tb + (size_t)n * g.hw;
        const f32x4 t0 = *at_u32(T, tp.off[0] * 16u), t1 = *at_u32(T, tp.off[1] * 16u);
        const f32x4 t2 = *at_u32(T, tp.off[2] * 16u), t3 = *at_u32(T, tp.off[3] * 16u);
        f32x4 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = tp.wt[0] * t0[e];
          v = __builtin_fmaf(tp.wt[1], t1[e], v);
          v = __builtin_fmaf(tp.wt[2], t2[e], v);
          a[e] = __builtin_fmaf(tp.wt[3], t3[e], v);
        }
        acc[n][j] = a;
      }
    }
  }
  // stores: row base + 32-bit byte offset of the window (slab < 2^30 elements)
  auto store_row = [&](OutT* row, const float* v) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (INTERIOR) {
        OutT* dst = at_u32(row, (unsigned)fs[s] * (unsigned)sizeof(OutT));
        if (PXL == 1) {
          store1(dst, v[s]);
        } else {
          const unsigned int u = (unsigned int)to_bf16(v[2 * s]) | ((unsigned int)to_bf16(v[2 * s + 1]) << 16);
          if (g.pair_ok) *reinterpret_cast<unsigned int*>(dst) = u;
          else { store1(dst, v[2 * s]); store1(dst + 1, v[2 * s + 1]); }
        }
      } else {
        store_px<OutT, PXL>(row, fs[s], g.slab, g.pair_ok, v + s * PXL);
      }
    }
  };
  if (g.ref_rows) {
#pragma unroll
    for (int c = 0; c < G; ++c) {
      if (c >= nc) break;
      store_row(out + ((size_t)b * g.rows + c0 + c) * (size_t)g.slab, cp[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < G; ++c) {
    if (c >= nc) break;
    float v[NPX];
#pragma unroll
    for (int j = 0; j < NPX; ++j) v[j] = acc[c >> 2][j][c & 3];
    store_row(out + wbase + (size_t)c * g.slab, v);
  }
}

template <typename OutT, int NQ>
__global__ __launch_bounds__(kSwThreads) void k_sweep_flat(const float* __restrict__ ref,
                                                           const f32x4* __restrict__ tq,
                                                           const float* __restrict__ pose,
                                                           const float* __restrict__ K4,
                                                           const float* __restrict__ K4inv, FlatGeom g,
                                                           OutT* __restrict__ out) {
  const unsigned item = blockIdx.x;            // grid = B * groups * nwin
  const unsigned r = magic_div(item, g.mwin);
  const int win = (int)(item - r * (unsigned)g.nwin);
  const int b = (int)magic_div(r, g.mgrp);
  const int k = (int)(r - (unsigned)b * (unsigned)g.groups);
  const size_t wbase = ((size_t)b * g.rows + g.ref_rows + k * 4 * NQ) * (size_t)g.slab;   // first warped row
  const int start = win * kFlatWin - (int)((wbase + (size_t)g.out_mis) & (size_t)g.amask);
  if (start >= g.slab) return;
  if (start >= 0 && start + kFlatWin <= g.slab)
    sweep_flat_item<OutT, NQ, true>(ref, tq, pose, K4, K4inv, g, out, b, k, start, wbase);
  else
    sweep_flat_item<OutT, NQ, false>(ref, tq, pose, K4, K4inv, g, out, b, k, start, wbase);
}

// ---------------------------------------------------------------------------
// Cost volume, narrow-window form (tuning key sweep_flat = 2, the default).
//
// The same aligned slab windows as k_sweep_flat, but a window is 256 * NJ
// elements and every lane owns NJ lane-consecutive pixels (wave pixel
// 64 j + lane), for both output types:
//   * HBM write rate on MI355X falls with the bytes that the resident
//     workgroups have in flight at once (profiles/r01_probe_store_bw2.txt:
//     items of 1 / 4 / 8 / 16 rows x 4 KB: 6.7 / 6.5 / 6.3 / 5.7 TB/s; one
//     contiguous span of 4 KB vs 64 KB per block: 7.0 vs 6.0 TB/s).  An item
//     writes 2G rows; NJ = 1 keeps it at 2G x 1 KB.
//   * bf16: neighbouring lanes' pixels are packed into 4-byte pairs with one
//     DPP quad swap (lane 2k stores pixels 64 j + 2k, +1 of register j = 2s,
//     lane 2k + 1 those of register 2s + 1), so the gathers stay
//     lane-consecutive and each wave store is still one 256-byte segment.
// ---------------------------------------------------------------------------

template <typename OutT, int NQ, int NJ, bool INTERIOR>
__device__ __forceinline__ void sweep_tile_item(const float* __restrict__ ref, const f32x4* __restrict__ tq,
                                                const float* __restrict__ pose,
                                                const float* __restrict__ K4, const float* __restrict__ K4inv,
                                                const FlatGeom& g, OutT* __restrict__ out, int b, int k,
                                                int start, size_t wbase) {
  constexpr bool BF = sizeof(OutT) == 2;
  static_assert(!BF || NJ % 2 == 0, "bf16 windows pack register pairs");
  constexpr int G = 4 * NQ, WW = 64 * NJ;
  const int c0 = k * G;
  const int l0 = (int)magic_div((unsigned)max(start, 0), g.mhw);
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int woff = start + WW * wave;                 // slab index of the wave's first pixel
  int ps[NJ], ls[NJ];
  bool okf[NJ];
  const int pbase = start - l0 * g.hw;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int f = woff + 64 * j + lane;
    int p = pbase + WW * wave + 64 * j + lane, l = l0;
    okf[j] = true;
    if (!INTERIOR) {
      okf[j] = f >= 0 && f < g.slab;
      if (!okf[j]) p = 0;
    }
    while (p >= g.hw) { p -= g.hw; ++l; }
    ps[j] = p;
    ls[j] = l;
  }
  const int nc = min(G, g.C - c0);
  constexpr bool LATE = NJ >= 8;                      // reference rows loaded at their stores (registers)
  float cp[LATE ? 1 : G][NJ];
  auto load_ref_row = [&](int c, float* v) {
    const float* R = ref + ((size_t)b * g.C + c0 + c) * g.hw;
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] = *at_u32(R, (unsigned)ps[j] * 4u);
  };
  if (!LATE && g.ref_rows && g.write_ref) {
#pragma unroll
    for (int c = 0; c < G; ++c) {
      if (c >= nc) break;
      load_ref_row(c, cp[LATE ? 0 : c]);
    }
  }
  Proj pr;
  load_proj(pose, K4, K4inv, b, pr);
  const SampleK sk = sample_consts(g.h, g.w);
  const float dA = plane_depth(g.dmax, g.dstep, l0), dB = plane_depth(g.dmax, g.dstep, l0 + 1);
  const f32x4* Tb = tq + ((size_t)b * g.C4 + k * NQ) * g.hw;
  f32x4 acc[NQ][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = ps[j], l = ls[j];
    float d = l == l0 ? dA : dB;
    if (l > l0 + 1) d = plane_depth(g.dmax, g.dstep, l);
    int y = (int)((float)p * g.inv_w);
    int x = p - y * g.w;
    if (x < 0) { --y; x += g.w; }
    if (x >= g.w) { ++y; x -= g.w; }
    const float xf = (float)x, yf = (float)y;
    float ray[3];
    ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
    ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
    ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
    float ix, iy;
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc[n][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (sample_pos_nr(pr, ray, d, sk, ix, iy)) {
      TapsIn tp;
      make_taps_inside(ix, iy, g.h, g.w, tp);
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        if (4 * n >= nc) break;
        const f32x4* T = Tb + (size_t)n * g.hw;
        const f32x4 t0 = *at_u32(T, tp.off[0] * 16u), t1 = *at_u32(T, tp.off[1] * 16u);
        const f32x4 t2 = *at_u32(T, tp.off[2] * 16u), t3 = *at_u32(T, tp.off[3] * 16u);
        f32x4 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = tp.wt[0] * t0[e];
          v = __builtin_fmaf(tp.wt[1], t1[e], v);
          v = __builtin_fmaf(tp.wt[2], t2[e], v);
          a[e] = __builtin_fmaf(tp.wt[3], t3[e], v);
        }
        acc[n][j] = a;
      }
    }
  }
  const bool odd = (lane & 1) != 0;
  auto store_row = [&](OutT* row, const float* v) {
    if (!BF) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int f = woff + 64 * j + lane;
        if (INTERIOR || okf[j]) store1(at_u32(row, (unsigned)f * 4u), v[j]);
      }
    } else {
#pragma unroll
      for (int s = 0; s < NJ / 2; ++s) {
        const unsigned a = to_bf16(v[2 * s]), bb = to_bf16(v[2 * s + 1]);
        const unsigned u = bf16_pair_swap(a, bb, odd);
        // even lane 2k: pixels 128 s + 2k, +1; odd lane 2k+1: 128 s + 64 + 2k, +1
        const int f = woff + 128 * s + lane + (odd ? 63 : 0);
        if (INTERIOR && g.pair_ok) {
          *reinterpret_cast<unsigned int*>(at_u32(row, (unsigned)f * 2u)) = u;
        } else {
          const bool okl = f >= 0 && f < g.slab, okh = f + 1 >= 0 && f + 1 < g.slab;
          if (g.pair_ok && okl && okh) {
            *reinterpret_cast<unsigned int*>(row + f) = u;
          } else {
            if (okl) row[f] = (unsigned short)(u & 0xffffu);
            if (okh) row[f + 1] = (unsigned short)(u >> 16);
          }
        }
      }
    }
  };
  if (g.ref_rows && g.write_ref) {
#pragma unroll
    for (int c = 0; c < G; ++c) {
      if (c >= nc) break;
      if (LATE) load_ref_row(c, cp[0]);
      store_row(out + ((size_t)b * g.rows + c0 + c) * (size_t)g.slab, cp[LATE ? 0 : c]);
    }
  }
#pragma unroll
  for (int c = 0; c < G; ++c) {
    if (c >= nc) break;
    float v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] = acc[c >> 2][j][c & 3];
    store_row(out + wbase + (size_t)c * g.slab, v);
  }
}

// Interior windows of a full channel group (the bulk of the volume), with
// buffer addressing: one SGPR resource per pair and tensor, the per-lane
// pixel byte offset in one VGPR shared by every row, each row's offset in an
// SGPR (soffset).  The generic body above spends ~200 VALU per wave item on
// 64-bit address arithmetic, partial-group branches and their zero moves
// (SQ_INSTS_VALU 324 per item at KITTI, ~110 of them the sampling itself);
// here stores and loads need no VALU address work.  Same arithmetic, so the
// same bits.  Requires every per-pair byte range below 2^32 (g.buf_ok).
// (sweep_tile_fast below; buf_rsrc: sweep_common.h)

// Lane i + 1's value in lane i (DPP wave_shl:1; lane 63 reads 0).
__device__ __forceinline__ unsigned next_lane_u(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true);
}
__device__ __forceinline__ float next_lane_f(float v) { return __uint_as_float(next_lane_u(__float_as_uint(v))); }

template <typename OutT, int NQ, int NJ, bool SHARE, bool NT, bool WIDE = false, int WPOL = -1>
__device__ __forceinline__ void sweep_tile_fast(const float* __restrict__ ref, const f32x4* __restrict__ tq,
                                                const Proj* __restrict__ projs, const FlatGeom& g,
                                                OutT* __restrict__ out, int b, int k, int start) {
  constexpr bool BF = sizeof(OutT) == 2;
  constexpr int G = 4 * NQ, WW = 64 * NJ;
  const int c0 = k * G;
  const int l0 = (int)magic_div((unsigned)start, g.mhw);
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int woff = start + WW * wave;
  const int pbase = start - l0 * g.hw;
  int ps[NJ], ls[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    int p = pbase + WW * wave + 64 * j + lane, l = l0;
    if (g.hw >= 256 * NJ) {                    // a window spans at most two planes
      if (p >= g.hw) { p -= g.hw; ++l; }
    } else {
      while (p >= g.hw) { p -= g.hw; ++l; }
    }
    ps[j] = p;
    ls[j] = l;
  }
  const __amdgpu_buffer_rsrc_t rout = buf_rsrc(out + (size_t)b * g.rows * g.slab, g.pair_bytes);
  const unsigned row_bytes = (unsigned)g.slab * (unsigned)sizeof(OutT);
  // the reference rows: loaded up front (their latency under the sampling),
  // or, with wide stores (more pixels per lane), row by row at their stores
  const __amdgpu_buffer_rsrc_t rref = buf_rsrc(ref + ((size_t)b * g.C + c0) * g.hw, (unsigned)G * g.hw * 4u);
  auto load_ref_row = [&](int c, float* v) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      v[j] = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rref, (unsigned)ps[j] * 4u, (unsigned)c * g.hw * 4u, 0));
  };
  constexpr bool LATE = WIDE && NJ == 8;        // registers: the reference rows at their stores
  float cp[LATE ? 1 : G][NJ];
  if (!LATE && g.ref_rows && g.write_ref) {
#pragma unroll
    for (int c = 0; c < G; ++c) load_ref_row(c, cp[LATE ? 0 : c]);
  }
  const Proj pr = projs[b];                    // uniform: scalar loads
  const SampleK sk = sample_consts(g.h, g.w);
  float dA, dB;
  if (g.depths) {
    dA = g.depths[l0];
    dB = l0 + 1 < g.L ? g.depths[l0 + 1] : dA;
  } else {
    dA = plane_depth(g.dmax, g.dstep, l0);
    dB = plane_depth(g.dmax, g.dstep, l0 + 1);
  }
  const __amdgpu_buffer_rsrc_t rtq =
      buf_rsrc(tq + ((size_t)b * g.C4 + k * NQ) * g.hw, (unsigned)NQ * g.hw * 16u);
  f32x4 acc[NQ][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = ps[j], l = ls[j];
    float d = l == l0 ? dA : dB;
    if (l > l0 + 1) d = plane_depth(g.dmax, g.dstep, l);
    int y = (int)((float)p * g.inv_w);
    int x = p - y * g.w;
    if (x < 0) { --y; x += g.w; }
    if (x >= g.w) { ++y; x -= g.w; }
    const float xf = (float)x, yf = (float)y;
    float ray[3];
    ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
    ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
    ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
    float ix, iy;
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc[n][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (SHARE) {
      // Lanes hold consecutive pixels, and a fronto-parallel plane maps
      // neighbouring pixels ~one source pixel apart: lane i's right-hand taps
      // (off[1], off[3]) are usually lane i + 1's left-hand taps (off[0],
      // off[2]).  Each lane gathers its left-hand taps, takes the right-hand
      // ones from the next lane where the offsets are equal (then the values
      // are the same memory words), and gathers them itself elsewhere: half
      // the tap gathers through the texture path, the same bits.
      const bool in = sample_pos_nr(pr, ray, d, sk, ix, iy);
      TapsIn tp;
      if (in) {
        make_taps_inside(ix, iy, g.h, g.w, tp);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { tp.off[e] = 0u; tp.wt[e] = 0.0f; }
      }
      const unsigned n0 = next_lane_u(tp.off[0]), n2 = next_lane_u(tp.off[2]);
      const unsigned nin = next_lane_u(in ? 1u : 0u);
      const bool own = in && !(nin != 0u && n0 == tp.off[1] && n2 == tp.off[3]);
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        const unsigned so = (unsigned)n * g.hw * 16u;
        f32x4 t[4];
        t[0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        t[2] = t[0];
        if (in) {
          t[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[0] * 16u, so, 0));
          t[2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[2] * 16u, so, 0));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[1][e] = next_lane_f(t[0][e]);
          t[3][e] = next_lane_f(t[2][e]);
        }
        if (own) {
          t[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[1] * 16u, so, 0));
          t[3] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[3] * 16u, so, 0));
        }
        f32x4 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = tp.wt[0] * t[0][e];
          v = __builtin_fmaf(tp.wt[1], t[1][e], v);
          v = __builtin_fmaf(tp.wt[2], t[2][e], v);
          a[e] = __builtin_fmaf(tp.wt[3], t[3][e], v);
        }
        if (in) acc[n][j] = a;
      }
    } else if (sample_pos_nr(pr, ray, d, sk, ix, iy)) {
      TapsIn tp;
      make_taps_inside(ix, iy, g.h, g.w, tp);
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        const unsigned so = (unsigned)n * g.hw * 16u;
        f32x4 t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          t[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[e] * 16u, so, 0));
        f32x4 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = tp.wt[0] * t[0][e];
          v = __builtin_fmaf(tp.wt[1], t[1][e], v);
          v = __builtin_fmaf(tp.wt[2], t[2][e], v);
          a[e] = __builtin_fmaf(tp.wt[3], t[3][e], v);
        }
        acc[n][j] = a;
      }
    }
  }
  const bool odd = (lane & 1) != 0;
  // volume stores: with NT the cache policy is sc0 nt (non-temporal, the
  // volume is never re-read by this kernel), so the 7.7 GB of streaming
  // writes do not evict the reference rows and target quads that every plane
  // re-reads from L2 (tuning key sweep_store_nt, profiles/r02_sweep_nt_ab.txt:
  // bf16 0.474 -> 0.442 ms; fp32 1.255 -> 1.265, so by default bf16 only)
  auto bstore = [&](unsigned v, __amdgpu_buffer_rsrc_t r, unsigned off, unsigned so) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, off, so, NT ? 3 : 0);
  };
  // row r of the pair: soffset r * row_bytes; per-lane byte offset(s) of the window
  auto store_row = [&](unsigned r, const float* v) {
    const unsigned so = r * row_bytes;
    if (!BF) {                                  // (wide stores: put / flush below)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        bstore(__float_as_uint(v[j]), rout, (unsigned)(woff + 64 * j + lane) * 4u, so);
    } else {
#pragma unroll
      for (int s = 0; s < NJ / 2; ++s) {
        const unsigned u = bf16_pair_swap(to_bf16(v[2 * s]), to_bf16(v[2 * s + 1]), odd);
        const int f = woff + 128 * s + lane + (odd ? 63 : 0);
        bstore(u, rout, (unsigned)f * 2u, so);
      }
    }
  };
  if constexpr (WIDE) {
    // 16-byte lane stores (sweep_store_px): a 16-byte store holds EPL pixels
    // (8 bf16 / 4 fp32) and the wave's window of a row, 64 NJ pixels, takes
    // LPR = 64 NJ / EPL lanes, so one store instruction covers RPS = 64 / LPR
    // consecutive rows.  The pixels go through a per-wave LDS stage of RPS
    // rows (1 KB) at their window positions and come back as EPL consecutive
    // pixels per lane; the tap gathers stay lane-consecutive.
    constexpr int EPL = 16 / (int)sizeof(OutT), LPR = 64 * NJ / EPL, RPS = 64 / LPR;
    // the 16-byte stores' cache policy: sc0 nt / plain by NT, or WPOL (sc1:
    // write-through, the line is not kept in the XCD's L2 -- tuning key
    // sweep_store_wt)
    constexpr int POL = WPOL >= 0 ? WPOL : (NT ? 3 : 0);
    static_assert(NJ <= EPL && EPL % NJ == 0, "wide stores: NJ divides the pixels of a 16-byte store");
    __shared__ __attribute__((aligned(16))) uint32_t s_rows[kSwThreads / 64][RPS][16 * LPR / 4];
    const int rr = lane / LPR, cl = lane - rr * LPR;
    const unsigned voff = (unsigned)(woff + EPL * cl) * (unsigned)sizeof(OutT) + (unsigned)rr * row_bytes;
    // (per-pixel LDS writes; the DPP-packed pairs staged as 4-byte writes are
    // equally correct since the store-hazard fix below, profiles/r05_store_hazard.txt)
    auto put = [&](int slot, const float* v) {
      OutT* st = reinterpret_cast<OutT*>(s_rows[wave][slot]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (BF) st[64 * j + lane] = (unsigned short)to_bf16(v[j]);
        else st[64 * j + lane] = v[j];
      }
    };
    auto flush = [&](unsigned r0) {             // rows r0 .. r0 + RPS - 1
      sweep_wave_sync();
      const u32x4 x = *reinterpret_cast<const u32x4*>(&s_rows[wave][rr][4 * cl]);
      // the row offset in voffset with a literal-0 soffset, not an SGPR
      // soffset: a 128-bit store's data VGPRs must not be overwritten by the
      // next instruction (gfx950 stores the new value for lanes 16r+12..15
      // otherwise, scripts/probe_store_hazard.hip), and LLVM's hazard
      // recognizer inserts that wait state only for stores without an SGPR
      // soffset -- the round-4 "4-byte staging miscompute" was this pair
      // (profiles/r05_store_hazard.txt)
      __builtin_amdgcn_raw_buffer_store_b128(x, rout, voff + r0 * row_bytes, 0, POL);
      sweep_wave_sync();                        // the stage's reads before the next rows' writes
    };
    static_assert(G % RPS == 0, "row groups");
#pragma unroll
    for (int c = 0; c < G; c += RPS) {
#pragma unroll
      for (int t = 0; t < RPS; ++t) {
        float v[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[j] = acc[(c + t) >> 2][j][(c + t) & 3];
        put(t, v);
      }
      flush((unsigned)(g.ref_rows + c0 + c));
    }
    if (g.ref_rows && g.write_ref) {
#pragma unroll
      for (int c = 0; c < G; c += RPS) {
#pragma unroll
        for (int t = 0; t < RPS; ++t) {
          if (LATE) {
            float v[NJ];
            load_ref_row(c + t, v);
            put(t, v);
          } else {
            put(t, cp[LATE ? 0 : c + t]);
          }
        }
        flush((unsigned)(c0 + c));
      }
    }
  } else {
    if (g.ref_rows && g.write_ref) {
#pragma unroll
      for (int c = 0; c < G; ++c) store_row((unsigned)(c0 + c), cp[LATE ? 0 : c]);
    }
#pragma unroll
    for (int c = 0; c < G; ++c) {
      float v[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] = acc[c >> 2][j][c & 3];
      store_row((unsigned)(g.ref_rows + c0 + c), v);
    }
  }
}

// bf16 volumes at NJ = 2 (the default; round 6): 8 waves per SIMD instead of the 6 the allocator
// picks (76 -> 64 VGPRs, a 48-byte spill outside the fast path): the tap
// gathers' latency is what the extra waves hide -- the C3 sweep 0.363-0.368
// -> 0.351-0.355 ms in three alternating rounds on one box
// (profiles/r06_sweep_occupancy_ab.txt); fp32 kernels already run at 8.
template <typename OutT, int NQ, int NJ>
__global__ __launch_bounds__(kSwThreads) __attribute__((amdgpu_waves_per_eu(sizeof(OutT) == 2 && NJ == 2 ? 8 : 1)))
void k_sweep_tile(const float* __restrict__ ref,
                                                           const f32x4* __restrict__ tq,
                                                           const float* __restrict__ pose,
                                                           const float* __restrict__ K4,
                                                           const float* __restrict__ K4inv, FlatGeom g,
                                                           OutT* __restrict__ out, const Proj* __restrict__ projs) {
  constexpr int WIN = 256 * NJ;
  const unsigned item = blockIdx.x;            // grid = B * groups * nwin
  const unsigned r = magic_div(item, g.mwin);
  const int win = (int)(item - r * (unsigned)g.nwin);
  const int b = (int)magic_div(r, g.mgrp);
  const int k = (int)(r - (unsigned)b * (unsigned)g.groups);
  const size_t wbase = ((size_t)b * g.rows + g.ref_rows + k * 4 * NQ) * (size_t)g.slab;
  const int start = win * WIN - (int)((wbase + (size_t)g.out_mis) & (size_t)g.amask);
  if (start >= g.slab) return;
  if (g.buf_ok && start >= 0 && start + WIN <= g.slab && (k + 1) * 4 * NQ <= g.C)
  {
    if constexpr (NJ <= 16 / (int)sizeof(OutT)) {
      if (NJ == 8 || (g.store_px == NJ && !g.share)) {     // NJ = 8 is launched for wide stores only
        if (g.wpol == 16) sweep_tile_fast<OutT, NQ, NJ, false, false, true, 16>(ref, tq, projs, g, out, b, k, start);
        else if (g.wpol == 17) sweep_tile_fast<OutT, NQ, NJ, false, false, true, 17>(ref, tq, projs, g, out, b, k, start);
        else if (g.wpol == 18) sweep_tile_fast<OutT, NQ, NJ, false, false, true, 18>(ref, tq, projs, g, out, b, k, start);
        else if (g.store_nt) sweep_tile_fast<OutT, NQ, NJ, false, true, true>(ref, tq, projs, g, out, b, k, start);
        else sweep_tile_fast<OutT, NQ, NJ, false, false, true>(ref, tq, projs, g, out, b, k, start);
        return;
      }
    }
    if constexpr (NJ == 8) return;
    else if (g.store_nt) {
      if (g.share) sweep_tile_fast<OutT, NQ, NJ, true, true>(ref, tq, projs, g, out, b, k, start);
      else sweep_tile_fast<OutT, NQ, NJ, false, true>(ref, tq, projs, g, out, b, k, start);
    } else {
      if (g.share) sweep_tile_fast<OutT, NQ, NJ, true, false>(ref, tq, projs, g, out, b, k, start);
      else sweep_tile_fast<OutT, NQ, NJ, false, false>(ref, tq, projs, g, out, b, k, start);
    }
  }
  else if (start >= 0 && start + WIN <= g.slab)
    sweep_tile_item<OutT, NQ, NJ, true>(ref, tq, pose, K4, K4inv, g, out, b, k, start, wbase);
  else
    sweep_tile_item<OutT, NQ, NJ, false>(ref, tq, pose, K4, K4inv, g, out, b, k, start, wbase);
}

template <typename OutT, int NQ, int NJ>
static void launch_k_sweep_tile(const SweepPlan& p, const SweepOperands& op, const FlatGeom& g, hipStream_t s) {
  hipLaunchKernelGGL((k_sweep_tile<OutT, NQ, NJ>), dim3(p.blocks), dim3(kSwThreads), 0, s, op.ref, op.tq, op.pose,
                     op.K4, op.K4inv, g, (OutT*)op.out, op.projs);
}

// plan.nj is the instantiated window: fp32 1, 2, 4 pixels per lane, bf16 2, 4, 8
template <typename OutT, int NQ>
static void launch_k_sweep_tile_nj(const SweepPlan& p, const SweepOperands& op, const FlatGeom& g, hipStream_t s) {
  constexpr int S = sizeof(OutT) == 2 ? 2 : 1;   // bf16 windows pack register pairs
  if (p.nj == 4 * S) launch_k_sweep_tile<OutT, NQ, 4 * S>(p, op, g, s);
  else if (p.nj == 2 * S) launch_k_sweep_tile<OutT, NQ, 2 * S>(p, op, g, s);
  else launch_k_sweep_tile<OutT, NQ, S>(p, op, g, s);
}

int launch_sweep_tile(const SweepPlan& p, const SweepOperands& op, hipStream_t s) {
  FlatGeom g = p.flat;
  g.depths = p.depth_table ? op.depths : nullptr;
  with_out_type(p.out_dtype, [&](auto tag) {
    using OutT = decltype(tag);
    if (p.nq == 2) launch_k_sweep_tile_nj<OutT, 2>(p, op, g, s);
    else launch_k_sweep_tile_nj<OutT, 1>(p, op, g, s);
  });
  SFM_LAUNCHED();
  return SFM_OK;
}

int launch_sweep_flat(const SweepPlan& p, const SweepOperands& op, hipStream_t s) {
  const dim3 grid(p.blocks), block(kSwThreads);
  FlatGeom g = p.flat;
  g.depths = p.depth_table ? op.depths : nullptr;
  with_out_type(p.out_dtype, [&](auto tag) {
    using OutT = decltype(tag);
    if (p.nq == 2)
      hipLaunchKernelGGL((k_sweep_flat<OutT, 2>), grid, block, 0, s, op.ref, op.tq, op.pose, op.K4, op.K4inv, g,
                         (OutT*)op.out);
    else
      hipLaunchKernelGGL((k_sweep_flat<OutT, 1>), grid, block, 0, s, op.ref, op.tq, op.pose, op.K4, op.K4inv, g,
                         (OutT*)op.out);
  });
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace sfm
