// Plane-sweep cost volume, per-row form (tuning key sweep_flat = 0, and every
// shape outside the slab forms' range): k_sweep and its launcher.
#include "sweep_common.h"

namespace sfm {

// ---------------------------------------------------------------------------
// Cost volume: the output is produced in address order.
//
// The [B, 2C, L, h, w] volume is cut into work items of 1024 consecutive
// pixels (256 threads x 4, one 16-byte store per thread per row):
//   * reference rows c < C: one item = one row segment (pure copy)
//   * warped rows: one item = the same segment of a channel QUAD (4 rows),
//     so the sampling position, mask and bilinear taps of a pixel are computed
//     once for 4 channels and each tap is one 16-byte load from the
//     channel-quad layout tq[B][C4][h*w][4] of the target features.
// Items are enumerated in the volume's memory order (window fastest, then
// plane, then row / quad, then pair) and each block takes `ipb` consecutive
// items, so the resident blocks sweep one contiguous window of the volume.
// MI355X write bandwidth drops with the number of interleaved store streams
// (git-history scripts/probe_store_bw.hip: 1 stream 4.9 TB/s, 2 -> 4.5, 4 -> 4.0, many
// scattered row chunks -> 3.7): the copy half therefore runs as a single
// stream, the warped half as 4 (the price of sharing the taps; one row per
// item would need ~45 VALU ops and 5 vector loads per output element).
//
// 16-byte alignment: a row starts at element ((b*rows + r)*L + l)*h*w.  With
// h*w = 2 (mod 4) and L even, that is 2*(l & 1) (mod 4) for every row of the
// plane, so the pixel windows of odd planes are shifted by 2.  Other shapes
// take the element-wise store path (correct, slower).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void store4(float* dst, const float (&v)[4]) {
  *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ void store4(unsigned short* dst, const float (&v)[4]) {
  u32x2 u;
  u[0] = (unsigned int)to_bf16(v[0]) | ((unsigned int)to_bf16(v[1]) << 16);
  u[1] = (unsigned int)to_bf16(v[2]) | ((unsigned int)to_bf16(v[3]) << 16);
  *reinterpret_cast<u32x2*>(dst) = u;
}

// VEC: rows are 16-byte aligned at the (shifted) window starts (see above)
template <typename OutT, bool VEC>
__device__ __forceinline__ void store_row(OutT* row, int p0, int hw, const float (&v)[4]) {
  if (VEC && p0 >= 0 && p0 + 3 < hw) {
    store4(row + p0, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p0 + j >= 0 && p0 + j < hw) store1(row + p0 + j, v[j]);
  }
}

template <typename OutT> __device__ __forceinline__ void store1_nt(OutT* dst, float v);
template <> __device__ __forceinline__ void store1_nt<float>(float* dst, float v) { __builtin_nontemporal_store(v, dst); }
template <> __device__ __forceinline__ void store1_nt<unsigned short>(unsigned short* dst, float v) {
  __builtin_nontemporal_store(to_bf16(v), dst);
}

// one warped item: 4 channels of the window at plane l
template <typename OutT, bool VEC, bool LANE_PIX, bool NT = false>
__device__ __forceinline__ void warp_quad(const f32x4* __restrict__ tq, const float* __restrict__ pose,
                                          const float* __restrict__ K4, const float* __restrict__ K4inv,
                                          const SweepGeom& g, int b, int q, int l, int p0, OutT* plane,
                                          size_t rstride) {
  const int hw = g.h * g.w;
  Proj pr;
  load_proj(pose, K4, K4inv, b, pr);
  // PSNet.py:150-153: depth planes (i+1)*MIN_DEPTH, or disp2depth / (i+1)
  const float d = g.dstep > 0.0f ? (float)(l + 1) * g.dstep : g.dmax / (float)(l + 1);
  const f32x4* T = tq + ((size_t)b * g.C4 + q) * hw;
  f32x4 acc[4];
  // LANE_PIX: pixel j of this lane is p0 + j (one 16-byte store per row);
  // otherwise the window's pixels are lane-consecutive (w0 + 64 j + lane, with
  // w0 = the wave's 256-pixel span), so each gather instruction reads
  // neighbouring source pixels, at the price of 4-byte stores.
  const int wave_base = p0 - 4 * (int)(threadIdx.x & 63);
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pj = LANE_PIX ? p0 + j : wave_base + 64 * j + lane;
    const int p = min(max(pj, 0), hw - 1);
    const float x = (float)(p % g.w), y = (float)(p / g.w);
    float ray[3];
    ray[0] = (pr.ki[0] * x + pr.ki[1] * y) + pr.ki[2];
    ray[1] = (pr.ki[3] * x + pr.ki[4] * y) + pr.ki[5];
    ray[2] = (pr.ki[6] * x + pr.ki[7] * y) + pr.ki[8];
    float ix, iy;
    acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (sample_pos(pr, ray, d, g.h, g.w, ix, iy)) {
      Taps tp;
      make_taps(ix, iy, g.h, g.w, tp);
      const f32x4 t0 = T[tp.off[0]], t1 = T[tp.off[1]], t2 = T[tp.off[2]], t3 = T[tp.off[3]];
      f32x4 a = tp.wt[0] * t0;
      a = a + tp.wt[1] * t1;
      a = a + tp.wt[2] * t2;
      a = a + tp.wt[3] * t3;
      acc[j] = a;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * q + k;
    if (c >= g.C) break;
    OutT* row = plane + (size_t)(g.ref_rows + c) * rstride;
    if (LANE_PIX) {
      const float v[4] = {acc[0][k], acc[1][k], acc[2][k], acc[3][k]};
      store_row<OutT, VEC>(row, p0, hw, v);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pj = wave_base + 64 * j + lane;
        if (pj >= 0 && pj < hw) {
          if (NT) store1_nt(row + pj, acc[j][k]);
          else store1(row + pj, acc[j][k]);
        }
      }
    }
  }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 4 reference pixels p0..p0+3 of a row starting at element `row_off` of `ref`.
// Even-aligned interior windows use two 8-byte loads (4 scalar loads per
// thread cap the copy at ~3.6 TB/s on MI355X: the address unit, not HBM, is
// the limit); edges and odd alignments load element-wise with clamping.
__device__ __forceinline__ void load_ref4(const float* __restrict__ ref, size_t row_off, int p0, int hw,
                                          float (&v)[4]) {
  if (p0 >= 0 && p0 + 3 < hw && ((row_off + (size_t)p0) & 1) == 0) {
    const f32x2 a = *reinterpret_cast<const f32x2*>(ref + row_off + p0);
    const f32x2 b = *reinterpret_cast<const f32x2*>(ref + row_off + p0 + 2);
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ref[row_off + min(max(p0 + j, 0), hw - 1)];
  }
}

struct ItemPos {
  int pw, l, grp, b;
  __device__ __forceinline__ void decode(int item, const SweepGeom& g) {
    pw = item % g.npw;
    int r = item / g.npw;
    l = r % g.L;
    r /= g.L;
    grp = r % g.groups;
    b = r / g.groups;
  }
  __device__ __forceinline__ void next(const SweepGeom& g) {
    if (++pw == g.npw) {
      pw = 0;
      if (++l == g.L) {
        l = 0;
        if (++grp == g.groups) { grp = 0; ++b; }
      }
    }
  }
};

template <typename OutT, bool VEC, int IPB, bool LANE_PIX = true, bool NT = false>
__global__ __launch_bounds__(kSwThreads) void k_sweep(const float* __restrict__ ref, const f32x4* __restrict__ tq,
                                                      const float* __restrict__ pose, const float* __restrict__ K4,
                                                      const float* __restrict__ K4inv, SweepGeom g,
                                                      OutT* __restrict__ out) {
  const int hw = g.h * g.w;
  const int total = g.B * g.groups * g.L * g.npw;   // < 2^31 (checked by the launcher)
  const int first = blockIdx.x * IPB;
  if (first >= total) return;
  const size_t rstride = (size_t)g.L * hw;
  ItemPos ip;
  ip.decode(first, g);
  ItemPos last;
  last.decode(min(first + IPB, total) - 1, g);
  if (first + IPB <= total && last.b == ip.b && last.grp < g.ref_rows) {
    // copy block: every item is a reference row of pair b.  Issue all loads
    // first (IPB x 16 bytes in flight per thread), then the stores.
    float v[IPB][4];
    int p0s[IPB];
    OutT* dst[IPB];
#pragma unroll
    for (int it = 0; it < IPB; ++it) {
      const int shift = g.shift_mode ? 2 * (ip.l & 1) : 0;
      const int p0 = ip.pw * kSwWin - shift + (int)threadIdx.x * kSwPix;
      p0s[it] = p0;
      dst[it] = out + (((size_t)ip.b * g.rows + ip.grp) * g.L + ip.l) * hw;
      load_ref4(ref, ((size_t)ip.b * g.C + ip.grp) * hw, p0, hw, v[it]);
      ip.next(g);
    }
#pragma unroll
    for (int it = 0; it < IPB; ++it)
      if (p0s[it] < hw) store_row<OutT, VEC>(dst[it], p0s[it], hw, v[it]);
    return;
  }
  for (int it = 0, item = first; it < IPB && item < total; ++it, ++item, ip.next(g)) {
    const int shift = g.shift_mode ? 2 * (ip.l & 1) : 0;
    const int p0 = ip.pw * kSwWin - shift + (int)threadIdx.x * kSwPix;
    OutT* plane = out + ((size_t)ip.b * g.rows * g.L + ip.l) * hw;   // row c at plane + c * rstride
    if (ip.grp < g.ref_rows) {
      if (p0 >= hw) continue;
      float v[4];
      load_ref4(ref, ((size_t)ip.b * g.C + ip.grp) * hw, p0, hw, v);
      store_row<OutT, VEC>(plane + (size_t)ip.grp * rstride, p0, hw, v);
    } else {
      warp_quad<OutT, VEC, LANE_PIX, NT>(tq, pose, K4, K4inv, g, ip.b, ip.grp - g.ref_rows, ip.l, p0, plane, rstride);
    }
  }
}

template <typename OutT, bool VEC, bool LP, bool NT>
static void launch_k_sweep(const SweepPlan& p, const SweepOperands& op, hipStream_t s) {
  const dim3 grid(p.blocks), block(kSwThreads);
  OutT* out = (OutT*)op.out;
  switch (p.ipb) {
    case 1: hipLaunchKernelGGL((k_sweep<OutT, VEC, 1, LP, NT>), grid, block, 0, s, op.ref, op.tq, op.pose, op.K4, op.K4inv, p.row, out); break;
    case 2: hipLaunchKernelGGL((k_sweep<OutT, VEC, 2, LP, NT>), grid, block, 0, s, op.ref, op.tq, op.pose, op.K4, op.K4inv, p.row, out); break;
    case 4: hipLaunchKernelGGL((k_sweep<OutT, VEC, 4, LP, NT>), grid, block, 0, s, op.ref, op.tq, op.pose, op.K4, op.K4inv, p.row, out); break;
    default: hipLaunchKernelGGL((k_sweep<OutT, VEC, 8, LP, NT>), grid, block, 0, s, op.ref, op.tq, op.pose, op.K4, op.K4inv, p.row, out);
  }
}

// sweep_lane_pixels: 0 lane-consecutive pixels (default), 1 four pixels per
// lane (16-byte stores), 2 lane-consecutive with non-temporal stores
template <typename OutT, bool VEC>
static void launch_k_sweep_mode(const SweepPlan& p, const SweepOperands& op, hipStream_t s) {
  if (p.lane_pixels == 1) launch_k_sweep<OutT, VEC, true, false>(p, op, s);
  else if (p.lane_pixels == 2) launch_k_sweep<OutT, VEC, false, true>(p, op, s);
  else launch_k_sweep<OutT, VEC, false, false>(p, op, s);
}

int launch_sweep_row(const SweepPlan& p, const SweepOperands& op, hipStream_t s) {
  with_out_type(p.out_dtype, [&](auto tag) {
    using OutT = decltype(tag);
    if (p.vec) launch_k_sweep_mode<OutT, true>(p, op, s);
    else launch_k_sweep_mode<OutT, false>(p, op, s);
  });
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // namespace sfm
