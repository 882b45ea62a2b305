// Device helpers shared by the plane sweep's translation units (one per kernel
// form: sweep_row.hip, sweep_tile.hip, sweep_band.hip, sweep_ref.hip,
// sweep_cl.hip, and the driver sweep.hip), and the host launchers that cross
// them.  No kernel is declared here: every kernel is instantiated in the one
// unit that defines it.
#pragma once
#include "warp.h"
#include "sweep_plan.h"

namespace sfm {

static_assert(sizeof(Proj) == kProjBytes && sizeof(f32x4) == 16, "the workspace layout of sweep_plan.h");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float plane_depth(float dmax, float dstep, int l) {
  // PSNet.py:150-153: depth planes (i+1)*MIN_DEPTH, or disp2depth / (i+1)
  return dstep > 0.0f ? (float)(l + 1) * dstep : dmax / (float)(l + 1);
}

__device__ __forceinline__ void store1(float* dst, float v) { *dst = v; }
__device__ __forceinline__ void store1(unsigned short* dst, float v) { *dst = to_bf16(v); }

// Bilinear taps of an in-image sample (sample_pos returned true): then
// ix in [0, w-1] and iy in [0, h-1] exactly (monotone rounding of
// ((xn + 1) / 2) (w - 1) with |xn| <= 1), so x0, y0 are valid and x1 = w
// (y1 = h) only when ix = w - 1 exactly, where its weight ix - x0 is +0: the
// taps and weights equal make_taps' (invalid taps there weigh 0), without
// the validity tests.  Addresses of such taps are clamped.
struct TapsIn {
  unsigned off[4];
  float wt[4];
};
__device__ __forceinline__ void make_taps_inside(float ix, float iy, int h, int w, TapsIn& t) {
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix;
  const float wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
  t.wt[0] = wx0 * wy0;
  t.wt[1] = wx1 * wy0;
  t.wt[2] = wx0 * wy1;
  t.wt[3] = wx1 * wy1;
  const unsigned o0 = (unsigned)__mul24(y0, w) + (unsigned)x0;
  const unsigned dx = x0 < w - 1 ? 1u : 0u, dy = y0 < h - 1 ? (unsigned)w : 0u;
  t.off[0] = o0;
  t.off[1] = o0 + dx;
  t.off[2] = o0 + dy;
  t.off[3] = o0 + dy + dx;
}

// base + a 32-bit byte offset: uniform base pointers stay in SGPRs and the
// accesses use the saddr + 32-bit voffset form (no 64-bit address VALU).
template <typename T>
__device__ __forceinline__ T* at_u32(T* base, unsigned byte_off) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off);
}
template <typename T>
__device__ __forceinline__ const T* at_u32(const T* base, unsigned byte_off) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// a wave's LDS stage handed between its lanes: the compiler keeps every
// memory access on its side (the "memory" clobber; wavefront-scope fences do
// not order plain accesses) and the LDS operations before it have completed
__device__ __forceinline__ void sweep_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ unsigned bf16_pair_swap(unsigned a, unsigned b, bool odd) {
  // a, b: this lane's bf16 of pixel registers 2s and 2s+1; returns the pair
  // (lo, hi) this lane stores: even lane (a_self, a_next), odd (b_prev, b_self)
  const unsigned send = odd ? a : b;
  const unsigned r = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  return odd ? (r | (b << 16)) : (a | (r << 16));
}

// A buffer resource over [base, base + bytes): one SGPR quad per tensor, the
// uniform part of an address in the resource or an SGPR soffset, the per-lane
// part in one 32-bit VGPR.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// The device pointers of a planar sweep launch.
struct SweepOperands {
  const float* ref;      // [B][C][hw], null without reference rows
  const f32x4* tq;       // channel quads (workspace)
  const float *pose, *K4, *K4inv;
  const Proj* projs;     // per-pair Proj table (workspace)
  const float* depths;   // plane depths (workspace), null for L > kDepthTable
  void* out;
};

// out_dtype -> the planar volume's element type, as a tag value: f(float) or
// f(unsigned short) (bfloat16 as raw 16-bit patterns)
template <typename F>
static void with_out_type(int out_dtype, F&& f) {
  if (out_dtype == 0) f(float{});
  else f((unsigned short)0);
}

#pragma GCC visibility push(hidden)
// One launcher per form; each switches on the plan's fields to the kernel
// instantiation and launches plan.blocks blocks of it.  SFM_OK or SFM_ERR_HIP.
int launch_sweep_row(const SweepPlan& plan, const SweepOperands& op, hipStream_t s);    // sweep_row.hip
int launch_sweep_flat(const SweepPlan& plan, const SweepOperands& op, hipStream_t s);   // sweep_tile.hip
int launch_sweep_tile(const SweepPlan& plan, const SweepOperands& op, hipStream_t s);   // sweep_tile.hip
int launch_sweep_band(const SweepPlan& plan, const SweepOperands& op, hipStream_t s);   // sweep_band.hip

// The relayouts with the sweep's tables beside them (sweep.hip).  tgt [B][C][hw]
// float32 -> channel quads, or IEEE half -> channel octets; projs, depths and
// prep.out may be null (write_sweep_tables).  `extra`: the most table entries
// a thread of the first row writes (B, L).
void launch_tgt_quads(const float* tgt, int B, int C, int hw, f32x4* tq, const float* pose, const float* K4,
                      const float* K4inv, Proj* projs, int L, float dmax, float dstep, float* depths,
                      const PsnetPrep& prep, int extra, hipStream_t s);
void launch_tgt_octets(const unsigned short* tgt, int B, int C, int hw, u32x4* to, const float* pose, const float* K4,
                       const float* K4inv, Proj* projs, int L, float dmax, float dstep, int extra, hipStream_t s);

// The form the last sweep call on this thread launched (sfm_last_sweep): a static string literal.
void set_last_sweep(const char* name);
#pragma GCC visibility pop

}  // namespace sfm
