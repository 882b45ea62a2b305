// Plane-sweep cost volume and inverse warp on CDNA4 (gfx950): the driver.
//
// Replaces the per-plane Python loop of models/PSNet.py:144-158 (L iterations
// of ~10 ATen launches: bmm, elementwise, grid_sample, two strided copies)
// with one launch that writes the whole [B, 2C, L, h, w] volume (plus a tiny
// channel-quad relayout of the target features).  HBM-write-bound.
//
// Here: the relayout kernels with the sweep's tables, launch_sweep (check the
// arguments, make the plan, relayout, launch the plan's form), k_inverse_warp
// and the planar entry points.  The kernel forms have a translation unit each
// (sweep_row.hip, sweep_tile.hip, sweep_band.hip; the reference half alone in
// sweep_ref.hip, the channels-last volume in sweep_cl.hip); which form a call
// takes is decided by make_sweep_plan (sweep_plan.cpp).
//
// Arithmetic: warp.h (the reference's float32 expression order).
#include <algorithm>
#include "sweep_common.h"

namespace sfm {

// The tensor preparation of PSNet.forward before its sweep loop, one thread per
// pair (run by k_tgt_quads, before that pair's Proj), in the reference's float32 operations (PSNet.py:130-133 and the
// RESCALE_DEPTH branch): P.float() (RNE from float64), translation * t_scale,
// K rows 0-1 / 4, K^-1[:2,:2] * 4.  Division by 4 and multiplication by 4
// are exact, and the conversion and the one multiply are correctly rounded,
// so the results equal the torch ops bit for bit.
//
// one pair's preparation into P[12], K4[9], Ki4[9] (registers), also stored
// to the workspace for the sweep kernels that read them from there
__device__ __forceinline__ void psnet_prep_pair(const PsnetPrep& q, int B, int b, float (&P)[12], float (&K4)[9],
                                                float (&Ki4)[9]) {
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    float v = q.pose_f64 ? (float)static_cast<const double*>(q.pose)[(size_t)b * 12 + e]
                         : static_cast<const float*>(q.pose)[(size_t)b * 12 + e];
    if (q.t_scale > 0.0f && (e & 3) == 3) v = v * q.t_scale;
    P[e] = v;
    q.out[(size_t)b * 12 + e] = v;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const float k = q.K[(size_t)b * 9 + e], ki = q.Kinv[(size_t)b * 9 + e];
    K4[e] = e < 6 ? k / 4.0f : k;
    Ki4[e] = (e == 0 || e == 1 || e == 3 || e == 4) ? ki * 4.0f : ki;
    q.out[(size_t)B * 12 + (size_t)b * 9 + e] = K4[e];
    q.out[(size_t)B * 21 + (size_t)b * 9 + e] = Ki4[e];
  }
}

// The uniform tables the relayout kernels write beside their copy, from the
// first record row of pair 0.  With `projs`, threads 0..B-1 write each pair's
// Proj (K.pose rows and K^-1, load_proj's float32 expression order), so the
// sweep's waves read it with scalar loads instead of each recomputing the
// uniform 3x3.3x4 product on the VALU (~80 instructions per wave item);
// threads 0..L-1 the plane depths (two IEEE divisions per wave item otherwise).
__device__ __forceinline__ void write_sweep_tables(int i, int B, const float* __restrict__ pose,
                                                   const float* __restrict__ K4, const float* __restrict__ K4inv,
                                                   Proj* __restrict__ projs, int L, float dmax, float dstep,
                                                   float* __restrict__ depths, const PsnetPrep& prep) {
  if (projs && i < B) {
    // sfm_plane_sweep_psnet: the pair's PSNet preparation first (the sweep's
    // other paths read it from the workspace), then its Proj from those values
    Proj pr;
    if (prep.out) {
      float P[12], Kq[9], Kqi[9];
      psnet_prep_pair(prep, B, i, P, Kq, Kqi);
      load_proj(P, Kq, Kqi, 0, pr);
    } else {
      load_proj(pose, K4, K4inv, i, pr);
    }
    projs[i] = pr;
  }
  if (depths && i < L) depths[i] = plane_depth(dmax, dstep, i);
}

// tgt [B][C][hw] -> tq [B][C4][hw] float4 (channels >= C are zero), and the
// sweep's tables (write_sweep_tables).
__global__ void k_tgt_quads(const float* __restrict__ tgt, int B, int C, int C4, int hw, f32x4* __restrict__ tq,
                            const float* __restrict__ pose, const float* __restrict__ K4,
                            const float* __restrict__ K4inv, Proj* __restrict__ projs, int L, float dmax,
                            float dstep, float* __restrict__ depths, PsnetPrep prep) {
  // grid (pixels, quads, pairs): no integer division per thread; the uniform
  // per-pair and per-plane tables from the first quad row of pair 0
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int q = (int)blockIdx.y, b = (int)blockIdx.z;
  if (q == 0 && b == 0) write_sweep_tables(i, B, pose, K4, K4inv, projs, L, dmax, dstep, depths, prep);
  if (i >= hw) return;
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * q + k;
    v[k] = c < C ? tgt[((size_t)b * C + c) * hw + i] : 0.0f;
  }
  tq[((size_t)b * C4 + q) * hw + i] = v;
}

// The same for float16 features, which stay float16: tgt [B][C][hw] IEEE half
// (raw 16-bit patterns) -> to [B][C8][hw] octets of eight halves, 16 bytes like
// a quad, so one gather brings eight channels of a tap (channels >= C are
// zero).  The tables are k_tgt_quads' (the sweep's geometry is the same bits).
__global__ void k_tgt_octets(const unsigned short* __restrict__ tgt, int B, int C, int C8, int hw,
                             u32x4* __restrict__ to, const float* __restrict__ pose, const float* __restrict__ K4,
                             const float* __restrict__ K4inv, Proj* __restrict__ projs, int L, float dmax,
                             float dstep, float* __restrict__ depths) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int o = (int)blockIdx.y, b = (int)blockIdx.z;
  if (o == 0 && b == 0) write_sweep_tables(i, B, pose, K4, K4inv, projs, L, dmax, dstep, depths, PsnetPrep{});
  if (i >= hw) return;
  u32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 8 * o + 2 * k;
    const unsigned lo = c < C ? tgt[((size_t)b * C + c) * hw + i] : 0u;
    const unsigned hi = c + 1 < C ? tgt[((size_t)b * C + c + 1) * hw + i] : 0u;
    v[k] = lo | (hi << 16);
  }
  to[((size_t)b * C8 + o) * hw + i] = v;
}

static dim3 quads_grid(int B, int C4, int hw, int extra) {
  return dim3((unsigned)((std::max(hw, extra) + 255) / 256), (unsigned)C4, (unsigned)B);
}

void launch_tgt_quads(const float* tgt, int B, int C, int hw, f32x4* tq, const float* pose, const float* K4,
                      const float* K4inv, Proj* projs, int L, float dmax, float dstep, float* depths,
                      const PsnetPrep& prep, int extra, hipStream_t s) {
  const int C4 = (C + 3) / 4;
  hipLaunchKernelGGL(k_tgt_quads, quads_grid(B, C4, hw, extra), dim3(256), 0, s, tgt, B, C, C4, hw, tq, pose, K4, K4inv,
                     projs, L, dmax, dstep, depths, prep);
}

void launch_tgt_octets(const unsigned short* tgt, int B, int C, int hw, u32x4* to, const float* pose, const float* K4,
                       const float* K4inv, Proj* projs, int L, float dmax, float dstep, int extra, hipStream_t s) {
  const int C8 = (C + 7) / 8;
  hipLaunchKernelGGL(k_tgt_octets, quads_grid(B, C8, hw, extra), dim3(256), 0, s, tgt, B, C, C8, hw, to, pose, K4, K4inv,
                     projs, L, dmax, dstep, (float*)nullptr);
}

void launch_channel_quads(const float* feat, int B, int C, int hw, f32x4* quads, hipStream_t s) {
  launch_tgt_quads(feat, B, C, hw, quads, nullptr, nullptr, nullptr, nullptr, 0, 0.0f, 0.0f, nullptr, PsnetPrep{}, 0, s);
}

// inverse_warp for an arbitrary depth map (models/inverse_warp.py:121-153)
__global__ __launch_bounds__(kSweepThreads) void k_inverse_warp(const float* __restrict__ feat, int C, int h, int w,
                                                                const float* __restrict__ depth,
                                                                const float* __restrict__ pose,
                                                                const float* __restrict__ K,
                                                                const float* __restrict__ Kinv,
                                                                float* __restrict__ out) {
  const int b = blockIdx.y;
  const int hw = h * w;
  const int p = blockIdx.x * kSweepThreads + threadIdx.x;
  if (p >= hw) return;
  Proj pr;
  load_proj(pose, K, Kinv, b, pr);
  const float x = (float)(p % w), y = (float)(p / w);
  float ray[3];
  ray[0] = (pr.ki[0] * x + pr.ki[1] * y) + pr.ki[2];
  ray[1] = (pr.ki[3] * x + pr.ki[4] * y) + pr.ki[5];
  ray[2] = (pr.ki[6] * x + pr.ki[7] * y) + pr.ki[8];
  float ix, iy;
  const bool ok = sample_pos(pr, ray, depth[(size_t)b * hw + p], h, w, ix, iy);
  Taps tp;
  if (ok) make_taps(ix, iy, h, w, tp);
  const float* F = feat + (size_t)b * C * hw;
  float* O = out + (size_t)b * C * hw + p;
  for (int c = 0; c < C; ++c) {
    const float* Fc = F + (size_t)c * hw;
    float acc = 0.0f;
    if (ok) {
      acc = tp.wt[0] * Fc[tp.off[0]];
      acc = acc + tp.wt[1] * Fc[tp.off[1]];
      acc = acc + tp.wt[2] * Fc[tp.off[2]];
      acc = acc + tp.wt[3] * Fc[tp.off[3]];
    }
    O[(size_t)c * hw] = acc;
  }
}

static thread_local const char* t_last_sweep = "";
void set_last_sweep(const char* name) { t_last_sweep = name; }

// ptrs_ok: the entry point's own set of required pointers
static int launch_sweep(const SweepArgs& a, bool ptrs_ok, const float* ref, const float* tgt, const float* pose,
                        const float* K4, const float* K4inv, void* out, void* ws, size_t ws_bytes, hipStream_t s,
                        const PsnetPrep& prep = PsnetPrep{}) {
  if (int rc = check_sweep_args(SweepEntry::planar, ptrs_ok, a)) return rc;
  if (int rc = check_sweep_workspace(ws, ws_bytes, sweep_core_bytes(a.B, a.C, a.h, a.w))) return rc;
  SweepPlan plan;
  if (int rc = make_sweep_plan(a, tuning(), &plan)) {
    set_error(plan.error);
    return rc;
  }
  SweepOperands op;
  op.ref = ref; op.pose = pose; op.K4 = K4; op.K4inv = K4inv; op.out = out;
  f32x4* tq = (f32x4*)ws;
  Proj* projs = reinterpret_cast<Proj*>((char*)ws + sweep_quads_bytes(a.B, a.C, a.h, a.w));
  float* depths = plan.depth_table ? reinterpret_cast<float*>((char*)projs + sweep_proj_bytes(a.B)) : nullptr;
  op.tq = tq; op.projs = projs; op.depths = depths;
  {
    ProfScope ps("sweep_tgt_quads", s);
    launch_tgt_quads(tgt, a.B, a.C, a.h * a.w, tq, pose, K4, K4inv, projs, a.L, plan.row.dmax, plan.row.dstep, depths,
                     prep, std::max(a.B, a.L), s);
  }
  SFM_LAUNCHED();
  ProfScope ps(plan.scope, s);
  int rc = SFM_OK;
  switch (plan.form) {
    case SweepForm::band: rc = launch_sweep_band(plan, op, s); break;
    case SweepForm::tile: rc = launch_sweep_tile(plan, op, s); break;
    case SweepForm::flat: rc = launch_sweep_flat(plan, op, s); break;
    case SweepForm::row: rc = launch_sweep_row(plan, op, s); break;
  }
  if (rc == SFM_OK) set_last_sweep(plan.name);
  return rc;
}

// sfm_plane_sweep_psnet (write_ref) and sfm_plane_sweep_psnet_warped_half: PSNet's
// raw pose and intrinsics, prepared inside the sweep's first kernel
// (k_tgt_quads, one thread per pair before its Proj), not by a launch of its
// own.  Every argument is checked here, under the entry's own rules, before
// launch_sweep checks again under the planar ones; the sweep's own scratch
// excludes the prep region at the workspace's end.
static int psnet_sweep(const SweepArgs& a, bool ptrs_ok, const float* ref, const float* tgt, const void* pose,
                       int pose_dtype, const float* K, const float* Kinv, float t_scale, void* cost, void* workspace,
                       size_t workspace_bytes, hipStream_t s) {
  if (int rc = check_sweep_args(SweepEntry::psnet, ptrs_ok, a, pose_dtype)) return rc;
  if (int rc = check_sweep_workspace(workspace, workspace_bytes, sweep_ws_bytes(a.B, a.C, a.h, a.w))) return rc;
  const size_t core = sweep_core_bytes(a.B, a.C, a.h, a.w);
  float* prep = reinterpret_cast<float*>((char*)workspace + core);
  return launch_sweep(a, true, ref, tgt, prep, prep + (size_t)a.B * 12, prep + (size_t)a.B * 21, cost, workspace, core,
                      s, PsnetPrep{pose, pose_dtype, K, Kinv, t_scale, prep});
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_plane_sweep_workspace_bytes(int batch, int channels, int h, int w) {
  if (batch < 1 || channels < 1 || h < 1 || w < 1) return 0;
  return sweep_ws_bytes(batch, channels, h, w);
}

int sfm_plane_sweep_ex(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                       const float* pose, const float* K4, const float* K4inv, int nlabel, float min_depth,
                       int depth_mode, int out_dtype, void* cost, void* workspace, size_t workspace_bytes,
                       void* stream) {
  const SweepArgs a{batch, channels, h, w, nlabel, min_depth, depth_mode, out_dtype, ref != nullptr, true,
                    (uintptr_t)cost};
  return launch_sweep(a, tgt && pose && K4 && K4inv && cost, ref, tgt, pose, K4, K4inv, cost, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int sfm_plane_sweep(const float* ref, const float* tgt, int batch, int channels, int h, int w, const float* pose,
                    const float* K4, const float* K4inv, int nlabel, float min_depth, int out_dtype, void* cost,
                    void* workspace, size_t workspace_bytes, void* stream) {
  const SweepArgs a{batch, channels, h, w, nlabel, min_depth, 0, out_dtype, true, true, (uintptr_t)cost};
  return launch_sweep(a, ref && tgt && pose && K4 && K4inv && cost, ref, tgt, pose, K4, K4inv, cost, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int sfm_plane_sweep_psnet(const float* ref, const float* tgt, int batch, int channels, int h, int w,
                          const void* pose, int pose_dtype, const float* K, const float* Kinv, float t_scale,
                          int nlabel, float min_depth, int depth_mode, int out_dtype, void* cost, void* workspace,
                          size_t workspace_bytes, void* stream) {
  const SweepArgs a{batch, channels, h, w, nlabel, min_depth, depth_mode, out_dtype, ref != nullptr, true,
                    (uintptr_t)cost};
  return psnet_sweep(a, tgt && pose && K && Kinv && cost && workspace, ref, tgt, pose, pose_dtype, K, Kinv, t_scale,
                     cost, workspace, workspace_bytes, (hipStream_t)stream);
}

int sfm_plane_sweep_psnet_warped_half(const float* ref, const float* tgt, int batch, int channels, int h, int w, const void* pose,
                                      int pose_dtype, const float* K, const float* Kinv, float t_scale, int nlabel,
                                      float min_depth, int depth_mode, int out_dtype, void* cost, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  // the full volume's geometry (2C rows per plane) with its reference rows
  // left to sfm_plane_sweep_ref_planes; windows off k_sweep_tile's fast path
  // (edges, partial channel groups) leave them alone as well
  const SweepArgs a{batch, channels, h, w, nlabel, min_depth, depth_mode, out_dtype, true, false, (uintptr_t)cost};
  return psnet_sweep(a, ref && tgt && pose && K && Kinv && cost && workspace, ref, tgt, pose, pose_dtype, K, Kinv,
                     t_scale, cost, workspace, workspace_bytes, (hipStream_t)stream);
}

int sfm_plane_sweep_warped(const float* tgt, int batch, int channels, int h, int w, const float* pose,
                           const float* K4, const float* K4inv, int nlabel, float min_depth, int out_dtype,
                           void* out, void* workspace, size_t workspace_bytes, void* stream) {
  const SweepArgs a{batch, channels, h, w, nlabel, min_depth, 0, out_dtype, false, true, (uintptr_t)out};
  return launch_sweep(a, tgt && pose && K4 && K4inv && out, nullptr, tgt, pose, K4, K4inv, out, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

const char* sfm_last_sweep(void) { return t_last_sweep; }

int sfm_inverse_warp(const float* feat, int batch, int channels, int h, int w, const float* depth,
                     const float* pose, const float* K, const float* Kinv, float* out, void* stream) {
  SFM_REQUIRE(feat && depth && pose && K && Kinv && out, "null pointer argument");
  SFM_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 1 && h >= 2 && w >= 2, "invalid warp shape");
  const int hw = h * w;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps("inverse_warp", s);
  hipLaunchKernelGGL(k_inverse_warp, dim3((hw + kSweepThreads - 1) / kSweepThreads, batch), dim3(kSweepThreads), 0,
                     s, feat, channels, h, w, depth, pose, K, Kinv, out);
  SFM_LAUNCHED();
  return SFM_OK;
}

}  // extern "C"
