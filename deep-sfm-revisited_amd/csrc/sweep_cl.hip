// Plane-sweep cost volume in the regulariser's channels-last layout:
// k_sweep_cl, k_sweep_cl_any and the sfm_plane_sweep_cl entries.
#include <algorithm>
#include "sweep_common.h"
#include "act_cvt.h"

namespace sfm {

// ---------------------------------------------------------------------------
// Cost volume, channels-last: out[b][l][p][0:C] = ref[b][:, p] and
// out[b][l][p][C:2C] = warp(tgt[b], plane l)[:, p], in the regulariser's
// activation type -- the tensor CostRegularization reads (PSNet.py:159), so
// the planar [B, 2C, L, h, w] volume and its transpose are never written.
//
// A (plane, pixel) record is 2C contiguous elements and a pair's records are
// contiguous in (l, p) order, so a wave takes 64 consecutive pixel-planes
// f = l * hw + p (it may straddle planes) and owns one contiguous run of
// 64 records.  One lane = one record: the sampling position and the four
// taps once for all channels, then per 16-byte chunk of the record (4 fp32 /
// 8 half channels) the reference loads (lane-consecutive pixels of a channel
// row) or the tap gathers of its channel quads.  Same arithmetic as
// k_sweep_tile (Proj table, plane_depth, sample_pos_nr, make_taps_inside, the
// mul + 3 FMA tap sum), so the fp32 values are the same bits, and the 16-bit
// types round them with the regulariser's own conversion (act_cvt.h).
//
// Stores: a lane that stored its own record chunk by chunk would put 16 bytes
// into each of 64 different lines per instruction.  The chunks go through a
// per-wave LDS stage instead (records padded by one chunk: the odd stride
// spreads the 64 lanes' 16-byte writes over all banks) and come back in
// address order, chunk 64 i + lane of the run, so every store instruction
// covers 1 KB of whole consecutive lines (measured at KITTI, one pair, f16:
// 0.19 ms against 0.43 ms for lanes storing their own records).
// Records are 16-byte aligned for any h * w.  The stores are buffer stores
// with a literal-0 soffset (the guarded form, see sweep_tile_fast's flush) and
// the sc1 policy: write-through, the lines are not kept in the XCD's L2, which
// the 0.5 - 1 GB volume would only sweep clean of the target quads every plane
// re-reads (0.168 ms against 0.193 plain and 0.172 sc0 nt; sc0 sc1 and nt sc1
// equal sc1 within the spread).
//
// Fast path: C % 4 == 0 (fp32) or C % 8 == 0 (16-bit), per-pair byte ranges
// below 2^32, h * w < 2^24, a record stage of at most 64 KB per wave.  Every
// other shape takes k_sweep_cl_any (one thread per record, element stores,
// 64-bit indices).
//
// Float16 features (F16 = true; sfm_plane_sweep_cl_f16): `ref` is the planar
// half tensor and the target comes as k_tgt_octets' records, so the warped
// half gathers 4 octets per 8 channels where the float32 form gathers 8 quads.
// Every half is widened to float32 (exact, subnormals included) before the
// unchanged tap sum and the unchanged rounding, so the volume is the one the
// float32 form writes for the widened features, bit for bit.  With a float32
// output an octet fills two record chunks.  Fast path: C % 8 == 0 for every
// output type, and the limits above.
// ---------------------------------------------------------------------------
#ifndef SFM_SWEEP_CL_POLICY
#define SFM_SWEEP_CL_POLICY 16   // cache policy of the record stores (0 plain, 3 sc0 nt, 16 sc1, 17 sc0 sc1, 18 nt sc1)
#endif

struct F16Out {};    // IEEE half / bfloat16 records, as raw 16-bit patterns
struct BF16Out {};
template <typename OutT> struct ClOut;
template <> struct ClOut<float> {
  using elem = float;
  static __device__ __forceinline__ float cvt(float f) { return f; }
};
template <> struct ClOut<F16Out> {
  using elem = unsigned short;
  static __device__ __forceinline__ unsigned short cvt(float f) { return ActCvt<true>::from_f(f); }
};
template <> struct ClOut<BF16Out> {
  using elem = unsigned short;
  static __device__ __forceinline__ unsigned short cvt(float f) { return ActCvt<false>::from_f(f); }
};

// the features' storage: float32 and channel quads, or IEEE half (raw 16-bit patterns) and channel octets
template <bool F16> struct ClFeat;
template <> struct ClFeat<false> {
  using elem = float;
  using rec = f32x4;
};
template <> struct ClFeat<true> {
  using elem = unsigned short;
  using rec = u32x4;
};

struct ClGeom {
  int B, C, C4, h, w, hw, L;   // C4: 16-byte target records per pixel (quads, or octets of float16 features)
  int R;                 // 16-byte chunks per record
  int slab;              // pixel-planes (records) per pair: L * hw < 2^31
  unsigned pair_bytes;   // one pair's records in bytes (fast path)
  Magic mhw, mR;
  float inv_w;
  float dmax, dstep;
};

// A tap sum as a float32 value of its own.  Without it the compiler may fuse the
// sum's last FMA with the conversion to half (v_fma_mixlo_f16, even with
// -ffp-contract=off), which rounds the exact sum once instead of rounding its
// float32 value: another result at half-way cases, one element in ~10^4.
__device__ __forceinline__ float cl_f32(float v) {
  asm("" : "+v"(v));
  return v;
}

// one record chunk: 4 fp32 or 8 16-bit channels
template <typename OutT>
__device__ __forceinline__ u32x4 cl_pack(const float* v) {
  using O = ClOut<OutT>;
  u32x4 x;
  if constexpr (sizeof(typename O::elem) == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = __float_as_uint(v[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = (unsigned)O::cvt(v[2 * e]) | ((unsigned)O::cvt(v[2 * e + 1]) << 16);
  }
  return x;
}

constexpr int kClThreads = 256;

template <typename OutT, int POL, bool F16 = false>
__global__ __launch_bounds__(kClThreads) void k_sweep_cl(const typename ClFeat<F16>::elem* __restrict__ ref,
                                                         const typename ClFeat<F16>::rec* __restrict__ tq,
                                                         const Proj* __restrict__ projs, ClGeom g,
                                                         typename ClOut<OutT>::elem* __restrict__ out) {
  using E = typename ClOut<OutT>::elem;
  constexpr unsigned FB = (unsigned)sizeof(typename ClFeat<F16>::elem);   // bytes per feature element
  constexpr int EPC = 16 / (int)sizeof(E);      // channels per chunk
  constexpr int QPC = EPC / 4;                  // channel quads per chunk
  extern __shared__ __attribute__((aligned(16))) u32x4 s_stage[];   // [waves][64][R + 1]
  const int b = (int)blockIdx.y;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int f0 = ((int)blockIdx.x * (int)(blockDim.x >> 6) + wave) * 64;   // the wave's first record
  if (f0 >= g.slab) return;
  const int npx = min(64, g.slab - f0);
  const int f = min(f0 + lane, g.slab - 1);     // lanes past the pair's end recompute its last record, never stored
  const int l = (int)magic_div((unsigned)f, g.mhw);
  const int p = f - l * g.hw;
  const Proj pr = projs[b];                     // uniform: scalar loads
  const SampleK sk = sample_consts(g.h, g.w);
  const float d = plane_depth(g.dmax, g.dstep, l);
  int y = (int)((float)p * g.inv_w);            // (x, y) = (p % w, p / w): reciprocal and one correction (p < 2^24)
  int x = p - y * g.w;
  if (x < 0) { --y; x += g.w; }
  if (x >= g.w) { ++y; x -= g.w; }
  const float xf = (float)x, yf = (float)y;
  float ray[3];
  ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
  ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
  ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
  float ix, iy;
  const bool in = sample_pos_nr(pr, ray, d, sk, ix, iy);
  TapsIn tp;
  if (in) make_taps_inside(ix, iy, g.h, g.w, tp);
  const __amdgpu_buffer_rsrc_t rref = buf_rsrc(ref + (size_t)b * g.C * g.hw, (unsigned)g.C * g.hw * FB);
  const __amdgpu_buffer_rsrc_t rtq = buf_rsrc(tq + (size_t)b * g.C4 * g.hw, (unsigned)g.C4 * g.hw * 16u);
  const __amdgpu_buffer_rsrc_t rout = buf_rsrc(out + (size_t)b * g.slab * 2 * g.C, g.pair_bytes);
  const int R = g.R, RH = R >> 1;               // the reference half and the warped half: RH chunks each
  u32x4* st = s_stage + ((size_t)wave * 64 + lane) * (R + 1);
  auto emit = [&](int k, const float* v) { st[k] = cl_pack<OutT>(v); };
  for (int k = 0; k < RH; ++k) {
    float v[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const unsigned so = (unsigned)(k * EPC + e) * g.hw * FB;
      if constexpr (F16)   // through float32 and cl_pack's cvt, like the warped half: one function defines the rounding
        v[e] = ActCvt<true>::to_f((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rref, (unsigned)p * 2u, so, 0));
      else
        v[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rref, (unsigned)p * 4u, so, 0));
    }
    emit(k, v);
  }
  if constexpr (F16) {
    constexpr int CPO = 8 / EPC;                // record chunks an octet fills: 1 (16-bit) or 2 (float32)
    for (int o = 0; o < RH / CPO; ++o) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.0f;    // an out-of-image sample: zero for every channel
      if (in) {
        const unsigned so = (unsigned)o * g.hw * 16u;
        u32x4 t[4];
#pragma unroll
        for (int n = 0; n < 4; ++n)
          t[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[n] * 16u, so, 0));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          auto tap = [&](int n) { return ActCvt<true>::to_f((unsigned short)(t[n][e >> 1] >> (16 * (e & 1)))); };
          float a = tp.wt[0] * tap(0);
          a = __builtin_fmaf(tp.wt[1], tap(1), a);
          a = __builtin_fmaf(tp.wt[2], tap(2), a);
          v[e] = cl_f32(__builtin_fmaf(tp.wt[3], tap(3), a));
        }
      }
#pragma unroll
      for (int c = 0; c < CPO; ++c) emit(RH + o * CPO + c, v + c * EPC);
    }
  } else {
    for (int k = 0; k < RH; ++k) {
      float v[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) v[e] = 0.0f;  // an out-of-image sample: zero for every channel
      if (in) {
#pragma unroll
        for (int q = 0; q < QPC; ++q) {
          const unsigned so = (unsigned)(k * QPC + q) * g.hw * 16u;
          f32x4 t[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            t[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rtq, tp.off[e] * 16u, so, 0));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float a = tp.wt[0] * t[0][e];
            a = __builtin_fmaf(tp.wt[1], t[1][e], a);
            a = __builtin_fmaf(tp.wt[2], t[2][e], a);
            v[4 * q + e] = cl_f32(__builtin_fmaf(tp.wt[3], t[3][e], a));
          }
        }
      }
      emit(RH + k, v);
    }
  }
  // the run in address order: chunk i of the run is chunk i % R of record i / R
  sweep_wave_sync();
  const u32x4* sw = s_stage + (size_t)wave * 64 * (R + 1);
  const unsigned run = (unsigned)f0 * R * 16u;
  for (int i = lane; i < npx * R; i += 64) {
    const int rec = (int)magic_div((unsigned)i, g.mR);
    const u32x4 c = sw[rec * (R + 1) + (i - rec * R)];
    __builtin_amdgcn_raw_buffer_store_b128(c, rout, run + (unsigned)i * 16u, 0, POL);
  }
}

// any shape: one thread per record, element by element
template <typename OutT, bool F16 = false>
__global__ __launch_bounds__(256) void k_sweep_cl_any(const typename ClFeat<F16>::elem* __restrict__ ref,
                                                      const typename ClFeat<F16>::rec* __restrict__ tq,
                                                      const Proj* __restrict__ projs, ClGeom g,
                                                      typename ClOut<OutT>::elem* __restrict__ out) {
  using O = ClOut<OutT>;
  using FE = typename ClFeat<F16>::elem;
  constexpr int CPR = 16 / (int)sizeof(FE);     // channels per target record: a quad or an octet
  auto widen = [](FE v) {
    if constexpr (F16) return ActCvt<true>::to_f(v);
    else return v;
  };
  const int64_t total = (int64_t)g.B * g.slab;
  const SampleK sk = sample_consts(g.h, g.w);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int b = (int)(t / g.slab);
    const int f = (int)(t - (int64_t)b * g.slab);
    const int l = f / g.hw, p = f - l * g.hw;
    const Proj pr = projs[b];
    const float d = plane_depth(g.dmax, g.dstep, l);
    const float xf = (float)(p % g.w), yf = (float)(p / g.w);
    float ray[3];
    ray[0] = (pr.ki[0] * xf + pr.ki[1] * yf) + pr.ki[2];
    ray[1] = (pr.ki[3] * xf + pr.ki[4] * yf) + pr.ki[5];
    ray[2] = (pr.ki[6] * xf + pr.ki[7] * yf) + pr.ki[8];
    float ix, iy;
    const bool in = sample_pos_nr(pr, ray, d, sk, ix, iy);
    TapsIn tp;
    if (in) make_taps_inside(ix, iy, g.h, g.w, tp);
    typename O::elem* rec = out + (size_t)t * 2 * g.C;
    for (int c = 0; c < g.C; ++c) rec[c] = O::cvt(widen(ref[((size_t)b * g.C + c) * g.hw + p]));
    for (int c = 0; c < g.C; ++c) {
      float a = 0.0f;
      if (in) {
        // channel c of the record layout: element c % CPR of tq[b][c / CPR][pixel]
        const FE* T = reinterpret_cast<const FE*>(tq + ((size_t)b * g.C4 + c / CPR) * g.hw) + c % CPR;
        a = tp.wt[0] * widen(T[(size_t)tp.off[0] * CPR]);
        a = __builtin_fmaf(tp.wt[1], widen(T[(size_t)tp.off[1] * CPR]), a);
        a = __builtin_fmaf(tp.wt[2], widen(T[(size_t)tp.off[2] * CPR]), a);
        a = cl_f32(__builtin_fmaf(tp.wt[3], widen(T[(size_t)tp.off[3] * CPR]), a));
      }
      rec[g.C + c] = O::cvt(a);
    }
  }
}

template <typename OutT, bool F16>
static int launch_k_sweep_cl(const typename ClFeat<F16>::elem* ref, const typename ClFeat<F16>::rec* tq,
                             const Proj* projs, const ClGeom& g, bool fast, void* out, hipStream_t s) {
  using E = typename ClOut<OutT>::elem;
  if (fast) {
    // the stage: 64 padded records per wave; as many waves per block as fit 40 KB (four blocks per CU)
    const size_t wave_lds = (size_t)64 * (g.R + 1) * 16;
    int waves = kClThreads / 64;
    while (waves > 1 && waves * wave_lds > 40 * 1024) waves >>= 1;
    const unsigned blocks = (unsigned)(((int64_t)g.slab + 64 * waves - 1) / (64 * waves));
    hipLaunchKernelGGL((k_sweep_cl<OutT, SFM_SWEEP_CL_POLICY, F16>), dim3(blocks, (unsigned)g.B),
                       dim3(64 * waves), waves * wave_lds, s, ref, tq, projs, g, (E*)out);
  } else {
    const int64_t total = (int64_t)g.B * g.slab;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 20);
    hipLaunchKernelGGL((k_sweep_cl_any<OutT, F16>), dim3(blocks), dim3(256), 0, s, ref, tq, projs, g, (E*)out);
  }
  SFM_LAUNCHED();
  set_last_sweep(fast ? "k_sweep_cl" : "k_sweep_cl_any");
  return SFM_OK;
}

// sfm_plane_sweep_cl (F16 = false) and sfm_plane_sweep_cl_f16: the same checks, workspace and geometry; the
// float16 form relays the target as octets, which fit the quads' region (ceil(C/8) records against ceil(C/4))
template <bool F16>
static int plane_sweep_cl(const typename ClFeat<F16>::elem* ref, const typename ClFeat<F16>::elem* tgt, int batch,
                          int channels, int h, int w, const float* pose, const float* K4, const float* K4inv,
                          int nlabel, float min_depth, int predict_by_depth, int out_dtype, void* out,
                          void* workspace, size_t workspace_bytes, hipStream_t s) {
  const int B = batch, C = channels, L = nlabel;
  const SweepArgs a{B, C, h, w, L, min_depth, predict_by_depth, out_dtype, true, true, (uintptr_t)out};
  if (int rc = check_sweep_args(SweepEntry::channels_last, ref && tgt && pose && K4 && K4inv && out && workspace, a))
    return rc;
  if (int rc = check_sweep_workspace(workspace, workspace_bytes, sweep_ws_bytes(B, C, h, w))) return rc;
  const int hw = h * w;
  const int esz = out_dtype == 0 ? 4 : 2;
  ClGeom g;
  g.B = B; g.C = C; g.C4 = F16 ? (C + 7) / 8 : (C + 3) / 4; g.h = h; g.w = w; g.hw = hw; g.L = L;
  g.slab = L * hw;
  g.dmax = min_depth * (float)L;   // disp2depth = ones * MIN_DEPTH * nlabel (fp32)
  g.dstep = predict_by_depth ? min_depth : 0.0f;
  g.inv_w = 1.0f / (float)w;
  g.mhw = make_magic((unsigned)hw);
  const int64_t rec_bytes = (int64_t)2 * C * esz, pair_bytes = rec_bytes * g.slab;
  // whole 16-byte chunks per record half; with float16 features whole octets as well
  const bool fast = C % (F16 ? 8 : 16 / esz) == 0 && rec_bytes / 16 <= 63 && hw < (1 << 24) &&
                    pair_bytes < ((int64_t)1 << 32) && (int64_t)g.C4 * hw * 16 < ((int64_t)1 << 32);
  g.R = fast ? (int)(rec_bytes / 16) : 0;
  g.mR = make_magic((unsigned)std::max(g.R, 1));
  g.pair_bytes = fast ? (unsigned)pair_bytes : 0u;
  auto* tq = (typename ClFeat<F16>::rec*)workspace;
  Proj* projs = reinterpret_cast<Proj*>((char*)workspace + sweep_quads_bytes(B, C, h, w));
  {
    ProfScope ps(F16 ? "sweep_tgt_octets" : "sweep_tgt_quads", s);
    if constexpr (F16)
      launch_tgt_octets(tgt, B, C, hw, tq, pose, K4, K4inv, projs, L, g.dmax, g.dstep, B, s);
    else
      launch_tgt_quads(tgt, B, C, hw, tq, pose, K4, K4inv, projs, L, g.dmax, g.dstep, nullptr, PsnetPrep{}, B, s);
  }
  SFM_LAUNCHED();
  ProfScope ps(F16 ? "plane_sweep_cl_f16" : "plane_sweep_cl", s);
  if (out_dtype == 0) return launch_k_sweep_cl<float, F16>(ref, tq, projs, g, fast, out, s);
  if (out_dtype == 1) return launch_k_sweep_cl<BF16Out, F16>(ref, tq, projs, g, fast, out, s);
  return launch_k_sweep_cl<F16Out, F16>(ref, tq, projs, g, fast, out, s);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_plane_sweep_cl(const float* ref, const float* tgt, int batch, int channels, int h, int w, const float* pose,
                       const float* K4, const float* K4inv, int nlabel, float min_depth, int predict_by_depth,
                       int out_dtype, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  return plane_sweep_cl<false>(ref, tgt, batch, channels, h, w, pose, K4, K4inv, nlabel, min_depth, predict_by_depth,
                               out_dtype, out, workspace, workspace_bytes, (hipStream_t)stream);
}

int sfm_plane_sweep_cl_f16(const void* ref, const void* tgt, int batch, int channels, int h, int w, const float* pose,
                           const float* K4, const float* K4inv, int nlabel, float min_depth, int predict_by_depth,
                           int out_dtype, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  return plane_sweep_cl<true>((const unsigned short*)ref, (const unsigned short*)tgt, batch, channels, h, w, pose, K4,
                              K4inv, nlabel, min_depth, predict_by_depth, out_dtype, out, workspace, workspace_bytes,
                              (hipStream_t)stream);
}

}  // extern "C"
