// Internal helpers shared by the libsfm_hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "sfm_hip.h"

namespace sfm {

void set_error(const std::string& msg);

// Launch-shape tuning knobs (sfm_tune_set); read by the launchers.
struct Tuning {
  int solve_lanes = 16;          // active lanes per k_solve_front wave (1..16: LDS records)
  int solve_coop = 1;            // k_solve_front's reduction on DPP quads (4 lanes per hypothesis); 0: one lane
  int roots_lanes = 32;          // active lanes per k_roots wave (1..32: LDS stack columns)
  int roots_split = 1;           // 1: k_roots_split (per-wave task pool); 2: k_roots_split<4> (a block's 4 waves, slower); 0: k_roots
  int sweep_items_per_block = 4; // consecutive (row, plane, window) items per sweep block
  int sweep_lane_pixels = 0;     // 1: warped lanes own 4 consecutive pixels (16-byte stores)
  int sweep_flat = 2;            // 1: 256-byte-aligned slab windows (k_sweep_flat); 2: narrow windows (k_sweep_tile); 0: per-row
  int sweep_nj = 1;              // k_sweep_tile (sweep_flat = 2): pixels per lane, window 256 * nj (bf16: even)
  int sweep_group = 8;           // warped channels per k_sweep_flat item (4 or 8; 8 measured stable in the bench loop)
  int sweep_buffer = 1;          // k_sweep_tile: buffer-addressed fast path for interior full-group windows
  int sweep_share = 0;           // k_sweep_tile fast path: right-hand taps from the next lane's left-hand taps (DPP)
  int sweep_store_wt = -1;       // 16-byte sweep stores' cache policy: 0 by sweep_store_nt, 1 sc1, 2 sc0 sc1, 3 nt sc1;
                                 // -1 (default): fp32 volumes 3, bf16 by sweep_store_nt
  int sweep_store_px = -1;       // k_sweep_tile fast path: 16-byte lane stores via LDS, 1/2/4/8 pixels per lane; 0: plain; -1: bf16 2, fp32 1
  int sweep_store_nt = 2;        // k_sweep_tile fast path: volume stores with sc0 nt (streaming); 2: bf16 volumes and
                                 // fp32 volumes of slabs <= 6 MiB (measured by shape)
  int sweep_run = 16;            // k_sweep_band (sweep_flat = 3): planes per block
  int sweep_band_rows = 16;      // k_sweep_band: most target rows staged in LDS (further clipped to 80 KB)
  int score_blocks_per_cu = 32;  // persistent score grid
  int score_fp32 = 1;            // packed float32 pre-decision in the score kernel
  int score_prune = 1;           // exact bound pruning in k_score32 (PruneState)
  int score_mf = 2;              // split-f16 MFMA scoring (exact by bound): 2 = k_score_mf2 (span-major, default
                                 // when num_test == num_ransac_test), 1 = k_score_mf (item-major), 0 = off
  int score_mf_chunk2 = 0;       // the same for the pruned second launch (0: score_mf_chunk)
  int score_mf_prune = 880;      // k_score_mf2 count-bound pruning: the first launch's share of each pair's
                                 // spans in per mille (0: off; one launch); later pruning points per pair from
                                 // k_mf2_split (an empty middle launch when the pair's own point is not later)
  int score_mf_prune_margin = 10; // the pruning point: 1 - (inlier ratio) + margin, per mille (k_mf2_split)
  int score_mf_prune_upper = 1;   // pruning passes one-sided (upper-bound counts), the kept candidates rescored (round 6)
  int score_mf_exact_max = 256;   // with upper: kept candidates per pair counted in float64 (k_mf2_exact); more: MFMA
  int score_mf_chunk = 64;       // k_score_mf2: smallest unit range a block claims (32-candidate tiles of a span);
                                 // 64 measured ~1 % faster than 128 with pruning (profiles/r05_prune_ab.txt)
  int score_mf_blocks_per_cu = 1; // k_score_mf persistent grid (LDS: one block per CU)
  int score_interleave = 0;      // k_score32 items: pairs interleaved (1) or pair after pair (0)
  int score_precision = 64;      // 64: exact (reference float64 decisions); 32 / 16: ComputeError<float> /
                                 // <half> semantics (approximate inlier sets, BASELINE C5)
  int score_lowp_template = 0;   // 32 / 16: 0 = E and every operation held in T (this build's variant);
                                 // 1 = the literal ComputeError<T> with double Ematrix (double products)
  int conv_rolling = 1;          // 1: cin-32 conv layers roll along the planes (k_conv3r); 0: k_conv3
  int conv_planes = 0;           // k_conv3r planes per block: 4, 8, 16, 32; 0: by grid size (conv3_lp)
  int score_ref_rider = 1;       // the cost volume's reference half written by the one-sided scorer's first
                                 // launch (sfm_score_ref_job; score_mf2.h); 0: the sweep writes both halves
  int sweep_fused_cl = 1;        // read by the Python depth stage only (sfm_amd.regularize.fused_channels_last): 1: the
                                 // sweep writes the regulariser's channels-last input itself (sfm_plane_sweep_cl);
                                 // 0: planar volume, then sfm_to_channels_last_*
  int sweep_f16_feat = 1;        // read by the Python depth stage only (sfm_amd.regularize.sweep_regularize_fused,
                                 // sfm_amd.psnet): 1: float16 features go to the fused sweep as they come
                                 // (sfm_plane_sweep_cl_f16); 0: widened to float32 first (sfm_plane_sweep_cl)
  int conv_wgrad_blocks = 0;     // k_conv3_wgrad accumulating blocks (1..4096); 0: by tile count, at most 512
  int conv2_wgrad_blocks = 0;    // k_conv2_wgrad<NG, KS, STRIDE> (conv2_wgrad.hip) accumulating blocks, for both
                                 // 2-D weight-gradient entry points (1..4096); 0: by tile count, at most 512
  int bn_blocks = 0;             // k_bn3_stats / k_bn3_bwd_reduce reducing blocks (1..4096); 0: by voxel count, at most 512
};
Tuning& tuning();

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte (the entry points' aliasing checks); a null
// pointer, an optional operand left out, overlaps nothing
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// Uniform integer division by a host-made magic number (the sweep's window
// decode, the scorer's store rider).
struct Magic {   // floor(n / d) = (n * m) >> s for 0 <= n < 2^31
  unsigned m, s;
};
inline Magic make_magic(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  const unsigned long long two = 1ull << (31 + l);
  return Magic{(unsigned)((two + d - 1) / d), 31 + l};
}
__device__ __forceinline__ unsigned magic_div(unsigned n, Magic mg) {
  return (unsigned)(((unsigned long long)n * mg.m) >> mg.s);
}

// The reference half of a cost volume that a RANSAC call writes from inside
// its scorer (sfm_score_ref_job): ref [B*C][hw] float32 -> cost [B][2C][L][hw].
struct RefJob {
  const float* ref = nullptr;
  void* cost = nullptr;
  int batch = 0, channels = 0, nlabel = 0, h = 0, w = 0, dtype = 0;
};
// the job armed for stream s, if any, disarmed (score_sync.cpp)
bool take_ref_job(hipStream_t s, RefJob* job);
// Stream coordination right before a RANSAC call's scoring phase
// (score_sync.cpp): record the score fence when enabled; wait for (and
// consume) the score gate armed for stream s.
#pragma GCC visibility push(hidden)
int record_score_fence(hipStream_t s);
int wait_score_gate(hipStream_t s);
#pragma GCC visibility pop

// The score kernel the last RANSAC / score call dispatched (sfm_last_scorer):
// a static string literal.
void set_last_scorer(const char* name);
const char* last_scorer();

// Profiling hooks (capi.hip): record HIP events around a launch when enabled.
struct ProfScope {
  ProfScope(const char* name, hipStream_t s);
  ~ProfScope();
  int slot;
  hipStream_t stream;
};

}  // namespace sfm

#define SFM_REQUIRE(cond, msg)                 \
  do {                                         \
    if (!(cond)) {                             \
      ::sfm::set_error(msg);                   \
      return SFM_ERR_ARG;                      \
    }                                          \
  } while (0)

#define SFM_HIP(call)                                                             \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      ::sfm::set_error(std::string(#call) + ": " + hipGetErrorString(e_));        \
      return SFM_ERR_HIP;                                                         \
    }                                                                             \
  } while (0)

#define SFM_LAUNCHED()                                                            \
  do {                                                                            \
    hipError_t e_ = hipGetLastError();                                            \
    if (e_ != hipSuccess) {                                                       \
      ::sfm::set_error(std::string("kernel launch: ") + hipGetErrorString(e_));   \
      return SFM_ERR_HIP;                                                         \
    }                                                                             \
  } while (0)
