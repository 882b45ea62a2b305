// The plane sweep's host side: the argument checks of its entry points, its
// workspace layout, the kernel geometry structs, and the SweepPlan that says
// which kernel form a call launches and with which parameters
// (sweep_plan.cpp).  Host code only -- no device function, so the plan can be
// built and run by a host compiler on its own; the device helpers the sweep's
// translation units share are in sweep_common.h.
#pragma once
#include "common.h"

namespace sfm {

constexpr int kSwThreads = 256;
constexpr int kSwPix = 4;
constexpr int kSwWin = kSwThreads * kSwPix;   // k_sweep: pixels per work item
constexpr int kFlatWin = 1024;                // k_sweep_flat: elements per window
constexpr int kBandThreads = 1024;            // k_sweep_band: 16 waves, 4 wave groups x 4 waves over the tile
constexpr int kDepthTable = 1024;             // plane depths kept in the workspace for L <= this

// sfm_plane_sweep_psnet's inputs (PSNet.py:130-133 + RESCALE_DEPTH); the
// preparation itself is psnet_prep_pair (sweep.hip)
struct PsnetPrep {
  const void* pose;
  int pose_f64;
  const float* K;
  const float* Kinv;
  float t_scale;
  float* out;               // planar: B poses (12), then B K4 (9), then B K4inv (9)
};

// k_sweep (sweep_row.hip)
struct SweepGeom {
  int B, C, C4, h, w, L;
  int ref_rows;    // C (full volume) or 0 (warped half only)
  int rows;        // output rows per plane: ref_rows + C
  int groups;      // row groups per pair: ref_rows single rows + C4 quads
  int npw;         // pixel windows per row
  int shift_mode;  // 1: odd planes' windows shifted by 2 elements
  float dmax;      // MIN_DEPTH * L
  float dstep;     // > 0: PREDICT_BY_DEPTH planes d_i = (i + 1) * dstep
};

// k_sweep_flat and k_sweep_tile (sweep_tile.hip)
struct FlatGeom {
  int B, C, C4, h, w, L, hw;
  int ref_rows, rows;
  int G;           // channels per group (4 * NQ)
  int groups;      // ceil(C / G) per pair
  int slab;        // L * hw elements
  int nwin;        // windows per slab
  int amask;       // elements per 256 bytes - 1
  int out_mis;     // element offset of the output pointer modulo amask + 1
  int pair_ok;     // bf16: every row starts at an even element (4-byte pair stores)
  int buf_ok;      // k_sweep_tile fast path: per-pair volume, ref and quad ranges < 2^32 bytes, pair_ok
  int share;       // k_sweep_tile fast path: neighbour-lane tap sharing (tuning key sweep_share)
  int store_nt;    // k_sweep_tile fast path: non-temporal volume stores (tuning key sweep_store_nt)
  int write_ref;   // k_sweep_tile: write the reference rows too (0: the warped half only, the reference
                   // half comes from k_ref_planes, e.g. on a side stream beside RANSAC)
  int store_px;    // bf16 fast path: consecutive pixels per lane store (tuning key sweep_store_px; 0: pairs)
  unsigned pair_bytes;   // one pair's output volume in bytes (buffer range)
  Magic mwin, mgrp, mhw;
  float inv_w;
  float dmax, dstep;
  const float* depths;   // plane depths (k_tgt_quads), or null; set by the launcher (SweepPlan::depth_table)
  int wpol;        // 16-byte stores' cache policy when not -1 (16 sc1, 17 sc0 sc1, 18 nt sc1; sweep_store_wt)
};

// k_sweep_band (sweep_band.hip)
struct BandGeom {
  int C, C4, h, w, hw, L;
  int ref_rows, rows;
  int slab;        // L * hw elements
  int ntiles;      // tiles per plane: ceil((hw + A - 1) / WIN)
  int nruns;       // plane runs per quad: ceil(L / run)
  int run;         // planes per block
  int amask;       // A - 1, A = elements per 256 bytes
  int out_mis;     // element offset of the output pointer modulo A
  int hwmod;       // hw mod A
  int pair_ok;     // bf16: every row starts at an even element
  int cap_rows;    // band rows the LDS holds
  Magic mtile, mrun, mgrp;
  float inv_w, dmax, dstep;
};

// LDS bytes of one k_sweep_band block holding `rows` band rows of quads
inline size_t band_lds_bytes(int rows, int w, int nj) {
  return (size_t)rows * w * 16 + 4 * (size_t)(256 * nj + 128) * sizeof(float);   // band + ref tile
}

// Workspace: channel quads tq [B][C4][hw] float4 (16 bytes each), then the
// per-pair Proj table (21 floats each: sweep_common.h asserts the size), then
// the plane depths, then the sfm_plane_sweep_psnet operands.
inline size_t sweep_quads_bytes(int B, int C, int h, int w) {
  const int C4 = (C + 3) / 4;
  return (size_t)B * C4 * (size_t)h * w * 16;
}
constexpr size_t kProjBytes = 21 * sizeof(float);
inline size_t sweep_proj_bytes(int B) { return ((size_t)B * kProjBytes + 255) & ~(size_t)255; }
// sfm_plane_sweep_psnet: float32 pose, K4, K4inv per pair (12 + 9 + 9 floats)
inline size_t sweep_psnet_bytes(int B) { return ((size_t)B * 30 * sizeof(float) + 255) & ~(size_t)255; }
// what launch_sweep uses: quads, Proj table, plane depths
inline size_t sweep_core_bytes(int B, int C, int h, int w) {
  return sweep_quads_bytes(B, C, h, w) + sweep_proj_bytes(B) + kDepthTable * sizeof(float);
}
// the public size: the core plus the sfm_plane_sweep_psnet operands at its end
inline size_t sweep_ws_bytes(int B, int C, int h, int w) { return sweep_core_bytes(B, C, h, w) + sweep_psnet_bytes(B); }

// What a sweep call is asked for, as far as checks and dispatch depend on it.
struct SweepArgs {
  int B, C, h, w, L;
  float min_depth;
  int depth_mode;      // 0: inverse-depth planes, 1: PREDICT_BY_DEPTH
  int out_dtype;       // 0 float32, 1 bfloat16 (channels-last entries: 2 float16 as well)
  bool with_ref;       // the volume has reference rows (2C rows per plane)
  bool write_ref;      // ... and this call writes them (false: sfm_plane_sweep_psnet_warped_half)
  uintptr_t out;       // the output pointer's address: only its alignment is used
};

// The entry points differ in a few limits and in the wording of two messages.
enum class SweepEntry {
  planar,          // sfm_plane_sweep, _ex, _warped, and launch_sweep under the psnet entries
  psnet,           // sfm_plane_sweep_psnet, _psnet_warped_half: the grid limits are left to launch_sweep's
                   // own check, after the workspace; pose_dtype is checked
  channels_last    // sfm_plane_sweep_cl, _cl_f16
};

enum class SweepForm { row, flat, tile, band };

// Everything launch_sweep decides, decided once (make_sweep_plan).
struct SweepPlan {
  SweepForm form;
  const char* name;    // sfm_last_sweep(): "k_sweep", "k_sweep+vec", "k_sweep_flat", "k_sweep_tile",
                       // "k_sweep_tile+wide", "k_sweep_band"
  const char* scope;   // profiler scope: "plane_sweep" or "plane_sweep_warped"
  const char* error;   // why no form takes the call (SFM_ERR_ARG), else null
  // template parameters of the form's kernel
  int out_dtype;       // 0 float32, 1 bfloat16
  int nq;              // flat, tile: channel quads per item (1, 2)
  int nj;              // tile: pixels per lane (fp32 1, 2, 4; bf16 2, 4, 8); band: 1 fp32, 2 bf16
  int ipb;             // row: items per block (1, 2, 4, 8)
  bool vec;            // row: 16-byte row stores
  int lane_pixels;     // row: tuning key sweep_lane_pixels (0, 1, 2)
  unsigned blocks;     // grid size
  unsigned lds;        // dynamic LDS bytes (band)
  bool depth_table;    // L <= kDepthTable: the relayout writes the plane depths, the tile form reads them
  SweepGeom row;       // always filled: the relayout takes C4, dmax and dstep from it
  FlatGeom flat;       // form flat or tile; holds the resolved store policy (store_px, store_nt, wpol)
  BandGeom band;       // form band
};

#pragma GCC visibility push(hidden)
// The checks every sweep entry point makes before it touches the device, in
// the order the messages have always been reported in.  ptrs_ok: the entry's
// own set of required pointers.  pose_dtype: SweepEntry::psnet only.
int check_sweep_args(SweepEntry entry, bool ptrs_ok, const SweepArgs& a, int pose_dtype = 0);
int check_sweep_workspace(const void* ws, size_t ws_bytes, size_t need);
// Pure: no HIP call, no global state, writes *plan only.  SFM_OK, or
// SFM_ERR_ARG with plan->error set.
int make_sweep_plan(const SweepArgs& a, const Tuning& t, SweepPlan* plan);
#pragma GCC visibility pop

}  // namespace sfm
