// The plane sweep's argument checks and its launch plan (host code only).
#include <algorithm>
#include <string>
#include "sweep_plan.h"

namespace sfm {

int check_sweep_args(SweepEntry entry, bool ptrs_ok, const SweepArgs& a, int pose_dtype) {
  const bool cl = entry == SweepEntry::channels_last;
  SFM_REQUIRE(ptrs_ok, "null pointer argument");
  const bool lower = a.B >= 1 && a.C >= 1 && a.h >= 2 && a.w >= 2;
  if (entry == SweepEntry::psnet) {
    SFM_REQUIRE(lower, "invalid sweep shape");
    SFM_REQUIRE(pose_dtype == 0 || pose_dtype == 1, "pose_dtype must be 0 (float32) or 1 (float64)");
    SFM_REQUIRE(a.L >= 1, "invalid sweep shape");
  } else {
    // the relayout's grid: quads (records) in y, pairs in z; channels-last:
    // make_taps_inside multiplies 24-bit row offsets
    SFM_REQUIRE(lower && a.B <= 65535 && a.C <= 4 * 65535 && (!cl || (a.h < (1 << 23) && a.w < (1 << 23))) && a.L >= 1,
                "invalid sweep shape");
  }
  if (cl) {
    SFM_REQUIRE(a.out_dtype >= 0 && a.out_dtype <= 2, "out_dtype must be 0 (float32), 1 (bfloat16) or 2 (float16)");
    SFM_REQUIRE(a.depth_mode == 0 || a.depth_mode == 1, "predict_by_depth must be 0 (inverse depth) or 1 (depth)");
  } else {
    SFM_REQUIRE(a.out_dtype == 0 || a.out_dtype == 1, "out_dtype must be 0 (float32) or 1 (bfloat16)");
    SFM_REQUIRE(a.depth_mode == 0 || a.depth_mode == 1, "depth_mode must be 0 (inverse depth) or 1 (depth)");
  }
  SFM_REQUIRE(a.min_depth > 0.0f, "min_depth must be positive");
  SFM_REQUIRE((int64_t)a.h * a.w < ((int64_t)1 << 30), "feature map too large");
  if (cl) {
    SFM_REQUIRE((int64_t)a.L * a.h * a.w < ((int64_t)1 << 31), "sweep too large: nlabel * h * w must be below 2^31");
    SFM_REQUIRE(a.out % 16 == 0, "out must be 16-byte aligned");
  }
  return SFM_OK;
}

int check_sweep_workspace(const void* ws, size_t ws_bytes, size_t need) {
  if (!ws || ws_bytes < need) {
    set_error("plane sweep workspace too small: need " + std::to_string(need) + " bytes");
    return SFM_ERR_WORKSPACE;
  }
  return SFM_OK;
}

// The aligned-slab forms' range: int slab offsets, 24-bit pixel indices (the
// float reciprocal that splits a pixel into x and y), 31-bit magic-number decode.
static bool slab_range(int hw, int64_t slab) { return hw < (1 << 24) && slab < ((int64_t)1 << 30); }

static bool plan_band(const SweepArgs& a, const Tuning& t, SweepPlan* p) {
  const int hw = a.h * a.w, esz = a.out_dtype == 0 ? 4 : 2;
  const int64_t slab = (int64_t)a.L * hw;
  const int bnj = a.out_dtype == 1 ? 2 : 1;
  BandGeom& bg = p->band;
  bg.C = a.C; bg.C4 = p->row.C4; bg.h = a.h; bg.w = a.w; bg.hw = hw; bg.L = a.L;
  bg.ref_rows = p->row.ref_rows; bg.rows = p->row.rows; bg.slab = (int)slab;
  bg.amask = 256 / esz - 1;
  bg.ntiles = (hw + bg.amask + 256 * bnj - 1) / (256 * bnj);
  bg.run = std::min(t.sweep_run, a.L);
  bg.nruns = (a.L + bg.run - 1) / bg.run;
  bg.out_mis = (int)((a.out / esz) & (uintptr_t)bg.amask);
  bg.hwmod = hw & bg.amask;
  bg.pair_ok = (slab % 2 == 0) && (a.out % 4 == 0);
  // two blocks per CU: <= 80 KB of LDS each
  const size_t lds_cap = 80 * 1024 - 64;
  const size_t row_bytes = (size_t)a.w * 16;
  const size_t fixed = band_lds_bytes(0, a.w, bnj);
  const int rows_fit = lds_cap > fixed ? (int)((lds_cap - fixed) / row_bytes) : 0;
  bg.cap_rows = std::min(std::min(t.sweep_band_rows, rows_fit), a.h);
  const int64_t nblk = (int64_t)a.B * bg.C4 * bg.nruns * bg.ntiles;
  // a band of one row holds no pixel's four taps; the block index is decoded with 31-bit magic numbers
  if (bg.cap_rows < 2 || nblk >= ((int64_t)1 << 31)) return false;
  bg.mtile = make_magic((unsigned)bg.ntiles);
  bg.mrun = make_magic((unsigned)bg.nruns);
  bg.mgrp = make_magic((unsigned)bg.C4);
  bg.inv_w = 1.0f / (float)a.w;
  bg.dmax = p->row.dmax; bg.dstep = p->row.dstep;
  p->form = SweepForm::band;
  p->name = "k_sweep_band";
  p->nj = bnj;
  p->blocks = (unsigned)nblk;
  p->lds = (unsigned)band_lds_bytes(bg.cap_rows, a.w, bnj);
  return true;
}

// tile (mode 2) or flat (mode 1, and mode 3 when the band did not take the call)
static bool plan_slab_windows(const SweepArgs& a, const Tuning& t, int mode, int nj, int store_px, SweepPlan* p) {
  const int hw = a.h * a.w, esz = a.out_dtype == 0 ? 4 : 2;
  const int64_t slab = (int64_t)a.L * hw;
  const int nq = p->nq;
  const int fgroups = (a.C + 4 * nq - 1) / (4 * nq);
  const int64_t win_el = mode == 2 ? 256 * (int64_t)nj : kFlatWin;
  const int64_t nwin = (slab + 127 + win_el - 1) / win_el;
  // the block index is decoded with 31-bit magic numbers
  if ((int64_t)a.B * fgroups * nwin >= ((int64_t)1 << 31)) return false;
  FlatGeom& fg = p->flat;
  fg.B = a.B; fg.C = a.C; fg.C4 = p->row.C4; fg.h = a.h; fg.w = a.w; fg.L = a.L; fg.hw = hw;
  fg.ref_rows = p->row.ref_rows; fg.rows = p->row.rows; fg.G = 4 * nq; fg.groups = fgroups;
  fg.slab = (int)slab; fg.nwin = (int)nwin;
  fg.amask = 256 / esz - 1;
  fg.out_mis = (int)((a.out / esz) & (uintptr_t)fg.amask);
  fg.pair_ok = (slab % 2 == 0) && (a.out % 4 == 0);
  const int64_t pair_bytes = (int64_t)fg.rows * slab * esz;
  fg.buf_ok = pair_bytes < ((int64_t)1 << 32) && (a.out_dtype == 0 || fg.pair_ok) && t.sweep_buffer;
  fg.share = t.sweep_share;
  // auto (2): bf16 volumes always; fp32 volumes when a channel slab (L x h x w
  // floats) is at most 6 MiB.  Measured, not derived (profiles/r05_sweep_store_shapes.txt):
  // non-temporal fp32 stores are faster at 120x160 L=64 (the indoor c4 volume:
  // 0.73 vs 0.69 of HBM inside the bench step), 120x161 L=64, and equal at
  // 128x128 L=64 (slabs 4.2-4.9 MiB), slower at every slab of 7.5 MiB or more
  // (KITTI 94x311 at L = 64 and 128, 120x160 L=128, 100x300 L=64, 96x320)
  fg.store_nt = t.sweep_store_nt == 2 ? (a.out_dtype != 0 || slab * 4 <= ((int64_t)6 << 20)) : t.sweep_store_nt;
  fg.write_ref = a.write_ref ? 1 : 0;
  fg.store_px = store_px;
  fg.pair_bytes = fg.buf_ok ? (unsigned)pair_bytes : 0u;
  fg.mwin = make_magic((unsigned)nwin);
  fg.mgrp = make_magic((unsigned)fgroups);
  fg.mhw = make_magic((unsigned)hw);
  fg.inv_w = 1.0f / (float)a.w;
  fg.dmax = p->row.dmax; fg.dstep = p->row.dstep;
  fg.depths = nullptr;
  // auto (-1): fp32 volumes nt sc1 (write-through: the volume's lines do
  // not stay in the XCD's L2, where plain / nt stores keep them), bf16 by
  // sweep_store_nt.  Measured (profiles/r05_sweep_store_wt.txt): inside the
  // bench step the fp32 sweep 1.275 -> 1.245 ms (c2) and 0.440 -> 0.422 ms
  // (c4); bf16 slower with sc1 (0.359 -> 0.384 ms, c3)
  int wt = t.sweep_store_wt;
  if (wt < 0) wt = a.out_dtype == 0 ? 3 : 0;
  fg.wpol = wt == 1 ? 16 : wt == 2 ? 17 : wt == 3 ? 18 : -1;
  p->blocks = (unsigned)((int64_t)a.B * fgroups * nwin);
  if (mode != 2) {
    p->form = SweepForm::flat;
    p->name = "k_sweep_flat";
    return true;
  }
  p->form = SweepForm::tile;
  // the instantiated window: fp32 1, 2 or 4 pixels per lane, bf16 2, 4 or 8 (register pairs)
  if (a.out_dtype == 1) p->nj = nj >= 8 ? 8 : nj >= 4 ? 4 : 2;
  else p->nj = nj >= 4 ? 4 : nj == 2 ? 2 : 1;
  // what the kernel's interior full-group windows take (k_sweep_tile): 16-byte stores via LDS, or plain ones
  const bool wide = fg.buf_ok && (p->nj == 8 || (fg.store_px == p->nj && !fg.share));
  p->name = wide ? "k_sweep_tile+wide" : "k_sweep_tile";
  return true;
}

int make_sweep_plan(const SweepArgs& a, const Tuning& t, SweepPlan* p) {
  *p = SweepPlan{};
  const int hw = a.h * a.w;
  p->scope = a.with_ref ? "plane_sweep" : "plane_sweep_warped";
  p->depth_table = a.L <= kDepthTable;
  p->out_dtype = a.out_dtype;

  // The per-row geometry, whatever the form: its item count bounds every call.
  SweepGeom& g = p->row;
  g.B = a.B; g.C = a.C; g.C4 = (a.C + 3) / 4; g.h = a.h; g.w = a.w; g.L = a.L;
  g.ref_rows = a.with_ref ? a.C : 0;
  g.rows = g.ref_rows + a.C;
  g.groups = g.ref_rows + g.C4;
  g.npw = (hw + 3 + kSwWin - 1) / kSwWin;
  // 16-byte row alignment (see k_sweep): every row aligned if hw % 4 == 0; rows of
  // plane l shifted by 2*(l&1) if hw % 4 == 2 and L even; element stores otherwise
  g.shift_mode = (hw % 4 == 2 && a.L % 2 == 0) ? 1 : 0;
  g.dmax = a.min_depth * (float)a.L;   // disp2depth = ones * MIN_DEPTH * nlabel (fp32)
  g.dstep = a.depth_mode ? a.min_depth : 0.0f;
  p->vec = (hw % 4 == 0) || g.shift_mode;
  p->ipb = t.sweep_items_per_block >= 8 ? 8 : t.sweep_items_per_block >= 4 ? 4 : t.sweep_items_per_block >= 2 ? 2 : 1;
  p->lane_pixels = t.sweep_lane_pixels;
  const int64_t items = (int64_t)a.B * g.groups * a.L * g.npw;
  if (items >= ((int64_t)1 << 31)) {
    p->error = "sweep too large for one launch";
    return SFM_ERR_ARG;
  }

  p->nq = t.sweep_group == 8 ? 2 : 1;
  const int64_t slab = (int64_t)a.L * hw;
  // The warped half alone (write_ref = 0): only k_sweep_tile honours write_ref
  // (the other forms would also write the reference rows, racing the side
  // stream's k_ref_planes with the same values), so it always takes that form.
  const int mode = a.write_ref ? t.sweep_flat : 2;
  // k_sweep_tile: 256 * nj elements per window (bf16 packs register pairs: nj even)
  int nj = t.sweep_nj;
  if (a.out_dtype == 1 && nj < 2) nj = 2;
  // 16-byte lane stores: NJ = the tuned pixels per lane (bf16: 2, 4, 8;
  // fp32: 1, 2, 4); rows keep 16-byte alignment from window to window (slab
  // a multiple of a store's pixels)
  // default (-1): bf16 volumes 2 pixels per lane (the C3 sweep 0.454 -> 0.347 ms
  // in the bench step, profiles/r04_sweep_wide_ab.txt), fp32 1 pixel per lane
  // (with the nt sc1 policy; 2 pixels per lane are slower)
  int store_px = t.sweep_store_px;
  if (store_px < 0) store_px = a.out_dtype == 1 ? 2 : 1;
  if (a.out_dtype == 1 && store_px == 1) store_px = 2;
  if (a.out_dtype == 0 && store_px == 8) store_px = 0;
  if (!(mode == 2 && slab % (a.out_dtype == 1 ? 8 : 4) == 0 && a.out % 16 == 0 && !t.sweep_share)) store_px = 0;
  if (store_px) nj = store_px;

  // The fall-through order.
  // 1. sweep_flat = 3: the band form, when the slab forms' range holds, the
  //    LDS takes at least two band rows and the grid fits.
  if (mode == 3 && slab_range(hw, slab) && plan_band(a, t, p)) return SFM_OK;
  // 2. sweep_flat = 2 (the default, and every warped-half call): k_sweep_tile;
  //    sweep_flat = 1: k_sweep_flat -- and sweep_flat = 3 whose band did not
  //    fit lands on k_sweep_flat too; all in the slab forms' range only.
  if (mode && slab_range(hw, slab) && plan_slab_windows(a, t, mode, nj, store_px, p)) return SFM_OK;
  // 3. sweep_flat = 0, and every shape outside that range: the per-row form,
  //    which always writes the reference rows.
  if (!a.write_ref) {
    p->error = "warped-half sweep: the shape is outside k_sweep_tile's range";
    return SFM_ERR_ARG;
  }
  p->form = SweepForm::row;
  p->name = p->vec ? "k_sweep+vec" : "k_sweep";
  p->blocks = (unsigned)((items + p->ipb - 1) / p->ipb);
  return SFM_OK;
}

}  // namespace sfm
