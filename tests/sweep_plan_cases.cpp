// Stand-alone driver of make_sweep_plan (csrc/sweep_plan.cpp, host code only):
// one line per case, "<the case> | <what the plan launches>": the kernel
// instantiation, grid, block, dynamic LDS and the resolved store policy.
// tests/test_sweep_plan.py builds it with -fsanitize=address,undefined, runs it
// and compares the lines with what the parent commit's library launched for
// the same calls (tests/golden/sweep_plan_parent_trace.txt) and, for the
// range edges that cannot be run, with forms derived from the parent's conditions.
#include <cstdio>
#include <string>
#include "sweep_plan.h"

namespace sfm {
void set_error(const std::string& msg) { std::printf("error: %s\n", msg.c_str()); }
}  // namespace sfm

using namespace sfm;

// the kernel instantiation as a demangler prints it
static std::string kernel_of(const SweepPlan& p) {
  const std::string t = p.out_dtype ? "unsigned short" : "float";
  auto b = [](bool v) { return std::string(v ? "true" : "false"); };
  switch (p.form) {
    case SweepForm::row:
      return "k_sweep<" + t + ", " + b(p.vec) + ", " + std::to_string(p.ipb) + ", " + b(p.lane_pixels == 1) + ", " +
             b(p.lane_pixels == 2) + ">";
    case SweepForm::flat: return "k_sweep_flat<" + t + ", " + std::to_string(p.nq) + ">";
    case SweepForm::tile: return "k_sweep_tile<" + t + ", " + std::to_string(p.nq) + ", " + std::to_string(p.nj) + ">";
    case SweepForm::band: return "k_sweep_band<" + t + ", " + std::to_string(p.nj) + ">";
  }
  return "";
}

// run: the case can be launched (small, and every key within its setter's range)
static void run(const char* tag, bool runnable, SweepArgs a, int off, const Tuning& t) {
  const uintptr_t base = 0x7f0000000000;   // a 256-byte aligned address; only its low bits matter
  a.out = base + (uintptr_t)off * (a.out_dtype ? 2 : 4);
  SweepPlan p;
  std::printf("%s run=%d B=%d C=%d L=%d h=%d w=%d dm=%d dt=%d ref=%d wr=%d off=%d flat=%d share=%d band_rows=%d px=%d "
              "buffer=%d group=%d nj=%d | ",
              tag, (int)runnable, a.B, a.C, a.L, a.h, a.w, a.depth_mode, a.out_dtype, (int)a.with_ref, (int)a.write_ref,
              off, t.sweep_flat, t.sweep_share, t.sweep_band_rows, t.sweep_store_px, t.sweep_buffer, t.sweep_group,
              t.sweep_nj);
  if (make_sweep_plan(a, t, &p) != SFM_OK) {
    std::printf("error=%s\n", p.error);
    return;
  }
  const int threads = p.form == SweepForm::band ? kBandThreads : kSwThreads;
  std::printf("form=%s scope=%s kernel=%s blocks=%u block=%d lds=%u store_px=%d store_nt=%d wpol=%d depths=%d\n", p.name,
              p.scope, kernel_of(p).c_str(), p.blocks, threads, p.lds, p.flat.store_px, p.flat.store_nt, p.flat.wpol,
              (int)p.depth_table);
}

static SweepArgs args(int B, int C, int h, int w, int L, int dt, bool with_ref = true, bool write_ref = true,
                      int depth_mode = 0) {
  return SweepArgs{B, C, h, w, L, 1.0f, depth_mode, dt, with_ref, write_ref, 0};
}

int main() {
  const int hws[3][2] = {{6, 8}, {6, 7}, {5, 7}};
  // the small shapes of tests/test_gpu_sweep_plan.py, crossed with the output
  // type, an output one element off, and every sweep_flat value
  for (int C : {8, 5})
    for (int L : {4, 3})
      for (auto& hw : hws)
        for (int dt : {0, 1})
          for (int off : {0, 1})
            for (int flat : {0, 1, 2, 3}) {
              Tuning t;
              t.sweep_flat = flat;
              run("small", true, args(2, C, hw[0], hw[1], L, dt), off, t);
            }
  // the other tuning keys the GPU cases set, the warped half, one larger map with interior windows
  for (int dt : {0, 1}) {
    Tuning t;
    t.sweep_share = 1;
    run("share", true, args(2, 8, 6, 8, 4, dt), 0, t);
    t = Tuning{};
    t.sweep_flat = 3;
    t.sweep_band_rows = 1;   // (the tuning setter refuses it; the plan's own fall-through to k_sweep_flat)
    run("band_rows1", false, args(2, 8, 6, 8, 4, dt), 0, t);
    t.sweep_band_rows = 16;
    run("band_too_wide", true, args(2, 5, 2, 2400, 3, dt), 0, t);
    for (int flat : {0, 3}) {
      t = Tuning{};
      t.sweep_flat = flat;
      run("warped_half", true, args(2, 8, 6, 8, 4, dt, true, false), 0, t);
    }
    t = Tuning{};
    run("warped_only", true, args(2, 8, 6, 8, 4, dt, false, true), 0, t);
    t.sweep_store_px = 0;
    run("store_px0", true, args(2, 8, 6, 8, 4, dt), 0, t);
    t = Tuning{};
    t.sweep_buffer = 0;
    run("buffer0", true, args(2, 8, 6, 8, 4, dt), 0, t);
    t = Tuning{};
    t.sweep_store_px = 8;
    run("store_px8", true, args(2, 8, 6, 8, 4, dt), 0, t);
    t = Tuning{};
    t.sweep_group = 4;
    t.sweep_nj = 4;
    t.sweep_store_px = 0;
    run("group4_nj4", true, args(2, 8, 6, 8, 4, dt), 0, t);
    for (int flat : {0, 1, 2, 3}) {
      t = Tuning{};
      t.sweep_flat = flat;
      run("interior", true, args(2, 8, 16, 24, 4, dt), 0, t);
    }
    t = Tuning{};
    run("depth_table", true, args(2, 8, 6, 8, 1024, dt, true, true, 1), 0, t);
    run("no_depth_table", true, args(2, 8, 6, 8, 1025, dt, true, true, 1), 0, t);
    run("one_channel", true, args(2, 1, 6, 8, 4, dt), 0, t);
  }
  // hw % 4 == 1 with L odd and even, per-row
  for (int L : {3, 4}) {
    Tuning t;
    t.sweep_flat = 0;
    run("hw_mod4_1", true, args(2, 5, 5, 5, L, 0), 0, t);
  }
  // range edges (none of them can be run), crossed with the output type, an
  // output one element off and every sweep_flat value
  for (int dt : {0, 1})
    for (int off : {0, 1})
      for (int flat : {0, 1, 2, 3}) {
        Tuning t;
        t.sweep_flat = flat;
        run("hw_below_2^24", false, args(1, 1, 4096, 4095, 1, dt), off, t);
        run("hw_at_2^24", false, args(1, 1, 4096, 4096, 1, dt), off, t);
        run("slab_below_2^30", false, args(1, 1, 1024, 1024, 1023, dt), off, t);
        run("slab_at_2^30", false, args(1, 1, 1024, 1024, 1024, dt), off, t);
        run("windows_below_2^31", false, args(1023, 1, 512, 1024, 1024, dt), off, t);
        run("windows_at_2^31", false, args(1024, 1, 512, 1024, 1024, dt), off, t);
        run("windows_at_2^31_warped_half", false, args(1024, 1, 512, 1024, 1024, dt, true, false), off, t);
        run("items_at_2^31", false, args(4096, 1, 512, 1024, 1024, dt), off, t);
      }
  return 0;
}
