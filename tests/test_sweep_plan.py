"""make_sweep_plan (csrc/sweep_plan.cpp: which sweep form a call takes, its
template parameters, grid, LDS and store policy) as a stand-alone host program
under ASan + UBSan: tests/sweep_plan_cases.cpp prints one line per case.

Runnable cases (run=1: the small shapes of tests/test_gpu_sweep_plan.py crossed
with fp32 / bf16, an aligned and an off-by-one output and every sweep_flat
value, and the other keys those tests set): the kernel instantiation, grid and
block must be what the PARENT commit's library launched for exactly those
calls.  tests/golden/sweep_plan_parent_trace.txt was written from a kernel
trace of that library (a run of its own, no counters) making the 226 calls in
the order of the table.  The trace's LDS column holds a kernel's static LDS
only, so the one dynamic amount, k_sweep_band's, is checked against the
parent's formula (csrc/sweep.hip of the parent, lines 1379-1381 and 1542-1554):
cap_rows * w * 16 + 4 * (256 * nj + 128) * 4 bytes with cap_rows = min(16,
rows the 80 KB - 64 budget holds, h).

Range edges (run=0; no GPU can run them), crossed with the output type, the
off-by-one output and every sweep_flat value: the form is derived by hand
from the conditions of the parent's launch_sweep, see _edge_form."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep-sfm-revisited_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

TOO_LARGE = "error=sweep too large for one launch"
NO_TILE = "error=warped-half sweep: the shape is outside k_sweep_tile's range"


def _edge_form(tag, dt, flat):
    """The parent's conditions (line numbers of its csrc/sweep.hip).  Every edge
    map has h*w % 4 == 0, so the per-row form stores vectors (1485-1486)."""
    row = "form=k_sweep+vec"
    if tag == "items_at_2^31":            # 4096 * (1 + 1) * 1024 * 513 items >= 2^31, checked before any form (1492)
        return TOO_LARGE
    if tag in ("hw_at_2^24", "slab_at_2^30"):     # outside hw < 2^24 / slab < 2^30: no slab form (1528, 1573)
        return row
    if tag == "windows_at_2^31_warped_half":
        # write_ref = 0 forces the tile form whatever the key says (1511).  fp32: 256-element windows,
        # 1024 * (2^21 + 1) >= 2^31 blocks, so no slab form (1573) and the per-row form is refused (1627);
        # bf16: 512-element windows, 1024 * (2^20 + 1) blocks fit
        return "form=k_sweep_tile" if dt else NO_TILE
    if flat == 0:                          # (1573: mode 0 takes no slab form)
        return row
    if flat == 1:                          # 1024-element windows: at most 1024 * (2^19 + 1) blocks
        return "form=k_sweep_flat"
    if flat == 2:
        if tag == "windows_at_2^31" and dt == 0:   # 1024 * (2^21 + 1) >= 2^31 (1573); 1023 pairs stay below
            return row
        return "form=k_sweep_tile"
    # flat == 3 (1528-1548): a row of 4095 quads is 65,520 bytes, the LDS budget holds one, cap_rows < 2,
    # and the call lands on k_sweep_flat (1571-1573); 1024-wide maps hold 4 rows and at most
    # 1024 * 64 * 2049 blocks
    return "form=k_sweep_flat" if tag == "hw_below_2^24" else "form=k_sweep_band"


def _clang():
    for sub in ("lib/llvm/bin", "llvm/bin"):
        p = os.path.join(ROCM, sub, "clang++")
        if os.path.exists(p):
            return p
    raise AssertionError("no clang++ under " + ROCM)


def test_sweep_plan_cases_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sweep_plan_cases")
    subprocess.run([_clang(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "sweep_plan_cases.cpp"), os.path.join(CSRC, "sweep_plan.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = [tuple(x.strip() for x in l.split(" | ")) for l in r.stdout.splitlines()]
    parent = [tuple(x.strip() for x in l.split(" | "))
              for l in open(os.path.join(ROOT, "tests", "golden", "sweep_plan_parent_trace.txt")).read().splitlines()]
    launch = re.compile(r"kernel=(.*?) blocks=(\d+) block=(\d+) lds=(\d+)")
    runnable = [(c, p) for c, p in got if " run=1 " in c]
    assert [c for c, _ in runnable] == [c for c, _ in parent] and len(parent) == 226
    bad = []
    for (case, plan), (_, traced) in zip(runnable, parent):
        g, t = launch.search(plan), launch.search(traced)
        if g.groups()[:3] != t.groups()[:3]:
            bad.append((case, g.groups(), t.groups()))
        f = dict(x.split("=") for x in case.split()[1:])
        if g.group(1).startswith("k_sweep_band"):
            h, w, nj = int(f["h"]), int(f["w"]), 2 if f["dt"] == "1" else 1
            fixed = 4 * (256 * nj + 128) * 4
            cap = min(16, (80 * 1024 - 64 - fixed) // (16 * w), h)
            assert int(g.group(4)) == cap * w * 16 + fixed, case
        else:
            assert int(g.group(4)) == 0, case
    assert not bad, bad[:3]
    edges = [(c, p) for c, p in got if " run=0 " in c and not c.startswith("band_rows1")]
    assert len(edges) == 8 * 16
    for case, plan in edges:
        f = dict(x.split("=") for x in case.split()[1:])
        want = _edge_form(case.split()[0], int(f["dt"]), int(f["flat"]))
        assert plan.split()[0].split("+wide")[0] == want or plan == want, (case, plan, want)
    # a one-row band (refused by the key's setter, so never traced): the parent's cap_rows >= 2 (1548)
    assert all(p.startswith("form=k_sweep_flat ") for c, p in got if c.startswith("band_rows1"))


def test_sweep_files_stay_under_1024_lines():
    for f in sorted(os.listdir(CSRC)):
        if f.startswith("sweep"):
            assert sum(1 for _ in open(os.path.join(CSRC, f))) <= 1024, f
