"""Cases and expected values for the plane sweep's backward kernel
(csrc/sweep_bwd.hip): tests/test_sweep_bwd_cases.py checks them on the CPU,
tests/test_gpu_sweep_backward.py runs the kernel against them.

Expected value.  ``scatter64`` is the transpose of the forward's bilinear
gather, accumulated in float64: the sample coordinates are the oracle's own
float32 xn, yn (oracle.sweep.warp_coords), the in-range decision and the pixel
position ((xn + 1) / 2) (w - 1) are taken in float32 as grid_sample takes them,
and weights, products and sums are float64.

Bar.  The project's 1e-4 relative bar in test_gpu_sweep.py's form,
|got - want| <= 1e-4 max(|want|, FLOOR), with FLOOR the RMS of the expected
gradient, for the reason written there: sample coordinates move by float32
ulps between implementations, which moves a gradient element by a multiple
of the gradient's scale, however close that one element is to zero.

Exact lattice.  9 x 17 (w - 1 = 16, h - 1 = 8), K = [[16, 0, 8], [0, 16, 4],
[0, 0, 1]] at feature resolution, identity rotation, inverse-depth planes with
MIN_DEPTH = 12 and L in {1, 5}: the plane depths 12 L / (i + 1) are the
integers 12, or 60, 30, 20, 15, 12.  With t = (s 12 L / 16, 0, 0) plane i
samples pixel (x, y) at exactly (x + s (i + 1), y): every intermediate value is
a small dyadic rational, so any float32 evaluation order gives the same bits.
s = 0 (identity), +1 / -1 (whole pixels, pair 0 / pair 1) and +1/2 / -1/2
(weights 1/2).  With an integer-valued g every sum is exact in float32 in any
order, so the kernel's atomics must reproduce ``lattice_expected`` bit for bit.

General poses at 10 x 12 and 7 x 5, L = 4, C = 32, B = 2: pose entries of
tests/sweep_pose_cases.py paired up, a 90 degree roll either way (rows map to
columns), a pose that puts part of the image behind the camera (Z clamp), and
two that put every sample out of range.  At these shapes the kernel's LDS
window holds the whole image and a chunk is one plane (``bwd_geom``), so they
check the geometry, not the window: the TALL and WIDE cases below are there for
the taps that leave a window, chunks of several planes, a partial last
channel group and the form without a window, and ``window_replay`` counts how
many taps take which way.
"""
import math
from collections import namedtuple

import torch

from oracle import sweep as S
from tests import sweep_pose_cases as P

RTOL = 1e-4

LATTICE_HW = (9, 17)
LATTICE_MIN_DEPTH = 12.0
LATTICE_SHIFTS = {"identity": (0.0, 0.0), "whole": (1.0, -1.0), "half": (0.5, -0.5)}   # per pair, pixels per plane index
LATTICE_CL = [(3, 1), (3, 5), (32, 1), (32, 5)]

_I = ((0.0, 0.0, 1.0), 0.0)
GENERAL = {
    "roll30_sideways": [P.POSES["roll_30"][0], P.POSES["sideways"][0]],
    "rot5_backward": [P.POSES["pure_rot_5deg_y"][0], P.POSES["backward_big_t"][0]],
    # translations that keep the rolled lattice off the image border (a pure roll about the principal point puts
    # whole rows of samples at |xn| = 1 exactly, where float32 evaluation orders may decide differently)
    "roll_90": [((0.0, 0.0, 1.0), 90.0, (0.137, -0.071, 0.2)), ((0.0, 0.0, 1.0), -90.0, (-0.093, 0.041, 0.0))],
    # forward motion past the near planes: depths 4, 2 (pair 1: 4) stay in front, the nearer planes are behind
    "partly_behind": [(*_I, (0.02, 0.01, -1.5)), ((0.0, 0.0, 1.0), 4.0, (-0.03, 0.02, -2.5))],
    "all_out": [P.POSES["yaw_180_behind"][0], (*_I, (50.0, 0.0, 0.0))],
}
GENERAL_SHAPES = [(10, 12), (7, 5)]
GENERAL_L, GENERAL_C = 4, 32

# At the shapes above the kernel's LDS window holds every target row and its chunks are one plane each
# (bwd_geom below).  Two more cases reach the rest of the kernel:
#   tall   40 x 24, B = 4, C = 28, L = 52: a window of 10 of the 40 rows, chunks of 4 planes (1,040 workgroups), a
#          last channel group of 4; the two 90 degree rolls spread a band's taps over up to 25 target rows, so a
#          large share of the taps leaves the window for the global atomics (window_replay counts them)
#   wide   3 x 1100, B = 2, C = 12, L = 4: rows too long for any window, the "k_sweep_bwd+global" form, with a last
#          channel group of 4
TALL = dict(name="tall", h=40, w=24, C=28, L=52,
            specs=[GENERAL["roll_90"][0], GENERAL["roll_90"][1], GENERAL["partly_behind"][0],
                   ((0.0, 0.0, 1.0), 27.0, (0.21, 0.013, -0.3))])
# (poses of their own where sweep_pose_cases' put a sample within the float32 guard of the border at these shapes:
# tests/test_sweep_bwd_cases.py rejects a case with such a sample)
WIDE = dict(name="wide", h=3, w=1100, C=12, L=4,
            specs=[((1.0, 1.0, 0.0), 3.0, (-0.37, 0.05, 0.1)), ((0.0, 1.0, 0.0), 4.0, (0.113, 0.0007, 0.21))])

Case = namedtuple("Case", "name h w L min_depth by_depth pose K4 Ki4")


def close(got, want):
    """(ok, max abs error, floor): the bar of the module's docstring."""
    got, want = got.double().cpu(), want.double().cpu()
    floor = float(want.pow(2).mean().sqrt())
    err = (got - want).abs()
    return bool((err <= RTOL * want.abs().clamp(min=floor)).all()), float(err.max()), floor


def lattice_case(kind, L):
    h, w = LATTICE_HW
    K4 = torch.tensor([[16.0, 0.0, 8.0], [0.0, 16.0, 4.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1)
    pose = torch.zeros(2, 3, 4)
    pose[:, :, :3] = torch.eye(3)
    for b, s in enumerate(LATTICE_SHIFTS[kind]):
        pose[b, 0, 3] = s * LATTICE_MIN_DEPTH * L / 16.0
    return Case(f"lattice_{kind}_L{L}", h, w, L, LATTICE_MIN_DEPTH, False, pose, K4, torch.inverse(K4))


def lattice_positions(kind, L):
    """The intended sample positions [2, L, h, w] (x, y) of a lattice case, float64."""
    h, w = LATTICE_HW
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w).expand(2, L, h, w)
    y = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1).expand(2, L, h, w)
    s = torch.tensor(LATTICE_SHIFTS[kind], dtype=torch.float64).view(2, 1, 1, 1)
    i1 = torch.arange(1, L + 1, dtype=torch.float64).view(1, L, 1, 1)
    return x + s * i1, y


def lattice_expected(kind, g):
    """grad_tgt of a lattice case from its closed form: plane i moves column x
    to x + s (i + 1); a whole shift carries g there, a half shift splits it in
    halves between the two neighbours; positions outside [0, w - 1] contribute
    nothing.  g: the warped half's gradient [2, C, L, h, w], integer-valued."""
    B, C, L, h, w = g.shape
    out = torch.zeros(B, C, h, w, dtype=torch.float64)
    for b, s in enumerate(LATTICE_SHIFTS[kind]):
        for i in range(L):
            for x in range(w):
                pos = x + s * (i + 1)
                if pos < 0 or pos > w - 1:
                    continue
                x0 = math.floor(pos)
                fr = pos - x0
                out[b, :, :, x0] += (1.0 - fr) * g[b, :, i, :, x].double()
                if fr > 0:
                    out[b, :, :, x0 + 1] += fr * g[b, :, i, :, x].double()
    return out.float()


def integer_g(B, rows, L, h, w, seed):
    return torch.randint(-3, 4, (B, rows, L, h, w), generator=torch.Generator().manual_seed(seed)).float()


def general_case(name, h, w):
    from sfm_amd import synth
    specs = GENERAL[name]
    K = synth.intrinsics(len(specs), 4.0 * w, 4.0 * w, 2.0 * w, 2.0 * h)
    K4, Ki4 = S.quarter_intrinsics(K, torch.inverse(K))
    return Case(f"{name}_{h}x{w}", h, w, GENERAL_L, 1.0, False, torch.stack([P.pose_of(s) for s in specs]), K4, Ki4)


def plane_depth_maps(case):
    """[L] depth maps [B, h, w] of a case's planes (the oracle's expressions)."""
    d = P.plane_depths(case.L, case.min_depth, case.by_depth)
    B = case.pose.shape[0]
    return [torch.ones(B, case.h, case.w) * d[i] for i in range(case.L)]


def oracle_positions(depth_maps, pose, K, Kinv, h, w):
    """The oracle's float32 decision and pixel positions of every sample:
    (inside [B, L, hw] bool, ix, iy [B, L, hw] float32)."""
    xs, ys = [], []
    for d in depth_maps:
        _, _, _, xn, yn = S.warp_coords(d, pose, K, Kinv, h, w)
        xs.append(xn)
        ys.append(yn)
    xn, yn = torch.stack(xs, 1), torch.stack(ys, 1)
    inside = (xn <= 1) & (xn >= -1) & (yn <= 1) & (yn >= -1)
    ix = ((xn + 1) / 2) * (w - 1)
    iy = ((yn + 1) / 2) * (h - 1)
    return inside, ix, iy


def scatter64(g, inside, ix, iy, h, w):
    """The transpose of the bilinear gather in float64.  g [B, C, L, h, w]
    (the warped half's gradient); returns grad_tgt [B, C, h, w] float64."""
    B, C, L = g.shape[:3]
    hw = h * w
    gd = g.double().reshape(B, C, L * hw)
    ixd = torch.where(inside, ix, torch.zeros_like(ix)).double()
    iyd = torch.where(inside, iy, torch.zeros_like(iy)).double()
    x0, y0 = ixd.floor(), iyd.floor()
    wx1, wy1 = ixd - x0, iyd - y0
    out = torch.zeros(B, C, hw, dtype=torch.float64)
    for dx, dy, wt in ((0, 0, (1 - wx1) * (1 - wy1)), (1, 0, wx1 * (1 - wy1)), (0, 1, (1 - wx1) * wy1),
                       (1, 1, wx1 * wy1)):
        xx, yy = x0.long() + dx, y0.long() + dy
        ok = inside & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(B, 1, L * hw).expand(B, C, L * hw)
        wgt = torch.where(ok, wt, torch.zeros_like(wt)).reshape(B, 1, L * hw)
        out.scatter_add_(2, idx, wgt * gd)
    return out.reshape(B, C, h, w)


def expected_grad_tgt(case, g_warped):
    inside, ix, iy = oracle_positions(plane_depth_maps(case), case.pose, case.K4, case.Ki4, case.h, case.w)
    return scatter64(g_warped, inside, ix, iy, case.h, case.w), inside


def expected_warp_grad(feat_shape, depth, pose, K, Kinv, g):
    """inverse_warp's gradient into feat: one "plane" with a depth map."""
    B, C, h, w = feat_shape
    inside, ix, iy = oracle_positions([depth], pose, K, Kinv, h, w)
    return scatter64(g.reshape(B, C, 1, h, w), inside, ix, iy, h, w)


def shaped_case(spec):
    """A Case from TALL / WIDE: K as the general cases', the spec's poses."""
    from sfm_amd import synth
    h, w, specs = spec["h"], spec["w"], spec["specs"]
    K = synth.intrinsics(len(specs), 4.0 * w, 4.0 * w, 2.0 * w, 2.0 * h)
    K4, Ki4 = S.quarter_intrinsics(K, torch.inverse(K))
    return Case(spec["name"], h, w, spec["L"], 1.0, False, torch.stack([P.pose_of(s) for s in specs]), K4, Ki4)


Geom = namedtuple("Geom", "cg wr rb nbands lp nchunks blocks")


def bwd_geom(B, C, h, w, L):
    """csrc/sweep_bwd.hip's launch shape (bwd_geom there), restated: channels
    per group, window rows (0: none), rows per band, planes per chunk."""
    cg = min(C, 8)
    wr = min(h, (64 * 1024) // (cg * w * 4))
    if wr < 2:
        wr = 0
    wr = min(wr, 10)
    rb = max(1, wr - 2) if wr else min(h, 4)
    nbands = (h + rb - 1) // rb
    per_chunk = B * ((C + 7) // 8) * nbands
    lp = min(16, L)
    while lp > 1 and per_chunk * ((L + lp - 1) // lp) < 1024:
        lp = (lp + 1) // 2
    nchunks = (L + lp - 1) // lp
    return Geom(cg, wr, rb, nbands, lp, nchunks, per_chunk * nchunks)


def window_replay(case, C):
    """The kernel's window placement replayed on the oracle's positions: the
    row-taps (a sample's upper row, and its lower row where that weighs in)
    that land inside their workgroup's LDS window and those that leave it for
    a global atomic.  (inside, outside, geom).  The oracle's coordinates may
    differ from the kernel's in their last bits; this is a count, not an
    expected value."""
    B, h, w, L = case.pose.shape[0], case.h, case.w, case.L
    q = bwd_geom(B, C, h, w, L)
    ins, ix, iy = oracle_positions(plane_depth_maps(case), case.pose, case.K4, case.Ki4, h, w)
    ins, iy = ins.reshape(B, L, h, w), iy.reshape(B, L, h, w)
    n_in = n_out = 0
    for b in range(B):
        for ch in range(q.nchunks):
            l0 = ch * q.lp
            nl = min(q.lp, L - l0)
            for band in range(q.nbands):
                y0 = band * q.rb
                nrow = min(q.rb, h - y0)
                sel = ins[b, l0:l0 + nl, y0:y0 + nrow]
                top = iy[b, l0:l0 + nl, y0:y0 + nrow][sel].floor().long()
                frac = iy[b, l0:l0 + nl, y0:y0 + nrow][sel] - top
                rows = torch.cat([top, (top + 1)[(frac > 0) & (top + 1 < h)]])
                if q.wr == 0:
                    n_out += rows.numel()
                    continue
                cy, lc = y0 + nrow // 2, l0 + nl // 2
                if bool(ins[b, lc, cy, w // 2]):
                    cy = int(iy[b, lc, cy, w // 2].floor())
                wy0 = min(max(cy - nrow // 2 - (q.wr - nrow - 1) // 2, 0), h - q.wr)
                inside = (rows >= wy0) & (rows < wy0 + q.wr)
                n_in += int(inside.sum())
                n_out += int((~inside).sum())
    return n_in, n_out, q
