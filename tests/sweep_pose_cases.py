"""Pose cases outside the small-motion regime for the plane-sweep, inverse-warp
and correlation tests, with a float64 classifier of every sample and the
expected values that go with it (tests/test_sweep_pose_cases.py checks the
table on the CPU, tests/test_gpu_sweep_poses.py runs the kernels against it).

Cases.  R is a rotation by the given angle about the given axis
(synth._rotation), K = synth.intrinsics(B, 4w, 4w, 2w, 2h) quartered, planes
MIN_DEPTH * L / (i + 1) unless a test asks for the depth planes:

  identity_zero_t   I, 0: border pixels sample exactly |xn| = 1 or |yn| = 1
  zero_x            I, 0 with cx = 0: X == 0 exactly in column 0, xn == -1 there
  pure_rot_5deg_y   5 deg about y, 0
  roll_30           30 deg about z, (0.1, 0, -0.5)
  roll_180          180 deg about z, (0, 0, 0.3): lanes walk the target row backwards
  yaw_90            90 deg about y, (0.5, 0, 0): nothing in range
  yaw_180_behind    180 deg about y, (0, 0, 0.2): every point behind the camera (Z clamped)
  backward_big_t    I, (0, 0, 5): everything in range
  forward_big_t     I, (0, 0, -5): the near planes clamp Z
  sideways          3 deg about (1, 1, 0), (-1, 0.05, 0)
  twisted           170 deg about (0.3, 1, 0.1), (0.6, -0.2, 0.77)
  huge_t            I, (3e19, 0, 1): |X| beyond sample_pos_nr's 2^60 gate
  clamped_in_range  I, (0, 0, -1.7e-4) with MIN_DEPTH = 1e-4: planes whose Z is
                    under the 1e-3 clamp and still sample inside the image
  mixed_batch       B = 3: synth.relative_pose (seed 4), roll_180, yaw_90

clamped_in_range carries its own MIN_DEPTH: with Z clamped to 1e-3 the image
[0, w-1] x [0, h-1] is the window 0 <= X <= 1e-3 (w-1), 0 <= Y <= 1e-3 (h-1)
of the projected point, and neighbouring pixels are one plane depth apart in X
and Y, so with MIN_DEPTH = 1 at most one pixel of a plane can fall into it
whatever the translation.  Depths of 1e-4 .. 1.6e-3 put whole planes there.

Classification of a sample (pixel, plane), from xn, yn, Z in float64 on the
float32 inputs (Z clamped at float32(1e-3) as the kernels and the oracle do)
and the oracle's own float32 xn, yn (oracle.sweep.warp_coords):

  guard      4 x max |xn32 - xn64| (and the same for yn) over the case's
             samples with |xn64| <= 2 (|yn64| <= 2); the 4 covers a second
             float32 evaluation order erring as far again on either side
  ambiguous  | |xn64| - 1 | <= guard_x  or  | |yn64| - 1 | <= guard_y
  clamped    Z64 < 1e-3 (1 + 1e-3)
  delta      4 x max |pos32 - pos64| in pixels over the clamped samples with
             both coordinates inside [-2, 2]

Expected values: the oracle's (plane_sweep_cost / inverse_warp /
correlation_cost) within test_gpu_sweep.py's _close_rel, 1e-4 |want| + 2e-6.
  * Clamped in-range samples add delta x (largest absolute difference among
    the four taps of that channel): X / 1e-3 turns last-bit differences of X
    into a thousand times as many pixels.
  * An ambiguous sample is not skipped: all channels of that pixel and plane
    together are either zero (bitwise) or the in-range alternative,
    grid_sample at the oracle's coordinates clipped to [-1, 1], within the
    same bar plus guard (in pixels) x the tap difference: a kernel that takes
    such a sample as in range samples up to guard away from the clipped
    position.  A sample that is ambiguous in one coordinate and outside by
    more than the guard in the other can only be zero.

Measured at 24x78, L = 16, inverse-depth planes, on the host of an MI355X
(`python -m tests.sweep_pose_cases` prints the table).  Per case: in-range
samples by the kernels' written-order float32 arithmetic (written_order_coords;
the kernels decided exactly so), ambiguous share, clamped share, guard (x, y;
normalised units), delta (pixels; `-`: no clamped sample near the image).

  identity_zero_t   29103/29952  0.106838  0        1.1e-06 1.0e-06  -
  zero_x            29148/29952  0.106838  0        1.1e-06 1.0e-06  -
  pure_rot_5deg_y   25440/29952  0         0        1.7e-06 1.8e-06  -
  roll_30           11655/29952  0.000167  0        2.3e-06 2.5e-06  -
  roll_180          29617/29952  0         0        1.4e-06 1.1e-06  -
  yaw_90                0/29952  0.003205  0.5      0       2.1e-03  -
  yaw_180_behind        0/29952  0         1        0       0        -
  backward_big_t    29952/29952  0         0        7.9e-07 8.3e-07  -
  forward_big_t      1114/29952  0.002604  0.8125   4.6e-06 3.5e-04  -
  sideways          13540/29952  0         0        2.0e-06 1.7e-06  -
  twisted               0/29952  0         1        1.5e-03 1.8e-03  -
  huge_t                0/29952  0         0        0       1.1e-06  -
  clamped_in_range  10079/29952  0         0.9375   6.6e-07 7.4e-07  2.3e-05
  mixed_batch       35865/89856  0.001647  0.25     9.6e-04 2.1e-03  -

The guards of the cases with clamped samples are a thousand times the others':
where Z is clamped, X / 1e-3 carries the last bits of X into the third decimal
of xn.  clamped_in_range has 1449 clamped in-range samples on its fullest plane.

The oracle's own float32 coordinates come out of bmm and round as the CPU's
sgemm does.  On the MI355X host they were the written order's bit for bit: in
all fourteen cases, every shape and both plane spacings the kernels took every
decision as the oracle did (0 of 1.1 million samples unlike, the ambiguous ones
included) and the warped values differed by 0 (correlation cost: <= 2.4e-7).
On another CPU the oracle's coordinates differed from the written order's in
0.2 % (forward translation) to 42 % (pure rotation) of the in-range samples, by
up to 6e-5 pixels where Z nearly cancels, and 381 of identity_zero_t's exact
border samples (312 of zero_x's) fell the other way: 29,484 in range.  No
decision differed outside the ambiguous set on either.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import sweep as S

RTOL, ATOL = 1e-4, 2e-6                      # test_gpu_sweep.py's _close_rel
Z_CLAMP = float(torch.tensor(1e-3, dtype=torch.float32))   # the float32 constant of the kernels and the oracle
SHAPES = [(13, 21), (20, 31), (24, 78)]      # odd hw under one window; hw % 4 == 2; hw % 4 == 0, rows across windows

# name -> per pair (axis, degrees, translation), or "benign" for synth.relative_pose
_I = ((0.0, 0.0, 1.0), 0.0)
POSES = {
    "identity_zero_t": [(*_I, (0.0, 0.0, 0.0))],
    "zero_x": [(*_I, (0.0, 0.0, 0.0))],
    "pure_rot_5deg_y": [((0.0, 1.0, 0.0), 5.0, (0.0, 0.0, 0.0))],
    "roll_30": [((0.0, 0.0, 1.0), 30.0, (0.1, 0.0, -0.5))],
    "roll_180": [((0.0, 0.0, 1.0), 180.0, (0.0, 0.0, 0.3))],
    "yaw_90": [((0.0, 1.0, 0.0), 90.0, (0.5, 0.0, 0.0))],
    "yaw_180_behind": [((0.0, 1.0, 0.0), 180.0, (0.0, 0.0, 0.2))],
    "backward_big_t": [(*_I, (0.0, 0.0, 5.0))],
    "forward_big_t": [(*_I, (0.0, 0.0, -5.0))],
    "sideways": [((1.0, 1.0, 0.0), 3.0, (-1.0, 0.05, 0.0))],
    "twisted": [((0.3, 1.0, 0.1), 170.0, (0.6, -0.2, 0.77))],
    "huge_t": [(*_I, (3e19, 0.0, 1.0))],
    "clamped_in_range": [(*_I, (0.0, 0.0, -1.7e-4))],
    "mixed_batch": ["benign", ((0.0, 0.0, 1.0), 180.0, (0.0, 0.0, 0.3)), ((0.0, 1.0, 0.0), 90.0, (0.5, 0.0, 0.0))],
}
CASES = list(POSES)
MIN_DEPTH = {"clamped_in_range": 1e-4}       # every other case: 1.0
# in-range samples at 24x78, L = 16, inverse-depth planes
IN_RANGE_24x78 = {
    "identity_zero_t": 29103, "pure_rot_5deg_y": 25440, "roll_30": 11655, "roll_180": 29617, "yaw_90": 0,
    "yaw_180_behind": 0, "backward_big_t": 29952, "forward_big_t": 1114, "sideways": 13540, "twisted": 0,
    "huge_t": 0,
}

Scene = namedtuple("Scene", "name h w ref tgt pose K Kinv K4 Ki4 min_depth")


def pose_of(spec, gen=None):
    """[3, 4] float32 pose of one (axis, degrees, translation) entry."""
    from sfm_amd import synth
    if spec == "benign":
        return synth.relative_pose(1, gen or torch.Generator().manual_seed(4))[0]
    axis, deg, t = spec
    P = torch.zeros(3, 4, dtype=torch.float64)
    P[:, :3] = synth._rotation(torch.tensor(axis, dtype=torch.float64), math.radians(deg))
    P[:, 3] = torch.tensor(t, dtype=torch.float64)
    return P.float()


def scene(name, h, w, C=8, seed=0):
    """CPU inputs of a case at (h, w): N(0,1) features, the case's poses,
    full-resolution K and K^-1 and their quartered forms."""
    from sfm_amd import synth
    specs = POSES[name]
    B = len(specs)
    ref, tgt = synth.features(B, C, h, w, seed=seed + 31 * h + w)
    K = synth.intrinsics(B, 4.0 * w, 4.0 * w, 0.0 if name == "zero_x" else 2.0 * w, 2.0 * h)
    Kinv = torch.inverse(K)
    pose = torch.stack([pose_of(s) for s in specs])
    K4, Ki4 = S.quarter_intrinsics(K, Kinv)
    return Scene(name, h, w, ref, tgt, pose, K, Kinv, K4, Ki4, MIN_DEPTH.get(name, 1.0))


def plane_depths(L, min_depth, by_depth=False):
    """[L] float32 plane depths in the oracle's own expressions (PSNet.py:150-153)."""
    one = torch.ones(1)
    if by_depth:
        return torch.cat([one * (i + 1) * min_depth for i in range(L)])
    return torch.cat([torch.div(one * min_depth * L, i + 1 + 1e-16) for i in range(L)])


Classes = namedtuple("Classes", "in32 ambiguous clamped sure_out X32 Z64 xn32 yn32 guard_x guard_y guard_px delta")


def _max(t):
    return float(t.max()) if t.numel() else 0.0


def classify(sc, L, by_depth=False):
    """Every sample of the case's volume classified: bool tensors [B, L, h, w]
    (in32: the oracle's float32 decision) and the case's guard / delta."""
    B, h, w = sc.pose.shape[0], sc.h, sc.w
    depths = plane_depths(L, sc.min_depth, by_depth)
    p64, k64, ki64 = sc.pose.double(), sc.K4.double(), sc.Ki4.double()
    cols = {k: [] for k in ("X32", "xn32", "yn32", "xn64", "yn64", "Z64")}
    for d in depths:
        X, _, _, xn, yn = S.warp_coords(torch.ones(B, h, w) * d, sc.pose, sc.K4, sc.Ki4, h, w)
        X6, Y6, Z6, _, _ = S.warp_coords(torch.ones(B, h, w, dtype=torch.float64) * d.double(), p64, k64, ki64, h, w)
        Zc = Z6.clamp(min=Z_CLAMP)
        for k, v in (("X32", X), ("xn32", xn), ("yn32", yn), ("Z64", Z6),
                     ("xn64", 2 * (X6 / Zc) / (w - 1) - 1), ("yn64", 2 * (Y6 / Zc) / (h - 1) - 1)):
            cols[k].append(v.reshape(B, h, w))
    c = {k: torch.stack(v, 1) for k, v in cols.items()}          # [B, L, h, w]
    xn32, yn32, xn64, yn64 = c["xn32"], c["yn32"], c["xn64"], c["yn64"]
    near_x, near_y = xn64.abs() <= 2, yn64.abs() <= 2
    guard_x = 4 * _max((xn32.double() - xn64)[near_x].abs())
    guard_y = 4 * _max((yn32.double() - yn64)[near_y].abs())
    amb_x = (xn64.abs() - 1).abs() <= guard_x
    amb_y = (yn64.abs() - 1).abs() <= guard_y
    ambiguous = amb_x | amb_y
    sure_out = (xn64.abs() > 1 + guard_x) | (yn64.abs() > 1 + guard_y)
    clamped = c["Z64"] < Z_CLAMP * (1 + 1e-3)
    in32 = (xn32 <= 1) & (xn32 >= -1) & (yn32 <= 1) & (yn32 >= -1)
    sel = clamped & near_x & near_y
    dpx = torch.maximum((xn32.double() - xn64).abs() * (w - 1) / 2, (yn32.double() - yn64).abs() * (h - 1) / 2)
    delta = 4 * _max(dpx[sel])
    guard_px = max(guard_x * (w - 1) / 2, guard_y * (h - 1) / 2)
    return Classes(in32, ambiguous, clamped, sure_out, c["X32"], c["Z64"], xn32, yn32, guard_x, guard_y, guard_px,
                   delta)


def _tap_spread(feat, xn, yn):
    """Largest absolute difference among the four bilinear taps of every
    channel at the normalised coordinates xn, yn [B, h, w] (clipped into the
    image): [B, C, h, w]."""
    B, C, h, w = feat.shape
    ix = ((xn.double().clamp(-1, 1) + 1) / 2 * (w - 1)).nan_to_num(0.0)
    iy = ((yn.double().clamp(-1, 1) + 1) / 2 * (h - 1)).nan_to_num(0.0)
    x0 = ix.floor().long().clamp(0, w - 1)
    y0 = iy.floor().long().clamp(0, h - 1)
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    flat = feat.reshape(B, C, h * w)
    taps = torch.stack([flat.gather(2, (yy * w + xx).reshape(B, 1, h * w).expand(B, C, h * w))
                        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))])
    return (taps.max(0).values - taps.min(0).values).reshape(B, C, h, w)


Expected = namedtuple("Expected", "want alt spread cls")


def expected_warped(sc, L, by_depth=False, feat=None):
    """The oracle's warped volume [B, C, L, h, w] of the case, the in-range
    alternative of every sample (grid_sample at the clipped coordinates), the
    per-channel tap spread, and the classification."""
    feat = sc.tgt if feat is None else feat
    cls = classify(sc, L, by_depth)
    depths = plane_depths(L, sc.min_depth, by_depth)
    B, h, w = sc.pose.shape[0], sc.h, sc.w
    want, alt, spread = [], [], []
    for i, d in enumerate(depths):
        want.append(S.inverse_warp(feat, torch.ones(B, h, w) * d, sc.pose, sc.K4, sc.Ki4))
        xc, yc = cls.xn32[:, i].clamp(-1, 1), cls.yn32[:, i].clamp(-1, 1)
        grid = torch.stack([xc, yc], -1).nan_to_num(0.0)
        alt.append(F.grid_sample(feat, grid, mode="bilinear", padding_mode="zeros", align_corners=True))
        spread.append(_tap_spread(feat, xc, yc))
    return Expected(torch.stack(want, 2), torch.stack(alt, 2), torch.stack(spread, 2), cls)


def check_values(got, want, alt, bar, abar, cls, what=""):
    """got, want, alt, bar, abar [B, C, L, h, w]: outside the ambiguous set got
    is within bar of want; an ambiguous sample is zero in all channels or
    within abar of alt in all channels (zero only, where the other coordinate
    is outside by more than the guard).  Prints the figures, then asserts."""
    got = got.float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got).any(), (what, "NaN in the output")
    amb = cls.ambiguous.unsqueeze(1)
    err = (got - want).abs()
    over = (err > bar) & ~amb
    zero = (got == 0).all(dim=1)
    is_alt = ((got - alt).abs() <= abar).all(dim=1)
    bad = cls.ambiguous & ~torch.where(cls.sure_out, zero, zero | is_alt)
    flips = (~zero) != cls.in32
    n = cls.in32.numel()
    fig = {"what": what, "samples": n, "in_range": int(cls.in32.sum()), "ambiguous": int(cls.ambiguous.sum()),
           "clamped": int(cls.clamped.sum()), "guard": (cls.guard_x, cls.guard_y), "delta": cls.delta,
           "decisions_unlike_oracle": int(flips.sum()), "of_them_unambiguous": int((flips & ~cls.ambiguous).sum()),
           "max_err_unambiguous": _max(err[(~amb).expand_as(err)]), "values": err.numel(),
           "outside_bar": int(over.sum()), "worst_excess": _max((err - bar)[over]),
           "first_outside": over.nonzero()[:3].tolist(), "bad_ambiguous": int(bad.sum()),
           "first_bad_ambiguous": bad.nonzero()[:3].tolist()}
    print(fig)
    assert fig["outside_bar"] == 0, fig
    assert fig["bad_ambiguous"] == 0, fig
    assert fig["of_them_unambiguous"] == 0, fig
    return fig


def check_warped(got, exp, what="", pos_tol=0.0):
    """Assert a warped volume [B, C, L, h, w] against expected_warped's result
    under the rules in the module's docstring.  Returns the figures it saw.
    ``pos_tol`` (pixels, 0 in every GPU test) adds pos_tol x the tap spread to
    every sample's bar; the table test uses it to run the checker on the CPU
    restatement, whose coordinates are another float32 rounding of the oracle's."""
    cls, want, alt = exp.cls, exp.want, exp.alt
    pos = pos_tol + torch.where((cls.clamped & cls.in32).unsqueeze(1), cls.delta, 0.0)
    bar = RTOL * want.abs() + ATOL + pos * exp.spread
    abar = RTOL * alt.abs() + ATOL + (pos + cls.guard_px) * exp.spread
    return check_values(got, want, alt, bar, abar, cls, what)


def check_correlation(got, ref, exp, what=""):
    """Assert a correlation cost [B, L, h, w] = mean over channels of ref x
    warped, with the classification applied per pixel and plane.  The bar is
    the warped bar carried through the mean: every channel's warped value may
    be off by its own bar, times |ref|, averaged; plus the float32 rounding of
    C products, C - 1 additions and the division in any order, (C + 1) 2^-24
    of the mean absolute product."""
    cls = exp.cls
    C = ref.shape[1]
    r = ref.unsqueeze(2)
    pos = torch.where((cls.clamped & cls.in32).unsqueeze(1), cls.delta, 0.0)
    rnd = (C + 1) * 2.0 ** -24

    def mean_bar(v, p):
        return ((r.abs() * (RTOL * v.abs() + ATOL + p * exp.spread)).mean(1, keepdim=True)
                + rnd * (r * v).abs().mean(1, keepdim=True))
    want = (r * exp.want).mean(1, keepdim=True)
    alt = (r * exp.alt).mean(1, keepdim=True)
    return check_values(got.unsqueeze(1), want, alt, mean_bar(exp.want, pos), mean_bar(exp.alt, pos + cls.guard_px),
                        cls, what)


def written_order_coords(sc, L, by_depth=False, z_clamp=1e-3):
    """warp.h's load_proj + sample_pos restated on the CPU in float32, every
    operation rounded on its own in the written order (the library is built
    without FMA contraction): (xn, yn) [B, L, h, w] before the range test.
    A stand-in for the kernels where there is no GPU: the table test counts
    its decisions and runs check_warped on what it samples."""
    B, h, w = sc.pose.shape[0], sc.h, sc.w
    K, P, ki = sc.K4, sc.pose, sc.Ki4.reshape(B, 9, 1, 1, 1)
    m = [[(K[:, r, 0] * P[:, 0, c] + K[:, r, 1] * P[:, 1, c]) + K[:, r, 2] * P[:, 2, c] for c in range(4)]
         for r in range(3)]
    m = [[v.reshape(B, 1, 1, 1) for v in row] for row in m]
    x = torch.arange(w, dtype=torch.float32).reshape(1, 1, 1, w)
    y = torch.arange(h, dtype=torch.float32).reshape(1, 1, h, 1)
    d = plane_depths(L, sc.min_depth, by_depth).reshape(1, L, 1, 1)
    ray = [(ki[:, 3 * r] * x + ki[:, 3 * r + 1] * y) + ki[:, 3 * r + 2] for r in range(3)]
    c = [r * d for r in ray]
    X, Y, Z = [((m[r][0] * c[0] + m[r][1] * c[1]) + m[r][2] * c[2]) + m[r][3] for r in range(3)]
    Z = torch.where(Z < z_clamp, torch.full_like(Z, z_clamp), Z)
    xn = 2.0 * (X / Z) / float(w - 1) - 1.0
    yn = 2.0 * (Y / Z) / float(h - 1) - 1.0
    return xn, yn


def written_order_warped(sc, L, by_depth=False, z_clamp=1e-3, feat=None):
    """The warped volume [B, C, L, h, w] sampled at written_order_coords."""
    feat = sc.tgt if feat is None else feat
    xn, yn = written_order_coords(sc, L, by_depth, z_clamp)
    out = ~((xn <= 1) & (xn >= -1) & (yn <= 1) & (yn >= -1))
    grid = torch.stack([torch.where(out, torch.full_like(xn, 2.0), xn),
                        torch.where(out, torch.full_like(yn, 2.0), yn)], -1)
    return torch.stack([F.grid_sample(feat, grid[:, i], mode="bilinear", padding_mode="zeros", align_corners=True)
                        for i in range(L)], 2)


def table_row(name, h=24, w=78, L=16, by_depth=False):
    sc = scene(name, h, w)
    c = classify(sc, L, by_depth)
    n = c.in32.numel()
    xn, yn = written_order_coords(sc, L, by_depth)
    wo = (xn <= 1) & (xn >= -1) & (yn <= 1) & (yn >= -1)
    return {"name": name, "in_range": int(c.in32.sum()), "in_range_written_order": int(wo.sum()),
            "flips": int((wo != c.in32).sum()), "flips_unambiguous": int(((wo != c.in32) & ~c.ambiguous).sum()),
            "samples": n, "ambiguous": float(c.ambiguous.sum()) / n,
            "clamped": float(c.clamped.sum()) / n, "guard_x": c.guard_x, "guard_y": c.guard_y, "delta": c.delta,
            "clamped_in_range_per_plane": (c.clamped & c.in32).flatten(2).sum(2).max().item()}


if __name__ == "__main__":
    for nm in CASES:
        r = table_row(nm)
        print(f"  {r['name']:<17} {r['in_range']:>5}/{r['samples']}  {r['ambiguous']:.6f}  {r['clamped']:<8.6g} "
              f"{r['guard_x']:.1e} {r['guard_y']:.1e}  {r['delta']:.1e}  ({r['clamped_in_range_per_plane']}, "
              f"{r['in_range_written_order']}, {r['flips']}, {r['flips_unambiguous']})")
