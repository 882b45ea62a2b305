"""Batches for the GPU IRLS (sfm_essential_optimise_batched, csrc/irls.hip)
with the float64 oracle's result and the oracle's own sensitivity to the order
of its sums (tests/test_irls_cases.py checks the table on the CPU,
tests/test_gpu_irls.py runs the kernels against it).

Scenes.  sfm_amd.synth on a 72 x 64 image (4608 pixels) with intrinsics
(64, 64, 32, 36), so the normalised points span about +-0.5: a seeded depth
field and relative pose, the rigid flow they induce, pixel noise and uniformly
random outlier flows, turned into normalised correspondences in float64.  A
pair's points are a seeded shuffle of the pixels, the first n[b] of them; rows
k >= n[b] of the batch's ``pts`` are NaN.  E_init is [t]x R of the true pose
with R turned by a fraction of a degree and t nudged, or (pair 0 of the ragged
batch) the winner of oracle.ransac5 on that pair's points.

Reference.  oracle.ransac5.optimise on the pair's first n[b] points.

Tolerance.  The GPU differs from the oracle only by reassociated sums, so the
bar is taken from the oracle: d_perm is the largest entry-wise change of the
oracle's E, relative to max |E|, when the same points are fed in reversed
order and in one fixed seeded permutation.  The GPU must lie within
max(8 d_perm, 1e-12) relative of the oracle (8: a sequential sum against a
256-wide tree over several thousand terms, iterated) and under the project's
1e-4 bar.  Every compared pair must have d_perm <= 1e-8; a scene that does not
is changed (noise, delta, repetitions, alpha), never the bound.

Cases (B, n_stride, n; delta, alpha, max_reps) and the measured d_perm per
compared pair (`python -m tests.irls_cases` prints the table; another host's
libm moves the figures by a factor of about two):

  ragged(d, a, reps)   B = 5, stride 4608, n = 4608, 4097, 257, 64, 5 (pair : n : d_perm)
    (1e-3, 1, 30)      0:4608:1.5e-16  1:4097:8.1e-16  2:257:6.3e-16  3:64:3.1e-16  4:5:4.3e-15
    (1e-3, 0, 8)       0:4608:6.6e-16  1:4097:5.4e-16  2:257:3.3e-16  3:64:3.6e-16  4:5:4.3e-15
    (2e-3, 0.5, 0)     0 for every pair (E = U diag(1, 1, 0) V^T of the start)
  stops                B = 3, stride 4608; (1e-3, 1, 5)
                       0:4608:0  1:2000:3.1e-16  2:3000:7.6e-16
  blocks(n)            B = 1, stride n; (1e-3, 1, 10)
                       5: 5.2e-15   4096: 2.8e-16   4097: 1.5e-15
  wrap                 B = 1, n = stride = 1,048,833; (1e-3, 1, 2):  2.5e-14
  wide                 B = 65, stride 64, n = 64; (1e-3, 1, 3)
                       0: 2.1e-16   63: 1.0e-15   64: 1.9e-15
  empty                B = 3, stride 300, n = 300, 0, 77; (1e-3, 1, 5)
                       0: 3.3e-16   1: 0   2: 2.4e-15

Every 8 d_perm is under 1e-12 (wrap: 2e-13), so the floor of 1e-12 relative
is the bar of every pair.

An empty pair (n = 0) has zero sums: the oracle accepts it and returns the
Givens-reduced E_init, so it is compared too.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import ransac5 as R

HW = (72, 64)
INTR = (64.0, 64.0, 32.0, 36.0)
D_PERM_MAX = 1e-8
PROJECT_BAR = 1e-4
N_WRAP = 256 * 4096 + 257

Case = namedtuple("Case", "name pts n n_stride E_init delta alpha reps compared")


def bound(d_perm):
    """The relative bar of a pair with the given d_perm."""
    return min(max(8.0 * d_perm, 1e-12), PROJECT_BAR)


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def true_essential(pose):
    """[t]x R of a [3, 4] pose X2 = R X1 + t: qp^T E q = 0 for exact correspondences."""
    p = np.asarray(pose, np.float64)
    return _skew(p[:, 3]) @ p[:, :3]


def perturbed_essential(pose, seed, deg=0.3, dt=0.02):
    """[t']x R' with R' = R rot(random axis, deg) and t' = t + dt |t| N(0, 1)."""
    from sfm_amd import synth
    g = torch.Generator().manual_seed(int(seed))
    p = np.asarray(pose, np.float64)
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    Rp = p[:, :3] @ synth._rotation(axis, math.radians(deg)).numpy()
    t = p[:, 3] + dt * np.linalg.norm(p[:, 3]) * torch.randn(3, generator=g, dtype=torch.float64).numpy()
    return _skew(t) @ Rp


Scene = namedtuple("Scene", "pts pose")


@functools.lru_cache(maxsize=None)
def scene(seed, noise_px=0.02, outlier_frac=0.1):
    """All 4608 correspondences [4608, 4] float64 (q.x, q.y, qp.x, qp.y) of one
    seeded pair in a seeded shuffle, and its [3, 4] pose.  noise_px = 0 and
    outlier_frac = 0 give exact correspondences (float64 flow)."""
    from sfm_amd import synth
    gen = torch.Generator().manual_seed(int(seed))
    H, W = HW
    K = synth.intrinsics(1, *INTR).double()
    pose = synth.relative_pose(1, gen).double()
    depth = synth.depth_field(1, H, W, gen, min_depth=3.0, max_depth=32.0, coarse=(4, 4)).double()
    flow, _ = synth.rigid_flow(depth, pose, K)
    if noise_px > 0:
        flow = flow + noise_px * torch.randn(flow.shape, generator=gen, dtype=torch.float64)
    if outlier_frac > 0:
        out = torch.rand(1, H, W, generator=gen) < outlier_frac
        rnd = (torch.rand(1, 2, H, W, generator=gen, dtype=torch.float64) - 0.5) * 20.0
        flow = torch.where(out.unsqueeze(1), rnd, flow)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    one = torch.ones_like(xs)
    Ki = torch.inverse(K[0])
    q = (Ki @ torch.stack([xs, ys, one]).reshape(3, -1))[:2]
    qp = (Ki @ torch.stack([xs + flow[0, 0], ys + flow[0, 1], one]).reshape(3, -1))[:2]
    pts = torch.cat([q, qp]).t()
    order = torch.randperm(H * W, generator=gen)
    return Scene(np.ascontiguousarray(pts[order].numpy()), pose[0].numpy())


def _batch(name, scenes, n, n_stride, E_init, delta, alpha, reps, compared=None):
    B = len(n)
    pts = np.full((B, n_stride, 4), np.nan)
    for b in range(B):
        pts[b, :n[b]] = scenes[b][:n[b]]
    return Case(name, pts, list(n), n_stride, np.stack(E_init), delta, alpha, reps,
                list(range(B)) if compared is None else compared)


RAGGED_N = [4608, 4097, 257, 64, 5]
RAGGED_PARAMS = [(1e-3, 1.0, 30), (1e-3, 0.0, 8), (2e-3, 0.5, 0)]


@functools.lru_cache(maxsize=None)
def ragged(delta, alpha, reps):
    """Case 1: five pairs of their own scenes, n = 4608, 4097, 257, 64, 5 in a stride of 4608 (two blocks)."""
    sc = [scene(100 + b) for b in range(4)] + [scene(104, noise_px=0.002, outlier_frac=0.0)]
    E = [perturbed_essential(s.pose, 200 + b) for b, s in enumerate(sc)]
    p0 = sc[0].pts
    E[0] = R.ransac5(p0[:, :2], p0[:, 2:], iters=1, thr=1e-3)["E"]
    # five points fix the five parameters exactly: a starting point close enough that every residual is under delta
    E[4] = perturbed_essential(sc[4].pose, 204, deg=0.01, dt=0.001)
    return _batch(f"ragged({delta:g},{alpha:g},{reps})", [s.pts for s in sc], RAGGED_N, 4608, E, delta, alpha, reps)


STOPS_REPS = 5


@functools.lru_cache(maxsize=None)
def stops():
    """Case 3: an exact pair at the exact E (stops at repetition 0), an exact
    pair from a perturbed E (converges, then stops), a noisy pair with
    outliers under alpha = 1 (still moving at max_reps)."""
    a, b, c = scene(300, 0.0, 0.0), scene(301, 0.0, 0.0), scene(302, 0.05, 0.15)
    E = [true_essential(a.pose), perturbed_essential(b.pose, 311), perturbed_essential(c.pose, 312, deg=1.0, dt=0.05)]
    return _batch("stops", [a.pts, b.pts, c.pts], [4608, 2000, 3000], 4608, E, 1e-3, 1.0, STOPS_REPS)


BLOCK_N = [5, 4096, 4097]


@functools.lru_cache(maxsize=None)
def blocks(n):
    """Case 4: one pair with n_stride = n: one block with 5 and with 4096 points, two with 4097."""
    if n == 5:
        sc = scene(104, noise_px=0.002, outlier_frac=0.0)
        E = perturbed_essential(sc.pose, 204, deg=0.01, dt=0.001)
    else:
        sc = scene(400 + n)
        E = perturbed_essential(sc.pose, 500 + n)
    return _batch(f"blocks({n})", [sc.pts], [n], n, [E], 1e-3, 1.0, 10)


@functools.lru_cache(maxsize=None)
def wrap():
    """Case 5: 256 * 4096 + 257 points, where the grid-stride loop of the 256
    blocks wraps: one scene tiled, every copy of a point jittered by N(0, 1e-4)."""
    sc = scene(600)
    g = torch.Generator().manual_seed(601)
    reps_of_scene = -(-N_WRAP // sc.pts.shape[0])
    pts = np.tile(sc.pts, (reps_of_scene, 1))[:N_WRAP]
    pts = pts + 1e-4 * torch.randn(N_WRAP, 4, generator=g, dtype=torch.float64).numpy()
    return _batch("wrap", [pts], [N_WRAP], N_WRAP, [perturbed_essential(sc.pose, 602)], 1e-3, 1.0, 2)


@functools.lru_cache(maxsize=None)
def wide():
    """Case 6: 65 pairs of 64 points, every pair its own scene; pair 64 is
    initialised by the second block of k_irls_init."""
    sc = [scene(700 + b, noise_px=0.01, outlier_frac=0.05) for b in range(65)]
    E = [perturbed_essential(s.pose, 800 + b, deg=0.1, dt=0.01) for b, s in enumerate(sc)]
    return _batch("wide", [s.pts for s in sc], [64] * 65, 64, E, 1e-3, 1.0, 3, compared=[0, 63, 64])


@functools.lru_cache(maxsize=None)
def empty():
    """Case 7: a pair without points between two ordinary ones."""
    sc = [scene(900), scene(901), scene(902)]
    E = [perturbed_essential(s.pose, 910 + b) for b, s in enumerate(sc)]
    return _batch("empty", [s.pts for s in sc], [300, 0, 77], 300, E, 1e-3, 1.0, 5)


def all_cases():
    return ([ragged(*p) for p in RAGGED_PARAMS] + [stops()] + [blocks(n) for n in BLOCK_N] + [wrap(), wide(), empty()])


def pair_points(case, b):
    return np.ascontiguousarray(case.pts[b, :case.n[b]])


def oracle_pair(case, b, reps=None, order=None):
    """The oracle's E [3, 3] of pair b (optionally with its points reordered, or another max_reps)."""
    p = pair_points(case, b)
    if order is not None:
        p = np.ascontiguousarray(p[order])
    return R.optimise(p[:, :2], p[:, 2:], case.E_init[b], case.delta, case.alpha, case.reps if reps is None else reps)


def rel_dist(got, want):
    """Largest entry-wise difference relative to max |want|."""
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def _expected(name):
    case = {c.name: c for c in all_cases()}[name]
    out = {}
    for b in case.compared:
        n = case.n[b]
        want = oracle_pair(case, b)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1000 + b)).numpy()
        d = max(rel_dist(oracle_pair(case, b, order=np.arange(n)[::-1]), want),
                rel_dist(oracle_pair(case, b, order=perm), want)) if n else 0.0
        out[b] = (want, d)
    return out


def expected(case):
    """{pair: (the oracle's E, d_perm)} for the compared pairs of a case; computed once, shared, never written to."""
    return _expected(case.name)


def check_pair(got, case, b, what=""):
    """Print the figures of pair b, then assert the module's tolerance."""
    want, d = expected(case)[b]
    rel = rel_dist(got, want)
    print({"case": case.name, "pair": b, "n": case.n[b], "what": what, "rel": rel, "d_perm": d, "bound": bound(d)})
    assert np.isfinite(got).all(), (case.name, b, got)
    assert rel <= bound(d), (case.name, b, what, rel, d, bound(d))
    return rel


if __name__ == "__main__":
    for c in all_cases():
        e = expected(c)
        print(f"  {c.name:<22} B={len(c.n):<3} stride={c.n_stride:<8} " +
              "  ".join(f"{b}:{c.n[b]}:{e[b][1]:.1e}" for b in c.compared))
