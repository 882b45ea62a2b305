"""Two-view scenes outside the small-motion regime for the five-point solver
(five_point.h; k_solve_front, k_roots / k_roots_split, k_solve_back in
ransac_solve.hip): tests/test_solver_cases.py checks on the CPU, with the
oracle alone, that they reach the solver branches named below, and
tests/test_gpu_solver_cases.py runs every kernel form on them against the
oracle.

Every other RANSAC test draws its pair from one regime (a rotation of about
0.03 rad with forward translation, or a KITTI-like flow): root counts there are
even, at most a handful of hypotheses have 8 or 10 roots and none has more
than 6 cheirality candidates.  Exactly degenerate motion gives determinant
polynomials with multiple roots, and those are the only inputs that reach
  * the multi-root bisection that ends by writing several coincident roots
    (isolate_r / isolate_p1: `for r = iathi .. iatlo` at the iteration limit);
  * nodes dropped at kMaxDepth and nodes where modrf fails (bisect_deferred);
  * odd root counts, and root and candidate slots 7..9 of hypE / hypP.

Each case is (q, qp, params): float64 normalised coordinates [N, 2] with
N <= 640, params = dict(iters, thr, seed); iters is 1 or 2 (512 or 1024
hypotheses), thr 1e-3, seed the library's default.  Everything is generated
from fixed numpy seeds.

  zero_motion          qp = q, q uniform in [-0.8, 0.8]^2
  pure_rotation_exact  random depths, rotation 0.1 rad, t = 0, no noise
  pure_rotation_noisy  the same with 1e-4 noise
  planar_exact         points of one tilted plane, general motion, no noise
  planar_noisy         the same with 5e-4 noise
  grid_shift           30 x 20 grid, spacing 1/32, qp = q + (1/64, 0): every
                       coordinate exactly representable
  sideways_baseline    R = I, t = (1, 0, 0): the epipole at infinity; 10 % outliers
  large_rotation       rotation vector (0.3, -0.9, 0.5), oblique t; 10 % outliers
  scaled_up / _down    a geometric_scene times 1e3 / 1e-3 (coordinate range,
                       not degenerate)
  collinear            every point of the first image on one line
  half_duplicates      300 distinct correspondences, each present twice: many
                       samples repeat a point (rank-deficient null spaces,
                       NaN solves)
  tiny_n5 / 6 / 8      the first 5, 6, 8 points of zero_motion: the sampler
                       repeats indices

ragged() stacks six of them with different N into one [B, n_max, 4] batch
(NaN rows past each pair's n).

`python -m tests.solver_cases` prints, per case, the oracle's root-count
histogram (hypotheses with 0..10 real roots), the largest cheirality
candidate count and the root isolation's branch counters
(oracle.ransac5.isolate_stats).  The oracle here gives (N, H; roots 0..10;
largest candidate count):

  zero_motion          640,  512   2/0/16/11/96/27/189/34/111/4/22        10
  pure_rotation_exact  587, 1024   19/1/32/27/176/105/299/96/212/16/41     9
  pure_rotation_noisy  600,  512   2/0/57/0/206/0/180/0/58/0/9             8
  planar_exact         500, 1024   0/0/65/0/442/0/516/0/1/0/0              6
  planar_noisy         500, 1024   1/0/188/0/525/0/310/0/0/0/0             6
  grid_shift           600,  512   1/0/18/0/218/1/274/0/0/0/0              6
  sideways_baseline    640, 1024   2/0/138/0/473/0/372/0/30/0/9            5
  large_rotation       560, 1024   2/0/99/0/520/0/343/0/49/0/11            7
  scaled_up            600,  512   2/0/182/0/288/0/40/0/0/0/0              3
  scaled_down          600,  512   1/0/43/0/204/0/264/0/0/0/0              6
  collinear            320, 1024   20/0/541/0/152/0/289/0/22/0/0           6
  half_duplicates      600, 1024   9/0/172/0/539/0/298/0/5/0/1             6
  tiny_n5                5,  512   103/0/87/1/239/2/63/0/17/0/0            6
  tiny_n6                6,  512   80/0/68/7/230/4/111/0/11/0/1            7
  tiny_n8                8,  512   74/0/59/6/205/6/128/4/19/1/10          10

The seeds of zero_motion and pure_rotation_exact were chosen so that each
ends one multi-root bisection by writing coincident roots, and all of them so
that no Sturm sequence is non-monotone (no root slot outside [0, 10), at most
10 single-root nodes per solve, no node at kMaxDepth): the GPU's split
isolation does not guard those ("Degenerate two-view geometry"),
and tests/test_solver_cases.py keeps it so.  A seed that changes must keep
both properties and the floors of that test.
"""
import functools

import numpy as np

THR = 1e-3
SEED = 1234
N_MAX = 640

EXACT = ("zero_motion", "pure_rotation_exact")
TIE_SATURATED = ("zero_motion", "grid_shift", "pure_rotation_exact")
RAGGED = ("zero_motion", "pure_rotation_exact", "half_duplicates", "collinear", "tiny_n5", "planar_exact")
RAGGED_ITERS = 1


def _rot(w):
    """Rodrigues: the rotation matrix of rotation vector w."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * K @ K


def _project(X):
    return X[:, :2] / X[:, 2:]


def _points(rng, n, depth=(2.0, 40.0)):
    q = rng.uniform(-0.8, 0.8, (n, 2))
    return np.c_[q, np.ones(n)] * rng.uniform(depth[0], depth[1], (n, 1))


def _outliers(rng, qp, frac):
    m = int(len(qp) * frac)
    idx = rng.choice(len(qp), m, replace=False)
    qp[idx] = rng.uniform(-0.8, 0.8, (m, 2))
    return qp


def _params(iters):
    return dict(iters=int(iters), thr=THR, seed=SEED)


def zero_motion():
    rng = np.random.default_rng(191)
    q = rng.uniform(-0.8, 0.8, (640, 2))
    return q, q.copy(), _params(1)


def _pure_rotation(seed, n, noise):
    rng = np.random.default_rng(seed)
    X = _points(rng, n)
    w = rng.normal(0.0, 1.0, 3)
    Rm = _rot(0.1 * w / np.linalg.norm(w))
    qp = _project(X @ Rm.T)
    if noise:
        qp = qp + rng.normal(0.0, noise, (n, 2))
    return _project(X), qp


def pure_rotation_exact():
    q, qp = _pure_rotation(201, 587, 0.0)
    return q, qp, _params(2)


def pure_rotation_noisy():
    q, qp = _pure_rotation(315, 600, 1e-4)
    return q, qp, _params(1)


def _planar(seed, n, noise):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-0.8, 0.8, (n, 2))
    nrm = np.array([0.2, -0.1, 1.0])
    z = 5.0 / (np.c_[q, np.ones(n)] @ nrm)          # nrm . X = 5
    X = np.c_[q, np.ones(n)] * z[:, None]
    X2 = X @ _rot(rng.normal(0.0, 0.05, 3)).T + np.array([0.3, -0.1, 0.2])
    qp = _project(X2)
    if noise:
        qp = qp + rng.normal(0.0, noise, (n, 2))
    return q, qp


def planar_exact():
    q, qp = _planar(404, 500, 0.0)
    return q, qp, _params(2)


def planar_noisy():
    q, qp = _planar(505, 500, 5e-4)
    return q, qp, _params(2)


def grid_shift():
    i, j = np.meshgrid(np.arange(30), np.arange(20), indexing="ij")
    q = np.stack([(i.ravel() - 15) / 32.0, (j.ravel() - 10) / 32.0], 1)
    return q, q + np.array([1.0 / 64.0, 0.0]), _params(1)


def sideways_baseline():
    rng = np.random.default_rng(606)
    X = _points(rng, 640)
    qp = _project(X + np.array([1.0, 0.0, 0.0])) + rng.normal(0.0, 2e-4, (640, 2))
    return _project(X), _outliers(rng, qp, 0.10), _params(2)


def large_rotation():
    rng = np.random.default_rng(707)
    n = 560
    X = _points(rng, 6 * n)
    X2 = X @ _rot([0.3, -0.9, 0.5]).T + np.array([0.5, 0.3, -0.4])
    keep = np.flatnonzero(X2[:, 2] > 0.5)[:n]      # in front of the second camera too
    assert len(keep) == n
    qp = _project(X2[keep]) + rng.normal(0.0, 2e-4, (n, 2))
    return _project(X[keep]), _outliers(rng, qp, 0.10), _params(2)


def _scene(seed, n):
    from oracle.gen_golden import geometric_scene
    return geometric_scene(np.random.default_rng(seed), n)


def scaled_up():
    q, qp = _scene(808, 600)
    return q * 1e3, qp * 1e3, _params(1)


def scaled_down():
    q, qp = _scene(808, 600)
    return q * 1e-3, qp * 1e-3, _params(1)


def collinear():
    q, qp = _scene(909, 320)
    q = np.stack([q[:, 0], 0.5 * q[:, 0] + 0.1], 1)
    return q, qp, _params(2)


def half_duplicates():
    q, qp = _scene(1010, 300)
    return np.concatenate([q, q]), np.concatenate([qp, qp]), _params(2)


def _tiny(n):
    q, qp, _ = zero_motion()
    return q[:n].copy(), qp[:n].copy(), _params(1)


BUILDERS = dict(zero_motion=zero_motion, pure_rotation_exact=pure_rotation_exact,
                pure_rotation_noisy=pure_rotation_noisy, planar_exact=planar_exact, planar_noisy=planar_noisy,
                grid_shift=grid_shift, sideways_baseline=sideways_baseline, large_rotation=large_rotation,
                scaled_up=scaled_up, scaled_down=scaled_down, collinear=collinear, half_duplicates=half_duplicates,
                tiny_n5=lambda: _tiny(5), tiny_n6=lambda: _tiny(6), tiny_n8=lambda: _tiny(8))
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(q, qp, params) of the named case (built once; treat as read-only)."""
    q, qp, params = BUILDERS[name]()
    q = np.ascontiguousarray(q, np.float64)
    qp = np.ascontiguousarray(qp, np.float64)
    assert q.shape == qp.shape and q.shape[1] == 2 and 5 <= len(q) <= N_MAX, name
    assert params["iters"] in (1, 2) and np.isfinite(q).all() and np.isfinite(qp).all(), name
    q.setflags(write=False)
    qp.setflags(write=False)
    return q, qp, params


@functools.lru_cache(maxsize=None)
def oracle(name, cheir, iters=None, use_ref=False):
    """oracle.ransac5 on the case (computed once, shared; treat as read-only).
    ``iters`` overrides the case's own (the ragged batch runs every member at
    RAGGED_ITERS)."""
    from oracle import ransac5 as R
    q, qp, p = case(name)
    n = len(q)
    return R.ransac5(q, qp, n, n, p["iters"] if iters is None else iters, p["thr"], seed=p["seed"], cheir=bool(cheir),
                     use_ref=use_ref)


@functools.lru_cache(maxsize=None)
def ragged():
    """(pts [B, n_max, 4] with NaN rows past n[b], n, params, names): six cases
    with different N in one batch."""
    cs = [case(k) for k in RAGGED]
    n = [len(c[0]) for c in cs]
    assert len(set(n)) == len(n)
    pts = np.full((len(cs), max(n), 4), np.nan)
    for b, (q, qp, _) in enumerate(cs):
        pts[b, :n[b]] = np.c_[q, qp]
    pts.setflags(write=False)
    return pts, n, _params(RAGGED_ITERS), RAGGED


def branch_stats(name, iters=None):
    """The oracle's root-isolation branch counters (oracle.ransac5.isolate_stats)
    over one run of the case.  Not thread-safe against other oracle calls."""
    from oracle import ransac5 as R
    q, qp, p = case(name)
    R.isolate_stats(reset=True)
    R.ransac5(q, qp, len(q), len(q), p["iters"] if iters is None else iters, p["thr"], seed=p["seed"], cheir=False)
    return R.isolate_stats(reset=True)


def root_histogram(name):
    """Hypotheses with 0..10 real roots (the oracle without cheirality)."""
    return np.bincount(oracle(name, False)["hyp_ncand"], minlength=11)


if __name__ == "__main__":
    for k in NAMES:
        q, _, p = case(k)
        st = branch_stats(k)
        print(f"{k:20s} N={len(q):4d} H={512 * p['iters']:5d}  roots 0..10: "
              f"{'/'.join(str(v) for v in root_histogram(k))}  max candidates {int(oracle(k, True)['hyp_ncand'].max())}"
              f"  winner {oracle(k, True)['winner']} inliers {oracle(k, True)['inliers']}"
              f"  isolation {'/'.join(str(st[s]) for s in st)}")
