"""The degenerate two-view scenes of tests/solver_cases.py, checked on the CPU
with the oracle alone: they reach the solver states the small-motion scenes
never do (odd and full root counts, 8 or more cheirality candidates, the
coincident-root end of the multi-root bisection, hypotheses with no root), and
they stay inside the range in which the GPU's split root isolation is defined
(monotone sign-change counts, every root slot in [0, 10)).  Where the
reference's own solver is built (oracle/_ref), the oracle equals it on every
case."""
import ctypes

import numpy as np
import pytest

from oracle import ransac5 as R
from tests import solver_cases as SC


def test_cases_are_what_they_claim():
    assert len(SC.NAMES) == 15 and set(SC.EXACT + SC.TIE_SATURATED + SC.RAGGED) <= set(SC.NAMES)
    for k in SC.NAMES:
        q, qp, p = SC.case(k)
        assert q.dtype == np.float64 and qp.dtype == np.float64 and q.shape == qp.shape
        assert 5 <= len(q) <= 640 and p["iters"] in (1, 2) and p["thr"] == 1e-3
    q, qp, _ = SC.case("zero_motion")
    assert np.array_equal(q, qp) and float(np.abs(q).max()) <= 0.8
    q, qp, _ = SC.case("grid_shift")
    assert len(q) == 600 and np.array_equal(q * 64, np.round(q * 64)) and np.array_equal(qp - q, [[1 / 64, 0]] * 600)
    q, qp, _ = SC.case("collinear")
    assert float(np.abs(q[:, 1] - (0.5 * q[:, 0] + 0.1)).max()) < 1e-15
    q, qp, _ = SC.case("half_duplicates")
    assert np.array_equal(q[:300], q[300:]) and np.array_equal(qp[:300], qp[300:])
    assert len(np.unique(np.c_[q, qp], axis=0)) == 300
    assert [len(SC.case(k)[0]) for k in ("tiny_n5", "tiny_n6", "tiny_n8")] == [5, 6, 8]
    up, down = SC.case("scaled_up"), SC.case("scaled_down")
    assert 50.0 < float(np.abs(up[0]).max()) and float(np.abs(down[0]).max()) < 1e-3
    pts, n, p, names = SC.ragged()
    assert pts.shape == (6, 640, 4) and len(set(n)) == 6 and p["iters"] == SC.RAGGED_ITERS
    for b, k in enumerate(names):
        assert np.array_equal(pts[b, :n[b]], np.c_[SC.case(k)[0], SC.case(k)[1]]) and np.isnan(pts[b, n[b]:]).all()


def test_exact_cases_reach_full_and_odd_root_counts():
    """Without cheirality hyp_ncand is the root count."""
    union = np.zeros(11, np.int64)
    for k in SC.EXACT:
        h = SC.root_histogram(k)
        print(k, "hypotheses with 0..10 roots:", "/".join(str(v) for v in h))
        assert h[10] >= 8, (k, h)
        assert h[1::2].sum() >= 8, (k, h)
        union += h
    assert (union[1:] > 0).all(), union


def test_exact_cases_reach_eight_candidates():
    for k in SC.EXACT:
        m = int(SC.oracle(k, True)["hyp_ncand"].max())
        print(k, "largest candidate count:", m)
        assert m >= 8, (k, m)


def test_noisy_rotation_reaches_ten_roots():
    h = SC.root_histogram("pure_rotation_noisy")
    assert h[10] >= 4, h


def test_degenerate_samples_give_rootless_hypotheses():
    for k in ("half_duplicates", "collinear"):
        assert SC.root_histogram(k)[0] >= 1, k


def test_isolation_branches_reached_and_slots_in_range():
    """The exact cases end a multi-root bisection by writing coincident roots,
    every case has nodes where regula falsi fails (sbisect's bisection), and
    no case (at its own iteration count, which includes the ragged batch's
    hypotheses) has a non-monotone Sturm sequence: a root slot outside
    [0, 10), more than 10 single-root nodes or a node at kMaxDepth.  The oracle
    drops such writes; the GPU's split isolation (isolate_p1 / falsi_tasks)
    indexes its LDS root table and task list without that test, so scenes that
    produce them are kept out of the GPU tests ("Degenerate
    two-view geometry")."""
    for k in SC.NAMES:
        st = SC.branch_stats(k)
        print(k, st)
        assert st["falsi_fail"] >= 1, k
        for key in ("depth_drop", "non_monotone", "slot_range", "many_nodes"):
            assert st[key] == 0, (k, key, st)
        if k in SC.EXACT:
            assert st["coincident"] >= 1, (k, st)
    assert SC.RAGGED_ITERS <= min(SC.case(k)[2]["iters"] for k in SC.RAGGED)   # a prefix of the same hypotheses


@pytest.mark.parametrize("cheir", [True, False])
@pytest.mark.parametrize("name", SC.NAMES)
def test_oracle_equals_reference_solver(name, cheir):
    if not R.ref_available():
        pytest.skip("oracle/_ref not built")
    a, b = SC.oracle(name, cheir), SC.oracle(name, cheir, use_ref=True)
    assert np.array_equal(a["hyp_score"], b["hyp_score"])
    assert np.array_equal(a["hyp_ncand"], b["hyp_ncand"])
    assert a["winner"] == b["winner"] and a["inliers"] == b["inliers"]
    assert a["E"].tobytes() == b["E"].tobytes()
    assert a["P"].tobytes() == b["P"].tobytes()


def test_hypothesis_counts_validates_arguments():
    """sfm_ransac5_hypothesis_counts refuses null pointers, a bad batch and a
    workspace that is too small before any device call (no GPU here)."""
    from sfm_amd import _lib
    lib = _lib.load()
    v = ctypes.c_void_p(8)
    need = lib.sfm_ransac5_workspace_bytes(2, 0, 1)
    assert lib.sfm_ransac5_hypothesis_counts(None, need, 2, 1, v, v) == 1
    assert lib.sfm_ransac5_hypothesis_counts(v, need, 2, 1, None, v) == 1
    assert lib.sfm_ransac5_hypothesis_counts(v, need, 2, 1, v, None) == 1
    assert lib.sfm_ransac5_hypothesis_counts(v, need, 0, 1, v, v) == 1
    assert lib.sfm_ransac5_hypothesis_counts(v, need, 65, 1, v, v) == 1
    assert lib.sfm_ransac5_hypothesis_counts(v, need, 2, 0, v, v) == 1
    assert lib.sfm_ransac5_hypothesis_counts(v, need - 1, 2, 1, v, v) == 1 and b"workspace" in lib.sfm_last_error()
