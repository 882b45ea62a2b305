"""The IRLS batches of tests/irls_cases.py, checked on the CPU: the cases are
what they claim, the oracle's own order sensitivity d_perm is under the limit
for every pair that the GPU test compares tightly, and the stop cases stop
where they should."""
import numpy as np
import pytest

from tests import irls_cases as IC


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in IC.all_cases()}


def test_shapes_reach_every_launch_shape(cases):
    r = IC.ragged(*IC.RAGGED_PARAMS[0])
    assert r.n == [4608, 4097, 257, 64, 5] and r.n_stride == 4608 and r.pts.shape == (5, 4608, 4)
    assert [IC.blocks(n).n_stride for n in IC.BLOCK_N] == [5, 4096, 4097]
    assert IC.wrap().n == [256 * 4096 + 257] and IC.wrap().n_stride == IC.N_WRAP
    w = IC.wide()
    assert len(w.n) == 65 and w.n_stride == 64 and w.compared == [0, 63, 64]
    assert IC.empty().n[1] == 0
    assert {(c.delta, c.alpha, c.reps) for c in map(lambda p: IC.ragged(*p), IC.RAGGED_PARAMS)} == \
        {(1e-3, 1.0, 30), (1e-3, 0.0, 8), (2e-3, 0.5, 0)}


def test_padding_rows_are_nan_and_points_are_finite(cases):
    for c in cases.values():
        for b, n in enumerate(c.n):
            assert np.isfinite(c.pts[b, :n]).all(), (c.name, b)
            assert np.isnan(c.pts[b, n:]).all(), (c.name, b)
        assert np.isfinite(c.E_init).all()


def test_every_pair_is_its_own_scene(cases):
    for name in ("ragged(0.001,1,30)", "wide", "empty", "stops"):
        c = cases[name]
        B = len(c.n)
        m = min(v for v in c.n if v > 0)
        for a in range(B):
            for b in range(a + 1, B):
                assert not np.array_equal(c.E_init[a], c.E_init[b]), (name, a, b)
                if c.n[a] and c.n[b]:
                    assert not np.array_equal(c.pts[a, :m], c.pts[b, :m]), (name, a, b)


def test_d_perm_is_under_the_limit(cases):
    """The condition on the cases: the oracle's own E moves by at most 1e-8
    relative when its sums run in another order, for every compared pair."""
    for c in cases.values():
        for b, (want, d) in IC.expected(c).items():
            print(c.name, b, c.n[b], d)
            assert np.isfinite(want).all(), (c.name, b)
            assert d <= IC.D_PERM_MAX, (c.name, b, d)
            assert IC.bound(d) <= IC.PROJECT_BAR


def test_the_tiled_scene_is_jittered():
    c = IC.wrap()
    p = c.pts[0]
    assert not np.array_equal(p[:4608], p[4608:9216]) and np.abs(p[:4608] - p[4608:9216]).max() < 1e-3


def test_stop_case_stops_where_it_should():
    c = IC.stops()
    assert c.reps == IC.STOPS_REPS
    # the exact pair at the exact E: |g|^2 < 1e-20 at repetition 0, the Givens-reduced E_init comes back
    assert np.array_equal(IC.oracle_pair(c, 0, reps=0), IC.oracle_pair(c, 0, reps=50))
    assert not np.array_equal(IC.oracle_pair(c, 0, reps=0), IC.oracle_pair(c, 1, reps=0))
    p = IC.pair_points(c, 0)
    E = c.E_init[0] / np.abs(c.E_init[0]).max()
    r = np.einsum("ni,ij,nj->n", np.c_[p[:, 2:], np.ones(len(p))], E, np.c_[p[:, :2], np.ones(len(p))])
    assert np.abs(r).max() < 1e-14
    # a pair that moves away from its start does not return the reduced E_init
    moved = IC.oracle_pair(c, 1, reps=0)
    assert IC.rel_dist(moved, IC.oracle_pair(c, 1)) > 1e-4
    # the converging pair: the result stops changing before max_reps
    assert np.array_equal(IC.oracle_pair(c, 1, reps=c.reps - 2), IC.oracle_pair(c, 1, reps=50))
    assert np.array_equal(IC.oracle_pair(c, 1, reps=c.reps - 2), IC.expected(c)[1][0])
    # the noisy pair: still moving at max_reps
    assert IC.rel_dist(IC.oracle_pair(c, 2, reps=c.reps - 1), IC.expected(c)[2][0]) > 1e-6
    assert IC.rel_dist(IC.oracle_pair(c, 2, reps=c.reps + 1), IC.expected(c)[2][0]) > 1e-6


def test_oracle_accepts_an_empty_pair():
    """n = 0: zero sums, the stop at repetition 0, the Givens-reduced E_init."""
    c = IC.empty()
    want, d = IC.expected(c)[1]
    assert d == 0.0 and np.isfinite(want).all()
    assert np.array_equal(want, IC.oracle_pair(c, 1, reps=0))


def test_check_pair_refuses_a_neighbouring_pair_and_a_small_error():
    c = IC.ragged(*IC.RAGGED_PARAMS[0])
    e = IC.expected(c)
    IC.check_pair(e[0][0], c, 0)
    with pytest.raises(AssertionError):
        IC.check_pair(e[1][0], c, 0)
    with pytest.raises(AssertionError):
        IC.check_pair(e[0][0] * (1 + 1e-11), c, 0)
    # one repetition short is outside the bar wherever the pair is still moving
    s = IC.stops()
    with pytest.raises(AssertionError):
        IC.check_pair(IC.oracle_pair(s, 2, reps=s.reps - 1), s, 2)
