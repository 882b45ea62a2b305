"""The pose-case table of tests/sweep_pose_cases.py, checked on the CPU: the
cases are what their names say, the classifier separates what it should, and
check_warped accepts the kernels' arithmetic restated on the CPU
(written_order_warped) and refuses it with the Z clamp taken out."""
import pytest
import torch

from tests import sweep_pose_cases as PC

H, W, L = 24, 78, 16


@pytest.fixture(scope="module")
def rows():
    return {name: PC.table_row(name, H, W, L) for name in PC.CASES}


def test_in_range_counts(rows):
    """The in-range counts at 24x78, L = 16, by the kernels' written-order
    float32 arithmetic (elementwise operations: the same on every CPU).  The
    oracle's bmm rounds as the CPU's sgemm does: where that is the written
    order the oracle counts the same, elsewhere (measured: 29,484 for
    identity_zero_t, 381 exact-border samples the other way) it may differ,
    but only inside the ambiguous set."""
    for name, n in PC.IN_RANGE_24x78.items():
        assert rows[name]["in_range_written_order"] == n, (name, rows[name])
    for name, r in rows.items():
        assert r["flips_unambiguous"] == 0, r
        assert r["flips"] <= round(r["ambiguous"] * r["samples"]), r
        if r["ambiguous"] == 0:
            assert r["in_range"] == r["in_range_written_order"], r
    per_pair = PC.classify(PC.scene("mixed_batch", H, W), L).in32.flatten(1).sum(1).tolist()
    assert per_pair[1:] == [rows["roll_180"]["in_range"], rows["yaw_90"]["in_range"]] and per_pair[0] > 0, per_pair


def test_ambiguous_shares(rows):
    for name, r in rows.items():
        if name in ("identity_zero_t", "zero_x"):
            assert r["ambiguous"] > 0, r
        else:
            assert r["ambiguous"] <= 0.01, r


def test_cases_cover_the_regimes(rows):
    assert any(r["in_range"] == 0 for r in rows.values())
    assert rows["clamped_in_range"]["clamped_in_range_per_plane"] >= 50, rows["clamped_in_range"]
    assert 0 < rows["forward_big_t"]["clamped"] < 1 and rows["forward_big_t"]["in_range"] > 0
    assert rows["clamped_in_range"]["delta"] > 0


def test_huge_t_is_beyond_the_gate():
    c = PC.classify(PC.scene("huge_t", H, W), L)
    assert float(c.X32.abs().min()) > 2.0 ** 60 and bool(torch.isfinite(c.X32).all())


def test_zero_x_is_exactly_zero_in_column_0():
    sc = PC.scene("zero_x", H, W)
    c = PC.classify(sc, L)
    assert bool((c.X32[..., 0] == 0).all())
    assert bool((c.xn32[..., 0] == -1).all()) and bool(c.ambiguous[..., 0].all())
    xn, _ = PC.written_order_coords(sc, L)
    assert bool((xn[..., 0] == -1).all())


@pytest.mark.parametrize("name", PC.CASES)
def test_checker_accepts_the_written_order(name):
    sc = PC.scene(name, H, W)
    exp = PC.expected_warped(sc, L)
    PC.check_warped(exp.want, exp, name)
    # the restatement's coordinates are within the guard of the oracle's: its samples within guard x tap spread
    PC.check_warped(PC.written_order_warped(sc, L), exp, name, pos_tol=exp.cls.guard_px)


def test_checker_refuses_a_missing_clamp_a_channel_mix_and_a_wrong_pair():
    sc = PC.scene("clamped_in_range", H, W)
    exp = PC.expected_warped(sc, L)
    with pytest.raises(AssertionError):
        PC.check_warped(PC.written_order_warped(sc, L, z_clamp=0.0), exp, pos_tol=exp.cls.guard_px)
    # an ambiguous sample zero in one channel and the alternative in the others
    sc = PC.scene("identity_zero_t", H, W)
    exp = PC.expected_warped(sc, L)
    got = exp.alt.clone()
    b, l, y, x = exp.cls.ambiguous.nonzero()[0].tolist()
    PC.check_warped(got, exp)
    got[b, 3, l, y, x] = 0.0
    with pytest.raises(AssertionError):
        PC.check_warped(got, exp)
    # the pairs of a batch swapped: every pair read another pair's Proj
    sc = PC.scene("mixed_batch", H, W)
    exp = PC.expected_warped(sc, L)
    with pytest.raises(AssertionError):
        PC.check_warped(exp.want.roll(1, 0), exp)
