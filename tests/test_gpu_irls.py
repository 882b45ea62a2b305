"""sfm_essential_optimise_batched (csrc/irls.hip) on ragged, wide and
degenerate batches (tests/irls_cases.py) against the float64 oracle, and the
batch independence of a pair's result, bit for bit.

Bar: max(8 d_perm, 1e-12) relative on E and never over 1e-4 (irls_cases.py
says where d_perm comes from; tests/test_irls_cases.py checks the cases).

Measured GPU-to-oracle distances (largest entry-wise difference relative to
max |E|, MI355X), per compared pair:

  ragged (1e-3, 1, 30)   4.0e-16  7.3e-17  2.2e-16  6.6e-16  3.9e-15   (pairs 0 .. 4)
  ragged (1e-3, 0, 8)    2.2e-16  5.0e-16  4.8e-16  2.9e-16  3.9e-15
  ragged (2e-3, 0.5, 0)  0 for every pair
  stops                  0        2.1e-16  6.2e-16
  blocks                 5: 3.9e-15   4096: 3.2e-16   4097: 1.1e-16
  wrap                   7.7e-15  (d_perm there 3.4e-14)
  wide                   0: 5.5e-16   63: 9.0e-16   64: 7.9e-16
  empty                  2.2e-16  0        2.1e-15

Every distance is of the size of that pair's d_perm, three orders under the
1e-12 floor of the bar.
"""
import numpy as np
import pytest
import torch

from tests import irls_cases as IC

pytestmark = pytest.mark.gpu


def _run(cuda, case, idx=None, reps=None, workspace=None):
    """The GPU's E [len(idx), 3, 3] (numpy) for the pairs ``idx`` of a case, in that order, as one batch."""
    from sfm_amd import ransac
    idx = list(range(len(case.n))) if idx is None else list(idx)
    pts = torch.from_numpy(np.ascontiguousarray(case.pts[idx])).to(cuda)
    E0 = torch.from_numpy(np.ascontiguousarray(case.E_init[idx])).to(cuda)
    out = ransac.optimise_batched(pts, E0, case.delta, case.alpha, case.reps if reps is None else reps,
                                  n=[case.n[b] for b in idx], workspace=workspace)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _workspace(cuda, B, n_stride):
    from sfm_amd import _lib
    nb = _lib.load().sfm_essential_optimise_workspace_bytes(B, n_stride)
    return torch.empty(int(nb), dtype=torch.uint8, device=cuda)


@pytest.mark.parametrize("params", IC.RAGGED_PARAMS, ids=lambda p: f"{p[0]:g}-{p[1]:g}-{p[2]}")
def test_ragged_batch_matches_oracle(cuda, params):
    c = IC.ragged(*params)
    got = _run(cuda, c)
    for b in c.compared:
        IC.check_pair(got[b], c, b)


@pytest.mark.parametrize("params", IC.RAGGED_PARAMS, ids=lambda p: f"{p[0]:g}-{p[1]:g}-{p[2]}")
def test_pair_is_independent_of_its_batch(cuda, params):
    """Alone, inside the batch, as the last pair of a batch in another order,
    and twice on one workspace that another batch used in between: the same
    nine doubles (the reduction order is fixed by design)."""
    c = IC.ragged(*params)
    B = len(c.n)
    batch = _run(cuda, c)
    ws = _workspace(cuda, B, c.n_stride)
    first = _run(cuda, c, workspace=ws)
    other = IC.ragged(*IC.RAGGED_PARAMS[1 if params == IC.RAGGED_PARAMS[0] else 0])
    _run(cuda, other, idx=[4, 3, 2, 1, 0], workspace=ws)
    again = _run(cuda, c, workspace=ws)
    assert np.array_equal(_bits(batch), _bits(first)) and np.array_equal(_bits(batch), _bits(again))
    for b in range(B):
        alone = _run(cuda, c, idx=[b])
        assert np.array_equal(_bits(alone[0]), _bits(batch[b])), (b, alone[0], batch[b])
        order = [k for k in reversed(range(B)) if k != b] + [b]
        last = _run(cuda, c, idx=order)
        assert np.array_equal(_bits(last[-1]), _bits(batch[b])), (b, order)
        for pos, k in enumerate(order):
            assert np.array_equal(_bits(last[pos]), _bits(batch[k])), (b, order, pos)


def test_pairs_that_stop_at_different_repetitions(cuda):
    c = IC.stops()
    got = _run(cuda, c)
    for b in c.compared:
        IC.check_pair(got[b], c, b)
    zero = _run(cuda, c, reps=0)
    assert np.array_equal(_bits(got[0]), _bits(zero[0]))           # stopped at repetition 0: the reduced E_init
    assert not np.array_equal(_bits(got[1]), _bits(zero[1]))
    long = _run(cuda, c, reps=50)                                   # the converged pair stays where it stopped
    assert np.array_equal(_bits(got[0]), _bits(long[0])) and np.array_equal(_bits(got[1]), _bits(long[1]))
    assert not np.array_equal(_bits(got[2]), _bits(long[2]))
    for b in range(3):
        assert np.array_equal(_bits(_run(cuda, c, idx=[b])[0]), _bits(got[b])), b


@pytest.mark.parametrize("n", IC.BLOCK_N)
def test_block_count_steps(cuda, n):
    c = IC.blocks(n)
    IC.check_pair(_run(cuda, c)[0], c, 0)


def test_grid_stride_wrap(cuda):
    c = IC.wrap()
    IC.check_pair(_run(cuda, c)[0], c, 0)


def test_wide_batch(cuda):
    c = IC.wide()
    got = _run(cuda, c)
    assert np.isfinite(got).all()
    for b in c.compared:
        IC.check_pair(got[b], c, b)
    for b in (63, 64):
        assert np.array_equal(_bits(_run(cuda, c, idx=[b])[0]), _bits(got[b])), b
    assert len({got[b].tobytes() for b in range(65)}) == 65


def test_empty_pair(cuda):
    c = IC.empty()
    got = _run(cuda, c)
    assert np.isfinite(got).all()
    for b in range(3):
        assert np.array_equal(_bits(_run(cuda, c, idx=[b])[0]), _bits(got[b])), b
        IC.check_pair(got[b], c, b)
