"""The store rider: TwoViewHotPath.step hands the cost volume's reference half
(cost[:, :C, l] = ref, PSNet.py:155) to the RANSAC call (sfm_score_ref_job),
whose one-sided scorer launch writes it from its own waves while HBM is idle;
the sweep then writes the warped half alone.  The volume and the RANSAC
outputs must be those of the one-launch sweep (score_ref_rider = 0) bit for
bit, on every path: the rider's fast path, its fallbacks (odd shapes, sparse
keypoints, short pairs), a copy longer than the scorer and the reverse; and
the job is one-shot and scoped to its stream.

Dense pairs of 200 x 220 with margin 10 have 36,000 points = 36 spans, the
smallest size at which the pruned scorer (pairs of >= 32 spans) runs."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

IMG = (200, 220)


@pytest.fixture
def rider_key():
    """Leaves the switch as it found it."""
    from sfm_amd import _lib
    old = _lib.tune_get("score_ref_rider")
    yield
    _lib.tune("score_ref_rider", old)


def _inputs(cuda, B, C, fhw, seed, img=IMG):
    from sfm_amd import synth
    flow, K, _, _ = synth.kitti_pair_batch(B, seed=seed, hw=img, device=cuda)
    ref, tgt = synth.features(B, C, *fhw, seed=seed, device=cuda)
    return flow, K, ref, tgt


def _hot(cuda, B, C, L, fhw, iters, dtype=torch.float32, img=IMG, **kw):
    from sfm_amd.pipeline import TwoViewHotPath
    return TwoViewHotPath(B, img, fhw, C, L, iters, 1e-4, 1.0, True, 0.6, cost_dtype=dtype, device=cuda, **kw)


def _both(cuda, B, C, L, fhw, iters, dtype, seed, fused=False):
    """(outputs with the one-launch sweep, outputs with the rider, rode): the
    same inputs through step with the switch off and on; every element of the
    volume must be written by the step (NaN fill)."""
    from sfm_amd import _lib
    args = _inputs(cuda, B, C, fhw, seed)
    outs = []
    for key in (0, 1):
        _lib.tune("score_ref_rider", key)
        hp = _hot(cuda, B, C, L, fhw, iters, dtype, fused=fused)
        assert hp.ref_rider() == bool(key)
        hp.cost.fill_(float("nan"))
        E, P, inl, cost = hp.step(*args)
        torch.cuda.synchronize()
        assert _lib.last_scorer() == "k_score_mf2+prune"
        assert _lib.load().sfm_score_ref_jobs_armed() == 0
        outs.append((E.clone(), P.clone(), inl.clone(), cost.clone()))
    return outs


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not bool(torch.isnan(a[3].float()).any())
    assert torch.equal(a[3], b[3])                       # both halves


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fused", [False, True])
def test_rider_volume_bit_identical(cuda, rider_key, dtype, fused):
    """1. hw = 2750 (hw % 4 == 2: periods of two planes), more than one chunk
    per period and a partial last chunk; packed and fused-flow sources."""
    a, b = _both(cuda, 2, 32, 8, (50, 55), 2, dtype, 41, fused)
    _same(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_odd_shapes_fall_back_and_match(cuda, rider_key, dtype):
    """2. hw = 2491 is odd: outside the rider's fast path, the RANSAC call
    writes the half with the reference kernels instead."""
    a, b = _both(cuda, 2, 2, 3, (47, 53), 2, dtype, 42)
    _same(a, b)


def test_copy_outlasts_the_scorer(cuda, rider_key):
    """3. 512 hypotheses against a 117 MB reference half: many pieces per run."""
    a, b = _both(cuda, 1, 32, 64, (94, 78), 1, torch.float32, 43)
    _same(a, b)


def test_scorer_outlasts_the_copy(cuda, rider_key):
    """4. 4096 hypotheses against a 44 KB reference half: most runs carry no
    piece (L = 2 with hw % 4 == 2: one period per slab)."""
    a, b = _both(cuda, 2, 2, 2, (50, 55), 8, torch.float32, 44)
    _same(a, b)


def test_ransac_outputs_unchanged(cuda, rider_key):
    """5. E, P, inlier counts and winners with a job armed and without, on the
    same inputs; the scorer is still the pruned matrix-core one."""
    from sfm_amd import _lib, ransac
    B, C, L, fhw = 2, 4, 4, (50, 56)
    flow, K, ref, _ = _inputs(cuda, B, C, fhw, 45)
    hp = _hot(cuda, B, C, L, fhw, 2)
    Kinv = hp.k_inverse(K)
    plain = [t.clone() for t in hp.pose(flow, K, Kinv)]
    assert _lib.last_scorer() == "k_score_mf2+prune"
    cost = torch.full((B, 2 * C, L, *fhw), 7.0, device=cuda)
    assert _lib.load().sfm_score_ref_job(_lib.stream_ptr(cuda), _lib.ptr(ref), _lib.ptr(cost), B, C, L, *fhw, 0) == 0
    rode = [t.clone() for t in hp.pose(flow, K, Kinv)]
    torch.cuda.synchronize()
    assert _lib.last_scorer() == "k_score_mf2+prune"
    assert len(plain) == 4 and all(torch.equal(x, y) for x, y in zip(plain, rode))
    assert torch.equal(cost[:, :C], ref.unsqueeze(2).expand(B, C, L, *fhw))
    assert bool((cost[:, C:] == 7.0).all())             # the warped half is not the job's


@pytest.mark.parametrize("path", ["sparse", "short"])
def test_paths_without_the_one_sided_launch(cuda, rider_key, path):
    """6. Sparse keypoints (N = 2,048) and a dense pair under 32 spans: step
    keeps the one-launch sweep there; a job armed by hand is still written (by
    the reference kernels, same stream) and consumed, and a second plain
    RANSAC call on the stream writes nothing into the cost buffer."""
    from sfm_amd import _lib, sweep, synth
    lib = _lib.load()
    B, C, L, fhw = 2, 4, 4, (50, 56)
    img = IMG if path == "sparse" else (120, 200)
    flow, K, ref, tgt = _inputs(cuda, B, C, fhw, 46, img)
    kw = {}
    if path == "sparse":
        kw["keypoints"] = (synth.keypoints(B, 2048, hw=img, seed=46, device=cuda), [2048] * B)
    _lib.tune("score_ref_rider", 0)
    want = _hot(cuda, B, C, L, fhw, 2, img=img, **kw).step(flow, K, ref, tgt)[3].clone()
    _lib.tune("score_ref_rider", 1)
    hp = _hot(cuda, B, C, L, fhw, 2, img=img, **kw)
    assert not hp.ref_rider()
    got = hp.step(flow, K, ref, tgt)[3].clone()
    torch.cuda.synchronize()
    assert torch.equal(want, got)
    # a job armed by hand on this path
    hp.cost.fill_(float("nan"))
    assert lib.sfm_score_ref_job(_lib.stream_ptr(cuda), _lib.ptr(ref), _lib.ptr(hp.cost), B, C, L, *fhw, 0) == 0
    assert lib.sfm_score_ref_jobs_armed() == 1
    Kinv = hp.k_inverse(K)
    E, P, inl, win = hp.pose(flow, K, Kinv)
    assert _lib.last_scorer() != "k_score_mf2+prune"
    assert lib.sfm_score_ref_jobs_armed() == 0
    sweep.plane_sweep_cost_psnet(ref, tgt, P, K, Kinv, L, 1.0, 0.6, out=hp.cost, workspace=hp.sweep_ws,
                                 warped_half=True)
    torch.cuda.synchronize()
    assert torch.equal(want, hp.cost)
    hp.cost.fill_(123.0)                                 # the sentinel: nothing left armed writes here
    hp.pose(flow, K, Kinv)
    torch.cuda.synchronize()
    assert bool((hp.cost == 123.0).all())


def test_job_is_one_shot_and_scoped_to_its_stream(cuda, rider_key):
    """7. A job armed on stream X is not consumed by a RANSAC call on stream Y;
    arming again replaces the job; disarming drops it; more armed streams than
    slots do not fail (the oldest is dropped)."""
    from sfm_amd import _lib
    lib = _lib.load()
    B, C, L, fhw = 2, 4, 4, (50, 56)
    flow, K, ref, _ = _inputs(cuda, B, C, fhw, 47)
    hp = _hot(cuda, B, C, L, fhw, 2)
    Kinv = hp.k_inverse(K)
    first = torch.full((B, 2 * C, L, *fhw), 5.0, device=cuda)
    cost = torch.full((B, 2 * C, L, *fhw), 5.0, device=cuda)
    X, Y = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    sx = ctypes.c_void_p(X.cuda_stream)
    arm = lambda s, out: lib.sfm_score_ref_job(s, _lib.ptr(ref), _lib.ptr(out), B, C, L, *fhw, 0)
    assert lib.sfm_score_ref_jobs_armed() == 0
    assert arm(sx, first) == 0 and arm(sx, cost) == 0   # replaced, not accumulated
    assert lib.sfm_score_ref_jobs_armed() == 1
    with torch.cuda.stream(Y):
        hp.pose(flow, K, Kinv)                           # another stream: neither written nor consumed
    torch.cuda.synchronize()
    assert lib.sfm_score_ref_jobs_armed() == 1
    assert bool((cost == 5.0).all()) and bool((first == 5.0).all())
    with torch.cuda.stream(X):
        hp.pose(flow, K, Kinv)                           # its own stream: the replacing job alone
    torch.cuda.synchronize()
    assert lib.sfm_score_ref_jobs_armed() == 0
    assert torch.equal(cost[:, :C], ref.unsqueeze(2).expand(B, C, L, *fhw))
    assert bool((first == 5.0).all()) and bool((cost[:, C:] == 5.0).all())
    cost.fill_(5.0)
    with torch.cuda.stream(X):
        hp.pose(flow, K, Kinv)                           # one-shot
    torch.cuda.synchronize()
    assert bool((cost == 5.0).all())
    assert arm(sx, cost) == 0 and lib.sfm_score_ref_jobs_armed() == 1
    assert lib.sfm_score_ref_job(sx, None, None, 0, 0, 0, 0, 0, 0) == 0      # disarm
    assert lib.sfm_score_ref_jobs_armed() == 0
    with torch.cuda.stream(X):
        hp.pose(flow, K, Kinv)
    torch.cuda.synchronize()
    assert bool((cost == 5.0).all())
    # jobs that are never consumed cannot exhaust the slots
    streams = [torch.cuda.Stream(device=cuda) for _ in range(40)]
    for s in streams:
        assert arm(ctypes.c_void_p(s.cuda_stream), cost) == 0
    assert 1 <= lib.sfm_score_ref_jobs_armed() <= 32
    for s in streams:
        assert lib.sfm_score_ref_job(ctypes.c_void_p(s.cuda_stream), None, None, 0, 0, 0, 0, 0, 0) == 0
    assert lib.sfm_score_ref_jobs_armed() == 0
    assert arm(sx, None) == 1                            # half a job is refused
