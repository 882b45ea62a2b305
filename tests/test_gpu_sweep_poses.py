"""Every form of the plane sweep, the inverse warp and the correlation cost on
poses outside the small-motion regime (tests/sweep_pose_cases.py: rolls, yaws
to 180 degrees, sideways and huge baselines, planes behind the camera or under
the Z clamp, exact border hits, a batch that mixes them), at the smallest
shapes where the forms still differ: 13x21 (odd hw, under one window), 20x31
(hw % 4 == 2), 24x78 (hw % 4 == 0, rows across windows), L = 7 and 16, C = 8.

  * the planar float32 volume and the correlation cost against the oracle,
    every sample classified in float64 (ambiguous border samples: zero or the
    in-range alternative in all channels together; clamped ones: the delta bar);
  * every kernel form against the default one, bit for bit (k_sweep_flat,
    k_sweep_tile at each window width / store width / with and without buffer
    addressing and tap sharing, k_sweep_band at three run / band shapes), the
    bf16 volume the RNE of the float32 one, the per-row kernel within 2e-6,
    every element of a NaN-filled buffer written;
  * sample_pos_nr against sample_pos: inverse_warp at each plane's constant
    depth has the same all-zero set as the sweep's warped half;
  * the channels-last entries (float32 and float16 features; float32, f16,
    bf16 output), the warped-only and warped-half entries against the planar
    volume, bit for bit.

Measured on an MI355X (each oracle test prints its figures, pytest -s; the
per-case shares are in tests/sweep_pose_cases.py): no kernel decided unlike
the oracle on any of the 1.1 million samples, ambiguous ones included; the
warped values differed from the oracle's by 0, the correlation cost by at most
2.4e-7; every form wrote the default form's bits.  With the Z clamp of
sample_pos_nr taken out (a scratch build) 20 of these tests fail, all on
clamped_in_range (oracle, form equality against the per-row kernel, inverse
warp), and the older sweep, depth and drop-in tests still pass."""
import pytest
import torch

from tests import sweep_pose_cases as PC

pytestmark = pytest.mark.gpu

C = 8
SHAPE_L = [(h, w, L) for (h, w) in PC.SHAPES for L in (7, 16)]
SHAPE_IDS = [f"{h}x{w}L{L}" for h, w, L in SHAPE_L]
# both plane spacings: the depth planes (i + 1) MIN_DEPTH on these cases
BY_DEPTH = [("roll_30", 20, 31, 7), ("sideways", 24, 78, 16), ("forward_big_t", 13, 21, 16),
            ("clamped_in_range", 24, 78, 16), ("mixed_batch", 20, 31, 16)]
_IVIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}

_scenes, _expected, _volumes = {}, {}, {}


def _scene(name, h, w, c=C):
    key = (name, h, w, c)
    if key not in _scenes:
        _scenes[key] = PC.scene(name, h, w, c)
    return _scenes[key]


def _exp(name, h, w, L, by_depth=False):
    """The oracle's values and the classification: computed once, shared, never modified."""
    key = (name, h, w, L, by_depth)
    if key not in _expected:
        _expected[key] = PC.expected_warped(_scene(name, h, w), L, by_depth)
    return _expected[key]


def _args(sc, cuda, L, half=False):
    ref, tgt = (sc.ref.half(), sc.tgt.half()) if half else (sc.ref, sc.tgt)
    return (ref.to(cuda), tgt.to(cuda), sc.pose.to(cuda), sc.K4.to(cuda), sc.Ki4.to(cuda), L, sc.min_depth)


def _volume(name, h, w, L, cuda, by_depth=False, c=C, half=False):
    """The planar float32 volume by the default form: computed once, shared, never modified."""
    from sfm_amd.sweep import plane_sweep_cost
    key = (name, h, w, L, by_depth, c, half)
    if key not in _volumes:
        a = _args(_scene(name, h, w, c), cuda, L, half)
        _volumes[key] = plane_sweep_cost(a[0].float(), a[1].float(), *a[2:], predict_by_depth=by_depth)
    return _volumes[key]


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(_IVIEW[a.dtype]), b.view(_IVIEW[b.dtype]))


def _oracle_params():
    p = [pytest.param(name, h, w, L, False, id=f"{name}-{sid}") for name in PC.CASES
         for (h, w, L), sid in zip(SHAPE_L, SHAPE_IDS)]
    return p + [pytest.param(name, h, w, L, True, id=f"{name}-{h}x{w}L{L}-by_depth") for name, h, w, L in BY_DEPTH]


@pytest.mark.parametrize("name,h,w,L,by_depth", _oracle_params())
def test_planar_volume_against_the_oracle(cuda, name, h, w, L, by_depth):
    """The default form's float32 volume: the reference half an exact copy,
    the warped half under sweep_pose_cases.check_warped (_close_rel outside
    the ambiguous and clamped sets)."""
    sc = _scene(name, h, w)
    got = _volume(name, h, w, L, cuda, by_depth).cpu()
    assert torch.equal(got[:, :C], sc.ref.unsqueeze(2).expand(-1, -1, L, -1, -1))     # reference half: exact copy
    PC.check_warped(got[:, C:], _exp(name, h, w, L, by_depth), f"{name} {h}x{w} L={L} by_depth={by_depth}")


@pytest.mark.parametrize("name,h,w,L,by_depth", _oracle_params())
def test_correlation_cost_against_the_oracle(cuda, name, h, w, L, by_depth):
    from oracle import sweep as S
    from sfm_amd.depth import correlation_cost
    sc = _scene(name, h, w)
    a = _args(sc, cuda, L)
    got = correlation_cost(*a, predict_by_depth=by_depth).cpu()
    exp = _exp(name, h, w, L, by_depth)
    # the checker's expected cost is the oracle's correlation_cost
    want = S.correlation_cost(sc.ref, sc.tgt, sc.pose, sc.K, sc.Kinv, L, sc.min_depth, predict_by_depth=by_depth)
    prod = sc.ref.unsqueeze(2) * exp.want
    assert float((want - prod.mean(1)).abs().max()) <= (C + 1) * 2.0 ** -24 * float(prod.abs().mean(1).max())
    PC.check_correlation(got, sc.ref, exp, f"corr {name} {h}x{w} L={L} by_depth={by_depth}")


# (label, tuning) -- every form computes the default form's bits, except the per-row kernel (sample_pos with true
# divisions and a mul/add tap sum: within 2e-6)
_PLAIN = dict(sweep_flat=2, sweep_group=8, sweep_nj=1, sweep_buffer=1, sweep_share=0, sweep_store_px=0,
              sweep_run=16, sweep_band_rows=16)
FORMS_F32 = [
    ("tile g8 nj1", {}),
    ("flat g4", dict(sweep_flat=1, sweep_group=4)), ("flat g8", dict(sweep_flat=1)),
    ("tile g4 nj1", dict(sweep_group=4)), ("tile g4 nj2", dict(sweep_group=4, sweep_nj=2)),
    ("tile g4 nj4", dict(sweep_group=4, sweep_nj=4)), ("tile g8 nj2", dict(sweep_nj=2)),
    ("tile g8 nj4", dict(sweep_nj=4)),
    ("band 16x16", dict(sweep_flat=3)), ("band 1x2", dict(sweep_flat=3, sweep_run=1, sweep_band_rows=2)),
    ("band 5x3", dict(sweep_flat=3, sweep_run=5, sweep_band_rows=3)),
    ("no buffer g8", dict(sweep_buffer=0)), ("no buffer g4 nj2", dict(sweep_buffer=0, sweep_group=4, sweep_nj=2)),
    ("share g8", dict(sweep_share=1)), ("share g4 nj2", dict(sweep_share=1, sweep_group=4, sweep_nj=2)),
    ("share nj4", dict(sweep_share=1, sweep_nj=4)),
    ("wide px1", dict(sweep_store_px=1)), ("wide px2", dict(sweep_store_px=2)), ("wide px4", dict(sweep_store_px=4)),
    ("wide px4 g4", dict(sweep_store_px=4, sweep_group=4)),
    ("default", None),
]
FORMS_BF16 = [
    ("tile g8 nj2", {}), ("flat g4", dict(sweep_flat=1, sweep_group=4)), ("flat g8", dict(sweep_flat=1)),
    ("tile g4 nj4", dict(sweep_group=4, sweep_nj=4)),
    ("band 16x16", dict(sweep_flat=3)), ("band 5x3", dict(sweep_flat=3, sweep_run=5, sweep_band_rows=3)),
    ("no buffer g8", dict(sweep_buffer=0)), ("share g8", dict(sweep_share=1)),
    ("wide px2", dict(sweep_store_px=2)), ("wide px4", dict(sweep_store_px=4)), ("wide px8", dict(sweep_store_px=8)),
    ("per row", dict(sweep_flat=0)),
    ("default", None),
]


def _run_form(tuning, snap, args, dtype, shape):
    from sfm_amd import _lib
    from sfm_amd.sweep import plane_sweep_cost
    _lib.tune_restore(snap)
    if tuning is not None:
        for k, v in {**_PLAIN, **tuning}.items():
            _lib.tune(k, v)
    out = torch.full(shape, float("nan"), dtype=dtype, device=args[0].device)
    plane_sweep_cost(*args, dtype=dtype, out=out)
    if tuning is not None:      # the form the keys select is the one that ran
        want = {0: "k_sweep", 1: "k_sweep_flat", 2: "k_sweep_tile", 3: "k_sweep_band"}[_lib.tune_get("sweep_flat")]
        assert _lib.last_sweep().split("+")[0] == want, (tuning, _lib.last_sweep())
        if tuning.get("sweep_share") or tuning.get("sweep_buffer") == 0:
            assert _lib.last_sweep() == "k_sweep_tile", (tuning, _lib.last_sweep())
    return out


@pytest.mark.parametrize("h,w,L", SHAPE_L, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", PC.CASES)
def test_every_form_writes_the_same_volume(cuda, name, h, w, L):
    from sfm_amd import _lib
    sc = _scene(name, h, w)
    a = _args(sc, cuda, L)
    B = sc.pose.shape[0]
    shape = (B, 2 * C, L, h, w)
    snap = _lib.tune_snapshot()
    try:
        base = _volume(name, h, w, L, cuda)
        per_row = _run_form(dict(sweep_flat=0), snap, a, torch.float32, shape)
        f32 = [(label, _run_form(t, snap, a, torch.float32, shape)) for label, t in FORMS_F32]
        b16 = [(label, _run_form(t, snap, a, torch.bfloat16, shape)) for label, t in FORMS_BF16]
    finally:
        _lib.tune_restore(snap)
    assert not bool(torch.isnan(base).any())
    assert torch.equal(base[:, :C], a[0].unsqueeze(2).expand(-1, -1, L, -1, -1))
    for label, out in f32:
        assert not bool(torch.isnan(out).any()), label          # every element written
        assert _bits_equal(out, base), (label, int((out != base).sum()), (out != base).nonzero()[:3].tolist())
    assert not bool(torch.isnan(per_row).any())
    assert torch.equal(per_row[:, :C], base[:, :C])
    d = float((per_row - base).abs().max())
    assert d <= 2e-6, ("per row", d)
    # sample_pos (true divisions) and sample_pos_nr decide alike
    assert torch.equal((per_row[:, C:] == 0).all(dim=1), (base[:, C:] == 0).all(dim=1))
    want16 = base.to(torch.bfloat16)                              # RNE of the float32 volume
    for label, out in b16:
        assert not bool(torch.isnan(out).any()), label
        if label == "per row":
            assert _bits_equal(out, per_row.to(torch.bfloat16)), label
        else:
            assert _bits_equal(out, want16), (label, int((out != want16).sum()), (out != want16).nonzero()[:3].tolist())


@pytest.mark.parametrize("name,h,w,L,by_depth", _oracle_params())
def test_inverse_warp_decides_as_the_sweep(cuda, name, h, w, L, by_depth):
    """k_inverse_warp (sample_pos, true divisions) at each plane's constant
    depth against the warped half (sample_pos_nr): the same (pixel, plane)
    positions are zero in all channels -- with N(0,1) features an in-range
    sample never is -- and the values agree within 2e-6 (mul/add against FMA
    tap sums of the same taps and weights)."""
    from sfm_amd.sweep import inverse_warp
    sc = _scene(name, h, w)
    a = _args(sc, cuda, L)
    B = sc.pose.shape[0]
    warped = _volume(name, h, w, L, cuda, by_depth)[:, C:]
    depths = PC.plane_depths(L, sc.min_depth, by_depth)
    planes = torch.stack([inverse_warp(a[1], torch.ones(B, h, w, device=cuda) * float(d), a[2], a[3], a[4])
                          for d in depths], 2)
    zero_iw, zero_sw = (planes == 0).all(dim=1), (warped == 0).all(dim=1)
    unlike = zero_iw != zero_sw
    assert not bool(unlike.any()), (int(unlike.sum()), unlike.nonzero()[:4].tolist())
    d = float((planes - warped).abs().max())
    assert d <= 2e-6, d
    exp = _exp(name, h, w, L, by_depth)
    assert int((~zero_sw).sum()) > 0 or int(exp.cls.in32.sum()) == 0


#           h,  w,  L,  C    (channel counts of test_gpu_sweep_cl.py: 32 and 8 the fast kernel, 12 the element-wise one)
CL_SHAPES = [(13, 21, 7, 32), (20, 31, 16, 12), (24, 78, 16, 8)]


@pytest.mark.parametrize("h,w,L,c", CL_SHAPES, ids=["13x21L7c32", "20x31L16c12", "24x78L16c8"])
@pytest.mark.parametrize("name", PC.CASES)
def test_channels_last_entries_equal_the_transposed_planar_volume(cuda, name, h, w, L, c):
    from sfm_amd.regularize import to_channels_last
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    sc = _scene(name, h, w, c)
    B = sc.pose.shape[0]
    for half in (False, True):
        a = _args(sc, cuda, L, half)
        planar = _volume(name, h, w, L, cuda, c=c, half=half)
        if bool(_exp(name, h, w, L).cls.in32.any()):
            assert bool((planar[:, c:] != 0).any())
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            got = plane_sweep_cost_channels_last(*a, dtype=dtype)
            assert tuple(got.shape) == (B, L, h, w, 2 * c) and got.dtype == dtype
            assert _bits_equal(got, to_channels_last(planar, dtype)), (half, dtype)
    by_depth = name in [b[0] for b in BY_DEPTH]
    if by_depth:
        a = _args(sc, cuda, L)
        planar = _volume(name, h, w, L, cuda, by_depth=True, c=c)
        got = plane_sweep_cost_channels_last(*a, dtype=torch.float16, predict_by_depth=True)
        assert _bits_equal(got, to_channels_last(planar, torch.float16))


@pytest.mark.parametrize("h,w,L", SHAPE_L, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", PC.CASES)
def test_warped_entries_equal_the_warped_half(cuda, name, h, w, L):
    """warped_only (sfm_plane_sweep_warped) and the warped-half entry
    (sfm_plane_sweep_psnet_warped_half, which leaves the reference rows alone)."""
    from sfm_amd.sweep import plane_sweep_cost, plane_sweep_cost_psnet
    sc = _scene(name, h, w)
    a = _args(sc, cuda, L)
    B = sc.pose.shape[0]
    full = _volume(name, h, w, L, cuda)
    for dtype in (torch.float32, torch.bfloat16):
        want = full.to(dtype)
        only = torch.full((B, C, L, h, w), float("nan"), dtype=dtype, device=cuda)
        plane_sweep_cost(None, *a[1:], dtype=dtype, out=only, warped_only=True)
        assert _bits_equal(only, want[:, C:].contiguous()), dtype
        out = torch.full((B, 2 * C, L, h, w), float("nan"), dtype=dtype, device=cuda)
        plane_sweep_cost_psnet(a[0], a[1], a[2], sc.K.to(cuda), sc.Kinv.to(cuda), L, sc.min_depth, None, dtype,
                               out=out, warped_half=True)
        assert _bits_equal(out[:, C:].contiguous(), want[:, C:].contiguous()), dtype
        assert bool(torch.isnan(out[:, :C]).all())                # the reference rows are not this entry's
