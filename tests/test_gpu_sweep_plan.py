"""Which kernel form a plane-sweep call launches (sfm_last_sweep, taken from the
call's SweepPlan) and that every form writes the volume of the per-row form
(sweep_flat = 0), bit for bit, fp32 and bf16.

Bitwise equality is an arithmetic fact here, not a tolerance of zero: the slab
forms sum the four taps with FMAs, the per-row form with mul / add, and the
two chains round alike exactly when every product weight * feature is exact.
The features are therefore signed powers of two (2^-3 .. 2^3), so any
difference is a dispatch, geometry or indexing error.  (On general features the
forms agree to 1 ulp: tests/test_gpu_sweep_flat.py.)

Shapes: B = 2, C in {8, 5}, L in {4, 3}, h x w in {6x8, 6x7, 5x7} (h*w % 4 =
0, 2, 3), every call a few blocks.  Three cases need another map: interior
windows of k_sweep_tile (16 x 24: the slab holds several whole windows), the band that
does not fit the LDS (one row of 2400 quads is over half the 80 KB budget; the
tuning setter refuses sweep_band_rows below 2, so a band of one row cannot be
asked for by key) and k_ref_planes' fast path (h*w >= 256, slabs of whole
64-element chunks)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
DTYPES = [torch.float32, torch.bfloat16]
KEYS = ("sweep_flat", "sweep_share", "sweep_band_rows")


@functools.lru_cache(maxsize=None)
def _inputs(C, h, w):
    """Host tensors: ref, tgt (signed powers of two), pose, full-resolution K, K^-1."""
    from sfm_amd import synth
    g = torch.Generator().manual_seed(100 * C + 10 * h + w)

    def pow2():
        sign = torch.randint(0, 2, (B, C, h, w), generator=g).float() * 2.0 - 1.0
        return sign * torch.exp2(torch.randint(-3, 4, (B, C, h, w), generator=g).float())
    K = synth.intrinsics(B, 4.0 * w, 4.0 * w, 2.0 * w, 2.0 * h)
    return pow2(), pow2(), synth.relative_pose(B, torch.Generator().manual_seed(h + w)), K, torch.inverse(K)


def _sweep_args(cuda, C, L, h, w):
    from sfm_amd.sweep import quarter_intrinsics
    ref, tgt, pose, K, Ki = _inputs(C, h, w)
    K4, Ki4 = quarter_intrinsics(K, Ki)
    return ref.to(cuda), tgt.to(cuda), pose.to(cuda), K4.to(cuda), Ki4.to(cuda), L, 0.8


def _tuned(values, call):
    """call() under the tuning `values`, every key restored afterwards."""
    from sfm_amd import _lib
    old = {k: _lib.tune_get(k) for k in KEYS}
    try:
        for k, v in values.items():
            _lib.tune(k, v)
        return call()
    finally:
        for k, v in old.items():
            _lib.tune(k, v)


@functools.lru_cache(maxsize=None)
def _per_row(C, L, h, w, dtype):
    """The per-row form's volume, computed once per shape and type (host copy)."""
    from sfm_amd import _lib
    from sfm_amd.sweep import plane_sweep_cost
    cuda = torch.device("cuda", 0)
    out = _tuned({"sweep_flat": 0}, lambda: plane_sweep_cost(*_sweep_args(cuda, C, L, h, w), dtype=dtype))
    assert _lib.last_sweep() in ("k_sweep", "k_sweep+vec")
    out = out.cpu()
    assert bool((out[:, C:] != 0).any()) and bool((out[:, C:] == 0).any())   # samples inside and outside the image
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


PLANAR = [
    # (case, C, L, h, w, tuning, out offset in elements, expected form)
    ("defaults", 8, 4, 6, 8, {}, 0, "k_sweep_tile+wide"),
    # slab = 6 windows (fp32) / 3 (bf16) and a full channel group: interior windows, which alone take
    # sweep_tile_fast and its 16-byte stores (on the shapes above every window is an edge window)
    ("interior_windows", 8, 4, 16, 24, {}, 0, "k_sweep_tile+wide"),
    ("odd_slab", 5, 3, 5, 7, {}, 0, "k_sweep_tile"),                       # store_px falls to 0
    ("out_off_by_one", 8, 4, 6, 8, {}, 1, "k_sweep_tile"),
    ("share", 8, 4, 6, 8, {"sweep_share": 1}, 0, "k_sweep_tile"),
    ("flat", 5, 3, 6, 7, {"sweep_flat": 1}, 0, "k_sweep_flat"),
    ("band", 8, 4, 6, 7, {"sweep_flat": 3}, 0, "k_sweep_band"),
    ("band_does_not_fit", 5, 3, 2, 2400, {"sweep_flat": 3}, 0, "k_sweep_flat"),
    ("rows_vector", 8, 4, 6, 7, {"sweep_flat": 0}, 0, "k_sweep+vec"),      # h*w % 4 == 2, L even
    ("rows_element", 5, 3, 5, 7, {"sweep_flat": 0}, 0, "k_sweep"),         # h*w odd
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case,C,L,h,w,tuning,offset,form", PLANAR, ids=[c[0] for c in PLANAR])
def test_planar_forms(cuda, case, C, L, h, w, tuning, offset, form, dtype):
    from sfm_amd import _lib
    from sfm_amd.sweep import plane_sweep_cost
    want = _per_row(C, L, h, w, dtype)
    buf = torch.full((want.numel() + offset,), float("nan"), dtype=dtype, device=cuda)
    out = buf[offset:].view(want.shape)
    _tuned(tuning, lambda: plane_sweep_cost(*_sweep_args(cuda, C, L, h, w), dtype=dtype, out=out))
    assert _lib.last_sweep() == form, _lib.last_sweep()
    assert torch.equal(_bits(out.cpu()), _bits(want))


def test_band_rows_below_two_are_refused():
    """The fall-through of sweep_flat = 3 to k_sweep_flat cannot be reached by
    asking for a one-row band: the key's range starts at 2."""
    from sfm_amd import _lib
    old = _lib.tune_get("sweep_band_rows")
    with pytest.raises(_lib.SfmError):
        _lib.tune("sweep_band_rows", 1)
    assert _lib.tune_get("sweep_band_rows") == old


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("flat", [0, 3])
def test_warped_half_takes_the_tile_form(cuda, flat, dtype):
    """sfm_plane_sweep_psnet_warped_half: k_sweep_tile whatever sweep_flat says,
    and the reference rows are left as they were."""
    from sfm_amd import _lib
    from sfm_amd.sweep import plane_sweep_cost_psnet
    C, L, h, w = 8, 4, 6, 8
    want = _per_row(C, L, h, w, dtype)
    ref, tgt, pose, K, Ki = (t.to(cuda) for t in _inputs(C, h, w))
    out = torch.full(want.shape, 7.0, dtype=dtype, device=cuda)
    _tuned({"sweep_flat": flat}, lambda: plane_sweep_cost_psnet(ref, tgt, pose, K, Ki, L, 0.8, dtype=dtype, out=out,
                                                                warped_half=True))
    assert _lib.last_sweep() == "k_sweep_tile+wide", _lib.last_sweep()
    out = out.cpu()
    assert bool((out[:, :C] == 7.0).all())
    assert torch.equal(_bits(out[:, C:]), _bits(want[:, C:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,form", [(8, "k_sweep_cl"), (5, "k_sweep_cl_any")])
def test_channels_last_forms(cuda, C, form, dtype):
    from sfm_amd import _lib
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    L, h, w = 4, 6, 8
    want = _per_row(C, L, h, w, torch.float32).permute(0, 2, 3, 4, 1).to(dtype)   # [B, L, h, w, 2C], RNE
    out = plane_sweep_cost_channels_last(*_sweep_args(cuda, C, L, h, w), dtype=dtype)
    assert _lib.last_sweep() == form, _lib.last_sweep()
    assert torch.equal(_bits(out.cpu()), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,L,h,w,form", [(5, 4, 16, 16, "k_ref_planes"), (5, 3, 6, 8, "k_ref_planes_generic")])
def test_reference_half_forms(cuda, C, L, h, w, form, dtype):
    from sfm_amd import _lib
    from sfm_amd.sweep import plane_sweep_ref_half
    want = _per_row(C, L, h, w, dtype)
    out = torch.full(want.shape, 7.0, dtype=dtype, device=cuda)
    plane_sweep_ref_half(_inputs(C, h, w)[0].to(cuda), L, out)
    assert _lib.last_sweep() == form, _lib.last_sweep()
    out = out.cpu()
    assert torch.equal(_bits(out[:, :C]), _bits(want[:, :C]))
    assert bool((out[:, C:] == 7.0).all())
