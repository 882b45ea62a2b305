"""The conv layer cases of tests/conv_cases.py, checked on the CPU: the
integer layers are exact in every precision for the reasons their docstring
gives, the split emulation behaves as the model says and picks the threshold
the kernel and the wrapper carry, and the guarded buffers are what the GPU
tests take them for."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_table():
    assert len(CC.INT_SHAPES) == 14 and len(set(CC.INT_SHAPES)) == 14
    assert {s[4] for s in CC.INT_SHAPES} >= {1, 2, 3, 63, 64, 65, 66, 70, 129, 130}
    assert any(s[0] == 3 for s in CC.INT_SHAPES) and any(s[3] < 4 and s[2] > 1 for s in CC.INT_SHAPES)
    assert CC.PLANE_SHAPES == [(1, 32, 33, 5, 66), (1, 32, 9, 5, 3)] and all(s[1] == 32 for s in CC.PLANE_SHAPES)
    cases = CC.all_int_cases()
    assert len(cases) == 42
    for c in cases:
        B, cin, D, H, W = c.shape
        assert c.x.shape == (B, cin, D, H, W) and c.w.shape == (c.cout, cin, 3, 3, 3)
        assert c.want.shape == ((B, 32, D, H, W) if c.cout == 32 else (B, D, H, W))
        assert (c.res is not None) == c.relu == (c.epilogue == "relu_res")
    # the plane runs 8, 16 and 32 put seams inside D = 33 with a one-plane tail, and a tail alone at D = 9
    assert [33 % n for n in (8, 16, 32)] == [1, 1, 1] and 9 % 8 == 1 and 9 < 16


@pytest.mark.parametrize("shape", CC.INT_SHAPES)
def test_integer_layers_are_exact(shape):
    """The premises of the bit-exact GPU comparison, per case: operand ranges,
    the largest |sum|, two float32 evaluations in different orders equal to
    each other and to float64, no lo term in the fp32x3 split, and 16-bit
    outputs in range."""
    from sfm_amd.regularize import weight_exponent
    for epi in CC.EPILOGUES:
        c = CC.int_case(shape, epi)
        for t, lim in ((c.x, 3), (c.w, 2), (c.bias, 4)) + (((c.res, 8),) if c.res is not None else ()):
            assert bool((t == t.round()).all()) and float(t.abs().max()) <= lim
        assert 0.1 < float((c.w == 0).double().mean()) < 0.6
        if c.x.numel() >= 1000:
            assert float(c.x.abs().max()) == 3 and float(c.w.abs().max()) == 2
        assert set(c.scale.tolist()) <= {0.25, 0.5, 1.0, 2.0}
        mag = F.conv3d(c.x.abs(), c.w.abs(), None, 1, 1)
        assert float(mag.max()) <= CC.SUM_MAX == 10368 < 2 ** 24
        conv64 = F.conv3d(c.x, c.w, None, 1, 1)
        a = F.conv3d(c.x.float(), c.w.float(), None, 1, 1)
        b = F.conv3d(c.x.flip(1).float(), c.w.flip(1).float(), None, 1, 1)
        # a third order: tap by tap, last tap first
        xp = F.pad(c.x.float(), (1, 1, 1, 1, 1, 1))
        D, H, W = shape[2:]
        t3 = torch.zeros_like(a)
        for tap in reversed(range(27)):
            dz, dy, dx = tap // 9, tap // 3 % 3, tap % 3
            t3 += torch.einsum("bcdhw,oc->bodhw", xp[:, :, dz:dz + D, dy:dy + H, dx:dx + W],
                               c.w[:, :, dz, dy, dx].float())
        assert torch.equal(a, b) and torch.equal(a, t3) and torch.equal(a.double(), conv64)
        # the epilogue in float32 is exact too
        res32 = None if c.res is None else c.res.float()
        y32 = CC.epilogue(a, c.scale.float(), c.bias.float(), res32, c.relu)
        want = c.want if c.cout == 32 else c.want[:, None]
        assert torch.equal(y32.double(), want)
        assert float(want.abs().max()) < 20800 < 65504
        # fp32x3: 2^wexp w exact in f16 (no lo term), x exact in f16, accumulator within 24 bits
        wp = CC.pack_weights(c.w.float())
        e = weight_exponent(wp)
        assert e == 12
        wh, wl = CC.split_f16(wp * 2.0 ** e)
        xh, xl = CC.split_f16(c.x.float())
        assert torch.equal(wh, wp * 2.0 ** e) and not bool(wl.any()) and not bool(xl.any()) and torch.equal(xh, c.x.float())
        assert float(mag.max()) < 2 ** 14          # multiples of 2^12 with a 14-bit integer factor
        assert torch.equal(CC.emulate_x3(c.x.float(), c.w.float(), e), conv64)
        # the 16-bit operands hold the integers
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(c.x.to(dt).double(), c.x) and torch.equal(c.w.to(dt).double(), c.w)
            if c.res is not None:
                assert torch.equal(c.res.to(dt).double(), c.res)


def test_rounding_of_want_is_a_single_rne():
    """want.to(16 bit) from float64 is one rounding to nearest even: ties
    (odd multiples of half an ulp) are in the tables and go to even."""
    c = CC.int_case((1, 64, 4, 17, 70), "plain")
    for dt, mant in ((torch.bfloat16, 8), (torch.float16, 11)):
        r = c.want.to(dt).double()
        err = (r - c.want).abs()
        ulp = 2.0 ** (torch.floor(torch.log2(c.want.abs().clamp_min(1e-30))) - (mant - 1))
        assert bool((err <= ulp / 2).all())
        assert torch.equal(c.want.float().to(dt), c.want.to(dt))       # float32 holds want exactly
        if dt == torch.bfloat16:
            assert bool((err == ulp / 2).any())                         # ties occur


def test_pack_and_layout_helpers():
    w = torch.arange(2 * 3 * 27, dtype=torch.float32).reshape(2, 3, 3, 3, 3)
    wp = CC.pack_weights(w)
    assert wp.shape == (27, 32, 3) and float(wp[:, 2:].abs().sum()) == 0
    assert float(wp[(1 * 3 + 2) * 3 + 0, 1, 2]) == float(w[1, 2, 1, 2, 0])      # tap = (dz * 3 + dy) * 3 + dx
    x = torch.randn(2, 5, 3, 4, 6)
    assert torch.equal(CC.channels_last(x)[1, 2, 3, 5, 4], x[1, 4, 2, 3, 5])


def test_emulation_error_is_inverse_to_amax_below_the_threshold():
    """The model the guard rests on: below 2^-3 the split's error doubles per
    halving of the scale (within 10 %), the float32 conv's does not move."""
    for relu_in in (False, True):
        rows = [CC.emulation_row(k, relu_in) for k in (6, 7, 10, 14, 20)]
        e32 = {r[2] for r in rows}
        assert max(e32) <= 1.001 * min(e32)
        for (a0, e0, _), (a1, e1, _) in zip(rows, rows[1:]):
            assert 0.9 <= (e1 / e0) / (a0 / a1) <= 1.1, (relu_in, a0, a1, e0, e1)
        assert rows[-1][1] > 1e-2                      # 2^-20: two digits left
    # the issue's table, Gaussian input
    a, e3, e32 = CC.emulation_row(0)
    assert e3 < e32
    a, e3, e32 = CC.emulation_row(10)
    assert 1.5e-5 < e3 < 2e-5 and 50 < e3 / e32 < 75


def test_threshold_is_the_kernels():
    """T = 2^-3: at amax = T the emulated split is within 4x the float32
    conv's error for a Gaussian and a ReLU'd input, at T / 2 it is not; the
    wrapper's constant and the kernel's are this T."""
    from sfm_amd.regularize import FP32X3_MIN_AMAX
    T = CC.threshold()
    assert T == 2.0 ** -3 == FP32X3_MIN_AMAX
    for relu_in in (False, True):
        for e in range(-3, 3):
            e3, e32 = CC.at_amax(2.0 ** e, relu_in)
            assert e3 <= 4 * e32, (relu_in, e, e3, e32)
        e3, e32 = CC.at_amax(T / 2, relu_in)
        assert e3 > 4 * e32
    src = open(os.path.join(ROOT, "deep-sfm-revisited_amd", "csrc", "regularize.hip")).read()
    assert re.search(r"constexpr float kX3AmaxMin = 0\.125f;", src)
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "below 2^-14" not in hdr.lower() and "below 2^-3" in hdr.lower().replace("\n * ", " ")


@pytest.mark.parametrize("shape", CC.SCALE_SHAPES)
@pytest.mark.parametrize("relu_in", [False, True])
def test_scale_cases_stay_inside_the_cap(shape, relu_in):
    """The inputs of the GPU activation-scale runs: at the scales the guard
    lets through (amax >= T) the emulated split meets both layer bars, from
    2^-7 down it misses the 4x bar (so the GPU run there tests the guard), and
    no scale sits within a factor 1.5 of T."""
    c = CC.scale_case(shape, relu_in)
    T = CC.threshold()
    wexp = CC.weight_exponent(CC.pack_weights(c.w))
    for k in CC.SCALE_KS:
        s = 2.0 ** -k
        amax = c.amax * s
        assert not (T / 1.5 < amax < T * 1.5), (k, amax)
        x = c.x * s
        assert float(x.abs().max()) == amax
        got = CC.emulate_x3(x, c.w, wexp)
        e3 = float((got - c.want * s).norm() / (c.want * s).norm())
        e32 = float((F.conv3d(x, c.w, None, 1, 1).double() - c.want * s).norm() / (c.want * s).norm())
        if amax >= T:
            assert e3 <= 4 * e32, (k, e3, e32)
            assert bool(((got - c.want * s).abs() <= 2e-5 * c.mag * s).all())
        elif k >= 7:
            assert e3 > 4 * e32 + 1e-7, (k, e3, e32)
    assert {k for k in CC.SCALE_KS if c.amax * 2.0 ** -k >= T} == {0, 3}


def test_conv_planes_knob():
    """conv_planes: 0 (the grid-size heuristic) by default; 4, 8, 16 and 32
    stick, anything else is refused and leaves the value; listed with the
    launch-shape keys."""
    from sfm_amd import _lib
    assert "conv_planes" in _lib.tune_keys() and _lib.tune_get("conv_planes") == 0
    try:
        for v in CC.PLANE_RUNS:
            _lib.tune("conv_planes", v)
            assert _lib.tune_get("conv_planes") == v
        for v in (-1, 1, 2, 5, 12, 33, 64):
            with pytest.raises(_lib.SfmError):
                _lib.tune("conv_planes", v)
            assert _lib.tune_get("conv_planes") == 32
    finally:
        _lib.tune("conv_planes", 0)
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    shape_only = hdr[hdr.index("launch shape only"):hdr.index("results MAY change")]
    assert '"conv_planes"' in shape_only and '"conv_rolling"' in shape_only


def test_guarded_buffers():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        t = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5).to(dt)
        buf, v = CC.guarded(t, "cpu")
        assert buf.numel() == t.numel() + 2 * CC.GUARD and (CC.GUARD * t.element_size()) % 16 == 0
        assert torch.equal(v, t) and v.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + CC.GUARD * t.element_size()
        assert bool(torch.isnan(buf[:CC.GUARD]).all()) and bool(torch.isnan(buf[-CC.GUARD:]).all())
        out, ov = CC.guarded(t, "cpu", canary=True)
        assert CC.canaries_intact(out) and ov.shape == t.shape and ov.dtype == dt
        assert not bool(torch.isnan(ov.float()).any())           # an unwritten output voxel reads as the canary, not NaN
        ov.copy_(t)
        assert CC.canaries_intact(out) and torch.equal(ov, t)
        out[CC.GUARD - 1] = 0
        assert not CC.canaries_intact(out)
        out, ov = CC.guarded(t, "cpu", canary=True)
        out[-1] = 0
        assert not CC.canaries_intact(out)
    a = torch.tensor([float("nan"), 1.0, -0.0])
    assert torch.equal(CC.bits(a), CC.bits(a.clone())) and not torch.equal(CC.bits(a), CC.bits(torch.tensor([float("nan"), 1.0, 0.0])))
