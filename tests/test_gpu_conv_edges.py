"""The four Conv3d kernels of csrc/regularize.hip (k_conv3, k_conv3r,
k_conv3_f32, k_conv3_x3) and the channels-last conversions at the places the
Gaussian unit-scale tests of tests/test_gpu_regularize.py cannot see
(cases and reasoning: tests/conv_cases.py, checked on the CPU by
tests/test_conv_cases.py):

1. exact-integer layers: every output is one bit pattern, at edge shapes, in
   guarded buffers;
2. the rolling kernel's plane runs of 4, 8, 16 and 32 (conv_planes) with seams
   and one-plane tails inside the compared region;
3. activation scales 2^0 .. 2^-20 for fp32x3, one layer and the stack;
4. where an out-of-range activation sits, the exact f16 boundary, -inf, NaN;
5. the channels-last conversions at C and P off the tile sizes.

Measured on an MI355X before the low-side guard (relative L2 of one fp32x3
layer against float64; sfm_conv3_f32 is at 3.3e-7 .. 6.5e-7 at every scale):
2^-6 1.1e-6, 2^-7 2.2e-6, 2^-9 8.8e-6, 2^-12 7.0e-5, 2^-16 1.1e-3, 2^-20
1.8e-2 at every shape; the homogeneous stack 1.7e-5 at 2^-10 and 1.8e-2 at
2^-20 (DESIGN.md 2.5 has the table).  With the guard those layers are the
f32 layer's bits and both stacks are at 1.2e-6.

Value-only mutants of the kernels, built apart (failing tests here / in
tests/test_gpu_regularize.py's layer and small-stack tests): halo columns
64/65 staged as zeros 14 / 20; dy and dx swapped in the weight read 25 / 29;
the (PH + 1) % 3 ring slot off by one 14 / 16; the 2^-wexp unscale dropped
25 / 9; the low-side check removed 5 / 0."""
import pytest
import torch

from oracle import regularize as R
from tests import conv_cases as CC

pytestmark = pytest.mark.gpu

_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x3": torch.float32}
# (kind, conv_rolling or None, with a range flag)
_RUNS = [("bf16", 0, False), ("bf16", 1, False), ("f16", 0, False), ("f16", 1, False), ("f32", None, False),
         ("f32x3", None, False), ("f32x3", None, True)]


def _fbits(v):
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item())


def _layer(dev, kind, x, wp, sc, bi, res, relu, cout, flag=None, wexp=None):
    """One layer on channels-last host operands (float32 or float64 values that
    the kind's dtype holds), through guarded device buffers.  Returns the
    output on the host ([B, D, H, W, 32] in the kind's dtype, or [B, D, H, W]
    float32 for cout 1); the canaries are checked here."""
    from sfm_amd import _lib
    from sfm_amd.regularize import weight_exponent
    dt = _DT[kind]
    B, D, H, W, cin = x.shape
    _, xg = CC.guarded(x.to(dt), dev)
    rg = None if res is None else CC.guarded(res.to(dt), dev)[1]
    shape, odt = ((B, D, H, W, 32), dt) if cout == 32 else ((B, D, H, W), torch.float32)
    obuf, og = CC.guarded(torch.empty(shape, dtype=odt), dev, canary=True)
    wd = wp.to(dt).to(dev).contiguous()
    scd, bid = sc.float().to(dev), bi.float().to(dev)
    lib = _lib.load()
    head = (_lib.ptr(xg), B, cin, D, H, W, _lib.ptr(wd))
    tail = (_lib.ptr(scd), _lib.ptr(bid), _lib.ptr(rg), 1 if relu else 0, cout, _lib.ptr(og))
    with torch.cuda.device(dev):
        if kind == "f32x3":
            e = weight_exponent(wp) if wexp is None else wexp
            rc = lib.sfm_conv3_f32x3(*head, e, *tail, None if flag is None else flag.data_ptr(), _lib.stream_ptr(dev))
        else:
            rc = getattr(lib, "sfm_conv3_" + kind)(*head, *tail, _lib.stream_ptr(dev))
        _lib.check(rc, "sfm_conv3_" + kind)
        torch.cuda.synchronize(dev)
    assert CC.canaries_intact(obuf), (kind, "a write outside the output")
    return og.cpu()


def _int_operands(c):
    sc, bi = CC.pack_affine(c.scale, c.bias)
    return CC.channels_last(c.x), CC.pack_weights(c.w), sc, bi, None if c.res is None else CC.channels_last(c.res)


def _int_want(c, kind):
    if c.cout == 1:
        return c.want.float()
    return CC.channels_last(c.want).to(_DT[kind])


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = CC.bits(got) != CC.bits(want)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError((what, "mismatches", int(bad.sum()), "of", bad.numel(), "first at", idx,
                              float(got[tuple(idx)]), float(want[tuple(idx)])))


def _run_int(dev, c, kind, rolling, with_flag, x=None):
    from sfm_amd import _lib
    xcl, wp, sc, bi, res = _int_operands(c)
    if x is not None:
        xcl = x
    if rolling is not None:
        _lib.tune("conv_rolling", rolling)
    flag = torch.full((2,), 7, dtype=torch.int32, device=dev) if with_flag else None
    got = _layer(dev, kind, xcl, wp, sc, bi, res, c.relu, c.cout, flag=flag)
    if with_flag:
        f = flag.cpu().tolist()
        finite = xcl[~torch.isnan(xcl)]
        assert f == [0, _fbits(float(finite.abs().max()))], (c.shape, c.epilogue, f)
    return got


@pytest.mark.parametrize("shape", CC.INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_layers(cuda, shape):
    """Every kernel on small-integer operands: bit-equal to the float64 result
    (rounded once for the 16-bit outputs), canaries intact, no NaN pulled in
    from the margins, the range flag clear and its second word the input's
    largest magnitude."""
    for epi in CC.EPILOGUES:
        c = CC.int_case(shape, epi)
        for kind, rolling, with_flag in _RUNS:
            got = _run_int(cuda, c, kind, rolling, with_flag)
            what = (shape, epi, kind, rolling, with_flag)
            assert not bool(torch.isnan(got.float()).any()), what
            _same_bits(got, _int_want(c, kind), what)


def test_nan_pair_leaves_the_other_pairs_alone(cuda):
    """B = 3 with pair 1 all NaN: pairs 0 and 2 keep their exact bits (no
    block reads across a pair boundary), in every kernel.  Pair 1 itself is
    all NaN where the epilogue has no ReLU (the kernels' fmaxf(v, 0) returns 0
    for a NaN, where torch.relu would keep it)."""
    shape = (3, 32, 9, 5, 3)
    for epi in CC.EPILOGUES:
        c = CC.int_case(shape, epi)
        x = CC.channels_last(c.x).clone()
        x[1] = float("nan")
        for kind, rolling, with_flag in _RUNS:
            got = _run_int(cuda, c, kind, rolling, with_flag, x=x)
            want = _int_want(c, kind)
            what = (epi, kind, rolling, with_flag)
            if not c.relu:
                assert bool(torch.isnan(got[1].float()).all()), what
            _same_bits(got[0], want[0], what)
            _same_bits(got[2], want[2], what)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("shape", CC.PLANE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plane_runs(cuda, shape, kind):
    """k_conv3r with 4, 8, 16 and 32 planes per block: exact on the integer
    layers, and on Gaussian operands bit-equal to k_conv3 (conv_rolling 0).
    At D = 33 the seams d0 = 8, 16, 24, 32 / 16, 32 / 32 and the one-plane
    tails after them are all inside the compared volume."""
    from sfm_amd import _lib
    assert _lib.tune_get("conv_planes") == 0
    for epi in CC.EPILOGUES:
        c = CC.int_case(shape, epi)
        x, wp, sc, bi, res = CC.gauss_layer(shape, epi)
        relu, cout = epi == "relu_res", 1 if epi == "cout1" else 32
        _lib.tune("conv_rolling", 0)
        base = _layer(cuda, kind, x, wp, sc, bi, res, relu, cout)
        assert bool(torch.isfinite(base.float()).all())
        _lib.tune("conv_rolling", 1)
        for planes in CC.PLANE_RUNS:
            _lib.tune("conv_planes", planes)
            _same_bits(_run_int(cuda, c, kind, 1, False), _int_want(c, kind), (shape, epi, kind, planes, "integers"))
            _same_bits(_layer(cuda, kind, x, wp, sc, bi, res, relu, cout), base, (shape, epi, kind, planes, "gauss"))
        _lib.tune("conv_planes", 0)


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm())


@pytest.mark.parametrize("relu_in", [False, True], ids=["gauss", "relu"])
@pytest.mark.parametrize("shape", CC.SCALE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_activation_scale_layer(cuda, shape, relu_in):
    """One fp32x3 layer with a range flag at activation scales 2^0 .. 2^-20
    against the float64 conv: |got - want| <= 2e-5 mag with no absolute term,
    relative L2 <= 4x sfm_conv3_f32's + 1e-7 (test_conv_layer_f32x3's bars),
    bit-equal to sfm_conv3_f32 where the largest activation is below T; and
    sfm_conv3_f32 itself exactly equivariant to the power of two.

    MI355X, before the guard: the 4x bar was missed from k = 7 on (cin 64
    Gaussian: from k = 9), the elementwise one from k = 12 on (worst
    |err| / mag 2.1e-5 .. 3.0e-5 there; cin 64 Gaussian 1.5e-5, from k = 16),
    4.3e-3 .. 8.9e-3 at k = 20."""
    from sfm_amd.regularize import FP32X3_MIN_AMAX
    c = CC.scale_case(shape, relu_in)
    wp = CC.pack_weights(c.w)
    sc, bi = torch.ones(32), torch.zeros(32)
    xcl = CC.channels_last(c.x)
    want0, mag0 = CC.channels_last(c.want), CC.channels_last(c.mag)
    f32_unit, failures = None, []
    for k in CC.SCALE_KS:
        s = 2.0 ** -k
        x = xcl * s
        flag = torch.full((2,), 7, dtype=torch.int32, device=cuda)
        got3 = _layer(cuda, "f32x3", x, wp, sc, bi, None, False, 32, flag=flag)
        got32 = _layer(cuda, "f32", x, wp, sc, bi, None, False, 32)
        want, mag = want0 * s, mag0 * s
        e3, e32 = _rel(got3, want), _rel(got32, want)
        worst = float(((got3.double() - want).abs() / mag).max())
        f = flag.cpu().tolist()
        print(dict(shape=shape, relu_in=relu_in, k=k, amax=c.amax * s, x3=e3, f32=e32, worst_over_mag=worst, flag=f))
        if f != [0, _fbits(c.amax * s)]:
            failures.append((k, "flag", f))
        if worst > 2e-5:
            failures.append((k, "elementwise", worst))
        if e3 > 4 * e32 + 1e-7:
            failures.append((k, "relative L2", e3, e32))
        if c.amax * s < FP32X3_MIN_AMAX and not torch.equal(CC.bits(got3), CC.bits(got32)):
            failures.append((k, "not the f32 layer's bits"))
        if k == 0:
            f32_unit = got32
        elif not torch.equal(CC.bits(got32 * 2.0 ** k), CC.bits(f32_unit)):
            failures.append((k, "f32 layer not equivariant"))
    assert not failures, failures


@pytest.mark.parametrize("random_bn", [False, True], ids=["plain_bn", "random_bn"])
@pytest.mark.parametrize("k", [10, 20])
def test_activation_scale_stack(cuda, k, random_bn):
    """The fp32x3 stack on a cost volume scaled by 2^-k against the fp32
    oracle stack: test_stack_f32x3_vs_oracle's 2e-5.  With untouched
    BatchNorms (scale 1, shift 0) the stack is homogeneous and every layer
    sees the small scale; with random ones the first layer does."""
    from tests.test_regularize import _module
    m = _module(5, 64, random_bn)
    cost = torch.randn(1, 64, 8, 10, 24, generator=torch.Generator().manual_seed(3)) * 2.0 ** -k
    got = m.to(cuda)(cost.to(cuda), precision="fp32x3").cpu()
    m = m.cpu()
    want = R.regularize_fp32(m, cost)
    r = float((got - want).norm() / want.norm())
    print(dict(k=k, random_bn=random_bn, rel_l2=r))
    assert got.shape == want.shape and r <= 2e-5, r


_FIRST, _LAST = (0, 0, 0, 0, 0), (1, 63, 2, 8, 69)
_F16_MAX = 65504.0
_F16_NEXT = float(torch.nextafter(torch.tensor(_F16_MAX), torch.tensor(float("inf"))))


@pytest.mark.parametrize("where", [_FIRST, _LAST], ids=["first", "last"])
@pytest.mark.parametrize("value,rerun", [(7.0e4, True), (_F16_MAX, False), (-_F16_MAX, False), (_F16_NEXT, True),
                                         (float("-inf"), True), (float("nan"), False)],
                         ids=["7e4", "65504", "-65504", "next", "-inf", "nan"])
def test_range_flag_placement(cuda, where, value, rerun):
    """One disturbed activation at the first voxel's channel 0 or the last
    pair's last voxel's channel 63 (cin 64, B = 2): beyond 65504 the flag is
    set and the output is the fp32 layer's, bit for bit; at exactly +-65504
    it stays clear and the split's finite result stands; a NaN does not set it
    and gives the fp32 layer's NaN set."""
    shape = (2, 64, 3, 9, 70)
    c = CC.scale_case(shape, False)
    assert tuple(i + 1 for i in _LAST) == shape
    x = c.x.clone()
    x[where] = value
    xcl, wp = CC.channels_last(x), CC.pack_weights(c.w)
    g = torch.Generator().manual_seed(12)
    sc, bi = 0.5 + torch.rand(32, generator=g), 0.3 * torch.randn(32, generator=g)
    flag = torch.full((2,), 7, dtype=torch.int32, device=cuda)
    # no ReLU: the epilogue's fmaxf(v, 0) turns a NaN into 0 in all four kernels
    got = _layer(cuda, "f32x3", xcl, wp, sc, bi, None, False, 32, flag=flag)
    ref32 = _layer(cuda, "f32", xcl, wp, sc, bi, None, False, 32)
    f = flag.cpu().tolist()
    finite_max = float(xcl[~torch.isnan(xcl)].abs().max())
    assert f == [1 if rerun else 0, _fbits(finite_max)], f
    nan32 = torch.isnan(ref32)
    assert torch.equal(torch.isnan(got), nan32)
    if rerun:
        assert torch.equal(CC.bits(got)[~nan32], CC.bits(ref32)[~nan32])
    elif value == value:
        assert bool(torch.isfinite(got).all())
        unguarded = _layer(cuda, "f32x3", xcl, wp, sc, bi, None, False, 32)
        assert torch.equal(CC.bits(got), CC.bits(unguarded))
        mag = CC.channels_last(torch.nn.functional.conv3d(x.double().abs(), c.w.double().abs(), None, 1, 1)) * sc.double()
        assert bool(((got.double() - ref32.double()).abs() <= 4e-5 * mag + 1e-6).all())
    else:
        assert bool(nan32.any()) and not bool(nan32.all())


@pytest.mark.parametrize("P", [1, 63, 65, 257])
@pytest.mark.parametrize("C", [8, 72, 128])
def test_channels_last_conversions(cuda, C, P):
    """[B][C][P] -> [B][P][C] for float32 and bfloat16 inputs into bfloat16,
    float16 and float32: torch's bits, at C below, between and at twice the
    64-channel tile and P around the 64-pixel tile; values on and beyond the
    f16 range included (they round to 65504 or to inf, as torch's do)."""
    from sfm_amd.regularize import to_channels_last
    B = 2
    x = torch.randn(B, C, 1, 1, P, generator=torch.Generator().manual_seed(C * 1000 + P)) * 100
    flat = x.view(-1)
    for i, v in enumerate((7.0e4, -7.0e4, 65504.0, 65519.0, 65520.0, 3.4e38, 1e-8, -6.1e-5)):
        flat[i * (flat.numel() // 8 + 1) % flat.numel()] = v      # eight distinct places, the first element among them
    for src in (x, x.to(torch.bfloat16)):
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            got = to_channels_last(src.to(cuda), dt).cpu()
            want = src.float().permute(0, 2, 3, 4, 1).contiguous().to(dt)
            _same_bits(got, want, (C, P, src.dtype, dt))
    assert bool(torch.isinf(x.to(torch.bfloat16).float().to(torch.float16)).any())
