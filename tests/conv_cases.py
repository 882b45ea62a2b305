"""Inputs for the Conv3d layers of the regularisation stack (k_conv3,
k_conv3r, k_conv3_f32, k_conv3_x3 in csrc/regularize.hip) with their float64
results (tests/test_conv_cases.py checks the premises on the CPU,
tests/test_gpu_conv_edges.py runs the kernels against them).

Exact-integer layers.  Activations are integers in [-3, 3], weights integers
in [-2, 2] (a fifth of them zero), the per-channel scale a power of two in
2^-2 .. 2^1, the bias an integer in [-4, 4], the residual an integer in
[-8, 8].  Then
  * |sum| <= 27 * 64 * 3 * 2 = 10,368 < 2^24: every partial sum of a float32
    accumulator is an integer it holds exactly, in any order;
  * for fp32x3, weight_exponent gives 2^12 w <= 8192, exact in f16: every lo
    term of the split is zero and the accumulator holds multiples of 2^12
    with at most 14 significant bits;
  * the epilogue's scale * sum + bias is a multiple of 1/4 below 2^15, exact
    in float32, and so are the ReLU and the residual add.
So ``want``, the float64 conv3d plus the epilogue, is the one bit pattern a
float32 output may have, and a 16-bit output is its single rounding to
nearest even (|want| < 20,800 < 65504).  A layout error on one voxel (a
dropped halo column, a swapped tap, a wrong swizzle chunk, a slipped
accumulator ring slot) changes an integer and cannot hide in a tolerance.

The split emulation.  sfm_conv3_f32x3's arithmetic on the CPU: hi / lo halves
by ``.half()`` (round to nearest even, subnormals kept), the three kept
products summed in float64.  x_lo = f16(x - f16(x)) is about 2^-11 |x|, so it
is a subnormal f16 (below 2^-14) for |x| < 2^-3 and then carries an absolute
error of 2^-25: below that scale the layer's error doubles with every halving
of the activations.  ``threshold()`` is the smallest power of two T such that
an input whose largest magnitude is T or more keeps the emulated error within
4x the float32 conv's; the kernel re-runs a layer below it in float32
(FP32X3_MIN_AMAX in sfm_amd/regularize.py, kX3AmaxMin in the kernel file).
`python -m tests.conv_cases` prints the table.

Guarded buffers.  ``guarded`` places a tensor's bytes in the middle of a
larger allocation, 16-byte aligned, between margins filled with NaN (inputs,
residual) or a canary bit pattern (output): a kernel that reads past its
tensor pulls a NaN into an otherwise exact result, one that writes past it
changes a canary.  Nothing here moves an address out of an allocation.
"""
import functools
import math
import os
import sys
from collections import namedtuple

import torch
import torch.nn.functional as F

# (B, cin, D, H, W): one voxel; one column, two columns, W = 63 .. 66 around the 64-column tile and its two halo
# columns; H below one row tile with D > 1; more than one tile in x and in y; B = 3; a plane run of 33 at W = 66
INT_SHAPES = [(1, 32, 1, 1, 1), (1, 64, 1, 1, 1), (1, 32, 2, 1, 2), (2, 32, 3, 3, 1), (1, 32, 5, 4, 63),
              (1, 32, 5, 4, 64), (1, 32, 5, 4, 65), (1, 32, 5, 4, 66), (1, 32, 6, 8, 64), (1, 64, 4, 17, 70),
              (1, 64, 2, 9, 129), (2, 64, 3, 8, 130), (3, 32, 9, 5, 3), (1, 32, 33, 5, 66)]
EPILOGUES = ("plain", "relu_res", "cout1")
PLANE_SHAPES = [(1, 32, 33, 5, 66), (1, 32, 9, 5, 3)]
PLANE_RUNS = (4, 8, 16, 32)
SUM_MAX = 27 * 64 * 3 * 2

IntCase = namedtuple("IntCase", "shape epilogue x w scale bias res relu cout want")


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 1) % 2147483647
    return torch.Generator().manual_seed(seed)


def epilogue(conv, scale, bias, res, relu):
    """The layer's epilogue on a conv result [B, cout, D, H, W] (any dtype)."""
    y = conv * scale.to(conv.dtype).view(1, -1, 1, 1, 1) + bias.to(conv.dtype).view(1, -1, 1, 1, 1)
    if relu:
        y = torch.relu(y)
    if res is not None:
        y = y + res.to(conv.dtype)
    return y


@functools.lru_cache(maxsize=None)
def int_case(shape, epi):
    """One exact-integer layer: float64 operands and ``want`` ([B, 32, D, H, W],
    or [B, D, H, W] for the cout-1 epilogue)."""
    B, cin, D, H, W = shape
    cout = 1 if epi == "cout1" else 32
    g = _gen(1, *shape, EPILOGUES.index(epi))
    x = torch.randint(-3, 4, (B, cin, D, H, W), generator=g).double()
    w = torch.randint(-2, 3, (cout, cin, 3, 3, 3), generator=g).double()
    w = w * (torch.rand(w.shape, generator=g) >= 0.2)
    scale = 2.0 ** torch.randint(-2, 2, (cout,), generator=g).double()
    bias = torch.randint(-4, 5, (cout,), generator=g).double()
    relu = epi == "relu_res"
    res = torch.randint(-8, 9, (B, 32, D, H, W), generator=g).double() if relu else None
    want = epilogue(F.conv3d(x, w, None, 1, 1), scale, bias, res, relu)
    return IntCase(shape, epi, x, w, scale, bias, res, relu, cout, want[:, 0] if cout == 1 else want)


def all_int_cases():
    return [int_case(s, e) for s in INT_SHAPES for e in EPILOGUES]


def pack_weights(w):
    """[cout, cin, 3, 3, 3] -> the kernels' [27 taps][32 cout][cin], cout zero-padded."""
    cout, cin = w.shape[:2]
    wp = torch.zeros(27, 32, cin, dtype=w.dtype)
    wp[:, :cout] = w.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    return wp


def pack_affine(scale, bias):
    sc, bi = torch.ones(32), torch.zeros(32)
    sc[:scale.numel()], bi[:bias.numel()] = scale.float(), bias.float()
    return sc, bi


def channels_last(t):
    """[B, C, D, H, W] -> contiguous [B, D, H, W, C]."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=None)
def gauss_layer(shape, epi):
    """Gaussian operands of a cin-32 layer, channels-last float32 (x, packed
    weights, scale, bias, residual): for comparisons between launch shapes,
    where no reference is needed."""
    B, cin, D, H, W = shape
    g = _gen(2, *shape, EPILOGUES.index(epi))
    x = torch.randn(B, D, H, W, cin, generator=g)
    wp = torch.randn(27, 32, cin, generator=g) * 0.1
    if epi == "cout1":
        wp[:, 1:] = 0
    sc, bi = 0.5 + torch.rand(32, generator=g), 0.1 * torch.randn(32, generator=g)
    res = torch.randn(B, D, H, W, 32, generator=g) if epi == "relu_res" else None
    return x, wp, sc, bi, res


# ---------------------------------------------------------------------------
# the split emulation

def split_f16(t):
    """t = hi + lo + (dropped), both halves as sfm_conv3_f32x3 forms them."""
    hi = t.half().float()
    return hi, (t - hi).half().float()


def emulate_x3(x, w, wexp):
    """The float64 value of what k_conv3_x3 sums for a conv of float32 x
    [B, cin, D, H, W] with float32 w [cout, cin, 3, 3, 3] (scale 1, bias 0)."""
    wh, wl = split_f16(w * 2.0 ** wexp)
    xh, xl = split_f16(x)
    d = lambda a, b: F.conv3d(a.double(), b.double(), None, 1, 1)
    return (d(xh, wh) + d(xl, wh) + d(xh, wl)) * 2.0 ** -wexp


def _rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm())


SCALE_SHAPES = [(1, 32, 4, 9, 70), (1, 64, 3, 9, 70)]
SCALE_KS = (0, 3, 6, 7, 9, 12, 16, 20)

ScaleCase = namedtuple("ScaleCase", "shape relu_input x w want mag amax")


@functools.lru_cache(maxsize=None)
def scale_case(shape, relu_input):
    """Unit-scale operands of the activation-scale runs: x (Gaussian, or its
    ReLU), w ~ 0.1 N(0, 1), the float64 conv ``want`` and ``mag`` = conv(|x|,
    |w|).  At scale 2^-k the input is x * 2^-k and the expected result
    want * 2^-k, both exact."""
    B, cin, D, H, W = shape
    g = _gen(3, *shape, int(relu_input))
    x = torch.randn(B, cin, D, H, W, generator=g)
    if relu_input:
        x = torch.relu(x)
    w = torch.randn(32, cin, 3, 3, 3, generator=g) * 0.1
    want = F.conv3d(x.double(), w.double(), None, 1, 1)
    mag = F.conv3d(x.double().abs(), w.double().abs(), None, 1, 1)
    return ScaleCase(shape, relu_input, x, w, want, mag, float(x.abs().max()))


def weight_exponent(w):
    """sfm_amd.regularize.weight_exponent (the package path as tests/conftest.py sets it, for `python -m`)."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep-sfm-revisited_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from sfm_amd.regularize import weight_exponent as we
    return we(w)


def emulated_errors(x, w, want=None):
    """(relative L2 of the emulated split, of the float32 conv) against float64."""
    if want is None:
        want = F.conv3d(x.double(), w.double(), None, 1, 1)
    return _rel_l2(emulate_x3(x, w, weight_exponent(w)), want), _rel_l2(F.conv3d(x, w, None, 1, 1), want)


@functools.lru_cache(maxsize=None)
def _table_operands(relu_input):
    g = _gen(4, int(relu_input))
    x = torch.randn(1, 32, 4, 9, 20, generator=g)
    if relu_input:
        x = torch.relu(x)
    w = torch.randn(32, 32, 3, 3, 3, generator=g) * 0.1
    return x, w, F.conv3d(x.double(), w.double(), None, 1, 1)


def emulation_row(k, relu_input=False):
    """(amax, split error, float32 error) of the table's operands at scale 2^-k."""
    x, w, want = _table_operands(relu_input)
    e3, e32 = emulated_errors(x * 2.0 ** -k, w, want * 2.0 ** -k)
    return float(x.abs().max()) * 2.0 ** -k, e3, e32


def at_amax(amax, relu_input):
    """The table's operands scaled so that the largest |x| is exactly amax
    (a power of two): the worst input the guard lets through at T = amax."""
    x, w, _ = _table_operands(relu_input)
    x = (x.double() * (amax / float(x.abs().max()))).float()
    assert float(x.abs().max()) == amax
    return emulated_errors(x, w)


@functools.lru_cache(maxsize=None)
def threshold():
    """The smallest power of two T with the emulated split within 4x the
    float32 conv's error for every tested amax = 2^e >= T, Gaussian and
    ReLU'd inputs."""
    ok = {e: all(e3 <= 4.0 * e32 for e3, e32 in (at_amax(2.0 ** e, r) for r in (False, True)))
          for e in range(-8, 3)}
    T = 3
    while T - 1 in ok and ok[T - 1]:
        T -= 1
    assert T <= 2, ok
    return 2.0 ** T


# ---------------------------------------------------------------------------
# guarded buffers

GUARD = 64                    # margin elements on either side (a multiple of 16 bytes for every element size here)
CANARY = {2: 0x5A3C, 4: 0x5A3C5A3C}
_INT = {2: torch.int16, 4: torch.int32}


def guarded(t, device, canary=False):
    """(buffer, view): ``t``'s values in a contiguous view of ``t``'s shape and
    dtype, GUARD elements inside a one-dimensional buffer on ``device``; the
    margins are NaN, or with ``canary`` the whole buffer starts as the canary
    pattern (an output's: pass any tensor of its shape and dtype)."""
    n, sz = t.numel(), t.element_size()
    if canary:
        buf = torch.full((n + 2 * GUARD,), CANARY[sz], dtype=_INT[sz], device=device).view(t.dtype)
    else:
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=t.dtype, device=device)
    view = buf[GUARD:GUARD + n].view(t.shape)
    if not canary:
        view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def canaries_intact(buf):
    b = buf.view(_INT[buf.element_size()])
    c = CANARY[buf.element_size()]
    return bool((b[:GUARD] == c).all()) and bool((b[-GUARD:] == c).all())


def bits(t):
    """The tensor's bit patterns, for exact comparisons (NaNs included)."""
    return t.contiguous().view(_INT[t.element_size()])


if __name__ == "__main__":
    for relu_in in (False, True):
        print("ReLU'd input" if relu_in else "Gaussian input")
        for k in (0, 3, 4, 5, 6, 7, 10, 14, 20):
            a, e3, e32 = emulation_row(k, relu_in)
            print(f"  2^-{k:<2d} amax {a:8.2e}  fp32x3 {e3:8.2e}  f32 {e32:8.2e}  x{e3 / e32:8.1f}")
        for e in range(-6, 1):
            e3, e32 = at_amax(2.0 ** e, relu_in)
            print(f"  amax = 2^{e:<3d} fp32x3 {e3:8.2e}  f32 {e32:8.2e}  x{e3 / e32:6.2f}")
    print("T =", threshold(), "= 2^%d" % round(math.log2(threshold())))
