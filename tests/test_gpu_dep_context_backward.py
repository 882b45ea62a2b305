"""sfm_dep_context_unpack_grad_f16 on the GPU (csrc/context_bwd.hip
``k_dep_unpack_grad``; models/PSNet.py:218-221): the backward of the refinement
stack's fused bilinear upsample into the features, against the float64 CPU
autograd backward of F.interpolate fed channels 1..32 of the float16 gradient --
bit for bit on an exact lattice, within a derived float32 bound at a general
ratio and at the degenerate ones, the same bits for any chunking and from call
to call."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _unpack(cuda, g, B, h, w, calls=None, sentinel=None):
    """The kernel on a device copy of g [B, H, W, 64] float16, as the (b0, nb)
    calls given (default: one call for all pairs) -> [B, 32, h, w] float32 on
    the CPU; grad_feat starts as ``sentinel`` (default NaN)."""
    from sfm_amd.context import dep_context_unpack_grad
    gd = g.to(cuda).contiguous()
    out = torch.full((B, 32, h, w), float("nan") if sentinel is None else sentinel, dtype=torch.float32, device=cuda)
    for b0, nb in calls or [(0, B)]:
        dep_context_unpack_grad(gd[b0:b0 + nb], b0, out)
    return out.cpu()


def _want(g, h, w, absolute=False):
    """The float64 CPU autograd backward of F.interpolate(bilinear,
    align_corners=True) on channels 1..32 of g [B, H, W, 64] (of |g| with
    ``absolute``: the bound's A, the same adjoint, whose weights are >= 0)."""
    B, H, W, _ = g.shape
    go = g[..., 1:33].double().permute(0, 3, 1, 2).contiguous()
    feat = torch.zeros(B, 32, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(feat, [H, W], mode="bilinear", align_corners=True).backward(go.abs() if absolute else go)
    return feat.grad


def _axis_receives(n_src, n_dst):
    """Which sources get a non-zero weight from some destination: the float64
    restatement of the forward's index expression (test_dep_context_backward_abi.py)."""
    s = (n_src - 1) / (n_dst - 1) if n_dst > 1 else 0.0
    wt = torch.zeros(n_src, dtype=torch.float64)
    for d in range(n_dst):
        f = s * float(d)
        i0 = min(int(f), n_src - 1)
        i1 = i0 + (1 if i0 < n_src - 1 else 0)
        wt[i0] += 1.0 - (f - float(i0))
        wt[i1] += f - float(i0)
    return wt != 0


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _lattice():
    """h, w = 4, 18 -> H, W = 13, 69, B = 3 (the forward test's lattice): both
    scales are exactly 1/4, every weight product a multiple of 1/16, the
    gradient integers in [-8, 8]: every sum is exact in float32, whatever the
    order.  Channels 0 and 33..63 hold other integers, which the kernel must
    ignore."""
    B, h, w, H, W = 3, 4, 18, 13, 69
    gen = torch.Generator().manual_seed(41)
    g = torch.randint(-8, 9, (B, H, W, 64), generator=gen).half()
    g[..., 0] = torch.randint(100, 200, (B, H, W), generator=gen).half()
    g[..., 33:] = torch.randint(100, 200, (B, H, W, 31), generator=gen).half()
    want = _want(g, h, w)
    assert torch.equal(want * 16, (want * 16).round()) and float(want.abs().max()) < 2 ** 20
    return g, want.float(), (B, h, w)


def test_exact_lattice_bit_for_bit(cuda):
    g, want, (B, h, w) = _lattice()
    got = _unpack(cuda, g, B, h, w)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(_bits(got) & 0x7FFFFFFF, _bits(want) & 0x7FFFFFFF) and bool((want != 0).any())
    # the other channels are ignored: zeroing them changes no bit
    clean = g.clone()
    clean[..., 0] = 0
    clean[..., 33:] = 0
    assert torch.equal(_bits(_unpack(cuda, clean, B, h, w)), _bits(got))


def test_chunking_and_untouched_pairs(cuda):
    g, want, (B, h, w) = _lattice()
    whole = _unpack(cuda, g, B, h, w)
    for calls in ([(0, 1), (1, 2)], [(2, 1), (0, 2)], [(1, 1), (2, 1), (0, 1)]):
        assert torch.equal(_bits(_unpack(cuda, g, B, h, w, calls)), _bits(whole)), calls
    # pairs outside the range keep what was there; the kernel writes, it does not add
    part = _unpack(cuda, g, B, h, w, [(1, 1)], sentinel=-77.0)
    assert torch.equal(_bits(part[1]), _bits(whole[1]))
    assert bool((part[0] == -77.0).all()) and bool((part[2] == -77.0).all())


# (B, h, w, H, W): the general ratio (scales 5/21 and 19/77; at most 11 x 9 destinations per source), sy = 0 with
# one source row, H == 1, a downsample by 2 in y (the odd source rows get weight 0 only), a downsample by 4 (source
# rows that no destination reads), and more than one 256-thread block per pair at a ragged ratio
RATIOS = [(2, 6, 20, 22, 78), (2, 1, 3, 5, 7), (2, 3, 4, 1, 6), (2, 9, 11, 5, 7), (2, 9, 11, 3, 4), (1, 7, 23, 9, 31)]


@pytest.mark.parametrize("B,h,w,H,W", RATIOS, ids=["%dx%d_to_%dx%d" % r[1:] for r in RATIOS])
def test_general_and_degenerate_ratios(cuda, B, h, w, H, W):
    """|got - want| <= 2^-16 A elementwise, A the same adjoint applied to |g|.
    Derived, not measured: a source pixel sums at most 11 x 9 = 99 < 2^7
    weighted terms (fewer at the other shapes), which in float32 (unit
    round-off 2^-24) is off by at most 2^7 2^-24 A = 2^-17 A; one more bit is
    allowed for the products."""
    gen = torch.Generator().manual_seed(42)
    g = torch.randn(B, H, W, 64, generator=gen).half()
    want = _want(g, h, w)
    bound = 2.0 ** -16 * _want(g, h, w, absolute=True)
    got = _unpack(cuda, g, B, h, w)
    assert bool(torch.isfinite(got).all())                  # every element of every pair was written
    err = (got.double() - want).abs()
    print(f"dep unpack grad {h}x{w} <- {H}x{W}: max |got - want| {float(err.max()):.3e}, "
          f"max of |got - want| / A {float((err / bound.clamp_min(1e-300)).max() * 2.0 ** -16):.3e} (bound 2^-16 = 1.526e-05)")
    assert bool((err <= bound).all())
    # the source pixels that receive nothing are +0, bit for bit
    nothing = ~(_axis_receives(h, H)[:, None] & _axis_receives(w, W)[None, :])
    assert bool(nothing.any()) == ((h, w, H, W) in ((3, 4, 1, 6), (9, 11, 5, 7), (9, 11, 3, 4)))
    assert bool((want[:, :, nothing] == 0).all())
    assert bool((_bits(got)[:, :, nothing] == 0).all())
    # two calls: the same bits
    assert torch.equal(_bits(_unpack(cuda, g, B, h, w)), _bits(got))


def test_non_finite_gradient_comes_through(cuda):
    """A GradScaler must see an overflow: an inf in the feature channels
    reaches the sources that read it; one in an ignored channel reaches none."""
    B, h, w, H, W = 1, 6, 20, 22, 78
    g = torch.zeros(B, H, W, 64).half()
    g[0, 10, 40, 5] = float("inf")
    got = _unpack(cuda, g, B, h, w)
    assert not bool(torch.isfinite(got[0, 4]).all()) and bool(torch.isfinite(got[0, :4]).all())
    g = torch.zeros(B, H, W, 64).half()
    g[0, 10, 40, 0] = float("inf")
    g[0, 10, 40, 33] = float("nan")
    assert bool((_unpack(cuda, g, B, h, w) == 0).all())
