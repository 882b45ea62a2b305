"""The float16 BatchNorm3d / ReLU / residual kernels on the GPU (csrc/bn3.hip):
sfm_bn3_stats_f16, sfm_bn3_apply_f16, sfm_bn3_backward_f16 and
batchnorm3_act_autograd around them.

Exact lattices must come back bit for bit.  General float16 values are held to
bounds that follow from float64 accumulation and one rounding (statistics,
apply), and the backward to the project's rule for float16 routes: err =
max|g - g64| / max|g64| against the float64 restatement on the CPU on the same
float16 values, at most 2 x the error of bn -> relu -> add as torch modules
under float16 autocast on the GPU, measured in the same test.

General values (``_general``): per channel a mean of a few units and a spread
of 0.25 .. 1.75; channel 5 holds 256 + {-1, 0, 1} / 4, where a float32
E[x^2] - mean^2 loses every digit.  Below 8 voxels the spread is scaled by 2^-9:
with 2 voxels per channel a training-mode input gradient is a (dy0 - dy1) delta
with delta = eps / (2 var) -- every float32 evaluation, torch's included, forms
it from terms 1 / delta times larger, and at var ~ 1 the comparison of two such
errors says nothing; at var ~ eps the case is conditioned like the others.
From 8 voxels on the values lie on the grid of sixteenths: among 10^5 free
values some pre-activation always falls within a float32 rounding of zero,
and the backward tests' precondition (``mask_margin``) asks that none does; on
the grid the nearest value to a channel's zero crossing is a fixed distance
away, and the seed is one at which that distance is large enough in every
channel, shape and mode (checked on the CPU, asserted in the test)."""
import functools
from fractions import Fraction

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 1, 1, 2),      # the minimum training mode takes: 2 voxels
    (1, 2, 3, 5),      # 30 voxels: less than one wave's worth (a wave covers 16, a block 128), no multiple of 16
    (2, 4, 8, 12),     # 768 voxels: 6 blocks of one step each
    (1, 3, 37, 53),    # 5883 voxels: ragged, 46 blocks, the last one short
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
EPS, MOM = 1e-5, 0.1


def _launches(fn, names=("bn3_stats", "bn3_apply", "bn3_bwd")):
    from sfm_amd import _lib
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, {k: _lib.profile_read(k)[1] for k in names}


@functools.lru_cache(maxsize=None)
def _general(shape, seed=31):
    """Float16 operands on the CPU (shared, left unchanged)."""
    B, L, h, w = shape
    n = B * L * h * w
    g = torch.Generator().manual_seed(seed + n)
    mean = 2.0 * torch.randn(32, generator=g)
    spread = 0.25 + 1.5 * torch.rand(32, generator=g)
    if n < 8:
        spread = spread * 2.0 ** -9
    x = mean + spread * torch.randn(B, L, h, w, 32, generator=g)
    if n >= 8:
        x = torch.round(x * 16.0) / 16.0
    x[..., 5] = 256.0 + 0.25 * torch.randint(-1, 2, (B, L, h, w), generator=g)
    d = dict(x=x.half(), res=torch.randn(B, L, h, w, 32, generator=g).half(),
             gout=torch.randn(B, L, h, w, 32, generator=g).half(),
             gamma=1.0 + 0.3 * torch.randn(32, generator=g), beta=0.3 * torch.randn(32, generator=g),
             rm=mean + 0.1 * spread * torch.randn(32, generator=g), rv=spread ** 2 * (0.5 + torch.rand(32, generator=g)))
    d["rm"][5], d["rv"][5] = 256.1, 0.05
    return d


def _stats64(x, gamma, beta, rm=None, rv=None, training=True):
    """mean, biased variance, a, b in float64 from the float16 values (two-pass variance)."""
    f = x.double().reshape(-1, 32)
    if training:
        mean = f.mean(0)
        var = ((f - mean) ** 2).mean(0)
    else:
        mean, var = rm.double(), rv.double()
    a = gamma.double() / torch.sqrt(var + EPS)
    return mean, var, a, beta.double() - mean * a


def _dev(d, cuda, *keys):
    return [d[k].to(cuda) for k in keys]


# ---- exact lattices ------------------------------------------------------------------------------------------------
LATTICE = (2, 4, 8, 16)                                     # 1024 voxels: a power of two


@functools.lru_cache(maxsize=None)
def _lattice():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, LATTICE + (32,), generator=g)
    res = torch.randint(-8, 9, LATTICE + (32,), generator=g)
    gout = torch.randint(-8, 9, LATTICE + (32,), generator=g)
    stats = torch.zeros(5, 32)
    stats[0] = torch.randint(-3, 4, (32,), generator=g).float()              # mean: integers
    stats[1] = 1.0
    stats[2] = 2.0 ** torch.randint(-2, 3, (32,), generator=g).float()       # invstd: powers of two
    stats[3] = (2.0 ** torch.randint(-2, 3, (32,), generator=g).float()) * (1 - 2 * torch.randint(0, 2, (32,), generator=g))
    stats[4] = torch.randint(-8, 9, (32,), generator=g).float()              # b: integers
    return x, res, gout, stats


def test_lattice_statistics_bit_for_bit(cuda):
    """Integers in [-8, 8], 1024 voxels: both sums are exact in any order, mean
    = S / N and var = Q / N - mean^2 are exact in float64, so rows 0 and 1 are
    the exact rationals rounded once to float32 -- at one block, few blocks, a
    count that divides nothing and more blocks than voxels, and the default."""
    from sfm_amd import _lib
    from sfm_amd.regularize import bn3_stats_f16
    x = _lattice()[0]
    f = x.reshape(-1, 32)
    n = f.shape[0]
    S, Q = f.sum(0).tolist(), (f * f).sum(0).tolist()
    mean = torch.tensor([float(Fraction(s, n)) for s in S], dtype=torch.float64).float()
    var = torch.tensor([float(Fraction(q * n - s * s, n * n)) for s, q in zip(S, Q)], dtype=torch.float64).float()
    xd = x.half().to(cuda)
    one, zero = torch.ones(32, device=cuda), torch.zeros(32, device=cuda)
    try:
        for nb in (1, 3, 7, 4096, 0):
            _lib.tune("bn_blocks", nb)
            st = bn3_stats_f16(xd, one, zero, EPS, None, None, MOM, True).cpu()
            assert torch.equal(st[0].view(torch.int32), mean.view(torch.int32)), nb
            assert torch.equal(st[1].view(torch.int32), var.view(torch.int32)), nb
            inv = 1.0 / torch.sqrt(var.double() + EPS)
            assert float((st[2].double() - inv).abs().max()) <= 2.0 ** -22 * float(inv.max()), nb
            assert torch.equal(st[2], st[3])                                    # gamma 1: a is invstd
    finally:
        _lib.tune("bn_blocks", 0)                               # not enumerated, so no fixture restores it


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("resid", [False, True], ids=["nores", "res"])
def test_lattice_apply_and_eval_backward_bit_for_bit(cuda, relu, resid):
    """Hand-written statistics (a a signed power of two, b, mean and the
    residual integers): a x + b + res is a multiple of 1/4 below 2^7, exact in
    float32 and float16, so apply equals torch bit for bit; so does the
    eval-mode backward, dx = a dy, dbeta an exact integer sum, dgamma an exact
    multiple of 1/4."""
    from sfm_amd.regularize import bn3_apply_f16, bn3_backward_f16
    x, res, gout, stats = _lattice()
    a, b = stats[3], stats[4]
    z = a * x.float() + b
    want = torch.relu(z) if relu else z
    want = (want + res.float() if resid else want).half()
    xd, rd, gd, sd = x.half().to(cuda), res.half().to(cuda), gout.half().to(cuda), stats.to(cuda)
    got = bn3_apply_f16(xd, sd, rd if resid else None, relu)
    assert got.dtype == torch.float16 and torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    dy = gout.double() * ((z > 0).double() if relu else 1.0)
    gx, ggb = bn3_backward_f16(xd, gd, sd, relu, training=False)
    # by value: where the mask is shut both sides hold a zero, whose sign is that of a here and of a dy there
    assert gx.dtype == torch.float16 and torch.equal(gx.cpu(), (a.double() * dy).half())
    dyf, xf = dy.reshape(-1, 32), x.double().reshape(-1, 32)
    dbeta = dyf.sum(0)
    dgamma = ((dyf * xf).sum(0) - stats[0].double() * dbeta) * stats[2].double()
    assert torch.equal(ggb[1].cpu().double(), dbeta) and torch.equal(ggb[0].cpu().double(), dgamma)
    _, only = bn3_backward_f16(xd, gd, sd, relu, training=False, need_grad_x=False)
    assert torch.equal(only, ggb)


# ---- statistics, general values ------------------------------------------------------------------------------------
def _stat_bounds(x):
    f = x.double().reshape(-1, 32)
    n = f.shape[0]
    mean = f.mean(0)
    var = ((f - mean) ** 2).mean(0)
    return n, mean, var, 2.0 ** -23 * mean.abs(), 2.0 ** -23 * var + n * 2.0 ** -52 * (f * f).mean(0)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statistics_against_float64(cuda, shape):
    """|mean - mean64| <= 2^-23 |mean64| and |var - var64| <= 2^-23 var64 + N 2^-52
    E[x^2]: float64 sums of exact terms, one rounding to float32.  a and b follow
    from the kernel's own mean and variance to two float32 roundings.  The
    running statistics after one and two steps: the same bounds through torch's
    rule, plus one float32 rounding per step."""
    from sfm_amd.regularize import bn3_stats_f16
    d = _general(shape)
    d2 = _general(shape, seed=77)
    gamma, beta = _dev(d, cuda, "gamma", "beta")
    rm, rv = d["rm"].clone().to(cuda), d["rv"].clone().to(cuda)
    rm64, rv64 = d["rm"].double(), d["rv"].double()
    em = torch.zeros(32, dtype=torch.float64)
    ev = torch.zeros(32, dtype=torch.float64)
    for step, dd in enumerate((d, d2)):
        n, mean64, var64, bm, bv = _stat_bounds(dd["x"])
        st = bn3_stats_f16(dd["x"].to(cuda), gamma, beta, EPS, rm, rv, MOM, True).cpu().double()
        dm, dv = (st[0] - mean64).abs(), (st[1] - var64).abs()
        print({"shape": shape, "step": step, "mean_err/bound": float((dm / bm.clamp_min(1e-300)).max()),
               "var_err/bound": float((dv / bv.clamp_min(1e-300)).max()), "ch5_var": float(st[1][5]), "ch5_var64": float(var64[5])})
        assert bool((dm <= bm).all()), (dm / bm).max()
        assert bool((dv <= bv).all()), (dv / bv).max()
        assert bool((st[1] >= 0).all())
        a = d["gamma"].double() / torch.sqrt(st[1] + EPS)
        assert bool(((st[2] - 1.0 / torch.sqrt(st[1] + EPS)).abs() <= 2.0 ** -22 * st[2].abs()).all())
        assert bool(((st[3] - a).abs() <= 2.0 ** -22 * a.abs()).all())
        b = d["beta"].double() - st[0] * st[3]
        assert bool(((st[4] - b).abs() <= 2.0 ** -22 * (d["beta"].double().abs() + (st[0] * st[3]).abs())).all())
        rm64 = (1 - MOM) * rm64 + MOM * mean64
        rv64 = (1 - MOM) * rv64 + MOM * var64 * n / (n - 1)
        em = (1 - MOM) * em + MOM * bm + 2.0 ** -24 * rm64.abs()
        ev = (1 - MOM) * ev + MOM * bv * n / (n - 1) + 2.0 ** -24 * rv64.abs()
        assert bool(((rm.cpu().double() - rm64).abs() <= em).all()), step
        assert bool(((rv.cpu().double() - rv64).abs() <= ev).all()), step
    # eval mode: the rows from the running statistics, which stay put
    before = rm.clone(), rv.clone()
    st = bn3_stats_f16(d["x"].to(cuda), gamma, beta, EPS, rm, rv, MOM, False).cpu()
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1])
    assert torch.equal(st[0], rm.cpu()) and torch.equal(st[1], rv.cpu())
    a = d["gamma"].double() / torch.sqrt(rv.cpu().double() + EPS)
    assert bool(((st[3].double() - a).abs() <= 2.0 ** -23 * a.abs()).all())


# ---- apply, general values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_against_float64_on_its_own_statistics(cuda, shape):
    """Per element |z - z64| <= 2^-11 |z64| + 2^-21 (|a x| + |b| + |res|) + 2^-24:
    one float16 rounding, float32 arithmetic before it, the float16 subnormal
    step."""
    from sfm_amd.regularize import bn3_apply_f16, bn3_stats_f16
    d = _general(shape)
    x, res, gamma, beta = _dev(d, cuda, "x", "res", "gamma", "beta")
    st = bn3_stats_f16(x, gamma, beta, EPS, None, None, MOM, True)
    a, b = st[3].cpu().double(), st[4].cpu().double()
    ax = a * d["x"].double()
    for relu in (False, True):
        for resid in (False, True):
            z64 = ax + b
            z64 = torch.relu(z64) if relu else z64
            r64 = d["res"].double() if resid else torch.zeros_like(z64)
            z64 = z64 + r64
            got = bn3_apply_f16(x, st, res if resid else None, relu).cpu().double()
            bound = 2.0 ** -11 * z64.abs() + 2.0 ** -21 * (ax.abs() + b.abs() + r64.abs()) + 2.0 ** -24
            worst = float(((got - z64).abs() / bound).max())
            print({"shape": shape, "relu": relu, "resid": resid, "err/bound": worst})
            assert worst <= 1.0, (relu, resid, worst)


# ---- backward, general values --------------------------------------------------------------------------------------
def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def _backward64(d, gout, relu, training):
    from sfm_amd.regularize import bn3_act_reference
    x = d["x"].double().requires_grad_()
    gam, bet = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    out, _, _ = bn3_act_reference(x, gam, bet, d["rm"], d["rv"], training, MOM, EPS, relu, d["res"].double())
    out.backward(gout.double())
    return x.grad, gam.grad, bet.grad


def _backward_modules(d, gout, relu, training, cuda):
    bn = nn.BatchNorm3d(32, eps=EPS, momentum=MOM).to(cuda).train(training)
    with torch.no_grad():
        for t, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "rm"), (bn.running_var, "rv")):
            t.copy_(d[k])
    x = d["x"].to(cuda).requires_grad_()
    # torch's own batch-norm kernels at every shape (the vendor-library dispatch off): the 2-voxel shape is not one
    # that library is exercised at
    with torch.backends.cudnn.flags(enabled=False), torch.autocast("cuda", torch.float16):
        y = bn(x.permute(0, 4, 1, 2, 3))
        y = torch.relu(y) if relu else y
        y = y.permute(0, 2, 3, 4, 1) + d["res"].to(cuda)
        y.backward(gout.to(cuda))
    return x.grad, bn.weight.grad, bn.bias.grad


def mask_margin(d, relu, training):
    """The precondition of the ReLU cases, on the float64 restatement alone: the
    smallest |z64| - 2^-18 (|a x| + |b|) over all elements (positive: no
    pre-activation is close enough to zero for a float32 evaluation to flip)."""
    if not relu:
        return 1.0
    _, _, a, b = _stats64(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], training)
    ax = a * d["x"].double()
    return float(((ax + b).abs() - 2.0 ** -18 * (ax.abs() + b.abs())).min())


@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -10], ids=["g1", "g2^-10"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_against_float64(cuda, shape, training, relu, gscale):
    from sfm_amd.regularize import bn3_backward_f16, bn3_stats_f16
    d = _general(shape)
    assert mask_margin(d, relu, training) > 0.0              # a mask flip cannot explain a difference
    gout = (d["gout"].float() * gscale).half()
    x, gamma, beta = _dev(d, cuda, "x", "gamma", "beta")
    rm, rv = d["rm"].clone().to(cuda), d["rv"].clone().to(cuda)
    st = bn3_stats_f16(x, gamma, beta, EPS, rm, rv, MOM, training)
    gx, ggb = bn3_backward_f16(x, gout.to(cuda), st, relu, training)
    ref = _backward64(d, gout, relu, training)
    tor = _backward_modules(d, gout, relu, training, cuda)
    assert gx.dtype == torch.float16 and gx.shape == x.shape
    bad = []
    for name, ours, theirs, g64 in (("dx", gx, tor[0], ref[0]), ("dgamma", ggb[0], tor[1], ref[1]),
                                    ("dbeta", ggb[1], tor[2], ref[2])):
        e, t = _err(ours, g64), _err(theirs, g64)
        print({"shape": shape, "training": training, "relu": relu, "gscale": gscale, "grad": name, "err_hip": e,
               "err_modules_f16": t})
        if not e <= 2.0 * t:
            bad.append((name, e, t))
    assert not bad, bad


def test_two_calls_give_identical_bits(cuda):
    from sfm_amd.regularize import bn3_backward_f16, bn3_stats_f16
    d = _general(SHAPES[3])
    x, gout, gamma, beta = _dev(d, cuda, "x", "gout", "gamma", "beta")
    s1 = bn3_stats_f16(x, gamma, beta, EPS, None, None, MOM, True)
    s2 = bn3_stats_f16(x, gamma, beta, EPS, None, None, MOM, True)
    assert bool((s1 != 0).all()) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    a = bn3_backward_f16(x, gout, s1, True, True)
    b = bn3_backward_f16(x, gout, s1, True, True)
    assert bool((a[0] != 0).any()) and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_offsets_past_two_gigabytes(cuda):
    """voxels = 2^25 + 48: x is 2.1 GB, so the last voxels lie past 2^31 bytes.
    x is zero except for the last 48 voxels."""
    from sfm_amd.regularize import bn3_apply_f16, bn3_backward_f16, bn3_stats_f16
    n, tail = 2 ** 25 + 48, 48
    g = torch.Generator().manual_seed(9)
    tx = torch.randint(-8, 9, (tail, 32), generator=g)
    tg = torch.randint(-8, 9, (tail, 32), generator=g)
    x = torch.zeros(n, 32, dtype=torch.float16, device=cuda)
    x[-tail:] = tx.half().to(cuda)
    one, zero = torch.ones(32, device=cuda), torch.zeros(32, device=cuda)
    st = bn3_stats_f16(x, one, zero, EPS, None, None, MOM, True).cpu().double()
    mean64 = tx.double().sum(0) / n
    var64 = (tx.double() ** 2).sum(0) / n - mean64 ** 2
    assert bool(((st[0] - mean64).abs() <= 2.0 ** -23 * mean64.abs()).all())
    assert bool(((st[1] - var64).abs() <= 2.0 ** -23 * var64 + 2.0 ** -52 * (tx.double() ** 2).sum(0)).all())
    hand = torch.zeros(5, 32)
    hand[2], hand[3], hand[4] = 1.0, 2.0, 1.0
    hand = hand.to(cuda)
    out = bn3_apply_f16(x, hand, None, True)
    want = torch.relu(2.0 * tx.float() + 1.0).half()
    assert torch.equal(out[-tail:].cpu(), want) and bool((out[0] == 1).all()) and bool((out[2 ** 25 - 1] == 1).all())
    del out
    gy = torch.zeros(n, 32, dtype=torch.float16, device=cuda)
    gy[-tail:] = tg.half().to(cuda)
    gx, ggb = bn3_backward_f16(x, gy, hand, True, training=False)
    dy = tg.double() * (2.0 * tx.double() + 1.0 > 0).double()
    assert torch.equal(gx[-tail:].cpu().double(), 2.0 * dy) and bool((gx[0] == 0).all())
    assert torch.equal(ggb[1].cpu().double(), dy.sum(0))


# ---- batchnorm3_act_autograd ---------------------------------------------------------------------------------------
def _module(d, cuda, training):
    bn = nn.BatchNorm3d(32, eps=EPS, momentum=MOM).to(cuda).train(training)
    with torch.no_grad():
        for t, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "rm"), (bn.running_var, "rv")):
            t.copy_(d[k])
    return bn


def test_autograd_forward_bits_buffers_and_needs_input_grad(cuda):
    from sfm_amd import batchnorm3_act_autograd
    from sfm_amd.regularize import bn3_apply_f16, bn3_stats_f16
    d = _general(SHAPES[2])
    x, res, gout, gamma, beta = _dev(d, cuda, "x", "res", "gout", "gamma", "beta")
    for training in (True, False):
        rm, rv = d["rm"].clone().to(cuda), d["rv"].clone().to(cuda)
        st = bn3_stats_f16(x, gamma, beta, EPS, rm, rv, MOM, training)
        want = bn3_apply_f16(x, st, res, True)
        for need_x, need_p, need_r in ((True, True, True), (False, True, False), (True, False, False),
                                       (False, False, True), (False, False, False)):
            bn = _module(d, cuda, training)
            bn.weight.requires_grad_(need_p)
            bn.bias.requires_grad_(need_p)
            xa, ra = x.clone().requires_grad_(need_x), res.clone().requires_grad_(need_r)
            versions = bn.running_mean._version, bn.running_var._version
            y, n = _launches(lambda: batchnorm3_act_autograd(xa, bn, relu=True, residual=ra))
            assert n == {"bn3_stats": 1, "bn3_apply": 1, "bn3_bwd": 0}, n
            assert y.dtype == torch.float16 and torch.equal(y.view(torch.int16), want.view(torch.int16))
            assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
            if training:
                assert int(bn.num_batches_tracked) == 1
                assert bn.running_mean._version > versions[0] and bn.running_var._version > versions[1]
                assert not torch.equal(bn.running_mean.cpu(), d["rm"])
            else:
                assert int(bn.num_batches_tracked) == 0
                assert torch.equal(bn.running_mean.cpu(), d["rm"]) and torch.equal(bn.running_var.cpu(), d["rv"])
            if not (need_x or need_p or need_r):
                assert not y.requires_grad
                continue
            _, n = _launches(lambda: y.backward(gout))
            assert n["bn3_bwd"] == (1 if need_x or need_p else 0), n
            assert (xa.grad is not None) == need_x and (bn.weight.grad is not None) == need_p
            assert (bn.bias.grad is not None) == need_p and (ra.grad is not None) == need_r
            if need_r:
                assert torch.equal(ra.grad, gout)                      # the residual's gradient is grad_out itself
            if need_x:
                assert xa.grad.dtype == torch.float16 and xa.grad.shape == x.shape
            if need_p:
                assert bn.weight.grad.dtype == torch.float32 and bn.weight.grad.shape == (32,)


def test_autograd_refuses_non_stock_modules_and_cpu_tensors(cuda):
    from sfm_amd import batchnorm3_act_autograd
    x = _general(SHAPES[1])["x"].to(cuda)
    for bad in (nn.BatchNorm3d(32, affine=False), nn.BatchNorm3d(32, track_running_stats=False),
                nn.BatchNorm3d(32, momentum=None), nn.BatchNorm3d(16), nn.BatchNorm2d(32)):
        with pytest.raises(RuntimeError):
            batchnorm3_act_autograd(x, bad.to(cuda))
    hooked = nn.BatchNorm3d(32).to(cuda)
    handle = hooked.register_forward_hook(lambda m, i, o: None)
    with pytest.raises(RuntimeError, match="hooks"):
        batchnorm3_act_autograd(x, hooked)
    handle.remove()
    assert batchnorm3_act_autograd(x, hooked).shape == x.shape
    with pytest.raises(RuntimeError, match="device tensor"):
        batchnorm3_act_autograd(x.cpu(), hooked)
    with pytest.raises(RuntimeError, match="float32 on x's device"):
        batchnorm3_act_autograd(x, nn.BatchNorm3d(32))
    with pytest.raises(RuntimeError, match="residual"):
        batchnorm3_act_autograd(x, hooked, residual=x.float())
    with pytest.raises(RuntimeError, match="more than one value"):
        batchnorm3_act_autograd(x[:, :1, :1, :1], hooked.train())
