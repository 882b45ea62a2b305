"""The float16 BatchNorm2d / ReLU / residual kernels on the GPU (csrc/bn2.hip on
csrc/bn_act.h): sfm_bn2_stats_f16, sfm_bn2_apply_f16, sfm_bn2_backward_f16 and
batchnorm2_act_autograd around them, at 32, 64 and 128 channels.

Nothing here calls torch's batch_norm, an nn.BatchNorm* module or a stock CNN
module on a device tensor: every reference is evaluated on the CPU.

Exact lattices must come back bit for bit.  General float16 values are held to
bounds that follow from float64 accumulation and one rounding (statistics,
apply: the forms of tests/test_gpu_bn3.py) and, for the backward, to a bound
per element of dx, dgamma and dbeta written as a sum of terms, each the effect
of one rounding the kernels make (``_bwd_bounds``; DESIGN.md §2.5 has the
derivation).  ``_emulate_backward`` is the kernels' formula in torch ops on the CPU at
the kernels' precisions; a CPU test holds it to the same bounds at every case,
so a bound that the formula itself cannot meet shows up without a GPU.

General values (``_general``, as tests/test_gpu_bn3.py's widened to C): per
channel a mean of a few units and a spread of 0.25 .. 1.75; channel 5 holds
256 + {-1, 0, 1} / 4.  Below 8 pixels the spread is scaled by 2^-9; from 8
pixels on the values lie on the grid of sixteenths, and the seed is one at
which no pre-activation is close enough to zero for a float32 evaluation to
flip the ReLU mask (``mask_margin`` > 0 in every C, shape and mode: searched on
the CPU, asserted in the tests)."""
import functools
from fractions import Fraction

import pytest
import torch
import torch.nn as nn

gpu = pytest.mark.gpu

CHANNELS = (32, 64, 128)
SHAPES = [
    (2, 1, 1),         # 2 pixels: the minimum training mode takes, and branch1's pooled map at batch 2
    (1, 3, 5),         # 15 pixels: less than one wave's coverage at C = 32, no multiple of 4, 8 or 16
    (2, 8, 12),        # 192 pixels
    (1, 37, 53),       # 1961 pixels: ragged, several blocks (16, 31, 62), the last one short
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
EPS, MOM = 1e-5, 0.1
SEED = 274
U, U64, H = 2.0 ** -24, 2.0 ** -53, 2.0 ** -11              # unit roundoffs: float32, float64, float16


def _launches(fn, names=("bn2_stats", "bn2_apply", "bn2_bwd")):
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
def _general(shape, C, seed=SEED):
    """Float16 operands on the CPU (shared, left unchanged)."""
    n = shape[0] * shape[1] * shape[2]
    g = torch.Generator().manual_seed(seed + n + C)
    mean = 2.0 * torch.randn(C, generator=g)
    spread = 0.25 + 1.5 * torch.rand(C, generator=g)
    if n < 8:
        spread = spread * 2.0 ** -9
    x = mean + spread * torch.randn(*shape, C, generator=g)
    if n >= 8:
        x = torch.round(x * 16.0) / 16.0
    x[..., 5] = 256.0 + 0.25 * torch.randint(-1, 2, shape, generator=g)
    d = dict(x=x.half(), res=torch.randn(*shape, C, generator=g).half(),
             gout=torch.randn(*shape, C, generator=g).half(),
             gamma=1.0 + 0.3 * torch.randn(C, generator=g), beta=0.3 * torch.randn(C, generator=g),
             rm=mean + 0.1 * spread * torch.randn(C, generator=g), rv=spread ** 2 * (0.5 + torch.rand(C, generator=g)))
    d["rm"][5], d["rv"][5] = 256.1, 0.05
    return d


def _stats64(x, gamma, beta, rm=None, rv=None, training=True):
    """mean, biased variance, a, b in float64 from the float16 values (two-pass variance)."""
    f = x.double().reshape(-1, x.shape[-1])
    if training:
        mean = f.mean(0)
        var = ((f - mean) ** 2).mean(0)
    else:
        mean, var = rm.double(), rv.double()
    a = gamma.double() / torch.sqrt(var + EPS)
    return mean, var, a, beta.double() - mean * a


def _dev(d, cuda, *keys):
    return [d[k].to(cuda) for k in keys]


def mask_margin(d, relu, training):
    """The precondition of the ReLU cases, on the float64 restatement alone: the
    smallest |z64| - 2^-18 (|a x| + |a mean| + |beta|) over all elements
    (positive: no pre-activation is close enough to zero for the kernels'
    float32 fma on float32 a and b to flip)."""
    if not relu:
        return 1.0
    mean, _, a, b = _stats64(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], training)
    ax = a * d["x"].double()
    return float(((ax + b).abs() - 2.0 ** -18 * (ax.abs() + (a * mean).abs() + d["beta"].double().abs())).min())


# ---- the kernels' formula on the CPU, and the derived bounds ------------------------------------------------------
def _emulate_stats(d, training):
    """The five rows as k_bn3_finalize derives them: float64 from float64 sums
    (E[x^2] - mean^2, clamped at 0), each rounded once to float32."""
    f = d["x"].double().reshape(-1, d["x"].shape[-1])
    n = f.shape[0]
    if training:
        mean = f.sum(0) / n
        var = ((f * f).sum(0) / n - mean * mean).clamp_min(0.0)
    else:
        mean, var = d["rm"].double(), d["rv"].double()
    invstd = 1.0 / torch.sqrt(var + EPS)
    a = d["gamma"].double() * invstd
    b = d["beta"].double() - mean * a
    return torch.stack([mean, var, invstd, a, b]).float()


def _emulate_backward(x, gout, st, relu, training):
    """k_bn3_bwd_reduce and k_bn3_bwd_apply in torch ops at their precisions:
    the mask from the float32 fma (evaluated exactly, rounded to float32), the
    two sums in float64, dgamma and the 1/n coefficients in float64 rounded to
    float32, then float32 (dy - k1) - ((x - mean) invstd) k2 and a t, one
    operation and one rounding each, and the one float16 rounding."""
    C = x.shape[-1]
    n = x.numel() // C
    mean_f, inv_f, a_f, b_f = st[0], st[2], st[3], st[4]
    xf, dy = x.float(), gout.float()
    if relu:
        z = (a_f.double() * xf.double() + b_f.double()).float()
        dy = torch.where(z > 0, dy, torch.zeros_like(dy))
    s1 = dy.double().reshape(-1, C).sum(0)
    s2 = (dy.double() * xf.double()).reshape(-1, C).sum(0)
    dbeta = s1
    dgamma = (s2 - mean_f.double() * s1) * inv_f.double()
    t = dy
    if training:
        k1, k2 = (dbeta / n).float(), (dgamma / n).float()
        xh = (xf - mean_f) * inv_f
        t = (dy - k1) - xh * k2
    return (a_f * t).half(), dgamma.float(), dbeta.float()


def _backward64(d, gout, relu, training):
    from sfm_amd.regularize import bn3_act_reference
    x = d["x"].double().requires_grad_()
    gam, bet = d["gamma"].double().requires_grad_(), d["beta"].double().requires_grad_()
    out, _, _ = bn3_act_reference(x, gam, bet, d["rm"], d["rv"], training, MOM, EPS, relu, d["res"].double())
    out.backward(gout.double())
    return x.grad, gam.grad, bet.grad


def _bwd_bounds(d, gout, relu, training):
    """(bound dx [.., C], bound dgamma [C], bound dbeta [C]) in float64, from the
    float64 restatement's own quantities: each line is one named rounding of the
    kernels ("the backward's bound")."""
    x = d["x"]
    C = x.shape[-1]
    f = x.double().reshape(-1, C)
    n = f.shape[0]
    mean, var, a, b = _stats64(x, d["gamma"], d["beta"], d["rm"], d["rv"], training)
    invstd = 1.0 / torch.sqrt(var + EPS)
    g = gout.double().reshape(-1, C)
    if relu:
        g = g * ((a * f + b) > 0).double()
    dbeta = g.sum(0)
    dgamma = (g * (f - mean)).sum(0) * invstd
    A1, A2 = g.abs().sum(0), (g * f).abs().sum(0)
    zero = torch.zeros(C, dtype=torch.float64)
    # the variance: float64 sums of n exact terms and E[x^2] - mean^2 in float64 -> relative effect on invstd and a
    rel_var = (3 * n + 3) * U64 * (f * f).mean(0) / (2.0 * (var + EPS)) if training else zero
    # mean to float32 (and its float64 sum); eval mode reads the float32 running mean: no error
    d_mean = U * mean.abs() + n * U64 * f.abs().mean(0) if training else zero
    rel_inv = U + rel_var + 2 * U64                            # invstd to float32 (sqrt, divide in float64)
    rel_a = U + rel_var + 3 * U64                              # a = gamma invstd to float32
    # float64 sums of dy and dy x (n exact terms each, any order) and the float64 operations on them
    sums = 4 * n * U64 * (A2 + mean.abs() * A1) * invstd
    b_beta = U * dbeta.abs() + n * U64 * A1 + 2.0 ** -150      # dbeta to float32
    b_gamma = (U * dgamma.abs()                                # dgamma to float32
               + rel_inv * dgamma.abs()                        # the float32 invstd it is formed with
               + d_mean * dbeta.abs() * invstd                 # the float32 mean it is formed with
               + sums + 2.0 ** -150)
    if training:
        k1, k2 = dbeta / n, dgamma / n
        xh = (f - mean) * invstd
        T = g - k1 - xh * k2
        e_k1 = U * k1.abs() + U64 * A1                         # dbeta / n to float32
        e_k2 = b_gamma / n                                     # dgamma / n to float32 (its rounding for dgamma's)
        e_d = U * (f - mean).abs() + d_mean                    # float32 x - mean on the float32 mean
        e_xh = invstd * e_d + (rel_inv + U) * xh.abs()         # float32 (x - mean) invstd on the float32 invstd
        e_p = k2.abs() * e_xh + xh.abs() * e_k2 + U * (xh * k2).abs()      # float32 xhat k2
        e_s = e_k1 + U * (g - k1).abs()                        # float32 dy - k1
        e_T = e_s + e_p + U * T.abs()                          # float32 (dy - k1) - xhat k2
    else:
        T, e_T = g, torch.zeros_like(g)
    dx = a * T
    e_m = a.abs() * e_T + (rel_a + U) * dx.abs()               # float32 a t on the float32 a
    # second-order products of the above, then the one float16 rounding of the computed value and its subnormal step
    b_x = (1.0 + 2.0 ** -20) * (1.0 + H) * e_m + H * dx.abs() + 2.0 ** -25
    return b_x.reshape(x.shape), b_gamma, b_beta


CASES = [(s, t, r, gs) for s in SHAPES for t in (True, False) for r in (False, True) for gs in (1.0, 2.0 ** -10)]
CASE_IDS = ["-".join(("x".join(map(str, s)), "train" if t else "eval", "relu" if r else "lin",
                      "g1" if gs == 1.0 else "g2^-10")) for s, t, r, gs in CASES]


def _ratios(got, ref, bounds):
    return [float(((o.detach().double().cpu() - r).abs() / bd).max()) for o, r, bd in zip(got, ref, bounds)]


@pytest.mark.parametrize("C", CHANNELS)
def test_mask_margin_and_emulation_inside_the_bounds_on_the_cpu(C):
    """No GPU: at every case the seed's mask margin is positive, and the
    kernels' formula at the kernels' precisions lies inside the derived bounds
    against float64 autograd of bn3_act_reference."""
    worst = [0.0, 0.0, 0.0]
    for shape, training, relu, gscale in CASES:
        d = _general(shape, C)
        assert mask_margin(d, relu, training) > 0.0, (shape, training, relu)
        gout = (d["gout"].float() * gscale).half()
        st = _emulate_stats(d, training)
        got = _emulate_backward(d["x"], gout, st, relu, training)
        r = _ratios(got, _backward64(d, gout, relu, training), _bwd_bounds(d, gout, relu, training))
        assert max(r) <= 1.0, (shape, training, relu, gscale, r)
        worst = [max(w, v) for w, v in zip(worst, r)]
    print({"C": C, "emulation err/bound (dx, dgamma, dbeta)": worst})
    # the bounds are not slack by orders of magnitude: the formula uses a tenth of dx's somewhere
    assert worst[0] >= 0.1


# ---- exact lattices ------------------------------------------------------------------------------------------------
LATTICE = (4, 16, 16)                                       # 1024 pixels: a power of two


@functools.lru_cache(maxsize=None)
def _lattice(C):
    g = torch.Generator().manual_seed(3 + C)
    x = torch.randint(-8, 9, LATTICE + (C,), generator=g)
    res = torch.randint(-8, 9, LATTICE + (C,), generator=g)
    gout = torch.randint(-8, 9, LATTICE + (C,), generator=g)
    stats = torch.zeros(5, C)
    stats[0] = torch.randint(-3, 4, (C,), generator=g).float()              # mean: integers
    stats[1] = 1.0
    stats[2] = 2.0 ** torch.randint(-2, 3, (C,), generator=g).float()       # invstd: powers of two
    stats[3] = (2.0 ** torch.randint(-2, 3, (C,), generator=g).float()) * (1 - 2 * torch.randint(0, 2, (C,), generator=g))
    stats[4] = torch.randint(-8, 9, (C,), generator=g).float()              # b: integers
    return x, res, gout, stats


@gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_lattice_statistics_bit_for_bit(cuda, C):
    """Integers in [-8, 8], 1024 pixels: both sums are exact in any order, mean
    = S / N and var = Q / N - mean^2 are exact in float64, so rows 0 and 1 are
    the exact rationals rounded once to float32 -- at one block, few blocks, a
    count that divides nothing and more blocks than pixels, and the default."""
    from sfm_amd import _lib
    from sfm_amd.feature import bn2_stats_f16
    x = _lattice(C)[0]
    f = x.reshape(-1, C)
    n = f.shape[0]
    S, Q = f.sum(0).tolist(), (f * f).sum(0).tolist()
    mean = torch.tensor([float(Fraction(s, n)) for s in S], dtype=torch.float64).float()
    var = torch.tensor([float(Fraction(q * n - s * s, n * n)) for s, q in zip(S, Q)], dtype=torch.float64).float()
    xd = x.half().to(cuda)
    one, zero = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    try:
        for nb in (1, 3, 7, 4096, 0):
            _lib.tune("bn_blocks", nb)
            st = bn2_stats_f16(xd, one, zero, EPS, None, None, MOM, True).cpu()
            assert st.shape == (5, C)
            assert torch.equal(st[0].view(torch.int32), mean.view(torch.int32)), nb
            assert torch.equal(st[1].view(torch.int32), var.view(torch.int32)), nb
            inv = 1.0 / torch.sqrt(var.double() + EPS)
            assert float((st[2].double() - inv).abs().max()) <= 2.0 ** -22 * float(inv.max()), nb
            assert torch.equal(st[2], st[3])                                    # gamma 1: a is invstd
    finally:
        _lib.tune("bn_blocks", 0)                               # not enumerated, so no fixture restores it


@gpu
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("resid", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("C", CHANNELS)
def test_lattice_apply_and_eval_backward_bit_for_bit(cuda, C, relu, resid):
    """Hand-written statistics (a a signed power of two, b, mean and the
    residual integers): a x + b + res is a multiple of 1/4 below 2^7, exact in
    float32 and float16, so apply equals the CPU's float32 evaluation bit for
    bit; so does the eval-mode backward, dx = a dy, dbeta an exact integer sum,
    dgamma an exact multiple of 1/4 -- with and without grad_x."""
    from sfm_amd.feature import bn2_apply_f16, bn2_backward_f16
    x, res, gout, stats = _lattice(C)
    a, b = stats[3], stats[4]
    z = a * x.float() + b
    want = torch.relu(z) if relu else z
    want = (want + res.float() if resid else want).half()
    xd, rd, gd, sd = x.half().to(cuda), res.half().to(cuda), gout.half().to(cuda), stats.to(cuda)
    got = bn2_apply_f16(xd, sd, rd if resid else None, relu)
    assert got.dtype == torch.float16 and torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    dy = gout.double() * ((z > 0).double() if relu else 1.0)
    gx, ggb = bn2_backward_f16(xd, gd, sd, relu, training=False)
    # by value: where the mask is shut both sides hold a zero, whose sign is that of a here and of a dy there
    assert gx.dtype == torch.float16 and torch.equal(gx.cpu(), (a.double() * dy).half())
    dyf, xf = dy.reshape(-1, C), x.double().reshape(-1, C)
    dbeta = dyf.sum(0)
    dgamma = ((dyf * xf).sum(0) - stats[0].double() * dbeta) * stats[2].double()
    assert ggb.shape == (2, C)
    assert torch.equal(ggb[1].cpu().double(), dbeta) and torch.equal(ggb[0].cpu().double(), dgamma)
    none, only = bn2_backward_f16(xd, gd, sd, relu, training=False, need_grad_x=False)
    assert none is None and torch.equal(only, ggb)


# ---- statistics and apply, general values ---------------------------------------------------------------------------
def _stat_bounds(x):
    f = x.double().reshape(-1, x.shape[-1])
    n = f.shape[0]
    mean = f.mean(0)
    var = ((f - mean) ** 2).mean(0)
    return n, mean, var, 2.0 ** -23 * mean.abs(), 2.0 ** -23 * var + n * 2.0 ** -52 * (f * f).mean(0)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("C", CHANNELS)
def test_statistics_against_float64(cuda, C, shape):
    """|mean - mean64| <= 2^-23 |mean64| and |var - var64| <= 2^-23 var64 + N 2^-52
    E[x^2]: float64 sums of exact terms, one rounding to float32.  a and b follow
    from the kernel's own mean and variance to two float32 roundings.  The
    running statistics after one and two steps: the same bounds through torch's
    rule, plus one float32 rounding per step.  Then eval mode."""
    from sfm_amd.feature import bn2_stats_f16
    d = _general(shape, C)
    d2 = _general(shape, C, seed=77)
    gamma, beta = _dev(d, cuda, "gamma", "beta")
    rm, rv = d["rm"].clone().to(cuda), d["rv"].clone().to(cuda)
    rm64, rv64 = d["rm"].double(), d["rv"].double()
    em = torch.zeros(C, dtype=torch.float64)
    ev = torch.zeros(C, dtype=torch.float64)
    for step, dd in enumerate((d, d2)):
        n, mean64, var64, bm, bv = _stat_bounds(dd["x"])
        st = bn2_stats_f16(dd["x"].to(cuda), gamma, beta, EPS, rm, rv, MOM, True).cpu().double()
        dm, dv = (st[0] - mean64).abs(), (st[1] - var64).abs()
        print({"C": C, "shape": shape, "step": step, "mean_err/bound": float((dm / bm.clamp_min(1e-300)).max()),
               "var_err/bound": float((dv / bv.clamp_min(1e-300)).max()), "ch5_var": float(st[1][5]),
               "ch5_var64": float(var64[5])})
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
    st = bn2_stats_f16(d["x"].to(cuda), gamma, beta, EPS, rm, rv, MOM, False).cpu()
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1])
    assert torch.equal(st[0], rm.cpu()) and torch.equal(st[1], rv.cpu())
    a = d["gamma"].double() / torch.sqrt(rv.cpu().double() + EPS)
    assert bool(((st[3].double() - a).abs() <= 2.0 ** -23 * a.abs()).all())


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("C", CHANNELS)
def test_apply_against_float64_on_its_own_statistics(cuda, C, shape):
    """Per element |z - z64| <= 2^-11 |z64| + 2^-21 (|a x| + |b| + |res|) + 2^-24:
    one float16 rounding, float32 arithmetic before it, the float16 subnormal
    step."""
    from sfm_amd.feature import bn2_apply_f16, bn2_stats_f16
    d = _general(shape, C)
    x, res, gamma, beta = _dev(d, cuda, "x", "res", "gamma", "beta")
    st = bn2_stats_f16(x, gamma, beta, EPS, None, None, MOM, True)
    a, b = st[3].cpu().double(), st[4].cpu().double()
    ax = a * d["x"].double()
    for relu in (False, True):
        for resid in (False, True):
            z64 = ax + b
            z64 = torch.relu(z64) if relu else z64
            r64 = d["res"].double() if resid else torch.zeros_like(z64)
            z64 = z64 + r64
            got = bn2_apply_f16(x, st, res if resid else None, relu).cpu().double()
            bound = 2.0 ** -11 * z64.abs() + 2.0 ** -21 * (ax.abs() + b.abs() + r64.abs()) + 2.0 ** -24
            worst = float(((got - z64).abs() / bound).max())
            print({"C": C, "shape": shape, "relu": relu, "resid": resid, "err/bound": worst})
            assert worst <= 1.0, (relu, resid, worst)


# ---- backward, general values --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,training,relu,gscale", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("C", CHANNELS)
def test_backward_inside_the_derived_bounds(cuda, C, shape, training, relu, gscale):
    """dx, dgamma and dbeta against float64 autograd of bn3_act_reference on the
    CPU, each element within ``_bwd_bounds``."""
    from sfm_amd.feature import bn2_backward_f16, bn2_stats_f16
    d = _general(shape, C)
    assert mask_margin(d, relu, training) > 0.0              # a mask flip cannot explain a difference
    gout = (d["gout"].float() * gscale).half()
    x, gamma, beta = _dev(d, cuda, "x", "gamma", "beta")
    rm, rv = d["rm"].clone().to(cuda), d["rv"].clone().to(cuda)
    st = bn2_stats_f16(x, gamma, beta, EPS, rm, rv, MOM, training)
    gx, ggb = bn2_backward_f16(x, gout.to(cuda), st, relu, training)
    assert gx.dtype == torch.float16 and gx.shape == x.shape and ggb.shape == (2, C)
    r = _ratios((gx, ggb[0], ggb[1]), _backward64(d, gout, relu, training), _bwd_bounds(d, gout, relu, training))
    print({"C": C, "shape": shape, "training": training, "relu": relu, "gscale": gscale, "dx err/bound": r[0],
           "dgamma err/bound": r[1], "dbeta err/bound": r[2]})
    assert max(r) <= 1.0, r


@gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_two_calls_give_identical_bits(cuda, C):
    from sfm_amd.feature import bn2_backward_f16, bn2_stats_f16
    d = _general(SHAPES[3], C)
    x, gout, gamma, beta = _dev(d, cuda, "x", "gout", "gamma", "beta")
    s1 = bn2_stats_f16(x, gamma, beta, EPS, None, None, MOM, True)
    s2 = bn2_stats_f16(x, gamma, beta, EPS, None, None, MOM, True)
    assert bool((s1 != 0).all()) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    a = bn2_backward_f16(x, gout, s1, True, True)
    b = bn2_backward_f16(x, gout, s1, True, True)
    assert bool((a[0] != 0).any()) and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- batchnorm2_act_autograd ---------------------------------------------------------------------------------------
def _module(d, C, cuda, training):
    """A stock module with the case's parameters, built on the CPU and moved:
    it is never called on a device tensor."""
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOM).train(training)
    with torch.no_grad():
        for t, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "rm"), (bn.running_var, "rv")):
            t.copy_(d[k])
    return bn.to(cuda)


@gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_autograd_forward_bits_buffers_and_needs_input_grad(cuda, C):
    from sfm_amd import batchnorm2_act_autograd
    from sfm_amd.feature import bn2_apply_f16, bn2_backward_f16, bn2_stats_f16
    d = _general(SHAPES[2], C)
    x, res, gout, gamma, beta = _dev(d, cuda, "x", "res", "gout", "gamma", "beta")
    n, mean64, var64, bm, bv = _stat_bounds(d["x"])
    for training in (True, False):
        rm, rv = d["rm"].clone().to(cuda), d["rv"].clone().to(cuda)
        st = bn2_stats_f16(x, gamma, beta, EPS, rm, rv, MOM, training)
        want = bn2_apply_f16(x, st, res, True)
        wgx, wggb = bn2_backward_f16(x, gout, st, True, training)
        for need_x, need_p, need_r in ((True, True, True), (False, True, False), (True, False, False),
                                       (False, False, True), (False, False, False)):
            bn = _module(d, C, cuda, training)
            bn.weight.requires_grad_(need_p)
            bn.bias.requires_grad_(need_p)
            xa, ra = x.clone().requires_grad_(need_x), res.clone().requires_grad_(need_r)
            versions = bn.running_mean._version, bn.running_var._version
            y, cnt = _launches(lambda: batchnorm2_act_autograd(xa, bn, relu=True, residual=ra))
            assert cnt == {"bn2_stats": 1, "bn2_apply": 1, "bn2_bwd": 0}, cnt
            assert y.dtype == torch.float16 and torch.equal(y.view(torch.int16), want.view(torch.int16))
            assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
            if training:
                # torch's rule, evaluated on the CPU in float64: (1 - m) r + m batch, the batch variance unbiased
                assert int(bn.num_batches_tracked) == 1
                assert bn.running_mean._version > versions[0] and bn.running_var._version > versions[1]
                rm64 = (1 - MOM) * d["rm"].double() + MOM * mean64
                rv64 = (1 - MOM) * d["rv"].double() + MOM * var64 * n / (n - 1)
                assert bool(((bn.running_mean.cpu().double() - rm64).abs() <= MOM * bm + 2.0 ** -24 * rm64.abs()).all())
                assert bool(((bn.running_var.cpu().double() - rv64).abs()
                             <= MOM * bv * n / (n - 1) + 2.0 ** -24 * rv64.abs()).all())
                assert not torch.equal(bn.running_mean.cpu(), d["rm"])
            else:
                assert int(bn.num_batches_tracked) == 0
                assert torch.equal(bn.running_mean.cpu(), d["rm"]) and torch.equal(bn.running_var.cpu(), d["rv"])
            if not (need_x or need_p or need_r):
                assert not y.requires_grad
                continue
            _, cnt = _launches(lambda: y.backward(gout))
            assert cnt == {"bn2_stats": 0, "bn2_apply": 0, "bn2_bwd": 1 if need_x or need_p else 0}, cnt
            assert (xa.grad is not None) == need_x and (bn.weight.grad is not None) == need_p
            assert (bn.bias.grad is not None) == need_p and (ra.grad is not None) == need_r
            if need_r:
                assert torch.equal(ra.grad, gout)                      # the residual's gradient is grad_out itself
            if need_x:
                assert xa.grad.dtype == torch.float16 and torch.equal(xa.grad.view(torch.int16), wgx.view(torch.int16))
            if need_p:
                assert bn.weight.grad.dtype == torch.float32 and bn.weight.grad.shape == (C,)
                assert torch.equal(bn.weight.grad, wggb[0]) and torch.equal(bn.bias.grad, wggb[1])


@gpu
def test_autograd_refuses_non_stock_modules_and_bad_tensors(cuda):
    from sfm_amd import batchnorm2_act_autograd
    x = _general(SHAPES[1], 64)["x"].to(cuda)
    for bad in (nn.BatchNorm2d(64, affine=False), nn.BatchNorm2d(64, track_running_stats=False),
                nn.BatchNorm2d(64, momentum=None), nn.BatchNorm2d(32), nn.BatchNorm3d(64)):
        with pytest.raises(RuntimeError):
            batchnorm2_act_autograd(x, bad.to(cuda))
    hooked = nn.BatchNorm2d(64).to(cuda)
    handle = hooked.register_forward_hook(lambda m, i, o: None)
    with pytest.raises(RuntimeError, match="hooks"):
        batchnorm2_act_autograd(x, hooked)
    handle.remove()
    assert batchnorm2_act_autograd(x, hooked).shape == x.shape
    with pytest.raises(RuntimeError, match="device tensor"):
        batchnorm2_act_autograd(x.cpu(), hooked)
    with pytest.raises(RuntimeError, match="float32 on x's device"):
        batchnorm2_act_autograd(x, nn.BatchNorm2d(64))
    with pytest.raises(RuntimeError, match="residual"):
        batchnorm2_act_autograd(x, hooked, residual=x.float())
    with pytest.raises(RuntimeError, match="more than one value"):
        batchnorm2_act_autograd(x[:, :1, :1], hooked.train())
    with pytest.raises(RuntimeError, match="32, 64 or 128"):
        batchnorm2_act_autograd(torch.zeros(1, 2, 3, 96, dtype=torch.float16, device=cuda), nn.BatchNorm2d(96).to(cuda))
