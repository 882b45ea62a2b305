"""basic_block_autograd (sfm_amd/feature.py): one reference BasicBlock
(models/submodule.py:22-44) forward and backward on libsfm_hip, with no torch
batch_norm on the device -- conv2x_autograd and batchnorm2_act_autograd only.

Nothing here calls torch's batch_norm, an nn.BatchNorm* module or a stock CNN
module on a device tensor: the stock block runs on the CPU (float64 as the
reference, float32 with float16 roundings as the comparison arm); on the device
its modules are containers of parameters and buffers.

Three block kinds at small maps, 2 images: 32 -> 32 at stride 1 (9 x 13),
32 -> 64 at stride 2 with the 1 x 1 stride-2 downsample (9 x 13), 128 -> 128 at
dilation 2 (6 x 10)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

gpu = pytest.mark.gpu

#        cin, cout, stride, dilation, (h, w)
KINDS = {"32to32": (32, 32, 1, 1, (9, 13)), "32to64s2": (32, 64, 2, 1, (9, 13)), "128d2": (128, 128, 1, 2, (6, 10))}
N = 2
MOM = 0.1


def _bns(blk):
    return [(n, m) for n, m in blk.named_modules() if isinstance(m, nn.BatchNorm2d)]


def _f16_values(t):
    return bool((t.detach().double() == t.detach().half().double()).all())


def _to64(blk):
    """The stock block in float64 on the CPU; its in-place ReLU made out of place so that hooks see every value."""
    b = copy.deepcopy(blk).cpu().double()
    b.conv1[1] = nn.ReLU()
    return b


def _run64(blk, x, gout):
    """out, dx (channels last) and the parameter gradients of the stock block in float64 on the CPU."""
    b64 = _to64(blk)
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    out = b64(x64)
    out.backward(gout.double().permute(0, 3, 1, 2))
    grads = {n: p.grad for n, p in b64.named_parameters()}
    return out.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1), grads, b64


def _run_hip(fn, blk, x, gout, cuda):
    """fn(block on the device, x) -> out, dx, parameter gradients, the block (all on the device)."""
    bd = copy.deepcopy(blk).to(cuda)
    xd = x.to(cuda).requires_grad_()
    out = fn(bd, xd)
    out.backward(gout.to(cuda))
    return out.detach(), xd.grad, {n: p.grad for n, p in bd.named_parameters()}, bd


def _chain(blk, x, taps=None):
    """The block written out in conv2x_autograd / batchnorm2_act_autograd calls; ``taps`` collects each
    BatchNorm2d's input."""
    from sfm_amd.feature import batchnorm2_act_autograd, conv2x_autograd
    taps = {} if taps is None else taps
    (c1, b1), (c2, b2) = blk.conv1[0], blk.conv2
    shortcut = x
    if blk.downsample is not None:
        cd, bd = blk.downsample
        taps["downsample.1"] = yd = conv2x_autograd(x, cd.weight, cd.stride[0], 1)
        shortcut = batchnorm2_act_autograd(yd, bd)
    taps["conv1.0.1"] = y1 = conv2x_autograd(x, c1.weight, c1.stride[0], c1.dilation[0])
    z1 = batchnorm2_act_autograd(y1, b1, relu=True)
    taps["conv2.1"] = y2 = conv2x_autograd(z1, c2.weight, 1, c2.dilation[0])
    return batchnorm2_act_autograd(y2, b2, residual=shortcut)


# ---- general values ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _general(kind, training=True, seed=5):
    """The stock block on the CPU with float16-valued conv weights (the HIP route reads them as float16) and
    general BatchNorm2d state, its input and output gradient (float16, channels last).  Shared, left unchanged."""
    from sfm_amd.psnet import _Residual
    cin, cout, stride, dil, (h, w) = KINDS[kind]
    g = torch.Generator().manual_seed(seed + cin + cout)
    blk = _Residual(cin, cout, stride, 1, dil).train(training)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.Conv2d):
                k = m.kernel_size[0] ** 2 * m.in_channels
                m.weight.copy_((torch.randn(m.weight.shape, generator=g) * (2.0 / k) ** 0.5).half().float())
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(1.0 + 0.3 * torch.randn(c, generator=g))
                m.bias.copy_(0.3 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = (0.3 + torch.randn(N, h, w, cin, generator=g)).half()
    gout = torch.randn(N, ho, wo, cout, generator=g).half()
    return blk, x, gout


class _Round(torch.autograd.Function):
    """The identity that rounds to float16 in both directions: a module boundary under float16 autocast."""
    @staticmethod
    def forward(ctx, t):
        return t.half().float()

    @staticmethod
    def backward(ctx, g):
        return g.half().float()


def _run_arm(blk, x, gout, rounding=True, seen=None):
    """The comparison arm, on the CPU: the stock block's own modules in float32, every module boundary rounded to
    float16 in both directions, conv weight gradients rounded to float16 as autocast's float16 conv returns them."""
    b = copy.deepcopy(blk).cpu().float()

    def r(t):
        if not rounding:
            return t
        if seen is not None:
            t.register_hook(seen.append)                     # the gradient that leaves the boundary
        t = _Round.apply(t)
        if seen is not None:
            seen.append(t)
        return t
    xl = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_()
    xr = r(xl)
    (c1, b1), (c2, b2) = b.conv1[0], b.conv2
    shortcut = xr if b.downsample is None else r(b.downsample[1](r(b.downsample[0](xr))))
    z1 = r(torch.relu(r(b1(r(c1(xr))))))
    out = r(r(b2(r(c2(z1)))) + shortcut)
    out.backward(gout.float().permute(0, 3, 1, 2))
    grads = {n: p.grad for n, p in b.named_parameters()}
    if rounding:
        for n, m in b.named_modules():
            if isinstance(m, nn.Conv2d):
                grads[n + ".weight"] = m.weight.grad.half().float()
    return out.detach().permute(0, 2, 3, 1), xl.grad.permute(0, 2, 3, 1), grads, b


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


@pytest.mark.parametrize("kind", list(KINDS))
def test_comparison_arm_is_the_stock_block_with_float16_boundaries(kind):
    """No GPU.  Without its roundings the arm is the float64 block to float32
    accuracy (the same graph); with them every boundary value and gradient and
    every conv weight gradient is a float16 value, and the arm differs from
    float64 by more than float32 rounding (the roundings are in it)."""
    blk, x, gout = _general(kind)
    out64, dx64, g64, _ = _run64(blk, x, gout)
    out, dx, grads, _ = _run_arm(blk, x, gout, rounding=False)
    assert _err(out, out64) <= 1e-5 and _err(dx, dx64) <= 1e-5
    assert set(grads) == set(g64) and all(_err(grads[n], g64[n]) <= 1e-4 for n in g64)
    seen = []
    out, dx, grads, _ = _run_arm(blk, x, gout, seen=seen)
    assert len(seen) >= 14 and all(_f16_values(t) for t in seen) and _f16_values(out) and _f16_values(dx)
    assert all(_f16_values(grads[n]) for n in grads if grads[n].dim() == 4)
    assert 1e-5 < _err(out, out64) < 1e-2 and 1e-5 < _err(dx, dx64)


@gpu
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_block_is_the_chain_of_its_ops_bit_for_bit(cuda, kind, training):
    from sfm_amd import basic_block_autograd
    blk, x, gout = _general(kind, training)
    out, dx, grads, b1 = _run_hip(basic_block_autograd, blk, x, gout, cuda)
    cout, cdx, cgrads, b2 = _run_hip(_chain, blk, x, gout, cuda)
    assert out.dtype == torch.float16 and out.shape == gout.shape and out.is_contiguous()
    assert torch.equal(out.view(torch.int16), cout.view(torch.int16))
    assert dx.dtype == torch.float16 and torch.equal(dx.view(torch.int16), cdx.view(torch.int16))
    assert set(grads) == set(cgrads) and len(grads) == (9 if blk.downsample is not None else 6)
    for n in grads:
        assert grads[n].dtype == torch.float32 and torch.equal(grads[n].view(torch.int32), cgrads[n].view(torch.int32)), n
    for (n, m1), (_, m2) in zip(_bns(b1), _bns(b2)):
        assert torch.equal(m1.running_mean, m2.running_mean) and torch.equal(m1.running_var, m2.running_var), n
        assert int(m1.num_batches_tracked) == int(m2.num_batches_tracked) == (1 if training else 0)


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_training_step_against_float64_next_to_the_float16_arm(cuda, kind):
    """err = max|g - g64| / max|g64| against the stock block in float64 on the
    CPU, for the output, dx and every parameter: at most 2 x the error of the
    stock block's modules with float16 module boundaries (the CPU arm)."""
    from sfm_amd import basic_block_autograd
    blk, x, gout = _general(kind)
    out64, dx64, g64, _ = _run64(blk, x, gout)
    aout, adx, agrads, _ = _run_arm(blk, x, gout)
    out, dx, grads, _ = _run_hip(basic_block_autograd, blk, x, gout, cuda)
    rows = [("out", out, aout, out64), ("dx", dx, adx, dx64)] + [(n, grads[n], agrads[n], g64[n]) for n in g64]
    bad = []
    for name, ours, arm, ref in rows:
        e, t = _err(ours, ref), _err(arm, ref)
        print({"kind": kind, "tensor": name, "err_hip": e, "err_arm_f16": t})
        if not e <= 2.0 * t:
            bad.append((name, e, t))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_buffers_agree_with_the_float64_block(cuda, kind):
    """Every BatchNorm2d's running statistics and num_batches_tracked after one
    training step.  Against torch's rule in float64 on the layer's own float16
    input y (the chain's conv output): the statistics bounds of
    tests/test_gpu_bn2.py, 2^-23 |mean| and 2^-23 var + N 2^-52 E[y^2], through
    the rule, plus one float32 rounding.  Against the float64 block, whose
    layer input y64 differs from y by d = y - y64: in addition |mean(y) -
    mean(y64)| <= mean|d| and |var(y) - var(y64)| <= 2 mean(|y64 - mean64| |d|)
    + mean(d^2), both identities of the mean and the variance."""
    from sfm_amd import basic_block_autograd
    blk, x, gout = _general(kind)
    b64, acts64 = _to64(blk), {}
    for n, m in _bns(b64):
        m.register_forward_pre_hook(lambda mod, inp, n=n: acts64.__setitem__(n, inp[0].detach()))
    b64(x.double().permute(0, 3, 1, 2))                      # one training step of the float64 block
    taps = {}
    _run_hip(lambda b, xd: _chain(b, xd, taps), blk, x, gout, cuda)
    _, _, _, bd = _run_hip(basic_block_autograd, blk, x, gout, cuda)
    start = dict(blk.named_modules())
    for n, m in _bns(bd):
        C = m.num_features
        y = taps[n].detach().cpu().double().reshape(-1, C)
        y64 = acts64[n].permute(0, 2, 3, 1).reshape(-1, C)
        cnt = y.shape[0]
        d = (y - y64).abs()
        rm0, rv0 = start[n].running_mean.double(), start[n].running_var.double()
        for src, dm, dv in ((y, 0.0, 0.0),
                            (y64, d.mean(0), 2.0 * ((y64 - y64.mean(0)).abs() * d).mean(0) + (d * d).mean(0))):
            mean, var = src.mean(0), ((src - src.mean(0)) ** 2).mean(0)
            rm = (1 - MOM) * rm0 + MOM * mean
            rv = (1 - MOM) * rv0 + MOM * var * cnt / (cnt - 1)
            bm = MOM * (2.0 ** -23 * mean.abs() + dm) + 2.0 ** -24 * rm.abs()
            bv = MOM * (2.0 ** -23 * var + cnt * 2.0 ** -52 * (src * src).mean(0) + dv) * cnt / (cnt - 1) + 2.0 ** -24 * rv.abs()
            em, ev = (m.running_mean.cpu().double() - rm).abs(), (m.running_var.cpu().double() - rv).abs()
            print({"kind": kind, "bn": n, "against": "own input" if src is y else "float64 block",
                   "mean err/bound": float((em / bm).max()), "var err/bound": float((ev / bv).max())})
            assert bool((em <= bm).all()) and bool((ev <= bv).all()), n
        assert int(m.num_batches_tracked) == int(dict(b64.named_modules())[n].num_batches_tracked) == 1


# ---- exact values, eval mode ---------------------------------------------------------------------------------------
EPS_EXACT = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def _exact(kind):
    """Weights in {-1, 0, 1} (about four live taps per output channel and input row of the kernel), inputs in
    [-2, 2], output gradients in [-1, 1]; BatchNorm2d in eval mode with eps 2^-10, running_var s^2 - 2^-10 (s 1 or
    2, so var + eps = s^2 and invstd = 1 / s exactly), gamma +-1, integer beta and running_mean: a = +-1 or +-1/2, b
    a multiple of 1/2."""
    from sfm_amd.psnet import _Residual
    cin, cout, stride, dil, (h, w) = KINDS[kind]
    g = torch.Generator().manual_seed(11 + cin + cout)
    blk = _Residual(cin, cout, stride, 1, dil).eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.Conv2d):
                live = (torch.rand(m.weight.shape, generator=g) < 4.0 / m.in_channels).float()
                m.weight.copy_(live * (1 - 2 * torch.randint(0, 2, m.weight.shape, generator=g)).float())
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.eps = EPS_EXACT
                m.weight.copy_((1 - 2 * torch.randint(0, 2, (c,), generator=g)).float())
                m.bias.copy_(torch.randint(-2, 3, (c,), generator=g).float())
                m.running_mean.copy_(torch.randint(-2, 3, (c,), generator=g).float())
                m.running_var.copy_(torch.randint(1, 3, (c,), generator=g).float() ** 2 - EPS_EXACT)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randint(-2, 3, (N, h, w, cin), generator=g).half()
    gout = torch.randint(-1, 2, (N, ho, wo, cout), generator=g).half()
    return blk, x, gout


def _exact_reference(kind):
    """The stock block in float64 on the CPU with every module's output and every gradient that reaches one."""
    blk, x, gout = _exact(kind)
    b64 = _to64(blk)
    seen = []

    def keep(mod, inp, out):
        seen.append(out.detach())
        out.register_hook(seen.append)
    for m in b64.modules():
        if isinstance(m, (nn.Conv2d, nn.BatchNorm2d, nn.ReLU)):
            m.register_forward_hook(keep)
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    out = b64(x64)
    out.backward(gout.double().permute(0, 3, 1, 2))
    grads = {n: p.grad for n, p in b64.named_parameters()}
    return out.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1), grads, seen


@pytest.mark.parametrize("kind", list(KINDS))
def test_exact_case_holds_float16_values_throughout(kind):
    """No GPU: every intermediate of the float64 evaluation -- each module's
    output, each gradient that reaches one, the result and dx -- is a float16
    value, and the parameter gradients are float32 values: one rounding or
    many, any order of summation, the result is the same."""
    out, dx, grads, seen = _exact_reference(kind)
    assert len(seen) >= 10 and all(_f16_values(t) for t in seen) and _f16_values(out) and _f16_values(dx)
    assert all(bool((g == g.float().double()).all()) for g in grads.values())
    assert float(out.abs().max()) > 4 and float(dx.abs().max()) >= 1 and all(bool((g != 0).any()) for g in grads.values())


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_exact_case_bit_for_bit(cuda, kind):
    """Output, dx and every parameter gradient equal the float64 evaluation of
    the stock block (by value: a zero may carry either sign); eval mode leaves
    the buffers alone."""
    from sfm_amd import basic_block_autograd
    blk, x, gout = _exact(kind)
    out64, dx64, g64, _ = _exact_reference(kind)
    out, dx, grads, bd = _run_hip(basic_block_autograd, blk, x, gout, cuda)
    assert out.dtype == torch.float16 and torch.equal(out.cpu().double(), out64)
    assert dx.dtype == torch.float16 and torch.equal(dx.cpu().double(), dx64)
    assert set(grads) == set(g64)
    for n in g64:
        assert torch.equal(grads[n].cpu().double(), g64[n]), n
    for (n, m), (_, m0) in zip(_bns(bd), _bns(blk)):
        assert torch.equal(m.running_mean.cpu(), m0.running_mean) and torch.equal(m.running_var.cpu(), m0.running_var)
        assert int(m.num_batches_tracked) == 0
