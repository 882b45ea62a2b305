"""CostRegularization.forward_differentiable(norm="hip") on the GPU: the
twelve-layer stack with every BatchNorm3d, ReLU and residual add on libsfm_hip
(batchnorm3_act_autograd: sfm_bn3_stats_f16, sfm_bn3_apply_f16,
sfm_bn3_backward_f16) between the sfm_conv3_f16 / sfm_conv3_wgrad_f16 layers.

The seeded stack and the rule are those of test_gpu_conv3_backward.py, restated
here: err = max|g - g64| / max|g64| against a float64 copy of the modules on the
CPU, at most 2 x the error of the modules under float16 autocast on the GPU,
measured in the same test."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RB, RL, Rh, Rw = 2, 4, 8, 12
NAMES = ("conv3_f16", "conv3_wgrad", "bn3_stats", "bn3_apply", "bn3_bwd")


def _launches(fn):
    from sfm_amd import _lib
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, {k: _lib.profile_read(k)[1] for k in NAMES}


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def _stack(reg, cost):
    c0 = reg.dres0(cost)
    for i in range(1, 5):
        c0 = getattr(reg, f"dres{i}")(c0) + c0
    return reg.classify(c0)


@functools.lru_cache(maxsize=None)
def _reg_case(training):
    """The seeded stack, its input and output gradient, and one step of the
    float64 copy on the CPU (computed once, shared, left unchanged)."""
    from sfm_amd.regularize import CostRegularization
    torch.manual_seed(21)
    reg = CostRegularization(64).train(training)
    g = torch.Generator().manual_seed(22)
    for m in reg.modules():                      # running statistics and affines away from 0 / 1, so eval mode uses them
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.copy_(0.1 * torch.randn(32, generator=g))
            m.running_var.copy_(1.0 + 0.5 * torch.rand(32, generator=g))
            m.weight.data.copy_(1.0 + 0.2 * torch.randn(32, generator=g))
            m.bias.data.copy_(0.1 * torch.randn(32, generator=g))
    cost = torch.randn(RB, 64, RL, Rh, Rw, generator=g)
    gout = torch.randn(RB, 1, RL, Rh, Rw, generator=g)
    r64 = copy.deepcopy(reg).double()
    c64 = cost.double().requires_grad_()
    out64 = _stack(r64, c64)
    out64.backward(gout.double())
    return reg, cost, gout, r64, c64.grad, out64.detach()


def _arm(reg, cost, gout, cuda, norm):
    """norm "hip" / "torch": forward_differentiable; None: the modules."""
    r = copy.deepcopy(reg).to(cuda)
    c = cost.to(cuda).requires_grad_()
    with torch.autocast("cuda", torch.float16):
        out = _stack(r, c) if norm is None else r.forward_differentiable(c, norm=norm)
    if gout is not None:
        out.float().backward(gout.to(cuda))
    return r, c.grad, out.detach().float()


def test_training_step(cuda):
    """Training mode: the output, the input gradient, all 12 conv weights, the
    22 BatchNorm parameters and the 22 running statistics after the step,
    against the float64 copy, next to the modules under float16 autocast."""
    reg, cost, gout, r64, gin64, out64 = _reg_case(True)
    (rh, gin_h, out_h), n = _launches(lambda: _arm(reg, cost, gout, cuda, "hip"))
    assert n == {"conv3_f16": 12 + 12 + 1, "conv3_wgrad": 12, "bn3_stats": 11, "bn3_apply": 11, "bn3_bwd": 11}, n
    rt, gin_t, out_t = _arm(reg, cost, gout, cuda, None)
    assert out_h.shape == (RB, 1, RL, Rh, Rw)
    p64, ph, pt = (dict(r.named_parameters()) for r in (r64, rh, rt))
    rows = [("input", gin_h, gin_t, gin64), ("output", out_h, out_t, out64)]
    rows += [(k, ph[k].grad, pt[k].grad, p64[k].grad) for k in p64]
    b64, bh, bt = (dict(r.named_buffers()) for r in (r64, rh, rt))
    rows += [(k, bh[k], bt[k], b64[k]) for k in b64 if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(rows) == 2 + 12 + 22 + 22
    bad = []
    for k, ours, theirs, ref in rows:
        assert ours is not None and bool(torch.isfinite(ours).all()), k
        e, t = _err(ours, ref), _err(theirs, ref)
        print({"tensor": k, "err_hip_norm": e, "err_modules_f16": t})
        if not e <= 2.0 * t:
            bad.append((k, e, t))
    assert not bad, bad
    for k in b64:
        if k.endswith("num_batches_tracked"):
            assert int(bh[k]) == int(b64[k]) == 1


def test_eval_mode(cuda):
    """Eval mode: the statistics launch is the finalize kernel alone (no pass
    over x), the buffers stay put, the output meets the same rule."""
    reg, cost, _, r64, _, out64 = _reg_case(False)
    (rh, _, out_h), n = _launches(lambda: _arm(reg, cost, None, cuda, "hip"))
    assert n == {"conv3_f16": 12, "conv3_wgrad": 0, "bn3_stats": 11, "bn3_apply": 11, "bn3_bwd": 0}, n
    _, _, out_t = _arm(reg, cost, None, cuda, None)
    e, t = _err(out_h, out64), _err(out_t, out64)
    print({"tensor": "eval output", "err_hip_norm": e, "err_modules_f16": t})
    assert e <= 2.0 * t, (e, t)
    for k, v in reg.named_buffers():
        assert torch.equal(dict(rh.named_buffers())[k].cpu(), v), k


def test_torch_norm_launches_no_bn3_kernel_and_unknown_norm_raises(cuda):
    reg, cost, gout, *_ = _reg_case(True)
    (_, gin_a, out_a), n = _launches(lambda: _arm(reg, cost, gout, cuda, "torch"))
    assert n == {"conv3_f16": 25, "conv3_wgrad": 12, "bn3_stats": 0, "bn3_apply": 0, "bn3_bwd": 0}, n
    # and it is the default
    r = copy.deepcopy(reg).to(cuda)
    with torch.autocast("cuda", torch.float16):
        out_b = r.forward_differentiable(cost.to(cuda))
    assert torch.equal(out_a, out_b.detach().float())
    with pytest.raises(ValueError, match="norm"):
        r.forward_differentiable(cost.to(cuda), norm="fused")
