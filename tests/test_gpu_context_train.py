"""The context stack's float16 training route on the GPU
(``sfm_amd.context.context_refine_autograd``, PSNet's ``context_grad``): the
forward's bits, every gradient against a float64 restatement on the CPU next to
the modules under float16 autocast (ours at most 2 x theirs, err = max|g - g64|
/ max|g64|), the chunking, the refusals, and a PSNet training step.  The stack
shape is test_gpu_context.py's; the scene, the small feature net and the
float64 graph are those of test_gpu_psnet_train_fp16.py, rebuilt here."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SB, SL, SH, SW = 2, 3, 19, 70           # the whole-stack shape
NAMES = ("conv2_wgrad", "conv2_dgrad", "context_conv2", "context_pack", "context_unpack_grad")


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


def _convs(bn=False):
    from sfm_amd.psnet import _context_stack
    torch.manual_seed(11)
    convs = _context_stack(33, bn)
    for m in convs.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return convs


def _stack(convs, ctx, costs):
    """PSNet.forward's own application of the stack (L-major images), [B, 1, L, h, w]."""
    B, _, L, h, w = costs.shape
    planes = costs[:, 0].permute(1, 0, 2, 3).reshape(L * B, 1, h, w)
    x = torch.cat([ctx.unsqueeze(0).expand(L, B, ctx.shape[1], h, w).reshape(L * B, -1, h, w), planes], 1)
    return (convs(x) + planes).reshape(L, B, h, w).permute(1, 0, 2, 3).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def _case():
    """(convs, ctx, costs, upstream gradient, float64 gradients {name: tensor})."""
    from sfm_amd import synth
    convs = _convs()
    g = torch.Generator().manual_seed(7)
    ctx = synth.features(SB, 32, SH, SW, seed=6)[0]
    costs = torch.randn(SB, 1, SL, SH, SW, generator=g)
    go = torch.randn(SB, 1, SL, SH, SW, generator=g)
    c64 = copy.deepcopy(convs).double()
    ctx64 = ctx.double().requires_grad_(True)
    costs64 = costs.double().requires_grad_(True)
    _stack(c64, ctx64, costs64).backward(go.double())
    g64 = {k: p.grad for k, p in c64.named_parameters()}
    g64["ctx"], g64["costs"] = ctx64.grad, costs64.grad
    return convs, ctx, costs, go, g64


def _grads(convs, fn, ctx, costs, go, cuda):
    """Gradients {name: tensor} of ``fn(convs, ctx, costs)`` under float16 autocast on a fresh device copy."""
    convs = copy.deepcopy(convs).to(cuda)
    ctx = ctx.to(cuda).requires_grad_(True)
    costs = costs.to(cuda).requires_grad_(True)
    with torch.autocast("cuda", torch.float16):
        out = fn(convs, ctx, costs)
    out.backward(go.to(cuda))
    g = {k: p.grad for k, p in convs.named_parameters()}
    g["ctx"], g["costs"] = ctx.grad, costs.grad
    return out.detach(), g


def test_forward_bits_and_every_gradient(cuda):
    from sfm_amd.context import context_refine, context_refine_autograd
    convs, ctx, costs, go, g64 = _case()
    (out, ours), n = _launches(lambda: _grads(convs, context_refine_autograd, ctx, costs, go, cuda))
    assert n["conv2_wgrad"] == 7 and n["conv2_dgrad"] == 7 and n["context_unpack_grad"] == 1, n
    assert n["context_conv2"] == 7 and n["context_pack"] == 1, n
    want = context_refine(copy.deepcopy(convs).to(cuda), ctx.to(cuda), costs.to(cuda), precision="fp16")
    assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), want.view(torch.int32))
    _, theirs = _grads(convs, _stack, ctx, costs, go, cuda)
    assert set(ours) == set(g64) and len(ours) == 9
    for k in sorted(g64):
        assert ours[k].dtype == theirs[k].dtype == torch.float32 and ours[k].shape == g64[k].shape, k
        rec = {"grad": k, "err_fp16_hip": _err(ours[k], g64[k]), "err_torch_autocast": _err(theirs[k], g64[k])}
        print(rec)
        assert rec["err_fp16_hip"] <= 2.0 * rec["err_torch_autocast"], rec
    # the same call again: the same bits
    _, again = _grads(convs, context_refine_autograd, ctx, costs, go, cuda)
    for k in ours:
        assert torch.equal(ours[k].view(torch.int32), again[k].view(torch.int32)), k


def test_one_plane_per_chunk(cuda):
    """max_scratch_bytes forcing one plane per chunk: the ctx / costs gradient
    bits of one chunk; weight gradients (fp32 sums over the chunks, another
    order) within 2 x the modules' error."""
    from sfm_amd.context import context_refine_autograd, planes_per_chunk
    convs, ctx, costs, go, g64 = _case()
    assert planes_per_chunk(SB, SH, SW, SL, 1) == 1
    _, whole = _grads(convs, context_refine_autograd, ctx, costs, go, cuda)
    (out1, one), n = _launches(lambda: _grads(
        convs, lambda c, a, b: context_refine_autograd(c, a, b, max_scratch_bytes=1), ctx, costs, go, cuda))
    assert n["conv2_wgrad"] == 7 * SL and n["conv2_dgrad"] == 7 * SL and n["context_unpack_grad"] == SL, n
    for k in ("ctx", "costs"):
        assert torch.equal(one[k].view(torch.int32), whole[k].view(torch.int32)), k
    _, theirs = _grads(convs, _stack, ctx, costs, go, cuda)
    for k in sorted(g64):
        rec = {"grad": k, "err_fp16_hip_chunked": _err(one[k], g64[k]), "err_torch_autocast": _err(theirs[k], g64[k])}
        print(rec)
        assert rec["err_fp16_hip_chunked"] <= 2.0 * rec["err_torch_autocast"], rec


def test_refusals(cuda):
    from sfm_amd.context import ContextStackError, context_refine_autograd
    _, ctx, costs, _, _ = _case()
    ctx, costs = ctx.to(cuda), costs.to(cuda)
    bn = _convs(bn=True).to(cuda).train()
    with torch.autocast("cuda", torch.float16):
        with pytest.raises(ContextStackError, match="BatchNorm2d in training mode"):
            context_refine_autograd(bn, ctx, costs)
        with pytest.raises(ContextStackError, match="BatchNorm2d"):
            context_refine_autograd(bn.eval(), ctx, costs)
        with pytest.raises(ContextStackError):
            context_refine_autograd(_convs()[:6].to(cuda), ctx, costs)         # does not end in one channel
        with pytest.raises(RuntimeError, match="device tensors"):
            context_refine_autograd(_convs().to(cuda), ctx.cpu(), costs)
    plain = _convs().to(cuda)
    with pytest.raises(RuntimeError, match="autocast"):
        context_refine_autograd(plain, ctx, costs)
    with torch.autocast("cuda", torch.bfloat16):
        with pytest.raises(RuntimeError, match="autocast"):
            context_refine_autograd(plain, ctx, costs)


# --- PSNet(context_grad=...) ---------------------------------------------------------
B, L, IH, IW = 2, 4, 32, 48
MIN_DEPTH = 1.0


def _net(cuda, **kw):
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(PSNET_CONTEXT=True, **kw.pop("cfg", {}))
    torch.manual_seed(4)
    net = PSNet(L, MIN_DEPTH, cfg=c, feature_fn=nn.Conv2d(3, 32, 4, stride=4), **kw)
    return net.to(cuda)


def _scene():
    from sfm_amd import synth
    gen = torch.Generator().manual_seed(12)
    ref = torch.randn(B, 3, IH, IW, generator=gen)
    tgt = torch.randn(B, 3, IH, IW, generator=gen)
    K = synth.intrinsics(B, float(IW), float(IW), IW / 2.0, IH / 2.0)
    pose = synth.relative_pose(B, gen)
    pose[:, :, 3] *= 0.2                       # a baseline the L = 4 planes (depths 4 .. 1) keep in view
    gt = 1.0 + 3.0 * torch.rand(B, 1, IH, IW, generator=gen)
    return ref, tgt, K, pose, gt


def _loss(outs, gt):
    return F.smooth_l1_loss(outs[0].float(), gt) + F.smooth_l1_loss(outs[1].float(), gt)


def _run(net, scene, cuda, autocast=True):
    ref, tgt, K, pose, gt = (t.to(cuda) for t in scene)
    with torch.autocast("cuda", torch.float16, enabled=autocast):
        return net(ref, [tgt], pose.unsqueeze(1).clone(), K, torch.inverse(K))


def _step(net, scene, cuda, autocast=True):
    outs = _run(net, scene, cuda, autocast)
    _loss(outs, scene[4].to(cuda)).backward()
    return outs


def _head(cost, H, W):
    up = F.interpolate(cost.unsqueeze(1), [L, H, W], mode="trilinear", align_corners=False)[:, 0]
    idx = torch.arange(1, L + 1, dtype=cost.dtype, device=cost.device).reshape(1, L, 1, 1)
    return MIN_DEPTH * L / ((F.softmax(up, dim=1) * idx).sum(1, keepdim=True) + 1e-16)


def _restated64(net, scene):
    """The same graph in torch ops alone on a float64 copy of the modules on
    the CPU (PSNet.py:138-216 with one target); the sampling grids are the
    float32 ones of the sweep, constants of the graph."""
    from oracle import sweep as S
    net = copy.deepcopy(net).to(device="cpu", dtype=torch.float64)
    ref, tgt, K, pose, gt = scene
    K4, Ki4 = S.quarter_intrinsics(K, torch.inverse(K))
    rf = net.feature_extraction(ref.double())
    tf = net.feature_extraction(tgt.double())
    _, C, h, w = rf.shape
    far = torch.ones(B, h, w) * MIN_DEPTH * L
    grids = [S.warp_grid(torch.div(far, i + 1 + 1e-16), pose, K4, Ki4, h, w).double() for i in range(L)]
    warped = torch.stack([F.grid_sample(tf, gr, mode="bilinear", padding_mode="zeros", align_corners=True)
                          for gr in grids], 2)
    cost = torch.cat([rf.unsqueeze(2).expand(B, C, L, h, w), warped], 1).contiguous()
    c0 = net.dres0(cost)
    for i in range(1, 5):
        c0 = getattr(net, f"dres{i}")(c0) + c0
    costs = net.classify(c0)
    costss = _stack(net.convs, rf, costs)[:, 0]
    outs = _head(costs[:, 0], IH, IW), _head(costss, IH, IW)
    _loss(outs, gt.double()).backward()
    return net


def test_psnet_training_step(cuda):
    scene = _scene()
    net = _net(cuda, context_grad="fp16").train()
    tor = _net(cuda, context_grad="torch").train()
    n64 = _restated64(net, scene)
    outs, n = _launches(lambda: _step(net, scene, cuda))
    assert outs[0].shape == outs[1].shape == (B, 1, IH, IW) and outs[1].grad_fn is not None
    assert n["conv2_wgrad"] == 7 and n["conv2_dgrad"] == 7, n             # one chunk of planes
    _, nt = _launches(lambda: _step(tor, scene, cuda))
    assert nt["conv2_wgrad"] == 0 and nt["conv2_dgrad"] == 0 and nt["context_conv2"] == 0, nt
    for k, p in net.convs.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k
    for name in ("convs.0.0.weight", "convs.6.0.weight", "feature_extraction.weight"):
        g64 = dict(n64.named_parameters())[name].grad
        ours = _err(dict(net.named_parameters())[name].grad, g64)
        theirs = _err(dict(tor.named_parameters())[name].grad, g64)
        print({"param": name, "err_context_fp16_hip": ours, "err_context_torch": theirs})
        assert ours <= 2.0 * theirs, (name, ours, theirs)


def test_default_route_is_unchanged(cuda):
    """The default net launches neither backward kernel and gives the output
    bits of context_grad="torch" spelled out."""
    scene = _scene()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        res = []
        for kw in ({}, {"context_grad": "torch"}):
            net = _net(cuda, **kw).train()
            assert net.context_grad == "torch"
            outs, n = _launches(lambda: _step(net, scene, cuda))
            assert n["conv2_wgrad"] == 0 and n["conv2_dgrad"] == 0 and n["context_unpack_grad"] == 0, n
            res.append(outs)
    finally:
        torch.backends.cudnn.deterministic = det
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_forced_fp16_outside_autocast_and_with_batchnorm_raises(cuda):
    from sfm_amd.context import ContextStackError
    net = _net(cuda, context_grad="fp16").train()
    with pytest.raises(RuntimeError, match="context_grad='fp16'.*autocast"):
        _run(net, _scene(), cuda, autocast=False)
    bn = _net(cuda, context_grad="fp16", cfg={"CONTEXT_BN": True}).train()
    with pytest.raises(ContextStackError, match="BatchNorm2d in training mode"):
        _run(bn, _scene(), cuda)
