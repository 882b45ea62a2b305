"""PSNet's differentiable route under float16 autocast with the stack's Conv3d
layers on libsfm_hip (``regularize_grad``): a training step runs, reaches every
parameter, launches the forward and weight-gradient kernels, and its stack
gradients meet the float16 rule -- err = max|g - g64| / max|g64| against a
float64 restatement on the CPU, at most 2 x the error of the same net with
regularize_grad="torch" under the same autocast.  The scene and the small
feature net are those of test_gpu_psnet_train.py, restated here."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, L, IH, IW = 2, 4, 32, 48
MIN_DEPTH = 1.0
NAMES = ("conv3_f16", "conv3_wgrad", "sweep_bwd", "depth_head_bwd", "depth_head")


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


def _net(cuda, **kw):
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(PSNET_CONTEXT=True)
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
    planes = costs[:, 0].permute(1, 0, 2, 3).reshape(L * B, 1, h, w)
    x = torch.cat([rf.unsqueeze(0).expand(L, B, C, h, w).reshape(L * B, C, h, w), planes], 1)
    costss = (net.convs(x) + planes).reshape(L, B, h, w).permute(1, 0, 2, 3)
    outs = _head(costs[:, 0], IH, IW), _head(costss, IH, IW)
    _loss(outs, gt.double()).backward()
    return net


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def test_fp16_training_step(cuda):
    import sfm_amd.psnet as P
    scene = _scene()
    net = _net(cuda, regularize_grad="fp16").train()
    tor = _net(cuda, regularize_grad="torch").train()
    n64 = _restated64(net, scene)
    outs, n = _launches(lambda: _step(net, scene, cuda))
    assert outs[0].shape == outs[1].shape == (B, 1, IH, IW) and outs[0].grad_fn is not None
    assert n["conv3_f16"] == 25 and n["conv3_wgrad"] == 12, n           # 12 forward, 13 data-gradient, 12 weight-gradient
    assert n["sweep_bwd"] >= 1, n
    assert n["depth_head_bwd"] == (2 if P.HEAD_BWD_HIP else 0) and n["depth_head"] == (2 if P.HEAD_BWD_HIP else 0), n
    _, nt = _launches(lambda: _step(tor, scene, cuda))
    assert nt["conv3_f16"] == 0 and nt["conv3_wgrad"] == 0 and nt["sweep_bwd"] >= 1, nt
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k
    for name in ("dres0.0.0.weight", "dres4.2.0.weight", "classify.2.weight"):
        g64 = dict(n64.named_parameters())[name].grad
        ours = _err(dict(net.named_parameters())[name].grad, g64)
        theirs = _err(dict(tor.named_parameters())[name].grad, g64)
        print({"param": name, "err_fp16_hip": ours, "err_torch_autocast": theirs})
        assert ours <= 2.0 * theirs, (name, ours, theirs)


def test_auto_follows_the_flag_and_hooks(cuda, monkeypatch):
    import sfm_amd.psnet as P
    net = _net(cuda).train()
    for flag in (True, False):
        monkeypatch.setattr(P, "STACK_BWD_HIP", flag)
        with torch.autocast("cuda", torch.float16):
            assert net.regularize_grad_route(cuda) == ("fp16" if flag else "torch")
        assert net.regularize_grad_route(cuda) == "torch"                # no autocast: the float32 modules
        with torch.autocast("cuda", torch.bfloat16):
            assert net.regularize_grad_route(cuda) == "torch"
    monkeypatch.setattr(P, "STACK_BWD_HIP", True)
    handle = net.dres2.register_forward_hook(lambda m, i, o: None)
    with torch.autocast("cuda", torch.float16):
        assert net.regularize_grad_route(cuda) == "torch"
        handle.remove()
        assert net.regularize_grad_route(cuda) == "fp16"
        # and the step takes what the route says
        scene = _scene()
        _, n = _launches(lambda: _step(net, scene, cuda))
        assert n["conv3_wgrad"] == 12, n


def test_forced_fp16_without_autocast_raises(cuda):
    net = _net(cuda, regularize_grad="fp16").train()
    with pytest.raises(RuntimeError, match="autocast"):
        _run(net, _scene(), cuda, autocast=False)


def test_float32_route_is_unchanged(cuda, monkeypatch):
    """No autocast: no weight-gradient kernel whatever the flag says, and the
    output bits of a regularize_grad="torch" net."""
    import sfm_amd.psnet as P
    monkeypatch.setattr(P, "STACK_BWD_HIP", True)
    scene = _scene()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        res = []
        for rg in ("auto", "torch"):
            net = _net(cuda, regularize_grad=rg).train()
            outs, n = _launches(lambda: _step(net, scene, cuda, autocast=False))
            assert n["conv3_wgrad"] == 0 and n["conv3_f16"] == 0, n
            res.append((outs, net))
    finally:
        torch.backends.cudnn.deterministic = det
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
