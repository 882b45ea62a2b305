"""PSNet's differentiable route under float16 autocast with the whole 3-D
stack on libsfm_hip: ``regularize_grad="fp16"`` (the Conv3d layers) together
with ``regularize_norm="hip"`` (every BatchNorm3d, ReLU and residual add).  A
training step runs, reaches every parameter, launches the kernels it should,
and its stack gradients meet the float16 rule -- err = max|g - g64| / max|g64|
against a float64 restatement on the CPU, at most 2 x the error of the same net
with regularize_grad="torch" under the same autocast.  The scene and the small
feature net are those of test_gpu_psnet_train_fp16.py, restated here."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, L, IH, IW = 2, 4, 32, 48
MIN_DEPTH = 1.0
NAMES = ("conv3_f16", "conv3_wgrad", "bn3_stats", "bn3_apply", "bn3_bwd", "sweep_bwd")


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


def _step(net, scene, cuda):
    ref, tgt, K, pose, gt = (t.to(cuda) for t in scene)
    with torch.autocast("cuda", torch.float16):
        outs = net(ref, [tgt], pose.unsqueeze(1).clone(), K, torch.inverse(K))
    _loss(outs, gt).backward()
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


def test_fp16_training_step_with_hip_norm(cuda):
    scene = _scene()
    net = _net(cuda, regularize_grad="fp16", regularize_norm="hip").train()
    tor = _net(cuda, regularize_grad="torch").train()
    n64 = _restated64(net, scene)
    outs, n = _launches(lambda: _step(net, scene, cuda))
    assert outs[0].shape == outs[1].shape == (B, 1, IH, IW) and outs[0].grad_fn is not None
    assert n["conv3_f16"] == 25 and n["conv3_wgrad"] == 12, n
    assert n["bn3_stats"] == 11 and n["bn3_apply"] == 11 and n["bn3_bwd"] == 11, n
    assert n["sweep_bwd"] >= 1, n
    _step(tor, scene, cuda)
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k
    for k, b in net.named_buffers():
        if k.endswith("num_batches_tracked") and k.startswith(("dres", "classify")):
            assert int(b) == 1, k
    bad = []
    for name in ("dres0.0.0.weight", "dres4.2.0.weight", "classify.2.weight", "dres0.0.1.weight", "dres4.2.1.bias"):
        g64 = dict(n64.named_parameters())[name].grad
        ours = _err(dict(net.named_parameters())[name].grad, g64)
        theirs = _err(dict(tor.named_parameters())[name].grad, g64)
        print({"param": name, "err_fp16_hip_norm": ours, "err_torch_autocast": theirs})
        if not ours <= 2.0 * theirs:
            bad.append((name, ours, theirs))
    assert not bad, bad


def test_default_net_launches_no_bn3_kernel(cuda):
    """regularize_norm defaults to "torch": the default route's Conv3d kernels
    run (float16 autocast, regularize_grad "auto") and no sfm_bn3_* launch does;
    on the "torch" route the argument has no effect."""
    import sfm_amd.psnet as P
    scene = _scene()
    net = _net(cuda).train()
    assert net.regularize_norm == "torch"
    _, n = _launches(lambda: _step(net, scene, cuda))
    assert n["bn3_stats"] == 0 and n["bn3_apply"] == 0 and n["bn3_bwd"] == 0, n
    assert n["conv3_wgrad"] == (12 if P.STACK_BWD_HIP else 0), n
    tor = _net(cuda, regularize_grad="torch", regularize_norm="hip").train()
    _, n = _launches(lambda: _step(tor, scene, cuda))
    assert n["bn3_stats"] == 0 and n["bn3_apply"] == 0 and n["bn3_bwd"] == 0 and n["conv3_wgrad"] == 0, n
