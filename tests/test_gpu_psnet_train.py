"""PSNet's differentiable route (sfm_amd/psnet.py): with grad mode on and
features that require grad, forward runs the differentiable sweep, the stacks as
the modules they are and the differentiable head, so a loss on both outputs
back-propagates into every parameter.  Checked against a pure-torch restatement
of the same graph (a per-plane grid_sample loop, the F.interpolate head) in
float64 on the CPU, next to the same restatement in float32 on the GPU, under
the bar of tests/test_gpu_depth_head_backward.py:
err = max|g - g64| / max|g64| <= max(2 x torch's float32 err, 1e-5)."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, L, IH, IW = 2, 4, 32, 48
MIN_DEPTH = 1.0


def _launches(fn):
    """test_gpu_context.py's launch-name hook, reading the backward kernels' names."""
    from sfm_amd import _lib
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, {k: _lib.profile_read(k)[1] for k in ("sweep_bwd", "depth_head_bwd", "depth_head")}


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
    return F.smooth_l1_loss(outs[0], gt) + F.smooth_l1_loss(outs[1], gt)


def _run(net, scene, cuda):
    ref, tgt, K, pose, gt = (t.to(cuda) for t in scene)
    return net(ref, [tgt], pose.unsqueeze(1).clone(), K, torch.inverse(K))


def _head(cost, H, W):
    up = F.interpolate(cost.unsqueeze(1), [L, H, W], mode="trilinear", align_corners=False)[:, 0]
    idx = torch.arange(1, L + 1, dtype=cost.dtype, device=cost.device).reshape(1, L, 1, 1)
    return MIN_DEPTH * L / ((F.softmax(up, dim=1) * idx).sum(1, keepdim=True) + 1e-16)


def _restated(net, scene, dtype, device):
    """The same graph in torch ops alone, on a copy of the modules in ``dtype``
    on ``device``: PSNet.py:138-216 with one target.  The sampling grids are the
    float32 ones of the sweep (oracle.sweep.warp_grid, the kernel's own
    positions), constants of the graph in every arm."""
    from oracle import sweep as S
    net = copy.deepcopy(net).to(device=device, dtype=dtype)
    ref, tgt, K, pose, gt = scene
    K4, Ki4 = S.quarter_intrinsics(K, torch.inverse(K))
    rf = net.feature_extraction(ref.to(device=device, dtype=dtype))
    tf = net.feature_extraction(tgt.to(device=device, dtype=dtype))
    _, C, h, w = rf.shape
    far = torch.ones(B, h, w) * MIN_DEPTH * L
    grids = [S.warp_grid(torch.div(far, i + 1 + 1e-16), pose, K4, Ki4, h, w).to(device=device, dtype=dtype)
             for i in range(L)]
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
    _loss(outs, gt.to(device=device, dtype=dtype)).backward()
    return net, outs


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def test_training_step_gradients(cuda):
    """forward + backward of a smooth-L1 on both outputs in training mode: it
    runs (the parent raised "forward-only"), every parameter gets a finite
    non-zero gradient, the HIP backward kernels ran, and the gradients of the
    feature conv and of the last classify conv meet the bar."""
    import sfm_amd.psnet as P
    scene = _scene()
    net = _net(cuda).train()
    n64, _ = _restated(net, scene, torch.float64, "cpu")
    n32, _ = _restated(net, scene, torch.float32, cuda)

    def step():
        outs = _run(net, scene, cuda)
        _loss(outs, scene[4].to(cuda)).backward()
        return outs
    outs, n = _launches(step)
    assert outs[0].shape == outs[1].shape == (B, 1, IH, IW) and outs[0].grad_fn is not None
    assert n["sweep_bwd"] >= 1, n
    assert n["depth_head_bwd"] == (2 if P.HEAD_BWD_HIP else 0) and n["depth_head"] == (2 if P.HEAD_BWD_HIP else 0), n
    names = [k for k, _ in net.named_parameters()]
    assert any(k.startswith("feature_extraction.") for k in names) and any(k.startswith("convs.") for k in names)
    assert any(k.startswith("dres4.") for k in names) and any(k.startswith("classify.") for k in names)
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k
    for name in ("feature_extraction.weight", "classify.2.weight"):
        g64 = dict(n64.named_parameters())[name].grad
        ours = _err(dict(net.named_parameters())[name].grad, g64)
        theirs = _err(dict(n32.named_parameters())[name].grad, g64)
        bar = max(2.0 * theirs, 1e-5)
        print({"param": name, "err_route": ours, "err_torch_f32": theirs, "bar": bar})
        assert ours <= bar, (name, ours, theirs, bar)


def test_eval_mode_with_grad_takes_the_same_route(cuda):
    """Eval mode outside no_grad: the differentiable route, whose outputs match
    the forward-only conv_precision="fp32" route of the same net within the
    regularisation tests' depth bars (median 1e-5, max 1e-3 relative)."""
    scene = _scene()
    net = _net(cuda, conv_precision="fp32").eval()
    outs, n = _launches(lambda: _run(net, scene, cuda))
    assert outs[0].grad_fn is not None and outs[1].grad_fn is not None and n["sweep_bwd"] == 0
    with torch.no_grad():
        want = _run(net, scene, cuda)
    assert want[0].grad_fn is None
    for got, ref in zip(outs, want):
        rel = ((got.detach() - ref).abs() / ref.abs()).flatten()
        print({"median": float(rel.median()), "max": float(rel.max())})
        assert float(rel.median()) <= 1e-5 and float(rel.max()) <= 1e-3, (float(rel.median()), float(rel.max()))


def test_no_grad_in_training_mode_is_unchanged(cuda):
    """Under torch.no_grad() the forward-only route runs as before: no backward
    link, and the bits of context_precision="torch" (as
    test_gpu_context.py::test_auto_stays_on_torch_elsewhere compares them)."""
    scene = _scene()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        outs = []
        for cp in ("auto", "torch"):
            net = _net(cuda, context_precision=cp).train()
            with torch.no_grad():
                out, n = _launches(lambda: _run(net, scene, cuda))
            assert n["depth_head"] == 2 and n["depth_head_bwd"] == 0 and out[0].grad_fn is None, n
            outs.append(out)
    finally:
        torch.backends.cudnn.deterministic = det
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(outs[0][0], outs[0][1])


def test_forced_hip_stacks_have_no_backward(cuda):
    """A forced "fp16" context precision keeps raising in training mode, and is
    refused on the differentiable route in eval mode instead of dropping the gradient."""
    scene = _scene()
    net = _net(cuda, context_precision="fp16").train()
    with pytest.raises(RuntimeError, match="eval"):
        _run(net, scene, cuda)
    with pytest.raises(RuntimeError, match="no backward"):
        _run(net.eval(), scene, cuda)
