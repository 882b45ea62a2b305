"""The full-resolution refinement stack's float16 training route on the GPU
(``sfm_amd.context.dep_context_refine_autograd``, PSNet's ``dep_context_grad``;
models/PSNet.py:218-221): the forward's bits, every gradient against a float64
restatement on the CPU next to the modules under float16 autocast (ours at most
2 x theirs, err = max|g - g64| / max|g64|), the chunking, the refusals, and a
PSNet training step.  The stack shape is test_gpu_dep_context.py's; the scene
and the small feature net are those of test_gpu_context_train.py, rebuilt
here."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SB, SH, SW, Sh, Sw = 2, 38, 142, 10, 36     # the whole-stack image and its feature map
NAMES = ("conv2_wgrad", "conv2_dgrad", "context_conv2", "context_pack", "context_unpack_grad", "dep_context_pack",
         "dep_context_unpack_grad")
DEPTH_OUT_CAP = 4 * 2.627e-03               # test_gpu_dep_context.py's cap on depth_out against the torch route


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
    m = float(g64.abs().max())
    return float((g.detach().double().cpu() - g64).abs().max() / (m if m > 0 else 1.0))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _convs(cin=36, bn=False):
    from sfm_amd.psnet import _context_stack
    torch.manual_seed(13)
    convs = _context_stack(cin, bn)
    for m in convs.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return convs


def _up(feat, H, W):
    return F.interpolate(feat, [H, W], mode="bilinear", align_corners=True)


def _parent_path(dep_convs, depth, feat, image):
    """PSNet.forward's torch route (PSNet.py:218-221): the float32 upsample and cat, the modules, + depth."""
    up = _up(feat.float(), depth.shape[2], depth.shape[3])
    return dep_convs(torch.cat((depth.detach(), up, image.float()), dim=1)) + depth


@functools.lru_cache(maxsize=None)
def _case():
    """(dep_convs, depth, feat, image, upstream gradient, float64 gradients {name: tensor}); the features are
    float32 tensors of float16 values (what cfg.MIXED_PREC's feature CNN gives)."""
    convs = _convs()
    g = torch.Generator().manual_seed(15)
    feat = torch.randn(SB, 32, Sh, Sw, generator=g).half().float()
    depth = 1.0 + 9.0 * torch.rand(SB, 1, SH, SW, generator=g)
    image = torch.rand(SB, 3, SH, SW, generator=g)
    go = torch.randn(SB, 1, SH, SW, generator=g)
    c64 = copy.deepcopy(convs).double()
    feat64 = feat.double().requires_grad_(True)
    depth64 = depth.double().requires_grad_(True)
    (c64(torch.cat((depth64.detach(), _up(feat64, SH, SW), image.double()), 1)) + depth64).backward(go.double())
    g64 = {k: p.grad for k, p in c64.named_parameters()}
    g64["feat"], g64["depth"] = feat64.grad, depth64.grad
    return convs, depth, feat, image, go, g64


def _grads(convs, fn, depth, feat, image, go, cuda, feat_dtype=torch.float32):
    """(output, gradients {name: tensor}, image.grad) of ``fn(convs, depth, feat, image)`` under float16
    autocast on a fresh device copy."""
    convs = copy.deepcopy(convs).to(cuda)
    depth = depth.to(cuda).requires_grad_(True)
    feat = feat.to(cuda, feat_dtype).requires_grad_(True)
    image = image.to(cuda).requires_grad_(True)
    with torch.autocast("cuda", torch.float16):
        out = fn(convs, depth, feat, image)
    out.backward(go.to(cuda))
    g = {k: p.grad for k, p in convs.named_parameters()}
    g["feat"], g["depth"] = feat.grad, depth.grad
    return out.detach(), g, image.grad


def test_forward_bits_and_every_gradient(cuda):
    from sfm_amd.context import dep_context_refine, dep_context_refine_autograd
    convs, depth, feat, image, go, g64 = _case()
    (out, ours, gimage), n = _launches(lambda: _grads(convs, dep_context_refine_autograd, depth, feat, image, go, cuda))
    assert n["conv2_wgrad"] == 7 and n["conv2_dgrad"] == 7 and n["dep_context_unpack_grad"] == 1, n
    assert n["context_conv2"] == 7 and n["dep_context_pack"] == 1, n
    assert n["context_pack"] == 0 and n["context_unpack_grad"] == 0, n
    want = dep_context_refine(copy.deepcopy(convs).to(cuda), depth.to(cuda), feat.to(cuda), image.to(cuda), "fp16")
    assert out.dtype == torch.float32 and out.shape == want.shape and torch.equal(_bits(out), _bits(want))
    assert gimage is None
    assert torch.equal(_bits(ours["depth"]), _bits(go.to(cuda)))
    _, theirs, _ = _grads(convs, _parent_path, depth, feat, image, go, cuda)
    assert set(ours) == set(g64) and len(ours) == 9
    for k in sorted(g64):
        assert ours[k].dtype == theirs[k].dtype == torch.float32 and ours[k].shape == g64[k].shape, k
        rec = {"grad": k, "err_fp16_hip": _err(ours[k], g64[k]), "err_torch_autocast": _err(theirs[k], g64[k])}
        print(rec)
        assert rec["err_fp16_hip"] <= 2.0 * rec["err_torch_autocast"], rec
    assert bool((ours["feat"] != 0).any())
    # the same call again: the same bits
    _, again, _ = _grads(convs, dep_context_refine_autograd, depth, feat, image, go, cuda)
    for k in ours:
        assert torch.equal(_bits(ours[k]), _bits(again[k])), k
    # float16 features: their gradient in float16, the float32 one rounded once
    _, half, _ = _grads(convs, dep_context_refine_autograd, depth, feat, image, go, cuda, torch.float16)
    assert half["feat"].dtype == torch.float16 and torch.equal(_bits(half["feat"]), _bits(ours["feat"].half()))


def test_one_pair_per_chunk(cuda):
    """max_scratch_bytes forcing one pair per chunk: the feat / depth gradient
    bits of one chunk; weight gradients (fp32 sums over the chunks, another
    order) within 2 x the modules' error; twice the launches."""
    from sfm_amd.context import dep_context_refine_autograd, pairs_per_chunk
    convs, depth, feat, image, go, g64 = _case()
    assert pairs_per_chunk(SB, SH, SW, 1) == 1
    out, whole, _ = _grads(convs, dep_context_refine_autograd, depth, feat, image, go, cuda)
    (out1, one, _), n = _launches(lambda: _grads(
        convs, lambda c, d, f, i: dep_context_refine_autograd(c, d, f, i, max_scratch_bytes=1), depth, feat, image, go,
        cuda))
    assert n["conv2_wgrad"] == 7 * SB and n["conv2_dgrad"] == 7 * SB and n["dep_context_unpack_grad"] == SB, n
    assert n["context_conv2"] == 7 * SB and n["dep_context_pack"] == SB, n
    assert torch.equal(_bits(out1), _bits(out))
    for k in ("feat", "depth"):
        assert torch.equal(_bits(one[k]), _bits(whole[k])), k
    _, theirs, _ = _grads(convs, _parent_path, depth, feat, image, go, cuda)
    for k in sorted(g64):
        rec = {"grad": k, "err_fp16_hip_chunked": _err(one[k], g64[k]), "err_torch_autocast": _err(theirs[k], g64[k])}
        print(rec)
        assert rec["err_fp16_hip_chunked"] <= 2.0 * rec["err_torch_autocast"], rec


def test_refusals(cuda):
    from sfm_amd.context import ContextStackError, dep_context_refine_autograd
    _, depth, feat, image, _, _ = _case()
    depth, feat, image = depth.to(cuda), feat.to(cuda), image.to(cuda)
    bn = _convs(bn=True).to(cuda).train()
    with torch.autocast("cuda", torch.float16):
        with pytest.raises(ContextStackError, match="BatchNorm2d in training mode"):
            dep_context_refine_autograd(bn, depth, feat, image)
        with pytest.raises(ContextStackError, match="BatchNorm2d in eval mode"):
            dep_context_refine_autograd(bn.eval(), depth, feat, image)
        with pytest.raises(ContextStackError, match="36 channels"):
            dep_context_refine_autograd(_convs(cin=33).to(cuda), depth, feat, image)
        with pytest.raises(RuntimeError, match="device tensors"):
            dep_context_refine_autograd(_convs().to(cuda), depth, feat.cpu(), image)
        with pytest.raises(ContextStackError, match="float32 on the tensors' device"):
            dep_context_refine_autograd(_convs().to(cuda).half(), depth, feat, image)
        with pytest.raises(ContextStackError, match="float32 on the tensors' device"):
            dep_context_refine_autograd(_convs(), depth, feat, image)
    plain = _convs().to(cuda)
    with pytest.raises(RuntimeError, match="autocast"):
        dep_context_refine_autograd(plain, depth, feat, image)
    with torch.autocast("cuda", torch.bfloat16):
        with pytest.raises(RuntimeError, match="autocast"):
            dep_context_refine_autograd(plain, depth, feat, image)


# --- PSNet(dep_context_grad=...) -------------------------------------------------------
B, L, IH, IW = 2, 4, 32, 48
MIN_DEPTH = 1.0


def _net(cuda, **kw):
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(PSNET_CONTEXT=True, PSNET_DEP_CONTEXT=True, **kw.pop("cfg", {}))
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
    the CPU (PSNet.py:138-225 with one target); the sampling grids are the
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
    x = torch.cat([rf.unsqueeze(0).expand(L, B, C, h, w).reshape(L * B, -1, h, w), planes], 1)
    costss = (net.convs(x) + planes).reshape(L, B, h, w).permute(1, 0, 2, 3)
    depth = _head(costss, IH, IW)
    refined = net.dep_convs(torch.cat((depth.detach(), _up(rf, IH, IW), ref.double()), 1)) + depth
    _loss((depth, refined), gt.double()).backward()
    return net


def test_psnet_training_step(cuda):
    scene = _scene()
    net = _net(cuda, dep_context_grad="fp16").train()
    tor = _net(cuda, dep_context_grad="torch").train()
    n64 = _restated64(net, scene)
    outs, n = _launches(lambda: _step(net, scene, cuda))
    assert outs[0].shape == outs[1].shape == (B, 1, IH, IW) and outs[1].grad_fn is not None
    assert n["conv2_wgrad"] == 7 and n["conv2_dgrad"] == 7 and n["dep_context_unpack_grad"] == 1, n
    assert n["context_conv2"] == 7 and n["dep_context_pack"] == 1, n
    touts, nt = _launches(lambda: _step(tor, scene, cuda))
    assert all(v == 0 for v in nt.values()), nt
    d = float((outs[1].detach() - touts[1].detach()).abs().max() / touts[1].detach().abs().max())
    print(f"PSNet training step depth_out B={B} L={L} {IH}x{IW}: dep_context_grad fp16 vs torch, "
          f"max-abs / max-abs {d:.3e} (cap {DEPTH_OUT_CAP:.3e})")
    assert d <= DEPTH_OUT_CAP, (d, DEPTH_OUT_CAP)
    for k, p in net.dep_convs.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k
    for name in ("dep_convs.0.0.weight", "dep_convs.6.0.weight", "feature_extraction.weight"):
        g64 = dict(n64.named_parameters())[name].grad
        ours = _err(dict(net.named_parameters())[name].grad, g64)
        theirs = _err(dict(tor.named_parameters())[name].grad, g64)
        print({"param": name, "err_dep_context_fp16_hip": ours, "err_dep_context_torch": theirs})
        assert ours <= 2.0 * theirs, (name, ours, theirs)


def test_default_route_is_unchanged(cuda):
    """The default net launches no kernel of the new route and gives the
    output and gradient bits of a model built without the argument.

    The feature net's gradient is the one exception to "bits": on the torch
    route it comes through torch's upsample_bilinear2d backward, which adds
    with float atomics in an order that varies from run to run (16 identical
    steps of one model gave two bit patterns of feature_extraction.weight.grad
    and one of every other parameter's).  The two models run the same code, so
    what can differ is that order alone: a feature cell sums at most 8 x 8 = 64
    = 2^6 destination terms in float32 (unit round-off 2^-24), 2^-18 of their
    magnitude, and two bits are allowed for the cancellation on the way to the
    weights: max|a - b| <= 2^-16 max|a|."""
    scene = _scene()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        res = []
        for kw in ({}, {"dep_context_grad": "torch"}):
            net = _net(cuda, **kw).train()
            assert net.dep_context_grad == "torch"
            outs, n = _launches(lambda: _step(net, scene, cuda))
            assert all(v == 0 for v in n.values()), n
            res.append((outs, {k: p.grad for k, p in net.named_parameters()}))
    finally:
        torch.backends.cudnn.deterministic = det
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(_bits(a), _bits(b))
    assert set(res[0][1]) == set(res[1][1])
    checked = 0
    for k in res[0][1]:
        a, b = res[0][1][k], res[1][1][k]
        assert (a is None) == (b is None), k
        if a is None:
            continue
        checked += 1
        if k.startswith("feature_extraction."):
            d = float((a - b).abs().max() / a.abs().max())
            print(f"default route: {k} max|a - b| / max|a| = {d:.3e} (bound 2^-16 = 1.526e-05)")
            assert d <= 2.0 ** -16, (k, d)
        else:
            assert torch.equal(_bits(a), _bits(b)), k
    assert checked >= 2 + 7 + 7 and res[0][1]["dep_convs.0.0.weight"] is not None


def test_forced_fp16_outside_autocast_and_with_batchnorm_raises(cuda):
    from sfm_amd.context import ContextStackError
    net = _net(cuda, dep_context_grad="fp16").train()
    with pytest.raises(RuntimeError, match="dep_context_grad='fp16'.*autocast"):
        _run(net, _scene(), cuda, autocast=False)
    bn = _net(cuda, dep_context_grad="fp16", cfg={"CONTEXT_BN": True}).train()
    with pytest.raises(ContextStackError, match="BatchNorm2d in training mode"):
        _run(bn, _scene(), cuda)
