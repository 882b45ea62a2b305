"""The feature CNN on libsfm_hip against torch (csrc/feature.hip,
sfm_amd/feature.py, PSNet's ``feature_precision``): every kernel form of
sfm_conv2x_f16 on exact integers, the pack, pool and SPP kernels bit for bit,
the whole CNN against a float64 yardstick next to torch's own autocast run,
chunking and batching, and the routing rules of ``"auto"``."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import feature_cases as FC

pytestmark = pytest.mark.gpu

# Absolute cap on the HIP route's error, max|got - float64| / max|float64|, at the recipe of tests/feature_cases.py:
# 4 x the figure measured on the first GPU run (the feature CNN, lists the measured pair
# (a) torch autocast, (b) HIP route)
# measured: (a) 2.829e-03, (b) 1.177e-03
CNN_CAP = 4 * 1.177e-03

# (cin, cout, ksize, stride, dilation, (images, h, w), residual)
CASES = {
    "3x3s2_32to64": (32, 64, 3, 2, 1, (2, 9, 70), False),
    "3x3s2_32to32": (32, 32, 3, 2, 1, (1, 10, 131), False),
    "1x1s2_32to64": (32, 64, 1, 2, 1, (2, 9, 70), False),
    "1x1s1_64to128": (64, 128, 1, 1, 1, (3, 5, 67), False),
    "1x1s1_128to32": (128, 32, 1, 1, 1, (3, 5, 67), False),
    "3x3s1_320to128": (320, 128, 3, 1, 1, (1, 5, 67), False),
    "3x3s1d2_128to128_residual": (128, 128, 3, 1, 2, (2, 19, 70), True),
    "3x3s1d16_all_padding": (64, 64, 3, 1, 16, (2, 2, 3), False),
}


@functools.lru_cache(maxsize=None)
def _integer_case(name):
    """Activations in {0, 1}, weights in {-1, 0, 1}, a residual in -3..3, and
    the float64 CPU convolution (+ residual), before any ReLU."""
    cin, cout, k, stride, dil, (n, h, w), res = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randint(0, 2, (n, h, w, cin), generator=g).float()
    wt = torch.randint(-1, 2, (k * k, cout, cin), generator=g).float()
    w4 = wt.reshape(k, k, cout, cin).permute(2, 3, 0, 1).double()
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w4, stride=stride, dilation=dil, padding=dil if k == 3 else 0)
    r = None
    if res:
        r = torch.randint(-3, 4, (n, want.shape[2], want.shape[3], cout), generator=g).float()
    return x, wt, r, want


def _bits(t):
    return t.contiguous().view(torch.int16)


def _f16_steps(a, b):
    """|a - b| in float16 steps: the distance between their places on the ordered line of float16 values."""
    def key(t):
        v = _bits(t).int()
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("name", list(CASES))
def test_layer_exact_integers(cuda, name):
    """Every partial sum is an integer of magnitude <= 9 * 320 = 2880: exact
    in fp32, so the output is the float64 convolution (ReLU, or + residual)
    rounded once to float16: bit-equal, no tolerance."""
    from sfm_amd.feature import conv2x_f16
    cin, cout, k, stride, dil, (n, h, w), res = CASES[name]
    x, wt, r, want = _integer_case(name)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    assert tuple(want.shape) == (n, cout, ho, wo) and float(want.abs().max()) <= 2880
    one, zero = torch.ones(cout), torch.zeros(cout)
    if res:
        want = want + r.permute(0, 3, 1, 2).double()
        assert float(want.min()) < 0
    else:
        want = F.relu(want)
        assert float(want.max()) > 0
    got = conv2x_f16(x.half().to(cuda), wt.half().to(cuda), one, zero, k, stride, dil, relu=not res,
                     residual=None if r is None else r.half().to(cuda))
    assert got.dtype == torch.float16 and tuple(got.shape) == (n, ho, wo, cout)
    assert torch.equal(_bits(got.cpu().permute(0, 3, 1, 2)), _bits(want.to(torch.float16)))
    if name == "3x3s1d16_all_padding":           # only the centre tap sees the image
        centre = F.relu(torch.einsum("nhwc,oc->nohw", x.double(), wt[4].double()))
        assert torch.equal(got.cpu().permute(0, 3, 1, 2).double(), centre)


@pytest.mark.parametrize("dil", [1, 16])
def test_conv2x_is_conv2_at_3x3_stride1(cuda, dil):
    """ksize 3, stride 1, no residual: sfm_conv2_f16's bits, on N(0, 1) data
    where any other order of the fp32 sum would show."""
    from sfm_amd.context import conv2_f16
    from sfm_amd.feature import conv2x_f16
    g = torch.Generator().manual_seed(40 + dil)
    x = torch.randn(3, 19, 70, 64, generator=g).half().to(cuda)
    wt = (0.05 * torch.randn(9, 128, 64, generator=g)).half().to(cuda)
    scale, bias = 0.5 + torch.rand(128, generator=g), torch.randn(128, generator=g)
    for relu in (True, False):
        a = conv2_f16(x, wt, scale, bias, dil, relu=relu)
        b = conv2x_f16(x, wt, scale, bias, 3, 1, dil, relu=relu)
        assert torch.equal(_bits(a), _bits(b)) and bool((a != 0).any())


@pytest.mark.parametrize("name", ["3x3s2_32to64", "1x1s1_64to128", "3x3s1d2_128to128_residual"])
def test_layer_scale_bias_no_relu(cuda, name):
    """Per-channel powers of two as scale and small dyadic biases, ReLU off:
    acc * scale + bias (+ residual) is exact in fp32, so the output is the
    float64 value rounded once."""
    from sfm_amd.feature import conv2x_f16
    cin, cout, k, stride, dil, _, res = CASES[name]
    x, wt, r, want = _integer_case(name)
    scale = torch.tensor([0.5, 1.0, 2.0, 4.0]).repeat(cout // 4)
    bias = torch.tensor([-1.0, 0.0, 0.5, 3.0, 0.25, -2.0, 1.0, -0.5]).repeat(cout // 8)
    want = want * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
    if res:
        want = want + r.permute(0, 3, 1, 2).double()
    assert float(want.min()) < 0
    got = conv2x_f16(x.half().to(cuda), wt.half().to(cuda), scale, bias, k, stride, dil, relu=False,
                     residual=None if r is None else r.half().to(cuda))
    assert torch.equal(_bits(got.cpu().permute(0, 3, 1, 2)), _bits(want.float().to(torch.float16)))


def test_image_pack_bit_equal(cuda):
    from sfm_amd.feature import image_pack_f16
    img = torch.randn(2, 3, 9, 71, generator=torch.Generator().manual_seed(5))
    got = image_pack_f16(img.to(cuda)).cpu()
    assert tuple(got.shape) == (2, 9, 71, 32)
    assert torch.equal(_bits(got[..., :3]), _bits(img.permute(0, 2, 3, 1).half()))
    assert bool((_bits(got[..., 3:]) == 0).all()) and bool((got[..., :3] != 0).any())


@pytest.mark.parametrize("p", [4, 8, 16, 32])
def test_avgpool(cuda, p):
    """At 33 x 38 (both divisions floor).  Integers in -3..3: every sum is
    an integer below 3 * 1024 and the mean a multiple of 2^-10, exact in fp32
    and in float16 steps of the result: bit-equal.  N(0, 1): the fp32 sum of
    p^2 float16 values is within 2^-24 p^2 |sum of magnitudes| of the exact
    one, far inside a float16 step of the mean, so the rounded mean is the
    float64 mean rounded once or its neighbour."""
    from sfm_amd.feature import avgpool_f16
    g = torch.Generator().manual_seed(60 + p)
    h, w = FC.MAP
    xi = torch.randint(-3, 4, (2, h, w, 128), generator=g).float()
    xn = torch.randn(2, h, w, 128, generator=g).half()
    for x, exact in ((xi.half(), True), (xn, False)):
        want = F.avg_pool2d(x.permute(0, 3, 1, 2).double(), p, p).permute(0, 2, 3, 1).to(torch.float16)
        got = avgpool_f16(x.to(cuda), p).cpu()
        assert tuple(got.shape) == (2, h // p, w // p, 128) == tuple(want.shape)
        steps = _f16_steps(got, want)
        assert int(steps.max()) <= (0 if exact else 1), int(steps.max())
        assert bool((got != 0).any())
    got8 = avgpool_f16(xi[..., :8].contiguous().half().to(cuda), p).cpu()      # another channel count: C = 8
    want8 = F.avg_pool2d(xi[..., :8].permute(0, 3, 1, 2).double(), p, p).permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(_bits(got8), _bits(want8))


def test_spp_pack_bit_equal(cuda):
    """Every 32-channel slice against the float64 upsample of
    tests/feature_cases.py (torch's order of terms, written out) rounded once
    as torch rounds a float64 tensor; raw and skip copied; torch's own float64
    F.interpolate within one float16 step of it."""
    from sfm_amd.feature import spp_pack_f16
    g = torch.Generator().manual_seed(70)
    n, (h, w) = 2, FC.MAP
    raw = torch.randn(n, h, w, 64, generator=g).half()
    skip = torch.randn(n, h, w, 128, generator=g).half()
    sizes = [(h // p, w // p) for p in (4, 8, 16, 32)]                  # cat order: branch4 .. branch1
    assert sizes == [(8, 9), (4, 4), (2, 2), (1, 1)]
    maps = [torch.randn(n, a, b, 32, generator=g).half() for a, b in sizes]
    out = spp_pack_f16(raw.to(cuda), skip.to(cuda), [m.to(cuda) for m in maps]).cpu()
    assert tuple(out.shape) == (n, h, w, 320)
    assert torch.equal(_bits(out[..., :64]), _bits(raw)) and torch.equal(_bits(out[..., 64:192]), _bits(skip))
    for i, m in enumerate(maps):
        got = out[..., 192 + 32 * i:224 + 32 * i]
        want = FC.up64(m, h, w).to(torch.float16)
        assert torch.equal(_bits(got), _bits(want)), i
        t64 = F.interpolate(m.permute(0, 3, 1, 2).double(), (h, w), mode="bilinear", align_corners=True)
        assert int(_f16_steps(got, t64.permute(0, 2, 3, 1).to(torch.float16)).max()) <= 1, i
    assert torch.equal(out[..., 288:], maps[3].expand(n, h, w, 32))           # the 1 x 1 source: scale 0, a constant


# --- the whole CNN ------------------------------------------------------------------
def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def test_cnn_accuracy_against_float64(cuda):
    """(a) torch's own float16-autocast run of the module on the GPU and (b)
    feature_extract, both as max-abs error against the float64 CPU forward
    relative to its max-abs: (b) <= 2 (a), the project's rule for the other
    two stacks, and (b) under its cap."""
    from sfm_amd.feature import feature_extract
    net, image, ref = FC.recipe_case()
    net = copy.deepcopy(net).to(cuda)
    img = image.to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        y = net(img)
        assert y.dtype == torch.float16
    a = _rel(y, ref)
    got = feature_extract(net, img)
    assert got.dtype == torch.float16 and got.is_contiguous() and tuple(got.shape) == tuple(ref.shape)
    b = _rel(got, ref)
    print(f"feature CNN {tuple(image.shape)} -> {tuple(ref.shape)}: (a) torch autocast {a:.3e}  (b) HIP {b:.3e}")
    assert b <= 2 * a, (a, b)
    assert CNN_CAP is not None and b <= CNN_CAP, (b, CNN_CAP)


def test_extract_bit_equal_across_chunks_and_batches(cuda):
    from sfm_amd.feature import feature_extract, images_per_chunk
    net, image, _ = FC.recipe_case()
    net = copy.deepcopy(net).to(cuda)
    img = image.to(cuda)
    H, W = image.shape[2:]
    assert images_per_chunk(2, H, W, 1) == 1 and images_per_chunk(2, H, W, 1 << 30) == 2
    whole = feature_extract(net, img)
    assert torch.equal(_bits(feature_extract(net, img, max_scratch_bytes=1)), _bits(whole))     # one image per chunk
    # reference and target as one batch against two separate calls
    sep = torch.cat([feature_extract(net, img[:1]), feature_extract(net, img[1:])])
    assert torch.equal(_bits(sep), _bits(whole)) and not torch.equal(whole[0], whole[1])
    with pytest.raises(RuntimeError, match="under 32 x 32"):
        feature_extract(net, img[:, :, :100, :100])


# --- PSNet routing ------------------------------------------------------------------
L = 4


def _psnet(cuda, feature_precision="auto", feature_fn=None, **cfg):
    from sfm_amd.config import kitti
    from sfm_amd.psnet import PSNet
    c = kitti()
    c.update(**cfg)
    torch.manual_seed(9)
    net = PSNet(L, 1.0, cfg=c, feature_fn=feature_fn, feature_precision=feature_precision)
    for name in ("feature_extraction", "context_net"):
        if isinstance(getattr(net, name, None), torch.nn.Module):
            getattr(net, name).load_state_dict(FC.recipe_case()[0].state_dict())
    return net.to(cuda).eval()


def _spy(monkeypatch):
    import sfm_amd.feature as FT
    calls = []
    real = FT.feature_extract

    def spy(module, image, **kw):
        out = real(module, image, **kw)
        calls.append((module, image, out))
        return out
    monkeypatch.setattr(FT, "feature_extract", spy)
    return calls


def _forward(net, img, autocast=torch.float16):
    from sfm_amd import synth
    B, _, H, W = img.shape
    K = synth.intrinsics(B, 1.0 * W, 1.0 * W, 0.5 * W, 0.5 * H).to(img.device)
    pose = synth.relative_pose(B, torch.Generator().manual_seed(3)).to(img.device)
    with torch.no_grad(), torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        return net(img[:1], [img[1:]], pose[:1].unsqueeze(1).clone(), K[:1], torch.inverse(K[:1]))


def test_auto_takes_the_hip_route_and_feeds_the_sweep(cuda, monkeypatch):
    """End to end under kitti()'s flags in eval mode: the reference and the
    target go through feature_extract as one batch, the fused sweep receives
    exactly those float16 maps, both depths are finite."""
    import sfm_amd.psnet as P
    from sfm_amd.feature import feature_extract
    net = _psnet(cuda)
    img = FC.recipe_case()[1].to(cuda)
    with torch.autocast("cuda", dtype=torch.float16):
        assert net.feature_route(cuda, img.shape[2:]) == ("fp16" if P.FEATURE_AUTO_HIP else "torch")
    assert net.feature_route(cuda, img.shape[2:]) == "torch"           # no autocast at this call
    if not P.FEATURE_AUTO_HIP:
        net.feature_precision = "fp16"
    calls = _spy(monkeypatch)
    seen = []
    real = P.sweep_regularize_fused

    def sweep_spy(self, r, t, *a, **kw):
        seen.append((r, t))
        return real(self, r, t, *a, **kw)
    monkeypatch.setattr(P, "sweep_regularize_fused", sweep_spy)
    depth, depth_out = _forward(net, img)
    assert len(calls) == 1 and calls[0][0] is net.feature_extraction and calls[0][1].shape[0] == 2
    direct = feature_extract(net.feature_extraction, img)
    assert len(seen) == 1 and seen[0][0].dtype == torch.float16
    assert torch.equal(_bits(seen[0][0]), _bits(direct[:1])) and torch.equal(_bits(seen[0][1]), _bits(direct[1:]))
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(depth_out).all())
    assert tuple(depth.shape) == (1, 1) + tuple(img.shape[2:])


@pytest.mark.parametrize("how", ["no_autocast", "bf16_autocast", "train", "hook", "feature_fn", "small_image"])
def test_auto_stays_on_torch_elsewhere(cuda, monkeypatch, how):
    """No feature_extract call, and the features are the module's own, bit for bit
    (the injected feature_fn's; at 100 x 100 the route alone is checked)."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        fn = (lambda im: F.avg_pool2d(im, 4).repeat(1, 11, 1, 1)[:, :32].half()) if how == "feature_fn" else None
        net = _psnet(cuda, feature_fn=fn)
        img = FC.recipe_case()[1].to(cuda)
        if how == "small_image":
            img = img[:, :, :100, :100].contiguous()
        if how == "hook":
            net.feature_extraction.register_forward_hook(lambda m, i, o: None)
        calls = _spy(monkeypatch)
        autocast = None if how == "no_autocast" else torch.bfloat16 if how == "bf16_autocast" else torch.float16
        with torch.no_grad(), torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
            if how == "train":
                net.train()         # batch statistics: the output does not depend on the running ones
            assert net.feature_route(cuda, img.shape[2:]) == "torch"
            if how == "small_image":
                return              # a 25 x 25 map: the module's own AvgPool2d(32) has no window either
            # training mode: both images as one batch (BatchNorm2d needs two values per channel on branch1's 1 x 1 map)
            images = [img] if how == "train" else [img[:1], img[1:]]
            got = net._features("feature_extraction", images)
            want = [net.feature_extraction(im) for im in images]
        assert calls == []
        for g_, w_ in zip(got, want):
            assert g_.dtype == w_.dtype and torch.equal(g_, w_)
    finally:
        torch.backends.cudnn.deterministic = det


def test_forced_precision(cuda, monkeypatch):
    """"fp16" takes the HIP route without autocast; training mode raises; a
    module that is not the stock graph gets the named error."""
    from sfm_amd.feature import FeatureLayoutError
    net = _psnet(cuda, feature_precision="fp16")
    img = FC.recipe_case()[1].to(cuda)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        got = net._features("feature_extraction", [img[:1]])
    assert len(calls) == 1 and got[0].dtype == torch.float16 and tuple(got[0].shape) == (1, 32) + FC.MAP
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        net._features("feature_extraction", [img[:1]])
    odd = _psnet(cuda, feature_precision="fp16", feature_fn=lambda im: im)
    with pytest.raises(FeatureLayoutError, match="FeatureExtraction"):
        odd._features("feature_extraction", [img[:1]])


def test_ind_context_runs_context_net_on_the_hip_route(cuda, monkeypatch):
    """IND_CONTEXT: context_net goes through feature_extract too, and its
    features are what convs and dep_convs read (PSNet.py:177-178, 219)."""
    import sfm_amd.psnet as P
    net = _psnet(cuda, IND_CONTEXT=True)
    if not P.FEATURE_AUTO_HIP:
        net.feature_precision = "fp16"
    with torch.no_grad():                       # context_net differs from feature_extraction
        net.context_net.lastconv[2].weight.mul_(0.5)
    img = FC.recipe_case()[1].to(cuda)
    calls = _spy(monkeypatch)
    seen = {}
    for name in ("context_refine", "dep_context_refine"):
        real = getattr(P, name)

        def spy(*a, _real=real, _name=name, **kw):
            seen[_name] = a
            return _real(*a, **kw)
        monkeypatch.setattr(P, name, spy)
    depth, depth_out = _forward(net, img)
    assert [c[0] for c in calls] == [net.feature_extraction, net.context_net]
    ctx = calls[1][2]
    assert calls[1][1].shape[0] == 1 and not torch.equal(ctx, calls[0][2][:1])
    for got in (seen["context_refine"][1], seen["dep_context_refine"][2]):
        assert got.data_ptr() == ctx.data_ptr() and torch.equal(got, ctx)
    assert bool(torch.isfinite(depth_out).all())
