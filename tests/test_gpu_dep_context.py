"""The full-resolution refinement stack on libsfm_hip against torch
(csrc/context.hip ``k_dep_pack``, ``sfm_amd.context.dep_context_refine``,
PSNet's ``dep_context_precision``; models/PSNet.py:218-221): the pack kernel
with its fused upsample on an exact lattice and at a general ratio, the whole
stack against a float64 yardstick next to torch's own autocast run, chunking,
the routing rules of ``"auto"`` and the features ``IND_CONTEXT`` feeds it."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
PRECISION = {"f16": "fp16", "bf16": "bf16"}
FEAT_DTYPE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SB, SL = 2, 3
SH, SW, Sh, Sw = 38, 142, 10, 36        # the whole-stack image and its feature map (FeatureExtraction's size)

# Absolute caps on the HIP route's error, max|got - float64| / max|float64|: 4 x the figure measured on the
# first GPU run at this shape (the refinement stack, lists the measured pairs (a) torch autocast,
# (b) HIP route)
# measured (b): 8.173e-04 (f16), 9.679e-04 (f16, CONTEXT_BN), 5.860e-03 (bf16); PSNet depth_out against the
# torch route 2.627e-03 (that run interpolated in fp32; with the float64 upsample (b) is 7.651e-04, 1.110e-03,
# 5.792e-03 and 3.002e-03; the caps stay those of the first run)
STACK_CAPS = {("plain", "f16"): 4 * 8.173e-04, ("bn", "f16"): 4 * 9.679e-04, ("plain", "bf16"): 4 * 5.860e-03}
DEPTH_OUT_CAP = 4 * 2.627e-03


def _up(feat, H, W):
    return F.interpolate(feat, [H, W], mode="bilinear", align_corners=True)


def _pack(cuda, depth, feat, image, dt, b0=0, nb=None):
    """sfm_dep_context_pack_<dt> on device copies of the inputs -> [nb, H, W, 64] on the CPU."""
    from sfm_amd import _lib
    B, _, H, W = depth.shape
    nb = B if nb is None else nb
    d, f, im = depth.to(cuda).contiguous(), feat.to(cuda).contiguous(), image.to(cuda).contiguous()
    out = torch.full((nb, H, W, 64), 7.0, dtype=DTYPES[dt], device=cuda)
    fn = "sfm_dep_context_pack_" + dt
    _lib.check(getattr(_lib.load(), fn)(_lib.ptr(d), _lib.ptr(f), FEAT_DTYPE[f.dtype], _lib.ptr(im), B, b0, nb, 32,
                                        f.shape[2], f.shape[3], H, W, _lib.ptr(out), _lib.stream_ptr(cuda)), fn)
    return out.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


# --- the pack kernel ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice_case(bf16_exact):
    """h, w = 4, 18 -> H, W = 13, 69: both scales are exactly 1/4, so with
    integer features in [-3, 3] every weight is a multiple of 1/4 and every
    interpolated value a multiple of 1/16 below 4 in magnitude: exact in fp32,
    float16 and bfloat16, whatever the order of operations.  W is wider than
    64 and ragged, H a multiple of neither 4 nor 8."""
    B, h, w, H, W = 2, 4, 18, 13, 69
    g = torch.Generator().manual_seed(31)
    feat = torch.randint(-3, 4, (B, 32, h, w), generator=g).float()
    depth = 1.0 + 9.0 * torch.rand(B, 1, H, W, generator=g)
    image = torch.rand(B, 3, H, W, generator=g)
    if bf16_exact:
        depth, image = depth.bfloat16().float(), image.bfloat16().float()
    up = _up(feat, H, W)
    assert torch.equal(up.double(), _up(feat.double(), H, W)) and torch.equal(up * 16, (up * 16).round())
    want = torch.cat((depth, up, image), 1).permute(0, 2, 3, 1)          # torch's construction, channels-last
    return depth, feat, image, want


@pytest.mark.parametrize("dt", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("fdt", [torch.float16, torch.float32, torch.bfloat16], ids=["feat_f16", "feat_f32", "feat_bf16"])
def test_pack_exact_lattice(cuda, fdt, dt):
    depth, feat, image, want = _lattice_case(dt == "bf16")
    dtype = DTYPES[dt]
    got = _pack(cuda, depth, feat.to(fdt), image, dt)
    assert tuple(got.shape) == (2, 13, 69, 64)
    assert torch.equal(_bits(got[..., :36]), _bits(want.to(dtype)))
    assert bool((_bits(got[..., 36:]) == 0).all())
    assert bool((got[..., 1:33] != 0).any()) and bool((got[..., 0] != 0).all())
    # the second pair on its own: b0 = 1, nb = 1
    one = _pack(cuda, depth, feat.to(fdt), image, dt, b0=1, nb=1)
    assert torch.equal(_bits(one), _bits(got[1:2]))


def _f16_steps(a, b):
    """|a - b| in float16 steps: the distance between their places on the ordered line of float16 values."""
    def key(t):
        v = _bits(t).int()
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return (key(a) - key(b)).abs()


@functools.lru_cache(maxsize=None)
def _general_case():
    """6 x 20 -> 22 x 78 (scales 5/21 and 19/77), N(0,1) float16 features;
    the float64 CPU upsample rounded once to float16, channels-last; and how
    far torch's own fp32 CPU upsample is from it, in float16 steps."""
    B, h, w, H, W = 2, 6, 20, 22, 78
    g = torch.Generator().manual_seed(32)
    feat = torch.randn(B, 32, h, w, generator=g).half()
    depth = 1.0 + 9.0 * torch.rand(B, 1, H, W, generator=g)
    image = torch.rand(B, 3, H, W, generator=g)
    want = _up(feat.double(), H, W).permute(0, 2, 3, 1).half()
    t32 = _f16_steps(_up(feat.float(), H, W).permute(0, 2, 3, 1).half(), want)
    return depth, feat, image, want, t32


def test_pack_general_ratio(cuda):
    """Against the float64 upsample rounded once to float16 at most 1 % of
    the feature channels' elements differ (torch's own fp32 CPU upsample
    differs on 0.32 % at this shape and seed: the fp32 rounding of the scale,
    the weights and the products moves a sum across a float16 rounding
    boundary that rarely; the kernel interpolates in float64); depth and
    image are bit-equal."""
    depth, feat, image, want, t32 = _general_case()
    got = _pack(cuda, depth, feat, image, "f16")
    steps = _f16_steps(got[..., 1:33], want)
    frac = float((steps != 0).float().mean())
    print(f"dep pack 6x20 -> 22x78: {100 * frac:.3f} % of the feature elements differ from float64 "
          f"(torch fp32 CPU upsample: {100 * float((t32 != 0).float().mean()):.3f} %)")
    assert frac <= 0.01, frac
    assert torch.equal(_bits(got[..., 0]), _bits(depth[:, 0].half()))
    assert torch.equal(_bits(got[..., 33:36]), _bits(image.permute(0, 2, 3, 1).half()))
    assert bool((_bits(got[..., 36:]) == 0).all())
    # float32 features of the same values: the same bits
    assert torch.equal(_bits(_pack(cuda, depth, feat.float(), image, "f16")), _bits(got))


def test_pack_general_ratio_adjacent_float16(cuda):
    """Every element is the same as or adjacent to the float64 upsample
    rounded once to float16.

    An fp32 evaluation in torch's form does not meet this on N(0,1)
    features: src = scale * dst carries an fp32 rounding error of up to
    2^-24 * src (1e-6 at the right edge), the weights carry it on, and times
    feature differences of magnitude 1 that is more than a float16 step
    (2^-20 and less) wherever the four terms cancel to |value| < 2^-9 or so.
    Torch's own fp32 CPU upsample is up to 10 float16 steps away at this
    shape and seed, on 22 elements (between 4 and 51 steps at each of the
    seeds 0..399), and so was the kernel while it interpolated in fp32 (10
    steps, 23 of 109,824 elements).  The kernel therefore evaluates the same
    expression in float64."""
    depth, feat, image, want, t32 = _general_case()
    got = _pack(cuda, depth, feat, image, "f16")
    steps = _f16_steps(got[..., 1:33], want)
    far = steps > 1
    print(f"dep pack 6x20 -> 22x78: max {int(steps.max())} float16 steps from float64 on {int(far.sum())} of "
          f"{steps.numel()} elements more than one step away, largest |value| among them "
          f"{float(want[far].abs().max()) if bool(far.any()) else 0.0:.3e} "
          f"(torch fp32 CPU upsample: max {int(t32.max())} steps, {int((t32 > 1).sum())} elements)")
    assert int(steps.max()) <= 1, int(steps.max())


# --- the whole stack ------------------------------------------------------------------
def _net(bn):
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(CONTEXT_BN=bn, PSNET_DEP_CONTEXT=True)
    torch.manual_seed(13)
    net = PSNet(SL, 1.0, cfg=c, feature_fn=lambda img: img).eval()
    if bn:
        g = torch.Generator().manual_seed(14)
        for m in net.dep_convs.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.data = 0.75 + 0.5 * torch.rand(n, generator=g)
                m.bias.data = 0.1 * torch.randn(n, generator=g)
                m.running_mean.data = 0.1 * torch.randn(n, generator=g)
                m.running_var.data = 0.5 + torch.rand(n, generator=g)
    return net


def _stack_inputs():
    """N(0,1) features as float16 (what cfg.MIXED_PREC's feature CNN gives), positive depth, image in [0, 1]."""
    g = torch.Generator().manual_seed(15)
    feat = torch.randn(SB, 32, Sh, Sw, generator=g).half()
    depth = 1.0 + 9.0 * torch.rand(SB, 1, SH, SW, generator=g)
    image = torch.rand(SB, 3, SH, SW, generator=g)
    return depth, feat, image


def _parent_path(dep_convs, depth, feat, image):
    """PSNet.forward's nn.Conv2d route, as it stood before the HIP one."""
    up = _up(feat.float(), depth.shape[2], depth.shape[3])
    return dep_convs(torch.cat((depth.detach(), up, image.float()), dim=1)) + depth


@functools.lru_cache(maxsize=None)
def _stack_case(bn):
    """(net, depth, feat, image, float64 yardstick [B, 1, H, W]): dep_convs(cat(depth, up(feat), image)) + depth
    in float64 on the CPU with the float32 weights."""
    net = _net(bn)
    depth, feat, image = _stack_inputs()
    with torch.no_grad():
        x = torch.cat((depth.double(), _up(feat.double(), SH, SW), image.double()), 1)
        ref = copy.deepcopy(net.dep_convs).double()(x) + depth.double()
    return net, depth, feat, image, ref


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("variant,dt", [("plain", "f16"), ("bn", "f16"), ("plain", "bf16")],
                         ids=["f16", "f16_context_bn", "bf16"])
def test_refine_accuracy_against_float64(cuda, variant, dt):
    """(a) torch's own autocast run of dep_convs on the GPU and (b) the HIP
    route, both as max-abs error against the float64 yardstick relative to its
    max-abs: (b) <= 2 (a), the context stack's bar (the same arithmetic), and
    (b) under its cap."""
    from sfm_amd.context import dep_context_refine
    net, depth, feat, image, ref = _stack_case(variant == "bn")
    convs = copy.deepcopy(net.dep_convs).to(cuda)
    depth, feat, image = depth.to(cuda), feat.to(cuda), image.to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=DTYPES[dt]):
        a = _rel(_parent_path(convs, depth, feat, image), ref)
    got = dep_context_refine(convs, depth, feat, image, precision=PRECISION[dt])
    assert tuple(got.shape) == (SB, 1, SH, SW) and got.dtype == torch.float32
    b = _rel(got, ref)
    print(f"refinement stack {variant} {dt} B={SB} {SH}x{SW} (features {Sh}x{Sw}): "
          f"(a) torch autocast {a:.3e}  (b) HIP {b:.3e}")
    assert bool((got != depth).any())
    assert b <= 2 * a, (a, b)
    cap = STACK_CAPS[(variant, dt)]
    assert cap is not None and b <= cap, (b, cap)


def test_refine_bit_equal_across_chunks(cuda):
    from sfm_amd.context import dep_context_refine, pairs_per_chunk
    net, depth, feat, image, _ = _stack_case(False)
    convs = copy.deepcopy(net.dep_convs).to(cuda)
    depth, feat, image = depth.to(cuda), feat.to(cuda), image.to(cuda)
    whole = dep_context_refine(convs, depth, feat, image)
    assert pairs_per_chunk(SB, SH, SW, 1) == 1 and pairs_per_chunk(SB, SH, SW, 1 << 30) == SB
    assert pairs_per_chunk(SB, SH, SW, 2 * SH * SW * 128 * 2) == 1
    assert torch.equal(dep_context_refine(convs, depth, feat, image, max_scratch_bytes=1), whole)   # a pair per chunk
    assert torch.equal(dep_context_refine(convs, depth, feat.float(), image), whole)
    assert torch.equal(dep_context_refine(convs, depth[1:], feat[1:], image[1:]), whole[1:])


# --- PSNet routing ----------------------------------------------------------------------
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
    return out, {k: _lib.profile_read(k)[1] for k in ("context_conv2", "context_pack", "dep_context_pack")}


class _Fixed(nn.Module):
    def __init__(self, fea):
        super().__init__()
        self.fea = fea

    def forward(self, img):
        return self.fea


def _route_net(cuda, dep_context_precision="auto", **cfg):
    """A stock PSNet under cfg.MIXED_PREC with PSNET_CONTEXT and PSNET_DEP_CONTEXT on and fixed float16
    features: (net, run, image, reference features)."""
    from sfm_amd import synth
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(MIXED_PREC=True, PSNET_CONTEXT=True, PSNET_DEP_CONTEXT=True, **cfg)
    feas = [t.half().to(cuda) for t in synth.features(SB, 32, Sh, Sw, seed=3)]
    calls = []

    def feature_fn(img):
        calls.append(1)
        return feas[(len(calls) - 1) % 2]
    torch.manual_seed(9)
    net = PSNet(SL, 1.0, cfg=c, feature_fn=feature_fn, dep_context_precision=dep_context_precision).to(cuda).eval()
    K = synth.intrinsics(SB, 4.0 * Sw, 4.0 * Sw, 2.0 * Sw, 2.0 * Sh).to(cuda)
    pose = synth.relative_pose(SB, torch.Generator().manual_seed(3)).to(cuda)
    img = torch.rand(SB, 3, SH, SW, generator=torch.Generator().manual_seed(4)).to(cuda)

    def run(autocast=True):
        calls.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            return net(img, [img], pose.unsqueeze(1).clone(), K, torch.inverse(K))
    return net, run, img, feas[0]


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _raise(*a, **k):
    raise AssertionError("dep_convs.forward was called on the HIP route")


def test_auto_takes_the_hip_route_under_float16_autocast(cuda):
    net, run, img, fea = _route_net(cuda)
    assert net.dep_context_precision == "auto"
    net.dep_convs.forward = _raise
    (depth, depth_out), n = _launches(run)
    assert n["dep_context_pack"] == 1 and n["context_conv2"] == 14 and n["context_pack"] >= 1, n
    assert depth_out.dtype == torch.float32 and tuple(depth_out.shape) == (SB, 1, SH, SW)
    assert not _bits_equal(depth, depth_out)
    tnet, trun, _, _ = _route_net(cuda, dep_context_precision="torch")
    (tdepth, tout), tn = _launches(trun)
    assert tn["dep_context_pack"] == 0 and tn["context_conv2"] == 7, tn
    assert _bits_equal(tdepth, depth)
    d = float((depth_out - tout).abs().max() / tout.abs().max())
    print(f"PSNet depth_out B={SB} L={SL} {SH}x{SW}: HIP refinement route vs torch autocast, max-abs / max-abs {d:.3e}")
    assert DEPTH_OUT_CAP is not None and d <= DEPTH_OUT_CAP, (d, DEPTH_OUT_CAP)


@pytest.mark.parametrize("how", ["no_autocast", "train", "pre_hook"])
def test_auto_stays_on_torch_elsewhere(cuda, how):
    """Outside autocast, in training mode or with a forward pre-hook on
    net.dep_convs: no pack launch and the bits of dep_context_precision="torch"."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        outs = []
        for dp in ("auto", "torch"):
            net, run, _, _ = _route_net(cuda, dep_context_precision=dp)
            if how == "train":
                net.train()
            if how == "pre_hook":
                net.dep_convs.register_forward_pre_hook(lambda m, i: None)
            out, n = _launches(lambda: run(autocast=how != "no_autocast"))
            assert n["dep_context_pack"] == 0, (dp, n)
            outs.append(out)
    finally:
        torch.backends.cudnn.deterministic = det
    assert _bits_equal(outs[0][0], outs[1][0]) and _bits_equal(outs[0][1], outs[1][1])
    assert not _bits_equal(outs[0][0], outs[0][1])


def test_torch_precision_is_the_parent_path(cuda):
    """dep_context_precision="torch" under float16 autocast: dep_convs is called on the float32
    cat(depth, F.interpolate(features.float()), image) and the result is its output + depth."""
    net, run, img, fea = _route_net(cuda, dep_context_precision="torch")
    rec = {}
    net.dep_convs.register_forward_hook(lambda m, i, o: rec.update(x=i[0].detach().clone(), y=o.detach().clone()))
    (depth, depth_out), n = _launches(run)
    assert n["dep_context_pack"] == 0 and n["context_conv2"] == 7, n
    want = torch.cat((depth, _up(fea.float(), SH, SW), img), 1)
    assert rec["x"].dtype == torch.float32 and torch.equal(rec["x"], want)
    assert rec["y"].dtype == torch.float16 and _bits_equal(depth_out, rec["y"] + depth)


def test_forced_precisions(cuda):
    """"fp16" / "bf16" take the HIP route without autocast; training mode raises."""
    from sfm_amd.context import dep_context_refine
    for dp in ("fp16", "bf16"):
        net, run, img, fea = _route_net(cuda, dep_context_precision=dp)
        (depth, depth_out), n = _launches(lambda: run(autocast=False))
        assert n["dep_context_pack"] == 1 and n["context_conv2"] == 7, n
        assert _bits_equal(depth_out, dep_context_refine(net.dep_convs, depth, fea, img, precision=dp))
        assert not _bits_equal(depth, depth_out)
        net.train()
        with pytest.raises(RuntimeError, match="eval"):
            run(autocast=False)


@pytest.mark.parametrize("dp", ["torch", "auto"])
def test_ind_context_feeds_context_net_features(cuda, dp):
    """IND_CONTEXT: dep_convs upsamples context_net's features (PSNet.py:177-178, 219), not the sweep's, on
    either route of dep_convs -- also where the per-plane stack took its HIP route."""
    from sfm_amd import synth
    from sfm_amd.context import dep_context_refine
    net, run, img, fea = _route_net(cuda, dep_context_precision=dp, IND_CONTEXT=True)
    own = synth.features(SB, 32, Sh, Sw, seed=21)[0].half().to(cuda)
    net.context_net = _Fixed(own)
    if dp == "torch":
        rec = {}
        net.dep_convs.register_forward_pre_hook(lambda m, i: rec.__setitem__("x", i[0].detach().clone()))
        (depth, depth_out), n = _launches(run)
        assert n["context_conv2"] == 7 and n["context_pack"] >= 1 and n["dep_context_pack"] == 0, n
        assert rec["x"].shape[1] == 36
        assert torch.equal(rec["x"][:, 1:33], _up(own.float(), SH, SW))
        assert not torch.equal(rec["x"][:, 1:33], _up(fea.float(), SH, SW))
        return
    (depth, depth_out), n = _launches(run)
    assert n["context_conv2"] == 14 and n["dep_context_pack"] == 1, n
    assert _bits_equal(depth_out, dep_context_refine(net.dep_convs, depth, own, img))
    assert not _bits_equal(depth_out, dep_context_refine(net.dep_convs, depth, fea, img))
