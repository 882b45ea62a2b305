"""The context stack on libsfm_hip against torch (csrc/context.hip,
sfm_amd/context.py, PSNet's ``context_precision``): every layer of the plan on
exact integers, the pack kernel, the whole stack against a float64 yardstick
next to torch's own autocast run, and the routing rules of ``"auto"``."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (cin_pad, cout, dilation) of the seven stages (models/PSNet.py:64-71; the first one's 33 inputs padded to 64)
PLAN = ((64, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 1, 1))
PLAN_IDS = ["%dto%d_d%d" % p for p in PLAN]
# (images, h, w): ragged in both tile directions, wider than a column tile and taller than dilation 16;
# smaller than dilations 8 and 16 (every off-centre tap is padding); one column and one row past a tile edge
SHAPES = ((3, 19, 70), (2, 5, 7), (1, 33, 65))
SHAPE_IDS = ["3x19x70", "2x5x7", "1x33x65"]
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
PRECISION = {"f16": "fp16", "bf16": "bf16"}
SB, SL, SH, SW = 2, 3, 19, 70           # the whole-stack shape

# Absolute caps on the HIP route's error, max|got - float64| / max|float64|: 4 x the figure measured on the
# first GPU run at this shape (the context stack, lists the measured pairs (a) torch autocast, (b) HIP route)
# measured (b): 2.615e-03 (f16), 1.689e-03 (f16, CONTEXT_BN), 1.882e-02 (bf16); depth through the head 4.836e-04
STACK_CAPS = {("plain", "f16"): 4 * 2.615e-03, ("bn", "f16"): 4 * 1.689e-03, ("plain", "bf16"): 4 * 1.882e-02}
DEPTH_CAP = 4 * 4.836e-04


def _conv2(dt):
    from sfm_amd import context
    return context.conv2_f16 if dt == "f16" else context.conv2_bf16


@functools.lru_cache(maxsize=None)
def _integer_case(li, si):
    """Activations in {0, 1}, weights in {-1, 0, 1} (rows beyond cout zero),
    and the float64 CPU convolution, before the ReLU."""
    cin, cout, dil = PLAN[li]
    n, h, w = SHAPES[si]
    g = torch.Generator().manual_seed(100 * li + si)
    x = torch.randint(0, 2, (n, h, w, cin), generator=g).float()
    cout_pad = (cout + 31) // 32 * 32
    wt = torch.zeros(9, cout_pad, cin)
    wt[:, :cout] = torch.randint(-1, 2, (9, cout, cin), generator=g).float()
    w4 = wt[:, :cout].reshape(3, 3, cout, cin).permute(2, 3, 0, 1).double()          # [cout, cin, kh, kw]
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w4, dilation=dil, padding=dil)    # [n, cout, h, w]
    return x, wt, want


@pytest.mark.parametrize("dt", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=SHAPE_IDS)
@pytest.mark.parametrize("li", range(len(PLAN)), ids=PLAN_IDS)
def test_layer_exact_integers(cuda, li, si, dt):
    """Every partial sum is an integer of magnitude <= 9 * 128 = 1152 < 2048:
    exact in fp32 and in float16.  bfloat16 holds integers exactly up to 256
    only, so the expected output is the float64 result rounded once to the
    output type (the identity for float16): bit-equal, no tolerance."""
    cin, cout, dil = PLAN[li]
    x, wt, want = _integer_case(li, si)
    dtype = DTYPES[dt]
    cout_pad = wt.shape[1]
    one, zero = torch.ones(cout_pad), torch.zeros(cout_pad)
    want = F.relu(want)
    assert float(want.max()) > 0 and float(want.abs().max()) <= 1152
    xd, wd = x.to(cuda, dtype), wt.to(cuda, dtype)
    if cout != 1:
        got = _conv2(dt)(xd, wd, one, zero, dil, relu=True, cout=cout)
        assert got.dtype == dtype and tuple(got.shape) == x.shape[:3] + (cout,)
        assert torch.equal(got.cpu().permute(0, 3, 1, 2), want.to(dtype))
        return
    # cout == 1: fp32 output, with and without the fp32 residual
    got = _conv2(dt)(xd, wd, one, zero, dil, relu=True, cout=1)
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape[:3]
    rounded = want[:, 0].to(dtype).float()
    assert torch.equal(got.cpu(), rounded)
    res = torch.randn(x.shape[:3], generator=torch.Generator().manual_seed(si))
    got = _conv2(dt)(xd, wd, one, zero, dil, relu=True, cout=1, residual=res.to(cuda))
    assert torch.equal(got.cpu(), rounded + res)


@pytest.mark.parametrize("dt", list(DTYPES), ids=list(DTYPES))
def test_layer_scale_bias_no_relu(cuda, dt):
    """Per-channel powers of two as scale and small dyadic biases, ReLU off:
    acc * scale + bias is exact in fp32, so the output is the float64 value
    rounded once to the output type."""
    li, si = 5, 0                                   # 64 -> 32, |sum| <= 576
    cin, cout, dil = PLAN[li]
    x, wt, want = _integer_case(li, si)
    dtype = DTYPES[dt]
    scale = torch.tensor([0.5, 1.0, 2.0, 4.0]).repeat(cout // 4)
    bias = torch.tensor([-1.0, 0.0, 0.5, 3.0, 0.25, -2.0, 1.0, -0.5]).repeat(cout // 8)
    want = want * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
    assert float(want.min()) < 0
    got = _conv2(dt)(x.to(cuda, dtype), wt.to(cuda, dtype), scale, bias, dil, relu=False, cout=cout)
    assert torch.equal(got.cpu().permute(0, 3, 1, 2), want.float().to(dtype))


@pytest.mark.parametrize("dt", list(DTYPES), ids=list(DTYPES))
def test_pack_bit_equal(cuda, dt):
    from sfm_amd import _lib
    B, L, l0, nl, h, w = 2, 3, 1, 2, 19, 70
    g = torch.Generator().manual_seed(4)
    ctx = torch.randn(B, 32, h, w, generator=g).to(cuda)
    planes = torch.randn(B, L, h, w, generator=g).to(cuda)
    dtype = DTYPES[dt]
    out = torch.full((B, nl, h, w, 64), 7.0, dtype=dtype, device=cuda)
    fn = "sfm_context_pack_" + dt
    _lib.check(getattr(_lib.load(), fn)(_lib.ptr(ctx), _lib.ptr(planes), B, L, l0, nl, 32, h, w, _lib.ptr(out),
                                        _lib.stream_ptr(cuda)), fn)
    want = torch.zeros(B, nl, h, w, 64, device=cuda)
    want[..., :32] = ctx.permute(0, 2, 3, 1).unsqueeze(1)
    want[..., 32] = planes[:, l0:l0 + nl]
    assert torch.equal(out.view(torch.int16), want.to(dtype).view(torch.int16))
    assert bool((out[..., 33:] == 0).all()) and bool((out[..., 32] != 0).any())


# --- the whole stack ------------------------------------------------------------
def _net(bn, **cfg):
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(CONTEXT_BN=bn, **cfg)
    torch.manual_seed(11)
    net = PSNet(SL, 1.0, cfg=c, feature_fn=lambda img: img).eval()
    if bn:
        g = torch.Generator().manual_seed(12)
        for m in net.convs.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.data = 0.75 + 0.5 * torch.rand(n, generator=g)
                m.bias.data = 0.1 * torch.randn(n, generator=g)
                m.running_mean.data = 0.1 * torch.randn(n, generator=g)
                m.running_var.data = 0.5 + torch.rand(n, generator=g)
    return net


def _stack_inputs():
    from sfm_amd import synth
    ctx = synth.features(SB, 32, SH, SW, seed=6)[0]
    planes = torch.randn(SB, 1, SL, SH, SW, generator=torch.Generator().manual_seed(7))
    return ctx, planes


def _torch_x(ctx, costs):
    """PSNet.forward's own construction of the stack's input: (x, planes), L-major images."""
    B, _, L, h, w = costs.shape
    planes = costs[:, 0].permute(1, 0, 2, 3).reshape(L * B, 1, h, w)
    x = torch.cat([ctx.unsqueeze(0).expand(L, B, ctx.shape[1], h, w).reshape(L * B, -1, h, w), planes], 1)
    return x, planes


def _from_lmajor(y, B, L, h, w):
    return y.reshape(L, B, h, w).permute(1, 0, 2, 3).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def _stack_case(bn):
    """(net, ctx, costs, float64 yardstick [B, 1, L, h, w]): convs(cat(ctx, plane)) + plane in float64 on the
    CPU with the float32 weights."""
    net = _net(bn)
    ctx, costs = _stack_inputs()
    with torch.no_grad():
        x, planes = _torch_x(ctx.double(), costs.double())
        ref = _from_lmajor(copy.deepcopy(net.convs).double()(x) + planes, SB, SL, SH, SW)
    return net, ctx, costs, ref


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def test_refine_bit_equal_across_chunks_and_to_composed_layers(cuda):
    from sfm_amd import _lib
    from sfm_amd.context import context_refine, conv2_f16, pack_context_stack, planes_per_chunk
    net, ctx, costs, _ = _stack_case(False)
    convs = copy.deepcopy(net.convs).to(cuda)
    ctx, costs = ctx.to(cuda), costs.to(cuda)
    whole = context_refine(convs, ctx, costs)
    assert tuple(whole.shape) == (SB, 1, SL, SH, SW) and whole.dtype == torch.float32
    assert planes_per_chunk(SB, SH, SW, SL, 1) == 1 and planes_per_chunk(SB, SH, SW, SL, 1 << 30) == SL
    assert torch.equal(context_refine(convs, ctx, costs, max_scratch_bytes=1), whole)       # one plane per chunk
    assert torch.equal(context_refine(convs, ctx.half(), costs), context_refine(convs, ctx.half().float(), costs))
    # seven conv2_f16 calls composed by hand on torch's construction of the first input
    x = torch.zeros(SB, SL, SH, SW, 64, device=cuda)
    x[..., :32] = ctx.permute(0, 2, 3, 1).unsqueeze(1)
    x[..., 32] = costs[:, 0]
    y = x.half().view(SB * SL, SH, SW, 64)
    packed = pack_context_stack(convs, cuda, "fp16")
    for lay in packed[:-1]:
        y = conv2_f16(y, lay["w"], lay["scale"], lay["bias"], lay["dilation"], relu=lay["relu"], cout=lay["cout"])
    lay = packed[-1]
    y = conv2_f16(y, lay["w"], lay["scale"], lay["bias"], lay["dilation"], relu=lay["relu"], cout=1,
                  residual=costs[:, 0].contiguous())
    assert torch.equal(y.view(SB, 1, SL, SH, SW), whole)
    assert bool((whole != costs).any())


@pytest.mark.parametrize("variant,dt", [("plain", "f16"), ("bn", "f16"), ("plain", "bf16")],
                         ids=["f16", "f16_context_bn", "bf16"])
def test_refine_accuracy_against_float64(cuda, variant, dt):
    """(a) torch's own autocast run of net.convs on the GPU and (b) the HIP
    route, both as max-abs error against the float64 yardstick relative to its
    max-abs: (b) <= 2 (a) -- another fp32 summation order flips 16-bit
    roundings that pass through six further layers -- and (b) under its cap."""
    from sfm_amd.context import context_refine
    net, ctx, costs, ref = _stack_case(variant == "bn")
    convs = copy.deepcopy(net.convs).to(cuda)
    ctx, costs = ctx.to(cuda), costs.to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=DTYPES[dt]):
        x, planes = _torch_x(ctx, costs)
        y = convs(x)
        assert y.dtype == DTYPES[dt]
        a = _rel(_from_lmajor(y + planes, SB, SL, SH, SW), ref)
    b = _rel(context_refine(convs, ctx, costs, precision=PRECISION[dt]), ref)
    print(f"context stack {variant} {dt} B={SB} L={SL} {SH}x{SW}: (a) torch autocast {a:.3e}  (b) HIP {b:.3e}")
    assert b <= 2 * a, (a, b)
    cap = STACK_CAPS[(variant, dt)]
    assert cap is not None and b <= cap, (b, cap)


# --- PSNet routing ----------------------------------------------------------------
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
    return out, {k: _lib.profile_read(k)[1] for k in ("context_conv2", "context_pack")}


class _Fixed(nn.Module):
    def __init__(self, fea):
        super().__init__()
        self.fea = fea

    def forward(self, img):
        return self.fea


def _route_net(cuda, context_precision="auto", **cfg):
    """A stock PSNet under cfg.MIXED_PREC with PSNET_CONTEXT on and fixed float16 features."""
    from sfm_amd import synth
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(MIXED_PREC=True, PSNET_CONTEXT=True, **cfg)
    feas = [t.half().to(cuda) for t in synth.features(SB, 32, SH, SW, seed=3)]
    calls = []

    def feature_fn(img):
        calls.append(1)
        return feas[(len(calls) - 1) % 2]
    torch.manual_seed(9)
    net = PSNet(SL, 1.0, cfg=c, feature_fn=feature_fn, context_precision=context_precision).to(cuda).eval()
    K = synth.intrinsics(SB, 4.0 * SW, 4.0 * SW, 2.0 * SW, 2.0 * SH).to(cuda)
    pose = synth.relative_pose(SB, torch.Generator().manual_seed(3)).to(cuda)
    img = torch.zeros(SB, 3, 4 * SH, 4 * SW, device=cuda)

    def run(autocast=True):
        calls.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            return net(img, [img], pose.unsqueeze(1).clone(), K, torch.inverse(K))
    return net, run


def _bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_auto_takes_the_hip_route_under_float16_autocast(cuda):
    net, run = _route_net(cuda)
    (depth_init, depth), n = _launches(run)
    assert n["context_conv2"] >= 7 and n["context_pack"] >= 1, n
    assert depth.dtype == torch.float32 and not _bits_equal(depth_init, depth)
    tnet, trun = _route_net(cuda, context_precision="torch")
    (tinit, tdepth), tn = _launches(trun)
    assert tn == {"context_conv2": 0, "context_pack": 0}
    assert _bits_equal(tinit, depth_init)
    d = float((depth - tdepth).abs().max() / tdepth.abs().max())
    print(f"PSNet depth B={SB} L={SL} {4 * SH}x{4 * SW}: HIP context route vs torch autocast, max-abs / max-abs {d:.3e}")
    assert DEPTH_CAP is not None and d <= DEPTH_CAP, (d, DEPTH_CAP)


@pytest.mark.parametrize("how", ["no_autocast", "train", "pre_hook"])
def test_auto_stays_on_torch_elsewhere(cuda, how):
    """Outside autocast, in training mode or with a forward pre-hook on
    net.convs: no HIP launch and the bits of context_precision="torch"."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        outs = []
        for cp in ("auto", "torch"):
            net, run = _route_net(cuda, context_precision=cp)
            if how == "train":
                net.train()
            if how == "pre_hook":
                net.convs.register_forward_pre_hook(lambda m, i: None)
            out, n = _launches(lambda: run(autocast=how != "no_autocast"))
            assert n == {"context_conv2": 0, "context_pack": 0}, (cp, n)
            outs.append(out)
    finally:
        torch.backends.cudnn.deterministic = det
    assert _bits_equal(outs[0][0], outs[1][0]) and _bits_equal(outs[0][1], outs[1][1])
    assert not _bits_equal(outs[0][0], outs[0][1])


def test_forced_precisions(cuda):
    """"fp16" / "bf16" take the HIP route without autocast; training mode raises."""
    for cp in ("fp16", "bf16"):
        net, run = _route_net(cuda, context_precision=cp)
        (depth_init, depth), n = _launches(lambda: run(autocast=False))
        assert n["context_conv2"] >= 7 and n["context_pack"] >= 1 and not _bits_equal(depth_init, depth)
        net.train()
        with pytest.raises(RuntimeError, match="eval"):
            run(autocast=False)


def test_ind_context_feeds_context_net_features(cuda):
    """IND_CONTEXT: the stack reads context_net's features (PSNet.py:177-178), not the sweep's."""
    from sfm_amd import synth
    from sfm_amd.context import context_refine
    net, run = _route_net(cuda, IND_CONTEXT=True)
    own = synth.features(SB, 32, SH, SW, seed=21)[0].half().to(cuda)
    net.context_net = _Fixed(own)
    seen = []
    import sfm_amd.psnet as P
    real = P.context_refine

    def spy(convs, ctx, costs, **kw):
        seen.append((ctx, costs))
        return real(convs, ctx, costs, **kw)
    P.context_refine = spy
    try:
        (depth_init, depth), n = _launches(run)
    finally:
        P.context_refine = real
    assert n["context_conv2"] >= 7 and len(seen) == 1 and seen[0][0] is own
    # and the result is the one those features give, not the sweep's
    from sfm_amd.depth import depth_head
    want = depth_head(context_refine(net.convs, own, seen[0][1]).reshape(SB, SL, SH, SW).contiguous(), SL, 1.0,
                      (4 * SH, 4 * SW), False)
    assert _bits_equal(depth, want)
    net2, run2 = _route_net(cuda)
    assert not _bits_equal(run2()[1], depth)
