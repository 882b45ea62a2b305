"""CPU-side checks of the context stack on libsfm_hip (csrc/context.hip,
sfm_amd/context.py): exported symbols, argument validation without a device,
weight packing and BatchNorm2d folding, the named packing errors and PSNet's
``context_precision`` argument."""
import ctypes

import pytest
import torch
import torch.nn as nn

NEW = ("sfm_conv2_f16", "sfm_conv2_bf16", "sfm_context_pack_f16", "sfm_context_pack_bf16")
PLAN = ((33, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 1, 1))


def _stack(bn, seed=0):
    from sfm_amd.psnet import _context_stack
    torch.manual_seed(seed)
    convs = _context_stack(33, bn)
    for m in convs.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return convs.eval()


def test_symbols_exported():
    from sfm_amd import _lib
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n


@pytest.mark.parametrize("fn", ["sfm_conv2_f16", "sfm_conv2_bf16"])
def test_conv2_argument_errors(fn):
    from sfm_amd import _lib
    lib = _lib.load()
    f = getattr(lib, fn)
    v, o = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def call(in_=v, images=1, cin=32, h=4, w=4, wt=v, cout=32, dil=1, sc=v, bi=v, relu=1, res=None, out=o):
        return f(in_, images, cin, h, w, wt, cout, dil, sc, bi, relu, res, out, None)
    for kw in (dict(in_=None), dict(wt=None), dict(sc=None), dict(bi=None), dict(out=None)):
        assert call(**kw) == 1 and b"null" in lib.sfm_last_error(), kw
    for cin in (0, 16, 33, 48, 160):
        assert call(cin=cin) == 1 and b"cin" in lib.sfm_last_error(), cin
    for cout in (0, 2, 16, 48, 160):
        assert call(cout=cout) == 1 and b"cout" in lib.sfm_last_error(), cout
    for dil in (0, -1, 17):
        assert call(dil=dil) == 1 and b"dilation" in lib.sfm_last_error(), dil
    for kw in (dict(images=0), dict(h=0), dict(w=-3)):
        assert call(**kw) == 1 and b"shape" in lib.sfm_last_error(), kw
    assert call(res=v) == 1 and b"residual1" in lib.sfm_last_error()         # residual only with cout 1
    assert call(out=v) == 1 and b"alias" in lib.sfm_last_error()
    assert call(in_=ctypes.c_void_p(18)) == 1 and b"aligned" in lib.sfm_last_error()


@pytest.mark.parametrize("fn", ["sfm_context_pack_f16", "sfm_context_pack_bf16"])
def test_pack_argument_errors(fn):
    from sfm_amd import _lib
    lib = _lib.load()
    f = getattr(lib, fn)
    v, o = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def call(ctx=v, planes=v, batch=2, nlabel=3, l0=1, nl=2, ch=32, h=4, w=4, out=o):
        return f(ctx, planes, batch, nlabel, l0, nl, ch, h, w, out, None)
    for kw in (dict(ctx=None), dict(planes=None), dict(out=None)):
        assert call(**kw) == 1 and b"null" in lib.sfm_last_error(), kw
    assert call(ch=33) == 1 and b"32" in lib.sfm_last_error()
    for kw in (dict(batch=0), dict(nlabel=0), dict(h=0), dict(w=0)):
        assert call(**kw) == 1 and b"shape" in lib.sfm_last_error(), kw
    for kw in (dict(l0=-1), dict(nl=0), dict(l0=2, nl=2)):
        assert call(**kw) == 1 and b"plane range" in lib.sfm_last_error(), kw


@pytest.mark.parametrize("precision,dtype", [("fp16", torch.float16), ("bf16", torch.bfloat16)])
def test_pack_shapes_and_padding(precision, dtype):
    from sfm_amd.context import pack_context_stack
    convs = _stack(False)
    packed = pack_context_stack(convs, "cpu", precision)
    assert len(packed) == 7
    for lay, (cin, cout, dil), blk in zip(packed, PLAN, convs):
        cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
        assert tuple(lay["w"].shape) == (9, cout_pad, cin_pad) and lay["w"].dtype == dtype
        assert (lay["cin"], lay["cin_pad"], lay["cout"], lay["cout_pad"], lay["dilation"], lay["relu"]) == \
            (cin, cin_pad, cout, cout_pad, dil, True)
        assert lay["scale"].dtype == torch.float32 and tuple(lay["scale"].shape) == (cout_pad,)
        assert bool((lay["w"][:, cout:] == 0).all()) and bool((lay["w"][:, :, cin:] == 0).all())
        w = blk[0].weight.detach()
        for kh in range(3):
            for kw in range(3):
                assert torch.equal(lay["w"][kh * 3 + kw, :cout, :cin], w[:, :, kh, kw].to(dtype))
        assert bool((lay["scale"] == 1).all()) and bool((lay["bias"] == 0).all())
    assert pack_context_stack(convs, "cpu", precision) is packed          # cached
    with torch.no_grad():
        convs[0][0].weight.mul_(2.0)
    assert pack_context_stack(convs, "cpu", precision) is not packed      # a changed parameter repacks


def test_batchnorm_fold_matches_float64():
    from sfm_amd.context import pack_context_stack
    convs = _stack(True, seed=3)
    g = torch.Generator().manual_seed(5)
    for m in convs.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.weight.data = 0.5 + torch.rand(n, generator=g)
            m.bias.data = torch.randn(n, generator=g)
            m.running_mean.data = torch.randn(n, generator=g)
            m.running_var.data = 0.25 + 2.0 * torch.rand(n, generator=g)
    packed = pack_context_stack(convs, "cpu", "fp16")
    for lay, blk in zip(packed, convs):
        bn = blk[1]
        cout = lay["cout"]
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        bias = bn.bias.detach().double() - bn.running_mean.double() * scale
        # fp32 rounding of a handful of fp32 operations: a few ulp of the larger operand
        assert float((lay["scale"][:cout].double() - scale).abs().max()) <= 4 * 2.0 ** -24 * float(scale.abs().max())
        tol = 4 * 2.0 ** -24 * float((bn.bias.detach().double().abs() + (bn.running_mean.double() * scale).abs()).max())
        assert float((lay["bias"][:cout].double() - bias).abs().max()) <= tol
        assert bool((lay["scale"][cout:] == 1).all()) and bool((lay["bias"][cout:] == 0).all())
        assert isinstance(blk[2], nn.ReLU) and lay["relu"]


def test_unsupported_stacks_raise():
    from sfm_amd.context import ContextStackError, pack_context_stack
    five = nn.Sequential(nn.Sequential(nn.Conv2d(33, 32, 5, padding=2, bias=False), nn.ReLU()))
    with pytest.raises(ContextStackError, match="3 x 3"):
        pack_context_stack(five, "cpu", "fp16")
    biased = nn.Sequential(nn.Sequential(nn.Conv2d(33, 32, 3, padding=1, bias=True), nn.ReLU()))
    with pytest.raises(ContextStackError, match="bias"):
        pack_context_stack(biased, "cpu", "fp16")
    strided = nn.Sequential(nn.Sequential(nn.Conv2d(33, 32, 3, padding=1, stride=2, bias=False), nn.ReLU()))
    with pytest.raises(ContextStackError, match="stride"):
        pack_context_stack(strided, "cpu", "fp16")
    padded = nn.Sequential(nn.Sequential(nn.Conv2d(33, 32, 3, padding=1, dilation=2, bias=False), nn.ReLU()))
    with pytest.raises(ContextStackError, match="padding"):
        pack_context_stack(padded, "cpu", "fp16")
    with pytest.raises(ValueError):
        pack_context_stack(_stack(False), "cpu", "fp8")


def test_psnet_context_precision_argument():
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    with pytest.raises(ValueError, match="fp8"):
        PSNet(8, cfg=c, feature_fn=lambda x: x, context_precision="fp8")
    net = PSNet(8, cfg=c, feature_fn=lambda x: x).eval()
    assert net.context_precision == "auto"
    assert net.context_route(torch.device("cpu")) == "torch"              # no GPU tensor: torch
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert net.context_route(torch.device("cpu")) == "torch"
    assert PSNet(8, cfg=c, feature_fn=lambda x: x, context_precision="torch").context_route() == "torch"
    forced = PSNet(8, cfg=c, feature_fn=lambda x: x, context_precision="fp16")
    assert forced.eval().context_route() == "fp16"
    with pytest.raises(RuntimeError, match="eval"):
        forced.train().context_route()


def test_context_refine_refuses_cpu_tensors():
    from sfm_amd.context import context_refine
    with pytest.raises(RuntimeError, match="device"):
        context_refine(_stack(False), torch.zeros(1, 32, 4, 4), torch.zeros(1, 1, 2, 4, 4))
