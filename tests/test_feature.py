"""CPU-side checks of the feature CNN on libsfm_hip (csrc/feature.hip,
sfm_amd/feature.py): exported symbols, the layout check, weight packing and
BatchNorm2d folding against the module's own float64 forward, PSNet's
``feature_precision`` argument, argument validation without a device, and the
condition the GPU tests' seeded weights have to meet."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from tests import feature_cases as FC

NEW = ("sfm_conv2x_f16", "sfm_image_pack_f16", "sfm_avgpool_f16", "sfm_spp_pack_f16")


def _stock():
    from sfm_amd.psnet import FeatureExtraction
    torch.manual_seed(1)
    return FeatureExtraction().eval()


def test_symbols_exported():
    from sfm_amd import _lib
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n


def test_layout_accepts_the_stock_module():
    from sfm_amd.feature import feature_layout_ok
    assert feature_layout_ok(_stock())
    assert feature_layout_ok(FC.recipe()[0])


def test_layout_rejects_anything_else():
    from sfm_amd.feature import FeatureLayoutError, feature_extract, feature_layout_ok, pack_feature_extraction
    m = _stock()
    m.layer2[0].conv1[0][0].stride = (1, 1)                              # a changed stride
    assert not feature_layout_ok(m)
    with pytest.raises(FeatureLayoutError, match="stride"):
        pack_feature_extraction(m, "cpu")
    m = _stock()
    m.layer1[1].conv2[0] = nn.Conv2d(32, 32, 3, padding=1, bias=True)    # an added bias
    assert not feature_layout_ok(m)
    with pytest.raises(FeatureLayoutError, match="bias"):
        pack_feature_extraction(m, "cpu")
    m = _stock()
    m.branch3[1][1] = nn.BatchNorm2d(32, track_running_stats=False)     # nothing to fold
    assert not feature_layout_ok(m)
    with pytest.raises(FeatureLayoutError, match="running statistics"):
        pack_feature_extraction(m, "cpu")
    m = _stock()
    m.branch2[0] = nn.AvgPool2d((8, 8), stride=(8, 8))                   # another pool size
    assert not feature_layout_ok(m)
    m = _stock()
    m.lastconv[2] = nn.Conv2d(128, 32, 1, dilation=2, bias=False)        # another dilation
    assert not feature_layout_ok(m)
    m = _stock()
    m.extra = nn.Identity()                                              # another child
    assert not feature_layout_ok(m)
    fn = lambda x: x                                                     # noqa: E731
    assert not feature_layout_ok(fn) and not feature_layout_ok(nn.Sequential(_stock()))
    with pytest.raises(FeatureLayoutError, match="FeatureExtraction"):
        pack_feature_extraction(fn, "cpu")
    with pytest.raises(RuntimeError, match="device"):                    # no CPU fallback
        feature_extract(_stock(), torch.zeros(1, 3, 130, 150))


def test_pack_shapes_and_cache():
    from sfm_amd.feature import pack_feature_extraction
    m = _stock()
    packed = pack_feature_extraction(m, "cpu")
    assert [len(b) for b in packed["layers"]] == [3, 16, 3, 3] and len(packed["first"]) == 3
    first = packed["first"][0]
    assert tuple(first["w"].shape) == (9, 32, 32) and first["w"].dtype == torch.float16
    assert (first["cin"], first["cin_pad"], first["stride"], first["relu"]) == (3, 32, 2, True)
    assert bool((first["w"][:, :, 3:] == 0).all())
    w = m.firstconv[0][0].weight.detach()
    for kh in range(3):
        for kw in range(3):
            assert torch.equal(first["w"][kh * 3 + kw, :, :3], w[:, :, kh, kw].half())
    c1, c2, ds = packed["layers"][1][0]
    assert (c1["stride"], c1["relu"], c2["stride"], c2["relu"]) == (2, True, 1, False)
    assert (ds["ksize"], ds["stride"], ds["relu"], tuple(ds["w"].shape)) == (1, 2, False, (1, 64, 32))
    assert packed["layers"][1][1][2] is None and packed["layers"][3][0][0]["dilation"] == 2
    assert [p for p, _ in packed["branches"]] == [32, 16, 8, 4]
    last = packed["last"]
    assert tuple(last[0]["w"].shape) == (9, 128, 320) and tuple(last[1]["w"].shape) == (1, 32, 128)
    assert bool((last[1]["scale"] == 1).all()) and bool((last[1]["bias"] == 0).all()) and not last[1]["relu"]
    assert pack_feature_extraction(m, "cpu") is packed                   # cached
    with torch.no_grad():
        m.layer3[2].conv2[1].running_mean.add_(1.0)
    assert pack_feature_extraction(m, "cpu") is not packed               # a changed buffer repacks


def test_batchnorm_fold_matches_float64_forward():
    """The packed layers composed in float64 against the module's own float64
    forward, the module's conv weights rounded to float16 first so that both
    hold the same weights.  What is left is the fp32 rounding of each folded
    scale and bias, a few 2^-24 relative per layer over about 70 layers whose
    outputs stay of the magnitude of their inputs: 1e-4 of the output's
    max-abs is a wide bound on that and 1000 times below a wrong fold (a
    dropped mean, variance or eps changes outputs by 1e-1 and more)."""
    from sfm_amd.feature import pack_feature_extraction
    net, image = FC.recipe()
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            m.weight.data = m.weight.data.half().float()
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(image.double())
        got = FC.composed64(pack_feature_extraction(net, "cpu"), image)
    assert got.shape == ref.shape
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"folded float64 composition vs module float64 forward: max-abs / max-abs {err:.3e}")
    assert err <= 1e-4, err


def test_recipe_stays_in_float16_range():
    """A condition on the GPU tests' inputs: every Conv2d, BatchNorm2d and
    residual-block output of the float64 forward stays under 1e3."""
    from sfm_amd.psnet import _Residual
    net, image = FC.recipe()
    net = net.double()
    peak = [0.0]

    def hook(mod, inp, out):
        peak[0] = max(peak[0], float(out.abs().max()))
    n = 0
    for m in net.modules():
        if isinstance(m, (nn.Conv2d, nn.BatchNorm2d, _Residual)):
            m.register_forward_hook(hook)
            n += 1
    with torch.no_grad():
        out = net(image.double())
    print(f"recipe: max |activation| over {n} hooked modules {peak[0]:.1f}, max |feature| {float(out.abs().max()):.2f}")
    assert n == 146 and 0.0 < peak[0] < 1e3, peak[0]      # 61 Conv2d + 60 BatchNorm2d + 25 blocks


def test_psnet_feature_precision_argument():
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    with pytest.raises(ValueError, match="fp8"):
        PSNet(8, cfg=c, feature_precision="fp8")
    net = PSNet(8, cfg=c).eval()
    assert net.feature_precision == "auto"
    assert net.feature_route(torch.device("cpu"), (130, 150)) == "torch"          # no GPU tensor: torch
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert net.feature_route(torch.device("cpu"), (130, 150)) == "torch"
    assert net.train().feature_route(torch.device("cpu"), (130, 150)) == "torch"
    assert PSNet(8, cfg=c, feature_precision="torch").feature_route() == "torch"
    forced = PSNet(8, cfg=c, feature_precision="fp16")
    assert forced.eval().feature_route() == "fp16"
    with pytest.raises(RuntimeError, match="eval"):
        forced.train().feature_route()
    injected = PSNet(8, cfg=c, feature_fn=lambda x: x).eval()
    assert injected.feature_route(torch.device("cpu"), (130, 150)) == "torch"


def test_conv2x_argument_errors():
    from sfm_amd import _lib
    lib = _lib.load()
    v, o = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def call(in_=v, images=1, cin=32, h=4, w=4, wt=v, cout=32, k=3, stride=1, dil=1, sc=v, bi=v, relu=1, res=None,
             out=o):
        return lib.sfm_conv2x_f16(in_, images, cin, h, w, wt, cout, k, stride, dil, sc, bi, relu, res, out, None)
    for kw in (dict(in_=None), dict(wt=None), dict(sc=None), dict(bi=None), dict(out=None)):
        assert call(**kw) == 1 and b"null" in lib.sfm_last_error(), kw
    for cin in (0, 16, 48, 352):
        assert call(cin=cin) == 1 and b"cin" in lib.sfm_last_error(), cin
    for cout in (0, 1, 48, 160):
        assert call(cout=cout) == 1 and b"cout" in lib.sfm_last_error(), cout
    for k in (0, 2, 5):
        assert call(k=k) == 1 and b"ksize" in lib.sfm_last_error(), k
    for stride in (0, 3):
        assert call(stride=stride) == 1 and b"stride" in lib.sfm_last_error(), stride
    for dil in (0, 17):
        assert call(dil=dil) == 1 and b"dilation" in lib.sfm_last_error(), dil
    assert call(stride=2, dil=2) == 1 and b"dilation 1 only" in lib.sfm_last_error()
    assert call(k=1, dil=2) == 1 and b"dilation 1 only" in lib.sfm_last_error()
    assert call(relu=1, res=v) == 1 and b"relu with a residual" in lib.sfm_last_error()
    for kw in (dict(images=0), dict(h=0), dict(w=-3)):
        assert call(**kw) == 1 and b"shape" in lib.sfm_last_error(), kw
    assert call(out=v) == 1 and b"alias" in lib.sfm_last_error()
    assert call(relu=0, res=o) == 1 and b"alias" in lib.sfm_last_error()
    for kw in (dict(in_=ctypes.c_void_p(18)), dict(wt=ctypes.c_void_p(24)), dict(out=ctypes.c_void_p(4100)),
               dict(relu=0, res=ctypes.c_void_p(8))):
        assert call(**kw) == 1 and b"aligned" in lib.sfm_last_error(), kw


def test_pack_and_pool_argument_errors():
    from sfm_amd import _lib
    lib = _lib.load()
    v, o = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    assert lib.sfm_image_pack_f16(None, 1, 4, 4, o, None) == 1 and b"null" in lib.sfm_last_error()
    assert lib.sfm_image_pack_f16(v, 0, 4, 4, o, None) == 1 and b"shape" in lib.sfm_last_error()
    assert lib.sfm_image_pack_f16(v, 1, 4, 4, ctypes.c_void_p(4104), None) == 1 and b"aligned" in lib.sfm_last_error()
    for p in (0, 2, 5, 64):
        assert lib.sfm_avgpool_f16(v, 1, 64, 64, 128, p, o, None) == 1 and b"pool size" in lib.sfm_last_error(), p
    assert lib.sfm_avgpool_f16(v, 1, 64, 64, 12, 4, o, None) == 1 and b"multiple of 8" in lib.sfm_last_error()
    assert lib.sfm_avgpool_f16(v, 1, 3, 64, 128, 4, o, None) == 1 and b"shape" in lib.sfm_last_error()
    assert lib.sfm_avgpool_f16(ctypes.c_void_p(8), 1, 64, 64, 128, 4, o, None) == 1 and b"aligned" in lib.sfm_last_error()
    ptrs = (ctypes.c_void_p * 4)(16, 32, 48, 64)
    bh, bw = (ctypes.c_int * 4)(8, 4, 2, 1), (ctypes.c_int * 4)(9, 4, 2, 1)
    assert lib.sfm_spp_pack_f16(v, v, ptrs, bh, bw, 1, 0, 38, o, None) == 1 and b"shape" in lib.sfm_last_error()
    assert lib.sfm_spp_pack_f16(v, v, None, bh, bw, 1, 33, 38, o, None) == 1 and b"null" in lib.sfm_last_error()
    bad = (ctypes.c_void_p * 4)(16, 32, 40, 64)
    assert lib.sfm_spp_pack_f16(v, v, bad, bh, bw, 1, 33, 38, o, None) == 1 and b"aligned" in lib.sfm_last_error()
    zero = (ctypes.c_int * 4)(8, 4, 0, 1)
    assert lib.sfm_spp_pack_f16(v, v, ptrs, zero, bw, 1, 33, 38, o, None) == 1 and b"branch map" in lib.sfm_last_error()
