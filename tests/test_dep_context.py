"""CPU-side checks of the full-resolution refinement stack on libsfm_hip
(csrc/context.hip ``k_dep_pack``, ``sfm_amd.context.dep_context_refine``,
PSNet's ``dep_context_precision``): exported symbols and their declared
signatures, argument validation without a device (stand-in pointers that are
never dereferenced), the 36-channel first-stage packing, and the refusals of
the driver."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfm_dep_context_pack_f16", "sfm_dep_context_pack_bf16")
PLAN = ((36, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 1, 1))


def _stack(cin=36, seed=0):
    from sfm_amd.psnet import _context_stack
    torch.manual_seed(seed)
    convs = _context_stack(cin, False)
    for m in convs.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return convs.eval()


@pytest.mark.parametrize("fn", NEW)
def test_exported_with_declared_signature(fn):
    from sfm_amd import _lib
    lib = _lib.load()
    assert fn in _lib.SYMBOLS and hasattr(lib, fn)
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % fn, hdr)
    assert m, fn + " is not declared in sfm_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    want = ["const float* depth", "const void* feat", "int feat_dtype", "const float* image", "int batch", "int b0",
            "int nb", "int channels", "int h", "int w", "int H", "int W", "void* out", "void* stream"]
    assert params == want
    sig = dict((s[0], s) for s in _lib._SIGS)[fn]
    assert sig[1] is ctypes.c_int and len(sig[2]) == len(want)
    for p, t in zip(want, sig[2]):
        assert t is (ctypes.c_int if p.startswith("int ") else ctypes.c_void_p), p
    # the declaration cites the lines of the reference it replaces
    assert "PSNet.py:218-221" in hdr[:m.start()].rsplit("/*", 1)[1]


@pytest.mark.parametrize("fn", NEW)
def test_pack_argument_errors(fn):
    from sfm_amd import _lib
    lib = _lib.load()
    f = getattr(lib, fn)
    v, o = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def call(depth=v, feat=v, dt=2, image=v, batch=2, b0=0, nb=2, ch=32, h=4, w=5, H=13, W=17, out=o):
        return f(depth, feat, dt, image, batch, b0, nb, ch, h, w, H, W, out, None)
    for kw in (dict(depth=None), dict(feat=None), dict(image=None), dict(out=None)):
        assert call(**kw) == 1 and b"null" in lib.sfm_last_error(), kw
    assert call(out=ctypes.c_void_p(4096 + 8)) == 1 and b"aligned" in lib.sfm_last_error()
    for ch in (31, 33, 36):
        assert call(ch=ch) == 1 and b"32" in lib.sfm_last_error(), ch
    for kw in (dict(h=0), dict(w=0), dict(H=0), dict(W=-1), dict(batch=0)):
        assert call(**kw) == 1 and b"shape" in lib.sfm_last_error(), kw
    for dt in (-1, 3):
        assert call(dt=dt) == 1 and b"feat_dtype" in lib.sfm_last_error(), dt
    for kw in (dict(b0=-1), dict(nb=0), dict(b0=1, nb=2), dict(b0=2, nb=1)):
        assert call(**kw) == 1 and b"pair range" in lib.sfm_last_error(), kw
    # size guards: the in-image offsets are 32-bit
    assert call(H=1 << 14, W=1 << 14) == 1 and b"too large" in lib.sfm_last_error()
    assert call(h=1 << 14, w=1 << 14) == 1 and b"too large" in lib.sfm_last_error()
    assert call(batch=1 << 12, nb=1 << 12, H=1 << 13, W=1 << 13) == 1 and b"grid" in lib.sfm_last_error()


@pytest.mark.parametrize("precision,dtype", [("fp16", torch.float16), ("bf16", torch.bfloat16)])
def test_pack_36_channel_stack(precision, dtype):
    from sfm_amd.context import dep_stock_layout, pack_context_stack, stock_layout
    convs = _stack()
    packed = pack_context_stack(convs, "cpu", precision)
    assert len(packed) == 7
    first = packed[0]
    assert tuple(first["w"].shape) == (9, 128, 64) and first["w"].dtype == dtype
    assert (first["cin"], first["cin_pad"], first["cout"]) == (36, 64, 128)
    assert bool((first["w"][:, :, 36:] == 0).all()) and bool((first["w"][:, :, :36] != 0).any())
    w = convs[0][0].weight.detach()
    for kh in range(3):
        for kw in range(3):
            # no permutation of the 36 inputs: depth, 32 features, image, in the reference's cat order
            assert torch.equal(first["w"][kh * 3 + kw, :, :36], w[:, :, kh, kw].to(dtype))
    for lay, (cin, cout, dil) in zip(packed, PLAN):
        assert (lay["cin"], lay["cout"], lay["dilation"], lay["relu"]) == (cin, cout, dil, True)
    assert dep_stock_layout(convs) and not stock_layout(convs)
    assert not dep_stock_layout(_stack(33)) and stock_layout(_stack(33))
    assert not dep_stock_layout(nn.Sequential(*list(_stack())[:1]))          # one stage, 128 outputs
    assert not dep_stock_layout(nn.Sequential(nn.Conv2d(36, 1, 5, padding=2, bias=False)))


def test_psnet_dep_context_precision_argument():
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    c = defaults()
    c.update(PSNET_DEP_CONTEXT=True)
    for bad in ("fp8", "fp32", None):
        with pytest.raises(ValueError, match="dep_context"):
            PSNet(8, cfg=c, feature_fn=lambda x: x, dep_context_precision=bad)
    net = PSNet(8, cfg=c, feature_fn=lambda x: x).eval()
    assert net.dep_context_precision == "auto"
    assert net.dep_context_route(torch.device("cpu")) == "torch"          # no GPU tensor: torch
    assert net.dep_context_route() == "torch"
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert net.dep_context_route(torch.device("cpu")) == "torch"
    for p in ("auto", "torch", "fp16", "bf16"):
        assert PSNet(8, cfg=c, feature_fn=lambda x: x, dep_context_precision=p).dep_context_precision == p
    assert PSNet(8, cfg=c, feature_fn=lambda x: x, dep_context_precision="torch").dep_context_route() == "torch"
    forced = PSNet(8, cfg=c, feature_fn=lambda x: x, dep_context_precision="bf16")
    assert forced.eval().dep_context_route() == "bf16" and forced.context_route() == "torch"
    with pytest.raises(RuntimeError, match="eval"):
        forced.train().dep_context_route()


def test_dep_context_refine_refusals():
    from sfm_amd.context import ContextStackError, dep_context_refine
    depth, feat, image = torch.zeros(1, 1, 8, 8), torch.zeros(1, 32, 2, 2), torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="device"):
        dep_context_refine(_stack(), depth, feat, image)
    with pytest.raises(ValueError, match="fp8"):
        dep_context_refine(_stack(), depth, feat, image, precision="fp8")
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        with pytest.raises(ContextStackError, match="36"):
            dep_context_refine(_stack(33), depth.to(dev), feat.to(dev), image.to(dev))


def test_dep_context_refine_refuses_a_33_channel_stack(monkeypatch):
    """The layout check comes before anything touches a device: tensors that
    only claim to be on one are enough to reach it."""
    from sfm_amd import context
    from sfm_amd.context import ContextStackError, dep_context_refine

    class OnDevice(torch.Tensor):
        is_cuda = True

    def fake(*shape):
        return torch.zeros(*shape).as_subclass(OnDevice)
    monkeypatch.setattr(context._lib, "load", lambda: pytest.fail("the library was reached"))
    with pytest.raises(ContextStackError, match="36"):
        dep_context_refine(_stack(33), fake(1, 1, 8, 8), fake(1, 32, 2, 2), fake(1, 3, 8, 8))
    five = nn.Sequential(nn.Sequential(nn.Conv2d(36, 32, 5, padding=2, bias=False), nn.ReLU()),
                         nn.Sequential(nn.Conv2d(32, 1, 3, padding=1, bias=False), nn.ReLU()))
    with pytest.raises(ContextStackError, match="3 x 3"):
        dep_context_refine(five, fake(1, 1, 8, 8), fake(1, 32, 2, 2), fake(1, 3, 8, 8))
