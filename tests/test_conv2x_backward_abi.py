"""CPU-side checks of the float16 training path of the feature CNN: the two
weight packings of sfm_amd.feature against torch's autograd in float64 over the
CNN's layer kinds (strided, 1 x 1, dilated, 320 input channels), the
declarations of sfm_conv2x_wgrad_f16 / sfm_conv2x_dgrad_f16, their refusals
(each returned with a message before anything is launched: no device is
touched, the pointers are never dereferenced) and the exported names.  The ABI
version stays 1."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 2
# (cin, cout, k, stride, dilation): firstconv.0, layer2.0.conv1, layer2.0.downsample, layer3.0.downsample,
# layer4's convs, lastconv.0
STAGES = [(3, 32, 3, 2, 1), (32, 64, 3, 2, 1), (32, 64, 1, 2, 1), (64, 128, 1, 1, 1), (128, 128, 3, 1, 2),
          (320, 128, 3, 1, 1)]
SIZES = [(7, 9), (8, 10)]           # odd and even at stride 2
CASES = [(st, hw) for st in STAGES for hw in SIZES]
IDS = [f"{a}to{b}-k{k}s{s}d{d}-{h}x{w}" for (a, b, k, s, d), (h, w) in CASES]


def _pad32(n):
    return (n + 31) // 32 * 32


def _case(stage, hw, seed):
    cin, cout, k, stride, dil = stage
    pad = dil if k == 3 else 0
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, *hw, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wt, stride=stride, padding=pad, dilation=dil)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    return x.detach(), wt.detach(), gy, x.grad, wt.grad


@pytest.mark.parametrize("stage,hw", CASES, ids=IDS)
def test_dgrad_packing_is_autograds_grad_input(stage, hw):
    """grad_in[p] = sum over t, q with q stride + (tap - pad) dil = p of
    W[tap] gy[q], tap = k^2 - 1 - t: with pack_dgrad_weights2x's pack viewed as
    a [cout_pad, cin_pad, k, k] weight (flipped back) that is conv_transpose2d
    of the padded output gradient; the output padding makes up the rows and
    columns the strided forward did not reach.  Autograd's grad_input, and
    zeros in the padding's channels."""
    from sfm_amd.feature import pack_dgrad_weights2x
    cin, cout, k, stride, dil = stage
    pad = dil if k == 3 else 0
    x, wt, gy, gx, _ = _case(stage, hw, 3)
    wd = pack_dgrad_weights2x(wt)
    cip, cop = _pad32(cin), _pad32(cout)
    assert tuple(wd.shape) == (k * k, cip, cop) and wd.dtype == torch.float64
    gp = torch.zeros(N, cop, *gy.shape[2:], dtype=torch.float64)
    gp[:, :cout] = gy
    # Wd[t][ci][co] = W[co][ci][k^2 - 1 - t]: flipped back and viewed [co, ci, kh, kw], the transposed conv's weight
    wv = wd.flip(0).permute(2, 1, 0).reshape(cop, cip, k, k)
    opad = tuple((n + 2 * pad - dil * (k - 1) - 1) % stride for n in hw)
    got = F.conv_transpose2d(gp, wv, stride=stride, padding=pad, dilation=dil, output_padding=opad)
    assert tuple(got.shape[2:]) == tuple(hw)
    assert float((got[:, :cin] - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert bool((got[:, cin:] == 0).all())
    if stride == 1:
        # at stride 1 the pack is a plain convolution's weight, as sfm_conv2_dgrad_f16's
        direct = F.conv2d(gp, wd.permute(1, 2, 0).reshape(cip, cop, k, k), padding=pad, dilation=dil)
        assert float((direct[:, :cin] - gx).abs().max()) <= 1e-12 * float(gx.abs().max())


@pytest.mark.parametrize("stage,hw", CASES, ids=IDS)
def test_wgrad_formula_unpacked_is_autograds_grad_weight(stage, hw):
    """gW[tap][co][ci] = sum gy[img, y, x, co] in[img, y S + (kh - pad) dil, x S + (kw - pad) dil, ci]
    on padded operands, then unpack_wgrad2x: autograd's grad_weight."""
    from sfm_amd.feature import unpack_wgrad2x
    cin, cout, k, stride, dil = stage
    pad = dil if k == 3 else 0
    x, wt, gy, _, gw = _case(stage, hw, 4)
    cip, cop = _pad32(cin), _pad32(cout)
    ho, wo = gy.shape[2:]
    assert (ho, wo) == ((hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1)
    gp = torch.zeros(N, cop, ho, wo, dtype=torch.float64)
    gp[:, :cout] = gy
    xp = torch.zeros(N, cip, *hw, dtype=torch.float64)
    xp[:, :cin] = x
    xp = F.pad(xp, (pad, pad + stride, pad, pad + stride))          # room for the last strided window
    gwp = torch.zeros(k * k, cop, cip, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            win = xp[:, :, kh * dil:kh * dil + stride * ho:stride, kw * dil:kw * dil + stride * wo:stride]
            gwp[kh * k + kw] = torch.einsum("bohw,bihw->oi", gp, win)
    got = unpack_wgrad2x(gwp, cout, cin, k)
    assert tuple(got.shape) == tuple(gw.shape)
    assert float((got - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


def _params(hdr, name, ret="int"):
    m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in sfm_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    return [" ".join(p.split()) for p in params], hdr[:m.start()].rsplit("/*", 1)[1]


def test_exported_with_declared_signatures():
    from sfm_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    sigs = dict((s[0], s) for s in _lib._SIGS)
    want = {
        "sfm_conv2x_wgrad_f16_workspace_bytes": ["int images", "int cin", "int cout", "int hin", "int win",
                                                 "int ksize", "int stride"],
        "sfm_conv2x_wgrad_f16": [
            "const void* in", "const void* grad_out", "int images", "int cin", "int cout", "int hin", "int win",
            "int ksize", "int stride", "int dilation", "float* grad_weights", "void* workspace",
            "size_t workspace_bytes", "void* stream"],
        "sfm_conv2x_dgrad_f16": [
            "const void* grad_out", "int images", "int cout", "int hout", "int wout", "const void* weights", "int cin",
            "int hin", "int win", "int ksize", "int stride", "int dilation", "void* grad_in", "void* stream"],
    }
    for name, params in want.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        ret = "size_t" if name.endswith("_bytes") else "int"
        got, doc = _params(hdr, name, ret)
        assert got == params, name
        sig = sigs[name]
        assert sig[1] is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and len(sig[2]) == len(params), name
        for kind, p in zip(sig[2], params):
            assert (kind is ctypes.c_size_t) == p.startswith("size_t "), (name, p)
            assert (kind is ctypes.c_int) == p.startswith("int "), (name, p)
        # every declaration cites the reference lines it differentiates
        assert "models/submodule.py" in doc and "11-15" in doc and "22-44" in doc and "108-184" in doc, name
    _, doc = _params(hdr, "sfm_conv2x_wgrad_f16_workspace_bytes", "size_t")
    assert "conv2_wgrad_blocks" in doc and '"conv2x_wgrad"' in doc and "32-bit" in doc
    _, doc = _params(hdr, "sfm_conv2x_dgrad_f16")
    assert "Wd[t][ci][co] = W[co][ci][ksize^2 - 1 - t]" in doc and '"conv2x_dgrad"' in doc
    assert lib.sfm_abi_version() == 1


# distinct, 16-byte aligned stand-in pointers far enough apart that no operand overlaps another
X, G, GW, WS, WD = (ctypes.c_void_p(a << 32) for a in (1, 2, 3, 4, 5))
SH = dict(images=2, cin=32, cout=64, hin=9, win=131, k=3, stride=2, dil=1)


def _ws_bytes(lib, s):
    return lib.sfm_conv2x_wgrad_f16_workspace_bytes(s["images"], s["cin"], s["cout"], s["hin"], s["win"], s["k"],
                                                    s["stride"])


def _wgrad(lib, x=X, g=G, gw=GW, ws=WS, ws_bytes=None, **kw):
    s = dict(SH, **kw)
    if ws_bytes is None:
        ws_bytes = _ws_bytes(lib, s) or _ws_bytes(lib, SH)
    return lib.sfm_conv2x_wgrad_f16(x, g, s["images"], s["cin"], s["cout"], s["hin"], s["win"], s["k"], s["stride"],
                                    s["dil"], gw, ws, ws_bytes, None)


def test_wgrad_refuses_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def refused(**kw):
        rc = _wgrad(lib, **kw)
        msg = lib.sfm_last_error()
        assert rc != 0 and msg, (kw, rc, msg)
        return rc, msg

    for name in ("x", "g", "gw"):
        rc, msg = refused(**{name: None})
        assert rc == 1 and b"null" in msg, (name, msg)
    for bad in (48, 16, 352, 0, 3):
        rc, msg = refused(cin=bad)
        assert rc == 1 and b"cin" in msg, bad
    for bad in (48, 160, 1, 0):
        rc, msg = refused(cout=bad)
        assert rc == 1 and b"cout" in msg, bad
    for bad in (2, 5, 0):
        rc, msg = refused(k=bad)
        assert rc == 1 and b"ksize" in msg
    for bad in (0, 3, 4):
        rc, msg = refused(stride=bad)
        assert rc == 1 and b"stride" in msg
    for bad in (0, 17, -1):
        rc, msg = refused(dil=bad, stride=1)
        assert rc == 1 and b"dilation" in msg
    for kw in (dict(dil=2), dict(dil=2, k=1, stride=1), dict(dil=2, k=1)):          # a dilation at stride 2 or 1 x 1
        rc, msg = refused(**kw)
        assert rc == 1 and b"dilation 1 only" in msg, kw
    for k in ("images", "hin", "win"):
        rc, msg = refused(**{k: 0})
        assert rc == 1 and b"shape" in msg, k
    rc, msg = refused(hin=4096, win=4096, cin=320, stride=1)                         # 2^24 pixels x 320 channels
    assert rc == 1 and b"32-bit" in msg
    # 2 images of 9 x 131 at stride 2: 5 x 66 outputs, 2 x 2 tiles of 4 rows x 64 columns each
    need = _ws_bytes(lib, SH)
    assert need == 2 * 2 * 2 * 9 * 64 * 32 * 4
    assert _ws_bytes(lib, dict(SH, k=1)) == 8 * 64 * 32 * 4
    assert _ws_bytes(lib, dict(SH, cin=320, cout=128, stride=1)) == 2 * 3 * 3 * 9 * 128 * 320 * 4
    for kw in (dict(cin=48), dict(cout=1), dict(images=0), dict(k=2), dict(stride=3)):
        assert _ws_bytes(lib, dict(SH, **kw)) == 0, kw
    # at 3 x 3 / stride 1 / cin <= 128 the delegated kernel's own figure
    assert _ws_bytes(lib, dict(SH, cin=64, cout=96, hin=9, win=67, stride=1)) == \
        lib.sfm_conv2_wgrad_f16_workspace_bytes(2, 64, 96, 9, 67)
    rc, msg = refused(ws_bytes=need - 1)
    assert rc == 3 and b"workspace" in msg and str(need).encode() in msg
    rc, msg = refused(ws=None)
    assert rc == 3 and b"workspace" in msg
    for name, p in (("x", X), ("g", G), ("gw", GW), ("ws", WS)):
        for off in (2, 8):
            rc, msg = refused(**{name: ctypes.c_void_p(p.value + off)})
            assert rc == 1 and b"aligned" in msg, (name, off, msg)
    for kw in (dict(gw=X), dict(gw=G), dict(gw=WS), dict(ws=X), dict(ws=G),
               dict(gw=ctypes.c_void_p(X.value + 64)), dict(ws=ctypes.c_void_p(G.value + 1024))):
        rc, msg = refused(**kw)
        assert rc == 1 and b"alias" in msg, (kw, msg)
    # the tuning key is the context stack's
    try:
        _lib.tune("conv2_wgrad_blocks", 7)
        assert _ws_bytes(lib, SH) == 7 * 9 * 64 * 32 * 4
    finally:
        _lib.tune("conv2_wgrad_blocks", 0)


def test_dgrad_refuses_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def dgrad(g=G, wts=WD, out=X, images=2, cout=64, hout=5, wout=66, cin=32, hin=9, win=131, k=3, stride=2, dil=1):
        rc = lib.sfm_conv2x_dgrad_f16(g, images, cout, hout, wout, wts, cin, hin, win, k, stride, dil, out, None)
        return rc, lib.sfm_last_error()

    for kw, word in ((dict(g=None), b"null"), (dict(wts=None), b"null"), (dict(out=None), b"null"),
                     (dict(cout=48), b"cout"), (dict(cout=1), b"cout"), (dict(cin=33), b"cin"), (dict(cin=352), b"cin"),
                     (dict(k=2), b"ksize"), (dict(stride=3), b"stride"), (dict(dil=0, stride=1, hout=9, wout=131), b"dilation"),
                     (dict(dil=17, stride=1, hout=9, wout=131), b"dilation"), (dict(dil=2), b"dilation 1 only"),
                     (dict(dil=2, k=1, stride=1, hout=9, wout=131), b"dilation 1 only"),
                     (dict(hin=0), b"shape"), (dict(images=0), b"shape"),
                     (dict(hin=11), b"not an input size"), (dict(hin=8), b"not an input size"),
                     (dict(win=133), b"not an input size"), (dict(hout=9), b"not an input size"),
                     (dict(stride=1), b"not an input size"),
                     (dict(out=G), b"alias"), (dict(out=WD), b"alias"), (dict(out=ctypes.c_void_p(G.value + 256)), b"alias"),
                     (dict(out=ctypes.c_void_p(X.value + 8)), b"aligned"),
                     (dict(wts=ctypes.c_void_p(WD.value + 4)), b"aligned"),
                     (dict(g=ctypes.c_void_p(G.value + 2)), b"aligned")):
        rc, msg = dgrad(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
    # both input heights of 5 output rows pass the shape check: the next refusal is another one
    for hin in (9, 10):
        rc, msg = dgrad(hin=hin, out=None)
        assert rc == 1 and b"null" in msg


def test_lazy_export_and_cpu_tensors_raise():
    import sfm_amd
    from sfm_amd import feature
    for name in ("conv2x_autograd", "conv2x_wgrad_f16", "conv2x_dgrad_f16", "pack_dgrad_weights2x", "unpack_wgrad2x"):
        assert name in sfm_amd.__all__ and getattr(sfm_amd, name) is getattr(feature, name), name
    half = lambda *s: torch.zeros(*s, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.conv2x_wgrad_f16(half(1, 4, 4, 32), half(1, 4, 4, 32), 3, 1, 1)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.conv2x_dgrad_f16(half(1, 4, 4, 32), half(9, 32, 32), (4, 4), 3, 1, 1)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.conv2x_autograd(half(1, 4, 4, 32), torch.zeros(32, 32, 3, 3))
