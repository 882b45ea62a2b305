"""CPU-side checks of the float16 training path of the per-plane context stack:
the two weight packings of sfm_amd.context against torch's autograd in float64,
the declarations of sfm_conv2_wgrad_f16 / sfm_conv2_dgrad_f16 /
sfm_context_unpack_grad_f16, their refusals (each returned with a message before
anything is launched: no device is touched, the pointers are never
dereferenced), the tuning key and PSNet's ``context_grad`` argument.  The ABI
version stays 1."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, H, W = 2, 7, 9
# (cin, cout, dilation): the stock stack's first, widest-dilation and last stages
STAGES = [(33, 128, 1), (96, 64, 16), (128, 96, 8), (32, 1, 1)]


def _pad32(n):
    return (n + 31) // 32 * 32


def _case(cin, cout, dil, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(N, cout, H, W, generator=g, dtype=torch.float64)
    F.conv2d(x, wt, padding=dil, dilation=dil).backward(gy)
    return x.detach(), wt.detach(), gy, x.grad, wt.grad


@pytest.mark.parametrize("cin,cout,dil", STAGES)
def test_dgrad_packing_is_autograds_grad_input(cin, cout, dil):
    """sfm_conv2_f16 computes y[p, o] = sum Wp[tap][o][i] x[p + (tap - 1) dil, i];
    as a Conv2d that is the weight Wp.permute(1, 2, 0) viewed [o, i, 3, 3].  With
    pack_dgrad_weights2's pack in that role on the padded output gradient:
    autograd's grad_input, and zeros in the padding's channels."""
    from sfm_amd.context import pack_dgrad_weights2
    x, wt, gy, gx, _ = _case(cin, cout, dil, 3)
    wd = pack_dgrad_weights2(wt)
    cip, cop = _pad32(cin), _pad32(cout)
    assert tuple(wd.shape) == (9, cip, cop) and wd.dtype == torch.float64
    gp = torch.zeros(N, cop, H, W, dtype=torch.float64)
    gp[:, :cout] = gy
    got = F.conv2d(gp, wd.permute(1, 2, 0).reshape(cip, cop, 3, 3), padding=dil, dilation=dil)
    assert float((got[:, :cin] - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert bool((got[:, cin:] == 0).all())


@pytest.mark.parametrize("cin,cout,dil", STAGES)
def test_wgrad_formula_unpacked_is_autograds_grad_weight(cin, cout, dil):
    """gW[tap][co][ci] = sum gy[img, y, x, co] x[img, y + (kh-1) dil, x + (kw-1) dil, ci]
    on padded operands, then unpack_wgrad2: autograd's grad_weight."""
    from sfm_amd.context import unpack_wgrad2
    x, wt, gy, _, gw = _case(cin, cout, dil, 4)
    cip, cop = _pad32(cin), _pad32(cout)
    gp = torch.zeros(N, cop, H, W, dtype=torch.float64)
    gp[:, :cout] = gy
    xp = torch.zeros(N, cip, H, W, dtype=torch.float64)
    xp[:, :cin] = x
    xp = F.pad(xp, (dil, dil, dil, dil))
    gwp = torch.zeros(9, cop, cip, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            gwp[kh * 3 + kw] = torch.einsum("bohw,bihw->oi", gp, xp[:, :, kh * dil:kh * dil + H, kw * dil:kw * dil + W])
    got = unpack_wgrad2(gwp, cout, cin)
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
        "sfm_conv2_wgrad_f16_workspace_bytes": ["int images", "int cin", "int cout_pad", "int h", "int w"],
        "sfm_conv2_wgrad_f16": [
            "const void* in", "const void* grad_out", "int images", "int cin", "int cout_pad", "int h", "int w",
            "int dilation", "float* grad_weights", "void* workspace", "size_t workspace_bytes", "void* stream"],
        "sfm_conv2_dgrad_f16": [
            "const void* grad_out", "int images", "int cout_pad", "int h", "int w", "const void* weights",
            "int cin_pad", "int dilation", "const void* act", "void* grad_in", "void* stream"],
        "sfm_context_unpack_grad_f16": [
            "const void* grad_in0", "const float* grad_out", "int batch", "int nlabel", "int l0", "int nl", "int h",
            "int w", "int first", "float* grad_ctx", "float* grad_planes", "void* stream"],
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
        assert "models/PSNet.py" in doc and "17-26" in doc and "64-71" in doc and "175-190" in doc, name
    _, doc = _params(hdr, "sfm_conv2_wgrad_f16_workspace_bytes", "size_t")
    assert "conv2_wgrad_blocks" in doc and '"conv2_wgrad"' in doc
    _, doc = _params(hdr, "sfm_conv2_dgrad_f16")
    assert "Wd[t][ci][co] = W[co][ci][8 - t]" in doc and '"conv2_dgrad"' in doc
    assert lib.sfm_abi_version() == 1


# distinct, 16-byte aligned stand-in pointers far enough apart that no operand overlaps another
X, G, GW, WS, A = (ctypes.c_void_p(a << 32) for a in (1, 2, 3, 4, 5))
SH = dict(images=2, cin=64, cop=96, h=9, w=67, dil=2)


def _wgrad(lib, x=X, g=G, gw=GW, ws=WS, ws_bytes=None, **kw):
    s = dict(SH, **kw)
    if ws_bytes is None:
        ok = lambda c: c if c in (32, 64, 96, 128) else 32
        ws_bytes = lib.sfm_conv2_wgrad_f16_workspace_bytes(max(s["images"], 1), ok(s["cin"]), ok(s["cop"]),
                                                           max(s["h"], 1), max(s["w"], 1))
    return lib.sfm_conv2_wgrad_f16(x, g, s["images"], s["cin"], s["cop"], s["h"], s["w"], s["dil"], gw, ws, ws_bytes,
                                   None)


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
    for bad in (48, 16, 160, 1):
        rc, msg = refused(cin=bad)
        assert rc == 1 and b"cin" in msg
        rc, msg = refused(cop=bad)
        assert rc == 1 and b"cout_pad" in msg and b"padded" in msg
    for bad in (0, 17, -1):
        rc, msg = refused(dil=bad)
        assert rc == 1 and b"dilation" in msg
    for k in ("images", "h", "w"):
        rc, msg = refused(**{k: 0})
        assert rc == 1 and b"shape" in msg, k
    need = lib.sfm_conv2_wgrad_f16_workspace_bytes(2, 64, 96, 9, 67)
    tiles = 2 * 3 * 2                                        # 4-row x 64-column tiles of each image
    assert need == tiles * 9 * 96 * 64 * 4
    assert lib.sfm_conv2_wgrad_f16_workspace_bytes(2, 48, 96, 9, 67) == 0
    assert lib.sfm_conv2_wgrad_f16_workspace_bytes(2, 64, 1, 9, 67) == 0
    assert lib.sfm_conv2_wgrad_f16_workspace_bytes(0, 64, 96, 9, 67) == 0
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
    # the KITTI chunk: a grid sized to the machine, not one partial per tile
    kitti = lib.sfm_conv2_wgrad_f16_workspace_bytes(128, 128, 128, 94, 311)
    assert kitti == 512 * 9 * 128 * 128 * 4


def test_dgrad_and_unpack_refuse_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def dgrad(g=G, wts=WS, act=A, out=X, images=2, cop=96, h=9, w=67, cip=64, dil=2):
        rc = lib.sfm_conv2_dgrad_f16(g, images, cop, h, w, wts, cip, dil, act, out, None)
        return rc, lib.sfm_last_error()

    for kw, word in ((dict(g=None), b"null"), (dict(wts=None), b"null"), (dict(out=None), b"null"),
                     (dict(cop=48), b"cout_pad"), (dict(cop=1), b"cout_pad"), (dict(cip=33), b"cin_pad"),
                     (dict(dil=0), b"dilation"), (dict(dil=17), b"dilation"), (dict(h=0), b"shape"),
                     (dict(out=G), b"alias"), (dict(out=A), b"alias"),
                     (dict(act=ctypes.c_void_p(A.value + 8)), b"aligned"),
                     (dict(g=ctypes.c_void_p(G.value + 2)), b"aligned")):
        rc, msg = dgrad(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)

    def unpack(g=G, go=X, gc=GW, gp=WS, batch=2, nlabel=4, l0=1, nl=2, h=9, w=67, first=1):
        rc = lib.sfm_context_unpack_grad_f16(g, go, batch, nlabel, l0, nl, h, w, first, gc, gp, None)
        return rc, lib.sfm_last_error()

    for kw, word in ((dict(g=None), b"null"), (dict(gc=None), b"null"), (dict(gp=None), b"null"),
                     (dict(go=None), b"null"), (dict(batch=0), b"shape"), (dict(l0=3), b"plane range"),
                     (dict(nl=0), b"plane range"), (dict(l0=-1), b"plane range"),
                     (dict(g=ctypes.c_void_p(G.value + 8)), b"aligned"), (dict(gp=X), b"alias")):
        rc, msg = unpack(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)


def test_block_count_key_changes_the_workspace_only():
    """conv2_wgrad_blocks fixes the number of accumulating blocks (launch shape
    only); like conv_wgrad_blocks it is set and read but not enumerated."""
    from sfm_amd import _lib
    lib = _lib.load()
    assert _lib.tune_get("conv2_wgrad_blocks") == 0 and "conv2_wgrad_blocks" not in _lib.tune_keys()
    try:
        for nb in (1, 7, 100):
            _lib.tune("conv2_wgrad_blocks", nb)
            assert lib.sfm_conv2_wgrad_f16_workspace_bytes(2, 64, 96, 9, 67) == nb * 9 * 96 * 64 * 4
        for bad in (-1, 4097):
            with pytest.raises(_lib.SfmError):
                _lib.tune("conv2_wgrad_blocks", bad)
        assert _lib.tune_get("conv2_wgrad_blocks") == 100
        assert _lib.tune_get("conv_wgrad_blocks") == 0                 # the conv3 key is another one
    finally:
        _lib.tune("conv2_wgrad_blocks", 0)


def test_lazy_export_and_psnet_argument():
    import sfm_amd
    from sfm_amd import context
    assert "context_refine_autograd" in sfm_amd.__all__
    assert sfm_amd.context_refine_autograd is context.context_refine_autograd
    import sfm_amd.psnet as P
    feat = lambda: torch.nn.Conv2d(3, 32, 4, stride=4)
    net = P.PSNet(4, 1.0, feature_fn=feat())
    assert net.context_grad == "torch" and net.context_grad_route("cpu") == "torch"
    for bad in ("auto", "bf16", "hip", None):
        with pytest.raises(ValueError, match="context_grad"):
            P.PSNet(4, 1.0, feature_fn=feat(), context_grad=bad)
    forced = P.PSNet(4, 1.0, feature_fn=feat(), context_grad="fp16")
    assert forced.context_grad == "fp16"
    with pytest.raises(RuntimeError, match="autocast"):
        forced.context_grad_route("cpu")
    with pytest.raises(RuntimeError, match="device tensors"):
        context.context_refine_autograd(net.convs, torch.zeros(1, 32, 3, 4), torch.zeros(1, 1, 2, 3, 4))
