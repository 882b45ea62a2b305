"""CPU-side checks of the float16 training path of the 3-D regularisation
stack: the two weight packings of sfm_amd.regularize against torch's autograd
in float64, and sfm_conv3_wgrad_f16's refusals, each returned with a message
before anything is launched (no device is touched: the pointers are never
dereferenced).  The ABI version stays 1."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, D, H, W = 2, 3, 4, 5


def _case(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, D, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(B, cout, D, H, W, generator=g, dtype=torch.float64)
    F.conv3d(x, wt, padding=1).backward(gy)
    return x.detach(), wt.detach(), gy, x.grad, wt.grad


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 32), (32, 1), (64, 1)])
def test_dgrad_packing_is_autograds_grad_input(cin, cout):
    """sfm_conv3_f16 computes y[p, o] = sum Wp[tap][o][i] x[p + tap - 1, i]; as a
    Conv3d that is the weight Wp.permute(1, 2, 0) viewed [o, i, 3, 3, 3].  With
    pack_dgrad_weights' packs in that role, on the output gradient padded to 32
    channels, the halves joined: autograd's grad_input."""
    from sfm_amd.regularize import pack_dgrad_weights
    x, wt, gy, gx, _ = _case(cin, cout, 3)
    wd = pack_dgrad_weights(wt)
    assert tuple(wd.shape) == (cin // 32, 27, 32, 32) and wd.dtype == torch.float64
    gp = torch.zeros(B, 32, D, H, W, dtype=torch.float64)
    gp[:, :cout] = gy
    got = torch.cat([F.conv3d(gp, wd[k].permute(1, 2, 0).reshape(32, 32, 3, 3, 3), padding=1)
                     for k in range(cin // 32)], 1)
    assert float((got - gx).abs().max()) <= 1e-12 * float(gx.abs().max())


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 32), (32, 1), (64, 1)])
def test_wgrad_formula_unpacked_is_autograds_grad_weight(cin, cout):
    """gW[tap][co][ci] = sum over b, p of gy[b, p, co] x[b, p + tap - 1, ci] (zero
    outside the volume), evaluated tap by tap on the gradient padded to 32
    channels, then unpack_wgrad: autograd's grad_weight."""
    from sfm_amd.regularize import pack_weights, unpack_wgrad
    x, wt, gy, _, gw = _case(cin, cout, 4)
    gp = torch.zeros(B, 32, D, H, W, dtype=torch.float64)
    gp[:, :cout] = gy
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    gwp = torch.zeros(27, 32, cin, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                xs = xp[:, :, kd:kd + D, kh:kh + H, kw:kw + W]
                gwp[(kd * 3 + kh) * 3 + kw] = torch.einsum("bodhw,bidhw->oi", gp, xs)
    got = unpack_wgrad(gwp, cout, cin)
    assert tuple(got.shape) == tuple(gw.shape)
    assert float((got - gw).abs().max()) <= 1e-12 * float(gw.abs().max())
    # and the forward pack is the layout the formula is written in
    wp = pack_weights(wt)
    assert tuple(wp.shape) == (27, 32, cin) and torch.equal(unpack_wgrad(wp, cout, cin), wt)
    assert bool((wp[:, cout:] == 0).all())


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
        "sfm_conv3_wgrad_f16_workspace_bytes": ["int batch", "int cin", "int depth", "int h", "int w"],
        "sfm_conv3_wgrad_f16": [
            "const void* in", "const void* grad_out", "int batch", "int cin", "int cout", "int depth", "int h", "int w",
            "float* grad_weights", "void* workspace", "size_t workspace_bytes", "void* stream"],
    }
    for name, params in want.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        ret = "size_t" if name.endswith("_bytes") else "int"
        got, _ = _params(hdr, name, ret)
        assert got == params, name
        sig = sigs[name]
        assert sig[1] is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and len(sig[2]) == len(params), name
        for kind, p in zip(sig[2], params):
            assert (kind is ctypes.c_size_t) == p.startswith("size_t "), (name, p)
            assert (kind is ctypes.c_int) == p.startswith("int "), (name, p)
    # the declaration cites the reference lines it differentiates and tells a C caller how to get the data gradient
    _, doc = _params(hdr, "sfm_conv3_wgrad_f16_workspace_bytes", "size_t")
    assert "models/PSNet.py:79-102" in doc and "159-165" in doc
    assert "Wd[t][ci][co] = W[co][ci][26 - t]" in doc and "sfm_conv3_f16" in doc and "conv3_wgrad" in doc
    assert lib.sfm_abi_version() == 1


# distinct, 16-byte aligned stand-in pointers far enough apart that no operand overlaps another
X, G, GW, WS = (ctypes.c_void_p(a << 32) for a in (1, 2, 3, 4))
SH = dict(batch=2, cin=32, cout=32, depth=3, h=9, w=67)


def _wgrad(lib, x=X, g=G, gw=GW, ws=WS, ws_bytes=None, **kw):
    s = dict(SH, **kw)
    if ws_bytes is None:
        ws_bytes = lib.sfm_conv3_wgrad_f16_workspace_bytes(s["batch"], s["cin"] if s["cin"] in (32, 64) else 32,
                                                           max(s["depth"], 1), max(s["h"], 1), max(s["w"], 1))
    return lib.sfm_conv3_wgrad_f16(x, g, s["batch"], s["cin"], s["cout"], s["depth"], s["h"], s["w"], gw, ws, ws_bytes,
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
    rc, msg = refused(cin=48)
    assert rc == 1 and b"cin" in msg
    rc, msg = refused(cout=1)
    assert rc == 1 and b"cout" in msg and b"padded" in msg
    for k in ("batch", "depth", "h", "w"):
        rc, msg = refused(**{k: 0})
        assert rc == 1 and b"shape" in msg, k
    need = lib.sfm_conv3_wgrad_f16_workspace_bytes(2, 32, 3, 9, 67)
    tiles = 2 * 3 * 3 * 2                                    # 4-row x 64-column tiles of each plane
    assert need == tiles * 27 * 32 * 32 * 4
    assert lib.sfm_conv3_wgrad_f16_workspace_bytes(2, 64, 3, 9, 67) == 2 * need
    assert lib.sfm_conv3_wgrad_f16_workspace_bytes(2, 48, 3, 9, 67) == 0
    assert lib.sfm_conv3_wgrad_f16_workspace_bytes(0, 32, 3, 9, 67) == 0
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
    # the KITTI volume: a grid sized to the machine, not one partial per tile
    kitti = lib.sfm_conv3_wgrad_f16_workspace_bytes(1, 64, 128, 94, 311)
    assert 0 < kitti <= 2 * 512 * 27 * 32 * 32 * 4


def test_block_count_key_changes_the_workspace_only():
    """conv_wgrad_blocks fixes the number of accumulating blocks (launch shape
    only); like sweep_fused_cl it is set and read but not enumerated."""
    from sfm_amd import _lib
    lib = _lib.load()
    assert _lib.tune_get("conv_wgrad_blocks") == 0 and "conv_wgrad_blocks" not in _lib.tune_keys()
    try:
        for nb in (1, 7, 100):
            _lib.tune("conv_wgrad_blocks", nb)
            assert lib.sfm_conv3_wgrad_f16_workspace_bytes(2, 32, 3, 9, 67) == nb * 27 * 32 * 32 * 4
        for bad in (-1, 4097):
            with pytest.raises(_lib.SfmError):
                _lib.tune("conv_wgrad_blocks", bad)
        assert _lib.tune_get("conv_wgrad_blocks") == 100
    finally:
        _lib.tune("conv_wgrad_blocks", 0)


def test_lazy_export_and_psnet_argument():
    import sfm_amd
    from sfm_amd import regularize
    assert "conv3_autograd" in sfm_amd.__all__ and sfm_amd.conv3_autograd is regularize.conv3_autograd
    import sfm_amd.psnet as P
    assert isinstance(P.STACK_BWD_HIP, bool)
    net = P.PSNet(4, 1.0, feature_fn=torch.nn.Conv2d(3, 32, 4, stride=4))
    assert net.regularize_grad == "auto" and net.regularize_grad_route("cpu") == "torch"
    with pytest.raises(ValueError):
        P.PSNet(4, 1.0, feature_fn=torch.nn.Conv2d(3, 32, 4, stride=4), regularize_grad="bf16")
    forced = P.PSNet(4, 1.0, feature_fn=torch.nn.Conv2d(3, 32, 4, stride=4), regularize_grad="fp16")
    with pytest.raises(RuntimeError, match="autocast"):
        forced.regularize_grad_route("cpu")
    with pytest.raises(RuntimeError, match="device tensor"):
        net.forward_differentiable(torch.zeros(1, 64, 2, 3, 4))
