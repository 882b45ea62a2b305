"""CPU-side checks of the float16 BatchNorm2d / ReLU / residual entries
(csrc/bn2.hip): the declarations and exports, every refusal with its message
before anything is launched (no device is touched: the pointers are never
dereferenced), the channels refusal, the workspace sizes per channel count
following bn_blocks, and the Python-side refusals of the wrappers and of the
autograd ops.  The ABI version stays 1."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (32, 64, 128)


def _params(hdr, name, ret="int"):
    m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in sfm_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    return [" ".join(p.split()) for p in params], hdr[:m.start()].rsplit("/*", 1)[1]


WANT = {
    "sfm_bn2_stats_f16_workspace_bytes": ["int64_t pixels", "int channels", "int training"],
    "sfm_bn2_stats_f16": [
        "const void* x", "int64_t pixels", "int channels", "const float* gamma", "const float* beta", "double eps",
        "float* running_mean", "float* running_var", "double momentum", "int training", "float* stats",
        "void* workspace", "size_t workspace_bytes", "void* stream"],
    "sfm_bn2_apply_f16": ["const void* x", "int64_t pixels", "int channels", "const float* stats",
                          "const void* residual", "int relu", "void* out", "void* stream"],
    "sfm_bn2_backward_f16_workspace_bytes": ["int64_t pixels", "int channels"],
    "sfm_bn2_backward_f16": [
        "const void* x", "const void* grad_out", "int64_t pixels", "int channels", "const float* stats", "int relu",
        "int training", "void* grad_x", "float* grad_gamma_beta", "void* workspace", "size_t workspace_bytes",
        "void* stream"],
}
KIND = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def test_exported_with_declared_signatures():
    from sfm_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    sigs = dict((s[0], s) for s in _lib._SIGS)
    for name, params in WANT.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        ret = "size_t" if name.endswith("_bytes") else "int"
        got, doc = _params(hdr, name, ret)
        assert got == params, name
        sig = sigs[name]
        assert sig[1] is KIND[ret] and len(sig[2]) == len(params), name
        for kind, p in zip(sig[2], params):
            want = KIND.get(p.split()[0], ctypes.c_void_p)
            assert kind is want, (name, p)
        # each entry's comment cites the reference lines it replaces
        assert "models/submodule.py:11-14" in doc and "models/submodule.py:22-44" in doc, name
    assert lib.sfm_abi_version() == 1
    # entry points only: the kernels are the shared definition, not a second copy
    src = open(os.path.join(ROOT, "deep-sfm-revisited_amd", "csrc", "bn2.hip")).read()
    assert "__global__" not in src and '#include "bn_act.h"' in src
    src3 = open(os.path.join(ROOT, "deep-sfm-revisited_amd", "csrc", "bn3.hip")).read()
    assert "__global__" not in src3 and '#include "bn_act.h"' in src3


# distinct, 16-byte aligned stand-in pointers far enough apart that no operand overlaps another
X, G, RES, OUT, GX, WS, GAM, BET, RM, RV, ST, GGB = (ctypes.c_void_p(a << 36) for a in range(1, 13))
PIX = 1000


def _stats(lib, C=64, x=X, pixels=PIX, gamma=GAM, beta=BET, eps=1e-5, rm=RM, rv=RV, momentum=0.1, training=1,
           stats=ST, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sfm_bn2_stats_f16_workspace_bytes(max(pixels, 1), C, 1)
    return lib.sfm_bn2_stats_f16(x, pixels, C, gamma, beta, eps, rm, rv, momentum, training, stats, ws, ws_bytes, None)


def _apply(lib, C=64, x=X, pixels=PIX, stats=ST, res=RES, relu=1, out=OUT):
    return lib.sfm_bn2_apply_f16(x, pixels, C, stats, res, relu, out, None)


def _bwd(lib, C=64, x=X, g=G, pixels=PIX, stats=ST, relu=1, training=1, gx=GX, ggb=GGB, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sfm_bn2_backward_f16_workspace_bytes(max(pixels, 1), C)
    return lib.sfm_bn2_backward_f16(x, g, pixels, C, stats, relu, training, gx, ggb, ws, ws_bytes, None)


def _off(p, n):
    return ctypes.c_void_p(p.value + n)


@pytest.mark.parametrize("C", CHANNELS)
def test_every_refusal_comes_with_its_message(C):
    from sfm_amd import _lib
    lib = _lib.load()

    def refused(fn, code=1, **kw):
        rc = fn(lib, C, **kw)
        msg = lib.sfm_last_error()
        assert rc == code and msg, (fn.__name__, kw, rc, msg)
        return msg

    # null pointers
    for fn, names in ((_stats, ("x", "gamma", "beta", "stats")), (_apply, ("x", "stats", "out")),
                      (_bwd, ("x", "g", "stats", "ggb"))):
        for n in names:
            assert b"null" in refused(fn, **{n: None}), (fn.__name__, n)
    assert b"null" in refused(_stats, training=0, rm=None) and b"running" in lib.sfm_last_error()
    assert b"null" in refused(_stats, training=0, rv=None)
    # flags and counts
    assert b"training" in refused(_stats, training=2)
    assert b"relu" in refused(_apply, relu=2)
    assert b"relu" in refused(_bwd, relu=-1) and b"training" in refused(_bwd, training=3)
    for fn in (_stats, _apply, _bwd):
        for v in (0, -5, (1 << 40) + 1):
            assert b"pixel" in refused(fn, pixels=v), (fn.__name__, v)
    # torch refuses one value per channel in training mode; eval mode takes it (the call would launch: not made here)
    assert b"more than one value per channel" in refused(_stats, pixels=1) and b"pixels >= 2" in lib.sfm_last_error()
    assert b"more than one value per channel" in refused(_bwd, pixels=1)
    assert b"eps" in refused(_stats, eps=-1.0) and b"momentum" in refused(_stats, momentum=1.5)
    # alignment
    for fn, names in ((_stats, dict(x=X, gamma=GAM, beta=BET, rm=RM, rv=RV, stats=ST, ws=WS)),
                      (_apply, dict(x=X, stats=ST, res=RES, out=OUT)),
                      (_bwd, dict(x=X, g=G, stats=ST, gx=GX, ggb=GGB, ws=WS))):
        for n, p in names.items():
            for off in (2, 8):
                assert b"aligned" in refused(fn, **{n: _off(p, off)}), (fn.__name__, n, off)
    # workspace: ceil(1000 / (4096 / C)) blocks, one [2][C] double partial each
    blocks = -(-PIX // (4096 // C))
    need = lib.sfm_bn2_stats_f16_workspace_bytes(PIX, C, 1)
    assert need == blocks * 2 * C * 8
    assert lib.sfm_bn2_backward_f16_workspace_bytes(PIX, C) == need
    assert lib.sfm_bn2_stats_f16_workspace_bytes(PIX, C, 0) == 0 and lib.sfm_bn2_stats_f16_workspace_bytes(0, C, 1) == 0
    assert lib.sfm_bn2_backward_f16_workspace_bytes(0, C) == 0
    for fn in (_stats, _bwd):
        msg = refused(fn, code=3, ws_bytes=need - 1)
        assert b"workspace" in msg and str(need).encode() in msg
        assert b"workspace" in refused(fn, code=3, ws=None)
    # the CNN's half-resolution map at batch 2: a grid sized to the machine
    assert lib.sfm_bn2_stats_f16_workspace_bytes(2 * 188 * 621, C, 1) == 512 * 2 * C * 8
    # outputs aliasing inputs (or each other)
    xb = PIX * 2 * C
    for kw in (dict(stats=X), dict(stats=_off(X, xb - 16)), dict(stats=GAM), dict(stats=BET), dict(stats=RM),
               dict(stats=RV), dict(stats=WS), dict(ws=X), dict(ws=GAM), dict(rm=X), dict(rv=_off(X, 2 * C)),
               dict(rm=RV), dict(rm=GAM), dict(rv=BET), dict(stats=_off(GAM, 4 * C - 16))):
        assert b"alias" in refused(_stats, **kw), kw
    for kw in (dict(out=X), dict(out=_off(X, xb - 16)), dict(out=RES), dict(out=ST), dict(out=_off(ST, -2 * C)),
               dict(out=_off(ST, 20 * C - 16))):
        assert b"alias" in refused(_apply, **kw), kw
    for kw in (dict(gx=X), dict(gx=G), dict(gx=ST), dict(gx=GGB), dict(gx=WS), dict(ggb=X), dict(ggb=_off(G, 4 * C)),
               dict(ggb=ST), dict(ggb=WS), dict(ws=X), dict(ws=G), dict(ws=ST), dict(gx=_off(GGB, 8 * C - 16))):
        assert b"alias" in refused(_bwd, **kw), kw


def test_channels_refusal():
    """Any channel count but 32, 64 and 128 is refused, before anything else is
    looked at (every other argument is null here), and has no workspace."""
    from sfm_amd import _lib
    lib = _lib.load()
    for c in (0, -32, 8, 16, 31, 33, 48, 96, 127, 256, 320):
        for rc in (lib.sfm_bn2_stats_f16(None, 0, c, None, None, -1.0, None, None, 2.0, 7, None, None, 0, None),
                   lib.sfm_bn2_apply_f16(None, 0, c, None, None, 7, None, None),
                   lib.sfm_bn2_backward_f16(None, None, 0, c, None, 7, 7, None, None, None, 0, None)):
            assert rc == 1 and lib.sfm_last_error() == b"channels must be 32, 64 or 128", (c, lib.sfm_last_error())
        assert lib.sfm_bn2_stats_f16_workspace_bytes(PIX, c, 1) == 0
        assert lib.sfm_bn2_backward_f16_workspace_bytes(PIX, c) == 0


def test_workspace_follows_bn_blocks():
    """bn_blocks fixes the number of reducing blocks of these entries too; it is
    still not enumerated: no tuning key was added."""
    from sfm_amd import _lib
    lib = _lib.load()
    assert _lib.tune_get("bn_blocks") == 0
    assert "bn_blocks" not in _lib.tune_keys() and len(_lib.tune_keys()) == 32
    try:
        for nb in (1, 7, 4096):
            _lib.tune("bn_blocks", nb)
            for C in CHANNELS:
                assert lib.sfm_bn2_stats_f16_workspace_bytes(PIX, C, 1) == nb * 2 * C * 8
                assert lib.sfm_bn2_backward_f16_workspace_bytes(PIX, C) == nb * 2 * C * 8
                msg_rc = _stats(lib, C, ws_bytes=nb * 2 * C * 8 - 1)
                assert msg_rc == 3 and str(nb * 2 * C * 8).encode() in lib.sfm_last_error()
    finally:
        _lib.tune("bn_blocks", 0)
    # the default: one block per load step of 4096 / C pixels, at most 512
    for C in CHANNELS:
        rows = 4096 // C
        for pix, blocks in ((2, 1), (rows, 1), (rows + 1, 2), (511 * rows + 1, 512), (10 ** 7, 512)):
            assert lib.sfm_bn2_backward_f16_workspace_bytes(pix, C) == blocks * 2 * C * 8, (C, pix)


def test_python_side_refusals():
    """The wrappers and the autograd ops refuse CPU tensors, wrong layouts and
    modules that are not the stock ones before anything reaches the library."""
    import sfm_amd
    from sfm_amd import feature
    for name in ("batchnorm2_act_autograd", "convbn2_autograd", "basic_block_autograd"):
        assert name in sfm_amd.__all__ and getattr(sfm_amd, name) is getattr(feature, name), name
    x = torch.zeros(2, 3, 4, 64, dtype=torch.float16)
    st = torch.zeros(5, 64)
    one = torch.ones(64)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.bn2_stats_f16(x, one, one)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.bn2_apply_f16(x, st)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.bn2_backward_f16(x, x, st)
    bn = nn.BatchNorm2d(64)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.batchnorm2_act_autograd(x, bn)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.batchnorm2_act_autograd(x.float(), bn)
    # layer checks come before the tensor is looked at: they go through _conv_bn / _check_layer
    from sfm_amd.psnet import _Residual, _conv_bn
    good = _conv_bn(32, 64, 3, 2, 1, 1)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.convbn2_autograd(torch.zeros(2, 5, 6, 32, dtype=torch.float16), good)
    with pytest.raises(feature.FeatureLayoutError, match="bias"):
        feature.convbn2_autograd(x, nn.Sequential(nn.Conv2d(64, 64, 3, padding=1), nn.BatchNorm2d(64)))
    with pytest.raises(feature.FeatureLayoutError, match="padding"):
        feature.convbn2_autograd(x, nn.Sequential(nn.Conv2d(64, 64, 3, padding=0, bias=False), nn.BatchNorm2d(64)))
    with pytest.raises(RuntimeError, match="ksize"):
        feature.convbn2_autograd(x, nn.Sequential(nn.Conv2d(64, 64, 5, padding=2, bias=False), nn.BatchNorm2d(64)))
    with pytest.raises(feature.FeatureLayoutError, match="32, 64 or 128"):
        feature.convbn2_autograd(x, nn.Sequential(nn.Conv2d(64, 96, 3, padding=1, bias=False), nn.BatchNorm2d(96)))
    with pytest.raises(feature.FeatureLayoutError, match="Conv2d \\+ BatchNorm2d"):
        feature.convbn2_autograd(x, nn.Conv2d(64, 64, 3, padding=1, bias=False))
    with pytest.raises(feature.FeatureLayoutError, match="running statistics"):
        feature.convbn2_autograd(x, nn.Sequential(nn.Conv2d(64, 64, 3, padding=1, bias=False),
                                                  nn.BatchNorm2d(64, track_running_stats=False)))
    blk = _Residual(32, 64, 2, 1, 1)
    with pytest.raises(RuntimeError, match="device tensor"):
        feature.basic_block_autograd(blk, torch.zeros(2, 5, 6, 32, dtype=torch.float16))
    with pytest.raises(feature.FeatureLayoutError, match="conv1"):
        feature.basic_block_autograd(nn.Conv2d(32, 32, 3), x)
    blk.downsample = None
    with pytest.raises(feature.FeatureLayoutError, match="downsample"):
        feature.basic_block_autograd(blk, x)
    blk = _Residual(32, 32, 1, 1, 1)
    blk.downsample = _conv_bn(32, 32, 3, 1, 1, 1)
    with pytest.raises(feature.FeatureLayoutError, match="1 x 1"):
        feature.basic_block_autograd(blk, x)
