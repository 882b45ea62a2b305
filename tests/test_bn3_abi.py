"""CPU-side checks of the float16 BatchNorm3d / ReLU / residual entries
(csrc/bn3.hip): the declarations and exports, every refusal with its message
before anything is launched (no device is touched: the pointers are never
dereferenced), the bn_blocks key, and bn3_act_reference against torch's own
modules in float64.  The ABI version stays 1."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(hdr, name, ret="int"):
    m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in sfm_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    return [" ".join(p.split()) for p in params], hdr[:m.start()].rsplit("/*", 1)[1]


WANT = {
    "sfm_bn3_stats_f16_workspace_bytes": ["int64_t voxels", "int training"],
    "sfm_bn3_stats_f16": [
        "const void* x", "int64_t voxels", "const float* gamma", "const float* beta", "double eps",
        "float* running_mean", "float* running_var", "double momentum", "int training", "float* stats",
        "void* workspace", "size_t workspace_bytes", "void* stream"],
    "sfm_bn3_apply_f16": ["const void* x", "int64_t voxels", "const float* stats", "const void* residual", "int relu",
                          "void* out", "void* stream"],
    "sfm_bn3_backward_f16_workspace_bytes": ["int64_t voxels"],
    "sfm_bn3_backward_f16": [
        "const void* x", "const void* grad_out", "int64_t voxels", "const float* stats", "int relu", "int training",
        "void* grad_x", "float* grad_gamma_beta", "void* workspace", "size_t workspace_bytes", "void* stream"],
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
        assert "models/submodule.py:17-20" in doc and "models/PSNet.py:79-102" in doc and "159-165" in doc, name
    assert lib.sfm_abi_version() == 1


# distinct, 16-byte aligned stand-in pointers far enough apart that no operand overlaps another
X, G, RES, OUT, GX, WS, GAM, BET, RM, RV, ST, GGB = (ctypes.c_void_p(a << 36) for a in range(1, 13))
VOX = 1000


def _stats(lib, x=X, voxels=VOX, gamma=GAM, beta=BET, eps=1e-5, rm=RM, rv=RV, momentum=0.1, training=1, stats=ST,
           ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sfm_bn3_stats_f16_workspace_bytes(max(voxels, 1), 1)
    return lib.sfm_bn3_stats_f16(x, voxels, gamma, beta, eps, rm, rv, momentum, training, stats, ws, ws_bytes, None)


def _apply(lib, x=X, voxels=VOX, stats=ST, res=RES, relu=1, out=OUT):
    return lib.sfm_bn3_apply_f16(x, voxels, stats, res, relu, out, None)


def _bwd(lib, x=X, g=G, voxels=VOX, stats=ST, relu=1, training=1, gx=GX, ggb=GGB, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sfm_bn3_backward_f16_workspace_bytes(max(voxels, 1))
    return lib.sfm_bn3_backward_f16(x, g, voxels, stats, relu, training, gx, ggb, ws, ws_bytes, None)


def _off(p, n):
    return ctypes.c_void_p(p.value + n)


def test_every_refusal_comes_with_its_message():
    from sfm_amd import _lib
    lib = _lib.load()

    def refused(fn, code=1, **kw):
        rc = fn(lib, **kw)
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
            assert b"voxel" in refused(fn, voxels=v), (fn.__name__, v)
    # torch refuses one value per channel in training mode; eval mode takes it (the call would launch: not made here)
    assert b"more than one value per channel" in refused(_stats, voxels=1)
    assert b"more than one value per channel" in refused(_bwd, voxels=1)
    assert b"eps" in refused(_stats, eps=-1.0) and b"momentum" in refused(_stats, momentum=1.5)
    # alignment
    for fn, names in ((_stats, dict(x=X, gamma=GAM, beta=BET, rm=RM, rv=RV, stats=ST, ws=WS)),
                      (_apply, dict(x=X, stats=ST, res=RES, out=OUT)),
                      (_bwd, dict(x=X, g=G, stats=ST, gx=GX, ggb=GGB, ws=WS))):
        for n, p in names.items():
            for off in (2, 8):
                assert b"aligned" in refused(fn, **{n: _off(p, off)}), (fn.__name__, n, off)
    # workspace
    need = lib.sfm_bn3_stats_f16_workspace_bytes(VOX, 1)
    assert need == 8 * 64 * 8                                  # ceil(1000 / 128) blocks, one [2][32] double partial each
    assert lib.sfm_bn3_backward_f16_workspace_bytes(VOX) == need
    assert lib.sfm_bn3_stats_f16_workspace_bytes(VOX, 0) == 0 and lib.sfm_bn3_stats_f16_workspace_bytes(0, 1) == 0
    assert lib.sfm_bn3_backward_f16_workspace_bytes(0) == 0
    for fn in (_stats, _bwd):
        msg = refused(fn, code=3, ws_bytes=need - 1)
        assert b"workspace" in msg and str(need).encode() in msg
        assert b"workspace" in refused(fn, code=3, ws=None)
    # the KITTI volume at batch 8: a grid sized to the machine
    assert lib.sfm_bn3_stats_f16_workspace_bytes(8 * 128 * 94 * 311, 1) == 512 * 64 * 8
    # outputs aliasing inputs (or each other)
    xb = VOX * 64
    for kw in (dict(stats=X), dict(stats=_off(X, xb - 16)), dict(stats=GAM), dict(stats=BET), dict(stats=RM),
               dict(stats=RV), dict(stats=WS), dict(ws=X), dict(ws=GAM), dict(rm=X), dict(rv=_off(X, 64)),
               dict(rm=RV), dict(rm=GAM), dict(rv=BET)):
        assert b"alias" in refused(_stats, **kw), kw
    for kw in (dict(out=X), dict(out=_off(X, xb - 16)), dict(out=RES), dict(out=ST), dict(out=_off(ST, -64))):
        assert b"alias" in refused(_apply, **kw), kw
    for kw in (dict(gx=X), dict(gx=G), dict(gx=ST), dict(gx=GGB), dict(gx=WS), dict(ggb=X), dict(ggb=_off(G, 128)),
               dict(ggb=ST), dict(ggb=WS), dict(ws=X), dict(ws=G), dict(ws=ST)):
        assert b"alias" in refused(_bwd, **kw), kw


def test_bn_blocks_key():
    """bn_blocks fixes the number of reducing blocks (launch shape only); like
    conv_wgrad_blocks it is set and read but not enumerated."""
    from sfm_amd import _lib
    lib = _lib.load()
    assert _lib.tune_get("bn_blocks") == 0
    assert "bn_blocks" not in _lib.tune_keys() and len(_lib.tune_keys()) == 32
    try:
        for nb in (1, 7, 4096):
            _lib.tune("bn_blocks", nb)
            assert _lib.tune_get("bn_blocks") == nb
            assert lib.sfm_bn3_stats_f16_workspace_bytes(VOX, 1) == nb * 64 * 8
            assert lib.sfm_bn3_backward_f16_workspace_bytes(VOX) == nb * 64 * 8
        for bad in (-1, 4097):
            with pytest.raises(_lib.SfmError):
                _lib.tune("bn_blocks", bad)
        assert _lib.tune_get("bn_blocks") == 4096
    finally:
        _lib.tune("bn_blocks", 0)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu,resid", [(True, False), (False, True), (True, True), (False, False)])
def test_reference_is_the_modules_in_float64(training, relu, resid):
    """bn3_act_reference against autograd of BatchNorm3d -> ReLU -> + residual in
    float64: output, the four gradients and the running statistics after two
    steps."""
    from sfm_amd.regularize import bn3_act_reference
    g = torch.Generator().manual_seed(11)
    B, L, h, w, C = 2, 3, 4, 5, 32
    bn = torch.nn.BatchNorm3d(C, eps=1e-3, momentum=0.3).double().train(training)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_var.copy_(1.0 + torch.rand(C, generator=g, dtype=torch.float64))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    for step in range(2):
        x = (0.5 + 2.0 * torch.randn(B, L, h, w, C, generator=g, dtype=torch.float64)).requires_grad_()
        res = torch.randn(B, L, h, w, C, generator=g, dtype=torch.float64).requires_grad_()
        gout = torch.randn(B, L, h, w, C, generator=g, dtype=torch.float64)
        y = bn(x.permute(0, 4, 1, 2, 3))
        y = torch.relu(y) if relu else y
        y = y.permute(0, 2, 3, 4, 1)
        y = y + res if resid else y
        y.backward(gout)
        want = (y.detach(), x.grad, bn.weight.grad.clone(), bn.bias.grad.clone(), res.grad)
        bn.weight.grad = bn.bias.grad = None
        x2, res2 = x.detach().clone().requires_grad_(), res.detach().clone().requires_grad_()
        gam, bet = bn.weight.detach().clone().requires_grad_(), bn.bias.detach().clone().requires_grad_()
        out, rm, rv = bn3_act_reference(x2, gam, bet, rm, rv, training, 0.3, 1e-3, relu, res2 if resid else None)
        out.backward(gout)
        assert out.dtype == torch.float64 and rel(out.detach(), want[0]) <= 1e-12
        assert rel(x2.grad, want[1]) <= 1e-12 and rel(gam.grad, want[2]) <= 1e-12 and rel(bet.grad, want[3]) <= 1e-12
        if resid:
            assert rel(res2.grad, want[4]) <= 1e-12
        else:
            assert res2.grad is None and want[4] is None
        assert rel(rm, bn.running_mean) <= 1e-12 and rel(rv, bn.running_var) <= 1e-12
    if not training:
        assert torch.equal(rm, bn.running_mean) and int(bn.num_batches_tracked) == 0


def test_export_and_arguments():
    import sfm_amd
    from sfm_amd import regularize
    assert "batchnorm3_act_autograd" in sfm_amd.__all__
    assert sfm_amd.batchnorm3_act_autograd is regularize.batchnorm3_act_autograd
    bn = torch.nn.BatchNorm3d(32)
    with pytest.raises(RuntimeError, match="device tensor"):
        regularize.batchnorm3_act_autograd(torch.zeros(1, 2, 3, 4, 32, dtype=torch.float16), bn)
    reg = regularize.CostRegularization(64)
    with pytest.raises(ValueError, match="norm"):
        reg.forward_differentiable(torch.zeros(1, 64, 2, 3, 4), norm="fused")
    import sfm_amd.psnet as P
    net = P.PSNet(4, 1.0, feature_fn=torch.nn.Conv2d(3, 32, 4, stride=4))
    assert net.regularize_norm == "torch"
    assert P.PSNet(4, 1.0, feature_fn=torch.nn.Conv2d(3, 32, 4, stride=4), regularize_norm="hip").regularize_norm == "hip"
    with pytest.raises(ValueError):
        P.PSNet(4, 1.0, feature_fn=torch.nn.Conv2d(3, 32, 4, stride=4), regularize_norm="fp16")
