"""CPU-side checks of sfm_plane_sweep_backward and sfm_inverse_warp_backward:
the symbols are exported with the declared parameter lists, and bad arguments
are refused with a message before anything is launched (no device is touched:
the pointers are never dereferenced).  The ABI version stays 1."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V = ctypes.c_void_p(4096)          # a non-null, aligned stand-in pointer
B, C, H, W, L = 2, 32, 10, 12, 4


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
        "sfm_plane_sweep_backward_workspace_bytes": ["int batch", "int channels", "int h", "int w", "int nlabel"],
        "sfm_plane_sweep_backward": [
            "const float* grad_cost", "int warped_only", "int batch", "int channels", "int h", "int w",
            "const float* pose", "const float* K4", "const float* K4inv", "int nlabel", "float min_depth",
            "int predict_by_depth", "float* grad_ref", "float* grad_tgt", "void* workspace", "size_t workspace_bytes",
            "void* stream"],
        "sfm_inverse_warp_backward": [
            "const float* grad_out", "int batch", "int channels", "int h", "int w", "const float* depth",
            "const float* pose", "const float* K", "const float* Kinv", "float* grad_feat", "void* stream"],
    }
    for name, params in want.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        ret = "size_t" if name.endswith("_bytes") else "int"
        got, doc = _params(hdr, name, ret)
        assert got == params, name
        sig = sigs[name]
        assert sig[1] is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and len(sig[2]) == len(params), name
        for kind, p in zip(sig[2], params):
            assert (kind is ctypes.c_float) == p.startswith("float "), (name, p)
            assert (kind is ctypes.c_size_t) == p.startswith("size_t "), (name, p)
    # the declarations cite the reference lines they differentiate
    _, doc = _params(hdr, "sfm_plane_sweep_backward_workspace_bytes", "size_t")
    assert "PSNet.py:155" in doc and "inverse_warp.py:151" in doc
    _, doc = _params(hdr, "sfm_inverse_warp_backward")
    assert "inverse_warp.py:151" in doc and "PANet.py:129" in doc
    assert lib.sfm_abi_version() == 1


def _sweep(lib, g=V, warped_only=0, pose=V, K=V, Ki=V, nlabel=L, min_depth=1.0, pbd=0, grad_ref=V, grad_tgt=V, ws=V,
           ws_bytes=None, h=H):
    if ws_bytes is None:
        ws_bytes = lib.sfm_plane_sweep_backward_workspace_bytes(B, C, H, W, max(nlabel, 1))
    return lib.sfm_plane_sweep_backward(g, warped_only, B, C, h, W, pose, K, Ki, nlabel, min_depth, pbd, grad_ref,
                                        grad_tgt, ws, ws_bytes, None)


def test_sweep_backward_refuses_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def refused(**kw):
        rc = _sweep(lib, **kw)
        msg = lib.sfm_last_error()
        assert rc != 0 and msg, (kw, rc, msg)
        return rc, msg

    for name in ("g", "pose", "K", "Ki", "grad_tgt", "ws"):
        rc, msg = refused(**{name: None})
        assert rc == 1 and b"null" in msg, (name, msg)
    rc, msg = refused(nlabel=0)
    assert rc == 1 and b"shape" in msg
    refused(nlabel=-3)
    refused(h=1)
    for md in (0.0, -1.0, float("nan")):
        rc, msg = refused(min_depth=md)
        assert rc == 1 and b"min_depth" in msg, md
    for pbd in (2, -1):
        rc, msg = refused(pbd=pbd)
        assert rc == 1 and b"predict_by_depth" in msg
    refused(warped_only=2)
    rc, msg = refused(warped_only=1)                       # grad_ref given for a volume without reference rows
    assert rc == 1 and b"grad_ref" in msg
    odd = ctypes.c_void_p(4096 + 2)
    for name in ("g", "grad_ref", "grad_tgt", "pose", "K", "Ki", "ws"):
        rc, msg = refused(**{name: odd})
        assert rc == 1 and b"aligned" in msg, (name, msg)
    need = lib.sfm_plane_sweep_backward_workspace_bytes(B, C, H, W, L)
    assert need > 0 and lib.sfm_plane_sweep_backward_workspace_bytes(B, C, H, W, 0) == 0
    assert lib.sfm_plane_sweep_backward_workspace_bytes(B, C, H, W, 4096) >= 4 * 4096     # a depth per plane
    rc, msg = refused(ws_bytes=need - 1)
    assert rc == 3 and b"workspace" in msg
    refused(ws_bytes=0)


def test_inverse_warp_backward_refuses_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def call(g=V, depth=V, pose=V, K=V, Ki=V, out=V, batch=B, h=H):
        return lib.sfm_inverse_warp_backward(g, batch, C, h, W, depth, pose, K, Ki, out, None)

    for name in ("g", "depth", "pose", "K", "Ki", "out"):
        assert call(**{name: None}) == 1 and b"null" in lib.sfm_last_error(), name
    assert call(batch=0) == 1 and b"shape" in lib.sfm_last_error()
    assert call(h=1) == 1
    for name in ("g", "depth", "pose", "K", "Ki", "out"):
        for off in (1, 2):
            assert call(**{name: ctypes.c_void_p(4096 + off)}) == 1 and b"aligned" in lib.sfm_last_error(), name