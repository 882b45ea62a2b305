"""CPU-side checks of sfm_plane_sweep_cl (the channels-last plane sweep): the
symbol is exported with the declared signature, bad arguments are refused
with a message before anything is launched (no device is touched: the
pointers are never dereferenced), and the routing switch defaults to on."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V = ctypes.c_void_p(4096)          # a non-null, 16-byte aligned stand-in pointer
B, C, H, W, L = 1, 32, 10, 12, 4


def _call(lib, ref=V, tgt=V, out=V, ws=V, ws_bytes=None, nlabel=L, out_dtype=2, min_depth=1.0, pbd=0):
    if ws_bytes is None:
        ws_bytes = lib.sfm_plane_sweep_workspace_bytes(B, C, H, W)
    return lib.sfm_plane_sweep_cl(ref, tgt, B, C, H, W, V, V, V, nlabel, min_depth, pbd, out_dtype, out, ws, ws_bytes,
                                  None)


def test_exported_with_declared_signature():
    from sfm_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "sfm_plane_sweep_cl") and "sfm_plane_sweep_cl" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    m = re.search(r"int\s+sfm_plane_sweep_cl\s*\(([^;]*)\)\s*;", hdr)
    assert m, "sfm_plane_sweep_cl is not declared in sfm_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    want = ["const float* ref", "const float* tgt", "int batch", "int channels", "int h", "int w",
            "const float* pose", "const float* K4", "const float* K4inv", "int nlabel", "float min_depth",
            "int predict_by_depth", "int out_dtype", "void* out", "void* workspace", "size_t workspace_bytes",
            "void* stream"]
    assert [" ".join(p.split()) for p in params] == want
    # the binding's ctypes table has the same arity and kinds
    sig = dict((s[0], s) for s in _lib._SIGS)["sfm_plane_sweep_cl"]
    assert sig[1] is ctypes.c_int and len(sig[2]) == len(want)
    assert sig[2][10] is ctypes.c_float and sig[2][15] is ctypes.c_size_t
    # the declaration cites the loop it replaces and its consumer
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    assert "PSNet.py:144-157" in doc and "159" in doc
    assert lib.sfm_abi_version() == 1


def test_bad_arguments_are_refused_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def refused(**kw):
        rc = _call(lib, **kw)
        msg = lib.sfm_last_error()
        assert rc != 0 and msg, (kw, rc, msg)
        return rc, msg

    for name in ("ref", "tgt", "out", "ws"):
        rc, msg = refused(**{name: None})
        assert b"null" in msg, (name, msg)
    rc, msg = refused(out_dtype=3)
    assert rc == 1 and b"out_dtype" in msg
    refused(out_dtype=-1)
    rc, msg = refused(nlabel=0)
    assert rc == 1
    need = lib.sfm_plane_sweep_workspace_bytes(B, C, H, W)
    assert need > 0
    rc, msg = refused(ws_bytes=need - 1)
    assert rc == 3 and b"workspace" in msg
    rc, msg = refused(out=ctypes.c_void_p(4096 + 8))
    assert rc == 1 and b"aligned" in msg
    refused(min_depth=0.0)
    refused(pbd=2)


def test_fused_route_switch_defaults_on():
    from sfm_amd import _lib
    v = ctypes.c_int(-1)
    assert _lib.load().sfm_tune_get(b"sweep_fused_cl", ctypes.byref(v)) == 0 and v.value == 1
    assert _lib.tune_get("sweep_fused_cl") == 1
    try:
        _lib.tune("sweep_fused_cl", 0)
        assert _lib.tune_get("sweep_fused_cl") == 0
        assert _lib.load().sfm_tune_set(b"sweep_fused_cl", 2) != 0
        assert _lib.tune_get("sweep_fused_cl") == 0
    finally:
        _lib.tune("sweep_fused_cl", 1)
    # a switch, not a launch-shape knob: sfm_tune_key does not enumerate it
    assert "sweep_fused_cl" not in _lib.tune_keys()
