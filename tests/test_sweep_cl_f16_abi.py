"""CPU-side checks of sfm_plane_sweep_cl_f16 (the channels-last plane sweep
that reads float16 features as they come): the symbol is exported with the
declared signature, every bad argument is refused with sfm_plane_sweep_cl's
code and message before anything is launched (no device is touched: the
pointers are never dereferenced), it needs no workspace query of its own, and
the routing switch sweep_f16_feat behaves like sweep_fused_cl."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V = ctypes.c_void_p(4096)          # a non-null, 16-byte aligned stand-in pointer
B, C, H, W, L = 1, 32, 10, 12, 4


def _call(lib, fn="sfm_plane_sweep_cl_f16", ref=V, tgt=V, pose=V, K4=V, K4inv=V, out=V, ws=V, ws_bytes=None,
          batch=B, channels=C, h=H, w=W, nlabel=L, out_dtype=2, min_depth=1.0, pbd=0):
    if ws_bytes is None:
        ws_bytes = lib.sfm_plane_sweep_workspace_bytes(B, C, H, W)
    return getattr(lib, fn)(ref, tgt, batch, channels, h, w, pose, K4, K4inv, nlabel, min_depth, pbd, out_dtype, out,
                            ws, ws_bytes, None)


def test_exported_with_declared_signature():
    from sfm_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "sfm_plane_sweep_cl_f16") and "sfm_plane_sweep_cl_f16" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    m = re.search(r"int\s+sfm_plane_sweep_cl_f16\s*\(([^;]*)\)\s*;", hdr)
    assert m, "sfm_plane_sweep_cl_f16 is not declared in sfm_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    want = ["const void* ref", "const void* tgt", "int batch", "int channels", "int h", "int w",
            "const float* pose", "const float* K4", "const float* K4inv", "int nlabel", "float min_depth",
            "int predict_by_depth", "int out_dtype", "void* out", "void* workspace", "size_t workspace_bytes",
            "void* stream"]
    assert [" ".join(p.split()) for p in params] == want
    # the binding's ctypes table: the arity and kinds of sfm_plane_sweep_cl's entry
    sigs = dict((s[0], s) for s in _lib._SIGS)
    sig = sigs["sfm_plane_sweep_cl_f16"]
    assert sig[1] is ctypes.c_int and len(sig[2]) == len(want)
    assert list(sig[2]) == list(sigs["sfm_plane_sweep_cl"][2])
    assert sig[2][10] is ctypes.c_float and sig[2][15] is ctypes.c_size_t
    # the declaration states the contract, the fast-path condition and the workspace query it shares
    doc = " ".join(hdr[:m.start()].rsplit("/*", 1)[1].replace("*", " ").split())
    assert "bit for bit" in doc and "finite or infinite" in doc and "multiple of 8" in doc
    assert "sfm_plane_sweep_workspace_bytes" in doc and "no query of its own" in doc
    # additive: the ABI version stays
    assert lib.sfm_abi_version() == 1
    assert re.search(r"#define\s+SFM_ABI_VERSION\s+1\b", hdr)


def test_bad_arguments_are_refused_like_the_float32_entry():
    """Every argument check: the code and the message of sfm_plane_sweep_cl for
    the same bad argument."""
    from sfm_amd import _lib
    lib = _lib.load()

    def refused(**kw):
        rc = _call(lib, **kw)
        msg = lib.sfm_last_error()
        assert rc != 0 and msg, (kw, rc, msg)
        rc32 = _call(lib, fn="sfm_plane_sweep_cl", **kw)
        assert (rc, msg) == (rc32, lib.sfm_last_error()), (kw, rc, msg, rc32, lib.sfm_last_error())
        return rc, msg

    for name in ("ref", "tgt", "pose", "K4", "K4inv", "out", "ws"):
        rc, msg = refused(**{name: None})
        assert rc == 1 and b"null" in msg, (name, msg)
    for kw in (dict(batch=0), dict(batch=65536), dict(channels=0), dict(channels=4 * 65535 + 1), dict(h=1), dict(w=1),
               dict(h=1 << 23), dict(nlabel=0)):
        rc, msg = refused(**kw)
        assert rc == 1 and b"shape" in msg, (kw, msg)
    for bad in (3, -1):
        rc, msg = refused(out_dtype=bad)
        assert rc == 1 and b"out_dtype" in msg
    rc, msg = refused(pbd=2)
    assert rc == 1 and b"predict_by_depth" in msg
    for bad in (0.0, -1.0):
        rc, msg = refused(min_depth=bad)
        assert rc == 1 and b"min_depth" in msg
    rc, msg = refused(h=1 << 15, w=1 << 15)
    assert rc == 1 and b"too large" in msg
    rc, msg = refused(h=1 << 10, w=1 << 10, nlabel=1 << 11)           # nlabel * h * w = 2^31
    assert rc == 1 and b"2^31" in msg
    rc, msg = refused(out=ctypes.c_void_p(4096 + 8))
    assert rc == 1 and b"aligned" in msg


def test_workspace_too_small_names_the_shared_query():
    from sfm_amd import _lib
    lib = _lib.load()
    need = lib.sfm_plane_sweep_workspace_bytes(B, C, H, W)
    assert need > 0
    rc = _call(lib, ws_bytes=need - 1)
    msg = lib.sfm_last_error()
    assert rc == 3 and b"workspace" in msg and str(need).encode() in msg, (rc, msg)
    assert _call(lib, ws_bytes=0) == 3
    # a channel count that is no multiple of 8 (the last octet half padding): the same query
    need6 = lib.sfm_plane_sweep_workspace_bytes(B, 6, H, W)
    rc = _call(lib, channels=6, ws_bytes=need6 - 1)
    assert rc == 3 and str(need6).encode() in lib.sfm_last_error()


def test_f16_feature_switch():
    from sfm_amd import _lib
    v = ctypes.c_int(-1)
    assert _lib.load().sfm_tune_get(b"sweep_f16_feat", ctypes.byref(v)) == 0 and v.value in (0, 1)
    old = _lib.tune_get("sweep_f16_feat")
    assert old == v.value
    try:
        for x in (0, 1):
            _lib.tune("sweep_f16_feat", x)
            assert _lib.tune_get("sweep_f16_feat") == x
        assert _lib.load().sfm_tune_set(b"sweep_f16_feat", 2) != 0
        assert _lib.load().sfm_tune_set(b"sweep_f16_feat", -1) != 0
        assert _lib.tune_get("sweep_f16_feat") == 1
    finally:
        _lib.tune("sweep_f16_feat", old)
    # a switch, not a launch-shape knob: sfm_tune_key does not enumerate it, and the enumerated set is the
    # launch-shape and scoring knobs (32 since conv_planes)
    assert "sweep_f16_feat" not in _lib.tune_keys() and len(_lib.tune_keys()) == 32
