"""CPU-side checks of sfm_depth_head_backward and sfm_depth_head_contributors:
bad arguments are refused with a message before anything is launched (no device
is touched: the pointers are never dereferenced), and the contributor runs the
backward's gather walks are the exact transpose of the forward's source-index
map (a Python restatement of csrc/depth_head.h's axis_weights applied to every
output index).  The ABI version stays 1."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V = ctypes.c_void_p(4096)          # a non-null, aligned stand-in pointer
B, L, h, w, H, W = 2, 5, 6, 7, 18, 27


def _call(lib, cost=V, grad_depth=V, batch=B, nlabel=L, mode=0, min_depth=1.0, step=0.0, grad_cost=ctypes.c_void_p(8192),
          ws=V, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sfm_depth_head_backward_workspace_bytes(B, H, W)
    return lib.sfm_depth_head_backward(cost, grad_depth, batch, nlabel, h, w, H, W, mode, min_depth, step, grad_cost, ws,
                                       ws_bytes, None)


def test_backward_refuses_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    m = re.search(r"size_t\s+sfm_depth_head_backward_workspace_bytes\s*\(", hdr)
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    assert "PSNet.py:194-216" in doc and "submodule.py:57-93" in doc       # the reference lines it differentiates
    assert lib.sfm_abi_version() == 1

    def refused(**kw):
        rc = _call(lib, **kw)
        msg = lib.sfm_last_error()
        assert rc != 0 and msg, (kw, rc, msg)
        return rc, msg

    for name in ("cost", "grad_depth", "grad_cost"):
        rc, msg = refused(**{name: None})
        assert rc == 1 and b"null" in msg, (name, msg)
    for mode in (2, -1, 5):
        rc, msg = refused(mode=mode, step=1.0)
        assert rc == 1 and b"depth_mode" in msg, mode
    for step in (0.0, -1.0):
        rc, msg = refused(mode=1, step=step)
        assert rc == 1 and b"step" in msg, step
    rc, msg = refused(batch=0)
    assert rc == 1 and b"shape" in msg
    refused(nlabel=0)
    rc, msg = refused(grad_cost=V)                       # the gather reads cost while it writes grad_cost
    assert rc == 1 and b"alias" in msg
    # the workspace: 24 bytes per output pixel; one byte short, missing or absent is refused with the size
    need = lib.sfm_depth_head_backward_workspace_bytes(B, H, W)
    assert need >= 24 * B * H * W and lib.sfm_depth_head_backward_workspace_bytes(0, H, W) == 0
    assert lib.sfm_depth_head_backward_workspace_bytes(B, 0, W) == 0
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None)):
        rc, msg = refused(**kw)
        assert rc == 3 and b"workspace" in msg and str(need).encode() in msg, (kw, msg)
    rc, msg = refused(ws=ctypes.c_void_p(4096 + 4))
    assert rc == 1 and b"aligned" in msg
    # the contributor query checks its arguments too
    out = [ctypes.c_int(0) for _ in range(4)]
    refs = [ctypes.byref(o) for o in out]
    assert lib.sfm_depth_head_contributors(5, 18, 5, *refs) == 1 and lib.sfm_depth_head_contributors(5, 18, -1, *refs) == 1
    assert lib.sfm_depth_head_contributors(0, 18, 0, *refs) == 1 and lib.sfm_depth_head_contributors(5, 0, 0, *refs) == 1
    assert lib.sfm_depth_head_contributors(5, 18, 0, None, refs[1], refs[2], refs[3]) == 1
    assert b"null" in lib.sfm_last_error()


def _axis_weights(dst, in_size, out_size):
    """axis_weights of csrc/depth_head.h (PyTorch's area_pixel_compute_source_index
    and guard_index_and_lambda) in Python's float64: (i0, i1)."""
    if in_size == out_size:
        return dst, dst
    src = (in_size / out_size) * (dst + 0.5) - 0.5
    if src < 0.0:
        src = 0.0
    i0 = min(int(math.floor(src)), in_size - 1)
    return i0, i0 + (1 if i0 < in_size - 1 else 0)


@pytest.mark.parametrize("in_size", [1, 2, 3, 5, 7, 9])
@pytest.mark.parametrize("out_size", [1, 2, 5, 6, 18, 27])
def test_contributor_runs_transpose_the_source_index_map(in_size, out_size):
    from sfm_amd import _lib
    lib = _lib.load()
    taps = [_axis_weights(d, in_size, out_size) for d in range(out_size)]
    seen0, seen1 = [0] * out_size, [0] * out_size
    for cell in range(in_size):
        f0, c0, f1, c1 = (ctypes.c_int(-7) for _ in range(4))
        rc = lib.sfm_depth_head_contributors(in_size, out_size, cell, ctypes.byref(f0), ctypes.byref(c0),
                                             ctypes.byref(f1), ctypes.byref(c1))
        assert rc == 0, lib.sfm_last_error()
        run0 = list(range(f0.value, f0.value + c0.value))
        run1 = list(range(f1.value, f1.value + c1.value))
        assert c0.value >= 0 and c1.value >= 0
        assert run0 == [d for d in range(out_size) if taps[d][0] == cell], (cell, run0)
        assert run1 == [d for d in range(out_size) if taps[d][1] == cell], (cell, run1)
        if not any(cell in t for t in taps):                  # downsampling: nobody reads the cell
            assert c0.value == 0 and c1.value == 0
        for d in run0:
            seen0[d] += 1
        for d in run1:
            seen1[d] += 1
    # every output index is tap 0 of exactly one cell and tap 1 of exactly one cell
    assert seen0 == [1] * out_size and seen1 == [1] * out_size
    if in_size == out_size:                                   # the identity: its own cell, both taps
        assert all(t == (d, d) for d, t in enumerate(taps))
    else:                                                     # the clamped edge: tap 1 is tap 0's cell
        assert all(t[1] == t[0] + 1 or t[0] == t[1] == in_size - 1 for t in taps)
