"""CPU-side checks of the float16 training path of the full-resolution
refinement stack dep_convs (models/PSNet.py:218-221): the declaration of
sfm_dep_context_unpack_grad_f16, its refusals (each returned with a message
before anything is launched: no device is touched, the pointers are never
dereferenced), PSNet's ``dep_context_grad`` argument, and the specification the
GPU tests compare the kernel against -- the gather rule of include/sfm_hip.h
restated in float64, equal to autograd's backward of F.interpolate."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w, H, W): the exact lattice, the general ratio, sy = 0 with one source row, H == 1, a downsample by 2 in y
# (the odd source rows are read with weight 0 only), a downsample by 4 (source rows no destination reads at all)
SHAPES = [(4, 18, 13, 69), (6, 20, 22, 78), (1, 3, 5, 7), (3, 4, 1, 6), (9, 11, 5, 7), (9, 11, 3, 4)]


def _axis(n_src, n_dst):
    """wy(i, y) = ly0 [y0 == i] + ly1 [y1 == i] as an [n_src, n_dst] float64
    matrix, and which sources receive anything (a non-zero weight from some
    destination): the forward's index expression (k_dep_pack) evaluated per
    destination."""
    s = (n_src - 1) / (n_dst - 1) if n_dst > 1 else 0.0
    wt = torch.zeros(n_src, n_dst, dtype=torch.float64)
    for d in range(n_dst):
        f = s * float(d)
        i0 = min(int(f), n_src - 1)
        i1 = i0 + (1 if i0 < n_src - 1 else 0)
        l1 = f - float(i0)
        wt[i0, d] += 1.0 - l1
        wt[i1, d] += l1
    return wt, wt.sum(1) != 0


def gather_adjoint(g, h, w):
    """The kernel's rule on g [B, C, H, W] float64 -> ([B, C, h, w] float64,
    [h, w] bool: the source pixels that receive anything)."""
    wy, ry = _axis(h, g.shape[2])
    wx, rx = _axis(w, g.shape[3])
    return torch.einsum("iy,bcyx,jx->bcij", wy, g.double(), wx), ry[:, None] & rx[None, :]


@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_gather_rule_is_autograds_backward_of_interpolate(h, w, H, W):
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    go = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    F.interpolate(feat, [H, W], mode="bilinear", align_corners=True).backward(go)
    got, read = gather_adjoint(go, h, w)
    assert float((got - feat.grad).abs().max()) <= 1e-12
    # what receives nothing is exactly zero in both
    assert bool((feat.grad[:, :, ~read] == 0).all()) and bool((got[:, :, ~read] == 0).all())
    # the adjoint of a map whose rows sum to one: the total is kept
    assert abs(float(got.sum() - go.sum())) <= 1e-10


def test_which_sources_receive_anything_in_the_degenerate_shapes():
    assert _axis(3, 1)[1].tolist() == [True, False, False]      # H == 1: y0 = 0, and y1 = 1 with weight 0
    assert _axis(1, 5)[1].tolist() == [True] and _axis(1, 5)[0].tolist() == [[1.0] * 5]
    assert _axis(9, 5)[1].tolist() == [True, False] * 4 + [True]        # scale 2: the even rows
    assert _axis(9, 3)[1].tolist() == [True, False, False, False] * 2 + [True]
    assert bool(_axis(4, 13)[1].all()) and bool(_axis(20, 78)[1].all())
    # the last row's two taps land on the same source
    assert _axis(4, 13)[0][3].tolist() == [0.0] * 9 + [0.25, 0.5, 0.75, 1.0]


def _params(hdr, name, ret="int"):
    m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in sfm_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    return [" ".join(p.split()) for p in params], hdr[:m.start()].rsplit("/*", 1)[1]


def test_exported_with_declared_signature():
    from sfm_amd import _lib
    lib = _lib.load()
    name = "sfm_dep_context_unpack_grad_f16"
    assert hasattr(lib, name) and name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    got, doc = _params(hdr, name)
    assert got == ["const void* grad_in0", "int batch", "int b0", "int nb", "int channels", "int h", "int w", "int H",
                   "int W", "float* grad_feat", "void* stream"]
    sig = dict((s[0], s) for s in _lib._SIGS)[name]
    assert sig[1] is ctypes.c_int and len(sig[2]) == len(got)
    for kind, p in zip(sig[2], got):
        assert (kind is ctypes.c_int) == p.startswith("int "), p
    assert "models/PSNet.py:218-221" in doc and '"dep_context_unpack_grad"' in doc
    assert "y0 = min((int)fy, h - 1)" in doc and "+0" in doc
    assert lib.sfm_abi_version() == 1
    # no new enumerated tuning key
    assert not any("dep" in k for k in _lib.tune_keys())


G, GF = (ctypes.c_void_p(a << 32) for a in (1, 2))       # 16-byte aligned stand-in pointers


def test_refuses_bad_arguments_before_any_launch():
    from sfm_amd import _lib
    lib = _lib.load()

    def unpack(g=G, gf=GF, batch=3, b0=1, nb=2, channels=32, h=4, w=18, H=13, W=69):
        rc = lib.sfm_dep_context_unpack_grad_f16(g, batch, b0, nb, channels, h, w, H, W, gf, None)
        return rc, lib.sfm_last_error()

    big = 1 << 14
    for kw, word in ((dict(g=None), b"null"), (dict(gf=None), b"null"),
                     (dict(channels=31), b"32 feature"), (dict(channels=33), b"32 feature"),
                     (dict(b0=2), b"pair range"), (dict(nb=0), b"pair range"), (dict(b0=-1), b"pair range"),
                     (dict(b0=0, nb=4), b"pair range"),
                     (dict(batch=0), b"shape"), (dict(h=0), b"shape"), (dict(W=0), b"shape"),
                     (dict(g=ctypes.c_void_p(G.value + 8)), b"aligned"),
                     (dict(g=ctypes.c_void_p(G.value + 2)), b"aligned"),
                     (dict(gf=ctypes.c_void_p(GF.value + 2)), b"aligned"),
                     (dict(h=big, w=big), b"feature map too large"),
                     (dict(H=big, W=big), b"image too large")):
        rc, msg = unpack(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)


def test_lazy_export_and_psnet_argument():
    import sfm_amd
    from sfm_amd import context
    for name in ("dep_context_refine_autograd", "dep_context_unpack_grad"):
        assert name in sfm_amd.__all__ and getattr(sfm_amd, name) is getattr(context, name)
    import sfm_amd.psnet as P
    from sfm_amd.config import defaults
    c = defaults()
    c.update(PSNET_DEP_CONTEXT=True)
    feat = lambda: torch.nn.Conv2d(3, 32, 4, stride=4)
    net = P.PSNet(4, 1.0, cfg=c, feature_fn=feat())
    assert net.dep_context_grad == "torch" and net.dep_context_grad_route("cpu") == "torch"
    for bad in ("x", "auto", "bf16", None):
        with pytest.raises(ValueError, match="dep_context_grad"):
            P.PSNet(4, 1.0, cfg=c, feature_fn=feat(), dep_context_grad=bad)
    forced = P.PSNet(4, 1.0, cfg=c, feature_fn=feat(), dep_context_grad="fp16")
    assert forced.dep_context_grad == "fp16" and forced.context_grad == "torch"
    with pytest.raises(RuntimeError, match="dep_context_grad='fp16'.*autocast"):
        forced.dep_context_grad_route("cpu")
    with pytest.raises(RuntimeError, match="device tensors"):
        context.dep_context_refine_autograd(net.dep_convs, torch.zeros(1, 1, 8, 12), torch.zeros(1, 32, 2, 3),
                                            torch.zeros(1, 3, 8, 12))
    with pytest.raises(RuntimeError, match="device tensor"):
        context.dep_context_unpack_grad(torch.zeros(1, 8, 12, 64, dtype=torch.float16), 0, torch.zeros(1, 32, 2, 3))
