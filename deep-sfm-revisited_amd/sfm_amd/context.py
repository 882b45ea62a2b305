"""PSNet's per-plane context stack on the gfx950 matrix cores.

The reference refines every plane of the regularised cost volume with a
seven-stage dilated 2-D CNN over ``cat(ref features, plane)`` and adds the
plane back (models/PSNet.py:17-26 ``convtext``, 64-71 the stack, 175-190 its
application):

    costss[:, :, l] = convs(cat(refimg_fea, costs[:, :, l])) + costs[:, :, l]

``context_refine`` runs it as one ``sfm_context_pack_*`` and seven
``sfm_conv2_*`` launches per chunk of planes: float16 (or bfloat16)
channels-last activations and weights, fp32 accumulation, BatchNorm2d folded
in eval mode, ReLU and the final fp32 "+ plane" fused into the epilogue --
the precision torch computes these convolutions at under ``cfg.MIXED_PREC``
autocast (SFMnet.py:164).  There is no PyTorch fallback: without
libsfm_hip.so or a GPU the call raises.

``dep_context_refine`` runs the second stack of the same plan, ``dep_convs``
(PSNet.py:53-61, 218-222, cfg.PSNET_DEP_CONTEXT), at full image resolution:

    depth_out = dep_convs(cat(depth, upsample(refimg_fea), ref)) + depth

as one ``sfm_dep_context_pack_*`` (the bilinear upsample fused in) and the same
seven ``sfm_conv2_*`` launches per chunk of pairs.
"""
import weakref

import torch
import torch.nn as nn

from . import _lib

_ACT_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
_SUFFIX = {"fp16": "f16", "bf16": "bf16"}
_CHANNELS = (32, 64, 96, 128)
MAX_DILATION = 16


class ContextStackError(RuntimeError):
    """The module is not a stack ``sfm_conv2_*`` can run."""


def _pad32(n):
    return (n + 31) // 32 * 32


def _conv2(x, weights, scale, bias, dilation, relu, cout, residual, precision):
    dtype = _ACT_DTYPE[precision]
    name = str(dtype).replace("torch.", "")
    for t, n in ((x, "x"), (weights, "weights")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise RuntimeError(f"{n} must be a contiguous {name} device tensor")
    if x.dim() != 4:
        raise RuntimeError("x must be [images, h, w, cin] (channels-last)")
    n, h, w, cin = x.shape
    if cin not in _CHANNELS:
        raise RuntimeError(f"cin must be one of {_CHANNELS}")
    if weights.dim() != 3 or weights.shape[0] != 9 or weights.shape[2] != cin or weights.shape[1] % 32:
        raise RuntimeError(f"weights must be [9, cout_pad, {cin}] with cout_pad a multiple of 32")
    cout_pad = weights.shape[1]
    cout = cout_pad if cout is None else int(cout)
    if _pad32(cout) != cout_pad or (cout != 1 and cout not in _CHANNELS):
        raise RuntimeError(f"cout {cout} does not match weights of {cout_pad} rows")
    if not 1 <= int(dilation) <= MAX_DILATION:
        raise RuntimeError(f"dilation must be 1..{MAX_DILATION}")
    scale = scale.to(device=x.device, dtype=torch.float32).contiguous()
    bias = bias.to(device=x.device, dtype=torch.float32).contiguous()
    if scale.numel() != cout_pad or bias.numel() != cout_pad:
        raise RuntimeError(f"scale and bias must have {cout_pad} entries")
    if residual is not None:
        if cout != 1:
            raise RuntimeError("residual needs cout 1")
        if not (residual.is_cuda and residual.dtype == torch.float32 and residual.numel() == n * h * w):
            raise RuntimeError("residual must be a float32 device tensor of images x h x w values")
        residual = residual.contiguous()
    if cout == 1:
        out = torch.empty((n, h, w), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty((n, h, w, cout), dtype=dtype, device=x.device)
    fn = "sfm_conv2_" + _SUFFIX[precision]
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), fn)(_lib.ptr(x), n, cin, h, w, _lib.ptr(weights), cout, int(dilation),
                                      _lib.ptr(scale), _lib.ptr(bias), 1 if relu else 0, _lib.ptr(residual),
                                      _lib.ptr(out), _lib.stream_ptr(x.device))
        _lib.check(rc, fn)
    return out


def conv2_f16(x, weights, scale, bias, dilation, relu=True, cout=None, residual=None):
    """One fused stage: x [images, h, w, cin] float16, weights [9, cout_pad,
    cin] float16, scale/bias [cout_pad] fp32 -> [images, h, w, cout] float16,
    or for ``cout=1`` [images, h, w] fp32 with ``residual`` (fp32, the same
    shape) added after the float16 rounding.  ``cout`` defaults to cout_pad."""
    return _conv2(x, weights, scale, bias, dilation, relu, cout, residual, "fp16")


def conv2_bf16(x, weights, scale, bias, dilation, relu=True, cout=None, residual=None):
    """``conv2_f16`` with bfloat16 activations and weights (sfm_conv2_bf16)."""
    return _conv2(x, weights, scale, bias, dilation, relu, cout, residual, "bf16")


def _stages(convs):
    """(conv, bn or None, relu) per stage of a stack of convtext blocks."""
    if not isinstance(convs, nn.Sequential) or len(convs) == 0:
        raise ContextStackError("the context stack must be a non-empty nn.Sequential of convtext blocks")
    out = []
    for i, blk in enumerate(convs):
        mods = list(blk) if isinstance(blk, nn.Sequential) else [blk]
        if not mods or not isinstance(mods[0], nn.Conv2d):
            raise ContextStackError(f"stage {i}: expected Conv2d [+ BatchNorm2d] [+ ReLU]")
        conv, rest = mods[0], mods[1:]
        bn = None
        if rest and isinstance(rest[0], nn.BatchNorm2d):
            bn, rest = rest[0], rest[1:]
        relu = False
        if rest and isinstance(rest[0], nn.ReLU):
            relu, rest = True, rest[1:]
        if rest:
            raise ContextStackError(f"stage {i}: expected Conv2d [+ BatchNorm2d] [+ ReLU], found {type(rest[0]).__name__}")
        d = conv.dilation[0]
        if tuple(conv.kernel_size) != (3, 3):
            raise ContextStackError(f"stage {i}: kernel size {tuple(conv.kernel_size)}, only 3 x 3 is built")
        if tuple(conv.stride) != (1, 1):
            raise ContextStackError(f"stage {i}: stride {tuple(conv.stride)}, only stride 1 is built")
        if conv.dilation[0] != conv.dilation[1] or not 1 <= d <= MAX_DILATION:
            raise ContextStackError(f"stage {i}: dilation {tuple(conv.dilation)}, only square 1..{MAX_DILATION}")
        if tuple(conv.padding) != (d, d) or conv.padding_mode != "zeros":
            raise ContextStackError(f"stage {i}: padding {conv.padding} must equal the dilation {d} (zeros)")
        if conv.bias is not None:
            raise ContextStackError(f"stage {i}: a Conv2d bias is not built (convtext has none)")
        if conv.groups != 1:
            raise ContextStackError(f"stage {i}: grouped convolutions are not built")
        if _pad32(conv.in_channels) > 128 or not (conv.out_channels == 1 or conv.out_channels in _CHANNELS):
            raise ContextStackError(f"stage {i}: {conv.in_channels} -> {conv.out_channels} channels is not built")
        if bn is not None and (not bn.track_running_stats or bn.running_mean is None):
            raise ContextStackError(f"stage {i}: BatchNorm2d without running statistics cannot be folded")
        if out and _pad32(out[-1][0].out_channels) != _pad32(conv.in_channels):
            raise ContextStackError(f"stage {i}: {conv.in_channels} inputs after {out[-1][0].out_channels} outputs")
        if out and out[-1][0].out_channels == 1:
            raise ContextStackError(f"stage {i}: a 1-channel stage must be the last")
        out.append((conv, bn, relu))
    return out


_PACKED = weakref.WeakKeyDictionary()      # convs -> (key, packed)


def pack_context_stack(convs, device, precision="fp16"):
    """Packed weights [9][cout_pad][cin_pad] in the precision's type (tap =
    kh*3 + kw; rows beyond cout and columns beyond cin zero) and the folded
    fp32 scale/bias [cout_pad] of every stage of ``convs``, an nn.Sequential
    of PSNet's convtext blocks (Conv2d [+ BatchNorm2d] + ReLU).  BatchNorm2d
    folds with its running statistics (eval mode), as
    ``CostRegularization.pack`` folds BatchNorm3d.  Cached until a parameter
    or buffer changes."""
    if precision not in _ACT_DTYPE:
        raise ValueError(f"unknown context precision {precision!r}")
    stages = _stages(convs)
    key = (str(device), precision) + tuple((t.data_ptr(), t._version)
                                           for t in list(convs.parameters()) + list(convs.buffers()))
    hit = _PACKED.get(convs)
    if hit is not None and hit[0] == key:
        return hit[1]
    wdt = _ACT_DTYPE[precision]
    packed = []
    with torch.no_grad():
        for conv, bn, relu in stages:
            w = conv.weight.detach().float().cpu()                 # [cout, cin, 3, 3]
            cout, cin = w.shape[:2]
            cout_pad, cin_pad = _pad32(cout), _pad32(cin)
            wp = torch.zeros(9, cout_pad, cin_pad, dtype=torch.float32)
            wp[:, :cout, :cin] = w.permute(2, 3, 0, 1).reshape(9, cout, cin)
            sc = torch.ones(cout_pad)
            bi = torch.zeros(cout_pad)
            if bn is not None:
                g = torch.ones(cout) if bn.weight is None else bn.weight.detach().float().cpu()
                b = torch.zeros(cout) if bn.bias is None else bn.bias.detach().float().cpu()
                scale = g / torch.sqrt(bn.running_var.detach().float().cpu() + bn.eps)
                sc[:cout] = scale
                bi[:cout] = b - bn.running_mean.detach().float().cpu() * scale
            packed.append(dict(w=wp.to(device=device, dtype=wdt).contiguous(), scale=sc.to(device),
                               bias=bi.to(device), cin=cin, cin_pad=cin_pad, cout=cout, cout_pad=cout_pad,
                               dilation=int(conv.dilation[0]), relu=relu))
    _PACKED[convs] = (key, packed)
    return packed


def stock_layout(convs):
    """Whether ``convs`` is a stack ``context_refine`` runs: stages the
    kernels take, 33 input channels (32 features + the plane), one output."""
    try:
        st = _stages(convs)
    except ContextStackError:
        return False
    return st[0][0].in_channels == 33 and st[-1][0].out_channels == 1 and len(st) >= 2


def planes_per_chunk(batch, h, w, nlabel, max_scratch_bytes):
    """The most planes whose two 128-channel ping-pong buffers fit
    ``max_scratch_bytes``; at least one, at most nlabel."""
    per_plane = 2 * batch * h * w * 128 * 2
    return max(1, min(int(nlabel), int(max_scratch_bytes) // per_plane))


def context_refine(convs, ctx, costs, precision="fp16", max_scratch_bytes=1 << 30):
    """``convs(cat(ctx, plane)) + plane`` for every plane (PSNet.py:175-190):
    ctx [B, 32, h, w] (any float dtype), costs [B, 1, L, h, w] fp32 ->
    [B, 1, L, h, w] fp32.  The planes go through in chunks of
    ``planes_per_chunk``; the result does not depend on the chunking."""
    if precision not in _ACT_DTYPE:
        raise ValueError(f"unknown context precision {precision!r}")
    for t, n in ((ctx, "ctx"), (costs, "costs")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"context_refine needs device tensors (HIP path, no CPU fallback): {n}")
    if costs.dim() != 5 or costs.shape[1] != 1 or costs.dtype != torch.float32:
        raise RuntimeError("costs must be [B, 1, L, h, w] float32")
    B, _, L, h, w = costs.shape
    if ctx.dim() != 4 or tuple(ctx.shape) != (B, 32, h, w) or not ctx.is_floating_point():
        raise RuntimeError(f"ctx must be [{B}, 32, {h}, {w}] floating point")
    if not stock_layout(convs):
        _stages(convs)          # raises the named reason, if that is it
        raise ContextStackError("the context stack must take 33 channels and end in one")
    dev = costs.device
    packed = pack_context_stack(convs, dev, precision)
    adt = _ACT_DTYPE[precision]
    lib = _lib.load()
    pack = getattr(lib, "sfm_context_pack_" + _SUFFIX[precision])
    conv = getattr(lib, "sfm_conv2_" + _SUFFIX[precision])
    ctx32 = ctx.detach().float().contiguous()
    planes = costs.detach().reshape(B, L, h, w).contiguous()
    nl_max = planes_per_chunk(B, h, w, L, max_scratch_bytes)
    out = torch.empty((B, L, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        bufs = [torch.empty(B * nl_max * h * w * 128, dtype=adt, device=dev) for _ in range(2)]
        for l0 in range(0, L, nl_max):
            nl = min(nl_max, L - l0)
            whole = nl == L
            resid = planes if whole else planes[:, l0:l0 + nl].contiguous()
            last = out if whole else torch.empty((B, nl, h, w), dtype=torch.float32, device=dev)
            _lib.check(pack(_lib.ptr(ctx32), _lib.ptr(planes), B, L, l0, nl, 32, h, w, _lib.ptr(bufs[0]), stream),
                       "sfm_context_pack")
            cur = 0
            for lay in packed:
                final = lay["cout"] == 1
                dst = last if final else bufs[1 - cur]
                rc = conv(_lib.ptr(bufs[cur]), B * nl, lay["cin_pad"], h, w, _lib.ptr(lay["w"]), lay["cout"],
                          lay["dilation"], _lib.ptr(lay["scale"]), _lib.ptr(lay["bias"]), 1 if lay["relu"] else 0,
                          _lib.ptr(resid) if final else None, _lib.ptr(dst), stream)
                _lib.check(rc, "sfm_conv2")
                cur = 1 - cur
            if not whole:
                out[:, l0:l0 + nl].copy_(last)
    return out.view(B, 1, L, h, w)


# --- the full-resolution refinement stack dep_convs (PSNet.py:53-61, 218-222) ------
_FEAT_DTYPE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # sfm_dep_context_pack_*'s feat_dtype


def dep_stock_layout(dep_convs):
    """Whether ``dep_convs`` is a stack ``dep_context_refine`` runs: stages
    the kernels take, 36 input channels (depth + 32 features + the image),
    one output."""
    try:
        st = _stages(dep_convs)
    except ContextStackError:
        return False
    return st[0][0].in_channels == 36 and st[-1][0].out_channels == 1 and len(st) >= 2


def pairs_per_chunk(batch, H, W, max_scratch_bytes):
    """The most pairs whose two 128-channel full-resolution ping-pong buffers
    fit ``max_scratch_bytes``; at least one, at most batch."""
    per_pair = 2 * H * W * 128 * 2
    return max(1, min(int(batch), int(max_scratch_bytes) // per_pair))


def dep_context_refine(dep_convs, depth, feat, image, precision="fp16", max_scratch_bytes=1 << 30):
    """``dep_convs(cat(depth, upsample(feat), image)) + depth``
    (PSNet.py:218-221): depth [B, 1, H, W] fp32, feat [B, 32, h, w] float16,
    bfloat16 or float32 (read as it is), image [B, 3, H, W] -> [B, 1, H, W]
    fp32.  One ``sfm_dep_context_pack_*`` (the bilinear align_corners=True
    upsample fused in) and the stack's ``sfm_conv2_*`` launches per chunk of
    ``pairs_per_chunk`` whole pairs; the result does not depend on the
    chunking.  No PyTorch fallback: CPU tensors raise."""
    if precision not in _ACT_DTYPE:
        raise ValueError(f"unknown context precision {precision!r}")
    for t, n in ((depth, "depth"), (feat, "feat"), (image, "image")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"dep_context_refine needs device tensors (HIP path, no CPU fallback): {n}")
    if depth.dim() != 4 or depth.shape[1] != 1 or depth.dtype != torch.float32:
        raise RuntimeError("depth must be [B, 1, H, W] float32")
    B, _, H, W = depth.shape
    if feat.dim() != 4 or feat.shape[0] != B or feat.shape[1] != 32 or feat.dtype not in _FEAT_DTYPE:
        raise RuntimeError(f"feat must be [{B}, 32, h, w] float16, bfloat16 or float32")
    if tuple(image.shape) != (B, 3, H, W) or not image.is_floating_point():
        raise RuntimeError(f"image must be [{B}, 3, {H}, {W}] floating point")
    if not dep_stock_layout(dep_convs):
        _stages(dep_convs)      # raises the named reason, if that is it
        raise ContextStackError("the refinement stack must take 36 channels and end in one")
    h, w = feat.shape[2:]
    dev = depth.device
    packed = pack_context_stack(dep_convs, dev, precision)
    adt = _ACT_DTYPE[precision]
    lib = _lib.load()
    pack = getattr(lib, "sfm_dep_context_pack_" + _SUFFIX[precision])
    conv = getattr(lib, "sfm_conv2_" + _SUFFIX[precision])
    depth = depth.detach().contiguous()
    feat = feat.detach().contiguous()
    image = image.detach().float().contiguous()
    nb_max = pairs_per_chunk(B, H, W, max_scratch_bytes)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        bufs = [torch.empty(nb_max * H * W * 128, dtype=adt, device=dev) for _ in range(2)]
        for b0 in range(0, B, nb_max):
            nb = min(nb_max, B - b0)
            whole = nb == B
            # a chunk's slice of depth is contiguous; the last stage writes a buffer of its own, 16-byte aligned
            last = out if whole else torch.empty((nb, H, W), dtype=torch.float32, device=dev)
            _lib.check(pack(_lib.ptr(depth), _lib.ptr(feat), _FEAT_DTYPE[feat.dtype], _lib.ptr(image), B, b0, nb, 32,
                            h, w, H, W, _lib.ptr(bufs[0]), stream), "sfm_dep_context_pack")
            cur = 0
            for lay in packed:
                final = lay["cout"] == 1
                dst = last if final else bufs[1 - cur]
                rc = conv(_lib.ptr(bufs[cur]), nb, lay["cin_pad"], H, W, _lib.ptr(lay["w"]), lay["cout"],
                          lay["dilation"], _lib.ptr(lay["scale"]), _lib.ptr(lay["bias"]), 1 if lay["relu"] else 0,
                          _lib.ptr(depth[b0:b0 + nb]) if final else None, _lib.ptr(dst), stream)
                _lib.check(rc, "sfm_conv2")
                cur = 1 - cur
            if not whole:
                out[b0:b0 + nb, 0].copy_(last)
    return out
