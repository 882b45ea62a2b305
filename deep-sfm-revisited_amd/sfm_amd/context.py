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

``context_refine_autograd`` is ``context_refine`` in float16 with a backward
(csrc/context_bwd.hip): per stage ``sfm_conv2_wgrad_f16`` and
``sfm_conv2_dgrad_f16``, then ``sfm_context_unpack_grad_f16``.
``dep_context_refine_autograd`` is the same for ``dep_context_refine``; its
last step is ``sfm_dep_context_unpack_grad_f16``, the backward of the bilinear
upsample into the features.
"""
import weakref

import torch
import torch.nn as nn

from . import _lib
from .feature import _fold_stage, _pad32, pack_dgrad_weights2x, unpack_wgrad2x

_ACT_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
_SUFFIX = {"fp16": "f16", "bf16": "bf16"}
_CHANNELS = (32, 64, 96, 128)
MAX_DILATION = 16


class ContextStackError(RuntimeError):
    """The module is not a stack ``sfm_conv2_*`` can run."""


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
    with torch.no_grad():
        packed = [_fold_stage(conv, bn, relu, device, _ACT_DTYPE[precision]) for conv, bn, relu in stages]
    _PACKED[convs] = (key, packed)
    return packed


def _stock(convs, cin):
    try:
        st = _stages(convs)
    except ContextStackError:
        return False
    return st[0][0].in_channels == cin and st[-1][0].out_channels == 1 and len(st) >= 2


def stock_layout(convs):
    """Whether ``convs`` is a stack ``context_refine`` runs: stages the
    kernels take, 33 input channels (32 features + the plane), one output."""
    return _stock(convs, 33)


def _need_device(who, **tensors):
    for n, t in tensors.items():
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{who} needs device tensors (HIP path, no CPU fallback): {n}")


def _autocast_gpu_dtype():
    """torch.get_autocast_gpu_dtype(), by its newer name where torch has it."""
    if hasattr(torch, "get_autocast_dtype"):
        return torch.get_autocast_dtype("cuda")
    return torch.get_autocast_gpu_dtype()


def _need_f16_autocast(who):
    if not torch.is_autocast_enabled() or _autocast_gpu_dtype() != torch.float16:
        raise RuntimeError(f"{who} computes the stack in float16: call it under torch.autocast('cuda', torch.float16)")


def _check_context(who, convs, ctx, costs, autocast=False):
    """``who``'s refusals in their order: device tensors, float16 autocast
    (the autograd route), shapes, layout."""
    _need_device(who, ctx=ctx, costs=costs)
    if autocast:
        _need_f16_autocast(who)
    if costs.dim() != 5 or costs.shape[1] != 1 or costs.dtype != torch.float32:
        raise RuntimeError("costs must be [B, 1, L, h, w] float32")
    B, _, L, h, w = costs.shape
    if ctx.dim() != 4 or tuple(ctx.shape) != (B, 32, h, w) or not ctx.is_floating_point():
        raise RuntimeError(f"ctx must be [{B}, 32, {h}, {w}] floating point")
    if not stock_layout(convs):
        _stages(convs)          # raises the named reason, if that is it
        raise ContextStackError("the context stack must take 33 channels and end in one")


def _trainable(stages, device):
    """The stages' Conv2d weights, or the reason the float16 route has no
    backward for them."""
    for i, (conv, bn, relu) in enumerate(stages):
        if bn is not None:
            mode = "in training mode (batch statistics)" if bn.training else "in eval mode (a folded affine)"
            raise ContextStackError(f"stage {i}: BatchNorm2d {mode} has no backward on the float16 route")
        if conv.weight.dtype != torch.float32 or conv.weight.device != device:
            raise ContextStackError(f"stage {i}: the weight must be float32 on the tensors' device")
    return [conv.weight for conv, _, _ in stages]


def _run_stack(conv, packed, x, n, h, w, stream, bufs, last, resid):
    """The packed stages over one chunk: x [n, h, w, 64] the packed first
    activation, ``conv`` the precision's ``sfm_conv2_*``.  The last stage
    writes ``last`` (fp32), with ``resid`` (fp32, or None) added in the same
    launch.  The stages between write the ping-pong buffers ``bufs`` in turn
    (x is bufs[0]); with ``bufs`` None each writes a tensor of its own and
    every stage's input is kept.  Returns the kept inputs."""
    acts = []
    for i, lay in enumerate(packed):
        final = lay["cout"] == 1
        if bufs is None:
            acts.append(x)
        if final:
            y = last
        elif bufs is None:
            y = torch.empty((n, h, w, lay["cout"]), dtype=x.dtype, device=x.device)
        else:
            y = bufs[(i + 1) % 2]
        rc = conv(_lib.ptr(x), n, lay["cin_pad"], h, w, _lib.ptr(lay["w"]), lay["cout"], lay["dilation"],
                  _lib.ptr(lay["scale"]), _lib.ptr(lay["bias"]), 1 if lay["relu"] else 0,
                  _lib.ptr(resid) if final else None, _lib.ptr(y), stream)
        _lib.check(rc, "sfm_conv2")
        x = y
    return acts


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
    _check_context("context_refine", convs, ctx, costs)
    B, _, L, h, w = costs.shape
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
            _run_stack(conv, packed, bufs[0], B * nl, h, w, stream, bufs, last, resid)
            if not whole:
                out[:, l0:l0 + nl].copy_(last)
    return out.view(B, 1, L, h, w)


# --- the full-resolution refinement stack dep_convs (PSNet.py:53-61, 218-222) ------
_FEAT_DTYPE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # sfm_dep_context_pack_*'s feat_dtype


def dep_stock_layout(dep_convs):
    """Whether ``dep_convs`` is a stack ``dep_context_refine`` runs: stages
    the kernels take, 36 input channels (depth + 32 features + the image),
    one output."""
    return _stock(dep_convs, 36)


def _check_dep_context(who, dep_convs, depth, feat, image, autocast=False):
    """``who``'s refusals in their order: device tensors, float16 autocast
    (the autograd route), shapes, layout."""
    _need_device(who, depth=depth, feat=feat, image=image)
    if autocast:
        _need_f16_autocast(who)
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
    _check_dep_context("dep_context_refine", dep_convs, depth, feat, image)
    B, _, H, W = depth.shape
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
            _run_stack(conv, packed, bufs[0], nb, H, W, stream, bufs, last, depth[b0:b0 + nb])
            if not whole:
                out[b0:b0 + nb, 0].copy_(last)
    return out


# --- the stack's backward in float16 (csrc/context_bwd.hip) -------------------------
def pack_dgrad_weights2(weight):
    """The weights that turn sfm_conv2_f16's kernel into the stage's data
    gradient (sfm_conv2_dgrad_f16): Wd[t][ci][co] = W[co][ci][8 - t] as
    [9, cin_pad, cout_pad], rows beyond cin and columns beyond cout zero.
    Pure torch, any device and dtype."""
    return pack_dgrad_weights2x(weight)


def unpack_wgrad2(gwp, cout, cin):
    """sfm_conv2_wgrad_f16's [9, cout_pad, cin_pad] result in the Conv2d
    parameter's layout [cout, cin, 3, 3]; the padded rows and columns are
    dropped.  Pure torch."""
    return unpack_wgrad2x(gwp, cout, cin, 3)


def _f16_cl(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and
            t.dim() == 4 and t.shape[-1] in _CHANNELS):
        raise RuntimeError(f"{name} must be a contiguous [images, h, w, c] float16 device tensor, c in {_CHANNELS} "
                           "(HIP path, no CPU fallback)")


def conv2_wgrad_f16(x, grad_out, dilation):
    """sfm_conv2_wgrad_f16: x [images, h, w, cin] and grad_out [images, h, w,
    cout_pad], contiguous float16 device tensors -> [9, cout_pad, cin]
    float32, reproducible bit for bit."""
    _f16_cl(x, "x")
    _f16_cl(grad_out, "grad_out")
    n, h, w, cin = x.shape
    if tuple(grad_out.shape[:3]) != (n, h, w):
        raise RuntimeError("grad_out must have x's images, h and w")
    cop = grad_out.shape[-1]
    lib = _lib.load()
    gw = torch.empty((9, cop, cin), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(16, lib.sfm_conv2_wgrad_f16_workspace_bytes(n, cin, cop, h, w)), dtype=torch.uint8,
                     device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_conv2_wgrad_f16(_lib.ptr(x), _lib.ptr(grad_out), n, cin, cop, h, w, int(dilation), _lib.ptr(gw),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_conv2_wgrad_f16")
    return gw


def conv2_dgrad_f16(grad_out, weights_d, dilation, act=None):
    """sfm_conv2_dgrad_f16: grad_out [images, h, w, cout_pad] float16,
    weights_d [9, cin_pad, cout_pad] float16 (``pack_dgrad_weights2``), act
    [images, h, w, cin_pad] float16 or None -> [images, h, w, cin_pad]
    float16, zero where act is not positive."""
    _f16_cl(grad_out, "grad_out")
    n, h, w, cop = grad_out.shape
    if not (weights_d.is_cuda and weights_d.dtype == torch.float16 and weights_d.is_contiguous() and
            weights_d.dim() == 3 and weights_d.shape[0] == 9 and weights_d.shape[2] == cop and
            weights_d.shape[1] in _CHANNELS):
        raise RuntimeError(f"weights_d must be a contiguous [9, cin_pad, {cop}] float16 device tensor")
    cip = weights_d.shape[1]
    if act is not None:
        _f16_cl(act, "act")
        if tuple(act.shape) != (n, h, w, cip):
            raise RuntimeError(f"act must be [{n}, {h}, {w}, {cip}]")
    out = torch.empty((n, h, w, cip), dtype=torch.float16, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        rc = _lib.load().sfm_conv2_dgrad_f16(_lib.ptr(grad_out), n, cop, h, w, _lib.ptr(weights_d), cip, int(dilation),
                                             _lib.ptr(act), _lib.ptr(out), _lib.stream_ptr(grad_out.device))
        _lib.check(rc, "sfm_conv2_dgrad_f16")
    return out


def context_unpack_grad(g0, grad_out, l0, first, grad_ctx, grad_planes):
    """sfm_context_unpack_grad_f16: g0 [B, nl, h, w, 64] float16, the first
    stage's data gradient for planes l0 .. l0+nl-1; grad_out and grad_planes
    [B, L, h, w] float32; grad_ctx [B, 32, h, w] float32, written when
    ``first`` and added to otherwise.  In place; returns nothing."""
    if not (g0.is_cuda and g0.dtype == torch.float16 and g0.is_contiguous() and g0.dim() == 5 and g0.shape[-1] == 64):
        raise RuntimeError("g0 must be a contiguous [B, nl, h, w, 64] float16 device tensor")
    B, nl, h, w, _ = g0.shape
    for t, n in ((grad_out, "grad_out"), (grad_planes, "grad_planes")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4 and
                t.shape[0] == B and tuple(t.shape[2:]) == (h, w)):
            raise RuntimeError(f"{n} must be a contiguous [B, L, h, w] float32 device tensor")
    L = grad_out.shape[1]
    if grad_planes.shape[1] != L:
        raise RuntimeError("grad_planes must have grad_out's shape")
    if not (grad_ctx.is_cuda and grad_ctx.dtype == torch.float32 and grad_ctx.is_contiguous() and
            tuple(grad_ctx.shape) == (B, 32, h, w)):
        raise RuntimeError("grad_ctx must be a contiguous [B, 32, h, w] float32 device tensor")
    with torch.cuda.device(g0.device):
        rc = _lib.load().sfm_context_unpack_grad_f16(_lib.ptr(g0), _lib.ptr(grad_out), B, L, int(l0), nl, h, w,
                                                     1 if first else 0, _lib.ptr(grad_ctx), _lib.ptr(grad_planes),
                                                     _lib.stream_ptr(g0.device))
        _lib.check(rc, "sfm_context_unpack_grad_f16")


def _stack_backward(acts, grad, relu_out, meta, wds, gws):
    """One chunk's backward through the stages, last to first: ``acts`` the
    kept stage inputs [n, h, w, c] float16, ``grad`` and ``relu_out`` the
    chunk's n h w upstream gradients and last-stage outputs (fp32, one shape),
    ``wds`` the packed data-gradient weights.  Every stage's weight gradient is
    added to ``gws`` in fp32 (call in ascending chunk order); returns the first
    stage's data gradient [n, h, w, 64] float16."""
    n, h, w = acts[0].shape[:3]
    # the last stage: through its ReLU, as channel 0 of a zero-padded 32-channel tensor
    if meta[-1][3]:
        grad = torch.where(relu_out > 0, grad, torch.zeros_like(grad))
    g = torch.zeros((n, h, w, 32), dtype=torch.float16, device=grad.device)
    g[..., 0] = grad.reshape(n, h, w)
    for s in range(len(meta) - 1, -1, -1):
        dil = meta[s][2]
        gw = conv2_wgrad_f16(acts[s], g, dil)
        gws[s] = gw if gws[s] is None else gws[s] + gw
        g = conv2_dgrad_f16(g, wds[s], dil, acts[s] if s > 0 else None)        # stage 0's input has no ReLU
    return g


class _ContextStack(torch.autograd.Function):
    @staticmethod
    def forward(fctx, convs, nl_max, ctx, costs, *weights):
        B, _, L, h, w = costs.shape
        dev = costs.device
        packed = pack_context_stack(convs, dev, "fp16")
        lib = _lib.load()
        ctx32 = ctx.detach().float().contiguous()
        planes = costs.detach().reshape(B, L, h, w).contiguous()
        relu_out = torch.empty((B, L, h, w), dtype=torch.float32, device=dev)
        saved = []                              # per chunk: the seven stages' float16 inputs
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            for l0 in range(0, L, nl_max):
                nl = min(nl_max, L - l0)
                x = torch.empty((B * nl, h, w, 64), dtype=torch.float16, device=dev)
                _lib.check(lib.sfm_context_pack_f16(_lib.ptr(ctx32), _lib.ptr(planes), B, L, l0, nl, 32, h, w,
                                                    _lib.ptr(x), stream), "sfm_context_pack")
                # the last stage without its residual, so that its ReLU output is kept; the fp32 "+ plane"
                # below gives the bits of the fused form
                last = torch.empty((B, nl, h, w), dtype=torch.float32, device=dev)
                saved.append(_run_stack(lib.sfm_conv2_f16, packed, x, B * nl, h, w, stream, None, last, None))
                relu_out[:, l0:l0 + nl].copy_(last)
        fctx.saved, fctx.relu_out, fctx.nl_max = saved, relu_out, nl_max
        fctx.meta = [(lay["cin"], lay["cout"], lay["dilation"], lay["relu"]) for lay in packed]
        fctx.ctx_dtype = ctx.dtype
        fctx.save_for_backward(*weights)
        return (relu_out + planes).view(B, 1, L, h, w)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad):
        weights = fctx.saved_tensors
        B, _, L, h, w = grad.shape
        dev = grad.device
        go = grad.detach().float().reshape(B, L, h, w).contiguous()
        nl_max, meta = fctx.nl_max, fctx.meta
        wds = [pack_dgrad_weights2(wt.detach().float()).half().contiguous() for wt in weights]
        gws = [None] * len(weights)
        grad_ctx = torch.empty((B, 32, h, w), dtype=torch.float32, device=dev)
        grad_planes = torch.empty((B, L, h, w), dtype=torch.float32, device=dev)
        for k, l0 in enumerate(range(0, L, nl_max)):        # ascending: the unpack kernel's summation order
            nl = min(nl_max, L - l0)
            g = _stack_backward(fctx.saved[k], go[:, l0:l0 + nl], fctx.relu_out[:, l0:l0 + nl], meta, wds, gws)
            context_unpack_grad(g.view(B, nl, h, w, 64), go, l0, k == 0, grad_ctx, grad_planes)
            fctx.saved[k] = None                            # a chunk's activations are done with
        out_w = [unpack_wgrad2(gw, m[1], m[0]).to(wt.dtype) for gw, m, wt in zip(gws, meta, weights)]
        return (None, None, grad_ctx.to(fctx.ctx_dtype), grad_planes.view(B, 1, L, h, w)) + tuple(out_w)


def context_refine_autograd(convs, ctx, costs, max_scratch_bytes=1 << 30):
    """``context_refine`` (float16) with a backward on libsfm_hip: one
    autograd function over the whole stack, ctx [B, 32, h, w] (any float
    dtype), costs [B, 1, L, h, w] fp32 -> [B, 1, L, h, w] fp32, the bits of
    ``context_refine(convs, ctx, costs, "fp16")``.  Gradients flow to the seven
    Conv2d weights (float32, the parameters' layout), ``ctx`` and ``costs``.

    Forward: the same ``sfm_context_pack_f16`` and seven ``sfm_conv2_f16``
    launches per chunk of ``planes_per_chunk`` planes; every stage's float16
    input is kept, and the last stage runs without its residual so that its
    ReLU output is kept too (the fp32 "+ plane" is a torch add).  Backward,
    per chunk in ascending plane order and from the last stage to the first:
    ``sfm_conv2_wgrad_f16``, ``sfm_conv2_dgrad_f16`` masked by the saved
    activation, then ``sfm_context_unpack_grad_f16``; weight gradients are
    added over the chunks in fp32.  The ``ctx`` and ``costs`` gradients have
    the same bits for any chunking.

    Memory: the saved activations are 64 + 128 + 128 + 128 + 96 + 64 + 32 =
    640 float16 channels, 1280 bytes per pixel and plane, for all L planes
    until the backward has run: 4.8 GB per KITTI pair at L = 128 (94 x 311);
    ``max_scratch_bytes`` bounds only the chunk's transient buffers.

    Refused with a named reason: CPU tensors, a call outside float16 CUDA
    autocast, a non-stock layout, and any BatchNorm2d stage (in training mode
    its batch statistics have no backward here; in eval mode the folded affine
    has none either)."""
    _check_context("context_refine_autograd", convs, ctx, costs, autocast=True)
    weights = _trainable(_stages(convs), costs.device)
    B, _, L, h, w = costs.shape
    nl_max = planes_per_chunk(B, h, w, L, max_scratch_bytes)
    return _ContextStack.apply(convs, nl_max, ctx, costs, *weights)


# --- dep_convs' backward in float16 (csrc/context_bwd.hip) --------------------------
def dep_context_unpack_grad(g0, b0, grad_feat):
    """sfm_dep_context_unpack_grad_f16: g0 [nb, H, W, 64] float16, the first
    stage's data gradient for pairs b0 .. b0+nb-1 (channels 1..32 the upsampled
    features'); grad_feat [B, 32, h, w] float32, whose pairs b0 .. b0+nb-1 are
    written with the backward of the bilinear align_corners=True upsample, the
    others left as they are.  In place; returns nothing."""
    if not (isinstance(g0, torch.Tensor) and g0.is_cuda and g0.dtype == torch.float16 and g0.is_contiguous() and
            g0.dim() == 4 and g0.shape[-1] == 64):
        raise RuntimeError("g0 must be a contiguous [nb, H, W, 64] float16 device tensor (HIP path, no CPU fallback)")
    nb, H, W, _ = g0.shape
    if not (isinstance(grad_feat, torch.Tensor) and grad_feat.is_cuda and grad_feat.dtype == torch.float32 and
            grad_feat.is_contiguous() and grad_feat.dim() == 4 and grad_feat.shape[1] == 32 and
            grad_feat.device == g0.device):
        raise RuntimeError("grad_feat must be a contiguous [B, 32, h, w] float32 tensor on g0's device")
    B, _, h, w = grad_feat.shape
    with torch.cuda.device(g0.device):
        rc = _lib.load().sfm_dep_context_unpack_grad_f16(_lib.ptr(g0), B, int(b0), nb, 32, h, w, H, W,
                                                         _lib.ptr(grad_feat), _lib.stream_ptr(g0.device))
        _lib.check(rc, "sfm_dep_context_unpack_grad_f16")


class _DepContextStack(torch.autograd.Function):
    @staticmethod
    def forward(fctx, dep_convs, nb_max, depth, feat, image, *weights):
        B, _, H, W = depth.shape
        h, w = feat.shape[2:]
        dev = depth.device
        packed = pack_context_stack(dep_convs, dev, "fp16")
        lib = _lib.load()
        depth32 = depth.detach().contiguous()
        feat_c = feat.detach().contiguous()
        image32 = image.detach().float().contiguous()
        relu_out = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        saved = []                              # per chunk: the seven stages' float16 inputs
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            for b0 in range(0, B, nb_max):
                nb = min(nb_max, B - b0)
                x = torch.empty((nb, H, W, 64), dtype=torch.float16, device=dev)
                _lib.check(lib.sfm_dep_context_pack_f16(_lib.ptr(depth32), _lib.ptr(feat_c), _FEAT_DTYPE[feat_c.dtype],
                                                        _lib.ptr(image32), B, b0, nb, 32, h, w, H, W, _lib.ptr(x),
                                                        stream), "sfm_dep_context_pack")
                # the last stage without its residual, so that its ReLU output is kept; the fp32 "+ depth"
                # below gives the bits of the fused form.  A chunk writes a buffer of its own, 16-byte aligned.
                last = relu_out if nb == B else torch.empty((nb, 1, H, W), dtype=torch.float32, device=dev)
                saved.append(_run_stack(lib.sfm_conv2_f16, packed, x, nb, H, W, stream, None, last, None))
                if nb != B:
                    relu_out[b0:b0 + nb].copy_(last)
        fctx.saved, fctx.relu_out, fctx.nb_max = saved, relu_out, nb_max
        fctx.meta = [(lay["cin"], lay["cout"], lay["dilation"], lay["relu"]) for lay in packed]
        fctx.feat_shape, fctx.feat_dtype = tuple(feat.shape), feat.dtype
        fctx.save_for_backward(*weights)
        return relu_out + depth32

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad):
        weights = fctx.saved_tensors
        B, _, H, W = grad.shape
        dev = grad.device
        go = grad.detach().float().contiguous()
        nb_max, meta = fctx.nb_max, fctx.meta
        wds = [pack_dgrad_weights2(wt.detach().float()).half().contiguous() for wt in weights]
        gws = [None] * len(weights)
        grad_feat = torch.empty(fctx.feat_shape, dtype=torch.float32, device=dev)
        for k, b0 in enumerate(range(0, B, nb_max)):        # ascending pair order
            nb = min(nb_max, B - b0)
            g = _stack_backward(fctx.saved[k], go[b0:b0 + nb, 0], fctx.relu_out[b0:b0 + nb, 0], meta, wds, gws)
            dep_context_unpack_grad(g, b0, grad_feat)
            fctx.saved[k] = None                            # a chunk's activations are done with
        out_w = [unpack_wgrad2(gw, m[1], m[0]).to(wt.dtype) for gw, m, wt in zip(gws, meta, weights)]
        # depth: the "+ depth" residual alone (the cat reads depth.detach()); image: none
        return (None, None, grad, grad_feat.to(fctx.feat_dtype), None) + tuple(out_w)


def dep_context_refine_autograd(dep_convs, depth, feat, image, max_scratch_bytes=1 << 30):
    """``dep_context_refine`` (float16) with a backward on libsfm_hip: one
    autograd function over the whole full-resolution stack
    (PSNet.py:218-221), depth [B, 1, H, W] fp32, feat [B, 32, h, w] float16,
    bfloat16 or float32, image [B, 3, H, W] -> [B, 1, H, W] fp32, the bits of
    ``dep_context_refine(dep_convs, depth, feat, image, "fp16")``.

    Forward: the same ``sfm_dep_context_pack_f16`` and seven
    ``sfm_conv2_f16`` launches per chunk of ``pairs_per_chunk`` whole pairs;
    every stage's float16 input is kept, and the last stage runs without its
    residual so that its ReLU output is kept too (the fp32 "+ depth" is a
    torch add).  Backward, per chunk in ascending pair order and from the last
    stage to the first: ``sfm_conv2_wgrad_f16``, ``sfm_conv2_dgrad_f16`` masked
    by the saved activation (unmasked for the first stage), then
    ``sfm_dep_context_unpack_grad_f16``, the bilinear upsample's backward.

    Gradients: the seven Conv2d weights (float32, the parameters' layout,
    added over the chunks in fp32); ``feat`` in its own dtype; ``depth`` the
    upstream gradient unchanged -- the "+ depth" of PSNet.py:221; the copy of
    depth inside the cat is detached in the reference and gets nothing;
    ``image`` none.  The ``feat`` and ``depth`` gradients have the same bits
    for any chunking.

    Memory: the saved activations are 64 + 128 + 128 + 128 + 96 + 64 + 32 =
    640 float16 channels, 1280 bytes per full-resolution pixel, for every pair
    until the backward has run: about 0.6 GB per KITTI pair (376 x 1242);
    ``max_scratch_bytes`` bounds only the chunk's transient buffers.

    The upstream gradient is cast to float16 before the last stage's
    backward: a mean loss over a KITTI image's 467 k pixels gives gradients of
    2e-6 a pixel, below float16's normal range, so train with the GradScaler
    the reference already uses under MIXED_PREC.

    Refused with a named reason: CPU tensors, a call outside float16 CUDA
    autocast, a non-stock layout (``dep_stock_layout``), any BatchNorm2d stage
    (in training mode its batch statistics have no backward here; in eval mode
    the folded affine has none either), and a weight that is not float32 on
    the tensors' device."""
    _check_dep_context("dep_context_refine_autograd", dep_convs, depth, feat, image, autocast=True)
    weights = _trainable(_stages(dep_convs), depth.device)
    B, _, H, W = depth.shape
    nb_max = pairs_per_chunk(B, H, W, max_scratch_bytes)
    return _DepContextStack.apply(dep_convs, nb_max, depth, feat, image, *weights)
