"""PSNet's feature CNN on the gfx950 matrix cores.

The reference extracts 32-channel quarter-resolution features from every
image with PSMNet's SPP network (models/submodule.py:108-184
``feature_extraction``; ``sfm_amd.psnet.FeatureExtraction`` here): a stride-2
stem, four stages of residual blocks, four average-pool pyramid branches
upsampled back, and a 320 -> 128 -> 32 fusion.

``feature_extract`` runs it on libsfm_hip: one ``sfm_image_pack_f16``, every
Conv2d as an ``sfm_conv2x_f16`` launch (float16 channels-last activations and
weights, fp32 accumulation, BatchNorm2d folded in eval mode, the ReLU and the
block's "+ x" fused into the epilogue, ``downsample`` as a 1 x 1 launch feeding
that residual), four ``sfm_avgpool_f16``, one ``sfm_spp_pack_f16`` (the bilinear
upsamples and the cat) -- the precision torch computes this network at under
``cfg.MIXED_PREC`` autocast (SFMnet.py:164).  There is no PyTorch fallback:
without libsfm_hip.so or a GPU the call raises.

``conv2x_autograd`` is one raw Conv2d of this layer set with a backward, the
building block for training the CNN under float16 autocast (the reference
trains in ``model.train()``, main.py:304): ``sfm_conv2x_f16`` forward,
``sfm_conv2x_wgrad_f16`` and ``sfm_conv2x_dgrad_f16`` backward
(csrc/feature_bwd.hip).  ``batchnorm2_act_autograd`` is what stands between
two of them: BatchNorm2d, ReLU and the residual add in float16 in both
directions (csrc/bn2.hip: sfm_bn2_stats_f16, sfm_bn2_apply_f16,
sfm_bn2_backward_f16); ``convbn2_autograd`` is one reference ``convbn`` and
``basic_block_autograd`` one ``BasicBlock`` on the two.  The whole CNN on them
(the pools' and the SPP upsample's backward) is not built yet.
"""
import ctypes
import weakref

import torch
import torch.nn as nn

from . import _lib

MIN_MAP = 32            # AvgPool2d(32) needs a 32 x 32 quarter-resolution map


class FeatureLayoutError(RuntimeError):
    """The module is not the stock FeatureExtraction graph ``feature_extract`` runs."""


def _half(n):
    return (n - 1) // 2 + 1


def feature_hw(image_hw):
    """Quarter-resolution map size of the CNN for an image (two stride-2 convs)."""
    return _half(_half(image_hw[0])), _half(_half(image_hw[1]))


def _conv_bn(seq, cin, cout, k, stride, dilation, what, bn=True):
    """(conv, bn) of a stock conv-BN pair, or FeatureLayoutError naming what differs."""
    mods = list(seq) if isinstance(seq, nn.Sequential) else [seq]
    if len(mods) != (2 if bn else 1) or not isinstance(mods[0], nn.Conv2d) or \
            (bn and not isinstance(mods[1], nn.BatchNorm2d)):
        raise FeatureLayoutError(f"{what}: expected Conv2d{' + BatchNorm2d' if bn else ''}")
    conv = mods[0]
    pad = dilation if k == 3 else 0
    if (conv.in_channels, conv.out_channels) != (cin, cout):
        raise FeatureLayoutError(f"{what}: {conv.in_channels} -> {conv.out_channels} channels, expected {cin} -> {cout}")
    if tuple(conv.kernel_size) != (k, k):
        raise FeatureLayoutError(f"{what}: kernel size {tuple(conv.kernel_size)}, expected {k} x {k}")
    if tuple(conv.stride) != (stride, stride):
        raise FeatureLayoutError(f"{what}: stride {tuple(conv.stride)}, expected {stride}")
    if tuple(conv.dilation) != (dilation, dilation):
        raise FeatureLayoutError(f"{what}: dilation {tuple(conv.dilation)}, expected {dilation}")
    if tuple(conv.padding) != (pad, pad) or conv.padding_mode != "zeros":
        raise FeatureLayoutError(f"{what}: padding {conv.padding}, expected {pad} (zeros)")
    if conv.groups != 1:
        raise FeatureLayoutError(f"{what}: grouped convolutions are not built")
    if conv.bias is not None:
        raise FeatureLayoutError(f"{what}: a Conv2d bias is not built (convbn has none)")
    if not bn:
        return conv, None
    b = mods[1]
    if b.num_features != cout or not b.track_running_stats or b.running_mean is None or b.running_var is None:
        raise FeatureLayoutError(f"{what}: BatchNorm2d without running statistics cannot be folded")
    return conv, b


def _plan(module):
    """The CNN as (conv, bn, relu) stages in execution order, or
    FeatureLayoutError: {"first": [3], "layers": [[(conv1, conv2, downsample
    or None)] x blocks] x 4, "branches": [(pool, stage)] x 4 (branch1..4),
    "last": [2]}."""
    from .psnet import FeatureExtraction, _Residual
    if type(module) is not FeatureExtraction:
        raise FeatureLayoutError(f"{type(module).__name__} is not sfm_amd.psnet.FeatureExtraction")
    want = ["firstconv"] + [s[0] for s in module.STAGES] + [f"branch{i + 1}" for i in range(4)] + ["lastconv"]
    names = [n for n, _ in module.named_children()]
    if names != want:
        raise FeatureLayoutError(f"children {names}, expected {want}")
    if tuple(module.STAGES) != FeatureExtraction.STAGES or tuple(module.POOLS) != FeatureExtraction.POOLS:
        raise FeatureLayoutError("STAGES / POOLS differ from the stock plan")
    fc = module.firstconv
    if not isinstance(fc, nn.Sequential) or len(fc) != 6 or not all(isinstance(fc[i], nn.ReLU) for i in (1, 3, 5)):
        raise FeatureLayoutError("firstconv: expected three conv-BN + ReLU stages")
    first = [_conv_bn(fc[0], 3, 32, 3, 2, 1, "firstconv.0") + (True,),
             _conv_bn(fc[2], 32, 32, 3, 1, 1, "firstconv.2") + (True,),
             _conv_bn(fc[4], 32, 32, 3, 1, 1, "firstconv.4") + (True,)]
    layers, cin = [], 32
    for name, ch, blocks, stride, dil in FeatureExtraction.STAGES:
        seq = getattr(module, name)
        if not isinstance(seq, nn.Sequential) or len(seq) != blocks:
            raise FeatureLayoutError(f"{name}: expected {blocks} residual blocks")
        blks = []
        for i, blk in enumerate(seq):
            what = f"{name}.{i}"
            if type(blk) is not _Residual:
                raise FeatureLayoutError(f"{what}: {type(blk).__name__} is not the stock residual block")
            s = stride if i == 0 else 1
            c1 = blk.conv1
            if not isinstance(c1, nn.Sequential) or len(c1) != 2 or not isinstance(c1[1], nn.ReLU):
                raise FeatureLayoutError(f"{what}.conv1: expected conv-BN + ReLU")
            a = _conv_bn(c1[0], cin, ch, 3, s, dil, what + ".conv1") + (True,)
            b = _conv_bn(blk.conv2, ch, ch, 3, 1, dil, what + ".conv2") + (False,)
            need_ds = s != 1 or cin != ch
            if (blk.downsample is not None) != need_ds:
                raise FeatureLayoutError(f"{what}: downsample {'missing' if need_ds else 'unexpected'}")
            ds = _conv_bn(blk.downsample, cin, ch, 1, s, 1, what + ".downsample") + (False,) if need_ds else None
            blks.append((a, b, ds))
            cin = ch
        layers.append(blks)
    branches = []
    for i, p in enumerate(FeatureExtraction.POOLS):
        br = getattr(module, f"branch{i + 1}")
        what = f"branch{i + 1}"
        if not isinstance(br, nn.Sequential) or len(br) != 3 or not isinstance(br[0], nn.AvgPool2d) or \
                not isinstance(br[2], nn.ReLU):
            raise FeatureLayoutError(f"{what}: expected AvgPool2d + conv-BN + ReLU")
        pool = br[0]
        ks = pool.kernel_size if isinstance(pool.kernel_size, tuple) else (pool.kernel_size,) * 2
        st = pool.stride if isinstance(pool.stride, tuple) else (pool.stride,) * 2
        pd = pool.padding if isinstance(pool.padding, tuple) else (pool.padding,) * 2
        if tuple(ks) != (p, p) or tuple(st) != (p, p) or tuple(pd) != (0, 0) or pool.ceil_mode or \
                pool.divisor_override is not None:
            raise FeatureLayoutError(f"{what}: AvgPool2d {ks} stride {st}, expected {p} x {p} stride {p}")
        branches.append((p, _conv_bn(br[1], 128, 32, 1, 1, 1, what + ".1") + (True,)))
    lc = module.lastconv
    if not isinstance(lc, nn.Sequential) or len(lc) != 3 or not isinstance(lc[1], nn.ReLU):
        raise FeatureLayoutError("lastconv: expected conv-BN + ReLU + Conv2d")
    last = [_conv_bn(lc[0], 320, 128, 3, 1, 1, "lastconv.0") + (True,),
            _conv_bn(lc[2], 128, 32, 1, 1, 1, "lastconv.2", bn=False) + (False,)]
    return dict(first=first, layers=layers, branches=branches, last=last)


def feature_layout_ok(module):
    """Whether ``module`` is exactly the stock FeatureExtraction graph: its
    named children, every Conv2d's kernel, stride, padding, dilation, groups
    and lack of bias, running statistics on every BatchNorm2d, the pool sizes
    and the channel plan.  Anything else (another class, a callable) is False."""
    try:
        _plan(module)
    except FeatureLayoutError:
        return False
    return True


def _pad32(n):
    return (n + 31) // 32 * 32


def pack_weights2x(weight, dtype=None):
    """A Conv2d parameter [cout, cin, k, k] as the kernels read it: [k^2,
    cout_pad, cin_pad] (tap = kh*k + kw), rows beyond cout and columns beyond
    cin zero, in ``dtype`` (the parameter's own by default; the values are
    rounded to nearest even on the way in).  Pure torch, any device."""
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    wp = weight.new_zeros(k * k, _pad32(cout), _pad32(cin), dtype=dtype)
    wp[:, :cout, :cin] = weight.permute(2, 3, 0, 1).reshape(k * k, cout, cin)
    return wp


def _fold_stage(conv, bn, relu, device, dtype):
    """One stage as a launch reads it: the packed weight in ``dtype`` and the
    fp32 scale / bias [cout_pad] of BatchNorm2d folded with its running
    statistics (eval mode), 1 / 0 without one.  Computed in float32 on the
    CPU, then moved to ``device``."""
    w = conv.weight.detach().float().cpu()                         # [cout, cin, k, k]
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    cout_pad, cin_pad = _pad32(cout), _pad32(cin)
    sc, bi = torch.ones(cout_pad), torch.zeros(cout_pad)
    if bn is not None:
        g = torch.ones(cout) if bn.weight is None else bn.weight.detach().float().cpu()
        b = torch.zeros(cout) if bn.bias is None else bn.bias.detach().float().cpu()
        scale = g / torch.sqrt(bn.running_var.detach().float().cpu() + bn.eps)
        sc[:cout] = scale
        bi[:cout] = b - bn.running_mean.detach().float().cpu() * scale
    return dict(w=pack_weights2x(w, dtype).to(device), scale=sc.to(device), bias=bi.to(device),
                cin=cin, cin_pad=cin_pad, cout=cout, cout_pad=cout_pad, ksize=k, stride=int(conv.stride[0]),
                dilation=int(conv.dilation[0]), relu=relu)


_PACKED = weakref.WeakKeyDictionary()      # module -> (key, packed)


def pack_feature_extraction(module, device):
    """Packed float16 weights [k^2][cout_pad][cin_pad] (tap = kh*k + kw; rows
    beyond cout and columns beyond cin zero) and the folded fp32 scale / bias
    [cout_pad] of every Conv2d of the stock CNN, in ``_plan``'s structure.
    BatchNorm2d folds with its running statistics (eval mode), as
    ``pack_context_stack`` folds it.  Cached until a parameter or buffer
    changes."""
    plan = _plan(module)
    key = (str(device),) + tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))
    hit = _PACKED.get(module)
    if hit is not None and hit[0] == key:
        return hit[1]

    def fold(stage):
        return _fold_stage(*stage, device, torch.float16)
    with torch.no_grad():
        packed = dict(
            first=[fold(s) for s in plan["first"]],
            layers=[[tuple(None if s is None else fold(s) for s in blk) for blk in blks] for blks in plan["layers"]],
            branches=[(p, fold(s)) for p, s in plan["branches"]],
            last=[fold(s) for s in plan["last"]])
    _PACKED[module] = (key, packed)
    return packed


# --- single launches ------------------------------------------------------------------
def _check_act(t, name, channels=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and t.dim() == 4):
        raise RuntimeError(f"{name} must be a contiguous float16 device tensor [images, h, w, channels]")
    if channels is not None and t.shape[3] != channels:
        raise RuntimeError(f"{name} must have {channels} channels")


def conv2x_f16(x, weights, scale, bias, ksize=3, stride=1, dilation=1, relu=True, residual=None):
    """One fused layer (sfm_conv2x_f16): x [images, h, w, cin] float16,
    weights [ksize^2, cout, cin] float16, scale / bias [cout] fp32, residual
    [images, hout, wout, cout] float16 or None -> [images, hout, wout, cout]
    float16."""
    _check_act(x, "x")
    n, h, w, cin = x.shape
    if not (isinstance(weights, torch.Tensor) and weights.is_cuda and weights.dtype == torch.float16 and
            weights.is_contiguous() and weights.dim() == 3 and weights.shape[0] == ksize * ksize and
            weights.shape[2] == cin):
        raise RuntimeError(f"weights must be a contiguous float16 device tensor [{ksize * ksize}, cout, {cin}]")
    cout = weights.shape[1]
    scale = scale.to(device=x.device, dtype=torch.float32).contiguous()
    bias = bias.to(device=x.device, dtype=torch.float32).contiguous()
    if scale.numel() != cout or bias.numel() != cout:
        raise RuntimeError(f"scale and bias must have {cout} entries")
    if stride not in (1, 2):
        raise RuntimeError("stride must be 1 or 2")
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if residual is not None:
        _check_act(residual, "residual", cout)
        if tuple(residual.shape) != (n, ho, wo, cout):
            raise RuntimeError(f"residual must be [{n}, {ho}, {wo}, {cout}]")
    out = torch.empty((n, ho, wo, cout), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().sfm_conv2x_f16(_lib.ptr(x), n, cin, h, w, _lib.ptr(weights), cout, int(ksize), int(stride),
                                        int(dilation), _lib.ptr(scale), _lib.ptr(bias), 1 if relu else 0,
                                        _lib.ptr(residual), _lib.ptr(out), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_conv2x_f16")
    return out


def image_pack_f16(image):
    """[B, 3, H, W] float32 -> [B, H, W, 32] float16, channels 3..31 zero (sfm_image_pack_f16)."""
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.float32 and
            image.is_contiguous() and image.dim() == 4 and image.shape[1] == 3):
        raise RuntimeError("image must be a contiguous float32 device tensor [B, 3, H, W]")
    B, _, H, W = image.shape
    out = torch.empty((B, H, W, 32), dtype=torch.float16, device=image.device)
    with torch.cuda.device(image.device):
        _lib.check(_lib.load().sfm_image_pack_f16(_lib.ptr(image), B, H, W, _lib.ptr(out),
                                                  _lib.stream_ptr(image.device)), "sfm_image_pack_f16")
    return out


def avgpool_f16(x, pool):
    """AvgPool2d(pool, stride pool) of [images, h, w, C] float16 (sfm_avgpool_f16)."""
    _check_act(x, "x")
    n, h, w, C = x.shape
    if h < pool or w < pool:
        raise RuntimeError(f"a {h} x {w} map holds no {pool} x {pool} window")
    out = torch.empty((n, h // pool, w // pool, C), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().sfm_avgpool_f16(_lib.ptr(x), n, h, w, C, int(pool), _lib.ptr(out),
                                               _lib.stream_ptr(x.device)), "sfm_avgpool_f16")
    return out


def spp_pack_f16(raw, skip, branches):
    """cat(raw, skip, up(branches[0]), .. up(branches[3])) channels-last
    (sfm_spp_pack_f16): raw [images, h, w, 64], skip [images, h, w, 128],
    branches four [images, hi, wi, 32] maps in cat order (branch4 .. branch1)
    -> [images, h, w, 320] float16."""
    _check_act(raw, "raw", 64)
    _check_act(skip, "skip", 128)
    n, h, w, _ = raw.shape
    if tuple(skip.shape[:3]) != (n, h, w) or len(branches) != 4:
        raise RuntimeError("skip must match raw, with four branch maps")
    for b in branches:
        _check_act(b, "branch", 32)
        if b.shape[0] != n:
            raise RuntimeError("every branch map must hold the same images")
    out = torch.empty((n, h, w, 320), dtype=torch.float16, device=raw.device)
    ptrs = (ctypes.c_void_p * 4)(*[b.data_ptr() for b in branches])
    bh = (ctypes.c_int * 4)(*[b.shape[1] for b in branches])
    bw = (ctypes.c_int * 4)(*[b.shape[2] for b in branches])
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().sfm_spp_pack_f16(_lib.ptr(raw), _lib.ptr(skip), ptrs, bh, bw, n, h, w, _lib.ptr(out),
                                                _lib.stream_ptr(raw.device)), "sfm_spp_pack_f16")
    return out


# --- the whole CNN ----------------------------------------------------------------------
def scratch_bytes_per_image(H, W):
    """Upper bound on the float16 activations alive at once for one image: the
    packed image next to the stem's first output; three half-resolution
    32-channel maps (a block's input, middle and output); at quarter resolution
    raw, three 128-channel maps, the four branch maps (at most 1/16 of the map
    each) and lastconv's 320-channel input."""
    H2, W2 = _half(H), _half(W)
    h, w = _half(H2), _half(W2)
    return 2 * max(H * W * 32 + H2 * W2 * 32, 3 * H2 * W2 * 32, h * w * (64 + 3 * 128 + 320 + 8))


def images_per_chunk(batch, H, W, max_scratch_bytes):
    """The most images whose activations fit ``max_scratch_bytes``; at least one, at most batch."""
    return max(1, min(int(batch), int(max_scratch_bytes) // scratch_bytes_per_image(H, W)))


def _layer(x, lay, residual=None):
    return conv2x_f16(x, lay["w"], lay["scale"], lay["bias"], lay["ksize"], lay["stride"], lay["dilation"],
                      relu=lay["relu"], residual=residual)


def _run(packed, image):
    x = image_pack_f16(image)
    for lay in packed["first"]:
        x = _layer(x, lay)
    raw = None
    for i, blks in enumerate(packed["layers"]):
        for c1, c2, ds in blks:
            x = _layer(_layer(x, c1), c2, residual=x if ds is None else _layer(x, ds))
        if i == 1:
            raw = x
    pyr = [_layer(avgpool_f16(x, p), lay) for p, lay in packed["branches"]]        # branch1..4
    y = spp_pack_f16(raw, x, pyr[::-1])
    for lay in packed["last"]:
        y = _layer(y, lay)
    return y


def feature_extract(module, image, max_scratch_bytes=1 << 30):
    """``module(image)`` for the stock FeatureExtraction in eval mode
    (submodule.py:161-184): image [B, 3, H, W] (any float dtype) -> [B, 32,
    h, w] float16, contiguous.  The images go through in chunks of
    ``images_per_chunk``; every image is computed on its own, so the result
    depends neither on the chunking nor on the batch.  No PyTorch fallback:
    CPU tensors raise; so does a quarter-resolution map under 32 x 32 (torch's
    AvgPool2d(32) fails there too)."""
    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        raise RuntimeError("feature_extract needs a device tensor (HIP path, no CPU fallback): image")
    if image.dim() != 4 or image.shape[1] != 3 or not image.is_floating_point():
        raise RuntimeError("image must be [B, 3, H, W] floating point")
    if not feature_layout_ok(module):
        _plan(module)           # raises the named reason
    B, _, H, W = image.shape
    h, w = feature_hw((H, W))
    if h < MIN_MAP or w < MIN_MAP:
        raise RuntimeError(f"the quarter-resolution map {h} x {w} is under {MIN_MAP} x {MIN_MAP}: branch1's "
                           f"AvgPool2d({MIN_MAP}) has no window")
    dev = image.device
    packed = pack_feature_extraction(module, dev)
    image = image.detach().float().contiguous()
    nb_max = images_per_chunk(B, H, W, max_scratch_bytes)
    if nb_max >= B:
        out = _run(packed, image)
    else:
        out = torch.empty((B, h, w, 32), dtype=torch.float16, device=dev)
        for b0 in range(0, B, nb_max):
            part = image[b0:b0 + nb_max]
            if part.data_ptr() % 16:
                part = part.clone()
            out[b0:b0 + nb_max].copy_(_run(packed, part))
    return out.permute(0, 3, 1, 2).contiguous()


# --- the CNN's backward in float16 (csrc/feature_bwd.hip) ---------------------------
def pack_dgrad_weights2x(weight):
    """The weights that turn a layer's kernel into its data gradient
    (sfm_conv2x_dgrad_f16): Wd[t][ci][co] = W[co][ci][k^2 - 1 - t] as [k^2,
    cin_pad, cout_pad] for a Conv2d parameter [cout, cin, k, k], rows beyond
    cin and columns beyond cout zero.  Pure torch, any device and dtype."""
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    wd = weight.new_zeros(k * k, _pad32(cin), _pad32(cout))
    wd[:, :cin, :cout] = weight.reshape(cout, cin, k * k).flip(2).permute(2, 1, 0)
    return wd


def unpack_wgrad2x(gwp, cout, cin, ksize):
    """sfm_conv2x_wgrad_f16's [k^2, cout_pad, cin_pad] result in the Conv2d
    parameter's layout [cout, cin, k, k]; the padded rows and columns are
    dropped.  Pure torch."""
    return gwp[:, :cout, :cin].permute(1, 2, 0).reshape(cout, cin, ksize, ksize).contiguous()


def _check_layer(ksize, stride, dilation):
    if ksize not in (1, 3) or stride not in (1, 2):
        raise RuntimeError("ksize must be 3 or 1 and stride 1 or 2")
    if not 1 <= int(dilation) <= 16 or (dilation != 1 and (ksize != 3 or stride != 1)):
        raise RuntimeError("dilation must be 1..16, and 1 for a 1 x 1 or stride 2 conv")


def conv2x_wgrad_f16(x, grad_out, ksize=3, stride=1, dilation=1):
    """sfm_conv2x_wgrad_f16: x [images, hin, win, cin] and grad_out [images,
    hout, wout, cout], contiguous float16 device tensors -> [ksize^2, cout,
    cin] float32, reproducible bit for bit."""
    _check_act(x, "x")
    _check_act(grad_out, "grad_out")
    _check_layer(ksize, stride, dilation)
    n, h, w, cin = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if tuple(grad_out.shape[:3]) != (n, ho, wo):
        raise RuntimeError(f"grad_out must be [{n}, {ho}, {wo}, cout]")
    cout = grad_out.shape[3]
    lib = _lib.load()
    gw = torch.empty((ksize * ksize, cout, cin), dtype=torch.float32, device=x.device)
    need = lib.sfm_conv2x_wgrad_f16_workspace_bytes(n, cin, cout, h, w, int(ksize), int(stride))
    ws = torch.empty(max(16, need), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_conv2x_wgrad_f16(_lib.ptr(x), _lib.ptr(grad_out), n, cin, cout, h, w, int(ksize), int(stride),
                                      int(dilation), _lib.ptr(gw), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_conv2x_wgrad_f16")
    return gw


def conv2x_dgrad_f16(grad_out, weights_d, in_hw, ksize=3, stride=1, dilation=1):
    """sfm_conv2x_dgrad_f16: grad_out [images, hout, wout, cout] float16,
    weights_d [ksize^2, cin_pad, cout] float16 (``pack_dgrad_weights2x``),
    in_hw the layer input's (hin, win) -> [images, hin, win, cin_pad]
    float16."""
    _check_act(grad_out, "grad_out")
    _check_layer(ksize, stride, dilation)
    n, ho, wo, cout = grad_out.shape
    if not (isinstance(weights_d, torch.Tensor) and weights_d.is_cuda and weights_d.dtype == torch.float16 and
            weights_d.is_contiguous() and weights_d.dim() == 3 and weights_d.shape[0] == ksize * ksize and
            weights_d.shape[2] == cout):
        raise RuntimeError(f"weights_d must be a contiguous float16 device tensor [{ksize * ksize}, cin_pad, {cout}]")
    cin = weights_d.shape[1]
    h, w = int(in_hw[0]), int(in_hw[1])
    out = torch.empty((n, h, w, cin), dtype=torch.float16, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        rc = _lib.load().sfm_conv2x_dgrad_f16(_lib.ptr(grad_out), n, cout, ho, wo, _lib.ptr(weights_d), cin, h, w,
                                              int(ksize), int(stride), int(dilation), _lib.ptr(out),
                                              _lib.stream_ptr(grad_out.device))
        _lib.check(rc, "sfm_conv2x_dgrad_f16")
    return out


_UNIT = {}      # (device, cout_pad) -> (ones, zeros): the unit affine of the raw convolution


def _unit_affine(device, n):
    key = (str(device), n)
    if key not in _UNIT:
        _UNIT[key] = (torch.ones(n, dtype=torch.float32, device=device), torch.zeros(n, dtype=torch.float32, device=device))
    return _UNIT[key]


class _Conv2x(torch.autograd.Function):
    @staticmethod
    def forward(fctx, x, weight, stride, dilation):
        k = weight.shape[2]
        wp = pack_weights2x(weight.detach(), torch.float16)
        one, zero = _unit_affine(x.device, wp.shape[1])
        fctx.save_for_backward(x, weight)
        fctx.layer = (k, int(stride), int(dilation))
        return conv2x_f16(x, wp, one, zero, k, int(stride), int(dilation), relu=False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad):
        x, weight = fctx.saved_tensors
        k, stride, dilation = fctx.layer
        gy = grad.to(torch.float16).contiguous()
        gx = gw = None
        if fctx.needs_input_grad[0]:
            wd = pack_dgrad_weights2x(weight.detach().float()).to(torch.float16).contiguous()
            gx = conv2x_dgrad_f16(gy, wd, x.shape[1:3], k, stride, dilation)
        if fctx.needs_input_grad[1]:
            gwp = conv2x_wgrad_f16(x, gy, k, stride, dilation)
            gw = unpack_wgrad2x(gwp, weight.shape[0], weight.shape[1], k).to(weight.dtype)
        return gx, gw, None, None


def conv2x_autograd(x, weight, stride=1, dilation=1):
    """The raw convolution of one layer with a backward on libsfm_hip: x [n, h,
    w, cin_pad] contiguous float16 on the device, weight the Conv2d parameter
    [cout, cin, k, k] (k 3 or 1; any float dtype) -> [n, hout, wout, cout_pad]
    float16, the bits of ``conv2x_f16`` on the packed float16 weights with
    scale 1, bias 0, no ReLU and no residual.  Backward: ``sfm_conv2x_dgrad_f16``
    for x and ``sfm_conv2x_wgrad_f16`` for weight, each run only when its input
    needs a gradient; the weight gradient comes back in the parameter's layout
    and dtype."""
    _check_act(x, "x")
    if not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dim() == 4 and weight.is_floating_point() and
            weight.shape[2] == weight.shape[3] and weight.shape[2] in (1, 3)):
        raise RuntimeError("weight must be a floating-point device tensor [cout, cin, k, k], k 3 or 1")
    if _pad32(weight.shape[1]) != x.shape[3]:
        raise RuntimeError(f"x has {x.shape[3]} channels, the weight's {weight.shape[1]} pad to {_pad32(weight.shape[1])}")
    _check_layer(int(weight.shape[2]), stride, dilation)
    return _Conv2x.apply(x, weight, int(stride), int(dilation))



# --- BatchNorm2d, ReLU and the residual add in float16 (csrc/bn2.hip) ----------------
BN2_CHANNELS = (32, 64, 128)


def _bn2_operand(t, name, like=None):
    _check_act(t, name)
    if t.shape[3] not in BN2_CHANNELS:
        raise RuntimeError(f"{name} must have 32, 64 or 128 channels")
    if like is not None and t.shape != like.shape:
        raise RuntimeError(f"{name} must have the shape of x")


def bn2_stats_f16(x, gamma, beta, eps=1e-5, running_mean=None, running_var=None, momentum=0.1, training=True):
    """sfm_bn2_stats_f16: x [n, h, w, C] float16 (channels last, C 32, 64 or
    128), gamma / beta and the running statistics [C] float32 on x's device ->
    stats [5, C] float32 (mean, biased variance, invstd, a, b).  In training
    mode the running statistics, where given, are updated in place; in eval
    mode they are read."""
    _bn2_operand(x, "x")
    lib = _lib.load()
    C = x.shape[3]
    pix = x.numel() // C
    stats = torch.empty((5, C), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(16, lib.sfm_bn2_stats_f16_workspace_bytes(pix, C, 1 if training else 0)), dtype=torch.uint8,
                     device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_bn2_stats_f16(_lib.ptr(x), pix, C, _lib.ptr(gamma), _lib.ptr(beta), float(eps),
                                   _lib.ptr(running_mean), _lib.ptr(running_var), float(momentum), 1 if training else 0,
                                   _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_bn2_stats_f16")
    if training:
        for r in (running_mean, running_var):       # written through the raw pointer: tell autograd and the pack keys
            if r is not None:
                torch.autograd.graph.increment_version(r)
    return stats


def bn2_apply_f16(x, stats, residual=None, relu=False):
    """sfm_bn2_apply_f16: f16(relu(fma(a, x, b)) + residual) with a, b from
    ``stats`` [5, C] float32; x and residual [n, h, w, C] float16."""
    _bn2_operand(x, "x")
    if residual is not None:
        _bn2_operand(residual, "residual", x)
    C = x.shape[3]
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = _lib.load().sfm_bn2_apply_f16(_lib.ptr(x), x.numel() // C, C, _lib.ptr(stats), _lib.ptr(residual),
                                           1 if relu else 0, _lib.ptr(out), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_bn2_apply_f16")
    return out


def bn2_backward_f16(x, grad_out, stats, relu=False, training=True, need_grad_x=True):
    """sfm_bn2_backward_f16 -> (grad_x float16 like x or None, grad_gamma_beta
    [2, C] float32: dgamma, dbeta), from x and ``stats`` alone."""
    _bn2_operand(x, "x")
    _bn2_operand(grad_out, "grad_out", x)
    lib = _lib.load()
    C = x.shape[3]
    pix = x.numel() // C
    gx = torch.empty_like(x) if need_grad_x else None
    ggb = torch.empty((2, C), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(16, lib.sfm_bn2_backward_f16_workspace_bytes(pix, C)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_bn2_backward_f16(_lib.ptr(x), _lib.ptr(grad_out), pix, C, _lib.ptr(stats), 1 if relu else 0,
                                      1 if training else 0, _lib.ptr(gx), _lib.ptr(ggb), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_bn2_backward_f16")
    return gx, ggb


class _BN2Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        training = bool(bn.training)
        stats = bn2_stats_f16(x, weight.detach(), bias.detach(), bn.eps, bn.running_mean, bn.running_var, bn.momentum,
                              training)
        if training:
            bn.num_batches_tracked.add_(1)
        out = bn2_apply_f16(x, stats, None if residual is None else residual.detach(), relu)
        ctx.save_for_backward(x, stats)
        ctx.relu, ctx.training, ctx.param_dtypes = relu, training, (weight.dtype, bias.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        gx = gw = gb = None
        if need_x or need_w or need_b:
            gx, ggb = bn2_backward_f16(x, g.to(torch.float16).contiguous(), stats, ctx.relu, ctx.training, need_x)
            gw = ggb[0].to(ctx.param_dtypes[0]) if need_w else None
            gb = ggb[1].to(ctx.param_dtypes[1]) if need_b else None
        return gx, gw, gb, (g if need_r else None), None, None


def batchnorm2_act_autograd(x, bn, relu=False, residual=None):
    """``bn`` (an nn.BatchNorm2d of 32, 64 or 128 features), then ReLU if
    ``relu``, then ``+ residual``, on libsfm_hip in both directions: x and
    residual [n, h, w, C] float16 on the device, channels last -> the same
    shape, float16, rounded once (sfm_bn2_stats_f16, sfm_bn2_apply_f16).  The
    contract of ``regularize.batchnorm3_act_autograd``: the module's mode, eps,
    momentum and affine parameters are honoured; training mode takes batch
    statistics, updates the running statistics in place by torch's rule and
    increments num_batches_tracked; eval mode reads the running statistics.
    Only x and the 5 x C floats of statistics are saved; the backward
    (sfm_bn2_backward_f16) returns gradients for x, bn.weight, bn.bias and the
    residual (the output gradient itself), each only where needed.  A module
    that is not the stock affine one with running statistics and a fixed
    momentum, or that carries forward hooks, raises; so does a CPU tensor."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and
            x.shape[3] in BN2_CHANNELS):
        raise RuntimeError("batchnorm2_act_autograd needs a [n, h, w, C] float16 device tensor, C 32, 64 or 128 (HIP "
                           "path, no CPU fallback)")
    C = x.shape[3]
    if type(bn) is not nn.BatchNorm2d or bn.num_features != C:
        raise RuntimeError(f"bn must be an nn.BatchNorm2d of x's {C} channels")
    if not bn.affine or not bn.track_running_stats or bn.momentum is None or bn.running_mean is None:
        raise RuntimeError("bn must be the stock module: affine=True, track_running_stats=True and a fixed momentum")
    if bn._forward_hooks or bn._forward_pre_hooks:
        raise RuntimeError("bn carries forward hooks, which the HIP route would not call")
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if not (t.device == x.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("bn's parameters and running statistics must be float32 on x's device")
    if x.numel() // C < 2 and bn.training:
        raise RuntimeError("training-mode batch statistics need more than one value per channel")
    if residual is not None and not (isinstance(residual, torch.Tensor) and residual.is_cuda and
                                     residual.dtype == torch.float16 and residual.shape == x.shape):
        raise RuntimeError("residual must be a float16 device tensor of x's shape")
    return _BN2Act.apply(x.contiguous(), bn.weight, bn.bias, None if residual is None else residual.contiguous(), bn,
                         bool(relu))


def _convbn_layer(seq, what):
    """(conv, bn) of a reference convbn, checked by ``_conv_bn`` against its own
    Conv2d's geometry and by ``_check_layer`` against the layer set."""
    mods = list(seq) if isinstance(seq, nn.Sequential) else []
    if len(mods) != 2 or not isinstance(mods[0], nn.Conv2d):
        raise FeatureLayoutError(f"{what}: expected Conv2d + BatchNorm2d")
    c = mods[0]
    k, stride, dilation = int(c.kernel_size[0]), int(c.stride[0]), int(c.dilation[0])
    _check_layer(k, stride, dilation)
    conv, bn = _conv_bn(seq, c.in_channels, c.out_channels, k, stride, dilation, what)
    if conv.out_channels not in BN2_CHANNELS or conv.in_channels % 32:
        raise FeatureLayoutError(f"{what}: {conv.in_channels} -> {conv.out_channels} channels; the output must have 32, "
                                 f"64 or 128 and the input a multiple of 32")
    return conv, bn


def convbn2_autograd(x, seq, relu=False, residual=None):
    """One reference ``convbn`` (models/submodule.py:11-14: Sequential(Conv2d,
    BatchNorm2d), no conv bias) with a backward, all on libsfm_hip:
    ``conv2x_autograd`` on the Conv2d's weight, then ``batchnorm2_act_autograd``
    on the BatchNorm2d with the ReLU and the residual.  x [n, h, w, cin]
    float16 channels last on the device -> [n, hout, wout, cout] float16."""
    conv, bn = _convbn_layer(seq, "convbn")
    y = conv2x_autograd(x, conv.weight, int(conv.stride[0]), int(conv.dilation[0]))
    return batchnorm2_act_autograd(y, bn, relu, residual)


def basic_block_autograd(block, x):
    """One reference BasicBlock (models/submodule.py:22-44;
    ``sfm_amd.psnet._Residual``) with a backward, on ``convbn2_autograd``:
    conv1 + ReLU, conv2, the 1 x 1 ``downsample`` convbn of x where the block
    has one, and ``+ x`` with no ReLU after it (submodule.py:35-44).  x [n, h,
    w, cin] float16 channels last on the device -> [n, hout, wout, cout]
    float16.  No torch batch_norm or convolution runs on the device."""
    c1 = getattr(block, "conv1", None)
    if not isinstance(c1, nn.Sequential) or len(c1) != 2 or not isinstance(c1[1], nn.ReLU) or \
            not hasattr(block, "conv2") or not hasattr(block, "downsample"):
        raise FeatureLayoutError("block: expected conv1 = convbn + ReLU, conv2 = convbn and a downsample attribute")
    conv1, _ = _convbn_layer(c1[0], "block.conv1")
    conv2, _ = _convbn_layer(block.conv2, "block.conv2")
    if tuple(conv2.stride) != (1, 1) or conv2.in_channels != conv1.out_channels or \
            conv2.out_channels != conv1.out_channels:
        raise FeatureLayoutError("block.conv2: expected stride 1 and conv1's output channels on both sides")
    if block.downsample is None:
        if tuple(conv1.stride) != (1, 1) or conv1.in_channels != conv1.out_channels:
            raise FeatureLayoutError("block: a strided or widening block needs its downsample")
        shortcut = x
    else:
        ds, _ = _convbn_layer(block.downsample, "block.downsample")
        if tuple(ds.kernel_size) != (1, 1) or ds.stride != conv1.stride or ds.in_channels != conv1.in_channels or \
                ds.out_channels != conv1.out_channels:
            raise FeatureLayoutError("block.downsample: expected a 1 x 1 convbn of conv1's stride and channels")
        shortcut = convbn2_autograd(x, block.downsample)
    y = convbn2_autograd(x, c1[0], relu=True)
    return convbn2_autograd(y, block.conv2, residual=shortcut)
