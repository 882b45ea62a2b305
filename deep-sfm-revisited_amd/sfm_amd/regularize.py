"""PSNet 3-D cost regularisation on the gfx950 matrix cores.

Mirrors the cost-filtering stack of models/PSNet.py:79-102 (module layout,
so a PSNet state_dict's ``dres*`` / ``classify`` entries load unchanged) and
its application at PSNet.py:159-165:

    cost0 = dres0(cost)
    cost0 = dres1(cost0) + cost0   ... dres4
    cost0 = classify(cost0)                      # [B, 1, L, h, w]

``CostRegularization.forward`` runs the 12 Conv3d layers as
``sfm_conv3_f32x3`` launches (default ``precision="fp32x3"``: the
reference's fp32 activations and weights, each product formed from split-f16
operands on the f16 matrix cores; ``precision="fp32"`` is the same on the
f32 matrix cores, ``sfm_conv3_f32``), with
``precision="fp16"`` as ``sfm_conv3_f16`` launches (float16 channels-last
activations and weights, fp32 accumulation: the precision of the reference's
Conv3d layers under ``cfg.MIXED_PREC`` autocast, SFMnet.py:164) or, with
``precision="bf16"``, as ``sfm_conv3_bf16`` launches (the fastest opt-in,
8-bit mantissa).  BatchNorm3d is folded in eval mode, ReLU
and residual are fused into the epilogue.  There is no PyTorch fallback: without libsfm_hip.so or a GPU
the call raises.
"""
import math

import torch
import torch.nn as nn

from . import _lib
from .depth import depth_head
from .sweep import plane_sweep_cost, plane_sweep_cost_channels_last, quarter_intrinsics


_ACT_DTYPE = {"fp32": torch.float32, "fp32x3": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# sfm_conv3_f32x3 with a range flag re-runs a layer as sfm_conv3_f32 when its largest |activation| is below
# this (kX3AmaxMin in csrc/regularize.hip): there the split's low halves are subnormal f16
FP32X3_MIN_AMAX = 2.0 ** -3


def weight_exponent(w):
    """sfm_conv3_f32x3's weight scale: the power of two 2^e with 2^e max|w| in
    [2^13, 2^14) (the lo terms of the split stay in the f16 normal range, the
    hi terms far from its maximum), clamped to the ABI's [-24, 24]."""
    m = float(w.abs().max())
    if not (m > 0.0 and math.isfinite(m)):
        return 0
    return max(-24, min(24, 13 - math.frexp(m)[1] + 1))


def convbn_3d(in_planes, out_planes, kernel_size=3, stride=1, pad=1):
    """models/submodule.py:17-20."""
    return nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=kernel_size, padding=pad, stride=stride,
                                   bias=False),
                         nn.BatchNorm3d(out_planes))


_LP_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
_CL_NAME = dict(_LP_NAME)
_CL_NAME[torch.float32] = "f32"


def to_channels_last(cost, dtype=torch.bfloat16):
    """[B, C, L, h, w] fp32/bf16 (device) -> [B, L, h, w, C] ``dtype`` (bf16 or
    fp16, round to nearest even; or float32, sfm_to_channels_last_f32)."""
    if not (isinstance(cost, torch.Tensor) and cost.is_cuda) or cost.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("to_channels_last needs a float32 / bfloat16 device tensor")
    if dtype not in _CL_NAME:
        raise RuntimeError("to_channels_last writes bfloat16, float16 or float32")
    cost = cost.contiguous()
    B, C = cost.shape[:2]
    P = cost[0, 0].numel()
    out = torch.empty((B,) + tuple(cost.shape[2:]) + (C,), dtype=dtype, device=cost.device)
    fn = "sfm_to_channels_last_" + _CL_NAME[dtype]
    with torch.cuda.device(cost.device):
        _lib.check(getattr(_lib.load(), fn)(_lib.ptr(cost), 0 if cost.dtype == torch.float32 else 1,
                                            B, C, P, _lib.ptr(out), _lib.stream_ptr(cost.device)), fn)
    return out


def _conv3_lp(x, weights, scale, bias, residual, relu, cout, dtype):
    name = {torch.bfloat16: "bfloat16", torch.float16: "float16"}[dtype]
    for t, n in ((x, "x"), (weights, "weights")):
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise RuntimeError(f"{n} must be a contiguous {name} device tensor")
    B, L, h, w, cin = x.shape
    if tuple(weights.shape) != (27, 32, cin):
        raise RuntimeError(f"weights must be [27, 32, {cin}]")
    if residual is not None and (residual.dtype != dtype or tuple(residual.shape) != (B, L, h, w, 32)):
        raise RuntimeError(f"residual must be {name} [B, L, h, w, 32]")
    if cout == 32:
        out = torch.empty((B, L, h, w, 32), dtype=dtype, device=x.device)
    else:
        out = torch.empty((B, L, h, w), dtype=torch.float32, device=x.device)
    scale = scale.to(device=x.device, dtype=torch.float32).contiguous()
    bias = bias.to(device=x.device, dtype=torch.float32).contiguous()
    fn = "sfm_conv3_" + _LP_NAME[dtype]
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), fn)(_lib.ptr(x), B, cin, L, h, w, _lib.ptr(weights), _lib.ptr(scale),
                                      _lib.ptr(bias), None if residual is None else _lib.ptr(residual.contiguous()),
                                      1 if relu else 0, cout, _lib.ptr(out), _lib.stream_ptr(x.device))
        _lib.check(rc, fn)
    return out


def conv3_bf16(x, weights, scale, bias, residual=None, relu=False, cout=32):
    """One fused layer: x [B, L, h, w, Cin] bf16, weights [27, 32, Cin] bf16,
    scale/bias [32] fp32 -> [B, L, h, w, 32] bf16 (cout 32) or [B, L, h, w]
    fp32 (cout 1)."""
    return _conv3_lp(x, weights, scale, bias, residual, relu, cout, torch.bfloat16)


def conv3_f16(x, weights, scale, bias, residual=None, relu=False, cout=32):
    """``conv3_bf16`` with float16 activations, weights and residual
    (sfm_conv3_f16)."""
    return _conv3_lp(x, weights, scale, bias, residual, relu, cout, torch.float16)


def pack_weights(weight):
    """A Conv3d weight [cout, cin, 3, 3, 3] in sfm_conv3_*'s pack layout:
    [27, 32, cin], tap = (kd*3 + kh)*3 + kw, cout zero-padded to 32.  Pure
    torch, any device and dtype."""
    cout, cin = weight.shape[:2]
    wp = weight.new_zeros(27, 32, cin)
    wp[:, :cout] = weight.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    return wp


def pack_dgrad_weights(weight):
    """The weights that turn sfm_conv3_f16 into the layer's data gradient
    (sfm_hip.h): Wd[half][t][ci][co] = W[co][32 half + ci][26 - t] as
    [cin / 32, 27, 32, 32], co zero-padded to 32 -- one pack per 32-channel
    half of ci, each an ordinary 32 -> 32 layer on the output gradient.  Pure
    torch, any device and dtype."""
    cout, cin = weight.shape[:2]
    flipped = weight.reshape(cout, cin, 27).flip(2)                  # [co][ci][t] = W[co][ci][26 - t]
    wd = weight.new_zeros(cin // 32, 27, 32, 32)
    wd[..., :cout] = flipped.permute(2, 1, 0).reshape(27, cin // 32, 32, cout).permute(1, 0, 2, 3)
    return wd


def unpack_wgrad(gwp, cout, cin):
    """sfm_conv3_wgrad_f16's [27, 32, cin] result in the Conv3d parameter's
    layout [cout, cin, 3, 3, 3] (rows co >= cout belong to the padding and are
    dropped).  Pure torch."""
    return gwp[:, :cout].permute(1, 2, 0).reshape(cout, cin, 3, 3, 3).contiguous()


def conv3_wgrad_f16(x, grad_out):
    """sfm_conv3_wgrad_f16: x [B, L, h, w, cin] and grad_out [B, L, h, w, 32],
    contiguous float16 device tensors -> [27, 32, cin] float32, reproducible
    bit for bit."""
    for t, n in ((x, "x"), (grad_out, "grad_out")):
        if not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and t.dim() == 5):
            raise RuntimeError(f"{n} must be a contiguous 5-D float16 device tensor")
    B, L, h, w, cin = x.shape
    if tuple(grad_out.shape) != (B, L, h, w, 32):
        raise RuntimeError("grad_out must be [B, L, h, w, 32]")
    lib = _lib.load()
    gw = torch.empty((27, 32, cin), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.sfm_conv3_wgrad_f16_workspace_bytes(B, cin, L, h, w)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_conv3_wgrad_f16(_lib.ptr(x), _lib.ptr(grad_out), B, cin, 32, L, h, w, _lib.ptr(gw), _lib.ptr(ws),
                                     ws.numel(), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_conv3_wgrad_f16")
    return gw


_UNIT = {}


def _unit_affine(device):
    """scale 1 / bias 0 of a raw convolution, once per device."""
    key = str(device)
    if key not in _UNIT:
        _UNIT[key] = (torch.ones(32, device=device), torch.zeros(32, device=device))
    return _UNIT[key]


class _Conv3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        cout = int(weight.shape[0])
        one, zero = _unit_affine(x.device)
        y = conv3_f16(x, pack_weights(weight.detach().float()).half().contiguous(), one, zero, None, False, cout)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        if cout == 32:
            gp = g.to(torch.float16).contiguous()
        else:
            # classify's 32 -> 1 layer: its gradient as channel 0 of a zero-padded 32-channel tensor
            gp = torch.zeros(tuple(g.shape) + (32,), dtype=torch.float16, device=g.device)
            gp[..., 0] = g
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            one, zero = _unit_affine(x.device)
            wd = pack_dgrad_weights(weight.detach().float()).half().contiguous()
            parts = [conv3_f16(gp, wd[k], one, zero, None, False, 32) for k in range(cin // 32)]
            grad_x = parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
        if ctx.needs_input_grad[1]:
            grad_w = unpack_wgrad(conv3_wgrad_f16(x, gp), cout, cin).to(weight.dtype)
        return grad_x, grad_w


def conv3_autograd(x, weight):
    """One raw 3x3x3 Conv3d of the stack with a backward on libsfm_hip: x
    [B, L, h, w, cin] float16 on the device (channels-last), ``weight`` the
    module's float32 parameter [cout, cin, 3, 3, 3] (rounded to float16 as
    autocast rounds it) -> sfm_conv3_f16's output with scale 1, bias 0, no
    ReLU and no residual, bit for bit: [B, L, h, w, 32] float16, or
    [B, L, h, w] float32 for cout 1.  Backward: the data gradient is
    sfm_conv3_f16 on ``pack_dgrad_weights``' weights, the weight gradient
    sfm_conv3_wgrad_f16, returned as float32 in the parameter's layout; each
    only when its input needs a gradient."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float16 and x.dim() == 5):
        raise RuntimeError("conv3_autograd needs a [B, L, h, w, cin] float16 device tensor (HIP path, no CPU fallback)")
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or weight.shape[0] not in (1, 32) or \
            weight.shape[1] != x.shape[-1] or weight.shape[1] not in (32, 64):
        raise RuntimeError("weight must be [32 or 1, cin, 3, 3, 3] with cin 32 or 64, the channels of x")
    return _Conv3.apply(x.contiguous(), weight)


def _bn3_operand(t, name, like=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.dim() >= 2 and
            t.shape[-1] == 32 and t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous [..., 32] float16 device tensor (HIP path, no CPU fallback)")
    if like is not None and t.shape != like.shape:
        raise RuntimeError(f"{name} must have the shape of x")


def bn3_stats_f16(x, gamma, beta, eps=1e-5, running_mean=None, running_var=None, momentum=0.1, training=True):
    """sfm_bn3_stats_f16: x [..., 32] float16 (channels last), gamma / beta and
    the running statistics [32] float32 on x's device -> stats [5, 32] float32
    (mean, biased variance, invstd, a, b).  In training mode the running
    statistics, where given, are updated in place; in eval mode they are read."""
    _bn3_operand(x, "x")
    lib = _lib.load()
    vox = x.numel() // 32
    stats = torch.empty((5, 32), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(16, lib.sfm_bn3_stats_f16_workspace_bytes(vox, 1 if training else 0)), dtype=torch.uint8,
                     device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_bn3_stats_f16(_lib.ptr(x), vox, _lib.ptr(gamma), _lib.ptr(beta), float(eps), _lib.ptr(running_mean),
                                   _lib.ptr(running_var), float(momentum), 1 if training else 0, _lib.ptr(stats),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_bn3_stats_f16")
    if training:
        for r in (running_mean, running_var):       # written through the raw pointer: tell autograd and pack()'s key
            if r is not None:
                torch.autograd.graph.increment_version(r)
    return stats


def bn3_apply_f16(x, stats, residual=None, relu=False):
    """sfm_bn3_apply_f16: f16(relu(fma(a, x, b)) + residual) with a, b from
    ``stats`` [5, 32] float32; x and residual [..., 32] float16."""
    _bn3_operand(x, "x")
    if residual is not None:
        _bn3_operand(residual, "residual", x)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = _lib.load().sfm_bn3_apply_f16(_lib.ptr(x), x.numel() // 32, _lib.ptr(stats), _lib.ptr(residual),
                                           1 if relu else 0, _lib.ptr(out), _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_bn3_apply_f16")
    return out


def bn3_backward_f16(x, grad_out, stats, relu=False, training=True, need_grad_x=True):
    """sfm_bn3_backward_f16 -> (grad_x float16 like x or None, grad_gamma_beta
    [2, 32] float32: dgamma, dbeta), from x and ``stats`` alone."""
    _bn3_operand(x, "x")
    _bn3_operand(grad_out, "grad_out", x)
    lib = _lib.load()
    vox = x.numel() // 32
    gx = torch.empty_like(x) if need_grad_x else None
    ggb = torch.empty((2, 32), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(16, lib.sfm_bn3_backward_f16_workspace_bytes(vox)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.sfm_bn3_backward_f16(_lib.ptr(x), _lib.ptr(grad_out), vox, _lib.ptr(stats), 1 if relu else 0,
                                      1 if training else 0, _lib.ptr(gx), _lib.ptr(ggb), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr(x.device))
        _lib.check(rc, "sfm_bn3_backward_f16")
    return gx, ggb


class _BN3Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        training = bool(bn.training)
        stats = bn3_stats_f16(x, weight.detach(), bias.detach(), bn.eps, bn.running_mean, bn.running_var, bn.momentum,
                              training)
        if training:
            bn.num_batches_tracked.add_(1)
        out = bn3_apply_f16(x, stats, None if residual is None else residual.detach(), relu)
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
            gx, ggb = bn3_backward_f16(x, g.to(torch.float16).contiguous(), stats, ctx.relu, ctx.training, need_x)
            gw = ggb[0].to(ctx.param_dtypes[0]) if need_w else None
            gb = ggb[1].to(ctx.param_dtypes[1]) if need_b else None
        return gx, gw, gb, (g if need_r else None), None, None


def batchnorm3_act_autograd(x, bn, relu=False, residual=None):
    """``bn`` (an nn.BatchNorm3d of 32 channels), then ReLU if ``relu``, then
    ``+ residual``, on libsfm_hip in both directions: x and residual
    [B, L, h, w, 32] float16 on the device, channels last -> the same shape,
    float16, rounded once (sfm_bn3_stats_f16, sfm_bn3_apply_f16).  The module's
    mode, eps, momentum and affine parameters are honoured: training mode takes
    batch statistics, updates the running statistics in place by torch's rule
    and increments num_batches_tracked; eval mode reads the running statistics.
    Only x and the 160 floats of statistics are saved; the backward
    (sfm_bn3_backward_f16) returns gradients for x, bn.weight, bn.bias and the
    residual (the output gradient itself), each only where needed.  A module
    that is not the stock affine one with running statistics and a fixed
    momentum, or that carries forward hooks, raises; so does a CPU tensor."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float16 and x.dim() == 5 and
            x.shape[-1] == 32):
        raise RuntimeError("batchnorm3_act_autograd needs a [B, L, h, w, 32] float16 device tensor (HIP path, no CPU "
                           "fallback)")
    if type(bn) is not nn.BatchNorm3d or bn.num_features != 32:
        raise RuntimeError("bn must be an nn.BatchNorm3d of 32 channels")
    if not bn.affine or not bn.track_running_stats or bn.momentum is None or bn.running_mean is None:
        raise RuntimeError("bn must be the stock module: affine=True, track_running_stats=True and a fixed momentum")
    if bn._forward_hooks or bn._forward_pre_hooks:
        raise RuntimeError("bn carries forward hooks, which the HIP route would not call")
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if not (t.device == x.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("bn's parameters and running statistics must be float32 on x's device")
    if x.numel() // 32 < 2 and bn.training:
        raise RuntimeError("training-mode batch statistics need more than one value per channel")
    if residual is not None and not (isinstance(residual, torch.Tensor) and residual.is_cuda and
                                     residual.dtype == torch.float16 and residual.shape == x.shape):
        raise RuntimeError("residual must be a float16 device tensor of x's shape")
    return _BN3Act.apply(x.contiguous(), bn.weight, bn.bias, None if residual is None else residual.contiguous(), bn,
                         bool(relu))


def bn3_act_reference(x, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5,
                      relu=False, residual=None):
    """The mathematics of ``batchnorm3_act_autograd`` in torch ops in float64,
    on any device (tests and documents only): x [..., C] channels last ->
    (out, new running_mean, new running_var), all float64; differentiable by
    autograd in x, gamma, beta and residual.  Training mode: batch mean and
    biased variance, the running statistics moved by (1 - momentum) r +
    momentum batch with the unbiased variance; eval mode: the running
    statistics, returned as they came."""
    x = x.double()
    gamma, beta = gamma.double(), beta.double()
    flat = x.reshape(-1, x.shape[-1])
    n = flat.shape[0]
    if training:
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
        new_mean = new_var = None
        if running_mean is not None:
            new_mean = (1.0 - momentum) * running_mean.double() + momentum * mean.detach()
        if running_var is not None:
            new_var = (1.0 - momentum) * running_var.double() + momentum * var.detach() * n / (n - 1)
    else:
        mean, var = running_mean.double(), running_var.double()
        new_mean, new_var = mean, var
    invstd = 1.0 / torch.sqrt(var + eps)
    a = gamma * invstd
    b = beta - mean * a
    z = a * x + b
    if relu:
        z = torch.relu(z)
    if residual is not None:
        z = z + residual.double()
    return z, new_mean, new_var


class CostRegularization(nn.Module):
    """dres0..dres4 + classify of PSNet (PSNet.py:79-102), initialised as
    PSNet.py:104-118 (Conv3d ~ N(0, sqrt(2 / (27 * out_channels))), BN = 1 / 0)."""

    def __init__(self, in_channels=64):
        super().__init__()
        if in_channels not in (32, 64):
            raise ValueError("in_channels must be 32 or 64 (2 x feature channels)")
        self.dres0 = nn.Sequential(convbn_3d(in_channels, 32), nn.ReLU(inplace=True),
                                   convbn_3d(32, 32), nn.ReLU(inplace=True))
        for i in range(1, 5):
            setattr(self, f"dres{i}", nn.Sequential(convbn_3d(32, 32), nn.ReLU(inplace=True), convbn_3d(32, 32)))
        self.classify = nn.Sequential(convbn_3d(32, 32), nn.ReLU(inplace=True),
                                      nn.Conv3d(32, 1, kernel_size=3, padding=1, stride=1, bias=False))
        for m in self.modules():
            if isinstance(m, nn.Conv3d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.kernel_size[2] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm3d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        self._packed = None
        self._packed_key = None

    # (conv, bn, relu, residual-from) per layer, in execution order
    def layer_plan(self):
        plan = [(self.dres0[0][0], self.dres0[0][1], True, False),
                (self.dres0[2][0], self.dres0[2][1], True, False)]
        for i in range(1, 5):
            blk = getattr(self, f"dres{i}")
            plan.append((blk[0][0], blk[0][1], True, False))
            plan.append((blk[2][0], blk[2][1], False, True))
        plan.append((self.classify[0][0], self.classify[0][1], True, False))
        plan.append((self.classify[2], None, False, False))
        return plan

    def _key(self, device):
        return (str(device),) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def pack(self, device, precision="bf16"):
        """Packed weights [27][32][Cin] in the precision's type (fp32 / fp16 /
        bf16) and folded fp32 scale/bias per layer."""
        key = self._key(device) + (precision,)
        if self._packed is not None and self._packed_key == key:
            return self._packed
        wdt = _ACT_DTYPE[precision]
        packed = []
        with torch.no_grad():
            for conv, bn, relu, resid in self.layer_plan():
                w = conv.weight.detach().float()                    # [Cout, Cin, 3, 3, 3]
                cout, cin = w.shape[:2]
                wp = torch.zeros(27, 32, cin, dtype=torch.float32, device=w.device)
                wp[:, :cout] = w.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
                if bn is not None:
                    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
                    bias = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
                else:
                    scale = torch.ones(cout)
                    bias = torch.zeros(cout)
                sc = torch.ones(32)
                bi = torch.zeros(32)
                sc[:cout] = scale.cpu()
                bi[:cout] = bias.cpu()
                packed.append(dict(w=wp.to(device=device, dtype=wdt).contiguous(),
                                   scale=sc.to(device), bias=bi.to(device), cin=cin, cout=cout, relu=relu,
                                   resid=resid, wexp=weight_exponent(wp)))
        self._packed, self._packed_key = packed, key
        return packed

    def forward(self, cost, precision="fp32x3"):
        """cost [B, Cin, L, h, w] fp32 or bf16 (the sweep's volume) -> [B, 1, L, h, w] fp32.
        ``precision``: "fp32x3" (default: the reference's fp32 activations
        and weights, each product formed from a two-term f16 split of both
        operands on the f16 matrix cores, sfm_conv3_f32x3: ~2^-21 per product,
        within the float64 depth bars at 3x the speed of "fp32"; a layer whose
        input holds an activation beyond the f16 maximum 65504 is re-run as
        "fp32" on the device, see sfm_hip.h), "fp32"
        (fp32 operands on the f32 matrix cores, sfm_conv3_f32: float32
        arithmetic exactly, in another summation order),
        "fp16" (fp16
        activations and weights, fp32 accumulation: sfm_conv3_f16, the
        reference's precision under cfg.MIXED_PREC) or "bf16" (bf16, fp32
        accumulation: sfm_conv3_bf16, the fastest opt-in)."""
        if precision not in _ACT_DTYPE:
            raise ValueError(f"unknown conv precision {precision!r}")
        if not (isinstance(cost, torch.Tensor) and cost.is_cuda):
            raise RuntimeError("CostRegularization.forward needs a device tensor (HIP path, no CPU fallback)")
        if cost.dtype not in (torch.float32, torch.bfloat16) or cost.dim() != 5:
            raise RuntimeError("cost must be a [B, C, L, h, w] float32 or bfloat16 tensor")
        cost = cost.contiguous()
        B, C, L, h, w = cost.shape
        packed = self.pack(cost.device, precision)
        if C != packed[0]["cin"]:
            raise RuntimeError(f"cost has {C} channels, the first layer expects {packed[0]['cin']}")
        return self.forward_channels_last(to_channels_last(cost, _ACT_DTYPE[precision]), precision=precision)

    def forward_differentiable(self, cost, norm="torch"):
        """The stack of PSNet.py:160-165 with a backward in float16 on
        libsfm_hip: cost [B, Cin, L, h, w] float32 on the device -> [B, 1, L,
        h, w] float32.  Every Conv3d is ``conv3_autograd`` (sfm_conv3_f16
        forward and data gradient, sfm_conv3_wgrad_f16) on channels-last
        float16 activations; every BatchNorm3d is called as the module it is,
        on the channels-last tensor viewed as [B, 32, L, h, w], so batch
        statistics in training mode, the running-stat updates, eval mode and a
        loaded state_dict are torch's; ReLU and the residual adds are torch
        ops.  The precision is that of the modules under float16 autocast.
        ``norm="hip"`` (opt-in) runs each BatchNorm3d with its ReLU and
        residual add as ``batchnorm3_act_autograd`` instead (sfm_bn3_stats_f16,
        sfm_bn3_apply_f16, sfm_bn3_backward_f16): the same module state read
        and updated, one rounding per layer instead of two, only the
        convolution's output and 160 floats saved; ``norm="torch"`` (default)
        is the route above, unchanged bit for bit."""
        if norm not in ("torch", "hip"):
            raise ValueError(f"unknown norm {norm!r}")
        if not (isinstance(cost, torch.Tensor) and cost.is_cuda):
            raise RuntimeError("CostRegularization.forward_differentiable needs a device tensor (HIP path, no CPU "
                               "fallback)")
        if cost.dim() != 5 or cost.shape[1] != self.dres0[0][0].in_channels:
            raise RuntimeError(f"cost must be [B, {self.dres0[0][0].in_channels}, L, h, w]")
        x = cost.permute(0, 2, 3, 4, 1).to(torch.float16).contiguous()        # [B, L, h, w, Cin]
        keep = None
        for li, (conv, bn, relu, resid) in enumerate(self.layer_plan()):
            y = conv3_autograd(x, conv.weight)
            if bn is None:
                return y.unsqueeze(1)                                          # classify's last layer: [B, L, h, w] fp32
            if norm == "hip":
                x = batchnorm3_act_autograd(y, bn, relu, keep if resid else None)
                if li == 1 or resid:
                    keep = x
                continue
            y = bn(y.permute(0, 4, 1, 2, 3))                                   # a [B, 32, L, h, w] view, channels last
            if relu:
                y = torch.relu(y)
            y = y.permute(0, 2, 3, 4, 1)
            if resid:
                y = y + keep
            x = y.to(torch.float16).contiguous()
            if li == 1 or resid:
                keep = x
        raise AssertionError("layer_plan ends with classify's plain convolution")

    def forward_channels_last(self, x, precision="fp32x3"):
        """``forward`` on the channels-last volume: x [B, L, h, w, Cin],
        contiguous, in the precision's activation dtype (float32 for "fp32" /
        "fp32x3", float16 for "fp16", bfloat16 for "bf16") -- what
        ``to_channels_last`` or ``plane_sweep_cost_channels_last`` writes --
        -> [B, 1, L, h, w] fp32."""
        if precision not in _ACT_DTYPE:
            raise ValueError(f"unknown conv precision {precision!r}")
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError("CostRegularization.forward_channels_last needs a device tensor (HIP path, no CPU "
                               "fallback)")
        adt = _ACT_DTYPE[precision]
        if x.dtype != adt or x.dim() != 5 or not x.is_contiguous():
            raise RuntimeError(f"x must be a contiguous [B, L, h, w, C] {adt} tensor for precision {precision!r}")
        B, L, h, w, C = x.shape
        packed = self.pack(x.device, precision)
        if C != packed[0]["cin"]:
            raise RuntimeError(f"x has {C} channels, the first layer expects {packed[0]['cin']}")
        lib = _lib.load()
        dev = x.device
        suffix = {"fp32": "f32", "fp32x3": "f32", "fp16": "f16", "bf16": "bf16"}[precision]
        if precision == "fp32x3":
            # the split-f16 kernel takes the weights' power-of-two exponent after them
            x3 = lib.sfm_conv3_f32x3
            fn_name = "sfm_conv3_f32x3"
        else:
            conv = getattr(lib, "sfm_conv3_" + suffix)
            fn_name = "sfm_conv3_" + suffix
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            bufs = [torch.empty((B, L, h, w, 32), dtype=adt, device=dev) for _ in range(3)]
            out = torch.empty((B, 1, L, h, w), dtype=torch.float32, device=dev)
            # fp32x3: one range flag (two words) per layer -- a layer whose input leaves the f16 range, or
            # stays below FP32X3_MIN_AMAX, is re-run by sfm_conv3_f32 inside the same call, stream-ordered
            flags = torch.empty(2 * len(packed), dtype=torch.int32, device=dev) if precision == "fp32x3" else None
            cur, keep = x, None           # keep: the block input of a residual pair (cost0)
            for li, lay in enumerate(packed):
                if lay["cout"] == 1:
                    dst = out
                else:
                    dst = next(bb for bb in bufs if bb is not cur and bb is not keep)
                res = keep if lay["resid"] else None
                if precision == "fp32x3":
                    rc = x3(_lib.ptr(cur), B, lay["cin"], L, h, w, _lib.ptr(lay["w"]), lay["wexp"],
                            _lib.ptr(lay["scale"]), _lib.ptr(lay["bias"]), None if res is None else _lib.ptr(res),
                            1 if lay["relu"] else 0, lay["cout"], _lib.ptr(dst), flags[2 * li].data_ptr(), stream)
                else:
                    rc = conv(_lib.ptr(cur), B, lay["cin"], L, h, w, _lib.ptr(lay["w"]), _lib.ptr(lay["scale"]),
                              _lib.ptr(lay["bias"]), None if res is None else _lib.ptr(res), 1 if lay["relu"] else 0,
                              lay["cout"], _lib.ptr(dst), stream)
                _lib.check(rc, fn_name)
                # cost0 after dres0 (layer 1) and after every residual add is the next block's input
                if li == 1 or lay["resid"]:
                    keep = dst
                cur = dst
        return out


def fused_channels_last(cost_dtype, precision):
    """Whether the depth stage takes the fused route for this sweep storage
    dtype and conv precision: the sweep writes the regulariser's channels-last
    input itself (``plane_sweep_cost_channels_last``) instead of a planar
    float32 volume that ``to_channels_last`` re-reads.  Same bits either way.
    Only a float32 volume has a fused equivalent (a bf16 volume rounds twice),
    and the library switch ``sweep_fused_cl`` (default 1) turns the route off."""
    return cost_dtype == torch.float32 and precision in _ACT_DTYPE and _lib.tune_get("sweep_fused_cl") == 1


def f16_features(ref_fea, tgt_fea):
    """Whether the fused route hands these features to the sweep as they come:
    both float16 (the feature CNN's output under cfg.MIXED_PREC autocast) and
    the library switch ``sweep_f16_feat`` at 1.  Otherwise they are widened to
    float32 first: the same bits either way."""
    return ref_fea.dtype == torch.float16 and tgt_fea.dtype == torch.float16 and \
        _lib.tune_get("sweep_f16_feat") == 1


def sweep_regularize_fused(regularizer, ref_fea, tgt_fea, pose, K4, Ki4, nlabel, min_depth, precision,
                           predict_by_depth=False):
    """Sweep + regularisation on the fused route: [B, 1, L, h, w] fp32, the
    bits of ``regularizer(plane_sweep_cost(...), precision=precision)``.
    Float16 features stay float16 (``f16_features``)."""
    if precision not in _ACT_DTYPE:
        raise ValueError(f"unknown conv precision {precision!r}")
    if not f16_features(ref_fea, tgt_fea):
        ref_fea, tgt_fea = ref_fea.float(), tgt_fea.float()
    x = plane_sweep_cost_channels_last(ref_fea, tgt_fea, pose, K4, Ki4, nlabel, min_depth,
                                       dtype=_ACT_DTYPE[precision], predict_by_depth=predict_by_depth)
    return CostRegularization.forward_channels_last(regularizer, x, precision=precision)


def psnet_depth(ref_fea, tgt_fea, pose, intrinsics, intrinsics_inv, regularizer, nlabel, min_depth=1.0,
                out_hw=None, predict_by_depth=False, cost_dtype=torch.float32, precision=None):
    """PSNet's single-target depth path at feature resolution, PSNet.py:130-216
    without the context network (cfg.PSNET_CONTEXT off): plane sweep ->
    dres/classify -> trilinear upsample, softmax, disparity regression.
    ``pose`` [B,3,4] already rescaled; full-resolution intrinsics.
    Returns depth [B, 1, H, W] fp32.  A stock ``CostRegularization`` with a
    float32 volume takes the fused sweep (``fused_channels_last``); a subclass
    that overrides ``forward``, a module with forward hooks and any other
    callable get ``regularizer(cost)`` on the planar volume as before."""
    K4, Ki4 = quarter_intrinsics(intrinsics, intrinsics_inv)
    # the fused route calls forward_channels_last directly, so it is taken only where regularizer(cost) would
    # run the stock forward and nothing else: no forward override and no forward (pre-)hooks on the module
    fused = isinstance(regularizer, CostRegularization) and \
        type(regularizer).forward is CostRegularization.forward and \
        not regularizer._forward_hooks and not regularizer._forward_pre_hooks and \
        fused_channels_last(cost_dtype, "fp32x3" if precision is None else precision)
    if fused:
        costs = sweep_regularize_fused(regularizer, ref_fea, tgt_fea, pose, K4, Ki4, nlabel, min_depth,
                                       "fp32x3" if precision is None else precision, predict_by_depth)
    else:
        cost = plane_sweep_cost(ref_fea, tgt_fea, pose, K4, Ki4, nlabel, min_depth, dtype=cost_dtype,
                                predict_by_depth=predict_by_depth)
        costs = regularizer(cost) if precision is None else regularizer(cost, precision=precision)
    B = costs.shape[0]
    h, w = costs.shape[-2:]
    H, W = out_hw if out_hw is not None else (4 * h, 4 * w)
    return depth_head(costs.view(B, int(nlabel), h, w), nlabel, min_depth, out_hw=(H, W),
                      predict_by_depth=predict_by_depth)
