"""PSNet-layout depth estimator: SFMnet's default ``depth_estimator``.

The reference builds ``PSNet(nlabel, min_depth)`` inside ``SFMnet.__init__``
(models/SFMnet.py:57-58; PSNet models/PSNet.py:40-227).  This module keeps
PSNet's module names and constructor, so a PSNet state_dict loads unchanged,
and runs its forward with the hot path on libsfm_hip:

  feature_extraction  2-D CNN at 1/4 resolution, 32 channels         sfm_image_pack_f16, sfm_conv2x_f16 (HIP MFMA),
                      (PSMNet SPP layout, models/submodule.py:108-184)  sfm_avgpool_f16, sfm_spp_pack_f16 under float16
                      and context_net (IND_CONTEXT)                    autocast in eval mode (``feature_precision``:
                                                                       2.25 ms against 7.04 per KITTI pair,
                                                                       profiles/feature_ab.txt); else torch (MIOpen)
  plane sweep         cost [B, 64, L, h, w] (PSNet.py:130-158)        sfm_plane_sweep (HIP); by default written
                      channels-last for the next stage                 sfm_plane_sweep_cl (HIP); float16 features
                      (cfg.MIXED_PREC) read as they come               sfm_plane_sweep_cl_f16 (HIP)
  dres0..4, classify  3-D cost regularisation (PSNet.py:79-102, 159-165)  sfm_conv3_* (HIP MFMA)
  convs               per-plane context CNN (PSNET_CONTEXT, 175-192)   sfm_conv2_* (HIP MFMA) under float16 autocast
                      in eval mode (``context_precision``); else       torch (MIOpen)
  head                trilinear up, softmax, disparity regression     sfm_depth_head (HIP)
  training            grad mode on, features that require grad:        sfm_plane_sweep_ex / _backward and
                      the sweep and both heads with a backward,        sfm_depth_head / _backward (HIP);
                      the stacks as the nn.Modules they are            torch (MIOpen)
                      dres0..4 / classify under float16 autocast       sfm_conv3_f16 / sfm_conv3_wgrad_f16 (HIP MFMA)
                      with ``regularize_grad`` "fp16"                   between torch's BatchNorm3d, or with
                      ``regularize_norm`` "hip"                        sfm_bn3_stats / _apply / _backward_f16 (HIP)
                      convs under float16 autocast with                sfm_conv2_f16 / sfm_conv2_dgrad_f16 /
                      ``context_grad`` "fp16"                          sfm_conv2_wgrad_f16 (HIP MFMA),
                                                                       sfm_context_pack_f16 / _unpack_grad_f16 (HIP)
                      dep_convs under float16 autocast with            the same three conv2 kernels,
                      ``dep_context_grad`` "fp16"                      sfm_dep_context_pack_f16 / _unpack_grad_f16 (HIP)
  dep_convs           full-resolution depth refinement (PSNET_DEP_CONTEXT, 218-225): bilinear upsample + cat
                      sfm_dep_context_pack_* (HIP), the stack      sfm_conv2_* (HIP MFMA) under float16 autocast
                      in eval mode (``dep_context_precision``); else   torch (MIOpen)

The 2-D CNNs are outside bench.py's measured path (feature
CNN and context networks are out of scope); they are plain torch modules here,
so the estimator is complete and a reference checkpoint's weights apply, and
the HIP routes read those modules' parameters.  The
``COST_BY_COLOR`` ablations (PSNet.py:75-78, 181-188) are not built.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import feature as _feature
from .config import cfg as _default_cfg
from .context import (_autocast_gpu_dtype, context_refine, context_refine_autograd, dep_context_refine,
                      dep_context_refine_autograd, dep_stock_layout, stock_layout)
from .depth import depth_head, depth_head_autograd
from .regularize import CostRegularization, f16_features, fused_channels_last, sweep_regularize_fused
from .sweep import plane_sweep_cost, plane_sweep_cost_autograd, quarter_intrinsics


# Whether feature_precision="auto" may resolve to "fp16": the same-process A/B of scripts/feature_ab.py decides it
# (profiles/feature_ab.txt: HIP 2.246 ms, torch float16 autocast 7.043 ms per KITTI pair of images)
FEATURE_AUTO_HIP = True

# Whether the differentiable route's heads are depth_head_autograd (sfm_depth_head + sfm_depth_head_backward) or
# torch_depth_head: the same-process A/B of scripts/depth_head_bwd_ab.py decides it (profiles/depth_head_bwd_ab.txt)
HEAD_BWD_HIP = True

# Whether regularize_grad="auto" may resolve to "fp16" (CostRegularization.forward_differentiable: sfm_conv3_f16 and
# sfm_conv3_wgrad_f16) on the differentiable route under float16 autocast, or stays with the nn.Modules: the
# same-process A/B of scripts/stack_bwd_ab.py decides it (profiles/stack_bwd_ab.txt)
STACK_BWD_HIP = True


def torch_depth_head(cost, nlabel, min_depth, out_hw, predict_by_depth=False, scale=None):
    """PSNet.py:194-216 in torch ops on a [B, L, h, w] cost, float32: trilinear
    upsample, softmax over planes, disparity / depth regression
    (submodule.py:57-93).  ``depth_head``'s arguments; what the differentiable
    route runs with HEAD_BWD_HIP off, and the torch arm of the A/B."""
    L = int(nlabel)
    up = F.interpolate(cost.float().unsqueeze(1), [L, int(out_hw[0]), int(out_hw[1])], mode="trilinear")[:, 0]
    prob = F.softmax(up, dim=1)
    idx = torch.arange(1, L + 1, dtype=torch.float32, device=cost.device).reshape(1, L, 1, 1)
    if predict_by_depth:
        mul = float(min_depth) if scale is None else float(scale)
        return torch.sum(prob * (idx * float(int(min_depth))), 1, keepdim=True) * mul
    return float(min_depth) * L / (torch.sum(prob * idx, 1, keepdim=True) + 1e-16)


def _conv_bn(cin, cout, k, stride, pad, dilation):
    """Conv2d (no bias) + BatchNorm2d; a dilated conv pads by its dilation
    (models/submodule.py:11-15)."""
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=dilation if dilation > 1 else pad,
                                   dilation=dilation, bias=False),
                         nn.BatchNorm2d(cout))


class _Residual(nn.Module):
    """Two 3x3 conv-BN stages with a ReLU between, plus the (projected) input."""

    def __init__(self, cin, cout, stride, pad, dilation):
        super().__init__()
        self.conv1 = nn.Sequential(_conv_bn(cin, cout, 3, stride, pad, dilation), nn.ReLU(inplace=True))
        self.conv2 = _conv_bn(cout, cout, 3, 1, pad, dilation)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        y = self.conv2(self.conv1(x))
        return y + (x if self.downsample is None else self.downsample(x))


class FeatureExtraction(nn.Module):
    """PSNet's feature CNN (layout of models/submodule.py:108-184): stride-2
    stem, four residual stages (the second stride 2, the last dilated), four
    average-pool pyramid branches upsampled back, and a 320 -> 32 fusion."""

    # (attribute, channels, blocks, stride, dilation)
    STAGES = (("layer1", 32, 3, 1, 1), ("layer2", 64, 16, 2, 1), ("layer3", 128, 3, 1, 1), ("layer4", 128, 3, 1, 2))
    POOLS = (32, 16, 8, 4)      # branch1..branch4

    def __init__(self):
        super().__init__()
        self.firstconv = nn.Sequential(_conv_bn(3, 32, 3, 2, 1, 1), nn.ReLU(inplace=True),
                                       _conv_bn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True),
                                       _conv_bn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True))
        cin = 32
        for name, ch, blocks, stride, dil in self.STAGES:
            mods = [_Residual(cin, ch, stride, 1, dil)] + [_Residual(ch, ch, 1, 1, dil) for _ in range(blocks - 1)]
            setattr(self, name, nn.Sequential(*mods))
            cin = ch
        for i, p in enumerate(self.POOLS):
            setattr(self, f"branch{i + 1}", nn.Sequential(nn.AvgPool2d((p, p), stride=(p, p)),
                                                          _conv_bn(128, 32, 1, 1, 0, 1), nn.ReLU(inplace=True)))
        self.lastconv = nn.Sequential(_conv_bn(320, 128, 3, 1, 1, 1), nn.ReLU(inplace=True),
                                      nn.Conv2d(128, 32, kernel_size=1, padding=0, stride=1, bias=False))

    def forward(self, x):
        x = self.layer1(self.firstconv(x))
        raw = self.layer2(x)
        skip = self.layer4(self.layer3(raw))
        size = skip.shape[2:]
        pyr = [F.interpolate(getattr(self, f"branch{i}")(skip), size, mode="bilinear", align_corners=True)
               for i in (4, 3, 2, 1)]
        return self.lastconv(torch.cat([raw, skip] + pyr, 1))


def _context_conv(cin, cout, k=3, stride=1, dilation=1, bn=False):
    """PSNet.py:17-26 (convtext)."""
    conv = nn.Conv2d(cin, cout, kernel_size=k, stride=stride, dilation=dilation,
                     padding=((k - 1) * dilation) // 2, bias=False)
    return nn.Sequential(conv, nn.BatchNorm2d(cout), nn.ReLU(inplace=True)) if bn else \
        nn.Sequential(conv, nn.ReLU(inplace=True))


def _context_stack(cin, bn):
    """Seven dilated 3x3 stages cin -> 128 -> ... -> 1 (PSNet.py:54-70)."""
    plan = ((cin, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 1, 1))
    return nn.Sequential(*[_context_conv(a, b, 3, 1, d, bn) for a, b, d in plan])


class PSNet(CostRegularization):
    """``PSNet(nlabel, mindepth)`` with the reference's module names
    (feature_extraction, dres0..4, classify, convs, dep_convs, context_net)
    and forward signature / return value ``(depth_init, depth)``
    (PSNet.py:128, 214-227).

    ``feature_fn`` replaces the feature CNN (any callable image -> [B, 32,
    H/4, W/4]); ``conv_precision`` selects the regularisation arithmetic
    (CostRegularization): "auto" (default) follows the reference --
    PSNet.py:159-165 in float32, or in float16 under cfg.MIXED_PREC, the
    autocast SFMnet.py:164 wraps the depth estimator in (cfgs/kitti.yml:10) --
    so it resolves to "fp32x3" (fp32 operands, each product from a two-term
    f16 split on the f16 matrix cores: within the float64 fixture's depth bars
    at 3x the speed of "fp32", the f32-MFMA path, which stays selectable) or
    "fp16"; "bf16" is the fastest opt-in path;
    ``cost_dtype`` the sweep volume's storage.  ``context_precision`` selects
    how the per-plane context stack ``convs`` runs (PSNet.py:175-190): "torch"
    (nn.Conv2d), "fp16" / "bf16" (``sfm_amd.context.context_refine``, eval
    mode only) or "auto" (default), which takes the "fp16" route exactly where
    torch would compute these convolutions in float16 anyway -- eval mode,
    float16 CUDA autocast active at the call (what SFMnet.forward sets under
    cfg.MIXED_PREC), no forward (pre-)hooks on ``convs``, the stock
    33-channel stack -- and "torch" everywhere else.
    ``dep_context_precision`` selects, with the same values and the same rule
    applied to ``dep_convs`` (the stock 36-channel stack), how the
    full-resolution refinement of cfg.PSNET_DEP_CONTEXT runs
    (PSNet.py:218-221): ``sfm_amd.context.dep_context_refine``, which
    upsamples the features in the dtype they arrive in, or nn.Conv2d on
    F.interpolate + torch.cat.  ``feature_precision`` ("auto", "torch" or
    "fp16") selects by the same rule how ``feature_extraction`` and, under
    cfg.IND_CONTEXT, ``context_net`` run: ``sfm_amd.feature.feature_extract``
    on the reference and every target image as one batch, or the module
    itself; "auto" asks besides for the stock FeatureExtraction graph
    (``feature_layout_ok``; an injected ``feature_fn`` never is) and a
    quarter-resolution map of at least 32 x 32.  It resolves to "fp16"
    because the HIP route measured faster (FEATURE_AUTO_HIP).

    Training.  With grad mode on and features that require grad (every
    training step, and an eval-mode call outside ``torch.no_grad()`` whose
    features come from a torch module) ``forward`` takes the differentiable
    route, the reference's graph with the sweep and both heads on libsfm_hip:
    ``plane_sweep_cost_autograd`` on the float32 planar volume; ``dres0..4``
    and ``classify`` as the modules they are (PSNet.py:160-165; BatchNorm
    follows ``self.training``, as in torch); the context stack's and
    ``dep_convs``' torch branches (on ``depth.detach()``, as the reference);
    ``depth_head_autograd`` for ``depth_init`` and ``depth`` (HEAD_BWD_HIP; the
    bits of ``depth_head``).  ``conv_precision`` and ``cost_dtype`` apply to
    the forward-only route alone; a forced "fp16" / "bf16" context,
    dep-context or feature precision has no backward and raises there.
    ``regularize_grad`` selects how that route runs ``dres0..4`` and
    ``classify``: "torch" (the modules), "fp16"
    (``CostRegularization.forward_differentiable``: every Conv3d forward and
    backward on libsfm_hip in float16, BatchNorm3d as the module it is; needs
    float16 CUDA autocast at the call and raises without it) or "auto"
    (default): "fp16" exactly where the modules would compute in float16
    anyway -- a CUDA device, float16 autocast active at the call -- the stacks
    are the stock modules without forward (pre-)hooks, and STACK_BWD_HIP is on;
    "torch" everywhere else.  ``regularize_norm`` says how the "fp16" route
    runs the stack's BatchNorm3d, ReLU and residual adds: "torch" (default: the
    modules and torch ops) or "hip" (opt-in: ``batchnorm3_act_autograd``,
    sfm_bn3_* in both directions; profiles/stack_norm_ab.txt); it has no effect
    on the "torch" route.  ``context_grad`` selects how the differentiable
    route runs the context stack ``convs``: "torch" (default: the modules) or
    "fp16" (opt-in: ``sfm_amd.context.context_refine_autograd``, every stage
    forward and backward on libsfm_hip in float16, at the cost of 1280 bytes
    of saved activations per pixel and plane; needs float16 CUDA autocast at
    the call and raises without it; a stack with BatchNorm2d, cfg.CONTEXT_BN,
    is refused; profiles/context_bwd_ab.txt).  ``dep_context_grad`` selects the
    same for ``dep_convs`` under cfg.PSNET_DEP_CONTEXT: "torch" (default: the
    float32 F.interpolate + torch.cat and the modules) or "fp16" (opt-in:
    ``sfm_amd.context.dep_context_refine_autograd``, the upsample, every stage
    and their backward on libsfm_hip in float16, at the cost of 1280 bytes of
    saved activations per full-resolution pixel; the same conditions and
    refusals; profiles/dep_context_bwd_ab.txt).
    Everything else is unchanged bit for bit: calls under ``torch.no_grad()``
    in either mode, and the float16 eval routes, whose HIP features carry no
    grad and so never enter the differentiable route."""

    def __init__(self, nlabel, mindepth=None, cfg=None, feature_fn=None, cost_dtype=torch.float32,
                 conv_precision="auto", context_precision="auto", dep_context_precision="auto",
                 feature_precision="auto", regularize_grad="auto", regularize_norm="torch", context_grad="torch",
                 dep_context_grad="torch"):
        super().__init__(64)
        c = _default_cfg if cfg is None else cfg
        if c.get("COST_BY_COLOR", False) or c.get("COST_BY_COLOR_WITH_FEAT", False):
            raise RuntimeError("PSNet: the COST_BY_COLOR ablations (PSNet.py:75-78) are not built")
        self.cfg = c
        self.nlabel = int(nlabel)
        self.mindepth = float(c.MIN_DEPTH)            # the reference reads cfg.MIN_DEPTH too (PSNet.py:44)
        self.cost_dtype = cost_dtype
        if conv_precision == "auto":
            conv_precision = "fp16" if c.get("MIXED_PREC", False) else "fp32x3"
        if conv_precision not in ("fp32", "fp32x3", "fp16", "bf16"):
            raise ValueError(f"unknown conv precision {conv_precision!r}")
        self.conv_precision = conv_precision
        if context_precision not in ("auto", "torch", "fp16", "bf16"):
            raise ValueError(f"unknown context precision {context_precision!r}")
        self.context_precision = context_precision
        if dep_context_precision not in ("auto", "torch", "fp16", "bf16"):
            raise ValueError(f"unknown dep_context precision {dep_context_precision!r}")
        self.dep_context_precision = dep_context_precision
        if feature_precision not in ("auto", "torch", "fp16"):
            raise ValueError(f"unknown feature precision {feature_precision!r}")
        self.feature_precision = feature_precision
        if regularize_grad not in ("auto", "torch", "fp16"):
            raise ValueError(f"unknown regularize_grad {regularize_grad!r}")
        self.regularize_grad = regularize_grad
        if regularize_norm not in ("torch", "hip"):
            raise ValueError(f"unknown regularize_norm {regularize_norm!r}")
        self.regularize_norm = regularize_norm
        if context_grad not in ("torch", "fp16"):
            raise ValueError(f"unknown context_grad {context_grad!r}")
        self.context_grad = context_grad
        if dep_context_grad not in ("torch", "fp16"):
            raise ValueError(f"unknown dep_context_grad {dep_context_grad!r}")
        self.dep_context_grad = dep_context_grad
        self.feature_extraction = FeatureExtraction() if feature_fn is None else feature_fn
        if c.get("IND_CONTEXT", False):
            self.context_net = FeatureExtraction()
        bn = bool(c.get("CONTEXT_BN", False))
        self.convs = _context_stack(33, bn)
        if c.get("PSNET_DEP_CONTEXT", False):
            self.dep_convs = _context_stack(36, bn)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def regularize(self, cost):
        return CostRegularization.forward(self, cost, precision=self.conv_precision)

    def context_route(self, device=None):
        """How the context stack runs at this call: "torch", "fp16" or "bf16"
        (see ``context_precision``)."""
        return self._stack_route("context_precision", "convs", stock_layout, device)

    def dep_context_route(self, device=None):
        """How ``dep_convs`` runs at this call: "torch", "fp16" or "bf16"
        (see ``dep_context_precision``; ``context_route``'s rule)."""
        return self._stack_route("dep_context_precision", "dep_convs", dep_stock_layout, device)

    def feature_route(self, device=None, image_hw=None, name="feature_extraction"):
        """How the feature CNN ``name`` ("feature_extraction" or
        "context_net") runs at this call: "torch" or "fp16" (see
        ``feature_precision``; ``context_route``'s rule, and for "auto" an
        image whose quarter-resolution map is at least 32 x 32)."""
        route = self._stack_route("feature_precision", name, _feature.feature_layout_ok, device)
        if route == "fp16" and self.feature_precision == "auto":
            if not FEATURE_AUTO_HIP or image_hw is None or min(_feature.feature_hw(image_hw)) < _feature.MIN_MAP:
                return "torch"
        return route

    def _features(self, name, images):
        """The feature CNN ``name`` on each of ``images``: on the HIP route as
        one batch (every image is computed on its own), else the module per
        image, as the reference calls it."""
        net = getattr(self, name)
        if self.feature_route(images[0].device, images[0].shape[2:], name) == "fp16":
            n = [im.shape[0] for im in images]
            return list(_feature.feature_extract(net, torch.cat(images) if len(images) > 1 else images[0]).split(n))
        return [net(im) for im in images]

    def _stack_route(self, arg, name, layout_ok, device):
        p = getattr(self, arg)
        if p == "torch":
            return p
        if p in ("fp16", "bf16"):
            if self.training:
                raise RuntimeError(f"{arg}={p!r} folds BatchNorm2d and has no backward: eval mode only")
            return p
        on_gpu = device is not None and torch.device(device).type == "cuda"
        if self.training or not on_gpu or not torch.is_autocast_enabled() or _autocast_gpu_dtype() != torch.float16:
            return "torch"
        # the HIP route calls no module, so it is taken only where self.convs(x) / self.dep_convs(x) would run
        # the stock stack and nothing else (the rule psnet_depth applies to the fused sweep)
        convs = getattr(self, name, None)
        if not isinstance(convs, nn.Module):         # absent, or an injected feature_fn: never a stock module
            return "torch"
        if convs._forward_hooks or convs._forward_pre_hooks or not layout_ok(convs):
            return "torch"
        return "fp16"

    def _grad_stack_route(self, arg, route_fn, device):
        """The differentiable route runs ``convs`` / ``dep_convs`` as the
        modules they are ("torch"); a forced HIP precision has no backward, so
        it is refused (in training mode with ``_stack_route``'s own message)."""
        p = getattr(self, arg)
        if p in ("fp16", "bf16"):
            route_fn(device)
            raise RuntimeError(f"{arg}={p!r} folds BatchNorm2d and has no backward, but the features require grad: "
                               f"run under torch.no_grad(), or leave {arg} at 'auto' or 'torch'")
        return "torch"

    def _stock_regularizer(self):
        """dres0..4 and classify are the stock modules and nothing else runs when they are called: the layout
        ``layer_plan`` reads, no forward (pre-)hooks on the blocks or anything inside them."""
        plan_mods = set()
        try:
            for conv, bn, _, _ in self.layer_plan():
                if type(conv) is not nn.Conv3d or conv.bias is not None or (bn is not None and
                                                                            type(bn) is not nn.BatchNorm3d):
                    return False
                plan_mods.add(conv)
                plan_mods.add(bn)
        except (AttributeError, IndexError, TypeError):
            return False
        for name in ("dres0", "dres1", "dres2", "dres3", "dres4", "classify"):
            for m in getattr(self, name).modules():
                if m._forward_hooks or m._forward_pre_hooks:
                    return False
                if not isinstance(m, (nn.Sequential, nn.ReLU)) and m not in plan_mods:
                    return False
        return True

    def regularize_grad_route(self, device=None):
        """How the differentiable route runs dres0..4 and classify at this
        call: "torch" or "fp16" (see ``regularize_grad``)."""
        p = self.regularize_grad
        if p == "torch":
            return p
        on_gpu = device is not None and torch.device(device).type == "cuda"
        half = on_gpu and torch.is_autocast_enabled() and _autocast_gpu_dtype() == torch.float16
        if p == "fp16":
            if not half:
                raise RuntimeError("regularize_grad='fp16' computes the stack in float16 on the GPU: call the model "
                                   "on a CUDA device under torch.autocast('cuda', torch.float16), or leave "
                                   "regularize_grad at 'auto' or 'torch'")
            return p
        return "fp16" if half and STACK_BWD_HIP and self._stock_regularizer() else "torch"

    def context_grad_route(self, device=None):
        """How the differentiable route runs the context stack at this call:
        "torch" or "fp16" (see ``context_grad``)."""
        p = self.context_grad
        if p == "torch":
            return p
        on_gpu = device is not None and torch.device(device).type == "cuda"
        if not (on_gpu and torch.is_autocast_enabled() and _autocast_gpu_dtype() == torch.float16):
            raise RuntimeError("context_grad='fp16' computes the context stack in float16 on the GPU: call the model "
                               "on a CUDA device under torch.autocast('cuda', torch.float16), or leave "
                               "context_grad at 'torch'")
        return p

    def dep_context_grad_route(self, device=None):
        """How the differentiable route runs ``dep_convs`` at this call:
        "torch" or "fp16" (see ``dep_context_grad``)."""
        p = self.dep_context_grad
        if p == "torch":
            return p
        on_gpu = device is not None and torch.device(device).type == "cuda"
        if not (on_gpu and torch.is_autocast_enabled() and _autocast_gpu_dtype() == torch.float16):
            raise RuntimeError("dep_context_grad='fp16' computes the refinement stack in float16 on the GPU: call the "
                               "model on a CUDA device under torch.autocast('cuda', torch.float16), or leave "
                               "dep_context_grad at 'torch'")
        return p

    def _regularize_modules(self, cost):
        """dres0..4 and classify as PSNet.py:160-165 calls them: the modules themselves, which carry a gradient
        and whose BatchNorm follows self.training (the matrix-core stack folds it and has no backward)."""
        c0 = self.dres0(cost)
        for i in range(1, 5):
            c0 = getattr(self, f"dres{i}")(c0) + c0
        return self.classify(c0)

    def _head(self, differentiable, cost, H, W, pbd, scale=None):
        """The soft-argmin head on a [B, L, h, w] cost: ``depth_head``, or on the differentiable route
        ``depth_head_autograd`` (the same bits) or, with HEAD_BWD_HIP off, PSNet.py:194-216 in torch ops."""
        if not differentiable:
            return depth_head(cost, self.nlabel, self.mindepth, (H, W), pbd, scale=scale)
        if HEAD_BWD_HIP:
            return depth_head_autograd(cost, self.nlabel, self.mindepth, (H, W), pbd, scale=scale)
        return torch_depth_head(cost, self.nlabel, self.mindepth, (H, W), pbd, scale=scale)

    def forward(self, ref, targets, pose, intrinsics, intrinsics_inv, pose_gt=None, depth_gt=None, E_mat=None):
        c = self.cfg
        K4, Ki4 = quarter_intrinsics(intrinsics.float(), intrinsics_inv.float())
        if c.get("RESCALE_DEPTH", False):
            pose[:, 0, :, -1:] = pose[:, 0, :, -1:] * c.NORM_TARGET      # in place, PSNet.py:135-136
        pbd = bool(c.get("PREDICT_BY_DEPTH", False))
        fused = fused_channels_last(self.cost_dtype, self.conv_precision)
        ref_raw, *tgt_raws = self._features("feature_extraction", [ref] + list(targets))
        # the differentiable route (see the class docstring): grad mode on and features that require grad
        diff = torch.is_grad_enabled() and any(f.requires_grad for f in [ref_raw] + tgt_raws)
        # the float32 copy of the reference features, made where something reads it: the sweep of anything but
        # float16 features on the fused route, the context stack, PSNET_DEP_CONTEXT
        ref_fea = None
        dep_src = ref_raw           # what PSNET_DEP_CONTEXT upsamples: refimg_fea as PSNet.py:219 finds it
        costs = None
        for j, target in enumerate(targets):
            tgt_raw = tgt_raws[j]
            if diff:
                # sweep and stack with a backward: the float32 planar volume, then the modules themselves
                ref_fea = ref_raw.float() if ref_fea is None else ref_fea
                cost = plane_sweep_cost_autograd(ref_fea, tgt_raw.float(), pose[:, j].float(), K4, Ki4, self.nlabel,
                                                 self.mindepth, predict_by_depth=pbd)
                if self.regularize_grad_route(cost.device) == "fp16":
                    c0 = self.forward_differentiable(cost, norm=self.regularize_norm)
                else:
                    c0 = self._regularize_modules(cost)
                costs = c0 if costs is None else costs + c0
                continue
            if fused and f16_features(ref_raw, tgt_raw):
                # MIXED_PREC: the fused sweep reads the float16 features as they come (the same bits)
                r, t = ref_raw, tgt_raw
            else:
                ref_fea = ref_raw.float() if ref_fea is None else ref_fea
                r, t = ref_fea, tgt_raw.float()
            if fused:
                # the sweep writes the stack's channels-last input itself: the same bits, no planar volume
                c0 = sweep_regularize_fused(self, r.contiguous(), t.contiguous(),
                                            pose[:, j].float().contiguous(), K4, Ki4, self.nlabel, self.mindepth,
                                            self.conv_precision, pbd)
            else:
                cost = plane_sweep_cost(r.contiguous(), t.contiguous(),
                                        pose[:, j].float().contiguous(), K4, Ki4, self.nlabel, self.mindepth,
                                        dtype=self.cost_dtype, predict_by_depth=pbd)
                c0 = self.regularize(cost)
            costs = c0 if costs is None else costs + c0
        costs = costs / len(targets)                                   # [B, 1, L, h, w]
        B, _, L, h, w = costs.shape
        H, W = ref.shape[2], ref.shape[3]
        costss = costs
        route = None
        if c.get("PSNET_CONTEXT", True):
            route = self._grad_stack_route("context_precision", self.context_route, costs.device) if diff else \
                self.context_route(costs.device)
            if diff and self.context_grad_route(costs.device) == "fp16":
                route = "grad-fp16"
        if route == "grad-fp16":
            # the stack with a backward on libsfm_hip: the planes b-major, as on the forward-only HIP route
            ctx = self._features("context_net", [ref])[0] if c.get("IND_CONTEXT", False) else ref_raw  # 177-178
            dep_src = ctx
            costss = context_refine_autograd(self.convs, ctx, costs.float())
        elif route in ("fp16", "bf16"):
            # the stack on libsfm_hip: the features in whatever dtype they arrive (no float32 copy), the planes
            # b-major, so the result is already the [B, L, h, w] volume the head reads
            ctx = self._features("context_net", [ref])[0] if c.get("IND_CONTEXT", False) else ref_raw  # 177-178
            dep_src = ctx
            costss = context_refine(self.convs, ctx, costs.float(), precision=route)
        elif route == "torch":
            if c.get("IND_CONTEXT", False):
                ref_fea = self._features("context_net", [ref])[0].float()      # PSNet.py:177-178 reassigns refimg_fea
                dep_src = ref_fea
            elif ref_fea is None:
                ref_fea = ref_raw.float()
            ctx = ref_fea
            # every plane through the same 2-D stack: one batch of B*L images
            planes = costs[:, 0].permute(1, 0, 2, 3).reshape(L * B, 1, h, w)
            x = torch.cat([ctx.unsqueeze(0).expand(L, B, ctx.shape[1], h, w).reshape(L * B, -1, h, w), planes], 1)
            costss = (self.convs(x) + planes).reshape(L, B, h, w).permute(1, 0, 2, 3).unsqueeze(1)
        # PREDICT_BY_DEPTH: depth_init is depthregression's output unscaled,
        # depth is scaled by mindepth (PSNet.py:200-202 vs 209-210)
        depth_init = self._head(diff, costs.reshape(B, L, h, w).contiguous(), H, W, pbd, scale=1.0 if pbd else None)
        depth = self._head(diff, costss.reshape(B, L, h, w).contiguous(), H, W, pbd)
        if c.get("PSNET_DEP_CONTEXT", False):
            droute = self._grad_stack_route("dep_context_precision", self.dep_context_route, depth.device) if diff \
                else self.dep_context_route(depth.device)
            if diff and self.dep_context_grad_route(depth.device) == "fp16":
                # the stack with a backward on libsfm_hip; depth goes in attached: the function routes only the
                # gradient of the "+ depth" residual to it, as the reference's cat of depth.detach() does
                return depth, dep_context_refine_autograd(self.dep_convs, depth, dep_src, ref)
            if droute in ("fp16", "bf16"):
                # upsample, cat and the stack on libsfm_hip: the features in the dtype they arrive in, no float32
                # copy, no full-resolution temporary but the stack's own
                return depth, dep_context_refine(self.dep_convs, depth.detach(), dep_src, ref, precision=droute)
            if dep_src is ref_raw:
                ref_fea = ref_raw.float() if ref_fea is None else ref_fea
            else:
                ref_fea = dep_src.float()
            up = F.interpolate(ref_fea, [H, W], mode="bilinear", align_corners=True)
            feat = torch.cat((depth.detach(), up, ref.float()), dim=1)
            return depth, self.dep_convs(feat) + depth
        return depth_init, depth


def default_feature_hw(image_hw):
    """Feature map size of FeatureExtraction for an image (two stride-2 convs)."""
    H, W = image_hw
    h = (H - 1) // 2 + 1
    w = (W - 1) // 2 + 1
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1

