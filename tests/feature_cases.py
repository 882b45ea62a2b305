"""Shared inputs of the feature-CNN tests (tests/test_feature.py,
tests/test_gpu_feature.py): the seeded weight recipe, the float64 yardstick and
the float64 bilinear upsample written out term by term."""
import copy
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

IMAGE = (2, 3, 130, 150)        # -> a 33 x 38 feature map: ragged against the 64-column tile, both stride-2 layers
MAP = (33, 38)                  # see odd sizes, the pools floor to 1 x 1, 2 x 2, 4 x 4 and 8 x 9


def recipe():
    """(net, image): FeatureExtraction in eval mode with Kaiming conv
    weights, seeded non-trivial BatchNorm statistics and affines, every
    residual block's second BatchNorm damped by 0.25 (without it the 25
    "+ x" in a row reach 5e7, which overflows float16 on any route), and an
    image in [-1, 1)."""
    from sfm_amd.psnet import FeatureExtraction, _Residual
    torch.manual_seed(0)
    net = FeatureExtraction()
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    g = torch.Generator().manual_seed(7)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.data = 0.1 * torch.randn(n, generator=g)
            m.running_var.data = 0.5 + torch.rand(n, generator=g)
            m.weight.data = 0.8 + 0.4 * torch.rand(n, generator=g)
            m.bias.data = 0.1 * torch.randn(n, generator=g)
    for m in net.modules():
        if isinstance(m, _Residual):
            m.conv2[1].weight.data *= 0.25
            m.conv2[1].bias.data *= 0.25
    image = torch.rand(*IMAGE, generator=g) * 2 - 1
    return net.eval(), image


@functools.lru_cache(maxsize=None)
def recipe_case():
    """(net, image, float64 CPU forward [2, 32, 33, 38]); shared, never modified."""
    net, image = recipe()
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(image.double())
    assert tuple(ref.shape) == (IMAGE[0], 32) + MAP
    return net, image, ref


def up64(m, h, w):
    """Bilinear align_corners=True upsample of m [n, hi, wi, c] to [n, h, w, c]
    in float64, torch's upsample_bilinear2d term by term: src = scale * dst
    with scale = (in - 1) / (out - 1) (0 for out == 1), i0 = min(int(src),
    in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1,
    value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)."""
    m = m.double()
    hi, wi = m.shape[1], m.shape[2]

    def axis(n_in, n_out):
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        src = torch.arange(n_out, dtype=torch.float64) * scale
        i0 = src.long().clamp(max=n_in - 1)
        i1 = i0 + (i0 < n_in - 1).long()
        l1 = src - i0.double()
        return i0, i1, 1.0 - l1, l1
    y0, y1, ly0, ly1 = axis(hi, h)
    x0, x1, lx0, lx1 = axis(wi, w)
    lx0, lx1 = lx0.view(1, 1, w, 1), lx1.view(1, 1, w, 1)
    ly0, ly1 = ly0.view(1, h, 1, 1), ly1.view(1, h, 1, 1)
    top = lx0 * m[:, y0][:, :, x0] + lx1 * m[:, y0][:, :, x1]
    bot = lx0 * m[:, y1][:, :, x0] + lx1 * m[:, y1][:, :, x1]
    return ly0 * top + ly1 * bot


def composed64(packed, image):
    """The packed layers (sfm_amd.feature.pack_feature_extraction) composed in
    float64 on the CPU in feature_extract's order -> [B, 32, h, w]."""
    def layer(x, lay, residual=None):
        k, cin = lay["ksize"], lay["cin_pad"]
        w = lay["w"].double().reshape(k, k, lay["cout_pad"], cin).permute(2, 3, 0, 1)
        if x.shape[1] < cin:
            x = F.pad(x, (0, 0, 0, 0, 0, cin - x.shape[1]))
        y = F.conv2d(x, w, stride=lay["stride"], dilation=lay["dilation"], padding=lay["dilation"] if k == 3 else 0)
        y = y * lay["scale"].double().view(1, -1, 1, 1) + lay["bias"].double().view(1, -1, 1, 1)
        if lay["relu"]:
            y = F.relu(y)
        return y if residual is None else y + residual
    x = image.double()
    for lay in packed["first"]:
        x = layer(x, lay)
    raw = None
    for i, blks in enumerate(packed["layers"]):
        for c1, c2, ds in blks:
            x = layer(layer(x, c1), c2, residual=x if ds is None else layer(x, ds))
        if i == 1:
            raw = x
    h, w = x.shape[2:]
    pyr = [up64(layer(F.avg_pool2d(x, p, p), lay).permute(0, 2, 3, 1), h, w).permute(0, 3, 1, 2)
           for p, lay in packed["branches"]]
    y = torch.cat([raw, x] + pyr[::-1], 1)
    for lay in packed["last"]:
        y = layer(y, lay)
    return y
