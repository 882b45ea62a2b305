"""The soft-argmin head's backward kernel (sfm_depth_head_backward,
csrc/depth_bwd.hip) and its Python surface (sfm_amd.depth.depth_head_autograd):
exact and closed-form cases, general cases against float64 autograd, the
fixture pinned to the reference's own autograd, and the surface.

The general bar.  err = max|g - g64| / max|g64| against torch's own ops in
float64 on the CPU (F.interpolate trilinear, softmax, the regression sums);
bar = max(2 x the err of torch's float32 autograd of the same graph on the
GPU, measured in the same test; 1e-5).  The factor 2 is the margin the project
gives its other stacks against torch's own error; the floor covers benign
inputs, where both errors are rounding noise: p_l carries at most about
1.2e-6 relative error (expf's 2 ulp plus the float32 rounding of v - m at
|v - m| <= 16), and 1e-5 gives that 8x headroom."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _torch_head(cost, L, min_depth, out_hw, by_depth, scale=None):
    """PSNet.py:194-216 in torch ops, in the cost's dtype and on its device."""
    H, W = out_hw
    up = F.interpolate(cost.unsqueeze(1), [L, H, W], mode="trilinear", align_corners=False)[:, 0]
    prob = F.softmax(up, dim=1)
    idx = torch.arange(1, L + 1, dtype=cost.dtype, device=cost.device).reshape(1, L, 1, 1)
    if by_depth:
        return (prob * (idx * int(min_depth))).sum(1, keepdim=True) * (min_depth if scale is None else scale)
    return min_depth * L / ((prob * idx).sum(1, keepdim=True) + 1e-16)


def _autograd(cost, g, L, min_depth, out_hw, by_depth, scale, dtype, device):
    c = cost.to(device=device, dtype=dtype).requires_grad_()
    _torch_head(c, L, min_depth, out_hw, by_depth, scale).backward(g.to(device=device, dtype=dtype))
    return c.grad.cpu()


def _hip(cuda, cost, g, L, min_depth, out_hw, by_depth, scale=None):
    """(depth, grad_cost) of depth_head_autograd on CPU tensors, back on the CPU."""
    from sfm_amd.depth import depth_head_autograd
    c = cost.to(cuda).requires_grad_()
    out = depth_head_autograd(c, L, min_depth, out_hw, predict_by_depth=by_depth, scale=scale)
    out.backward(g.to(cuda))
    return out.detach().cpu(), c.grad.cpu()


def _err(g, g64):
    return float((g.double() - g64).abs().max() / g64.abs().max())


def _inputs(B, L, h, w, H, W, seed, logits="benign"):
    gen = torch.Generator().manual_seed(seed)
    if logits == "benign":
        cost = 3.0 * torch.randn(B, L, h, w, generator=gen)
    else:
        # the regime depth.hip's comments describe: logits of order 1e2, and the plane after the best one
        # nearly tied with it, so the soft-argmin hangs on small differences of large interpolated values
        cost = 100.0 * torch.randn(B, L, h, w, generator=gen)
        top, arg = cost.max(1, keepdim=True)
        cost.scatter_(1, (arg + 1) % L, top - 0.05 * torch.rand(B, 1, h, w, generator=gen))
    return cost, torch.randn(B, 1, H, W, generator=gen)


# (B, L, h, w, H, W, logits)
CASES = {
    "non_integer_ratios": (2, 13, 5, 7, 18, 27, "benign"),
    "ratio_4": (1, 8, 6, 8, 24, 32, "benign"),
    "two_blocks_in_x": (1, 4, 3, 75, 7, 300, "benign"),          # more than one 256-thread block in X
    "one_row": (1, 5, 1, 6, 4, 24, "benign"),                    # size-1 axes
    "one_column": (1, 5, 6, 1, 24, 4, "benign"),
    "large_logits": (2, 9, 5, 7, 18, 27, "tied"),
}
# disparity; PREDICT_BY_DEPTH with a step of 2 under a multiplier of 2.5
MODES = {"disp": (False, 1.0), "depth": (True, 2.5)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_backward_vs_float64_autograd(cuda, case, mode):
    B, L, h, w, H, W, logits = CASES[case]
    by_depth, min_depth = MODES[mode]
    # depth_head's scale= override (PSNet's depth_init under PREDICT_BY_DEPTH) rides along on one depth-mode case
    scale = 1.0 if (by_depth and case == "non_integer_ratios") else None
    cost, g = _inputs(B, L, h, w, H, W, seed=len(case) + 100 * by_depth, logits=logits)
    g64 = _autograd(cost, g, L, min_depth, (H, W), by_depth, scale, torch.float64, "cpu")
    g32 = _autograd(cost, g, L, min_depth, (H, W), by_depth, scale, torch.float32, cuda)
    depth, got = _hip(cuda, cost, g, L, min_depth, (H, W), by_depth, scale)
    assert got.shape == cost.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    ours, theirs = _err(got, g64), _err(g32, g64)
    bar = max(2.0 * theirs, 1e-5)
    print({"case": case, "mode": mode, "err_hip": ours, "err_torch_f32": theirs, "bar": bar})
    assert float(g64.abs().max()) > 0 and ours <= bar, (ours, theirs, bar)


def test_reference_fixture(cuda, golden):
    """The reference's own head (its disparityregression / depthregression,
    scripts/gen_depth_head_grad_golden.py): the kernel against float64 under the
    general bar, with the reference's float32 gradient as torch's arm."""
    fx = golden("depth_head_grad.npz")
    for group in ("disp", "depth"):
        f = fx[group]
        cost, g = torch.from_numpy(f["cost"]), torch.from_numpy(f["g"])
        L, min_depth, by_depth = int(f["nlabel"]), float(f["min_depth"]), bool(f["predict_by_depth"])
        hw = tuple(int(x) for x in f["out_hw"])
        assert cost.dim() == 5 and by_depth == (group == "depth")
        g64 = _autograd(cost[:, 0], g, L, min_depth, hw, by_depth, None, torch.float64, "cpu")
        depth, got = _hip(cuda, cost, g, L, min_depth, hw, by_depth)
        assert got.shape == cost.shape
        ours, theirs = _err(got[:, 0], g64), _err(torch.from_numpy(f["grad_cost"])[:, 0], g64)
        bar = max(2.0 * theirs, 1e-5)
        print({"fixture": group, "err_hip": ours, "err_reference_f32": theirs, "bar": bar})
        assert ours <= bar, (group, ours, theirs, bar)
        want = torch.from_numpy(f["depth"])
        assert float(((depth - want).abs() / want.abs()).max()) <= 1e-4          # the forward's own bar


@pytest.mark.parametrize("by_depth", [False, True])
def test_one_plane_has_no_gradient(cuda, by_depth):
    """L = 1: the softmax is 1 whatever the cost, so grad_cost is exactly 0."""
    cost, g = _inputs(2, 1, 3, 4, 7, 9, seed=5)
    _, got = _hip(cuda, cost, g, 1, 2.0 if by_depth else 1.0, (7, 9), by_depth)
    assert torch.equal(got, torch.zeros_like(got))


@pytest.mark.parametrize("by_depth", [False, True])
def test_identity_size_closed_form(cuda, by_depth):
    """H = h, W = w: every cell has one contributor of weight 1, so grad_cost
    is d p_l (val_l - reg), here in float64 from the device's float32
    exponentials of the same rounded differences, within one float32 rounding."""
    B, L, h, w = 2, 7, 5, 9
    min_depth = 2.5 if by_depth else 1.0
    cost, g = _inputs(B, L, h, w, h, w, seed=6)
    _, got = _hip(cuda, cost, g, L, min_depth, (h, w), by_depth)
    v = cost.double()
    diff = (v - v.max(1, keepdim=True).values).float()
    e = torch.exp(diff.to(cuda)).cpu().double()
    p = e / e.sum(1, keepdim=True)
    val = (torch.arange(1, L + 1, dtype=torch.float32) * (float(int(min_depth)) if by_depth else 1.0)).double()
    val = val.reshape(1, L, 1, 1)
    reg = (p * val).sum(1, keepdim=True)
    d = g.double() * (min_depth if by_depth else -(min_depth * L) / (reg + 1e-16) ** 2)
    want = d * p * (val - reg)
    ulp = torch.from_numpy(np.spacing(want.float().abs().numpy()))
    assert bool(((got.double() - want).abs() <= ulp.double()).all()), float(((got.double() - want).abs() / ulp).max())


def _taps(dst, in_size, out_size):
    if in_size == out_size:
        return dst, dst
    src = max((in_size / out_size) * (dst + 0.5) - 0.5, 0.0)
    i0 = min(int(math.floor(src)), in_size - 1)
    return i0, i0 + (1 if i0 < in_size - 1 else 0)


@pytest.mark.parametrize("H,W", [(5, 6), (2, 3)])
def test_downsample_unread_cells_are_zero(cuda, H, W):
    """9 x 11 -> 5 x 6 and -> 2 x 3: a cell no output pixel reads gets exactly
    0.  At 5 x 6 the taps of the five rows and six columns between them still
    touch every cell (one of them with weight 0); at 2 x 3 whole rows and
    columns are skipped."""
    B, L, h, w = 1, 6, 9, 11
    cost, g = _inputs(B, L, h, w, H, W, seed=7)
    _, got = _hip(cuda, cost, g, L, 1.0, (H, W), False)
    rows = {i for Y in range(H) for i in _taps(Y, h, H)}
    cols = {i for X in range(W) for i in _taps(X, w, W)}
    read = torch.zeros(h, w, dtype=torch.bool)
    for y in rows:
        for x in cols:
            read[y, x] = True
    assert 0 < int(read.sum()) <= h * w and ((H, W) != (2, 3) or int(read.sum()) <= h * w // 2)
    assert bool((got[:, :, ~read] == 0).all())
    assert bool((got[:, :, read] != 0).any())
    g64 = _autograd(cost, g, L, 1.0, (H, W), False, None, torch.float64, "cpu")
    assert bool((g64[:, :, ~read] == 0).all()) and _err(got, g64) <= 1e-5


@pytest.mark.parametrize("by_depth", [False, True])
def test_zero_gradient_reproducibility_and_shift_invariance(cuda, by_depth):
    B, L, h, w, H, W = 2, 13, 5, 7, 18, 27
    min_depth = 2.5 if by_depth else 1.0
    cost, g = _inputs(B, L, h, w, H, W, seed=8)
    _, zero = _hip(cuda, cost, torch.zeros_like(g), L, min_depth, (H, W), by_depth)
    assert bool((zero == 0).all())
    _, a = _hip(cuda, cost, g, L, min_depth, (H, W), by_depth)
    _, b = _hip(cuda, cost, g, L, min_depth, (H, W), by_depth)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))           # a gather in a fixed order: the same bits
    # softmax's shift invariance: the plane sum of the gradient vanishes; the bound is the float32 store
    # rounding over L <= 13 terms
    total, mag = a.double().sum(1), a.double().abs().sum(1)
    assert bool((mag > 0).all()) and bool((total.abs() <= 1e-6 * mag).all()), float((total.abs() / mag).max())


def test_python_surface(cuda):
    import sfm_amd
    from sfm_amd.depth import depth_head, depth_head_autograd
    assert sfm_amd.depth_head_autograd is depth_head_autograd
    B, L, h, w, H, W = 2, 6, 5, 7, 18, 27
    cost, g = _inputs(B, L, h, w, H, W, seed=9)
    c = cost.to(cuda)
    for by_depth, scale in ((False, None), (True, None), (True, 1.0)):
        want = depth_head(c, L, 2.0, (H, W), by_depth, scale=scale)
        got = depth_head_autograd(c.clone().requires_grad_(), L, 2.0, (H, W), by_depth, scale=scale)
        assert got.grad_fn is not None and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # a 5-D cost and a float16 cost: gradients of the input's shape and dtype
    c5 = c.unsqueeze(1).clone().requires_grad_()
    depth_head_autograd(c5, L, 1.0, (H, W)).backward(g.to(cuda))
    c4 = c.clone().requires_grad_()
    depth_head_autograd(c4, L, 1.0, (H, W)).backward(g.to(cuda))
    assert c5.grad.shape == c5.shape and torch.equal(c5.grad[:, 0], c4.grad)
    ch = c.half().requires_grad_()
    depth_head_autograd(ch, L, 1.0, (H, W)).backward(g.to(cuda))
    assert ch.grad.dtype == torch.float16 and ch.grad.shape == ch.shape and bool((ch.grad != 0).any())
    # a non-contiguous grad_depth is made contiguous: the same bits as the contiguous one
    cn = c.clone().requires_grad_()
    gn = g.to(cuda).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not gn.is_contiguous()
    depth_head_autograd(cn, L, 1.0, (H, W)).backward(gn)
    assert torch.equal(cn.grad, c4.grad)
    # only the cost gets a gradient, and only once
    assert depth_head_autograd(c, L, 1.0, (H, W)).grad_fn is None
    cd = c.clone().requires_grad_()
    gg, = torch.autograd.grad(depth_head_autograd(cd, L, 1.0, (H, W)).sum(), cd, create_graph=True)
    assert gg.grad_fn is None and not gg.requires_grad                     # once_differentiable: no graph of the backward
    # depth_head itself stays forward-only and silent
    out = depth_head(c.clone().requires_grad_(), L, 1.0, (H, W))
    assert out.grad_fn is None and not out.requires_grad
