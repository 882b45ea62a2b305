"""HIP depth stage (correlation cost + soft-argmin head) vs the oracle
restatements of REG2D.py:103-109 and PSNet.py:191-213.  Floating-point bar
(north_star): 1e-4 relative on the depth map."""
import pytest
import torch

from oracle import sweep as S

pytestmark = pytest.mark.gpu


def _scene(B, C, h, w, seed):
    from sfm_amd import synth
    ref, tgt = synth.features(B, C, h, w, seed=seed)
    K = synth.intrinsics(B, 4.0 * w, 4.0 * w, 2.0 * w, 2.0 * h)
    pose = synth.relative_pose(B, torch.Generator().manual_seed(seed))
    return ref, tgt, K, torch.inverse(K), pose


@pytest.mark.parametrize("B,C,L,h,w,by_depth", [(2, 32, 16, 12, 20, False), (1, 6, 9, 10, 31, True),
                                                 (1, 32, 128, 24, 78, False)])
def test_correlation_cost(cuda, B, C, L, h, w, by_depth):
    from sfm_amd.depth import correlation_cost
    from sfm_amd.sweep import quarter_intrinsics
    ref, tgt, K, Ki, pose = _scene(B, C, h, w, seed=L)
    K4, Ki4 = quarter_intrinsics(K, Ki)
    got = correlation_cost(ref.to(cuda), tgt.to(cuda), pose.to(cuda), K4.to(cuda), Ki4.to(cuda), L, 0.8,
                           predict_by_depth=by_depth).cpu()
    want = S.correlation_cost(ref, tgt, pose, K, Ki, L, 0.8, predict_by_depth=by_depth)
    assert float(want.abs().max()) > 0.05
    err = (got - want).abs() - (1e-4 * want.abs() + 2e-5)
    assert float(err.max()) <= 0, float((got - want).abs().max())


@pytest.mark.parametrize("B,L,h,w,H,W,by_depth", [(2, 16, 12, 20, 48, 80, False), (1, 128, 24, 78, 96, 312, False),
                                                   (1, 10, 7, 9, 7, 9, True), (2, 12, 5, 6, 17, 23, False)])
def test_depth_head(cuda, B, L, h, w, H, W, by_depth):
    from sfm_amd.depth import depth_head
    g = torch.Generator().manual_seed(L + h)
    cost = torch.randn(B, L, h, w, generator=g) * 3.0
    got = depth_head(cost.to(cuda), L, 1.0, (H, W), predict_by_depth=by_depth).cpu()
    want = S.depth_head(cost, L, 1.0, (H, W), predict_by_depth=by_depth)
    assert got.shape == want.shape == (B, 1, H, W)
    rel = ((got - want).abs() / want.abs()).max()
    assert float(rel) <= 1e-4, float(rel)


def test_correlation_depth_module(cuda):
    from sfm_amd.depth import CorrelationDepth
    B, C, L, h, w = 2, 8, 24, 16, 40
    ref, tgt, K, Ki, pose = _scene(B, C, h, w, seed=3)
    m = CorrelationDepth(L, 1.0, rescale_depth=True, norm_target=0.6)
    got = m(ref.to(cuda), tgt.to(cuda), pose.to(cuda), K.to(cuda), Ki.to(cuda), (4 * h, 4 * w)).cpu()
    cost = S.correlation_cost(ref, tgt, pose, K, Ki, L, 1.0, rescale=0.6)
    want = S.depth_head(cost, L, 1.0, (4 * h, 4 * w))
    rel = ((got - want).abs() / want.abs()).max()
    assert float(rel) <= 1e-4, float(rel)


def test_flow2depth_golden(cuda, golden):
    # models/flow2depth.py run by the reference itself (tests/golden/warp.npz)
    from sfm_amd.depth import flow2depth
    g = golden("warp.npz")["flow2depth"]
    flow = torch.zeros(*g["shape"].tolist(), device=cuda)
    got = flow2depth(torch.from_numpy(g["R"]), torch.from_numpy(g["T"]), flow, torch.from_numpy(g["K"])).cpu()
    want = torch.from_numpy(g["out"])
    assert got.shape == want.shape
    err = (got - want).abs() - (1e-5 * want.abs() + 1e-5)
    assert float(err.max()) <= 0, float((got - want).abs().max())


@pytest.mark.parametrize("H,W", [(37, 53), (376, 1242)])
def test_flow2depth_vs_oracle(cuda, H, W):
    from sfm_amd import synth
    from sfm_amd.depth import flow2depth
    pose = synth.relative_pose(1, torch.Generator().manual_seed(H)).float()
    K = synth.intrinsics(1)
    R, T = pose[:, :, :3], pose[:, :, 3]
    got = flow2depth(R, T, torch.zeros(1, 2, H, W, device=cuda), K).cpu()
    want = S.flow2depth(R, T, torch.zeros(1, 2, H, W), K)
    # fp32 sums of O(1e3) terms in another order; near-cancelling outputs keep
    # the operands' absolute rounding (a few ulp of max|out|)
    err = (got - want).abs() - (1e-5 * want.abs() + 1e-6 * float(want.abs().max()))
    assert float(err.max()) <= 0, float((got - want).abs().max())


def _depth_head_f64(cost, L, min_depth, out_hw, by_depth):
    """The head in float64: trilinear align_corners=False on a float64 cost, float64 softmax and regression."""
    import torch.nn.functional as F
    H, W = out_hw
    up = F.interpolate(cost.double().unsqueeze(1), [L, H, W], mode="trilinear", align_corners=False)[:, 0]
    prob = F.softmax(up, dim=1)
    idx = torch.arange(1, L + 1, dtype=torch.float64).reshape(1, L, 1, 1)
    if by_depth:
        return (prob * idx * int(min_depth)).sum(1, keepdim=True) * min_depth
    return min_depth * L / ((prob * idx).sum(1, keepdim=True) + 1e-16)


@pytest.mark.parametrize("B,L,h,w,H,W,by_depth,min_depth,scale", [
    (2, 16, 12, 20, 48, 257, False, 1.0, 100.0),     # the classify logits' O(100); W = 257: a block and one column
    (2, 16, 12, 20, 48, 257, False, 1.0, 1e4),       # nearly an argmax
    (1, 16, 12, 20, 5, 9, False, 1.0, 100.0),        # downsampling in both axes
    (1, 12, 12, 20, 12, 45, False, 1.0, 100.0),      # rows identity, columns resized
    (1, 12, 12, 20, 30, 20, True, 2.0, 100.0),       # columns identity; depth regression with a step of 2
    (1, 1, 6, 7, 13, 15, False, 1.0, 100.0),         # one plane
    (1, 1, 6, 7, 13, 15, True, 3.0, 100.0),
])
def test_depth_head_vs_float64(cuda, B, L, h, w, H, W, by_depth, min_depth, scale):
    """Large logits, downsampling, an identity axis, the block edge and one
    plane against the same computation in float64: 1e-4 relative on the depth.

    Measured on an MI355X (largest relative distance): at most 8.3e-8 in every
    case.  With the interpolation weights and the interpolated logit in
    float32, as PyTorch's float32 head forms them, the 48 x 257 cases were
    1.83e-4 (logits of O(100)) and 1.90e-3 (1e4) away, exactly as far as
    oracle.sweep.depth_head on the CPU is from float64 on the same inputs:
    about 1e-6 on a weight times tap differences of several hundred, or of
    1e4.  k_depth_head now interpolates and normalises in float64."""
    from sfm_amd.depth import depth_head
    g = torch.Generator().manual_seed(1000 + L + H + int(scale))
    cost = torch.randn(B, L, h, w, generator=g) * scale
    got = depth_head(cost.to(cuda), L, min_depth, (H, W), predict_by_depth=by_depth).cpu()
    want = _depth_head_f64(cost, L, min_depth, (H, W), by_depth)
    assert got.shape == want.shape == (B, 1, H, W)
    assert bool(torch.isfinite(got).all())
    rel = ((got.double() - want).abs() / want.abs()).max()
    print({"shape": (B, L, h, w, H, W), "by_depth": by_depth, "scale": scale, "rel": float(rel)})
    assert float(rel) <= 1e-4, float(rel)
