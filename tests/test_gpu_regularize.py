"""HIP PSNet cost regularisation (sfm_conv3_bf16, 12-layer dres/classify
stack) vs the oracle (oracle/regularize.py, PSNet.py:159-165).

Tolerances (floating point, bf16 storage with fp32 accumulation):
* channels-last conversion: bit-exact (round to nearest even);
* one layer: within half a bf16 ulp (2^-8 relative) of the fp32 conv of the
  same bf16 inputs (the stored value is the RNE rounding of an fp32 sum that
  differs only in summation order);
* every layer of the stack, fed the oracle's own bf16 input (teacher
  forcing): within half a bf16 ulp, as for one layer;
* the whole stack: relative L2 error <= 2e-2 against the bf16-storage oracle
  and <= 3e-2 against the fp32 reference stack.  12 bf16-stored layers are
  chaotic in summation order: the CPU oracle computed with float64 sums
  instead of float32 already moves 5e-3 (relative L2) on these inputs;
* the depth map (sweep -> stack -> soft-argmin head): median relative error
  <= 1e-3 and relative L2 <= 8e-2 against the oracle chain with either
  stack.  The classify logits reach O(100), so the soft-argmin is nearly an
  argmax and inherits the stack's bf16 sensitivity: on these inputs the
  bf16-storage oracle itself is 2.9-4.0e-2 (relative L2) from the fp32 one.
  (The north-star 1e-4 depth bar applies to the fp32 sweep + head path,
  tests/test_gpu_depth.py; this stack computes in bf16 by design.)"""
import pytest
import torch
import torch.nn.functional as F

from oracle import regularize as R
from oracle import sweep as S

pytestmark = pytest.mark.gpu


def _module(seed, cin=64):
    from tests.test_regularize import _module as m
    return m(seed, cin)


def _bf16_ulp_close(got, want):
    # got = bf16(RNE) of an fp32 sum that differs from want only in order:
    # within half a bf16 ulp (<= 2^-8 |want|) plus the fp32 reordering slack
    tol = 2.0 ** -8 * want.abs() * 1.001 + 1e-5
    bad = (got - want).abs() > tol
    return int(bad.sum()), float((got - want).abs().max())


@pytest.mark.parametrize("shape", [(2, 64, 5, 7, 13), (2, 64, 4, 10, 30), (1, 32, 4, 6, 9), (1, 64, 2, 16, 16)])
def test_channels_last_bit_exact(cuda, shape):
    # (5, 7, 13): generic kernel; the others (plane % 4 == 0): the float4 kernel
    from sfm_amd.regularize import to_channels_last
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(1)) * 10
    got = to_channels_last(x.to(cuda)).cpu()
    want = x.permute(0, 2, 3, 4, 1).to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    got2 = to_channels_last(x.to(torch.bfloat16).to(cuda)).cpu()
    assert torch.equal(got2.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("B,cin,D,h,w,relu,resid,cout", [
    (1, 32, 3, 4, 64, False, False, 32),
    (2, 64, 5, 7, 70, True, False, 32),
    (1, 32, 4, 9, 131, False, True, 32),
    (1, 32, 6, 5, 33, False, False, 1),
    (1, 64, 1, 1, 1, True, False, 32),
])
def test_conv_layer(cuda, B, cin, D, h, w, relu, resid, cout):
    from sfm_amd.regularize import conv3_bf16
    g = torch.Generator().manual_seed(B * 100 + cin + D + h + w)
    x = torch.randn(B, cin, D, h, w, generator=g).to(torch.bfloat16).float()
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1).to(torch.bfloat16).float()
    scale = 0.5 + torch.rand(cout, generator=g)
    bias = 0.3 * torch.randn(cout, generator=g)
    res = torch.randn(B, 32, D, h, w, generator=g).to(torch.bfloat16).float() if resid else None
    want = F.conv3d(x, wt, None, 1, 1) * scale.view(1, -1, 1, 1, 1) + bias.view(1, -1, 1, 1, 1)
    if relu:
        want = torch.relu(want)
    if res is not None:
        want = want + res
    wp = torch.zeros(27, 32, cin)
    wp[:, :cout] = wt.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    sc, bi = torch.ones(32), torch.zeros(32)
    sc[:cout], bi[:cout] = scale, bias
    xcl = x.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).to(cuda)
    rcl = None if res is None else res.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).to(cuda)
    got = conv3_bf16(xcl, wp.to(torch.bfloat16).to(cuda), sc, bi, rcl, relu, cout).cpu()
    if cout == 32:
        got = got.float().permute(0, 4, 1, 2, 3)
        nbad, mx = _bf16_ulp_close(got, want)
        assert nbad == 0, (nbad, mx)
    else:
        want = want[:, 0]
        err = (got - want).abs() - (1e-5 * want.abs() + 1e-5)
        assert float(err.max()) <= 0, float((got - want).abs().max())


@pytest.mark.parametrize("B,cin,L,h,w", [(1, 64, 16, 12, 20), (2, 64, 8, 9, 70), (1, 32, 7, 5, 67)])
def test_stack_vs_oracle(cuda, B, cin, L, h, w):
    m = _module(11 + L, cin)
    cost = torch.randn(B, cin, L, h, w, generator=torch.Generator().manual_seed(L))
    got = m.to(cuda)(cost.to(cuda), precision="bf16").cpu()
    m = m.cpu()
    want16 = R.regularize_bf16(m, cost)
    want32 = R.regularize_fp32(m, cost)
    assert got.shape == want32.shape == (B, 1, L, h, w)
    r16 = float((got - want16).norm() / want16.norm())
    r32 = float((got - want32).norm() / want32.norm())
    assert r16 <= 2e-2, r16
    assert r32 <= 3e-2, r32


def test_stack_full_kitti_size_crop(cuda):
    # C2 geometry (L=128, 94x311): the full-size result restricted to a corner
    # crop equals the oracle run on the crop, away from the crop's cut faces
    # (12 layers -> receptive radius 12).
    m = _module(21)
    B, C, L, h, w = 1, 64, 128, 94, 311
    cost = torch.randn(B, C, L, h, w, generator=torch.Generator().manual_seed(4))
    got = m.to(cuda)(cost.to(cuda), precision="bf16").cpu()
    m = m.cpu()
    cl, ch, cw = 28, 28, 30
    crop = cost[:, :, L - cl:, :ch, w - cw:]
    want = R.regularize_bf16(m, crop)
    g = got[:, :, L - cl + 12:, :ch - 12, w - cw + 12:]
    wv = want[:, :, 12:, :ch - 12, 12:]
    r = float((g - wv).norm() / wv.norm())
    assert r <= 2e-2, r


def test_psnet_depth_end_to_end(cuda):
    from sfm_amd import synth
    from sfm_amd.regularize import psnet_depth
    B, C, h, w, L = 1, 32, 12, 20, 16
    ref, tgt = synth.features(B, C, h, w, seed=3)
    K = synth.intrinsics(B, 4.0 * w, 4.0 * w, 2.0 * w, 2.0 * h)
    Ki = torch.inverse(K)
    pose = synth.relative_pose(B, torch.Generator().manual_seed(3))
    m = _module(7)
    got = psnet_depth(ref.to(cuda), tgt.to(cuda), pose.to(cuda), K.to(cuda), Ki.to(cuda), m.to(cuda), L, 1.0,
                      out_hw=(4 * h, 4 * w), precision="bf16").cpu()
    m = m.cpu()
    cost = S.plane_sweep_cost(ref, tgt, pose, K, Ki, L, 1.0)
    for stack in (R.regularize_bf16, R.regularize_fp32):
        want = S.depth_head(stack(m, cost), L, 1.0, out_hw=(4 * h, 4 * w))
        rel = ((got - want).abs() / want.abs()).flatten()
        r = float((got - want).norm() / want.norm())
        assert float(rel.median()) <= 1e-3, float(rel.median())
        assert r <= 8e-2, r


def test_stack_layers_teacher_forced(cuda):
    from sfm_amd.regularize import conv3_bf16
    m = _module(31)
    B, L, h, w = 1, 6, 11, 70
    cost = torch.randn(B, 64, L, h, w, generator=torch.Generator().manual_seed(5))
    packed = m.to(cuda).pack(cuda)
    m = m.cpu()
    x = cost.to(torch.bfloat16).float()
    keep = None
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).to(cuda)
    for li, ((conv, bn, relu, resid), lay) in enumerate(zip(m.layer_plan(), packed)):
        with torch.no_grad():
            want = R._conv_bn(x, conv, bn, R._bf16)
            if relu:
                want = torch.relu(want)
            if resid:
                want = want + keep
        got = conv3_bf16(cl(x), lay["w"], lay["scale"], lay["bias"], cl(keep) if resid else None, relu,
                         lay["cout"]).cpu()
        if lay["cout"] == 32:
            nbad, mx = _bf16_ulp_close(got.float().permute(0, 4, 1, 2, 3), want)
            assert nbad == 0, (li, nbad, mx)
        else:
            err = (got - want[:, 0]).abs() - (1e-5 * want[:, 0].abs() + 1e-4)
            assert float(err.max()) <= 0, (li, float((got - want[:, 0]).abs().max()))
        y = want.to(torch.bfloat16).float()
        if li == 1 or resid:
            keep = y
        x = y


@pytest.mark.parametrize("D,h,w", [(13, 9, 70), (8, 4, 64), (2, 5, 3)])
def test_rolling_kernel_equals_per_plane_kernel(cuda, D, h, w):
    # k_conv3r (planes staged once, rotating accumulators) adds the same
    # products in the same order as k_conv3: bit-identical outputs
    from sfm_amd import _lib
    from sfm_amd.regularize import conv3_bf16
    g = torch.Generator().manual_seed(D + h + w)
    x = torch.randn(1, D, h, w, 32, generator=g).to(torch.bfloat16).to(cuda)
    wp = (torch.randn(27, 32, 32, generator=g) * 0.1).to(torch.bfloat16).to(cuda)
    sc, bi = 0.5 + torch.rand(32, generator=g), 0.1 * torch.randn(32, generator=g)
    res = torch.randn(1, D, h, w, 32, generator=g).to(torch.bfloat16).to(cuda)
    outs = []
    try:
        for rolling in (0, 1):
            _lib.tune("conv_rolling", rolling)
            outs.append((conv3_bf16(x, wp, sc, bi, res, False, 32).cpu(), conv3_bf16(x, wp, sc, bi, None, True, 1).cpu()))
    finally:
        _lib.tune("conv_rolling", 1)
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
    assert torch.equal(outs[0][1], outs[1][1])


def _psnet_golden(golden):
    from sfm_amd.regularize import CostRegularization
    g = golden("psnet.npz")
    m = CostRegularization(64)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["state"].items()})
    return g, m.eval()


def test_psnet_golden_regularisation(cuda, golden):
    """CostRegularization on the reference PSNet's own cost volume with its
    state_dict (psnet.npz) vs its classify output: bf16 storage tolerance, the
    same bar as test_stack_vs_oracle (relative L2 <= 3e-2 vs fp32)."""
    g, m = _psnet_golden(golden)
    got = m.to(cuda)(torch.from_numpy(g["out"]["cost"]).to(cuda), precision="bf16").cpu()
    want = torch.from_numpy(g["out"]["classify"])
    r = float((got - want).norm() / want.norm())
    assert got.shape == want.shape and r <= 3e-2, r


def test_psnet_golden_depth_head(cuda, golden):
    """Soft-argmin head on the reference's classify output vs the reference's
    depth_init: fp32 throughout, within 1e-4 relative (north_star's bar)."""
    from sfm_amd.depth import depth_head
    g = golden("psnet.npz")
    inp = g["input"]
    L = int(inp["nlabel"])
    got = depth_head(torch.from_numpy(g["out"]["classify"]).to(cuda), L, float(inp["min_depth"]),
                     out_hw=tuple(inp["ref_img"].shape[2:])).cpu()
    want = torch.from_numpy(g["out"]["depth_init"])
    rel = float(((got - want).abs() / want.abs()).max())
    assert rel <= 1e-4, rel


def test_psnet_golden_end_to_end(cuda, golden):
    """psnet_depth (sweep -> bf16 regularisation -> head) from the reference's
    features and rescaled pose vs the reference's fp32 depth map (psnet.npz).
    bf16 activation storage (8-bit mantissa) moves the logits by ~0.8 % of
    their scale, i.e. the soft-argmin by ~1 % of the depth: the bars are the
    bf16-storage oracle's own distance to the reference (median 0.84 %, rel.
    L2 2.2 %, max 9.5 %) x1.5; against that oracle (same storage precision,
    different summation order, measured 0.37 %) the median bar is 5e-3."""
    from oracle import regularize as OR
    from sfm_amd.regularize import psnet_depth
    g, m = _psnet_golden(golden)
    inp, out = g["input"], g["out"]
    L = int(inp["nlabel"])
    hw = tuple(inp["ref_img"].shape[2:])
    d = lambda k: torch.from_numpy(k).to(cuda)
    got = psnet_depth(d(out["ref_fea"]), d(out["tgt_fea"]), d(inp["pose_rescaled"])[:, 0], d(inp["K"]),
                      d(inp["Kinv"]), m.to(cuda), L, float(inp["min_depth"]), out_hw=hw, precision="bf16").cpu()
    want = torch.from_numpy(out["depth_init"])
    rel = ((got - want).abs() / want.abs()).flatten()
    r = float((got - want).norm() / want.norm())
    assert float(rel.median()) <= 1.3e-2 and r <= 3.3e-2 and float(rel.max()) <= 0.15, \
        (float(rel.median()), r, float(rel.max()))
    m = m.cpu()
    want16 = S.depth_head(OR.regularize_bf16(m, torch.from_numpy(out["cost"])), L, float(inp["min_depth"]), out_hw=hw)
    rel16 = ((got - want16).abs() / want16.abs()).flatten()
    assert float(rel16.median()) <= 5e-3, float(rel16.median())


# ---------------------------------------------------------------------------
# fp32 path (precision="fp32": sfm_conv3_f32 on v_mfma_f32_32x32x2_f32).
# Tolerances: one layer is the fp32 conv of the same fp32 operands in another
# summation order, so |got - want| <= 2e-5 * conv(|x|, |w|) * |scale| + 1e-6
# (the f32 MFMA rounds every product and sum as float32 arithmetic does; the
# bound is ~4x the sqrt(27 Cin) u random-walk of the reordered sums).

def _conv_f32(cuda, x, wt, scale, bias, res, relu, cout):
    from sfm_amd import _lib
    cin = x.shape[1]
    wp = torch.zeros(27, 32, cin)
    wp[:, :cout] = wt.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    sc, bi = torch.ones(32), torch.zeros(32)
    sc[:cout], bi[:cout] = scale, bias
    xcl = x.permute(0, 2, 3, 4, 1).contiguous().to(cuda)
    rcl = None if res is None else res.permute(0, 2, 3, 4, 1).contiguous().to(cuda)
    B, _, D, h, w = x.shape
    out = torch.empty((B, D, h, w, 32) if cout == 32 else (B, D, h, w), dtype=torch.float32, device=cuda)
    wp, sc, bi = wp.to(cuda), sc.to(cuda), bi.to(cuda)
    with torch.cuda.device(cuda):
        _lib.check(_lib.load().sfm_conv3_f32(_lib.ptr(xcl), B, cin, D, h, w, _lib.ptr(wp), _lib.ptr(sc), _lib.ptr(bi),
                                             None if rcl is None else _lib.ptr(rcl), 1 if relu else 0, cout,
                                             _lib.ptr(out), _lib.stream_ptr(cuda)), "sfm_conv3_f32")
    out = out.cpu()
    return out.permute(0, 4, 1, 2, 3) if cout == 32 else out


@pytest.mark.parametrize("B,cin,D,h,w,relu,resid,cout", [
    (1, 32, 3, 4, 64, False, False, 32),
    (2, 64, 5, 7, 70, True, False, 32),
    (1, 32, 4, 9, 131, False, True, 32),
    (1, 32, 6, 5, 33, False, False, 1),
    (1, 64, 1, 1, 1, True, False, 32),
    (1, 64, 3, 17, 65, True, True, 32),
])
def test_conv_layer_f32(cuda, B, cin, D, h, w, relu, resid, cout):
    g = torch.Generator().manual_seed(B * 100 + cin + D + h + w + 7)
    x = torch.randn(B, cin, D, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
    scale = 0.5 + torch.rand(cout, generator=g)
    bias = 0.3 * torch.randn(cout, generator=g)
    res = torch.randn(B, 32, D, h, w, generator=g) if resid else None
    want = F.conv3d(x, wt, None, 1, 1) * scale.view(1, -1, 1, 1, 1) + bias.view(1, -1, 1, 1, 1)
    mag = F.conv3d(x.abs(), wt.abs(), None, 1, 1) * scale.view(1, -1, 1, 1, 1)
    if relu:
        want = torch.relu(want)
    if res is not None:
        want = want + res
    got = _conv_f32(cuda, x, wt, scale, bias, res, relu, cout)
    if cout == 1:
        want, mag = want[:, 0], mag[:, 0]
    err = (got - want).abs() - (2e-5 * mag + 1e-6)
    assert float(err.max()) <= 0, float((got - want).abs().max())


# fp32x3 path (precision="fp32x3": sfm_conv3_f32x3, each fp32 product from a
# two-term f16 split of both operands on the f16 matrix cores).  One layer:
# every product within ~3 x 2^-22 relative (the two splits and the dropped
# lo x lo term; an activation's lo term can be subnormal: 2^-24 absolute),
# then the f32 accumulation as sfm_conv3_f32 -- the f32 layer bound holds.

def _conv_f32x3(cuda, x, wt, scale, bias, res, relu, cout, flag=None):
    from sfm_amd import _lib
    from sfm_amd.regularize import weight_exponent
    cin = x.shape[1]
    wp = torch.zeros(27, 32, cin)
    wp[:, :cout] = wt.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    sc, bi = torch.ones(32), torch.zeros(32)
    sc[:cout], bi[:cout] = scale, bias
    xcl = x.permute(0, 2, 3, 4, 1).contiguous().to(cuda)
    rcl = None if res is None else res.permute(0, 2, 3, 4, 1).contiguous().to(cuda)
    B, _, D, h, w = x.shape
    out = torch.empty((B, D, h, w, 32) if cout == 32 else (B, D, h, w), dtype=torch.float32, device=cuda)
    e = weight_exponent(wp)
    wp, sc, bi = wp.to(cuda), sc.to(cuda), bi.to(cuda)
    with torch.cuda.device(cuda):
        _lib.check(_lib.load().sfm_conv3_f32x3(_lib.ptr(xcl), B, cin, D, h, w, _lib.ptr(wp), e, _lib.ptr(sc),
                                               _lib.ptr(bi), None if rcl is None else _lib.ptr(rcl), 1 if relu else 0,
                                               cout, _lib.ptr(out), None if flag is None else flag.data_ptr(),
                                               _lib.stream_ptr(cuda)), "sfm_conv3_f32x3")
    out = out.cpu()
    return out.permute(0, 4, 1, 2, 3) if cout == 32 else out


@pytest.mark.parametrize("B,cin,D,h,w,relu,resid,cout", [
    (1, 32, 3, 4, 64, False, False, 32),
    (2, 64, 5, 7, 70, True, False, 32),
    (1, 32, 4, 9, 131, False, True, 32),
    (1, 32, 6, 5, 33, False, False, 1),
    (1, 64, 1, 1, 1, True, False, 32),
    (1, 64, 3, 17, 65, True, True, 32),
])
def test_conv_layer_f32x3(cuda, B, cin, D, h, w, relu, resid, cout):
    g = torch.Generator().manual_seed(B * 100 + cin + D + h + w + 9)
    x = torch.randn(B, cin, D, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
    scale = 0.5 + torch.rand(cout, generator=g)
    bias = 0.3 * torch.randn(cout, generator=g)
    res = torch.randn(B, 32, D, h, w, generator=g) if resid else None
    xd, wd = x.double(), wt.double()
    want = F.conv3d(xd, wd, None, 1, 1) * scale.double().view(1, -1, 1, 1, 1) + bias.double().view(1, -1, 1, 1, 1)
    mag = F.conv3d(xd.abs(), wd.abs(), None, 1, 1) * scale.double().view(1, -1, 1, 1, 1)
    if relu:
        want = torch.relu(want)
    if res is not None:
        want = want + res.double()
    got = _conv_f32x3(cuda, x, wt, scale, bias, res, relu, cout).double()
    if cout == 1:
        want, mag = want[:, 0], mag[:, 0]
    err = (got - want).abs() - (2e-5 * mag + 1e-6)
    assert float(err.max()) <= 0, float((got - want).abs().max())
    # and as close to the float64 conv as the f32-MFMA layer is, within 4x
    ref32 = _conv_f32(cuda, x, wt, scale, bias, res, relu, cout).double()
    e3 = float((got - want).norm() / want.norm())
    e32 = float((ref32 - want).norm() / want.norm())
    assert e3 <= 4 * e32 + 1e-7, (e3, e32)


@pytest.mark.parametrize("peak,rerun", [(6.0e4, False), (7.0e4, True), (float("inf"), True)])
def test_conv_layer_f32x3_out_of_f16_range(cuda, peak, rerun):
    """An activation beyond the f16 maximum (65504) would make x_hi infinite:
    with a range flag the layer detects it and re-runs as sfm_conv3_f32 in the
    same call, so the output is exactly the fp32 layer's (finite where the
    fp32 layer is); within range the flag stays clear and the split result
    stands (the reference's fp32 Conv3d has no such limit)."""
    g = torch.Generator().manual_seed(77)
    B, cin, D, h, w, cout = 1, 32, 4, 9, 70, 32
    x = torch.randn(B, cin, D, h, w, generator=g)
    x[0, 3, 1, 4, 17] = peak
    x[0, 9, 2, 0, 0] = -abs(peak) if peak != float("inf") else 5.0e4
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
    scale = 0.5 + torch.rand(cout, generator=g)
    bias = 0.3 * torch.randn(cout, generator=g)
    flag = torch.full((2,), 7, dtype=torch.int32, device=cuda)     # two words: out of range, largest activation
    got = _conv_f32x3(cuda, x, wt, scale, bias, None, True, cout, flag=flag)
    ref32 = _conv_f32(cuda, x, wt, scale, bias, None, True, cout)
    assert int(flag[0].item()) == (1 if rerun else 0)
    if rerun:
        assert torch.equal(torch.isnan(got), torch.isnan(ref32))
        m = ~torch.isnan(ref32)
        assert torch.equal(got[m], ref32[m])
    else:
        unguarded = _conv_f32x3(cuda, x, wt, scale, bias, None, True, cout)
        assert torch.equal(got, unguarded) and bool(torch.isfinite(got).all())
        mag = F.conv3d(x.abs().double(), wt.abs().double(), None, 1, 1) * scale.double().view(1, -1, 1, 1, 1)
        err = (got.double() - ref32.double()).abs() - (4e-5 * mag + 1e-6)
        assert float(err.max()) <= 0, float((got - ref32).abs().max())


def test_stack_fp32x3_survives_large_activations(cuda):
    """The fp32x3 stack on a cost volume scaled past the f16 range equals the
    fp32 stack wherever a layer re-ran (here every layer: the activations
    stay ~1e5) -- no inf / NaN from the split."""
    m = _module(5, 64)
    cost = torch.randn(1, 64, 8, 10, 24, generator=torch.Generator().manual_seed(3)) * 2.0e5
    md = m.to(cuda)
    got = md(cost.to(cuda), precision="fp32x3")
    want = md(cost.to(cuda), precision="fp32")
    assert bool(torch.isfinite(got).all())
    r = float((got - want).norm() / want.norm())
    assert r <= 2e-5, r                      # test_stack_f32x3_vs_oracle's bar


@pytest.mark.parametrize("B,cin,L,h,w", [(1, 64, 16, 12, 20), (1, 32, 7, 5, 67)])
def test_stack_f32x3_vs_oracle(cuda, B, cin, L, h, w):
    """12 fp32x3 layers vs the fp32 oracle stack: relative L2 <= 2e-5 (the
    fp32 path's 1e-5 plus the split's ~2^-21 per product)."""
    m = _module(11 + L, cin)
    cost = torch.randn(B, cin, L, h, w, generator=torch.Generator().manual_seed(L))
    got = m.to(cuda)(cost.to(cuda), precision="fp32x3").cpu()
    m = m.cpu()
    want = R.regularize_fp32(m, cost)
    r = float((got - want).norm() / want.norm())
    assert got.shape == want.shape and r <= 2e-5, r


def test_psnet_fp32x3_depth_vs_float64_reference(cuda, golden):
    """psnet_depth with the split-f16 fp32 regularisation (sweep ->
    sfm_conv3_f32x3 x 12 -> head) vs the float64 reference depth: the fp32
    path's bars -- median <= 1e-5 and max <= 1e-4 relative, and within 20x of
    the reference's own float32 error at both statistics."""
    from sfm_amd.regularize import psnet_depth
    g, m = _psnet64(golden)
    inp = g["input"]
    L, md = int(inp["nlabel"]), float(inp["min_depth"])
    hw = tuple(int(x) for x in inp["image_hw"])
    d = lambda k: torch.from_numpy(k).to(cuda)
    got = psnet_depth(d(inp["ref_fea"]), d(inp["tgt_fea"]), d(inp["pose_rescaled"])[:, 0], d(inp["K"]),
                      d(inp["Kinv"]), m.to(cuda), L, md, out_hw=hw, precision="fp32x3").cpu()
    want = torch.from_numpy(g["out64"]["depth"])
    ref32 = _rel(torch.from_numpy(g["out32"]["depth"]), want)
    r = _rel(got, want)
    msg = dict(ours_median=float(r.median()), ours_max=float(r.max()), ref32_median=float(ref32.median()),
               ref32_max=float(ref32.max()))
    print(msg)
    assert float(r.median()) <= 1e-5 and float(r.max()) <= 1e-4, msg
    assert float(r.median()) <= 20 * float(ref32.median()) and float(r.max()) <= 20 * float(ref32.max()), msg


@pytest.mark.parametrize("shape", [(2, 64, 5, 7, 13), (1, 32, 4, 6, 9)])
def test_channels_last_f32_exact(cuda, shape):
    from sfm_amd import _lib
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(2)) * 10
    B, C = shape[:2]
    P = x[0, 0].numel()
    for src in (x, x.to(torch.bfloat16)):
        xd = src.to(cuda).contiguous()
        out = torch.empty(B, P, C, dtype=torch.float32, device=cuda)
        with torch.cuda.device(cuda):
            _lib.check(_lib.load().sfm_to_channels_last_f32(_lib.ptr(xd), 0 if src.dtype == torch.float32 else 1, B, C,
                                                            P, _lib.ptr(out), _lib.stream_ptr(cuda)), "cl")
        want = src.float().reshape(B, C, P).permute(0, 2, 1)
        assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("B,cin,L,h,w", [(1, 64, 16, 12, 20), (1, 32, 7, 5, 67)])
def test_stack_f32_vs_oracle(cuda, B, cin, L, h, w):
    """12 fp32 layers vs the fp32 oracle stack: relative L2 <= 1e-5 (summation
    order only; the bf16 path's bar is 3e-2)."""
    m = _module(11 + L, cin)
    cost = torch.randn(B, cin, L, h, w, generator=torch.Generator().manual_seed(L))
    got = m.to(cuda)(cost.to(cuda), precision="fp32").cpu()
    m = m.cpu()
    want = R.regularize_fp32(m, cost)
    r = float((got - want).norm() / want.norm())
    assert got.shape == want.shape and r <= 1e-5, r


def test_psnet_golden_end_to_end_fp32(cuda, golden):
    """North_star's depth bar on the whole PSNet depth path: psnet_depth with
    the fp32 regularisation (sweep -> sfm_conv3_f32 x 12 -> head) from the
    reference's features and rescaled pose vs the reference's own fp32 depth
    map (psnet.npz).
    * from the reference's own cost volume (regularisation + head only):
      logits within 1e-5 (relative L2), depth median <= 1e-5, max <= 1e-3;
    * from the features (our sweep too): median <= 1e-4 (north_star's bar).
      The sweep is bit-identical to the oracle restatement (oracle/sweep.py),
      which differs from the reference's grid_sample in the last bit of ~5 %
      of the warped entries (its own summation order; the fixture's random-init
      features reach 7e5).  This random-init PSNet amplifies such 1-ulp input
      changes to > 1e-3 of the depth at ~12 % of the pixels (max ~5.5 %): the
      CPU reference chain itself, fed the oracle's cost instead of its own,
      moves just as much (asserted below), while the GPU path fed the same
      cost as the CPU chain agrees with it to <= 1e-3 everywhere."""
    from sfm_amd.depth import depth_head
    from sfm_amd.regularize import psnet_depth
    from sfm_amd.sweep import plane_sweep_cost, quarter_intrinsics
    g, m = _psnet_golden(golden)
    inp, out = g["input"], g["out"]
    L = int(inp["nlabel"])
    hw = tuple(inp["ref_img"].shape[2:])
    md = float(inp["min_depth"])
    d = lambda k: torch.from_numpy(k).to(cuda)
    want = torch.from_numpy(out["depth_init"])
    rel = lambda a, b: ((a - b).abs() / b.abs()).flatten()
    # 1. regularisation + head on the reference's cost volume
    logits = m.to(cuda)(d(out["cost"]), precision="fp32")
    cls = torch.from_numpy(out["classify"])
    rl = float((logits.cpu() - cls).norm() / cls.norm())
    r1 = rel(depth_head(logits, L, md, out_hw=hw).cpu(), want)
    msg1 = (rl, float(r1.median()), float(r1.max()))
    assert rl <= 1e-5 and float(r1.median()) <= 1e-5 and float(r1.max()) <= 1e-3, msg1
    # 2. the whole path from the features
    got = psnet_depth(d(out["ref_fea"]), d(out["tgt_fea"]), d(inp["pose_rescaled"])[:, 0], d(inp["K"]),
                      d(inp["Kinv"]), m.to(cuda), L, md, out_hw=hw, precision="fp32").cpu()
    r2 = rel(got, want)
    assert float(r2.median()) <= 1e-4, (float(r2.median()), float(r2.max()))
    # 3. the same cost on both sides: our sweep's volume (== the oracle's) through the CPU reference chain
    K4, Ki4 = quarter_intrinsics(d(inp["K"]), d(inp["Kinv"]))
    cost = plane_sweep_cost(d(out["ref_fea"]), d(out["tgt_fea"]), d(inp["pose_rescaled"])[:, 0], K4, Ki4, L, md)
    m = m.cpu()
    want_same = S.depth_head(R.regularize_fp32(m, cost.cpu()), L, md, out_hw=hw)
    r3 = rel(got, want_same)
    assert float(r3.median()) <= 1e-5 and float(r3.max()) <= 1e-3, (float(r3.median()), float(r3.max()))
    # the fixture's own sensitivity: the CPU chain from the two costs (1-ulp apart) differs as much as r2
    r4 = rel(want_same, want)
    assert float((r4 > 1e-3).float().mean()) >= 0.5 * float((r2 > 1e-3).float().mean())


# ---------------------------------------------------------------------------
# The depth bar against the exact answer (psnet64.npz, oracle/gen_golden.py
# gen_psnet64): the reference PSNet run in float64 and in float32 on the same
# float32 unit-scale features and float32 weights, with every sweep sample
# kept 1e-5 clear of the border step (tests/test_oracle_golden.py).  The
# reference's own float32 depth is median 6.1e-7 / max 7.8e-6 from the
# float64 one.

def _psnet64(golden):
    from sfm_amd.regularize import CostRegularization
    g = golden("psnet64.npz")
    m = CostRegularization(64)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["state"].items()})
    return g, m.eval()


def _rel(a, b):
    return ((a.double() - b.double()).abs() / b.double().abs()).flatten()


def test_psnet_fp32_depth_vs_float64_reference(cuda, golden):
    """psnet_depth (sweep -> sfm_conv3_f32 x 12 -> head) vs the float64
    reference depth: median <= 1e-5 and max <= 1e-4 relative (north_star's
    1e-4 bar as a maximum), and within 20x of the reference's own float32
    error at both statistics."""
    from sfm_amd.regularize import psnet_depth
    g, m = _psnet64(golden)
    inp = g["input"]
    L, md = int(inp["nlabel"]), float(inp["min_depth"])
    hw = tuple(int(x) for x in inp["image_hw"])
    d = lambda k: torch.from_numpy(k).to(cuda)
    got = psnet_depth(d(inp["ref_fea"]), d(inp["tgt_fea"]), d(inp["pose_rescaled"])[:, 0], d(inp["K"]),
                      d(inp["Kinv"]), m.to(cuda), L, md, out_hw=hw, precision="fp32").cpu()
    want = torch.from_numpy(g["out64"]["depth"])
    ref32 = _rel(torch.from_numpy(g["out32"]["depth"]), want)
    r = _rel(got, want)
    msg = dict(ours_median=float(r.median()), ours_max=float(r.max()), ref32_median=float(ref32.median()),
               ref32_max=float(ref32.max()))
    print(msg)
    assert float(r.median()) <= 1e-5 and float(r.max()) <= 1e-4, msg
    assert float(r.median()) <= 20 * float(ref32.median()) and float(r.max()) <= 20 * float(ref32.max()), msg


def test_default_psnet_module_vs_float64_reference(cuda, golden):
    """The PSNet module SFMnet(nlabel) builds by default (fp32 regularisation)
    on the fixture's features: both outputs vs the float64 reference, the
    same bars; the bf16 opt-in is measured beside it (it cannot meet them)."""
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    g, _ = _psnet64(golden)
    inp = g["input"]
    L, md = int(inp["nlabel"]), float(inp["min_depth"])
    H, W = (int(x) for x in inp["image_hw"])
    c = defaults()
    c.update(PSNET_CONTEXT=False, RESCALE_DEPTH=True, NORM_TARGET=0.8)
    feas = [torch.from_numpy(inp["ref_fea"]).to(cuda), torch.from_numpy(inp["tgt_fea"]).to(cuda)]
    calls = []

    def feature_fn(img):
        calls.append(img.shape)
        return feas[(len(calls) - 1) % 2]
    net = PSNet(L, md, cfg=c, feature_fn=feature_fn).to(cuda).eval()
    assert net.conv_precision == "fp32x3"
    net.load_state_dict({k: torch.from_numpy(v) for k, v in g["state"].items()}, strict=False)
    img = torch.zeros(1, 3, H, W, device=cuda)
    d = lambda k: torch.from_numpy(k).to(cuda)
    want = torch.from_numpy(g["out64"]["depth"])
    with torch.no_grad():
        d_init, dep = net(img, [img], d(inp["pose"]).clone(), d(inp["K"]), d(inp["Kinv"]))
        r0, r1 = _rel(d_init.cpu(), torch.from_numpy(g["out64"]["depth_init"])), _rel(dep.cpu(), want)
        assert float(r0.median()) <= 1e-5 and float(r0.max()) <= 1e-4, (float(r0.median()), float(r0.max()))
        assert float(r1.median()) <= 1e-5 and float(r1.max()) <= 1e-4, (float(r1.median()), float(r1.max()))
        net.conv_precision = "bf16"
        calls.clear()
        _, d16 = net(img, [img], d(inp["pose"]).clone(), d(inp["K"]), d(inp["Kinv"]))
    r16 = _rel(d16.cpu(), want)
    print(dict(fp32_max=float(r1.max()), bf16_median=float(r16.median()), bf16_max=float(r16.max())))
    assert float(r16.max()) > float(r1.max())


# ---------------------------------------------------------------------------
# float16 stack (sfm_conv3_f16): the precision of the reference's Conv3d
# layers under cfg.MIXED_PREC autocast (SFMnet.py:164, cfgs/kitti.yml:10).
# Same kernels as bf16, f16 MFMA and conversions: one layer within half an
# f16 ulp (2^-11 relative) of the fp32 conv of the same f16 operands; the
# rolling and per-plane kernels bit-identical; the stack close to the
# f16-storage oracle and to fp32; the depth against the float64 reference.

def _f16_ulp_close(got, want):
    tol = 2.0 ** -11 * want.abs() * 1.001 + 1e-5
    bad = (got - want).abs() > tol
    return int(bad.sum()), float((got - want).abs().max())


@pytest.mark.parametrize("shape", [(2, 64, 5, 7, 13), (1, 64, 2, 16, 16)])
def test_channels_last_f16_exact(cuda, shape):
    from sfm_amd.regularize import to_channels_last
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(2)) * 10
    got = to_channels_last(x.to(cuda), torch.float16).cpu()
    want = x.permute(0, 2, 3, 4, 1).to(torch.float16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # a bf16 volume (the C3 sweep's) -> f16: every bf16 value in f16 range converts exactly
    xb = x.to(torch.bfloat16)
    got2 = to_channels_last(xb.to(cuda), torch.float16).cpu()
    want2 = xb.float().permute(0, 2, 3, 4, 1).to(torch.float16)
    assert torch.equal(got2.view(torch.int16), want2.view(torch.int16))


@pytest.mark.parametrize("B,cin,D,h,w,relu,resid,cout", [
    (1, 32, 3, 4, 64, False, False, 32),
    (2, 64, 5, 7, 70, True, False, 32),
    (1, 32, 4, 9, 131, False, True, 32),
    (1, 32, 6, 5, 33, False, False, 1),
])
def test_conv_layer_f16(cuda, B, cin, D, h, w, relu, resid, cout):
    from sfm_amd.regularize import conv3_f16
    g = torch.Generator().manual_seed(B * 100 + cin + D + h + w + 1)
    x = torch.randn(B, cin, D, h, w, generator=g).to(torch.float16).float()
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1).to(torch.float16).float()
    scale = 0.5 + torch.rand(cout, generator=g)
    bias = 0.3 * torch.randn(cout, generator=g)
    res = torch.randn(B, 32, D, h, w, generator=g).to(torch.float16).float() if resid else None
    want = F.conv3d(x.double(), wt.double(), None, 1, 1) * scale.double().view(1, -1, 1, 1, 1) \
        + bias.double().view(1, -1, 1, 1, 1)
    if relu:
        want = torch.relu(want)
    if res is not None:
        want = want + res.double()
    want = want.float()
    wp = torch.zeros(27, 32, cin)
    wp[:, :cout] = wt.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    sc, bi = torch.ones(32), torch.zeros(32)
    sc[:cout], bi[:cout] = scale, bias
    xcl = x.permute(0, 2, 3, 4, 1).contiguous().to(torch.float16).to(cuda)
    rcl = None if res is None else res.permute(0, 2, 3, 4, 1).contiguous().to(torch.float16).to(cuda)
    got = conv3_f16(xcl, wp.to(torch.float16).to(cuda), sc, bi, rcl, relu, cout).cpu()
    if cout == 32:
        nbad, mx = _f16_ulp_close(got.float().permute(0, 4, 1, 2, 3), want)
        assert nbad == 0, (nbad, mx)
    else:
        err = (got - want[:, 0]).abs() - (1e-5 * want[:, 0].abs() + 1e-5)
        assert float(err.max()) <= 0, float((got - want[:, 0]).abs().max())


def test_rolling_kernel_equals_per_plane_kernel_f16(cuda):
    from sfm_amd import _lib
    from sfm_amd.regularize import conv3_f16
    g = torch.Generator().manual_seed(9)
    D, h, w = 13, 9, 70
    x = torch.randn(1, D, h, w, 32, generator=g).to(torch.float16).to(cuda)
    wp = (torch.randn(27, 32, 32, generator=g) * 0.1).to(torch.float16).to(cuda)
    sc, bi = 0.5 + torch.rand(32, generator=g), 0.1 * torch.randn(32, generator=g)
    res = torch.randn(1, D, h, w, 32, generator=g).to(torch.float16).to(cuda)
    outs = []
    try:
        for rolling in (0, 1):
            _lib.tune("conv_rolling", rolling)
            outs.append((conv3_f16(x, wp, sc, bi, res, False, 32).cpu(), conv3_f16(x, wp, sc, bi, None, True, 1).cpu()))
    finally:
        _lib.tune("conv_rolling", 1)
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("B,cin,L,h,w", [(1, 64, 16, 12, 20), (1, 32, 7, 5, 67)])
def test_stack_f16_vs_oracle(cuda, B, cin, L, h, w):
    """Relative L2 against the f16-storage oracle <= 3e-3 and against fp32 <=
    5e-3 (bf16's bars are 2e-2 / 3e-2: three more mantissa bits)."""
    m = _module(11 + L, cin)
    cost = torch.randn(B, cin, L, h, w, generator=torch.Generator().manual_seed(L))
    got = m.to(cuda)(cost.to(cuda), precision="fp16").cpu()
    m = m.cpu()
    want16 = R.regularize_f16(m, cost)
    want32 = R.regularize_fp32(m, cost)
    r16 = float((got - want16).norm() / want16.norm())
    r32 = float((got - want32).norm() / want32.norm())
    print(dict(r16=r16, r32=r32))
    assert r16 <= 3e-3, r16
    assert r32 <= 5e-3, r32


def test_psnet_fp16_depth_vs_float64_reference(cuda, golden):
    """The fp16 stack (what cfg.MIXED_PREC selects) against the float64
    reference PSNet depth (psnet64.npz): median <= 2e-3, max <= 2e-2
    relative (measured 1.2e-3 / 9.9e-3; an 11-bit mantissa cannot meet the
    fp32 path's 1e-4, and neither can the reference's own fp16 autocast), and
    five times closer than the bf16 stack at the median (measured 12x:
    bf16 1.4e-2 / 0.11)."""
    from sfm_amd.regularize import psnet_depth
    g, m = _psnet64(golden)
    inp = g["input"]
    L, md = int(inp["nlabel"]), float(inp["min_depth"])
    hw = tuple(int(x) for x in inp["image_hw"])
    d = lambda k: torch.from_numpy(k).to(cuda)
    want = torch.from_numpy(g["out64"]["depth"])
    res = {}
    for prec in ("fp16", "bf16"):
        got = psnet_depth(d(inp["ref_fea"]), d(inp["tgt_fea"]), d(inp["pose_rescaled"])[:, 0], d(inp["K"]),
                          d(inp["Kinv"]), m.to(cuda), L, md, out_hw=hw, precision=prec).cpu()
        r = _rel(got, want)
        res[prec] = (float(r.median()), float(r.max()))
    print(res)
    assert res["fp16"][0] <= 2e-3 and res["fp16"][1] <= 2e-2, res
    assert res["fp16"][0] * 5 <= res["bf16"][0], res
