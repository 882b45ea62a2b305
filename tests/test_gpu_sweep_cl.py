"""The channels-last plane sweep (sfm_plane_sweep_cl,
sfm_amd.sweep.plane_sweep_cost_channels_last) and the depth stage's route
through it.

The fused sweep writes [B, L, h, w, 2C] in the regulariser's activation type.
Its contract is bit-equality with the two-step path it replaces -- the planar
float32 sweep followed by sfm_to_channels_last_{f16,bf16,f32} -- so every
comparison here is torch.equal on an integer view, except the one against
the oracle, which is independent of the planar kernel and holds the bar
tests/test_gpu_sweep.py uses against the oracle (1e-4 |want| + 2e-6 on the
warped half, exact on the reference half).

Shapes (features synth.features N(0,1), poses synth.relative_pose):
  (47, 156) L=16 C=32 B=1   several waves, a partial last wave
  (94, 311) L=3  C=32 B=2   hw % 4 == 2 with L odd: the planar sweep's
                            unaligned fallback; pair index > 0
  (5, 7)    L=2  C=32       hw < 64: waves straddle planes, the last record
                            is the boundary
  (33, 65)  L=5  C=8        one 16-byte chunk per half (16-bit types)
  (16, 24)  L=4  C=12 B=2   C % 8 != 0: the element-wise kernel
  (9, 13)   L=3  C=6  B=2   C % 4 != 0: the element-wise kernel on a padded quad
"""
import pytest
import torch

from oracle import sweep as S

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
#        h,  w,   L,  C,  B
CASES = [(47, 156, 16, 32, 1),
         (94, 311, 3, 32, 2),
         (5, 7, 2, 32, 1),
         (33, 65, 5, 8, 1),
         (16, 24, 4, 12, 2)]
_IVIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(_IVIEW[a.dtype]), b.view(_IVIEW[b.dtype]))


def _inputs(case, t_scale=1.0):
    """CPU inputs of a case: ref, tgt, pose, full-resolution K, K^-1."""
    from sfm_amd import synth
    h, w, L, C, B = case
    ref, tgt = synth.features(B, C, h, w, seed=11 + h)
    K = synth.intrinsics(B, 4.0 * w, 4.0 * w, 2.0 * w, 2.0 * h)
    pose = synth.relative_pose(B, torch.Generator().manual_seed(3 + w))
    if t_scale != 1.0:
        pose = pose.clone()
        pose[:, :, 3] *= t_scale
    return ref, tgt, pose, K, torch.inverse(K)


def _args(case, cuda, t_scale=1.0, min_depth=1.0):
    from sfm_amd.sweep import quarter_intrinsics
    ref, tgt, pose, K, Ki = _inputs(case, t_scale)
    K4, Ki4 = quarter_intrinsics(K, Ki)
    return (ref.to(cuda), tgt.to(cuda), pose.to(cuda), K4.to(cuda), Ki4.to(cuda), case[2], min_depth)


_planar = {}


def _planar_cost(case, cuda, t_scale=1.0, min_depth=1.0, pbd=False):
    """The planar float32 volume of a case: computed once, shared, never modified."""
    from sfm_amd.sweep import plane_sweep_cost
    key = (case, t_scale, min_depth, pbd)
    if key not in _planar:
        _planar[key] = plane_sweep_cost(*_args(case, cuda, t_scale, min_depth), dtype=torch.float32,
                                        predict_by_depth=pbd)
    return _planar[key]


def _two_step(case, cuda, dtype, **kw):
    from sfm_amd.regularize import to_channels_last
    return to_channels_last(_planar_cost(case, cuda, **kw), dtype)     # float32: sfm_to_channels_last_f32


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=["47x156", "94x311", "5x7", "33x65c8", "16x24c12"])
def test_bit_equal_to_sweep_then_transpose(cuda, case, dtype):
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    h, w, L, C, B = case
    got = plane_sweep_cost_channels_last(*_args(case, cuda), dtype=dtype)
    from sfm_amd import _lib
    # the fast path takes whole 16-byte chunks per record half: C % 4 (float32) or C % 8 (16-bit)
    assert _lib.last_sweep() == ("k_sweep_cl" if C % (4 if dtype == torch.float32 else 8) == 0 else "k_sweep_cl_any")
    assert tuple(got.shape) == (B, L, h, w, 2 * C) and got.dtype == dtype and got.is_contiguous()
    assert _bits_equal(got, _two_step(case, cuda, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_element_wise_kernel_with_a_padded_quad(cuda, dtype):
    """C = 6: no fast path for any type, and the last channel quad of the
    target relayout is half padding.  2C = 12 is below the 16-bit transposes'
    channel multiple, so those types are compared with torch's round-to-
    nearest-even conversion of the planar volume (the transposes' function)."""
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    case = (9, 13, 3, 6, 2)
    got = plane_sweep_cost_channels_last(*_args(case, cuda), dtype=dtype)
    from sfm_amd import _lib
    assert _lib.last_sweep() == "k_sweep_cl_any"
    planar = _planar_cost(case, cuda)
    assert bool((planar[:, 6:] != 0).any())
    if dtype == torch.float32:
        want = _two_step(case, cuda, dtype)
    else:
        want = planar.permute(0, 2, 3, 4, 1).contiguous().to(dtype)
    assert _bits_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("pbd", [False, True], ids=["inverse_depth", "by_depth"])
def test_predict_by_depth(cuda, dtype, pbd):
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    case = CASES[0]
    got = plane_sweep_cost_channels_last(*_args(case, cuda), dtype=dtype, predict_by_depth=pbd)
    assert _bits_equal(got, _two_step(case, cuda, dtype, pbd=pbd))
    if pbd:     # the two plane spacings are different volumes
        assert not _bits_equal(got, _two_step(case, cuda, dtype, pbd=False))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_samples_leaving_the_image(cuda, dtype):
    """Translation x 20 (about 22 along the optical axis; the planes reach 16 x
    16 so that the nearer ones still see the target): most samples fall outside
    the image (zero for every channel, ~0.8 of them by the oracle) and every
    plane that stays crosses its border."""
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    case = CASES[0]
    C = case[3]
    far = dict(t_scale=20.0, min_depth=16.0)
    warped = _planar_cost(case, cuda, **far)[:, C:]
    outside = (warped == 0).all(dim=1)            # [B, L, h, w]: every channel zero
    print("share of samples outside the image:", float(outside.float().mean()))
    assert bool(outside.any()) and bool((warped != 0).any())     # zero and non-zero warped samples: not vacuous
    got = plane_sweep_cost_channels_last(*_args(case, cuda, **far), dtype=dtype)
    assert _bits_equal(got, _two_step(case, cuda, dtype, **far))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_caller_supplied_out_and_workspace(cuda, dtype):
    """out and workspace one element larger than needed, sliced: the element
    past the end of each is untouched."""
    from sfm_amd.sweep import plane_sweep_cost_channels_last, workspace_for
    case = CASES[0]
    h, w, L, C, B = case
    shape = (B, L, h, w, 2 * C)
    n = B * L * h * w * 2 * C
    flat = torch.full((n + 1,), 7.0, dtype=dtype, device=cuda)
    out = flat[:n].view(shape)
    nws = workspace_for(B, C, h, w, cuda).numel()
    wflat = torch.full((nws + 1,), 0xA5, dtype=torch.uint8, device=cuda)
    got = plane_sweep_cost_channels_last(*_args(case, cuda), dtype=dtype, out=out, workspace=wflat[:nws])
    assert got.data_ptr() == flat.data_ptr()
    assert _bits_equal(got, _two_step(case, cuda, dtype))
    assert float(flat[n]) == 7.0 and int(wflat[nws]) == 0xA5


def test_against_the_oracle(cuda):
    """fp32, independent of the planar kernel: the reference half exactly, the
    warped half within test_gpu_sweep.py's oracle bar."""
    from sfm_amd.sweep import plane_sweep_cost_channels_last
    case = CASES[0]
    h, w, L, C, B = case
    ref, tgt, pose, K, Ki = _inputs(case)
    want = S.plane_sweep_cost(ref, tgt, pose, K, Ki, L, 1.0).permute(0, 2, 3, 4, 1).contiguous()
    got = plane_sweep_cost_channels_last(*_args(case, cuda), dtype=torch.float32).cpu()
    assert torch.equal(got[..., :C], want[..., :C])
    err = (got[..., C:] - want[..., C:]).abs()
    print("max |got - oracle| on the warped half:", float(err.max()))
    assert float((err - (1e-4 * want[..., C:].abs() + 2e-6)).max()) <= 0.0, float(err.max())
    assert bool((want[..., C:] != 0).any())


# --- regulariser and routing ------------------------------------------------
RB, RC, RL, RH, RW = 1, 32, 8, 16, 24


def _module(seed):
    from tests.test_regularize import _module as m
    return m(seed, 2 * RC)


@pytest.mark.parametrize("precision", ["fp16", "fp32x3"])
def test_forward_channels_last_is_forward(cuda, precision):
    from sfm_amd.regularize import _ACT_DTYPE, to_channels_last
    m = _module(5).to(cuda)
    cost = torch.randn(RB, 2 * RC, RL, RH, RW, generator=torch.Generator().manual_seed(6)).to(cuda)
    want = m(cost, precision=precision)
    x = to_channels_last(cost, _ACT_DTYPE[precision])
    got = m.forward_channels_last(x, precision=precision)
    assert tuple(got.shape) == (RB, 1, RL, RH, RW)
    assert _bits_equal(got, want)
    with pytest.raises(RuntimeError):                       # wrong dtype for the precision
        m.forward_channels_last(x, precision="bf16")
    with pytest.raises(RuntimeError):                       # wrong channel count
        m.forward_channels_last(x[..., :32].contiguous(), precision=precision)
    with pytest.raises(RuntimeError):                       # not contiguous
        m.forward_channels_last(x.transpose(2, 3), precision=precision)


def _launches(fn):
    """fn() under the library's profiler: (result, launches per kernel name)."""
    from sfm_amd import _lib
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, {k: _lib.profile_read(k)[1] for k in ("plane_sweep_cl", "plane_sweep", "to_channels_last")}


def _both_routes(fn):
    """fn() with the switch at 1 and at 0; the switch is left at its default."""
    from sfm_amd import _lib
    assert _lib.tune_get("sweep_fused_cl") == 1
    try:
        fused, n1 = _launches(fn)
        _lib.tune("sweep_fused_cl", 0)
        plain, n0 = _launches(fn)
    finally:
        _lib.tune("sweep_fused_cl", 1)
    return fused, n1, plain, n0


def _depth_inputs(cuda):
    from sfm_amd import synth
    ref, tgt = synth.features(RB, RC, RH, RW, seed=3)
    K = synth.intrinsics(RB, 4.0 * RW, 4.0 * RW, 2.0 * RW, 2.0 * RH)
    pose = synth.relative_pose(RB, torch.Generator().manual_seed(3))
    return [t.to(cuda) for t in (ref, tgt, pose, K, torch.inverse(K))]


@pytest.mark.parametrize("precision", ["fp16", "fp32x3", None])
def test_psnet_depth_routes(cuda, precision):
    from sfm_amd.regularize import psnet_depth
    ref, tgt, pose, K, Ki = _depth_inputs(cuda)
    m = _module(7).to(cuda)
    fused, n1, plain, n0 = _both_routes(
        lambda: psnet_depth(ref, tgt, pose, K, Ki, m, RL, 1.0, precision=precision))
    assert torch.equal(fused, plain)
    assert n1["plane_sweep_cl"] >= 1 and n1["to_channels_last"] == 0 and n1["plane_sweep"] == 0, n1
    assert n0["plane_sweep_cl"] == 0 and n0["to_channels_last"] >= 1 and n0["plane_sweep"] >= 1, n0


def test_hooked_or_overriding_regulariser_is_called_as_before(cuda):
    """psnet_depth's fused route skips regularizer(cost); a module with a
    forward hook, or a subclass with its own forward, keeps the call."""
    from sfm_amd.regularize import CostRegularization, psnet_depth
    ref, tgt, pose, K, Ki = _depth_inputs(cuda)
    m = _module(7).to(cuda)
    want = psnet_depth(ref, tgt, pose, K, Ki, m, RL, 1.0, precision="fp16")
    seen = []
    handle = m.register_forward_hook(lambda mod, a, out: seen.append(tuple(a[0].shape)))
    try:
        got, n = _launches(lambda: psnet_depth(ref, tgt, pose, K, Ki, m, RL, 1.0, precision="fp16"))
    finally:
        handle.remove()
    assert seen == [(RB, 2 * RC, RL, RH, RW)] and n["plane_sweep_cl"] == 0 and n["to_channels_last"] >= 1, (seen, n)
    assert torch.equal(got, want)

    class Doubled(CostRegularization):
        def forward(self, cost, precision="fp32x3"):
            return 2.0 * super().forward(cost, precision=precision)
    d = Doubled(2 * RC).to(cuda).eval()
    d.load_state_dict(m.state_dict())
    got, n = _launches(lambda: psnet_depth(ref, tgt, pose, K, Ki, d, RL, 1.0, precision="fp16"))
    assert n["plane_sweep_cl"] == 0 and n["plane_sweep"] >= 1, n


def test_default_psnet_routes(cuda):
    """PSNet with its default cost_dtype and conv_precision (seeded weights,
    injected features; the 2-D context CNN, which the route does not touch, off)."""
    from sfm_amd.config import defaults
    from sfm_amd.psnet import PSNet
    ref, tgt, pose, K, Ki = _depth_inputs(cuda)
    c = defaults()
    c.update(PSNET_CONTEXT=False)
    feas = [ref, tgt]
    calls = []

    def feature_fn(img):
        calls.append(1)
        return feas[(len(calls) - 1) % 2]
    torch.manual_seed(9)
    net = PSNet(RL, 1.0, cfg=c, feature_fn=feature_fn).to(cuda).eval()
    assert net.cost_dtype == torch.float32 and net.conv_precision == "fp32x3"
    img = torch.zeros(RB, 3, 4 * RH, 4 * RW, device=cuda)

    def run():
        with torch.no_grad():
            return net(img, [img], pose.unsqueeze(1).clone(), K, Ki)
    fused, n1, plain, n0 = _both_routes(run)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])
    assert n1["plane_sweep_cl"] >= 1 and n1["to_channels_last"] == 0, n1
    assert n0["plane_sweep_cl"] == 0 and n0["to_channels_last"] >= 1, n0


def test_bf16_volume_keeps_the_two_step_route(cuda):
    from sfm_amd.regularize import psnet_depth
    ref, tgt, pose, K, Ki = _depth_inputs(cuda)
    m = _module(7).to(cuda)
    a, n1, b, n0 = _both_routes(
        lambda: psnet_depth(ref, tgt, pose, K, Ki, m, RL, 1.0, cost_dtype=torch.bfloat16, precision="fp16"))
    assert torch.equal(a, b)
    for n in (n1, n0):
        assert n["plane_sweep_cl"] == 0 and n["plane_sweep"] >= 1 and n["to_channels_last"] >= 1, n


def test_errors(cuda):
    from sfm_amd.sweep import plane_sweep_cost_channels_last as f
    case = CASES[2]
    h, w, L, C, B = case
    a = _args(case, cuda)
    shape = (B, L, h, w, 2 * C)
    with pytest.raises(RuntimeError):
        f(*a, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        f(a[0][:, :, :-1], *a[1:])
    with pytest.raises(RuntimeError):
        f(*a, dtype=torch.float16, out=torch.empty((B, 2 * C, L, h, w), dtype=torch.float16, device=cuda))
    with pytest.raises(RuntimeError):
        f(*a, dtype=torch.float16, out=torch.empty(shape, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(RuntimeError):
        f(*a, dtype=torch.float16,
          out=torch.empty((B, L, w, h, 2 * C), dtype=torch.float16, device=cuda).transpose(2, 3))
    tgt = a[1].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        f(a[0], tgt, *a[2:])
    with torch.no_grad():
        f(a[0], tgt, *a[2:])          # refused only while grad is enabled
