"""The float16 backward of the per-plane context stack on the GPU, kernel by
kernel (csrc/context_bwd.hip): sfm_conv2_wgrad_f16, sfm_conv2_dgrad_f16 with
its ReLU mask, sfm_context_unpack_grad_f16.

Exact integers must come back bit for bit; general float16 values are held to
the project's rule for float16 routes: err = max|g - g64| / max|g64| against
float64 autograd on the CPU on the same float16 operands, at most 2 x the error
of torch's own float16 conv2d backward on the GPU on the same operands,
measured in the same test."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the stock stack's seven (cin_pad, cout, dilation); cout 1 travels zero-padded to 32 channels
STAGES = [(64, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 1, 1)]
# (images, h, w).  k_conv2_wgrad's tile is 4 rows x 64 columns, k_conv2's 8 (or 4) x 64:
SHAPES = [
    (3, 5, 70),    # fewer rows than k_conv2's tile, one past the 4-row tile, crosses the 64-column tile
    (2, 19, 64),   # five row tiles, the last of three rows; exactly one column tile
    (2, 9, 65),    # one column past the tile
    (1, 3, 7),     # smaller than the dilation: at d8 and d16 every off-centre tap is outside
]
CASES = [(s, st) for st in STAGES for s in SHAPES]
IDS = ["x".join(map(str, s)) + f"-{ci}to{co}-d{d}" for s, (ci, co, d) in CASES]


def _pad32(n):
    return (n + 31) // 32 * 32


def _launches(fn, names=("conv2_wgrad", "conv2_dgrad", "context_unpack_grad")):
    from sfm_amd import _lib
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return out, {k: _lib.profile_read(k)[1] for k in names}


def _cl(t, cuda, pad=None):
    """[n, c, h, w] -> channels-last float16 on the device, c zero-padded to ``pad``."""
    t = t.permute(0, 2, 3, 1)
    if pad is not None and pad != t.shape[-1]:
        z = t.new_zeros(tuple(t.shape[:-1]) + (pad,))
        z[..., :t.shape[-1]] = t
        t = z
    return t.half().contiguous().to(cuda)


def _backward64(x, wt, gy, dil):
    x = x.double().clone().requires_grad_(True)
    wt = wt.double().clone().requires_grad_(True)
    F.conv2d(x, wt, padding=dil, dilation=dil).backward(gy.double())
    return x.grad, wt.grad


def _wgrad(x, gy, cout, cin, dil, cuda):
    from sfm_amd.context import conv2_wgrad_f16, unpack_wgrad2
    gwp = conv2_wgrad_f16(_cl(x, cuda), _cl(gy, cuda, _pad32(cout)), dil)
    assert gwp.dtype == torch.float32 and tuple(gwp.shape) == (9, _pad32(cout), cin)
    if cout < _pad32(cout):
        assert bool((gwp[:, cout:] == 0).all())             # the padding's rows: exactly zero
    return unpack_wgrad2(gwp, cout, cin)


def _dgrad(gy, wt, dil, cuda, act=None):
    from sfm_amd.context import conv2_dgrad_f16, pack_dgrad_weights2
    wd = pack_dgrad_weights2(wt.float()).half().to(cuda)
    out = conv2_dgrad_f16(_cl(gy, cuda, wd.shape[2]), wd, dil, None if act is None else _cl(act, cuda))
    return out.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _int_case(shape, stage):
    """Weights in {-1, 0, 1}, activations in {0, 1}, gradients in {-1, 0, 1} and
    the float64 CPU convolution backward on them."""
    n, h, w = shape
    cin, cout, dil = stage
    g = torch.Generator().manual_seed(sum(shape) * 64 + cin + cout + dil)
    x = torch.randint(0, 2, (n, cin, h, w), generator=g).double()
    gy = torch.randint(-1, 2, (n, cout, h, w), generator=g).double()
    wt = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).double()
    gx, gw = _backward64(x, wt, gy, dil)
    assert float(gw.abs().max()) < 2 ** 24 and float(gx.abs().max()) < 2048
    return x, gy, wt, gw, gx * (x > 0)


@pytest.mark.parametrize("shape,stage", CASES, ids=IDS)
def test_exact_integers_bit_for_bit(cuda, shape, stage):
    """Every sum is exact in float32 (weight gradient) and float16 (data
    gradient, |.| <= 9 * 128 < 2048) in any order, so both must equal the
    float64 evaluation -- the weight gradient at 1 and 3 accumulating blocks,
    more blocks than tiles, and the default; the data gradient through the mask
    of the {0, 1} activation."""
    from sfm_amd import _lib
    cin, cout, dil = stage
    x, gy, wt, gw, gx = _int_case(shape, stage)
    n, h, w = shape
    tiles = n * ((h + 3) // 4) * ((w + 63) // 64)
    try:
        for nb in (0, 1, 3, tiles + 5):
            _lib.tune("conv2_wgrad_blocks", nb)
            got = _wgrad(x, gy, cout, cin, dil, cuda)
            assert torch.equal(got.cpu().double(), gw), (nb, float((got.cpu().double() - gw).abs().max()))
    finally:
        _lib.tune("conv2_wgrad_blocks", 0)
    got = _dgrad(gy, wt, dil, cuda, act=x)
    assert got.dtype == torch.float16 and torch.equal(got.cpu().double(), gx)


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


GENERAL = [((2, 19, 64), STAGES[1]), ((2, 9, 65), STAGES[4]), ((3, 5, 70), STAGES[3]), ((3, 5, 70), STAGES[5]),
           ((2, 9, 65), STAGES[6])]


@functools.lru_cache(maxsize=None)
def _general(shape, stage, gscale):
    n, h, w = shape
    cin, cout, dil = stage
    g = torch.Generator().manual_seed(7 * cin + cout + dil + int(gscale < 1))
    x = torch.randn(n, cin, h, w, generator=g).half()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cout)) ** 0.5).half()
    gy = (torch.randn(n, cout, h, w, generator=g) * gscale).half()
    return (x, wt, gy) + _backward64(x, wt, gy, dil)


@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -10], ids=["g1", "g2^-10"])
@pytest.mark.parametrize("shape,stage", GENERAL, ids=["x".join(map(str, s)) + f"-{a}to{b}-d{d}" for s, (a, b, d) in GENERAL])
def test_general_values_against_float64_and_torch(cuda, shape, stage, gscale):
    """N(0, 1) rounded to float16, gradients at scale 1 and 2^-10: ours within
    2 x the error torch's own float16 conv2d backward makes on the same
    operands on the same GPU; two calls give equal bits."""
    cin, cout, dil = stage
    x, wt, gy, gx64, gw64 = _general(shape, stage, gscale)
    xt = x.to(cuda).requires_grad_(True)
    wtt = wt.to(cuda).requires_grad_(True)
    F.conv2d(xt, wtt, padding=dil, dilation=dil).backward(gy.to(cuda))
    ours_w = _wgrad(x, gy, cout, cin, dil, cuda)
    ours_x = _dgrad(gy, wt, dil, cuda)
    rec = {"stage": stage, "shape": shape, "gscale": gscale,
           "wgrad_err_hip": _err(ours_w, gw64), "wgrad_err_torch_f16": _err(wtt.grad, gw64),
           "dgrad_err_hip": _err(ours_x, gx64), "dgrad_err_torch_f16": _err(xt.grad, gx64)}
    print(rec)
    assert rec["wgrad_err_hip"] <= 2.0 * rec["wgrad_err_torch_f16"], rec
    assert rec["dgrad_err_hip"] <= 2.0 * rec["dgrad_err_torch_f16"], rec
    again_w = _wgrad(x, gy, cout, cin, dil, cuda)
    again_x = _dgrad(gy, wt, dil, cuda)
    assert torch.equal(ours_w.view(torch.int32), again_w.view(torch.int32))
    assert torch.equal(ours_x.contiguous().view(torch.int16), again_x.contiguous().view(torch.int16))


def test_mask_is_a_select(cuda):
    """act == 0 gives exactly +0 even where the gradient is infinite, act > 0
    lets the infinity through, act = NULL masks nothing."""
    n, h, w, cin, cout, dil = 1, 6, 9, 64, 32, 2
    g = torch.Generator().manual_seed(3)
    gy = torch.randn(n, cout, h, w, generator=g).half()
    gy[0, :, 3, 4] = float("inf")
    wt = torch.rand(cout, cin, 3, 3, generator=g).half() + 0.5           # positive: inf x w = inf, no NaN
    act = torch.randint(0, 2, (n, cin, h, w), generator=g).half() * 3.0
    masked = _dgrad(gy, wt, dil, cuda, act=act).cpu()
    plain = _dgrad(gy, wt, dil, cuda, act=None).cpu()
    reach = torch.zeros(h, w, dtype=torch.bool)                          # the pixels the infinite gradient reaches
    for ky in (-1, 0, 1):
        for kx in (-1, 0, 1):
            reach[3 + ky * dil, 4 + kx * dil] = True
    assert bool(torch.isposinf(plain[0][:, reach]).all()) and bool(torch.isfinite(plain[0][:, ~reach]).all())
    zero = act == 0
    assert bool(zero.any()) and bool((~zero).any())
    assert bool((masked.contiguous().view(torch.int16)[zero] == 0).all())      # +0: no sign bit, no NaN
    assert torch.equal(masked[~zero].view(torch.int16), plain[~zero].view(torch.int16))
    assert bool(torch.isposinf(masked[0][:, reach][~zero[0][:, reach]]).all())


def _unpack_restated(g0, go, L):
    """Ascending-order fp32 sums written as a loop."""
    B, nl = g0.shape[:2]
    s = torch.zeros_like(g0[:, 0, :, :, :32], dtype=torch.float32)
    for l in range(nl):
        s = s + g0[:, l, :, :, :32].float()
    return s.permute(0, 3, 1, 2).contiguous(), g0[..., 32].float() + go


def test_unpack_matches_the_restatement_for_any_chunking(cuda):
    from sfm_amd.context import context_unpack_grad
    B, L, h, w = 2, 3, 19, 70
    g = torch.Generator().manual_seed(9)
    g0 = torch.randn(B, L, h, w, 64, generator=g).half().to(cuda)
    go = torch.randn(B, L, h, w, generator=g).to(cuda)
    want_ctx, want_planes = _unpack_restated(g0, go, L)
    results = []
    for chunks in ([3], [1, 1, 1], [2, 1]):
        gc = torch.full((B, 32, h, w), float("nan"), device=cuda)
        gp = torch.full((B, L, h, w), float("nan"), device=cuda)
        l0 = 0
        for nl in chunks:
            context_unpack_grad(g0[:, l0:l0 + nl].contiguous(), go, l0, l0 == 0, gc, gp)
            l0 += nl
        results.append((gc, gp))
        assert torch.equal(gc.view(torch.int32), want_ctx.view(torch.int32)), chunks
        assert torch.equal(gp.view(torch.int32), want_planes.view(torch.int32)), chunks
    assert all(torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1]) for r in results)


def test_bad_arguments_launch_nothing(cuda):
    """Bad cin, cout or dilation, misalignment and a short workspace: an error
    code, a message, and no launch."""
    from sfm_amd import _lib
    lib = _lib.load()
    n, h, w, cin, cop = 2, 5, 70, 64, 32
    x = torch.zeros(n, h, w, cin, dtype=torch.float16, device=cuda)
    g = torch.zeros(n, h, w, cop, dtype=torch.float16, device=cuda)
    gw = torch.zeros(9, cop, cin, device=cuda)
    need = lib.sfm_conv2_wgrad_f16_workspace_bytes(n, cin, cop, h, w)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=cuda)
    wd = torch.zeros(9, cin, cop, dtype=torch.float16, device=cuda)
    out = torch.zeros(n, h, w, cin, dtype=torch.float16, device=cuda)
    P = _lib.ptr
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)

    def calls():
        rcs = []
        for kw in (dict(cin=48), dict(cop=1), dict(cop=40), dict(dil=0), dict(dil=17), dict(x=off(x, 8)),
                   dict(g=off(g, 2)), dict(ws=off(ws, 4)), dict(nbytes=need - 1)):
            a = dict(x=P(x), g=P(g), cin=cin, cop=cop, dil=1, ws=P(ws), nbytes=need)
            a.update(kw)
            rcs.append(lib.sfm_conv2_wgrad_f16(a["x"], a["g"], n, a["cin"], a["cop"], h, w, a["dil"], P(gw), a["ws"],
                                               a["nbytes"], None))
            assert lib.sfm_last_error()
        for kw in (dict(cop=48), dict(cip=1), dict(dil=17), dict(g=off(g, 8)), dict(act=off(x, 2))):
            a = dict(g=P(g), cop=cop, cip=cin, dil=1, act=P(x))
            a.update(kw)
            rcs.append(lib.sfm_conv2_dgrad_f16(a["g"], n, a["cop"], h, w, P(wd), a["cip"], a["dil"], a["act"], P(out),
                                               None))
            assert lib.sfm_last_error()
        return rcs

    rcs, launched = _launches(calls)
    assert all(rc != 0 for rc in rcs), rcs
    assert rcs[8] == 3                                                   # the short workspace has its own code
    assert launched == {"conv2_wgrad": 0, "conv2_dgrad": 0, "context_unpack_grad": 0}, launched
