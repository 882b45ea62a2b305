"""The float16 backward of the feature CNN's convolutions on the GPU, kernel by
kernel (csrc/feature_bwd.hip): sfm_conv2x_wgrad_f16 and sfm_conv2x_dgrad_f16
over the CNN's layer kinds -- 3 x 3 and 1 x 1, stride 1 and 2, a dilation, 320
input channels -- and ``conv2x_autograd`` over them.

Exact integers must come back bit for bit; general float16 values are held to
the project's rule for float16 routes: err = max|g - g64| / max|g64| against
float64 autograd on the CPU on the same float16 operands, at most 2 x the error
of torch's own float16 conv2d backward on the GPU on the same operands,
measured in the same test."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (cin_pad, real cin, cout, k, stride, dilation)
KINDS = [(32, 3, 32, 3, 2, 1), (32, 32, 64, 3, 2, 1), (32, 32, 64, 1, 2, 1), (64, 64, 128, 1, 1, 1),
         (128, 128, 32, 1, 1, 1), (128, 128, 128, 3, 1, 2), (320, 320, 128, 3, 1, 1)]
# (images, hin, win): odd both ways (66 output columns at stride 2 cross the 64-column tile), even, a third image
# and a row tile of one row, smaller than a kernel, a single pixel
SHAPES = [(2, 9, 131), (1, 8, 130), (3, 5, 70), (1, 2, 3), (1, 1, 1)]
CASES = [(s, kd) for kd in KINDS for s in SHAPES]


def _kid(kd):
    return f"{kd[1]}to{kd[2]}-k{kd[3]}s{kd[4]}d{kd[5]}"


IDS = ["x".join(map(str, s)) + "-" + _kid(kd) for s, kd in CASES]


def _launches(fn, names=("conv2x_wgrad", "conv2x_dgrad", "feature_conv2x")):
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


def _conv(x, wt, kd):
    _, _, _, k, stride, dil = kd
    return F.conv2d(x, wt, stride=stride, padding=dil if k == 3 else 0, dilation=dil)


def _backward64(x, wt, gy, kd):
    x = x.double().clone().requires_grad_(True)
    wt = wt.double().clone().requires_grad_(True)
    _conv(x, wt, kd).backward(gy.double())
    return x.grad, wt.grad


def _out_hw(shape, kd):
    return (shape[1] - 1) // kd[4] + 1, (shape[2] - 1) // kd[4] + 1


def _wgrad(x, gy, kd, cuda):
    from sfm_amd.feature import conv2x_wgrad_f16, unpack_wgrad2x
    cip, cin, cout, k, stride, dil = kd
    gwp = conv2x_wgrad_f16(_cl(x, cuda, cip), _cl(gy, cuda), k, stride, dil)
    assert gwp.dtype == torch.float32 and tuple(gwp.shape) == (k * k, cout, cip)
    if cin < cip:
        assert bool((gwp[:, :, cin:] == 0).all())               # the padding's columns: exactly zero
    return unpack_wgrad2x(gwp, cout, cin, k)


def _dgrad(gy, wt, shape, kd, cuda):
    from sfm_amd.feature import conv2x_dgrad_f16, pack_dgrad_weights2x
    cip, cin, cout, k, stride, dil = kd
    wd = pack_dgrad_weights2x(wt.float()).half().to(cuda)
    out = conv2x_dgrad_f16(_cl(gy, cuda), wd, shape[1:], k, stride, dil)
    assert out.dtype == torch.float16 and tuple(out.shape) == (shape[0], shape[1], shape[2], cip)
    if cin < cip:
        assert bool((out[..., cin:].contiguous().view(torch.int16) == 0).all())    # the padding's channels: +0
    return out[..., :cin].permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _int_case(shape, kd):
    """Weights in {-1, 0, 1}, activations in {0, 1}, gradients in {-1, 0, 1} and
    the float64 CPU convolution backward on them."""
    n, h, w = shape
    _, cin, cout, k, stride, dil = kd
    ho, wo = _out_hw(shape, kd)
    g = torch.Generator().manual_seed(sum(shape) * 64 + cin + cout + 7 * k + stride + dil)
    x = torch.randint(0, 2, (n, cin, h, w), generator=g).double()
    gy = torch.randint(-1, 2, (n, cout, ho, wo), generator=g).double()
    wt = torch.randint(-1, 2, (cout, cin, k, k), generator=g).double()
    gx, gw = _backward64(x, wt, gy, kd)
    assert float(gw.abs().max()) < 2 ** 24 and float(gx.abs().max()) < 2048
    return x, gy, wt, gw, gx


@pytest.mark.parametrize("shape,kd", CASES, ids=IDS)
def test_exact_integers_bit_for_bit(cuda, shape, kd):
    """Every sum is exact in float32 (weight gradient) and float16 (data
    gradient, |.| <= 9 * 128 < 2048) in any order, so both must equal the
    float64 evaluation -- the weight gradient at the default, 1 and 3
    accumulating blocks and more blocks than tiles."""
    from sfm_amd import _lib
    x, gy, wt, gw, gx = _int_case(shape, kd)
    ho, wo = _out_hw(shape, kd)
    tiles = shape[0] * ((ho + 3) // 4) * ((wo + 63) // 64)
    try:
        for nb in (0, 1, 3, tiles + 5):
            _lib.tune("conv2_wgrad_blocks", nb)
            got = _wgrad(x, gy, kd, cuda)
            assert torch.equal(got.cpu().double(), gw), (nb, float((got.cpu().double() - gw).abs().max()))
    finally:
        _lib.tune("conv2_wgrad_blocks", 0)
    got = _dgrad(gy, wt, shape, kd, cuda)
    assert torch.equal(got.cpu().double(), gx), float((got.cpu().double() - gx).abs().max())


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


GENERAL = [((2, 9, 131), KINDS[0]), ((2, 9, 131), KINDS[1]), ((1, 8, 130), KINDS[2]), ((3, 5, 70), KINDS[3]),
           ((2, 9, 131), KINDS[4]), ((3, 5, 70), KINDS[5]), ((2, 9, 131), KINDS[6])]


@functools.lru_cache(maxsize=None)
def _general(shape, kd, gscale):
    n, h, w = shape
    _, cin, cout, k, stride, dil = kd
    ho, wo = _out_hw(shape, kd)
    g = torch.Generator().manual_seed(7 * cin + cout + dil + 3 * k + stride + int(gscale < 1))
    x = torch.randn(n, cin, h, w, generator=g).half()
    wt = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cout)) ** 0.5).half()
    gy = (torch.randn(n, cout, ho, wo, generator=g) * gscale).half()
    return (x, wt, gy) + _backward64(x, wt, gy, kd)


@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -10], ids=["g1", "g2^-10"])
@pytest.mark.parametrize("shape,kd", GENERAL, ids=["x".join(map(str, s)) + "-" + _kid(kd) for s, kd in GENERAL])
def test_general_values_against_float64_and_torch(cuda, shape, kd, gscale):
    """N(0, 1) rounded to float16, gradients at scale 1 and 2^-10: ours within
    2 x the error torch's own float16 conv2d backward makes on the same
    operands on the same GPU; two calls give equal bits."""
    x, wt, gy, gx64, gw64 = _general(shape, kd, gscale)
    xt = x.to(cuda).requires_grad_(True)
    wtt = wt.to(cuda).requires_grad_(True)
    _conv(xt, wtt, kd).backward(gy.to(cuda))
    ours_w = _wgrad(x, gy, kd, cuda)
    ours_x = _dgrad(gy, wt, shape, kd, cuda)
    rec = {"kind": kd, "shape": shape, "gscale": gscale,
           "wgrad_err_hip": _err(ours_w, gw64), "wgrad_err_torch_f16": _err(wtt.grad, gw64),
           "dgrad_err_hip": _err(ours_x, gx64), "dgrad_err_torch_f16": _err(xt.grad, gx64)}
    print(rec)
    assert rec["wgrad_err_hip"] <= 2.0 * rec["wgrad_err_torch_f16"], rec
    assert rec["dgrad_err_hip"] <= 2.0 * rec["dgrad_err_torch_f16"], rec
    again_w = _wgrad(x, gy, kd, cuda)
    again_x = _dgrad(gy, wt, shape, kd, cuda)
    assert torch.equal(ours_w.view(torch.int32), again_w.view(torch.int32))
    assert torch.equal(ours_x.contiguous().view(torch.int16), again_x.contiguous().view(torch.int16))


@pytest.mark.parametrize("cin,cout,dil", [(64, 128, 1), (128, 96, 8), (96, 64, 16), (32, 32, 1)])
def test_bits_of_the_context_kernels_where_the_shapes_overlap(cuda, cin, cout, dil):
    """3 x 3 / stride 1 / cin <= 128: conv2x_wgrad_f16 is conv2_wgrad_f16 and
    conv2x_dgrad_f16 is conv2_dgrad_f16(act=None), bit for bit."""
    from sfm_amd.context import conv2_dgrad_f16, conv2_wgrad_f16
    from sfm_amd.feature import conv2x_dgrad_f16, conv2x_wgrad_f16
    g = torch.Generator().manual_seed(cin + cout + dil)
    n, h, w = 2, 9, 70
    x = torch.randn(n, h, w, cin, generator=g).half().to(cuda)
    gy = torch.randn(n, h, w, cout, generator=g).half().to(cuda)
    wd = (torch.randn(9, cin, cout, generator=g) * 0.05).half().to(cuda)
    a, b = conv2x_wgrad_f16(x, gy, 3, 1, dil), conv2_wgrad_f16(x, gy, dil)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = conv2x_dgrad_f16(gy, wd, (h, w), 3, 1, dil), conv2_dgrad_f16(gy, wd, dil, None)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("cout", [96, 64], ids=["ng3", "ng2"])
# two column tiles, the second ragged, two row tiles, the second of one row, a second image; a single pixel
@pytest.mark.parametrize("shape", [(2, 5, 70), (1, 1, 1)], ids=["2x5x70", "1x1x1"])
def test_one_weight_gradient_kernel_the_same_bits_per_channel_slice(cuda, shape, cout, dil):
    """3 x 3 / stride 1 at 160 input channels (past sfm_conv2_wgrad_f16's 128)
    against sfm_conv2_wgrad_f16 on the channels 0..127 and 128..159: each
    32-channel slice of ci is accumulated by its own blocks, over the same
    tile ranges, in the same order, so general float16 data gives the same
    bits -- no tolerance -- at the default and at 3 accumulating blocks."""
    from sfm_amd import _lib
    from sfm_amd.context import conv2_wgrad_f16
    from sfm_amd.feature import conv2x_wgrad_f16
    n, h, w = shape
    g = torch.Generator().manual_seed(160 + cout + dil + h * w)
    x = torch.randn(n, h, w, 160, generator=g).half().to(cuda)
    gy = torch.randn(n, h, w, cout, generator=g).half().to(cuda)
    lo, hi = x[..., :128].contiguous(), x[..., 128:].contiguous()
    try:
        for nb in (0, 3):
            _lib.tune("conv2_wgrad_blocks", nb)
            whole = conv2x_wgrad_f16(x, gy, 3, 1, dil)
            assert tuple(whole.shape) == (9, cout, 160) and bool((whole != 0).any())
            assert torch.equal(whole[:, :, :128], conv2_wgrad_f16(lo, gy, dil)), nb
            assert torch.equal(whole[:, :, 128:], conv2_wgrad_f16(hi, gy, dil)), nb
    finally:
        _lib.tune("conv2_wgrad_blocks", 0)


@pytest.mark.parametrize("kd", KINDS, ids=[_kid(kd) for kd in KINDS])
def test_autograd_forward_bits_and_needs_input_grad(cuda, kd):
    """conv2x_autograd's forward is conv2x_f16 with a unit affine, bit for
    bit; its backward launches each kernel only for an input that needs a
    gradient, and returns the weight gradient in the parameter's layout and
    dtype."""
    from sfm_amd.feature import conv2x_autograd, conv2x_dgrad_f16, conv2x_f16, conv2x_wgrad_f16, \
        pack_dgrad_weights2x, unpack_wgrad2x
    cip, cin, cout, k, stride, dil = kd
    n, h, w = 2, 9, 70
    g = torch.Generator().manual_seed(11 + cin + cout)
    x = torch.zeros(n, h, w, cip)
    x[..., :cin] = torch.randn(n, h, w, cin, generator=g)
    x = x.half().to(cuda)
    wt = (torch.randn(cout, cin, k, k, generator=g) * 0.1).to(cuda)
    wp = torch.zeros(k * k, cout, cip, device=cuda)
    wp[:, :, :cin] = wt.permute(2, 3, 0, 1).reshape(k * k, cout, cin)
    want = conv2x_f16(x, wp.half(), torch.ones(cout), torch.zeros(cout), k, stride, dil, relu=False)
    gy = torch.randn(want.shape, generator=g).half().to(cuda)
    for need_x, need_w in ((True, True), (False, True), (True, False)):
        xi = x.clone().requires_grad_(need_x)
        wi = wt.clone().requires_grad_(need_w)

        def step():
            y = conv2x_autograd(xi, wi, stride, dil)
            y.backward(gy)
            return y
        y, launched = _launches(step)
        assert torch.equal(y.detach().view(torch.int16), want.view(torch.int16))
        assert launched == {"conv2x_wgrad": int(need_w), "conv2x_dgrad": int(need_x), "feature_conv2x": 1}, launched
        if need_w:
            ref = unpack_wgrad2x(conv2x_wgrad_f16(x, gy, k, stride, dil), cout, cin, k)
            assert wi.grad.dtype == wt.dtype and tuple(wi.grad.shape) == tuple(wt.shape)
            assert torch.equal(wi.grad, ref)
        else:
            assert wi.grad is None
        if need_x:
            ref = conv2x_dgrad_f16(gy, pack_dgrad_weights2x(wt).half(), (h, w), k, stride, dil)
            assert torch.equal(xi.grad.view(torch.int16), ref.view(torch.int16))
        else:
            assert xi.grad is None


def test_bad_arguments_launch_nothing(cuda):
    """A bad layer, an inconsistent input size, misalignment and a short
    workspace on real device buffers: an error code, a message, no launch."""
    import ctypes
    from sfm_amd import _lib
    lib = _lib.load()
    n, h, w, cin, cout = 2, 9, 70, 32, 64
    ho, wo = 5, 35
    x = torch.zeros(n, h, w, cin, dtype=torch.float16, device=cuda)
    g = torch.zeros(n, ho, wo, cout, dtype=torch.float16, device=cuda)
    gw = torch.zeros(9, cout, cin, device=cuda)
    need = lib.sfm_conv2x_wgrad_f16_workspace_bytes(n, cin, cout, h, w, 3, 2)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=cuda)
    wd = torch.zeros(9, cin, cout, dtype=torch.float16, device=cuda)
    out = torch.zeros(n, h, w, cin, dtype=torch.float16, device=cuda)
    P = _lib.ptr
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)

    def calls():
        rcs = []
        for kw in (dict(cin=48), dict(cout=1), dict(k=2), dict(stride=3), dict(dil=2), dict(x=off(x, 8)),
                   dict(g=off(g, 2)), dict(ws=off(ws, 4)), dict(nbytes=need - 1)):
            a = dict(x=P(x), g=P(g), cin=cin, cout=cout, k=3, stride=2, dil=1, ws=P(ws), nbytes=need)
            a.update(kw)
            rcs.append(lib.sfm_conv2x_wgrad_f16(a["x"], a["g"], n, a["cin"], a["cout"], h, w, a["k"], a["stride"],
                                                a["dil"], P(gw), a["ws"], a["nbytes"], None))
            assert lib.sfm_last_error()
        for kw in (dict(cout=48), dict(cin=1), dict(dil=2), dict(hin=11), dict(g=off(g, 8)), dict(out=P(g))):
            a = dict(g=P(g), cout=cout, cin=cin, dil=1, hin=h, out=P(out))
            a.update(kw)
            rcs.append(lib.sfm_conv2x_dgrad_f16(a["g"], n, a["cout"], ho, wo, P(wd), a["cin"], a["hin"], w, 3, 2,
                                                a["dil"], a["out"], None))
            assert lib.sfm_last_error()
        return rcs

    rcs, launched = _launches(calls, names=("conv2x_wgrad", "conv2x_dgrad", "conv2_wgrad", "conv2_dgrad"))
    assert all(rc != 0 for rc in rcs), rcs
    assert rcs[8] == 3                                                   # the short workspace has its own code
    assert launched == {"conv2x_wgrad": 0, "conv2x_dgrad": 0, "conv2_wgrad": 0, "conv2_dgrad": 0}, launched
