"""The float16 training path of the 3-D regularisation stack on the GPU:
sfm_conv3_wgrad_f16 (csrc/regularize_bwd.hip), the data gradient as
sfm_conv3_f16 on pack_dgrad_weights' packs, conv3_autograd and
CostRegularization.forward_differentiable.

Exact integers must come back bit for bit; general float16 values are held to
the project's rule for float16 routes: err = max|g - g64| / max|g64| against
float64 autograd on the CPU on the same float16 values, at most 2 x the error
of torch's own float16 Conv3d backward (or of the modules under float16
autocast) on the GPU on the same operands, measured in the same test."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, D, H, W).  k_conv3_wgrad's tile is one plane x 4 rows x 64 columns (k_conv3's is 8 x 64):
SHAPES = [
    (2, 3, 9, 67),     # one past k_conv3's 8 x 64 tile in both axes (2 full row tiles + 1 row, 1 column tile + 3), 2 batches
    (1, 1, 5, 7),      # both depth neighbours outside the volume, narrower than any tile, one row past the 4-row tile
    (1, 8, 20, 130),   # 120 tiles: several per accumulating block at every block count below; 130 = 2 tiles + 2
]
CASES = [(s, cin, 32) for s in SHAPES for cin in (32, 64)] + [(SHAPES[0], 32, 1), (SHAPES[0], 64, 1)]
IDS = ["x".join(map(str, s)) + f"-cin{ci}-cout{co}" for s, ci, co in CASES]


def _launches(fn, names=("conv3_f16", "conv3_wgrad")):
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


def _pad32(g):
    """[B, D, H, W, cout] -> the same with cout zero-padded to 32."""
    out = g.new_zeros(tuple(g.shape[:-1]) + (32,))
    out[..., :g.shape[-1]] = g
    return out


def _wgrad(x, gy, cout, cin, cuda):
    from sfm_amd.regularize import conv3_wgrad_f16, unpack_wgrad
    gwp = conv3_wgrad_f16(x.half().to(cuda), _pad32(gy).half().to(cuda))
    assert gwp.dtype == torch.float32 and tuple(gwp.shape) == (27, 32, cin)
    if cout < 32:
        assert bool((gwp[:, cout:] == 0).all())             # the padding's rows: exactly zero
    return unpack_wgrad(gwp, cout, cin)


def _dgrad(gy, wt, cuda):
    from sfm_amd.regularize import conv3_f16, pack_dgrad_weights
    wd = pack_dgrad_weights(wt.float()).half().to(cuda)
    gp = _pad32(gy).half().to(cuda)
    one, zero = torch.ones(32), torch.zeros(32)
    return torch.cat([conv3_f16(gp, wd[k].contiguous(), one, zero) for k in range(wd.shape[0])], -1)


@functools.lru_cache(maxsize=None)
def _int_case(shape, cin, cout):
    """Integer operands and their gradients evaluated in int64 on the CPU, tap by tap."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) * 64 + cin + cout)
    x = torch.randint(-2, 3, (B, D, H, W, cin), generator=g)
    gy = torch.randint(-2, 3, (B, D, H, W, cout), generator=g)
    wt = torch.randint(-1, 2, (cout, cin, 3, 3, 3), generator=g)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    gp = F.pad(gy, (0, 0, 1, 1, 1, 1, 1, 1))
    gw = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.int64)
    gx = torch.zeros(B, D, H, W, cin, dtype=torch.int64)
    gyf = gy.reshape(-1, cout)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                xs = xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, cin)
                gw[:, :, kd, kh, kw] = gyf.t() @ xs                               # sum_p gy[p, co] x[p + k - 1, ci]
                gs = gp[:, 2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W].reshape(-1, cout)
                gx += (gs @ wt[:, :, kd, kh, kw]).reshape(B, D, H, W, cin)        # sum_co W[co, ci, k] gy[p - (k - 1), co]
    assert int(gw.abs().max()) < 2 ** 24 and int(gx.abs().max()) < 2048
    return x, gy, wt, gw, gx


@pytest.mark.parametrize("shape,cin,cout", CASES, ids=IDS)
def test_exact_integers_bit_for_bit(cuda, shape, cin, cout):
    """x, gy in {-2..2}, weights in {-1, 0, 1}: every sum is exact in float32
    (weight gradient) and float16 (data gradient) in any order, so both must
    equal the int64 evaluation -- at 1 accumulating block, a middle count, more
    blocks than tiles, and the default."""
    from sfm_amd import _lib
    x, gy, wt, gw, gx = _int_case(shape, cin, cout)
    B, D, H, W = shape
    tiles = B * D * ((H + 3) // 4) * ((W + 63) // 64)
    try:
        for nb in (0, 1, max(2, tiles // 3), tiles + 5):
            _lib.tune("conv_wgrad_blocks", nb)
            got = _wgrad(x, gy, cout, cin, cuda)
            assert torch.equal(got.cpu().double(), gw.double()), (nb, float((got.cpu().double() - gw).abs().max()))
    finally:
        _lib.tune("conv_wgrad_blocks", 0)
    got = _dgrad(gy, wt, cuda)
    assert got.dtype == torch.float16 and torch.equal(got.cpu().double(), gx.double())


def _general(shape, cin, cout, gscale, seed):
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, D, H, W, generator=g).half()
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cout)) ** 0.5).half()
    gy = (torch.randn(B, cout, D, H, W, generator=g) * gscale).half()
    return x, wt, gy


def _err(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def test_weight_gradient_is_reproducible(cuda):
    """Two calls on general float16 data: identical bits (partial sums added in
    block order, no float atomics)."""
    x, _, gy = _general(SHAPES[2], 64, 32, 1.0, 5)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    a = _wgrad(cl(x), cl(gy), 32, 64, cuda)
    b = _wgrad(cl(x), cl(gy), 32, 64, cuda)
    assert bool((a != 0).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -10], ids=["g1", "g2^-10"])
@pytest.mark.parametrize("shape,cin,cout", CASES, ids=IDS)
def test_general_values_against_float64(cuda, shape, cin, cout, gscale):
    """Activations about 1, gradients about 1 or 2^-10, weights at the stack's
    initial scale: both gradients against float64 autograd on the same float16
    values, next to torch's float16 Conv3d backward on the GPU."""
    x, wt, gy = _general(shape, cin, cout, gscale, 7)
    x64, w64 = x.double().requires_grad_(), wt.double().requires_grad_()
    F.conv3d(x64, w64, padding=1).backward(gy.double())
    xt, wtt = x.to(cuda).requires_grad_(), wt.to(cuda).requires_grad_()
    F.conv3d(xt, wtt, padding=1).backward(gy.to(cuda))
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    gw = _wgrad(cl(x), cl(gy), cout, cin, cuda)
    gx = _dgrad(cl(gy), wt, cuda).permute(0, 4, 1, 2, 3)
    for name, ours, theirs, ref in (("grad_weight", gw, wtt.grad, w64.grad), ("grad_input", gx, xt.grad, x64.grad)):
        e, t = _err(ours, ref), _err(theirs, ref)
        print({"case": name, "shape": shape, "cin": cin, "cout": cout, "gscale": gscale, "err_hip": e, "err_torch_f16": t})
        assert e <= 2.0 * t, (name, e, t)


def test_conv3_autograd_forward_bits_and_needs_input_grad(cuda):
    from sfm_amd import conv3_autograd
    from sfm_amd.regularize import conv3_f16, pack_weights
    for cin, cout in ((64, 32), (32, 1)):
        x, wt, gy = _general(SHAPES[0], cin, cout, 1.0, 9)
        xc = x.permute(0, 2, 3, 4, 1).contiguous().to(cuda)
        w32 = wt.float().to(cuda)
        want = conv3_f16(xc, pack_weights(w32).half(), torch.ones(32), torch.zeros(32), cout=cout)
        g = (gy.permute(0, 2, 3, 4, 1).contiguous() if cout == 32 else gy[:, 0].float()).to(cuda)
        for need_x, need_w in ((True, True), (True, False), (False, True)):
            xa, wa = xc.clone().requires_grad_(need_x), w32.clone().requires_grad_(need_w)
            y, n = _launches(lambda: conv3_autograd(xa, wa))
            assert y.dtype == want.dtype and torch.equal(y, want) and n == {"conv3_f16": 1, "conv3_wgrad": 0}
            _, n = _launches(lambda: y.backward(g))
            assert n == {"conv3_f16": (cin // 32 if need_x else 0), "conv3_wgrad": (1 if need_w else 0)}, n
            assert (xa.grad is not None) == need_x and (wa.grad is not None) == need_w
            if need_w:
                assert wa.grad.dtype == torch.float32 and wa.grad.shape == wa.shape
            if need_x:
                assert xa.grad.dtype == torch.float16 and xa.grad.shape == xa.shape


# ---- forward_differentiable on a seeded CostRegularization -------------------------------------------------------
RB, RL, Rh, Rw = 2, 4, 8, 12


def _stack(reg, cost):
    c0 = reg.dres0(cost)
    for i in range(1, 5):
        c0 = getattr(reg, f"dres{i}")(c0) + c0
    return reg.classify(c0)


@functools.lru_cache(maxsize=None)
def _reg_case(training):
    """The seeded stack, its input and output gradient, and one step of the
    float64 copy on the CPU (computed once, shared, left unchanged)."""
    from sfm_amd.regularize import CostRegularization
    torch.manual_seed(21)
    reg = CostRegularization(64).train(training)
    g = torch.Generator().manual_seed(22)
    for m in reg.modules():                      # running statistics and affines away from 0 / 1, so eval mode uses them
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.copy_(0.1 * torch.randn(32, generator=g))
            m.running_var.copy_(1.0 + 0.5 * torch.rand(32, generator=g))
            m.weight.data.copy_(1.0 + 0.2 * torch.randn(32, generator=g))
            m.bias.data.copy_(0.1 * torch.randn(32, generator=g))
    cost = torch.randn(RB, 64, RL, Rh, Rw, generator=g)
    gout = torch.randn(RB, 1, RL, Rh, Rw, generator=g)
    r64 = copy.deepcopy(reg).double()
    c64 = cost.double().requires_grad_()
    out64 = _stack(r64, c64)
    out64.backward(gout.double())
    return reg, cost, gout, r64, c64.grad, out64.detach()


def _arm(reg, cost, gout, cuda, hip):
    r = copy.deepcopy(reg).to(cuda)
    c = cost.to(cuda).requires_grad_()
    with torch.autocast("cuda", torch.float16):
        out = r.forward_differentiable(c) if hip else _stack(r, c)
    if gout is not None:
        out.float().backward(gout.to(cuda))
    return r, c.grad, out.detach().float()


def test_forward_differentiable_training_step(cuda):
    """Training mode: every parameter gradient, the input gradient and the
    BatchNorm running statistics after the step against the float64 copy, next
    to the modules under float16 autocast."""
    reg, cost, gout, r64, gin64, out64 = _reg_case(True)
    (rh, gin_h, out_h), n = _launches(lambda: _arm(reg, cost, gout, cuda, True))
    assert n == {"conv3_f16": 12 + 12 + 1, "conv3_wgrad": 12}, n       # dres0[0]'s data gradient is two calls
    rt, gin_t, out_t = _arm(reg, cost, gout, cuda, False)
    assert out_h.shape == (RB, 1, RL, Rh, Rw)
    p64, ph, pt = (dict(r.named_parameters()) for r in (r64, rh, rt))
    rows = [("input", gin_h, gin_t, gin64), ("output", out_h, out_t, out64)]
    rows += [(k, ph[k].grad, pt[k].grad, p64[k].grad) for k in p64]
    b64, bh, bt = (dict(r.named_buffers()) for r in (r64, rh, rt))
    rows += [(k, bh[k], bt[k], b64[k]) for k in b64 if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(rows) == 2 + 12 + 22 + 22
    bad = []
    for k, ours, theirs, ref in rows:
        assert ours is not None and bool(torch.isfinite(ours).all()), k
        e, t = _err(ours, ref), _err(theirs, ref)
        print({"tensor": k, "err_hip": e, "err_modules_f16": t})
        if not e <= 2.0 * t:
            bad.append((k, e, t))
    assert not bad, bad
    for k in b64:
        if k.endswith("num_batches_tracked"):
            assert int(bh[k]) == int(b64[k]) == 1


def test_forward_differentiable_eval_mode(cuda):
    """Eval mode: BatchNorm uses the running statistics (which stay put); the
    output against the float64 modules, next to the modules under autocast."""
    reg, cost, _, r64, _, out64 = _reg_case(False)
    rh, _, out_h = _arm(reg, cost, None, cuda, True)
    _, _, out_t = _arm(reg, cost, None, cuda, False)
    e, t = _err(out_h, out64), _err(out_t, out64)
    print({"tensor": "eval output", "err_hip": e, "err_modules_f16": t})
    assert e <= 2.0 * t, (e, t)
    for k, v in reg.named_buffers():
        assert torch.equal(dict(rh.named_buffers())[k].cpu(), v), k
