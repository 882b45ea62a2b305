"""The plane sweep's backward kernel (sfm_plane_sweep_backward,
sfm_inverse_warp_backward; csrc/sweep_bwd.hip) and the autograd entry points
over it, against tests/sweep_bwd_cases.py: exact lattices bit for bit, the
reference's own autograd (tests/golden/sweep_grad.npz), general poses against
the float64 scatter, the adjoint identity, and the Python surface.

Bar (sweep_bwd_cases.close): |got - want| <= 1e-4 max(|want|, RMS(want)).
Observed maxima on an MI355X: see each test's docstring."""
import pytest
import torch

from tests import sweep_bwd_cases as BC

pytestmark = pytest.mark.gpu


def _backward(g, case, cuda, warped_only=False, want_ref=True):
    """One sfm_plane_sweep_backward call on CPU tensors: (grad_ref or None, grad_tgt) on the CPU."""
    from sfm_amd import _lib
    from sfm_amd.sweep import backward_workspace_for
    B, rows, L, h, w = g.shape
    C = rows if warped_only else rows // 2
    gd = g.to(cuda).contiguous()
    pose, K4, Ki4 = case.pose.to(cuda).contiguous(), case.K4.to(cuda).contiguous(), case.Ki4.to(cuda).contiguous()
    grad_tgt = torch.full((B, C, h, w), 7.0, device=cuda)          # the call zeroes it itself
    grad_ref = torch.full((B, C, h, w), 7.0, device=cuda) if (want_ref and not warped_only) else None
    ws = backward_workspace_for(B, C, h, w, L, cuda)
    rc = _lib.load().sfm_plane_sweep_backward(_lib.ptr(gd), 1 if warped_only else 0, B, C, h, w, _lib.ptr(pose),
                                              _lib.ptr(K4), _lib.ptr(Ki4), L, case.min_depth,
                                              1 if case.by_depth else 0, _lib.ptr(grad_ref), _lib.ptr(grad_tgt),
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr(cuda))
    _lib.check(rc, "sfm_plane_sweep_backward")
    torch.cuda.synchronize()
    return (None if grad_ref is None else grad_ref.cpu()), grad_tgt.cpu()


@pytest.mark.parametrize("C,L", BC.LATTICE_CL)
@pytest.mark.parametrize("kind", list(BC.LATTICE_SHIFTS))
def test_exact_lattice(kind, C, L, cuda):
    """Integer-valued g on sample positions that are exact integers or
    half-integers: every sum is exact in any order, so the atomics reproduce
    the closed form bit for bit; grad_ref is the plane sum."""
    from sfm_amd import _lib
    case = BC.lattice_case(kind, L)
    g = BC.integer_g(2, 2 * C, L, case.h, case.w, seed=17 + C + L)
    grad_ref, grad_tgt = _backward(g, case, cuda)
    assert _lib.last_sweep() == "k_sweep_bwd"
    want = BC.lattice_expected(kind, g[:, C:])
    if kind == "identity":
        assert torch.equal(want, g[:, C:].sum(2))
    assert bool((want[0] != want[1]).any())
    assert torch.equal(grad_tgt, want), float((grad_tgt - want).abs().max())
    assert torch.equal(grad_ref, g[:, :C].sum(2))
    # the warped-only layout: the same gradient from the warped half alone
    none, tgt2 = _backward(g[:, C:].contiguous(), case, cuda, warped_only=True)
    assert none is None and torch.equal(tgt2, want)


def test_golden_reference_autograd(golden, cuda):
    """The reference's own autograd through its sweep loop and through one
    inverse_warp call with a depth map.  Observed max |diff|: cost grad_tgt
    7.0e-06 against a floor (RMS) of 1.06, grad_ref 4.8e-07 (floor 2.04);
    inverse_warp grad_feat 6.2e-06 (floor 0.58)."""
    from sfm_amd.sweep import inverse_warp_autograd, plane_sweep_cost_autograd
    z = golden("sweep_grad.npz")
    c = z["cost"]
    t = {k: torch.from_numpy(v).to(cuda) for k, v in c.items() if v.ndim > 0}
    ref, tgt = t["ref"].requires_grad_(), t["tgt"].requires_grad_()
    cost = plane_sweep_cost_autograd(ref, tgt, t["pose"], t["K4"], t["K4inv"], int(c["nlabel"]), float(c["min_depth"]))
    cost.backward(t["g"])
    for name, got in (("grad_tgt", tgt.grad), ("grad_ref", ref.grad)):
        ok, err, floor = BC.close(got, t[name])
        print({name: err, "floor": floor})
        assert ok, (name, err, floor)
    v = {k: torch.from_numpy(a).to(cuda) for k, a in z["warp"].items()}
    feat = v["feat"].requires_grad_()
    inverse_warp_autograd(feat, v["depth"], v["pose"], v["K"], v["Kinv"]).backward(v["g"])
    ok, err, floor = BC.close(feat.grad, v["grad_feat"])
    print({"grad_feat": err, "floor": floor})
    assert ok, (err, floor)


@pytest.mark.parametrize("h,w", BC.GENERAL_SHAPES)
@pytest.mark.parametrize("name", list(BC.GENERAL))
def test_general_poses(name, h, w, cuda):
    """Rolls, a 90 degree roll, samples behind the camera and nothing in
    range, against the float64 scatter at the oracle's float32 positions.  (At
    these shapes the kernel's window holds every target row: the taps that
    leave a window are test_window_paths'.)  Observed max |diff| over the cases 2.1e-06 against
    floors (RMS of the expected gradient) of 0.34 - 1.43."""
    case = BC.general_case(name, h, w)
    C, L = BC.GENERAL_C, case.L
    g = torch.randn(2, 2 * C, L, h, w, generator=torch.Generator().manual_seed(3 + h))
    want, inside = BC.expected_grad_tgt(case, g[:, C:])
    grad_ref, grad_tgt = _backward(g, case, cuda)
    if name == "all_out":
        assert int(inside.sum()) == 0 and not grad_tgt.any()
    else:
        ok, err, floor = BC.close(grad_tgt, want)
        print({"case": case.name, "max_err": err, "floor": floor, "in_range": int(inside.sum())})
        assert ok, (err, floor)
    ok, err, floor = BC.close(grad_ref, g[:, :C].double().sum(2))
    assert ok, (err, floor)


@pytest.mark.parametrize("spec", [BC.TALL, BC.WIDE], ids=lambda s: s["name"])
def test_window_paths(spec, cuda):
    """The parts of k_sweep_bwd the small shapes above never launch (there the
    LDS window is the whole image and a chunk is one plane), against the same
    float64 scatter and bar.
      tall  40 x 24, B = 4, C = 28, L = 52: a window of 10 of 40 rows, chunks of
            4 planes summed into one window placed on the chunk's middle
            plane, a last channel group of 4; by the replayed window placement
            44 % of the row-taps leave their window for a global atomic (the
            two 90 degree rolls spread a band over up to 25 target rows)
      wide  3 x 1100, C = 12: no row fits a window, "k_sweep_bwd+global"
    Observed max |diff|: tall 1.0e-05 against a floor (RMS) of 3.43, wide
    9.8e-07 against 0.77."""
    from sfm_amd import _lib
    case = BC.shaped_case(spec)
    B, C, L, h, w = case.pose.shape[0], spec["C"], case.L, case.h, case.w
    n_in, n_out, q = BC.window_replay(case, C)
    if spec is BC.TALL:
        assert q.lp == 4 and 2 <= q.wr < h and q.blocks >= 1024
        assert n_out > 0.4 * (n_in + n_out) and n_in > 0.4 * (n_in + n_out)
    else:
        assert q.wr == 0 and n_in == 0 and n_out > 0
    assert C % 8 == 4 and C > 8
    g = torch.randn(B, 2 * C, L, h, w, generator=torch.Generator().manual_seed(41))
    want, inside = BC.expected_grad_tgt(case, g[:, C:])
    grad_ref, grad_tgt = _backward(g, case, cuda)
    assert _lib.last_sweep() == ("k_sweep_bwd" if spec is BC.TALL else "k_sweep_bwd+global")
    ok, err, floor = BC.close(grad_tgt, want)
    print({"case": case.name, "max_err": err, "floor": floor, "in_range": int(inside.sum()), "outside_window": n_out,
           "in_window": n_in})
    assert ok, (err, floor)
    for b in range(B):                                   # every pair and every channel group contributes
        assert bool((want[b, C - 1] != 0).any()) and bool((grad_tgt[b, C - 1] != 0).any())
    ok, err, floor = BC.close(grad_ref, g[:, :C].double().sum(2))
    assert ok, (err, floor)
    # the warped-only layout through the same paths
    _, tgt2 = _backward(g[:, C:].contiguous(), case, cuda, warped_only=True)
    ok, err, floor = BC.close(tgt2, want)
    assert ok, (err, floor)


@pytest.mark.parametrize("name,h,w", [("roll30_sideways", 10, 12), ("roll_90", 7, 5), ("partly_behind", 10, 12)])
def test_adjoint_identity(name, h, w, cuda):
    """<F t, g> == <t, F^T g> for the forward's warped half F and the backward
    F^T, evaluated in float64 on the host from the GPU outputs: the difference
    is at most 1e-4 of the sum of the terms' magnitudes.  Measured ratio
    |lhs - rhs| / sum |terms|: 5.1e-10 or less."""
    from sfm_amd.sweep import plane_sweep_cost
    case = BC.general_case(name, h, w)
    C, L = BC.GENERAL_C, case.L
    gen = torch.Generator().manual_seed(11 + w)
    t = torch.randn(2, C, h, w, generator=gen)
    g = torch.randn(2, C, L, h, w, generator=gen)
    Ft = plane_sweep_cost(None, t.to(cuda), case.pose.to(cuda), case.K4.to(cuda), case.Ki4.to(cuda), L,
                          case.min_depth, warped_only=True).cpu()
    _, FTg = _backward(g, case, cuda, warped_only=True)
    lhs_terms, rhs_terms = Ft.double() * g.double(), t.double() * FTg.double()
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    scale = float(lhs_terms.abs().sum() + rhs_terms.abs().sum())
    print({"case": case.name, "lhs": lhs, "rhs": rhs, "ratio": abs(lhs - rhs) / scale})
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


def _surface_inputs(cuda, C=8):
    case = BC.general_case("roll30_sideways", 10, 12)
    gen = torch.Generator().manual_seed(23)
    ref = torch.randn(2, C, case.h, case.w, generator=gen).to(cuda)
    tgt = torch.randn(2, C, case.h, case.w, generator=gen).to(cuda)
    g = torch.randn(2, 2 * C, case.L, case.h, case.w, generator=gen).to(cuda)
    return case, ref, tgt, g, (case.pose.to(cuda), case.K4.to(cuda), case.Ki4.to(cuda), case.L, case.min_depth)


def test_python_surface_forward_bits_and_warped_only(cuda):
    from sfm_amd.sweep import plane_sweep_cost, plane_sweep_cost_autograd
    case, ref, tgt, g, geo = _surface_inputs(cuda)
    C = ref.shape[1]
    r, t = ref.clone().requires_grad_(), tgt.clone().requires_grad_()
    cost = plane_sweep_cost_autograd(r, t, *geo)
    assert cost.requires_grad and cost.dtype == torch.float32
    assert torch.equal(cost.detach(), plane_sweep_cost(ref, tgt, *geo, dtype=torch.float32))
    cost.backward(g)
    # (sfm_last_sweep is per thread and autograd runs the backward on its own: test_exact_lattice asserts the form)
    want, _ = BC.expected_grad_tgt(case, g[:, C:].cpu())
    ok, err, floor = BC.close(t.grad, want)
    assert ok, (err, floor)
    assert torch.equal(r.grad, _plane_sum(g[:, :C]))
    # warped_only: no reference features, the same target gradient from the warped half's gradient
    t2 = tgt.clone().requires_grad_()
    w_only = plane_sweep_cost_autograd(None, t2, *geo, warped_only=True)
    assert torch.equal(w_only.detach(), cost.detach()[:, C:])
    w_only.backward(g[:, C:].contiguous())
    ok, err, floor = BC.close(t2.grad, want)
    assert ok, (err, floor)
    # predict_by_depth planes go through both directions
    t3 = tgt.clone().requires_grad_()
    by_depth = plane_sweep_cost_autograd(ref, t3, *geo, predict_by_depth=True)
    assert torch.equal(by_depth.detach(), plane_sweep_cost(ref, tgt, *geo, predict_by_depth=True))
    by_depth.backward(g)
    want3, _ = BC.expected_grad_tgt(case._replace(by_depth=True), g[:, C:].cpu())
    ok, err, floor = BC.close(t3.grad, want3)
    assert ok, (err, floor)


def _plane_sum(g):
    """sum over planes in index order, float32 (k_sweep_bwd_ref's order)."""
    acc = g[:, :, 0].clone()
    for i in range(1, g.shape[2]):
        acc = acc + g[:, :, i]
    return acc


def test_python_surface_dtypes_refusals_and_module(cuda):
    from sfm_amd.sweep import PlaneSweep, inverse_warp, inverse_warp_autograd, plane_sweep_cost_autograd
    case, ref, tgt, g, geo = _surface_inputs(cuda)
    C = ref.shape[1]
    # float16 features in, float16 gradients out (of the float32 gradient, rounded once)
    r32, t32 = ref.half().float().requires_grad_(), tgt.half().float().requires_grad_()
    plane_sweep_cost_autograd(r32, t32, *geo).backward(g)
    r16, t16 = ref.half().requires_grad_(), tgt.half().requires_grad_()
    cost16 = plane_sweep_cost_autograd(r16, t16, *geo)
    assert cost16.dtype == torch.float32
    cost16.backward(g)
    assert t16.grad.dtype == torch.float16 and r16.grad.dtype == torch.float16
    assert torch.equal(r16.grad, r32.grad.half())
    assert float((t16.grad.float() - t32.grad).abs().max()) <= 2.0 ** -10 * float(t32.grad.abs().max())
    # geometry that requires grad is still refused
    pose = geo[0].clone().requires_grad_()
    with pytest.raises(RuntimeError, match="requires grad"):
        plane_sweep_cost_autograd(ref, tgt, pose, *geo[1:])
    with pytest.raises(RuntimeError, match="requires grad"):
        plane_sweep_cost_autograd(ref, tgt, geo[0], geo[1].clone().requires_grad_(), *geo[2:])
    depth = 2.0 + torch.rand(2, case.h, case.w, generator=torch.Generator().manual_seed(2)).to(cuda)
    with pytest.raises(RuntimeError, match="requires grad"):
        inverse_warp_autograd(tgt, depth.clone().requires_grad_(), *geo[:3])
    with pytest.raises(RuntimeError, match="requires grad"):
        inverse_warp_autograd(tgt, depth, pose, *geo[1:3])
    # inverse_warp_autograd: the forward's bits, and the scatter at a depth map
    f = tgt.clone().requires_grad_()
    out = inverse_warp_autograd(f, depth, *geo[:3])
    assert torch.equal(out.detach(), inverse_warp(tgt, depth, *geo[:3]))
    gw = g[:, :C, 0].contiguous()
    out.backward(gw)
    want = BC.expected_warp_grad(tgt.shape, depth.cpu(), case.pose, case.K4, case.Ki4, gw.cpu())
    ok, err, floor = BC.close(f.grad, want)
    assert ok, (err, floor)
    # the module: differentiable=True takes the autograd function, the default stays forward-only
    K = case.K4.clone()
    K[:, :2, :] = K[:, :2, :] * 4
    Kd, Kid = K.to(cuda), torch.inverse(K).to(cuda)
    rm, tm = ref.clone().requires_grad_(), tgt.clone().requires_grad_()
    vols = PlaneSweep(case.L, case.min_depth, differentiable=True)(rm, [tm], geo[0].unsqueeze(1).clone(), Kd, Kid)
    assert len(vols) == 1 and vols[0].requires_grad
    vols[0].backward(g)
    assert torch.equal(rm.grad, _plane_sum(g[:, :C]))
    from sfm_amd.sweep import quarter_intrinsics
    Kq, Kiq = quarter_intrinsics(Kd, Kid)
    want, _ = BC.expected_grad_tgt(case._replace(K4=Kq.cpu(), Ki4=Kiq.cpu()), g[:, C:].cpu())
    ok, err, floor = BC.close(tm.grad, want)
    assert ok, (err, floor)
    with pytest.raises(RuntimeError, match="forward-only"):
        PlaneSweep(case.L, case.min_depth)(rm, [tm], geo[0].unsqueeze(1).clone(), Kd, Kid)


def test_two_backward_calls_agree(cuda):
    """Float atomics: two calls on the same inputs agree within 1e-6 of the
    gradient's RMS (observed: 2.4e-07 at an RMS of 0.75, 3.2e-07 of it);
    grad_ref is the same bits, and sfm_last_sweep names the backward form."""
    from sfm_amd import _lib
    case = BC.general_case("roll30_sideways", 10, 12)
    C = BC.GENERAL_C
    g = torch.randn(2, 2 * C, case.L, case.h, case.w, generator=torch.Generator().manual_seed(29))
    ref1, tgt1 = _backward(g, case, cuda)
    ref2, tgt2 = _backward(g, case, cuda)
    assert _lib.last_sweep() == "k_sweep_bwd"
    rms = float(tgt1.double().pow(2).mean().sqrt())
    diff = float((tgt1 - tgt2).abs().max())
    print({"max_diff": diff, "rms": rms})
    assert rms > 0 and diff <= 1e-6 * rms, (diff, rms)
    assert torch.equal(ref1, ref2)
