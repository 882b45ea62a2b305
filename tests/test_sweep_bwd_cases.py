"""The backward kernel's expected values (tests/sweep_bwd_cases.py), checked on
the CPU without a GPU.

* The float64 scatter agrees with the reference's own autograd
  (tests/golden/sweep_grad.npz, scripts/gen_sweep_grad_golden.py) within the
  bar the GPU tests use: the reference itself stays inside the bar on the
  chosen inputs.  Measured: cost grad_tgt max |diff| 5.4e-7 against a floor
  (RMS) of 1.06; inverse_warp grad_feat 3.3e-7 against 0.58.
* The exact-lattice cases are exact: the oracle's float32 positions equal the
  intended integers or half-integers bit for bit, and the float64 scatter at
  them equals the closed form.  A case that is not exact is rejected here.
* The general-pose cases hold what they are there for: no sample within a
  float32 guard of the image border (where two float32 evaluation orders may
  decide differently), the roll's taps spread over most rows, some samples
  behind the camera, and nothing in range in the all-out case.  At their
  shapes the kernel's window is the whole image (asserted), so:
* The TALL and WIDE cases reach the rest of the kernel's launch shape (the
  restated bwd_geom and window_replay): chunks of 4 planes, a window of 10 of
  40 rows that 44 % of the row-taps leave, a last channel group of 4, and rows
  too long for any window.
"""
import pytest
import torch

from tests import sweep_bwd_cases as BC
from tests import sweep_pose_cases as PC


def _t(a):
    return torch.from_numpy(a)


def test_scatter_matches_reference_autograd(golden):
    z = golden("sweep_grad.npz")
    c = z["cost"]
    B, C, h, w = c["tgt"].shape
    L = int(c["nlabel"])
    assert (B, C, h, w, L) == (2, 8, 12, 16, 4) and not (c["pose"][0] == c["pose"][1]).all()
    case = BC.Case("golden", h, w, L, float(c["min_depth"]), False, _t(c["pose"]), _t(c["K4"]), _t(c["K4inv"]))
    g = _t(c["g"])
    want, inside = BC.expected_grad_tgt(case, g[:, C:])
    assert 0.5 < float(inside.float().mean()) < 1.0          # both in-range and zero samples
    ok, err, floor = BC.close(want, _t(c["grad_tgt"]))
    print({"cost_grad_tgt_max_err": err, "floor": floor})
    assert ok, (err, floor)
    ok, err, floor = BC.close(g[:, :C].double().sum(2), _t(c["grad_ref"]))
    assert ok, (err, floor)
    v = z["warp"]
    assert float(v["depth"].std()) > 0.5                      # a depth map, not a plane
    want = BC.expected_warp_grad(v["feat"].shape, _t(v["depth"]), _t(v["pose"]), _t(v["K"]), _t(v["Kinv"]), _t(v["g"]))
    ok, err, floor = BC.close(want, _t(v["grad_feat"]))
    print({"warp_grad_feat_max_err": err, "floor": floor})
    assert ok, (err, floor)


@pytest.mark.parametrize("kind", list(BC.LATTICE_SHIFTS))
@pytest.mark.parametrize("L", [1, 5])
def test_lattice_cases_are_exact(kind, L):
    case = BC.lattice_case(kind, L)
    h, w = case.h, case.w
    assert w - 1 == 16 and h - 1 == 8
    depths = PC.plane_depths(L, case.min_depth)
    assert torch.equal(depths, torch.tensor([12.0 * L / (i + 1) for i in range(L)]))      # integers
    inside, ix, iy = BC.oracle_positions(BC.plane_depth_maps(case), case.pose, case.K4, case.Ki4, h, w)
    px, py = BC.lattice_positions(kind, L)
    want_in = (px >= 0) & (px <= w - 1)
    assert torch.equal(inside.reshape(2, L, h, w), want_in)
    # bit for bit: the float32 positions are the intended integers / half-integers
    sel = want_in.reshape(2, L, h * w)
    assert torch.equal(ix[sel].double(), px.reshape(2, L, h * w)[sel])
    assert torch.equal(iy[sel].double(), py.reshape(2, L, h * w)[sel])
    assert torch.equal(ix[sel], px.reshape(2, L, h * w)[sel].float())
    if kind == "half":
        assert bool(((ix[sel] % 1) == 0.5).any())
    # the kernel's written-order arithmetic (warp.h restated on the CPU) gives the same bits
    K = case.K4.clone()
    sc = PC.Scene(case.name, h, w, None, None, case.pose, K, torch.inverse(K), case.K4, case.Ki4, case.min_depth)
    xn, yn = PC.written_order_coords(sc, L)
    wo_in = (xn <= 1) & (xn >= -1) & (yn <= 1) & (yn >= -1)
    assert torch.equal(wo_in, want_in)
    assert torch.equal((((xn + 1) / 2) * (w - 1))[want_in].double(), px[want_in])
    assert torch.equal((((yn + 1) / 2) * (h - 1))[want_in].double(), py[want_in])
    for C in (3, 32):
        g = BC.integer_g(2, C, L, h, w, seed=5 + C + L)
        got = BC.scatter64(g, inside, ix, iy, h, w)
        want = BC.lattice_expected(kind, g)
        assert torch.equal(got.float(), want) and torch.equal(got, want.double())
        if kind == "identity":
            assert torch.equal(want, g.sum(2))


@pytest.mark.parametrize("name", list(BC.GENERAL))
@pytest.mark.parametrize("h,w", BC.GENERAL_SHAPES)
def test_general_cases_hold_what_they_are_for(name, h, w):
    case = BC.general_case(name, h, w)
    L = case.L
    assert case.pose.shape[0] == 2
    K = case.K4.clone()
    K[:, :2, :] = K[:, :2, :] * 4
    sc = PC.Scene(case.name, h, w, None, None, case.pose, K, torch.inverse(K), case.K4, case.Ki4, case.min_depth)
    cls = PC.classify(sc, L)
    inside, ix, iy = BC.oracle_positions(BC.plane_depth_maps(case), case.pose, case.K4, case.Ki4, h, w)
    assert torch.equal(inside.reshape(2, L, h, w), cls.in32)
    if name == "all_out":
        assert int(inside.sum()) == 0 and bool(cls.sure_out.all())
        g = torch.randn(2, 4, L, h, w, generator=torch.Generator().manual_seed(1))
        assert not BC.scatter64(g, inside, ix, iy, h, w).any()
        return
    # no in-range decision hangs on float32 rounding
    assert int((cls.ambiguous & ~cls.sure_out).sum()) == 0, int(cls.ambiguous.sum())
    assert int(inside.sum()) > 0 and not bool(inside.all())
    if name == "partly_behind":
        assert int(cls.clamped.sum()) > 0 and int((~cls.clamped).sum()) > 0
        assert int((cls.clamped & cls.in32).sum()) == 0       # clamped samples leave the image: X / 1e-3
    # at these shapes the kernel's window is the whole image and a chunk one plane: nothing leaves the window
    n_in, n_out, q = BC.window_replay(case, BC.GENERAL_C)
    assert q.wr == h and q.lp == 1 and n_out == 0 and n_in > 0
    if name == "roll_90":
        # a reference row's taps land in one or two target columns, over many target rows
        for b in range(2):
            sel = inside[b, 0].reshape(h, w)
            rows = iy[b, 0].reshape(h, w)
            spans = [float(rows[y][sel[y]].max() - rows[y][sel[y]].min()) for y in range(h) if int(sel[y].sum()) > 1]
            assert spans and max(spans) >= min(h, w) - 2, spans


@pytest.mark.parametrize("spec", [BC.TALL, BC.WIDE], ids=lambda s: s["name"])
def test_shaped_cases_reach_the_window_paths(spec):
    case = BC.shaped_case(spec)
    B, C, h, w, L = case.pose.shape[0], spec["C"], case.h, case.w, case.L
    K = case.K4.clone()
    K[:, :2, :] = K[:, :2, :] * 4
    sc = PC.Scene(case.name, h, w, None, None, case.pose, K, torch.inverse(K), case.K4, case.Ki4, case.min_depth)
    cls = PC.classify(sc, L)
    assert int((cls.ambiguous & ~cls.sure_out).sum()) == 0      # no decision hangs on float32 rounding
    assert int((cls.clamped & cls.in32).sum()) == 0
    assert all(int(cls.in32[b].sum()) > 0 for b in range(B))
    n_in, n_out, q = BC.window_replay(case, C)
    print({"case": case.name, "geom": q, "row_taps_in_window": n_in, "row_taps_outside": n_out})
    assert C > 8 and C % 8 == 4                                  # a last channel group of 4
    if spec is BC.TALL:
        assert q.wr == 10 < h and q.rb == 8 and q.lp == 4 and q.nchunks == 13 and q.blocks >= 1024
        assert n_out > 0.4 * (n_in + n_out) and n_in > 0.4 * (n_in + n_out)
    else:
        assert q.wr == 0 and 8 * w * 4 > 32 * 1024 and n_in == 0 and n_out > 0
