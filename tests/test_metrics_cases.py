"""The depth-metrics cases of tests/metrics_cases.py, checked on the CPU: the
numpy reference against the reference fixture and the host specification, and
every case is what it claims (bin edges, signs, ties, bins per wave, mask and
rectangle edges)."""
import numpy as np
import pytest
import torch

from tests import metrics_cases as MC
from test_validate import CASES as GOLDEN_CASES, case_inputs, check_exact_slots


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in MC.all_cases()}


def _host(case):
    from sfm_amd import validate as V
    rs = None if case.rescale is None else torch.from_numpy(case.rescale)
    rows, depth = V.depth_metric_rows_host(torch.from_numpy(case.pred), torch.from_numpy(case.gt), rs, case.mode,
                                           case.min_depth, case.nlabel, return_depth=True)
    return rows.numpy(), depth.numpy()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_reference_matches_fixture_and_host(golden, name):
    from sfm_amd import validate as V
    c = golden("metrics.npz")[name]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    rect = V.eigen_crop(*gt.shape[1:]) if dataset == "kitti" else None
    want = MC.ref_rows(pred.numpy(), gt.numpy(), None if rescale is None else rescale.numpy(), dataset, rect,
                       min_depth, nlabel)
    check_exact_slots(want[0], want[1], c)
    host, hdepth = V.depth_metric_rows_host(pred, gt, rescale, dataset, min_depth, nlabel, return_depth=True)
    MC.check_rows(host.numpy(), hdepth.numpy(), want, name)
    for k in MC.EXACT_SLOTS:
        assert MC.same_or_both_nan(host.numpy()[:, k], want[0][:, k]), k


def test_host_specification_agrees_on_every_wrapper_case(cases):
    """torch's median (the host specification) against np.sort(x)[(n - 1) // 2] on every case that the wrapper's
    own rectangle can express."""
    for c in cases.values():
        if c.via != "wrapper" and not (c.mode == "demon"):
            continue
        rows, depth = _host(c)
        MC.check_rows(rows, depth, MC.expected(c), c.name)


def test_no_zero_among_the_selected_values(cases):
    for c in cases.values():
        for b in range(c.gt.shape[0]):
            g, p = MC.selected(c, b)
            assert not (g == 0).any() and not (p == 0).any(), (c.name, b)


def test_key_is_order_preserving_and_invertible():
    x = np.array([-np.inf, -3.5, -1e-40, 1e-41, 0.5, 2.0, np.inf], np.float32)
    k = MC.order_key(x)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(MC.key_value(k).view(np.uint32), x.view(np.uint32))
    assert (k[:3] >> 31 == 0).all() and (k[3:] >> 31 == 1).all()


def test_sizes(cases):
    shapes = {n: cases[n].gt.shape[1:] for n in ("size_1x1", "size_64x64", "size_1x4097", "size_3chunks+1")}
    assert shapes == {"size_1x1": (1, 1), "size_64x64": (64, 64), "size_1x4097": (1, 4097),
                      "size_3chunks+1": (1, 3 * 4096 + 1)}
    n = {name: MC.expected(cases[name])[0][:, 0].tolist() for name in shapes}
    assert n == {"size_1x1": [1, 0], "size_64x64": [4096, 1, 2], "size_1x4097": [3, 4097, 1],
                 "size_3chunks+1": [12289, 1, 2]}
    for name, b, first in (("size_1x4097", 2, 4096), ("size_3chunks+1", 1, 12288)):
        m = MC.mask_of(cases[name].gt[b], "demon", None).ravel()
        assert m.nonzero()[0].tolist() == [first]
    assert max(c.gt.shape[1] * c.gt.shape[2] for c in cases.values()) == 3 * 4096 + 1


@pytest.mark.parametrize("side", ["last", "first"])
def test_medians_straddle_their_bin_edges(cases, side):
    c = cases[f"edges_{side}"]
    for b, kind in enumerate(MC.EDGE_KEYS):
        sh = MC.EDGE_SHIFT[kind]
        for which, vals in enumerate(MC.selected(c, b)):
            ks = np.sort(MC.order_key(vals)).astype(np.int64)
            m = (ks.size - 1) // 2
            edge = MC.EDGE_KEYS[kind][which]
            lo, hi = (m, m + 1) if side == "last" else (m - 1, m)
            assert ks[lo] == edge - 1 and ks[hi] == edge, (kind, which, hex(ks[lo]), hex(ks[hi]))
            assert (ks[lo] >> sh) + 1 == (ks[hi] >> sh)                         # neighbouring bins of this digit
            if sh:
                assert ks[hi] & ((1 << sh) - 1) == 0 and ks[lo] & ((1 << sh) - 1) == (1 << sh) - 1
            if kind != "top":                                                   # the digits above agree
                up = 21 if kind == "mid" else 10
                assert ks[lo] >> up == ks[hi] >> up
            assert ks[lo - 1] == ks[lo] - 1 and ks[hi + 1] == ks[hi] + 1        # a neighbour inside each bin too
            assert np.array_equal(MC.key_value(ks[m].astype(np.uint32)).view(np.uint32),
                                  np.float32(MC.lower_median(vals)).view(np.uint32).reshape(()))
    # p0 runs among the negative floats in the middle and low pairs
    assert (MC.selected(c, 1)[1] < 0).all() and (MC.selected(c, 2)[1] < 0).all() and (MC.selected(c, 0)[1] > 0).all()


def test_sign_cases(cases):
    c = cases["sign"]
    rows = MC.expected(c)[0]
    assert (MC.selected(c, 0)[1] < 0).all() and rows[0, 2] < 0 and rows[0, 3] < 0
    p1 = MC.selected(c, 1)[1]
    assert (p1 < 0).any() and (p1 > 0).any() and rows[1, 2] < 0
    p2 = MC.selected(c, 2)[1]
    assert rows[2, 2] == p2[p2 > 0].min() and (p2 < 0).sum() == 200
    p3 = MC.selected(c, 3)[1]
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(p3) < tiny) & (p3 > 0)).any() and ((np.abs(p3) < tiny) & (p3 < 0)).any()
    assert (p3 == np.inf).any() and (p3 == -np.inf).any() and np.isfinite(rows[3, 2]) and rows[3, 2] > tiny
    assert np.isfinite(rows[:, 4:13]).all()
    f = cases["sign_fallback"]
    fr = MC.expected(f)[0]
    assert fr[0, 0] > 0 and fr[1, 0] == 0 and fr[1, 1] < 0 and (f.gt[1] < 0).all()


def test_ties(cases):
    c = cases["ties"]
    assert np.unique(c.gt[0]).size == 30 and np.array_equal(c.gt[0] * 256, np.round(c.gt[0] * 256))
    assert np.unique(c.pred[0]).size == 1 and np.array_equal(c.pred[1], c.gt[1])
    rows = MC.expected(c)[0]
    assert rows[1, 3] == 1.0 and np.array_equal(rows[1, 4:9], np.zeros(5)) and rows[1, 9] == c.gt[1].size


def test_wide_range_fills_more_than_six_bins_per_wave(cases):
    c = cases["wide_range"]
    for b in range(2):
        m = MC.mask_of(c.gt[b], "demon", None)
        assert m.all()
        assert MC.distinct_top_bins_per_wave(c.gt[b], m) > 6
        assert MC.distinct_top_bins_per_wave(c.pred[b], m) > 6
    p = np.abs(c.pred)
    assert p.min() < 2.0 ** -19 and p.max() > 2.0 ** 19
    # the fixture-like cases stay within the aggregated rounds somewhere: the two paths are both taken in the suite
    assert MC.distinct_top_bins_per_wave(np.full((1, 64), 2.0, np.float32), np.ones((1, 64), bool)) == 1


def test_nan_case(cases):
    c = cases["nan_pred"]
    rows, depth, _ = MC.expected(c)
    assert np.isfinite(rows[0]).all()
    assert rows[1, 0] == 300 and np.isfinite(rows[1, 1]) and np.isnan(rows[1, 2]) and np.isnan(rows[1, 3])
    assert np.isnan(rows[1, [4, 5, 6, 7, 8, 12]]).all() and np.array_equal(rows[1, 9:12], np.zeros(3))
    assert np.isnan(depth[1]).all() and not np.isnan(depth[0]).any()


def test_mask_and_rectangle_edges(cases):
    c = cases["demon_edges"]
    g = c.gt[0]
    m = MC.mask_of(g, "demon", None)
    assert m[g == np.float32(0.5)].all() and m[g == np.float32(10)].all() and (g == np.float32(0.5)).sum() == 2
    out = (g < np.float32(0.5)) | ((g > np.float32(10)) & (g < np.float32(10.1)))
    assert out.sum() == 4 and not m[out].any() and np.isnan(c.pred[0][out]).all()
    assert np.isfinite(MC.expected(c)[0]).all() and MC.expected(c)[0][0, 0] == 204
    k = cases["kitti_rect"]
    y0, y1, x0, x1 = k.rect
    m = MC.mask_of(k.gt[0], "kitti", k.rect)
    assert m[y0, x0] and m[y0, x1 - 1] and m[y1 - 1, x0] and m[y1 - 1, x1 - 1]
    assert not m[y0 - 1].any() and not m[y1].any() and not m[:, x0 - 1].any() and not m[:, x1].any()
    assert np.isnan(k.pred[0][y0 - 1]).all() and np.isnan(k.pred[0][y1]).all()
    assert np.isnan(k.pred[0][:, x0 - 1]).all() and np.isnan(k.pred[0][:, x1]).all()
    zero_or_80 = (k.gt[0] == 0) | (k.gt[0] == 80)
    assert zero_or_80.sum() == 4 and not m[zero_or_80].any() and np.isnan(k.pred[0][zero_or_80]).all()
    rows = MC.expected(k)[0]
    assert rows[0, 0] == (y1 - y0) * (x1 - x0) - 4 and np.isfinite(rows[0]).all()
    assert rows[1, 0] == 0 and rows[1, 1] == 90.0 and (k.gt[1] < 0).any()
    e = cases["empty_rect"]
    assert e.rect[0] == e.rect[1] and np.array_equal(MC.expected(e)[0][:, 0], np.zeros(2))
    assert np.isfinite(MC.expected(e)[0][:, 1:4]).all()


def test_strided_buffer(cases):
    c = cases["strided"]
    buf, bs, rs = MC.padded_pred(c)
    B, H, W = c.pred.shape
    assert rs == W + 5 and bs > H * rs and H * W > 4096
    assert np.isnan(buf).sum() == buf.size - B * H * W
    for b in range(B):
        assert np.array_equal(buf[b * bs:b * bs + H * rs].reshape(H, rs)[:, :W], c.pred[b])


def test_check_rows_refuses_a_neighbouring_key_and_a_dropped_pixel(cases):
    c = cases["edges_last"]
    want = MC.expected(c)
    MC.check_rows(want[0], want[1], want)
    bad = want[0].copy()
    bad[0, 1] = MC.key_value(MC.order_key(np.float32(bad[0, 1])) + np.uint32(1))[0]
    with pytest.raises(AssertionError):
        MC.check_rows(bad, want[1], want)
    bad = want[0].copy()
    bad[1, 8] += 2e-10 * want[2][1, 8]
    with pytest.raises(AssertionError):
        MC.check_rows(bad, want[1], want)
