"""Edge cases for sfm_depth_metrics (csrc/metrics.hip) with a numpy restatement
of the row contract (tests/test_metrics_cases.py checks both on the CPU,
tests/test_gpu_metrics_edges.py runs the kernels against them).

Reference.  ``ref_rows`` restates sfm_amd/validate.py's row (slots in that
module's docstring) in numpy with an explicit mask mode and crop rectangle.
The lower median is np.sort(x)[(n - 1) // 2], NaN if any selected value is
NaN.  Beside the row it returns, per slot, the sum of the absolute terms: the
sums 4-8 and 12 are compared within 1e-10 of that (for slot 8, sum l, which
cancels after median scaling, it is the measure that stays meaningful near
zero; for the others it is the sum itself).

+0 and -0 compare equal, so which of them a median returns is unspecified (in
torch as well): no case has a zero of either sign among its selected values.

A radix-select key is the kernel's order-preserving u32 of a float32
(``order_key``: sign bit set -> ~u, else u | 2^31); its three digits are bits
31..21, 20..10 and 9..0.

Batches (every pair of a batch has the batch's H x W; DeMoN mask 0.5 <= gt <=
10 unless said; ``via`` says whether the test drives depth_metric_rows or the
C ABI with a rectangle and strides of its own):

  size_1x1        n = 1; no masked pixel (whole-image fallback over one pixel)
  size_64x64      exactly one chunk: all pixels; n = 1; n = 2
  size_1x4097     one chunk and one pixel: n = 3; all pixels; only the pixel of the second chunk
  size_3chunks+1  1 x 12289: all pixels; only the pixel of the fourth chunk; n = 2 in chunks 0 and 3
  edges_last      the median is the last key of a top / middle / low digit bin, its upper neighbour the first of the next
  edges_first     the median is the first key of a bin, its lower neighbour the last of the bin before
                  (gt and p0 each at edges of their own; p0 among negative keys in the middle and low pairs)
  sign            negative rescale; mixed signs with a negative median; the median the smallest positive value
                  next to negatives; subnormals and +-inf around a finite median
  sign_fallback   KITTI: an ordinary pair beside one whose gt is negative everywhere (fallback, negative med_gt)
  ties            gt in 30 multiples of 1/256: pred constant; pred == gt
  wide_range      gt log-uniform over the mask, pred over 2^-20 .. 2^20: more than six top-digit bins per wave
  nan_pred        a NaN prediction at a masked pixel, beside an ordinary pair
  demon_edges     gt exactly 0.5 and 10 inside, their float32 neighbours outside (NaN predictions there)
  kitti_rect      C ABI: gt 0 and 80 outside; the rectangle's first and last rows and columns inside, the
                  ring around it outside (NaN predictions there); a pair without a masked pixel beside it
  empty_rect      C ABI: y0 == y1: every pair takes the whole-image fallback
  strided         C ABI: pred rows W + 5 apart, batch stride with slack, NaN padding
"""
from collections import namedtuple

import numpy as np

ROW_WIDTH = 16
EXACT_SLOTS = (0, 1, 2, 3, 9, 10, 11, 13, 14, 15)
SUM_SLOTS = (4, 5, 6, 7, 8, 12)
SUM_RTOL = 1e-10
CHUNK = 4096

Case = namedtuple("Case", "name mode rect pred gt rescale min_depth nlabel via")


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def order_key(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def lower_median(x):
    x = np.asarray(x, np.float32).ravel()
    if np.isnan(x).any():
        return np.float32("nan")
    return np.sort(x)[(x.size - 1) // 2]


def mask_of(gt, mode, rect):
    """[H, W] bool: DeMoN 0.5 <= gt <= 10; KITTI 0 < gt < 80 inside rows y0 .. y1 - 1, columns x0 .. x1 - 1."""
    if mode == "demon":
        return (gt >= np.float32(0.5)) & (gt <= np.float32(10))
    y0, y1, x0, x1 = rect
    m = np.zeros(gt.shape, bool)
    m[y0:y1, x0:x1] = True
    return m & (gt > 0) & (gt < np.float32(80))


def case_rect(case):
    """The rectangle a KITTI case runs with: its own, or the Eigen crop the wrapper passes."""
    if case.mode == "demon":
        return None
    if case.rect is not None:
        return case.rect
    from sfm_amd.validate import eigen_crop
    return eigen_crop(*case.gt.shape[1:])


def ref_rows(pred, gt, rescale, mode, rect, min_depth, nlabel):
    """(rows [B, 16] float64, depth [B, H, W] float32, abs_sums [B, 16]) of the row contract."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    B = gt.shape[0]
    lo, hi = np.float32(min_depth), np.float32(min_depth * nlabel)
    rows, mags = np.zeros((B, ROW_WIDTH)), np.zeros((B, ROW_WIDTH))
    depth = np.empty_like(gt)
    with np.errstate(all="ignore"):
        for b in range(B):
            p0 = pred[b] if rescale is None else pred[b] * np.float32(rescale[b])
            m = mask_of(gt[b], mode, rect)
            n = int(m.sum())
            sel = m if n else np.ones_like(m)
            med_gt, med_p = lower_median(gt[b][sel]), lower_median(p0[sel])
            scale = np.float32(med_gt) / np.float32(med_p)
            p = p0 * scale
            p = np.where(p <= lo, lo, p)
            p = np.where(p > hi, hi, p).astype(np.float32)
            depth[b] = p
            g, q = gt[b][m], p[m]
            d = g - q
            dd = d * d
            l = np.log(g.astype(np.float64)) - np.log(q.astype(np.float64))
            q0, q1 = g / q, q / g
            terms = {4: (np.abs(d) / g).astype(np.float64), 5: (dd / g).astype(np.float64), 6: dd.astype(np.float64),
                     7: l * l, 8: l, 12: np.abs(np.float32(1) / g - np.float32(1) / q).astype(np.float64)}
            rows[b, :4] = n, med_gt, med_p, scale
            for k, t in terms.items():
                rows[b, k] = t.sum()
                mags[b, k] = np.abs(t).sum()
            for k, t in enumerate((1.25, 1.5625, 1.953125)):
                rows[b, 9 + k] = np.count_nonzero((q0 < np.float32(t)) & (q1 < np.float32(t)))
    return rows, depth, mags


def expected(case):
    return ref_rows(case.pred, case.gt, case.rescale, case.mode, case_rect(case), case.min_depth, case.nlabel)


def same_or_both_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_bits_or_both_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def check_rows(rows, depth, want, what=""):
    """rows / depth (the kernel's, or the host specification's) against ref_rows' triple."""
    rows = np.asarray(rows, np.float64)
    wrows, wdepth, mags = want
    assert rows.shape == wrows.shape, (what, rows.shape)
    for k in EXACT_SLOTS:
        assert same_or_both_nan(rows[:, k], wrows[:, k]), (what, "slot", k, rows[:, k], wrows[:, k])
    for k in (1, 2, 3):
        assert same_bits_or_both_nan(rows[:, k].astype(np.float32), wrows[:, k].astype(np.float32)), (what, k)
    for k in SUM_SLOTS:
        for b in range(rows.shape[0]):
            g, w = rows[b, k], wrows[b, k]
            if np.isnan(w) or np.isinf(w):
                assert same_or_both_nan(g, w), (what, b, k, g, w)
            else:
                assert abs(g - w) <= SUM_RTOL * mags[b, k], (what, b, k, g, w, mags[b, k])
    if depth is not None:
        assert same_bits_or_both_nan(depth, wdepth), (what, "depth")


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
OFF_GT, OFF_PRED = np.float32(20.0), np.float32(1.0)      # an unmasked pixel (DeMoN): gt out of range


def _plain(rng, n, spread=0.2):
    """n ordinary (gt, pred): gt log-uniform over the DeMoN mask, pred = 1.7 gt lognormal."""
    gt = np.exp(rng.uniform(np.log(0.6), np.log(9.0), n)).astype(np.float32)
    pred = (1.7 * gt * np.exp(spread * rng.standard_normal(n))).astype(np.float32)
    return gt, pred


def place(H, W, gt_sel, pred_sel, where=None, seed=0, off_pred=OFF_PRED):
    """One [H, W] pair: the selected values at ``where`` (flat pixel indices; a
    seeded choice if None), every other pixel outside the DeMoN mask."""
    gt_sel, pred_sel = np.asarray(gt_sel, np.float32), np.asarray(pred_sel, np.float32)
    n = gt_sel.size
    if where is None:
        where = np.sort(np.random.default_rng(seed).choice(H * W, n, replace=False))
    gt = np.full(H * W, OFF_GT, np.float32)
    pred = np.full(H * W, off_pred, np.float32)
    gt[where], pred[where] = gt_sel, pred_sel
    return gt.reshape(H, W), pred.reshape(H, W)


def _case(name, pairs, mode="demon", rect=None, rescale=None, min_depth=1.0, nlabel=64, via="wrapper"):
    gt = np.stack([p[0] for p in pairs])
    pred = np.stack([p[1] for p in pairs])
    rs = None if rescale is None else np.asarray(rescale, np.float32)
    return Case(name, mode, rect, pred, gt, rs, min_depth, nlabel, via)


def sizes():
    rng = np.random.default_rng(11)
    out = []
    out.append(_case("size_1x1", [place(1, 1, [2.0], [3.0]), place(1, 1, [], [], off_pred=np.float32(5.0))]))
    g, p = _plain(rng, 4096)
    out.append(_case("size_64x64", [place(64, 64, g, p), place(64, 64, g[:1], p[:1], seed=1),
                                    place(64, 64, g[:2], p[:2], seed=2)]))
    g2, p2 = _plain(rng, 4097)
    out.append(_case("size_1x4097", [place(1, 4097, g2[:3], p2[:3], seed=3), place(1, 4097, g2, p2),
                                     place(1, 4097, g2[:1], p2[:1], where=[4096])]))
    g3, p3 = _plain(rng, 3 * CHUNK + 1)
    out.append(_case("size_3chunks+1", [place(1, 12289, g3, p3), place(1, 12289, g3[:1], p3[:1], where=[12288]),
                                        place(1, 12289, g3[:2], p3[:2], where=[5, 12288])]))
    return out


# edges of the three digits, as keys (the first key of a bin): for gt inside the DeMoN mask; for p0 among the
# positive floats (top) and among the negative ones (middle, low)
EDGE_KEYS = {
    "top": (0xC0000000, 0xC1000000),                                          # gt 2.0, p0 8.0
    "mid": (0xC0200000 | (0x155 << 10), 0x3F000000 | (0x2AA << 10)),
    "low": (0xC0200000 | (0x155 << 10) | 0x2A7, 0x3F000000 | (0x2AA << 10) | 0x158),
}
EDGE_SHIFT = {"top": 21, "mid": 10, "low": 0}


def _edge_keys(edge, n_low, n_high, rng, lo_key, hi_key):
    """n_low keys under ``edge`` (edge - 1 and edge - 2 among them) and n_high from it up (edge, edge + 1 among them)."""
    lows = np.concatenate([[edge - 1, edge - 2], rng.integers(lo_key, edge - (1 << 16), n_low - 2)])
    highs = np.concatenate([[edge, edge + 1], rng.integers(edge + (1 << 16), hi_key, n_high - 2)])
    return np.concatenate([lows, highs]).astype(np.uint32)


def edge_pair(kind, side, seed):
    """One 12 x 25 pair whose gt and p0 medians sit at a bin edge of digit
    ``kind``: side "last": 128 keys below the edge and 128 from it up, the
    lower median is edge - 1; side "first": 128 below and 129 from it up, the
    median is the edge itself."""
    rng = np.random.default_rng(seed)
    n_low, n_high = 128, 128 if side == "last" else 129
    eg, ep = EDGE_KEYS[kind]
    kg = _edge_keys(eg, n_low, n_high, rng, 0xBF000000, 0xC1200000)
    kp = _edge_keys(ep, n_low, n_high, rng, ep - (1 << 24), ep + (1 << 24))
    return place(12, 25, key_value(rng.permutation(kg)), key_value(rng.permutation(kp)), seed=seed)


def edges():
    return [_case(f"edges_{side}", [edge_pair(kind, side, 40 + 3 * i + j) for j, kind in enumerate(EDGE_KEYS)])
            for i, side in enumerate(("last", "first"))]


def signs():
    rng = np.random.default_rng(21)
    H, W = 20, 33
    g, p = _plain(rng, 400)
    neg_rescale = place(H, W, g, p, seed=1)
    mixed = p.copy()
    mixed[:260] *= -1                                   # 260 negatives of 400: a negative median
    neg_median = place(H, W, g, rng.permutation(mixed), seed=2)
    g3, p3 = _plain(rng, 401)
    small_pos = p3.copy()
    small_pos[:200] *= -1                               # 200 negatives, 201 positives: rank 200 is the smallest positive
    smallest_positive = place(H, W, g3, rng.permutation(small_pos), seed=3)
    odd = p3.copy()
    odd[:60] = np.float32(1e-40) * np.arange(1, 61, dtype=np.float32)          # subnormals
    odd[60:100] = -np.float32(1e-41) * np.arange(1, 41, dtype=np.float32)
    odd[100:130] = np.float32("inf")
    odd[130:150] = -np.float32("inf")
    oddities = place(H, W, g3, rng.permutation(odd), seed=4)
    a = _case("sign", [neg_rescale, neg_median, smallest_positive, oddities], rescale=[-0.75, 1.5, 1.0, 2.0])
    # KITTI through the wrapper (Eigen crop): an ordinary pair beside a pair whose gt is negative everywhere
    H, W = 24, 40
    gk = np.exp(rng.uniform(np.log(1.0), np.log(70.0), (H, W))).astype(np.float32)
    pk = (0.6 * gk * np.exp(0.2 * rng.standard_normal((H, W)))).astype(np.float32)
    gneg = -np.exp(rng.uniform(np.log(0.01), np.log(100.0), (H, W))).astype(np.float32)
    pmix = (pk * np.where(rng.random((H, W)) < 0.7, -1, 1)).astype(np.float32)
    b = _case("sign_fallback", [(gk, pk), (gneg, pmix)], mode="kitti")
    return [a, b]


def ties():
    rng = np.random.default_rng(31)
    H, W = 64, 65
    g = (1 + rng.integers(0, 30, H * W) / 256).astype(np.float32).reshape(H, W)
    return [_case("ties", [(g, np.full((H, W), 3.0, np.float32)), (g, g.copy())])]


def wide_range():
    rng = np.random.default_rng(41)
    H, W = 40, 120
    g = np.exp(rng.uniform(np.log(0.5), np.log(10.0), (2, H, W))).astype(np.float32)
    p = np.exp2(rng.uniform(-20, 20, (2, H, W))).astype(np.float32)
    p[1] *= np.where(rng.random((H, W)) < 0.5, -1, 1).astype(np.float32)
    return [_case("wide_range", [(g[0], p[0]), (g[1], p[1])])]


def distinct_top_bins_per_wave(x, sel):
    """For every aligned run of 64 pixels (what one wave loads at a time): the
    number of distinct top-digit bins among its selected values; the smallest."""
    k = (order_key(x.ravel()) >> 21).astype(np.int64)
    sel = sel.ravel()
    counts = []
    for s in range(0, k.size, 64):
        kk = k[s:s + 64][sel[s:s + 64]]
        if kk.size:
            counts.append(np.unique(kk).size)
    return min(counts)


def nan_pred():
    rng = np.random.default_rng(51)
    g, p = _plain(rng, 300)
    ok = place(15, 31, g, p, seed=1)
    bad_p = p.copy()
    bad_p[137] = np.float32("nan")
    return [_case("nan_pred", [ok, place(15, 31, g, bad_p, seed=2)])]


def demon_edges():
    rng = np.random.default_rng(61)
    g, p = _plain(rng, 200)
    nan = np.float32("nan")
    below, above = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(10), np.float32(20))
    g = np.concatenate([g, [0.5, 10.0, 0.5, 10.0], [below, above, below, above]]).astype(np.float32)
    p = np.concatenate([p, [0.9, 17.0, 1.1, 15.0], [nan, nan, nan, nan]]).astype(np.float32)
    order = rng.permutation(g.size)
    return [_case("demon_edges", [place(13, 29, g[order], p[order], seed=1), place(13, 29, g[:200], p[:200], seed=2)])]


KITTI_RECT = (3, 9, 4, 15)


def kitti_rect():
    rng = np.random.default_rng(71)
    H, W = 12, 20
    y0, y1, x0, x1 = KITTI_RECT
    g = np.exp(rng.uniform(np.log(1.0), np.log(70.0), (H, W))).astype(np.float32)
    p = (0.6 * g * np.exp(0.2 * rng.standard_normal((H, W)))).astype(np.float32)
    inside = np.zeros((H, W), bool)
    inside[y0:y1, x0:x1] = True
    p[~inside] = np.nan                                  # the ring around the rectangle and all beyond it
    g[4, 6], g[7, 13], g[y0, x0 + 1], g[y1 - 1, x1 - 2] = 0.0, 80.0, 80.0, 0.0
    for yx in ((4, 6), (7, 13), (y0, x0 + 1), (y1 - 1, x1 - 2)):
        p[yx] = np.nan
    g2 = np.full((H, W), 90.0, np.float32)               # no masked pixel: whole-image fallback
    g2[0, :] = -3.0
    p2 = (0.5 + rng.random((H, W))).astype(np.float32)
    return [_case("kitti_rect", [(g, p), (g2, p2)], mode="kitti", rect=KITTI_RECT, via="abi")]


def empty_rect():
    rng = np.random.default_rng(81)
    H, W = 12, 20
    g = np.exp(rng.uniform(np.log(1.0), np.log(70.0), (2, H, W))).astype(np.float32)
    p = (0.6 * g * np.exp(0.2 * rng.standard_normal((2, H, W)))).astype(np.float32)
    return [_case("empty_rect", [(g[0], p[0]), (g[1], p[1])], mode="kitti", rect=(5, 5, 2, 17), via="abi")]


def strided():
    rng = np.random.default_rng(91)
    H, W = 66, 63                                        # 4158 pixels: a chunk and 62
    g = np.exp(rng.uniform(np.log(0.3), np.log(12.0), (3, H, W))).astype(np.float32)
    p = (1.3 * g * np.exp(0.3 * rng.standard_normal((3, H, W)))).astype(np.float32)
    return [_case("strided", [(g[b], p[b]) for b in range(3)], rescale=[1.0, 0.5, 2.0], via="abi")]


def padded_pred(case, row_pad=5, batch_slack=7):
    """(flat float32 buffer, batch stride, row stride): the case's pred with rows W + row_pad apart and
    batch_slack further elements between pairs, every element outside the image NaN."""
    B, H, W = case.pred.shape
    rs = W + row_pad
    bs = H * rs + batch_slack
    buf = np.full(B * bs, np.nan, np.float32)
    for b in range(B):
        buf[b * bs:b * bs + H * rs].reshape(H, rs)[:, :W] = case.pred[b]
    return buf, bs, rs


def all_cases():
    out = (sizes() + edges() + signs() + ties() + wide_range() + nan_pred() + demon_edges() + kitti_rect()
           + empty_rect() + strided())
    assert len({c.name for c in out}) == len(out)
    return out


def selected(case, b):
    """(gt values, p0 values) the medians of pair b run over."""
    m = mask_of(case.gt[b], case.mode, case_rect(case))
    sel = m if m.any() else np.ones_like(m)
    p0 = case.pred[b] if case.rescale is None else case.pred[b] * np.float32(case.rescale[b])
    return case.gt[b][sel], p0[sel]
