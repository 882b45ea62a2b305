"""The five-point solver on the GPU (five_point.h; k_solve_front, k_roots /
k_roots_split, k_solve_back) against the oracle on the degenerate two-view
scenes of tests/solver_cases.py: zero motion, exact and noisy pure rotation,
planar scenes, an exactly representable grid, a sideways baseline, a large
rotation, scaled coordinates, collinear points, duplicated correspondences
and N = 5, 6, 8.  tests/test_solver_cases.py shows on the CPU that these reach
odd and full root counts, up to 10 cheirality candidates (every slot of hypE /
hypP) and the coincident-root end of the multi-root bisection.

Bar: exact.  Winner, inlier count, every hypothesis' score, root count and
candidate count, E and P byte for byte, and the inlier mask equal the
oracle's, with cheirality on and off; without cheirality also every
hypothesis' raw root count and the essential matrix of each of its roots
against the oracle's solve of the same five points (one documented exception,
the host's pow: _check_every_root).  Every solver form
(solve_coop 0, roots_split 0 and 1, solve_lanes 12, solve_coop 0 with
roots_split 0) gives the
default form's outputs and counts and leaves the same workspace: a differing
8-byte word passes only if it is a NaN in both runs (which NaN an operation on
NaN inputs returns is the compiler's choice per instantiation, as in
test_gpu_solve_coop.py), lies in the solve state's reduced-equation blocks or
determinant polynomial, and, outside the polynomial, belongs to a hypothesis
without a root (k_solve_back reads none of its blocks); anything else is
reported by field.  There is no cap on the number of such words.  The default
pruned launch, a ragged batch of six cases and a repeated run give the same
bits as well.

Measured on an MI355X (solve_coop = 0 against the default; the other forms
leave byte-identical workspaces): NaN words differ in the determinant
polynomial on most cases (3 per degenerate hypothesis; 258 on tiny_n5), and on
zero_motion, pure_rotation_exact and collinear also in rows of the equation
blocks (fields kStA + 9..14, 21..23, 30..32, up to 12 words per hypothesis:
12 / 57 / 12 words in 1 / 5 / 1 hypotheses): the reduction meets a zero pivot
although the five points are distinct.  The expectation that only the
polynomial fields would differ did not hold; every such hypothesis has no root.
"""
import numpy as np
import pytest
import torch

from oracle import ransac5 as R
from tests import solver_cases as SC

pytestmark = pytest.mark.gpu

FORMS = {
    "solve_coop=0": dict(solve_coop=0),
    "roots_split=0": dict(roots_split=0),
    "roots_split=1": dict(roots_split=1),
    "solve_lanes=12": dict(solve_lanes=12),
    "solve_coop=0,roots_split=0": dict(solve_coop=0, roots_split=0),
}
K_A, N_A, K_POLY, N_POLY, N_STATE = 36, 39, 95, 11, 116   # ransac_common.h: kStA (39 doubles), kStPoly (11), kStateFields
CASES = [(k, c) for k in SC.NAMES for c in (True, False)]
IDS = [f"{k}-{'cheir' if c else 'nocheir'}" for k, c in CASES]


def _regions(B, iters):
    """(name, first 8-byte word, words) of the workspace's fields: layout() of
    ransac_common.h for n_max = 0."""
    H = 512 * iters
    C = H * 10
    out, off = [], 0
    for name, nbytes in (("nroots", B * H * 4), ("ncand", B * H * 4), ("hypE", B * H * 90 * 8),
                         ("hypP", B * H * 120 * 8), ("hypP0", B * H * 12 * 8), ("sstate", N_STATE * B * H * 8),
                         ("cand_off", B * H * 4), ("chain_ref", B * H * 4), ("cand_total", 64 * 4),
                         ("candE", B * C * 18 * 8), ("cntT", B * C * 4), ("cntR", B * C * 4), ("cov", B * C * 8),
                         ("best_lb", 64 * 64 * 4), ("skipped", 8), ("score", B * H * 4), ("candF", B * C * 64 * 2),
                         ("claim", 72), ("cmap", B * C * 4), ("cmap2", B * C * 4), ("lead", 64 * 5 * 4),
                         ("bnd", 64 * 4 * 4)):
        words = ((nbytes + 255) & ~255) // 8
        out.append((name, off, words))
        off += words
    return out, off


def _field_of(word, B, iters):
    regs, _ = _regions(B, iters)
    for name, off, words in regs:
        if off <= word < off + words:
            if name == "sstate":
                return f"sstate[{(word - off) // (B * 512 * iters)}]"
            return name
    return "past the layout"


def _tuned(keys):
    """Context: set tuning keys, restore them in finally."""
    from sfm_amd import _lib

    class _T:
        def __enter__(self):
            self.prev = {k: _lib.tune_get(k) for k in keys}
            for k, v in keys.items():
                _lib.tune(k, v)

        def __exit__(self, *exc):
            for k, v in self.prev.items():
                _lib.tune(k, v)
    return _T()


def _launch(dev, pts, n, iters, cheir, tune=None, scores=True):
    """One ransac5_batched call on a zeroed caller-owned workspace."""
    from sfm_amd import _lib, ransac
    p = SC.THR, SC.SEED
    B = pts.shape[0]
    ws = ransac.workspace_for(B, iters, dev)
    assert ws.numel() == _regions(B, iters)[1] * 8
    ws.zero_()
    with _tuned(tune or {}):
        out = ransac.ransac5_batched(pts, n, None, None, iters, p[0], p[1], cheir, return_scores=scores, workspace=ws)
        torch.cuda.synchronize()
        scorer = _lib.last_scorer()
    nroots, ncand = ransac.hypothesis_counts(ws, B, iters)
    return dict(E=out[0], P=out[1], inliers=out[2], winner=out[3], scores=out[4] if scores else None,
                nroots=nroots, ncand=ncand, ws=ws, scorer=scorer)


_PTS, _DEFAULT = {}, {}


def _pts(dev, name):
    if name not in _PTS:
        q, qp, _ = SC.case(name)
        _PTS[name] = torch.from_numpy(np.c_[q, qp]).unsqueeze(0).contiguous().to(dev)
    return _PTS[name]


def _default(dev, name, cheir):
    """The default form's run with per-hypothesis scores (once per case)."""
    key = (name, cheir)
    if key not in _DEFAULT:
        _DEFAULT[key] = _launch(dev, _pts(dev, name), None, SC.case(name)[2]["iters"], cheir)
    return _DEFAULT[key]


def _same_outputs(a, b, what, scores=True):
    for k in ("winner", "inliers", "E", "P") + (("scores",) if scores else ()):
        if a[k] is None and b[k] is None:
            continue
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def _host_pow_correctly_rounded(v0):
    """Whether this host's pow(v0, -1/10), the oracle's root scaling, is the
    double nearest to the exact value (60 digits)."""
    import math
    from decimal import Decimal, localcontext
    with localcontext() as ctx:
        ctx.prec = 60
        got = math.pow(v0, -1.0 / 10)
        exact = Decimal(v0) ** Decimal(-1.0 / 10)
        err = abs(Decimal(got) - exact)
        return all(err <= abs(Decimal(float(np.nextafter(got, d))) - exact) for d in (-np.inf, np.inf))


def _check_every_root(r, name):
    """Without cheirality hypE holds the essential matrix of every root, in
    root order: each hypothesis' raw root count (negative ones included) and
    all 10 slots (zero past the count, the workspace starts zeroed) against
    the oracle's five-point solve of the same sample, bit for bit.

    One documented exception.  Polynomials with |c0 / c10| > 10 have their roots
    scaled by pow(|c0 / c10|, -1/10) (sturm.cu:570-590).  The device computes
    that power correctly rounded (cr_pow); the oracle calls the host's libm,
    which is within an ulp but not always the nearest double.  Where the host's
    value is demonstrably not the nearest one, the oracle's roots are not the
    specified ones and that hypothesis' matrices are not compared (its root
    count still is).  Measured: 1 of 11,264 hypotheses (half_duplicates, 470:
    the exact power lies 0.0004 ulp from the midpoint of two doubles; three
    roots differ by one ulp, E by 3.5e-16 relative)."""
    q, qp, p = SC.case(name)
    H, n = 512 * p["iters"], len(q)
    regs, _ = _regions(1, p["iters"])
    off = dict((k, o) for k, o, _ in regs)
    w = r["ws"].view(torch.float64).cpu().numpy()
    hypE = w[off["hypE"]: off["hypE"] + H * 90].reshape(H, 10, 9)
    poly = w[off["sstate"] + K_POLY * H: off["sstate"] + (K_POLY + N_POLY) * H].reshape(N_POLY, H)
    nroots = r["nroots"][0].numpy()
    excused = []
    for h in range(H):
        idx = [R.sample_index(p["seed"], h, d, n) for d in range(5)]
        s = R.solve5(q[idx], qp[idx], cheir=False)
        assert s["nroots"] == nroots[h], (name, h, s["nroots"], int(nroots[h]))
        if not np.array_equal(hypE[h], s["E_roots"], equal_nan=True):
            v0 = abs(poly[0, h] * (1.0 / poly[10, h]))          # real_roots_t: fabs(c0[0]) after normalisation
            assert v0 > 10.0 and not _host_pow_correctly_rounded(float(v0)), \
                f"{name}: hypothesis {h} ({s['nroots']} roots): the essential matrix of a root differs"
            excused.append(h)
    print(name, "hypotheses not compared (host pow not correctly rounded):", excused)
    assert len(excused) <= 2, excused        # about 1 scaled polynomial in 2,000 on a glibc host


@pytest.mark.parametrize("name,cheir", CASES, ids=IDS)
def test_solver_matches_oracle(cuda, name, cheir):
    from sfm_amd import ransac
    q, qp, p = SC.case(name)
    ref = SC.oracle(name, cheir)
    roots = SC.oracle(name, False)["hyp_ncand"]          # without cheirality hyp_ncand is the root count
    r = _default(cuda, name, cheir)
    win, inl = int(r["winner"][0]), int(r["inliers"][0])
    print(name, "cheirality", cheir, "winner", win, ref["winner"], "inliers", inl, ref["inliers"], "max candidates",
          int(r["ncand"].max()), "roots 0..10", np.bincount(r["nroots"][0].clamp(min=0).numpy(), minlength=11))
    assert win == ref["winner"] and inl == ref["inliers"]
    assert np.array_equal(r["scores"][0].cpu().numpy(), ref["hyp_score"])
    # the oracle reports a solve without a valid root (count <= 0) as 0 roots
    assert np.array_equal(r["nroots"][0].clamp(min=0).numpy(), roots)
    assert np.array_equal(r["ncand"][0].numpy(), ref["hyp_ncand"])
    E = r["E"][0].cpu().numpy()
    assert E.tobytes() == ref["E"].tobytes()
    if cheir:
        assert r["P"][0].cpu().numpy().tobytes() == ref["P"].tobytes()
    if ref["winner"] < 0:
        assert np.all(E == 0) and (not cheir or bool((r["P"] == 0).all()))
    if not cheir:
        _check_every_root(r, name)
    mask = ransac.inlier_mask(_pts(cuda, name), r["E"], p["thr"])[0].cpu().numpy()
    assert np.array_equal(mask, R.inlier_mask(ref["E"], q, qp, p["thr"]))
    assert int(mask.sum()) == ref["inliers"]


@pytest.mark.parametrize("name,cheir", CASES, ids=IDS)
def test_solver_forms_leave_the_same_workspace(cuda, name, cheir):
    iters = SC.case(name)[2]["iters"]
    base = _default(cuda, name, cheir)
    w0 = base["ws"].view(torch.int64)
    regs, _ = _regions(1, iters)
    s_off = dict((n, o) for n, o, _ in regs)["sstate"]
    H = 512 * iters
    poly = torch.zeros_like(w0, dtype=torch.bool)
    poly[s_off + K_POLY * H: s_off + (K_POLY + N_POLY) * H] = True
    state = poly.clone()
    state[s_off + K_A * H: s_off + (K_A + N_A) * H] = True
    for tag, keys in FORMS.items():
        r = _launch(cuda, _pts(cuda, name), None, iters, cheir, tune=keys)
        _same_outputs(base, r, tag)
        assert torch.equal(base["nroots"], r["nroots"]) and torch.equal(base["ncand"], r["ncand"]), tag
        w1 = r["ws"].view(torch.int64)
        diff = w0 != w1
        f0, f1 = base["ws"].view(torch.float64), r["ws"].view(torch.float64)
        finite = diff & ~(f0.isnan() & f1.isnan())
        bad = diff & ~state
        for what, m in (("differ and are not NaN in both runs", finite), ("differ outside the solve state's "
                        "equation blocks and determinant polynomial", bad)):
            if bool(m.any()):
                words = m.nonzero().flatten().tolist()
                raise AssertionError(f"{tag}: {len(words)} words {what}, in "
                                     f"{sorted({_field_of(w, 1, iters) for w in words})} (first words {words[:8]})")
        # a NaN outside the polynomial belongs to a hypothesis without a root: k_solve_back reads none of its blocks
        hyps = ((diff & ~poly).nonzero().flatten() - s_off) % H
        assert bool((base["nroots"][0][hyps.cpu()] <= 0).all()), f"{tag}: NaN blocks differ in a hypothesis with roots"
        print(name, tag, "NaN words that differ: determinant polynomial", int((diff & poly).sum()),
              "equation blocks", int((diff & ~poly).sum()), "in", int(hyps.unique().numel()), "hypotheses")


@pytest.mark.parametrize("name,cheir", CASES, ids=IDS)
def test_default_pruned_launch(cuda, name, cheir):
    """No per-hypothesis scores: the launch every pipeline makes.  On the
    tie-saturated cases hundreds of hypotheses share the score N, so k_select's
    first-maximum key and the pruned scorer decide among equals."""
    iters = SC.case(name)[2]["iters"]
    base = _default(cuda, name, cheir)
    r = _launch(cuda, _pts(cuda, name), None, iters, cheir, scores=False)
    if name in SC.TIE_SATURATED:
        n = len(SC.case(name)[0])
        assert int((base["scores"][0] == n).sum()) >= 100, "not tie-saturated"
    for k in ("winner", "inliers", "E", "P"):
        if base[k] is not None:
            assert torch.equal(base[k], r[k]), f"{k} differs under scorer {r['scorer']} (scores: {base['scorer']})"


@pytest.mark.parametrize("cheir", [True, False], ids=["cheir", "nocheir"])
def test_ragged_batch_equals_single_calls(cuda, cheir):
    """Six cases with different N in one call: degenerate hypotheses of one
    pair share waves and the roots_split = 2 pool with their neighbours'."""
    pts, n, p, names = SC.ragged()
    it = p["iters"]
    r = _launch(cuda, torch.from_numpy(pts).to(cuda), n, it, cheir)
    for b, k in enumerate(names):
        s = _launch(cuda, _pts(cuda, k), None, it, cheir)
        ref = SC.oracle(k, cheir, iters=it)
        assert int(s["winner"][0]) == ref["winner"] and np.array_equal(s["scores"][0].cpu().numpy(), ref["hyp_score"])
        for f in ("winner", "inliers", "E", "P", "scores", "nroots", "ncand"):
            if s[f] is not None:
                assert torch.equal(r[f][b].cpu(), s[f][0].cpu()), (k, f)


def test_repeatable(cuda):
    a = _launch(cuda, _pts(cuda, "pure_rotation_exact"), None, SC.case("pure_rotation_exact")[2]["iters"], True)
    b = _launch(cuda, _pts(cuda, "pure_rotation_exact"), None, SC.case("pure_rotation_exact")[2]["iters"], True)
    assert torch.equal(a["ws"], b["ws"])
    _same_outputs(a, b, "second run")
