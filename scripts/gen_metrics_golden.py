#!/usr/bin/env python
"""Generate tests/golden/metrics.npz: inputs and the reference's own results
for the validation depth metrics (sfm_amd/validate.py, csrc/metrics.hip).

    python scripts/gen_metrics_golden.py --reference <checkout of the reference>

Runs where the reference's sources are at hand (the build container), never
in a test.  ``evaluate_metric`` is taken out of the reference's main.py by
``ast`` (main.py itself cannot be imported without its training stack) and
``l1_inverse`` / ``scale_invariant`` come from its demon_metrics.py, imported
with a stand-in ``minieigen`` module (not installed; neither function uses
it).  Mask, median scale and clamp are applied with torch on the CPU in the
order of main.py:565-590.  Only data is written.

Cases (the smallest shapes at which the kernel can still go wrong):
  a  3 x 37 x 123 KITTI, pred a view into 3 x 128 x 128, values quantised to
     1/64 (median ties), one pair with even n and one with odd n, a rescale
     factor, predictions below min_depth and above max_depth
  b  2 x 37 x 123 KITTI, the second pair's mask empty (all gt >= 80)
  c  2 x 48 x 64 DeMoN with NaN and out-of-range gt
  d  2 x 96 x 320 KITTI: a pair spans several of the kernel's chunks

Per case ``tol_log`` is 4 x the largest |reference float32 value - the same
formula in float64 on the same float32 inputs| over rmse_log and sc_inv: the
noise of the reference's own float32 log and of the cancellation in sc_inv.
"""
import argparse
import ast
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGEN = (0.40810811, 0.99189189, 0.03594771, 0.96405229)


def load_reference(ref_dir):
    sys.modules.setdefault("minieigen", types.SimpleNamespace(Quaternion=None, Vector3=None))
    sys.path.insert(0, ref_dir)
    import demon_metrics
    tree = ast.parse(open(os.path.join(ref_dir, "main.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "evaluate_metric"]
    assert len(fn) == 1
    ns = {"np": np, "l1_inverse": demon_metrics.l1_inverse, "scale_invariant": demon_metrics.scale_invariant}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "main.py", "exec"), ns)
    return ns["evaluate_metric"]


def log_gap(gt, p, ref_vals):
    """|reference rmse_log / sc_inv - the float64 formula on the same float32 inputs|."""
    if gt.size == 0:
        return 0.0
    l = np.log(gt.astype(np.float64)) - np.log(p.astype(np.float64))
    rl = np.sqrt(np.mean(l * l))
    sc = np.sqrt(np.sum(l * l) / l.size - np.square(np.sum(l)) / np.square(float(l.size)))
    gaps = [abs(float(ref_vals[3]) - rl), abs(float(ref_vals[8]) - sc)]
    return max(g for g in gaps if np.isfinite(g)) if any(np.isfinite(g) for g in gaps) else 0.0


def run_case(evaluate_metric, pred, gt, rescale, demon, min_depth, nlabel):
    """main.py:536-593 on [B, 1, H, W] tensors."""
    depth = pred.clone()
    gt4 = gt
    B = gt4.shape[0]
    if rescale is not None:
        depth = depth * rescale.view(B, 1, 1, 1)
    if demon:
        mask = (gt4 >= 0.5) & (gt4 <= 10) & ~torch.isnan(gt4)
    else:
        H, W = gt4.shape[2:]
        y0, y1, x0, x1 = (int(v) for v in
                          np.array([EIGEN[0] * H, EIGEN[1] * H, EIGEN[2] * W, EIGEN[3] * W]).astype(np.int32))
        inside = torch.zeros_like(gt4, dtype=torch.bool)
        inside[:, :, y0:y1, x0:x1] = True
        mask = (gt4 > 0) & (gt4 < 80) & inside
    med_gt, med_p = [], []
    for b in range(B):
        sel = mask[b] if int(mask[b].sum()) else torch.ones_like(mask[b])   # empty mask: the whole image
        med_gt.append(gt4[b][sel].median())
        med_p.append(depth[b][sel].median())
    median_scale = torch.stack([g / p for g, p in zip(med_gt, med_p)]).float()
    depth = depth * median_scale.view(B, 1, 1, 1)
    lo, hi = float(min_depth), float(min_depth * nlabel)
    depth = torch.where(depth <= lo, torch.tensor(lo), depth)
    depth = torch.where(depth > hi, torch.tensor(hi), depth)
    out = {"mask": mask[:, 0].numpy(), "n": mask.reshape(B, -1).sum(1).numpy().astype(np.int64),
           "med_gt": np.array([float(v) for v in med_gt], np.float32),
           "med_p": np.array([float(v) for v in med_p], np.float32),
           "scale": median_scale.numpy().astype(np.float32), "depth": depth[:, 0].numpy()}
    gap = 0.0
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        per = []
        for b in range(B):
            g, p = gt4[b][mask[b]].numpy(), depth[b][mask[b]].numpy()
            per.append(np.array(evaluate_metric(g, p), np.float64))
            gap = max(gap, log_gap(g, p, per[-1]))
        g, p = gt4[mask].numpy(), depth[mask].numpy()
        pooled = np.array(evaluate_metric(g, p), np.float64)
        gap = max(gap, log_gap(g, p, pooled))
    out["ref_pair"] = np.stack(per)
    out["ref_pool"] = pooled
    out["tol_log"] = np.float64(4.0 * gap)
    return out


def kitti_scene(rng, B, H, W, quant):
    gt = rng.uniform(0.6, 95.0, (B, 1, H, W))
    gt[rng.random(gt.shape) < 0.15] = 0.0                        # no lidar return
    pred = np.where(gt > 0, gt, 20.0) * rng.uniform(0.7, 1.4, gt.shape)
    pred = pred * rng.uniform(0.3, 3.0, (B, 1, 1, 1))            # scale ambiguity
    if quant:
        gt = np.round(gt * quant) / quant
        pred = np.maximum(np.round(pred * quant) / quant, 1.0 / quant)
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(gt.astype(np.float32))


def padded(pred, hp, wp):
    """The crop's padded home: NaN outside the crop, so a stray read shows."""
    B, _, H, W = pred.shape
    pad = torch.full((B, 1, hp, wp), float("nan"), dtype=torch.float32)
    pad[:, :, :H, :W] = pred
    return pad


def set_parity(gt, b, even):
    """Give pair b an even / odd masked count by dropping one valid pixel inside the crop."""
    H, W = gt.shape[2:]
    c = np.array([EIGEN[0] * H, EIGEN[1] * H, EIGEN[2] * W, EIGEN[3] * W]).astype(np.int32)
    m = (gt[b, 0] > 0) & (gt[b, 0] < 80)
    n = int(m[c[0]:c[1], c[2]:c[3]].sum())
    if (n % 2 == 0) != even:
        ys, xs = np.nonzero(m[c[0]:c[1], c[2]:c[3]].numpy())
        gt[b, 0, c[0] + ys[0], c[2] + xs[0]] = 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference's main.py / demon_metrics.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    a = ap.parse_args()
    evaluate_metric = load_reference(a.reference)
    rng = np.random.default_rng(20240607)
    cases = {}

    pred, gt = kitti_scene(rng, 3, 37, 123, 64)
    set_parity(gt, 0, True)
    set_parity(gt, 1, False)
    cases["a"] = dict(pred_pad=padded(pred, 128, 128), gt=gt, rescale=torch.tensor([0.5, 1.25, 2.0]), demon=0,
                      min_depth=1.0, nlabel=64)

    pred, gt = kitti_scene(rng, 2, 37, 123, 64)
    gt[1] = torch.from_numpy(np.round(rng.uniform(80.0, 120.0, gt[1].shape) * 64) / 64).float()
    cases["b"] = dict(pred_pad=padded(pred, 128, 128), gt=gt, rescale=None, demon=0, min_depth=1.0, nlabel=64)

    g = rng.uniform(0.2, 12.0, (2, 1, 48, 64))
    p = g * rng.uniform(0.6, 1.6, g.shape) * rng.uniform(0.5, 2.0, (2, 1, 1, 1))
    g[rng.random(g.shape) < 0.1] = np.nan
    g[rng.random(g.shape) < 0.02] = np.inf
    g[rng.random(g.shape) < 0.02] = -1.0
    cases["c"] = dict(pred_pad=torch.from_numpy(p.astype(np.float32)), gt=torch.from_numpy(g.astype(np.float32)),
                      rescale=None, demon=1, min_depth=0.5, nlabel=16)

    pred, gt = kitti_scene(rng, 2, 96, 320, 256)
    cases["d"] = dict(pred_pad=pred, gt=gt, rescale=torch.tensor([0.75, 1.5]), demon=0, min_depth=1.0, nlabel=64)

    out = {}
    for name, c in cases.items():
        H, W = c["gt"].shape[2:]
        pred = c["pred_pad"][:, :, :H, :W]
        r = run_case(evaluate_metric, pred, c["gt"], c["rescale"], c["demon"], c["min_depth"], c["nlabel"])
        r.update(pred_pad=c["pred_pad"][:, 0].numpy(), gt=c["gt"][:, 0].numpy(),
                 rescale=(c["rescale"] if c["rescale"] is not None else torch.zeros(0)).numpy().astype(np.float32),
                 demon=np.int64(c["demon"]), min_depth=np.float64(c["min_depth"]), nlabel=np.int64(c["nlabel"]))
        for k, v in r.items():
            out[f"{name}/{k}"] = v
        print(name, "n", r["n"], "scale", r["scale"], "tol_log", float(r["tol_log"]))
        print("   pooled", r["ref_pool"])
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
