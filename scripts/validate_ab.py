#!/usr/bin/env python
"""A/B of the validation metrics stage on the GPU: depth_metric_rows (one
sfm_depth_metrics call, csrc/metrics.hip) against the reference's sequence
written with torch ops on the same GPU (main.py:565-593: boolean-mask
indexing, two .median() per pair, .cpu().numpy(), evaluate_metric's numpy
reductions).

    python scripts/validate_ab.py [--batch 8] [--hw 370 1226] [--reps 30] [--out FILE]

The kernel side is timed with HIP events around the call; the torch side ends
in host work, so it is timed with a host clock after a device synchronise.
Warm-up first, then the median of the repeats, the two sides alternating.
Also reports the kernel family's achieved bytes/s against the pixels it must
read: 8 B per pixel (pred + gt) per pass, four passes over the pixels (three
radix-select histograms and the accumulation).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))

PASSES = 4


def torch_sequence(pred, gt, rescale, min_depth, nlabel):
    """The per-pair Python loop of the reference's validate, on the device, ending on the host."""
    from sfm_amd.validate import eigen_crop
    B, H, W = gt.shape
    depth = pred * rescale.view(B, 1, 1)
    y0, y1, x0, x1 = eigen_crop(H, W)
    crop = torch.zeros_like(gt, dtype=torch.bool)
    crop[:, y0:y1, x0:x1] = True
    mask = (gt > 0) & (gt < 80) & crop
    scales = [float(gt[b][mask[b]].median() / depth[b][mask[b]].median()) for b in range(B)]
    depth = depth * torch.tensor(scales, device=depth.device).view(B, 1, 1)
    depth[depth <= min_depth] = min_depth
    depth[depth > min_depth * nlabel] = min_depth * nlabel
    g, p = gt[mask].cpu().numpy(), depth[mask].cpu().numpy()
    thresh = np.maximum(g / p, p / g)
    a = [(thresh < 1.25 ** k).mean() for k in (1, 2, 3)]
    d = g - p
    l = np.log(g) - np.log(p)
    return (np.mean(np.abs(d) / g), np.mean(d ** 2 / g), np.sqrt((d ** 2).mean()), np.sqrt((l ** 2).mean()), *a,
            np.mean(np.abs(1 / g - 1 / p)), np.sqrt(np.mean(l ** 2) - np.mean(l) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, nargs=2, default=(370, 1226))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validate_ab.py needs a GPU (no CPU timing stands in for it)")
    from sfm_amd import synth, validate as V
    dev = torch.device("cuda", 0)
    B, (H, W) = a.batch, a.hw
    gen = torch.Generator().manual_seed(3)
    gt = synth.depth_field(B, H, W, gen)
    gt[torch.rand(gt.shape, generator=gen) < 0.15] = 0.0
    pred = (torch.where(gt > 0, gt, torch.full_like(gt, 20.0)) * (0.7 + 0.7 * torch.rand(gt.shape, generator=gen))
            * (0.3 + 2.7 * torch.rand(B, 1, 1, generator=gen)))
    rescale = 0.5 + torch.rand(B, generator=gen)
    pred, gt, rescale = pred.to(dev), gt.to(dev), rescale.to(dev)

    def kernel_once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rows = V.depth_metric_rows(pred, gt, rescale, "kitti", 1.0, 64)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), rows

    def torch_once():
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = torch_sequence(pred, gt, rescale, 1.0, 64)
        return (time.perf_counter() - t) * 1e3, m

    for _ in range(a.warmup):
        kernel_once(); torch_once()
    tk, tt = [], []
    for _ in range(a.reps):
        ms, rows = kernel_once(); tk.append(ms)
        ms, ref = torch_once(); tt.append(ms)
    got = V.metrics_from_rows(rows, [B])[0]
    mk, mt = statistics.median(tk), statistics.median(tt)
    need = PASSES * 8.0 * B * H * W
    try:
        clocks = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        clocks = " | ".join(l.strip() for l in clocks.splitlines() if "sclk" in l or "mclk" in l)[:400]
    except Exception as e:        # the tool is optional
        clocks = f"not read ({type(e).__name__})"
    lines = [
        f"validate metrics A/B  B={B} HxW={H}x{W}  device={torch.cuda.get_device_name(dev)}",
        f"warm-up {a.warmup}, {a.reps} alternating repeats, median (min .. max)",
        f"depth_metric_rows (HIP events)   : {mk:9.4f} ms  ({min(tk):.4f} .. {max(tk):.4f})",
        f"torch + numpy sequence (host clk): {mt:9.4f} ms  ({min(tt):.4f} .. {max(tt):.4f})",
        f"ratio torch / kernel             : {mt / mk:9.1f} x",
        f"bytes the passes must read       : {need / 1e6:.2f} MB ({PASSES} passes x 8 B x {B * H * W} pixels)",
        f"achieved                         : {need / (mk * 1e-3) / 1e9:.1f} GB/s of required reads over the whole call",
        f"pooled metrics kernel            : {np.array2string(got, precision=6)}",
        f"pooled metrics torch sequence    : {np.array2string(np.array(ref, np.float64), precision=6)}",
        f"clocks                           : {clocks}",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
