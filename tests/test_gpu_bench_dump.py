"""bench.py's plain and --full runs on the GPU, at a small shape of the c3 /
c2 workloads (KITTI image size, 2 pairs or 1, 8 planes, H = 512).

A plain run prints the headline fields only and, with --dump-outputs, writes
what its last timed step returned: E, P and the inlier counts whole, the cost
volume (29.9 M elements here, above bench.DUMP_SAMPLE) as the fixed seeded
sample.  The files equal, bit for bit, what the same step computes in this
process from the same seeded inputs.  A --full run adds the per-kernel,
roofline, regularisation and CPU-baseline fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "roofline_sweep", "solve", "kernel_ms", "kernel_ms_source", "roofline_regularize",
             "roofline_regularize_fp16", "roofline_regularize_fp32", "roofline_regularize_fp32x3", "cpu_baseline")


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SFM_BENCH_CPU_STUB",
              "SFM_BENCH_SHARED_GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_step(cuda, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from sfm_amd import synth
    from sfm_amd.pipeline import TwoViewHotPath
    B, C, L, iters = 2, 32, 8, 1
    out = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "c3", "--batch", str(B),
                  "--nlabel", str(L), "--iters", str(iters), "--dump-outputs", str(tmp_path)])
    assert all(k in out for k in HEADLINE) and not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "pairs/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64+bf16" and out["ms_per_step"] > 0
    # value and ms_per_step state the same timed region, B pairs per step (ms_per_step is rounded to 1 us)
    assert out["value"] == pytest.approx(B / (out["ms_per_step"] * 1e-3), rel=2e-3 + 1e-3 / out["ms_per_step"])
    assert sorted(os.listdir(tmp_path)) == ["E.npy", "P.npy", "cost_sample.npy", "inliers.npy"]
    got = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in ("E", "P", "inliers", "cost_sample")}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["E"].dtype == got["P"].dtype == got["inliers"].dtype == np.float64
    assert got["cost_sample"].dtype == np.float32 and got["cost_sample"].shape == (bench.DUMP_SAMPLE,)
    # the same step here: bench.py's rank-0 inputs (seeds 1000 and 0) and hot path
    hw = synth.KITTI_HW
    fhw = synth.feature_hw(hw)
    flow, K, _, _ = synth.kitti_pair_batch(B, seed=1000, hw=hw, device=cuda)
    ref_fea, tgt_fea = synth.features(B, C, fhw[0], fhw[1], seed=0, device=cuda)
    hp = TwoViewHotPath(B, hw, fhw, C, L, iters, 1e-4, 1.0, rescale_depth=True, norm_target=0.6,
                        cost_dtype=torch.bfloat16, device=cuda, fused=True)
    E, P, inl, cost = hp.step(flow, K, ref_fea, tgt_fea)
    torch.cuda.synchronize()
    assert cost.numel() > bench.DUMP_SAMPLE
    assert np.array_equal(got["E"], E.cpu().numpy()) and got["E"].shape == (B, 3, 3)
    assert np.array_equal(got["P"], P.cpu().numpy()) and got["P"].shape == (B, 3, 4)
    assert np.array_equal(got["inliers"], inl.cpu().numpy().astype(np.float64))
    assert out["inliers"] == [int(v) for v in inl.cpu().tolist()]
    idx = torch.randint(cost.numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(bench.DUMP_SEED))
    assert np.array_equal(got["cost_sample"], cost.reshape(-1)[idx.to(cuda)].float().cpu().numpy())
    assert float(np.abs(got["cost_sample"]).sum()) > 0.0


def test_full_run_reports_what_moved(cuda):
    out = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--batch", "1", "--nlabel", "8",
                  "--iters", "1", "--cpu-runs", "1"])
    assert all(k in out for k in HEADLINE + FULL_ONLY)
    assert out["roofline"]["avg_launch_ms"] > 0 and out["roofline_sweep"]["achieved"] > 0
    assert out["solve"]["ms"] > 0 and {"ransac_solve", "ransac_score", "plane_sweep"} <= set(out["kernel_ms"])
    for k in FULL_ONLY:
        if k.startswith("roofline_regularize"):
            assert "error" not in out[k] and out[k]["achieved"] > 0, out[k]
    assert out["cpu_baseline"]["value"] > 0, out["cpu_baseline"]
