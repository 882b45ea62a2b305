"""Validation metrics on the CPU (sfm_amd/validate.py): the host specification
of the metric row against the reference's own results (tests/golden/metrics.npz,
scripts/gen_metrics_golden.py), pooled groups, two-rank gloo sharding of
``validate`` against one process, and the argument checks of
sfm_depth_metrics without a device.

Tolerances.  n, the mask, both medians, the scale, the three threshold counts
and the clamped depth are equal.  abs_rel, sq_rel, rmse and l1_inv are sums of
non-negative float32 terms: numpy's blocked pairwise float32 sum over
n <= 2^17 terms errs by at most about 30 * 2^-24 ~ 2e-6 relative, 1e-5 is that
bound with margin.  rmse_log and sc_inv carry the reference's own float32 log
and the cancellation in sc_inv; the generator measured that noise per case and
stored 4 x the largest gap as ``tol_log`` (absolute)."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["a", "b", "c", "d"]
SUMS = [0, 1, 2, 7]          # abs_rel, sq_rel, rmse, l1_inv
LOGS = [3, 8]                # rmse_log, sc_inv
COUNTS = [4, 5, 6]           # a1, a2, a3


def case_inputs(c):
    """(pred view [B,H,W] into the stored padded map, gt, rescale or None, dataset, min_depth, nlabel)."""
    gt = torch.from_numpy(c["gt"])
    H, W = gt.shape[1:]
    pred = torch.from_numpy(c["pred_pad"])[:, :H, :W]
    rescale = torch.from_numpy(c["rescale"]) if c["rescale"].size else None
    return pred, gt, rescale, "demon" if int(c["demon"]) else "kitti", float(c["min_depth"]), int(c["nlabel"])


def check_metrics(got, want, tol_log, what):
    """The nine metrics against the reference's values under the module docstring's rules."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if np.isnan(want).all():
        assert np.isnan(got).all(), (what, got)
        return
    for k in SUMS:
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (what, k, got[k], want[k])
    for k in LOGS:
        assert abs(got[k] - want[k]) <= tol_log, (what, k, got[k], want[k], tol_log)
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def check_exact_slots(rows, depth, c):
    """Row slots 0-3, the counts and the clamped depth equal the fixture's."""
    rows = np.asarray(rows)
    n = c["n"].astype(np.float64)
    assert np.array_equal(rows[:, 0], n)
    assert np.array_equal(rows[:, 1].astype(np.float32).view(np.uint32), c["med_gt"].view(np.uint32))
    assert np.array_equal(rows[:, 2].astype(np.float32).view(np.uint32), c["med_p"].view(np.uint32))
    assert np.array_equal(rows[:, 3].astype(np.float32).view(np.uint32), c["scale"].view(np.uint32))
    assert np.array_equal(rows[:, 1], c["med_gt"].astype(np.float64))       # float32 values, held exactly
    assert np.array_equal(rows[:, 3], c["scale"].astype(np.float64))
    for b in range(rows.shape[0]):
        if n[b] > 0:
            assert np.array_equal(rows[b, 9:12] / n[b], c["ref_pair"][b, 4:7]), b
        else:
            assert np.array_equal(rows[b, 4:13], np.zeros(9)), b
    assert np.array_equal(rows[:, 13:], np.zeros((rows.shape[0], 3)))
    assert np.array_equal(np.asarray(depth).view(np.uint32), c["depth"].view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_host_rows_match_reference(golden, name):
    from sfm_amd import validate as V
    c = golden("metrics.npz")[name]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    assert np.array_equal(V.depth_mask(gt, dataset).numpy(), c["mask"])
    rows, depth = V.depth_metric_rows_host(pred, gt, rescale, dataset, min_depth, nlabel, return_depth=True)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (gt.shape[0], 16)
    check_exact_slots(rows.numpy(), depth.numpy(), c)
    per = V.metrics_from_rows(rows)
    for b in range(gt.shape[0]):
        check_metrics(per[b], c["ref_pair"][b], float(c["tol_log"]), (name, b))
    pooled = V.metrics_from_rows(rows, [gt.shape[0]])
    check_metrics(pooled[0], c["ref_pool"], float(c["tol_log"]), (name, "pooled"))


def test_cases_cover_what_they_claim(golden):
    g = golden("metrics.npz")
    n = g["a"]["n"]
    assert any(v % 2 == 0 for v in n) and any(v % 2 == 1 for v in n)                # lower median, both parities
    assert (g["a"]["depth"] == 1.0).any() and (g["a"]["depth"] == 64.0).any()       # both clamps taken
    assert np.isnan(g["a"]["pred_pad"][:, 37:, :]).all()                            # outside the crop: never read
    assert g["b"]["n"][1] == 0 and g["b"]["n"][0] > 0
    assert np.isnan(g["c"]["gt"]).any() and int(g["c"]["demon"]) == 1
    assert g["d"]["gt"].shape[1] * g["d"]["gt"].shape[2] > 4 * 4096                 # several chunks per pair


def test_empty_mask_pair_falls_back_to_whole_image(golden):
    """main.py:582: the scale of a pair without a masked pixel comes from the
    whole image's medians; its metrics are NaN and it adds nothing to a pool."""
    from sfm_amd import validate as V
    c = golden("metrics.npz")["b"]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    rows = V.depth_metric_rows_host(pred, gt, rescale, dataset, min_depth, nlabel)
    want = gt[1].median() / pred[1].median()
    assert float(rows[1, 3]) == float(want) == float(c["scale"][1])
    m = V.metrics_from_rows(rows)
    assert np.isnan(m[1]).all() and np.isfinite(m[0]).all()
    assert np.array_equal(V.metrics_from_rows(rows, [2])[0], m[0])
    assert np.isnan(V.metrics_from_rows(rows[1:], [1, 0])).all()                    # an empty group too
    # a NaN anywhere in the whole-image fallback makes the median NaN, as torch's does
    gt2 = gt.clone(); gt2[1, 0, 0] = float("nan")
    assert np.isnan(float(V.depth_metric_rows_host(pred, gt2, rescale, dataset, min_depth, nlabel)[1, 1]))


# ---------------------------------------------------------------------------
# validate(): two gloo ranks against one process
# ---------------------------------------------------------------------------
class _StoredDepth(torch.nn.Module):
    """Stands in for SFMnet: returns the stored padded depth of the pairs whose
    index rides in pixel (0, 0) of the first image, in the eval return tuple."""

    def __init__(self, depth_pad):
        super().__init__()
        self.depth_pad = depth_pad

    def forward(self, ref, target, K, pose_gt=None, pred_pose=None, use_gt_pose=False, h_side=None, w_side=None):
        assert ref.shape[2] % 128 == 0 and ref.shape[3] % 128 == 0            # main.py:495-499
        idx = ref[:, 0, 0, 0].long()
        return None, None, self.depth_pad[idx].unsqueeze(1), {}


def _five_pairs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"), allow_pickle=False)
    depth_pad = torch.from_numpy(np.concatenate([g["a/pred_pad"], g["b/pred_pad"]]))
    gt = torch.from_numpy(np.concatenate([g["a/gt"], g["b/gt"]])).unsqueeze(1)
    B, H, W = 5, gt.shape[2], gt.shape[3]
    img = torch.zeros(B, 3, H, W)
    img[:, 0, 0, 0] = torch.arange(B, dtype=torch.float32)
    K = torch.eye(3).repeat(B, 1, 1)
    pose = torch.cat([torch.eye(3).repeat(B, 1, 1), torch.tensor([0.3, 0.6, 0.9, 1.2, 1.5]).reshape(B, 1, 1)
                      * torch.tensor([0.6, 0.0, 0.8]).reshape(1, 3, 1)], 2)
    batches = []
    for lo, hi in ((0, 2), (2, 5)):
        s = slice(lo, hi)
        batches.append(((img[s], img[s]), K[s], (pose[s], pose[s]), None, (gt[s], gt[s])))
    return _StoredDepth(depth_pad), batches


def _run_validate(world, rank):
    from sfm_amd import validate as V
    from sfm_amd.config import defaults
    cfg = defaults()
    cfg.update(RESCALE_DEPTH=True, NORM_TARGET=0.6)
    model, batches = _five_pairs()
    r = V.validate(model, batches, cfg, 64, world=world, rank=rank, host_rows=True)
    return np.concatenate([np.array([r["metrics"][k] for k in V.METRIC_NAMES]), r["batch_metrics"].ravel(),
                           r["rows"].numpy().ravel()])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
    from sfm_amd import dist
    r, w, _ = dist.init(backend="gloo")
    got = _run_validate(w, r)
    dist.barrier()
    if rank == 0:
        np.save(out_path, got)
    torch.distributed.destroy_process_group()


def test_two_rank_validate_is_byte_identical(tmp_path):
    out = str(tmp_path / "validate.npy")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = np.load(out)
    want = _run_validate(1, 0)
    assert got.shape == want.shape == (9 + 2 * 9 + 5 * 16,)
    assert got.tobytes() == want.tobytes()
    # the running average weights each batch's pooled metrics by its size (main.py:596-601)
    bm = want[9:27].reshape(2, 9)
    assert np.array_equal(want[:9], (bm[0] * 2 + bm[1] * 3) / 5)
    assert np.isfinite(want[:9]).all()


# ---------------------------------------------------------------------------
# C ABI argument rules (no device)
# ---------------------------------------------------------------------------
def test_depth_metrics_argument_rules():
    from sfm_amd import _lib
    lib = _lib.load()
    v = ctypes.c_void_p(8)
    H, W = 37, 123
    ws = lib.sfm_depth_metrics_workspace_bytes(2, H, W)
    assert ws > 0 and lib.sfm_depth_metrics_workspace_bytes(0, H, W) == 0
    assert lib.sfm_depth_metrics_workspace_bytes(3, H, W) > ws

    def call(pred=v, bs=128 * 128, rs=128, gt=v, B=2, H=H, W=W, rescale=None, mode=0, rect=(15, 36, 4, 118),
             lo=1.0, hi=64.0, rows=v, work=v, nbytes=ws):
        return lib.sfm_depth_metrics(pred, bs, rs, gt, B, H, W, rescale, mode, *rect, lo, hi, rows, None, work,
                                     nbytes, None)

    for kw in (dict(pred=None), dict(gt=None), dict(rows=None)):
        assert call(**kw) == 1 and b"null" in lib.sfm_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == 1 and b"shape" in lib.sfm_last_error()
    assert call(rs=W - 1) == 1 and b"pred_row_stride" in lib.sfm_last_error()
    assert call(bs=H * 128 - 1) == 1 and b"pred_batch_stride" in lib.sfm_last_error()
    assert call(mode=2) == 1 and call(mode=-1) == 1 and b"mask_mode" in lib.sfm_last_error()
    for rect in ((-1, 36, 4, 118), (15, 38, 4, 118), (15, 36, 4, 124), (20, 19, 4, 118), (15, 36, 9, 8)):
        assert call(rect=rect) == 1 and b"rectangle" in lib.sfm_last_error(), rect
    assert call(lo=0.0) == 1 and call(lo=-1.0) == 1 and call(lo=2.0, hi=1.0) == 1
    assert b"min_depth" in lib.sfm_last_error()
    assert call(work=None) == 3 and b"workspace" in lib.sfm_last_error()
    assert call(nbytes=ws - 1) == 3 and b"workspace" in lib.sfm_last_error()
    # mode 1 ignores the rectangle: a wild one gets past the argument checks to the workspace check
    assert call(mode=1, rect=(-5, 999, -5, 999), nbytes=0) == 3


def test_config_and_exports():
    import sfm_amd
    from sfm_amd import _lib, config
    assert config.defaults().DEMON_DATASET is False
    assert "validate" in sfm_amd.__all__
    assert {"sfm_depth_metrics", "sfm_depth_metrics_workspace_bytes"} <= set(_lib.SYMBOLS)
