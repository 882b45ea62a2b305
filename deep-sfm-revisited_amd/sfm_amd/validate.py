"""Validation: the reference's ``validate`` loop (main.py:477-601, the branch
without RECORD_POSE) and ``evaluate_metric`` (main.py:727-747 with
demon_metrics.py:63 ``l1_inverse`` and :130 ``scale_invariant``).

The reference masks, median-scales, clamps and reduces pair by pair in Python
(boolean indexing, two ``.median()`` host syncs, ``.cpu().numpy()``, nine
numpy reductions).  Here one stream-ordered call (``sfm_depth_metrics``) turns
predicted and ground-truth depth into one row of 16 float64 per pair:

    0 n        1 med_gt   2 med_p    3 scale
    4 sum |d|/gt   5 sum d*d/gt   6 sum d*d      (d = gt - p, float32 terms)
    7 sum l*l      8 sum l                       (l = log gt - log p, float64)
    9-11 counts of max(gt/p, p/gt) < 1.25, 1.25^2, 1.25^3
    12 sum |1/gt - 1/p|                          13-15 zero

The row holds sums, not means: the reference pools every pair of a loader
batch into one ``evaluate_metric`` call (main.py:593), and both the per-pair
and the pooled metrics follow from the same rows (``metrics_from_rows``).  A
pair's row depends on that pair alone, so rows computed on different ranks
gather into exactly the single-process result.

* ``depth_metric_rows``       the HIP path (CUDA tensors; no CPU fallback)
* ``depth_metric_rows_host``  the same contract in torch / numpy on the CPU:
                              the written specification of the row
* ``metrics_from_rows``       abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3,
                              l1_inv, sc_inv per pair or per group of pairs
* ``validate``                the loop of main.py:477-601

Deviation from the reference: logs and every accumulation are float64 where
numpy works in float32 on float32 arrays.
"""
import numpy as np
import torch

from . import _lib
from . import dist as _dist

METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "l1_inv", "sc_inv")
ROW_WIDTH = 16
_EIGEN_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)      # main.py:572


def eigen_crop(H, W):
    """(y0, y1, x0, x1) of main.py:572: the fractions times the size in float64, truncated to int32."""
    c = np.array([_EIGEN_CROP[0] * H, _EIGEN_CROP[1] * H, _EIGEN_CROP[2] * W, _EIGEN_CROP[3] * W]).astype(np.int32)
    return int(c[0]), int(c[1]), int(c[2]), int(c[3])


def _mode(dataset):
    if dataset == "kitti":
        return 0
    if dataset == "demon":
        return 1
    raise ValueError(f"dataset must be 'kitti' or 'demon', not {dataset!r}")


def _maps(pred, gt):
    """pred, gt as [B, H, W] (a [B, 1, H, W] channel axis is dropped; pred stays a view)."""
    if pred.dim() == 4:
        if pred.shape[1] != 1:
            raise RuntimeError("a 4-D depth must have one channel")
        pred = pred[:, 0]
    if gt.dim() == 4:
        if gt.shape[1] != 1:
            raise RuntimeError("a 4-D ground-truth depth must have one channel")
        gt = gt[:, 0]
    if pred.dim() != 3 or tuple(pred.shape) != tuple(gt.shape):
        raise RuntimeError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must both be [B, H, W]")
    return pred, gt


def depth_metric_rows(pred, gt, rescale=None, dataset="kitti", min_depth=1.0, nlabel=64, return_depth=False):
    """[B, 16] float64 rows on the device (module docstring) from predicted
    depth ``pred`` and ground truth ``gt`` ([B, H, W] or [B, 1, H, W] CUDA
    tensors).  ``pred`` may be the top-left crop view of a padded map; it is
    read in place.  ``rescale`` [B]: the RESCALE_DEPTH factor of main.py:540.
    With ``return_depth`` also the scaled, clamped depth [B, H, W]."""
    mode = _mode(dataset)
    pred, gt = _maps(pred, gt)
    if not (pred.is_cuda and gt.is_cuda):
        raise RuntimeError("depth_metric_rows needs CUDA tensors (HIP path, no CPU fallback); "
                           "depth_metric_rows_host is the CPU specification")
    B, H, W = gt.shape
    dev = gt.device
    if pred.dtype != torch.float32:
        pred = pred.float()
    if pred.stride(2) != 1 or pred.stride(1) < W or (B > 1 and pred.stride(0) < H * pred.stride(1)):
        pred = pred.contiguous()
    row_stride = pred.stride(1)
    batch_stride = pred.stride(0) if B > 1 else max(pred.stride(0), H * row_stride)
    gt = gt.float().contiguous()
    if rescale is not None:
        rescale = rescale.to(dev, torch.float32).reshape(B).contiguous()
    y0, y1, x0, x1 = eigen_crop(H, W) if mode == 0 else (0, H, 0, W)
    rows = torch.empty(B, ROW_WIDTH, dtype=torch.float64, device=dev)
    depth = torch.empty(B, H, W, dtype=torch.float32, device=dev) if return_depth else None
    lib = _lib.load()
    ws = torch.empty(int(lib.sfm_depth_metrics_workspace_bytes(B, H, W)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sfm_depth_metrics(_lib.ptr(pred), int(batch_stride), int(row_stride), _lib.ptr(gt), B, H, W,
                                   _lib.ptr(rescale), mode, y0, y1, x0, x1, float(min_depth),
                                   float(np.float32(min_depth * nlabel)), _lib.ptr(rows), _lib.ptr(depth),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "sfm_depth_metrics")
    return (rows, depth) if return_depth else rows


def depth_mask(gt, dataset="kitti"):
    """The pixels the metrics run over, [B, H, W] bool: main.py:566 (DeMoN:
    0.5 <= gt <= 10, NaN excluded) or main.py:568-574 (KITTI: 0 < gt < 80
    inside the Eigen crop)."""
    mode = _mode(dataset)
    if gt.dim() == 4:
        gt = gt[:, 0]
    if mode == 1:
        return (gt <= 10) & (gt >= 0.5) & (gt == gt)
    y0, y1, x0, x1 = eigen_crop(gt.shape[1], gt.shape[2])
    crop = torch.zeros_like(gt, dtype=torch.bool)
    crop[:, y0:y1, x0:x1] = True
    return (gt > 0) & (gt < 80) & crop


def depth_metric_rows_host(pred, gt, rescale=None, dataset="kitti", min_depth=1.0, nlabel=64, return_depth=False):
    """The row contract of ``depth_metric_rows`` in torch / numpy on the CPU:
    float32 steps as main.py:536-590 takes them, float32 terms as numpy forms
    them on float32 arrays, float64 logs and sums."""
    mode = _mode(dataset)
    pred, gt = _maps(pred.detach().cpu(), gt.detach().cpu())
    pred = pred.float()
    gt = gt.float()
    B, H, W = gt.shape
    if rescale is not None:
        pred = pred * rescale.detach().cpu().float().reshape(B, 1, 1)               # main.py:541
    mask = depth_mask(gt, dataset)
    lo = torch.tensor(min_depth, dtype=torch.float32)
    hi = torch.tensor(float(np.float32(min_depth * nlabel)), dtype=torch.float32)    # main.py:588
    rows = np.zeros((B, ROW_WIDTH), np.float64)
    depth = torch.empty_like(pred)
    for b in range(B):
        m = mask[b]
        n = int(m.sum())
        if n:
            med_gt, med_p = gt[b][m].median(), pred[b][m].median()                   # main.py:580
        else:
            med_gt, med_p = gt[b].median(), pred[b].median()                         # main.py:582
        scale = med_gt / med_p
        p = pred[b] * scale                                                          # main.py:585
        p = torch.where(p <= lo, lo, p)                                              # main.py:589-590
        p = torch.where(p > hi, hi, p)
        depth[b] = p
        g32 = gt[b][m].numpy()
        p32 = p[m].numpy()
        with np.errstate(all="ignore"):
            d = g32 - p32
            dd = d * d
            q0, q1 = g32 / p32, p32 / g32
            l = np.log(g32.astype(np.float64)) - np.log(p32.astype(np.float64))
            inv = np.abs(np.float32(1) / g32 - np.float32(1) / p32)
            rows[b, :4] = n, float(med_gt), float(med_p), float(scale)
            rows[b, 4] = np.sum((np.abs(d) / g32).astype(np.float64))
            rows[b, 5] = np.sum((dd / g32).astype(np.float64))
            rows[b, 6] = np.sum(dd.astype(np.float64))
            rows[b, 7] = np.sum(l * l)
            rows[b, 8] = np.sum(l)
            for k, t in enumerate((1.25, 1.5625, 1.953125)):
                rows[b, 9 + k] = np.count_nonzero((q0 < np.float32(t)) & (q1 < np.float32(t)))
            rows[b, 12] = np.sum(inv.astype(np.float64))
    rows = torch.from_numpy(rows)
    return (rows, depth) if return_depth else rows


def metrics_from_rows(rows, groups=None):
    """[G, 9] float64 (numpy): abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3,
    l1_inv, sc_inv (evaluate_metric's order) from the sums of ``rows`` [B, 16].
    ``groups`` = sizes of consecutive groups of pairs, each pooled as the
    reference pools a loader batch (main.py:593); None = one pair per group.
    A group without a masked pixel gives NaN, as numpy's mean of an empty
    array does."""
    r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
    r = np.asarray(r, np.float64).reshape(-1, ROW_WIDTH)
    if groups is None:
        groups = [1] * r.shape[0]
    if sum(int(g) for g in groups) != r.shape[0]:
        raise ValueError(f"groups {list(groups)} do not add up to {r.shape[0]} rows")
    out = np.empty((len(groups), 9), np.float64)
    start = 0
    for gi, size in enumerate(groups):
        s = np.zeros(ROW_WIDTH, np.float64)
        for row in r[start:start + int(size)]:       # pair order
            s = s + row
        start += int(size)
        n = s[0]
        with np.errstate(all="ignore"):
            n = n if n > 0 else np.float64("nan")
            out[gi] = (s[4] / n, s[5] / n, np.sqrt(s[6] / n), np.sqrt(s[7] / n), s[9] / n, s[10] / n, s[11] / n,
                       s[12] / n, np.sqrt(s[7] / n - (s[8] * s[8]) / (n * n)))
    return out


class AverageMeter:
    """main.py:751-766: running average weighted by the update's count."""

    def __init__(self):
        self.val = self.avg = self.sum = 0.0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _pad128(x):
    """main.py:495-499: replicate-pad bottom / right to a multiple of 128."""
    H, W = x.shape[2], x.shape[3]
    Hn, Wn = int(np.ceil(H / 128) * 128), int(np.ceil(W / 128) * 128)
    return torch.nn.functional.pad(x, (0, Wn - W, 0, Hn - H), "replicate")


def validate(model, batches, cfg, nlabel, dataset=None, world=1, rank=0, device=None, host_rows=False):
    """main.py:477-601 without RECORD_POSE.  ``batches`` yields the loader's
    tuples (inputs [2], intrinsics, poses [2], pred_poses [2] or None,
    depth_gt [2]); the backward pair (input1 -> input0) is scored, as in the
    reference.  Returns {"metrics": {name: running average}, "batch_metrics"
    [nbatch, 9], "rows" [npairs, 16]}.

    With ``world`` > 1 every rank calls this with its ``rank``: it runs the
    model on its ``dist.shard`` of the pairs (numbered through the batches),
    the rows meet in one ``dist.gather_rows`` and are pooled and averaged in
    pair order, which equals the single-process result bit for bit.
    ``host_rows`` computes the rows with ``depth_metric_rows_host`` (CPU)."""
    if cfg.get("RECORD_POSE", False):
        raise NotImplementedError("validate: the RECORD_POSE branch (compute_motion_errors) is not built")
    if dataset is None:
        dataset = "demon" if cfg.get("DEMON_DATASET", False) else "kitti"
    if device is None:
        device = torch.device("cpu") if host_rows else torch.device("cuda", torch.cuda.current_device())
    rows_fn = depth_metric_rows_host if host_rows else depth_metric_rows
    batches = list(batches)
    sizes = [int(b[1].shape[0]) for b in batches]
    mine = _dist.shard(sum(sizes), rank, world)
    model.eval()
    local = []
    first = 0
    with torch.no_grad():
        for (inputs, intrinsics, poses, pred_poses, depth_gt), size in zip(batches, sizes):
            lo, hi = max(mine.start, first) - first, min(mine.stop, first + size) - first
            first += size
            if hi <= lo:
                continue
            sl = slice(lo, hi)
            input0, input1 = inputs[0][sl].to(device), inputs[1][sl].to(device)
            pose_gt_bw = poses[1][sl].to(device)
            gt_bw = depth_gt[1][sl].to(device)
            pred_pose_bw = pred_poses[1][sl].to(device) if pred_poses is not None else None
            K = intrinsics[sl].float().to(device)
            h_raw, w_raw = input1.shape[2], input1.shape[3]
            input1, input0 = _pad128(input1), _pad128(input0)
            _, _, depth_bw, _ = model(input1, input0, K, pose_gt_bw, pred_pose_bw, cfg.GT_POSE, h_raw, w_raw)
            rescale = None
            if cfg.RESCALE_DEPTH:                                    # main.py:536-541
                rescale = torch.norm(pose_gt_bw[:, :, -1:].squeeze(-1), dim=-1) / cfg.NORM_TARGET
            depth_bw = depth_bw[:, :, :h_raw, :w_raw]                # main.py:543: a view, read in place
            local.append(rows_fn(depth_bw, gt_bw, rescale, dataset, cfg.MIN_DEPTH, nlabel))
    rows = torch.cat(local, 0) if local else torch.zeros(0, ROW_WIDTH, dtype=torch.float64, device=device)
    rows = _dist.gather_rows(rows, world).cpu()
    per_batch = metrics_from_rows(rows, sizes)
    meters = [AverageMeter() for _ in METRIC_NAMES]
    for vals, size in zip(per_batch, sizes):                         # main.py:596-601
        for m, v in zip(meters, vals):
            m.update(float(v), size)
    return {"metrics": {k: m.avg for k, m in zip(METRIC_NAMES, meters)}, "batch_metrics": per_batch, "rows": rows}
