"""sfm_depth_metrics (csrc/metrics.hip) on the device: the kernel's rows
against the reference fixture (tests/golden/metrics.npz) and the host
specification, the padded view read in place, batch independence, and
``validate`` end to end on synthetic pairs.

Rules (tests/test_validate.py states where they come from): row slots 0-3 and
9-11 and depth_out are bit-equal to the fixture; slots 4-8 and 12 are within
1e-10 relative of depth_metric_rows_host (the same float32 terms summed in
float64 in another order); the nine derived metrics against the reference's
values follow the CPU test's rules."""
import numpy as np
import pytest
import torch

from test_validate import CASES, case_inputs, check_exact_slots, check_metrics

pytestmark = pytest.mark.gpu

SUM_SLOTS = [4, 5, 6, 7, 8, 12]


def _close_sums(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    for k in SUM_SLOTS:
        assert np.all(np.abs(got[:, k] - want[:, k]) <= 1e-10 * np.abs(want[:, k])), (what, k, got[:, k], want[:, k])


@pytest.mark.parametrize("name", CASES)
def test_kernel_rows_match_fixture(cuda, golden, name):
    from sfm_amd import validate as V
    c = golden("metrics.npz")[name]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    H, W = gt.shape[1:]
    pred_dev = torch.from_numpy(c["pred_pad"]).to(cuda)[:, :H, :W]          # a view of the padded map
    rs = None if rescale is None else rescale.to(cuda)
    rows, depth = V.depth_metric_rows(pred_dev, gt.to(cuda), rs, dataset, min_depth, nlabel, return_depth=True)
    rows, depth = rows.cpu().numpy(), depth.cpu().numpy()
    check_exact_slots(rows, depth, c)
    host = V.depth_metric_rows_host(pred, gt, rescale, dataset, min_depth, nlabel).numpy()
    for k in (0, 1, 2, 3, 9, 10, 11, 13, 14, 15):
        assert np.array_equal(rows[:, k], host[:, k]), k
    _close_sums(rows, host, name)
    per = V.metrics_from_rows(rows)
    for b in range(gt.shape[0]):
        check_metrics(per[b], c["ref_pair"][b], float(c["tol_log"]), (name, b))
    check_metrics(V.metrics_from_rows(rows, [gt.shape[0]])[0], c["ref_pool"], float(c["tol_log"]), (name, "pooled"))


def test_padded_view_equals_contiguous_crop(cuda, golden):
    from sfm_amd import validate as V
    c = golden("metrics.npz")["a"]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    H, W = gt.shape[1:]
    pad = torch.from_numpy(c["pred_pad"]).to(cuda)
    view = pad[:, :H, :W]
    assert not view.is_contiguous()
    a = V.depth_metric_rows(view, gt.to(cuda), rescale.to(cuda), dataset, min_depth, nlabel)
    b = V.depth_metric_rows(view.contiguous(), gt.to(cuda), rescale.to(cuda), dataset, min_depth, nlabel)
    c4 = V.depth_metric_rows(view.unsqueeze(1), gt.to(cuda).unsqueeze(1), rescale.to(cuda), dataset, min_depth, nlabel)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(a.view(torch.int64), c4.view(torch.int64))


@pytest.mark.parametrize("name", ["a", "d"])
def test_row_is_independent_of_the_batch(cuda, golden, name):
    """One pair alone, as the last of a batch of 3, and run twice: the same 16 doubles."""
    from sfm_amd import validate as V
    c = golden("metrics.npz")[name]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    pred, gt, rescale = pred.to(cuda), gt.to(cuda), rescale.to(cuda)
    alone = V.depth_metric_rows(pred[1:2], gt[1:2], rescale[1:2], dataset, min_depth, nlabel)
    again = V.depth_metric_rows(pred[1:2], gt[1:2], rescale[1:2], dataset, min_depth, nlabel)
    order = [0, 0, 1]
    last = V.depth_metric_rows(pred[order], gt[order], rescale[order], dataset, min_depth, nlabel)
    assert torch.equal(alone.view(torch.int64), again.view(torch.int64))
    assert torch.equal(alone.view(torch.int64)[0], last.view(torch.int64)[2])


def test_nan_in_the_whole_image_fallback(cuda, golden):
    """An empty mask whose image holds a NaN: NaN medians and scale, zero sums (as torch's median)."""
    from sfm_amd import validate as V
    c = golden("metrics.npz")["b"]
    pred, gt, rescale, dataset, min_depth, nlabel = case_inputs(c)
    gt = gt.clone()
    gt[1, 3, 5] = float("nan")
    rows = V.depth_metric_rows(pred.to(cuda), gt.to(cuda), None, dataset, min_depth, nlabel).cpu().numpy()
    host = V.depth_metric_rows_host(pred, gt, None, dataset, min_depth, nlabel).numpy()
    assert rows[1, 0] == 0 and np.isnan(rows[1, 1]) and np.isnan(rows[1, 3]) and not np.isnan(rows[1, 2])
    assert np.array_equal(rows[1, 4:], np.zeros(12))
    assert np.array_equal(rows[0, :4], host[0, :4]) and np.array_equal(rows[1, 2], host[1, 2])


class _Flow(torch.nn.Module):
    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, x):
        return self.flow.to(x.device), torch.ones_like(self.flow[:, :1]).to(x.device)


class _Recorded(torch.nn.Module):
    """The model under validation, keeping the depth each forward returned."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.depths = []

    def forward(self, *args):
        out = self.inner(*args)
        self.depths.append(out[2].detach().clone())
        return out


@pytest.mark.parametrize("gt_pose", [True, False])
def test_validate_end_to_end(cuda, gt_pose):
    """validate on 4 synthetic pairs (2 batches of 2) at test_gpu_sfmnet.py's
    image shape: synth flow as the flow estimator, synth depth as ground truth,
    GT pose or RANSAC pose, RESCALE_DEPTH on.  The metrics equal the host
    specification's on the depth the model returned."""
    from models.SFMnet import SFMnet
    from sfm_amd import synth, validate as V
    from sfm_amd.config import defaults
    from sfm_amd.depth import SweepDepthEstimator
    HW, B, L = (96, 160), 2, 32
    cfg = defaults()
    cfg.update(ransac_iter=2, RESCALE_DEPTH=True, NORM_TARGET=0.6, GT_POSE=gt_pose)
    g = torch.Generator().manual_seed(7)
    batches, flows = [], []
    for i in range(2):
        flow, _, pose, depth = synth.kitti_pair_batch(B, seed=31 + i, hw=HW)
        K = synth.intrinsics(B, 180.0, 180.0, 80.0, 48.0)
        flows.append(flow)
        img0, img1 = torch.randn(B, 3, *HW, generator=g), torch.randn(B, 3, *HW, generator=g)
        batches.append(((img0, img1), K, (pose, pose), None, (depth.unsqueeze(1), depth.unsqueeze(1))))

    class _BatchFlow(torch.nn.Module):          # the stored flow of the batch in flight
        def forward(self, x):
            f = flows[len(model.depths)]
            return f.to(x.device), torch.ones_like(f[:, :1]).to(x.device)

    model = _Recorded(SFMnet(L, 1.0, flow_estimator=_BatchFlow(), cfg=cfg,
                             depth_estimator=SweepDepthEstimator(L, 1.0, rescale_depth=True, norm_target=0.6)))
    out = V.validate(model, batches, cfg, L)
    assert len(model.depths) == 2 and tuple(model.depths[0].shape) == (B, 1, *HW)
    host_rows = []
    for (_, _, poses, _, gts), d in zip(batches, model.depths):
        rescale = (torch.norm(poses[1].to(cuda)[:, :, -1:].squeeze(-1), dim=-1) / 0.6).cpu()   # as validate forms it
        host_rows.append(V.depth_metric_rows_host(d.cpu(), gts[1], rescale, "kitti", 1.0, L))
    host_rows = torch.cat(host_rows).numpy()
    rows = out["rows"].numpy()
    assert rows.shape == (4, 16) and np.all(rows[:, 0] > 0)
    for k in (0, 1, 2, 3, 9, 10, 11):
        assert np.array_equal(rows[:, k], host_rows[:, k]), k
    _close_sums(rows, host_rows, "validate")
    want = V.metrics_from_rows(host_rows, [B, B])
    got = out["batch_metrics"]
    assert np.array_equal(got[:, 4:7], want[:, 4:7])
    assert np.allclose(got, want, rtol=1e-9, atol=0.0)
    avg = np.array([out["metrics"][k] for k in V.METRIC_NAMES])
    assert np.all(np.isfinite(avg)) and np.allclose(avg, want.mean(0), rtol=1e-9, atol=0.0)
