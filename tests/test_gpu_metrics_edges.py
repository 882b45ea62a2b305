"""sfm_depth_metrics (csrc/metrics.hip) on the edge cases of
tests/metrics_cases.py against the numpy restatement of the row contract.

Rules: slots 0-3, 9-11, 13-15 and depth_out are bit-equal to the reference
(for NaN the NaN pattern); slots 4-8 and 12 are within 1e-10 of the sum of the
absolute terms as the reference forms them.  Every listed case runs: nothing
in this module skips."""
import numpy as np
import pytest
import torch

from tests import metrics_cases as MC

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in MC.all_cases()}


def _wrapper(cuda, case):
    from sfm_amd import validate as V
    rs = None if case.rescale is None else torch.from_numpy(case.rescale).to(cuda)
    rows, depth = V.depth_metric_rows(torch.from_numpy(case.pred).to(cuda), torch.from_numpy(case.gt).to(cuda), rs,
                                      case.mode, case.min_depth, case.nlabel, return_depth=True)
    return rows.cpu().numpy(), depth.cpu().numpy()


def _abi(cuda, case, pred_dev, batch_stride, row_stride):
    """sfm_depth_metrics itself with the case's mask mode and rectangle on a pred buffer laid out by the caller."""
    from sfm_amd import _lib
    B, H, W = case.gt.shape
    lib = _lib.load()
    gt = torch.from_numpy(case.gt).to(cuda).contiguous()
    rs = None if case.rescale is None else torch.from_numpy(case.rescale).to(cuda)
    rows = torch.full((B, MC.ROW_WIDTH), float("nan"), dtype=torch.float64, device=cuda)
    depth = torch.full((B, H, W), float("nan"), dtype=torch.float32, device=cuda)
    ws = torch.empty(int(lib.sfm_depth_metrics_workspace_bytes(B, H, W)), dtype=torch.uint8, device=cuda)
    rect = case.rect if case.mode == "kitti" else (0, H, 0, W)
    with torch.cuda.device(cuda):
        rc = lib.sfm_depth_metrics(_lib.ptr(pred_dev), int(batch_stride), int(row_stride), _lib.ptr(gt), B, H, W,
                                   _lib.ptr(rs), 0 if case.mode == "kitti" else 1, *rect, float(case.min_depth),
                                   float(np.float32(case.min_depth * case.nlabel)), _lib.ptr(rows), _lib.ptr(depth),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr(cuda))
        _lib.check(rc, "sfm_depth_metrics")
    return rows.cpu().numpy(), depth.cpu().numpy()


def _abi_contiguous(cuda, case):
    B, H, W = case.gt.shape
    return _abi(cuda, case, torch.from_numpy(case.pred).to(cuda).contiguous(), H * W, W)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.via == "wrapper"])
def test_wrapper_case(cuda, name):
    c = CASES[name]
    rows, depth = _wrapper(cuda, c)
    MC.check_rows(rows, depth, MC.expected(c), name)


@pytest.mark.parametrize("name", ["kitti_rect", "empty_rect"])
def test_rectangle_case(cuda, name):
    c = CASES[name]
    rows, depth = _abi_contiguous(cuda, c)
    MC.check_rows(rows, depth, MC.expected(c), name)


def test_strided_view_equals_contiguous(cuda):
    c = CASES["strided"]
    buf, bs, rs = MC.padded_pred(c)
    rows, depth = _abi(cuda, c, torch.from_numpy(buf).to(cuda), bs, rs)
    rows_c, depth_c = _abi_contiguous(cuda, c)
    assert np.array_equal(rows.view(np.int64), rows_c.view(np.int64))
    assert np.array_equal(depth.view(np.uint32), depth_c.view(np.uint32))
    MC.check_rows(rows, depth, MC.expected(c), "strided")


def test_abi_and_wrapper_agree_on_a_wrapper_case(cuda):
    """The same bits through either door (the wrapper passes the whole image for DeMoN)."""
    c = CASES["edges_first"]
    a, da = _wrapper(cuda, c)
    b, db = _abi_contiguous(cuda, c)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
