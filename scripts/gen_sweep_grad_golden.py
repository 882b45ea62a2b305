#!/usr/bin/env python
"""Generate tests/golden/sweep_grad.npz: the reference's own autograd through
its plane-sweep loop and through one inverse_warp call, for the backward
kernel (csrc/sweep_bwd.hip, sfm_amd.sweep.plane_sweep_cost_autograd /
inverse_warp_autograd).

    python scripts/gen_sweep_grad_golden.py --reference <checkout of the reference>

Runs on the CPU where the reference's sources are at hand, never in a test.
The reference's models/inverse_warp.py is imported at run time (its ``.cuda()``
calls made no-ops for the duration); the loop of PSNet.py:146-157 around it is
restated here in float32.  Only data is written.

  cost/  B = 2, C = 8, 12 x 16, L = 4, two different poses, feature-resolution
         intrinsics: ref, tgt, pose, K4, K4inv, nlabel, min_depth, the seeded
         N(0, 1) gradient g of the [B, 2C, L, h, w] volume, and the reference's
         grad_ref, grad_tgt
  warp/  one inverse_warp call with a non-constant depth map: feat, depth,
         pose, K, Kinv, g, grad_feat
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoCuda:
    def __enter__(self):
        self.orig = torch.Tensor.cuda
        torch.Tensor.cuda = lambda t, *a, **k: t
        return self

    def __exit__(self, *a):
        torch.Tensor.cuda = self.orig


def _rot(ax, ay, az):
    return torch.matrix_exp(torch.tensor([[0.0, -az, ay], [az, 0.0, -ax], [-ay, ax, 0.0]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sweep_grad.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_inverse_warp",
                                                  os.path.join(a.reference, "models", "inverse_warp.py"))
    iw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(iw)

    gen = torch.Generator().manual_seed(11)
    B, C, h, w, L, min_depth = 2, 8, 12, 16, 4, 1.0
    ref = torch.randn(B, C, h, w, generator=gen).requires_grad_()
    tgt = torch.randn(B, C, h, w, generator=gen).requires_grad_()
    K4 = torch.tensor([[[14.0, 0, 7.6], [0, 14.0, 5.7], [0, 0, 1]], [[15.5, 0, 7.3], [0, 13.0, 5.2], [0, 0, 1]]])
    Ki4 = torch.inverse(K4)
    pose = torch.zeros(B, 3, 4)
    pose[0, :, :3] = _rot(0.01, -0.02, 0.015)
    pose[0, :, 3] = torch.tensor([0.31, -0.12, -0.35])
    pose[1, :, :3] = _rot(-0.03, 0.04, -0.12)
    pose[1, :, 3] = torch.tensor([-0.45, 0.2, 0.4])
    g = torch.randn(B, 2 * C, L, h, w, generator=gen)
    # the volume of PSNet.py:146-157 in float32: reference rows, and the target warped to the inverse-depth
    # planes min_depth L / (i + 1) (the same float32 bits as the reference's own division)
    far = torch.full((B, h, w), min_depth * L)
    cost = torch.zeros(B, 2 * C, L, h, w)
    with _NoCuda():
        for i in range(L):
            cost[:, :C, i] = ref
            cost[:, C:, i] = iw.inverse_warp(tgt, far / (i + 1), pose, K4, Ki4)
    cost.backward(g)
    out = {f"cost/{k}": v for k, v in dict(
        ref=ref.detach().numpy(), tgt=tgt.detach().numpy(), pose=pose.numpy(), K4=K4.numpy(), K4inv=Ki4.numpy(),
        nlabel=np.int32(L), min_depth=np.float32(min_depth), g=g.numpy(), grad_ref=ref.grad.numpy(),
        grad_tgt=tgt.grad.numpy()).items()}
    assert float((cost[:, C:].detach() != 0).float().mean()) > 0.5       # most samples in range

    feat = torch.randn(B, C, h, w, generator=gen).requires_grad_()
    depth = 1.5 + 3.0 * torch.rand(B, h, w, generator=gen)
    gw = torch.randn(B, C, h, w, generator=gen)
    with _NoCuda():
        warped = iw.inverse_warp(feat, depth, pose, K4, Ki4)
    warped.backward(gw)
    assert float((warped.detach() != 0).float().mean()) > 0.5
    out.update({f"warp/{k}": v for k, v in dict(
        feat=feat.detach().numpy(), depth=depth.numpy(), pose=pose.numpy(), K=K4.numpy(), Kinv=Ki4.numpy(),
        g=gw.numpy(), grad_feat=feat.grad.numpy()).items()})
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
