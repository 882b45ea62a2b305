"""A ragged last chunk through all four entry points of the two conv2 stacks
(``context_refine`` / ``context_refine_autograd`` in chunks of 2, 2, 1 planes
against one chunk of 5; ``dep_context_refine`` / ``dep_context_refine_autograd``
in chunks of 2, 1 pairs against one of 3): the forward's bits and the input
gradients' bits do not depend on the chunking.

A weight gradient is an fp32 sum over the chunks, rounded in another order, so
it is compared with the unchunked one at the tolerance
test_gpu_context_train.py::test_one_plane_per_chunk gives a chunked weight
gradient: 2 x the error of the modules under float16 autocast against a
float64 restatement, max|g_torch - g64| (the stacks are those tests' stacks,
built the same way; the maps, 9 x 13 and 12 x 20, are smaller than the largest
dilation's reach)."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_context_train import _convs as _context_convs, _stack as _context_modules
from test_gpu_dep_context_train import _convs as _dep_convs

pytestmark = pytest.mark.gpu

WGRAD_FACTOR = 2.0          # test_one_plane_per_chunk / test_one_pair_per_chunk: "<= 2.0 * err_torch_autocast"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _grads(convs, fn, inputs, need_grad, go, cuda):
    """(output, {name: gradient}) of ``fn(convs, *inputs)`` under float16 autocast on a fresh device copy."""
    convs = copy.deepcopy(convs).to(cuda)
    inputs = {n: t.to(cuda).requires_grad_(n in need_grad) for n, t in inputs.items()}
    with torch.autocast("cuda", torch.float16):
        out = fn(convs, *inputs.values())
    out.backward(go.to(cuda))
    g = {k: p.grad for k, p in convs.named_parameters()}
    g.update({n: inputs[n].grad for n in need_grad})
    return out.detach(), g


def _module_errors(convs, modules, inputs, need_grad, go, cuda):
    """max|g_torch - g64| per Conv2d weight: the modules under float16 autocast on the device against the
    same graph in float64 on the CPU."""
    c64 = copy.deepcopy(convs).double()
    modules(c64, *[t.double().requires_grad_(n in need_grad) for n, t in inputs.items()]).backward(go.double())
    _, theirs = _grads(convs, modules, inputs, need_grad, go, cuda)
    return {k: float((theirs[k].double().cpu() - p.grad).abs().max()) for k, p in c64.named_parameters()}


def _check(whole, ragged, inference, errors, inputs_with_grad):
    (out_w, g_w), (out_r, g_r) = whole, ragged
    for out in (out_w, out_r, *inference):
        assert out.dtype == torch.float32 and torch.equal(_bits(out), _bits(out_w))
    for k in inputs_with_grad:
        assert torch.equal(_bits(g_r[k]), _bits(g_w[k])), k
    assert len(errors) == 7 and set(g_w) == set(errors) | set(inputs_with_grad)
    for k, e in sorted(errors.items()):
        tol = WGRAD_FACTOR * e
        print({"grad": k, "max_abs_ragged_minus_whole": float((g_r[k] - g_w[k]).abs().max()), "atol": tol})
        assert bool((g_w[k] != 0).any()), k
        torch.testing.assert_close(g_r[k], g_w[k], rtol=0.0, atol=tol)


@functools.lru_cache(maxsize=None)
def _context_case():
    B, L, h, w = 2, 5, 9, 13
    g = torch.Generator().manual_seed(17)
    inputs = {"ctx": torch.randn(B, 32, h, w, generator=g), "costs": torch.randn(B, 1, L, h, w, generator=g)}
    return _context_convs(), inputs, torch.randn(B, 1, L, h, w, generator=g)


def test_context_stack_ragged_chunk(cuda):
    from sfm_amd.context import context_refine, context_refine_autograd, planes_per_chunk
    convs, inputs, go = _context_case()
    B, _, L, h, w = inputs["costs"].shape
    per_plane = 2 * B * h * w * 128 * 2                 # two 128-channel float16 ping-pong buffers
    scratch = {2: 2 * per_plane, 5: 5 * per_plane}
    for n, s in scratch.items():
        assert planes_per_chunk(B, h, w, L, s) == n
    need = ("ctx", "costs")
    whole, ragged = [_grads(convs, lambda c, a, b: context_refine_autograd(c, a, b, max_scratch_bytes=scratch[n]),
                            inputs, need, go, cuda) for n in (5, 2)]
    dconvs = copy.deepcopy(convs).to(cuda)
    inference = [context_refine(dconvs, inputs["ctx"].to(cuda), inputs["costs"].to(cuda), "fp16",
                                max_scratch_bytes=scratch[n]) for n in (5, 2)]
    _check(whole, ragged, inference, _module_errors(convs, _context_modules, inputs, need, go, cuda), need)


def _dep_modules(dep_convs, depth, feat, image):
    """PSNet.forward's torch route (PSNet.py:218-221) in the inputs' dtype."""
    up = F.interpolate(feat, depth.shape[2:], mode="bilinear", align_corners=True)
    return dep_convs(torch.cat((depth.detach(), up, image), dim=1)) + depth


@functools.lru_cache(maxsize=None)
def _dep_case():
    B, h, w, H, W = 3, 5, 7, 12, 20
    g = torch.Generator().manual_seed(19)
    inputs = {"depth": 1.0 + 9.0 * torch.rand(B, 1, H, W, generator=g),
              "feat": torch.randn(B, 32, h, w, generator=g).half().float(),      # float16 values, as the CNN gives
              "image": torch.rand(B, 3, H, W, generator=g)}
    return _dep_convs(), inputs, torch.randn(B, 1, H, W, generator=g)


def test_refinement_stack_ragged_chunk(cuda):
    from sfm_amd.context import dep_context_refine, dep_context_refine_autograd, pairs_per_chunk
    convs, inputs, go = _dep_case()
    B, _, H, W = inputs["depth"].shape
    per_pair = 2 * H * W * 128 * 2                      # two 128-channel float16 ping-pong buffers
    scratch = {2: 2 * per_pair, 3: 3 * per_pair}
    for n, s in scratch.items():
        assert pairs_per_chunk(B, H, W, s) == n
    need = ("depth", "feat")
    whole, ragged = [_grads(convs, lambda c, d, f, i: dep_context_refine_autograd(c, d, f, i,
                                                                                  max_scratch_bytes=scratch[n]),
                            inputs, need, go, cuda) for n in (3, 2)]
    dconvs = copy.deepcopy(convs).to(cuda)
    inference = [dep_context_refine(dconvs, *(t.to(cuda) for t in inputs.values()), "fp16",
                                    max_scratch_bytes=scratch[n]) for n in (3, 2)]
    _check(whole, ragged, inference, _module_errors(convs, _dep_modules, inputs, need, go, cuda), need)
    for _, g in (whole, ragged):                        # the "+ depth" alone reaches depth
        assert torch.equal(_bits(g["depth"]), _bits(go.to(cuda)))
