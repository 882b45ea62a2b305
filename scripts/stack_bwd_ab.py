"""Same-process A/B of forward + backward of the twelve-layer 3-D regularisation
stack (dres0..dres4, classify; PSNet.py:79-102, 159-165) at the KITTI shape
(B = 1, 64 channels, L = 128, 94 x 311), training mode, float16 autocast:

  hip    CostRegularization.forward_differentiable: every Conv3d forward and data gradient as
         sfm_conv3_f16, every weight gradient as sfm_conv3_wgrad_f16 (csrc/regularize_bwd.hip),
         BatchNorm3d / ReLU / residual adds as torch ops on the channels-last tensors
  torch  PSNet._regularize_modules: the nn.Conv3d / nn.BatchNorm3d modules (MIOpen)

HIP-event time of forward plus backward (into the parameters and the cost
volume), arms alternating, WARMUP warm-ups, then median / min / max of REPEATS
repeats per arm (ms per step); the spread of an arm is (max - min) / median.
Peak memory is torch.cuda.max_memory_allocated over one step of the arm, above
what the inputs and parameters hold.  The HIP arm is timed once more with the
library's own events: forward, data-gradient and weight-gradient kernels, and
what remains of the step (torch: BatchNorm, ReLU, adds, casts, packing).  The
weight-gradient kernel's time is also given per layer next to sfm_conv3_f16's
per-layer forward time, its modelled floor (the same FLOPs).  The first line
carries the hash of the kernel sources the run was built from (bench.src_hash).
One process, one stream: it needs no more than the default 4 hardware queues
and sets no thread count.  Run it under a time limit of its own, e.g.
  timeout -k 10 900 python scripts/stack_bwd_ab.py && <next GPU step>
Usage: stack_bwd_ab.py [REPEATS=8] [WARMUP=2]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import torch.nn as nn
import bench
from sfm_amd import _lib, synth
from sfm_amd.psnet import PSNet

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dev = torch.device("cuda", 0)
B, C, L = 1, 64, 128
h, w = synth.feature_hw()

torch.manual_seed(3)
net = PSNet(L, 1.0, feature_fn=nn.Conv2d(3, 32, 4, stride=4)).to(dev).train()
gen = torch.Generator().manual_seed(5)
cost = torch.randn(B, C, L, h, w, generator=gen).to(dev)
gout = torch.randn(B, 1, L, h, w, generator=gen).to(dev)
stack = [p for n, p in net.named_parameters() if n.startswith(("dres", "classify"))]
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, C = {C}, L = {L}, {h} x {w}; "
      f"cost {cost.numel() * 4 / 1e6:.0f} MB; {REPEATS} alternating repeats after {WARMUP} warm-ups; one box, the "
      f"box-to-box spread is not measured", flush=True)


def forward(hip):
    c = cost.detach().requires_grad_()
    with torch.autocast("cuda", torch.float16):
        out = net.forward_differentiable(c) if hip else net._regularize_modules(c)
    return c, out


def step(hip):
    for p in stack:
        p.grad = None
    c, out = forward(hip)
    out.float().backward(gout)
    return c.grad


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    s = sorted(ts)
    med = s[len(s) // 2]
    return med, s[0], s[-1], (s[-1] - s[0]) / med


def peak(hip):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(hip)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


for _ in range(WARMUP):
    gt_ = step(False)
    gw_t = [p.grad.clone() for p in stack]
    gh = step(True)
    gw_h = [p.grad.clone() for p in stack]
torch.cuda.synchronize()
diff_in = float((gt_.float() - gh.float()).abs().max() / gt_.float().abs().max())
diff_w = max(float((a.float() - b.float()).abs().max() / a.float().abs().max()) for a, b in zip(gw_t, gw_h))
del gt_, gh, gw_t, gw_h
tt, th = [], []
for rep in range(REPEATS):
    for hip in ((False, True) if rep % 2 == 0 else (True, False)):
        (th if hip else tt).append(timed(lambda: step(hip))[0])
mem_t, mem_h = peak(False), peak(True)

# the HIP arm's kernels, by the library's own events: the forward alone, then the backward
_lib.profile_select(["conv3_f16", "conv3_wgrad"])
_lib.profile_reset()
_lib.profile_enable(True)
for p in stack:
    p.grad = None
t_total0 = torch.cuda.Event(enable_timing=True)
t_total1 = torch.cuda.Event(enable_timing=True)
t_total0.record()
c, out = forward(True)
torch.cuda.synchronize()
kfwd, nfwd = _lib.profile_read("conv3_f16")
out.float().backward(gout)
t_total1.record()
torch.cuda.synchronize()
_lib.profile_enable(False)
kall, nall = _lib.profile_read("conv3_f16")
kwg, nwg = _lib.profile_read("conv3_wgrad")
_lib.profile_select(None)
kdg, ndg = kall - kfwd, nall - nfwd
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
print(f"torch_ms med/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} peak_MB={mem_t:.0f}", flush=True)
print(f"hip_ms   med/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} peak_MB={mem_h:.0f}", flush=True)
print(f"hip_kernels_ms forward={kfwd:.3f} ({nfwd} launches) data_gradient={kdg:.3f} ({ndg}) "
      f"weight_gradient={kwg:.3f} ({nwg}) torch_remainder={hm - kfwd - kdg - kwg:.3f} (of the median step)", flush=True)
print(f"weight_gradient_per_layer_ms={kwg / max(nwg, 1):.3f} forward_per_layer_ms={kfwd / max(nfwd, 1):.3f} (the modelled "
      f"floor: the same FLOPs) ratio={(kwg / max(nwg, 1)) / (kfwd / max(nfwd, 1)):.2f}", flush=True)
print(f"hip/torch={hm / tm:.3f} hip_max_below_torch_min={hhi < tlo} grad_input_max_abs_diff_over_max_abs={diff_in:.3e} "
      f"grad_weight_worst={diff_w:.3e}", flush=True)
