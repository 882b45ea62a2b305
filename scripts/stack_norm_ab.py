"""Same-process A/B of forward + backward of the twelve-layer 3-D regularisation
stack (dres0..dres4, classify; PSNet.py:79-102, 159-165) at the KITTI shape
(B = 1, 64 channels, L = 128, 94 x 311), training mode, float16 autocast, both
arms CostRegularization.forward_differentiable (every Conv3d on libsfm_hip):

  torch  norm="torch": BatchNorm3d as the module it is, ReLU, residual adds and
         casts as torch ops on the channels-last tensors (the baseline)
  hip    norm="hip": batchnorm3_act_autograd per layer -- sfm_bn3_stats_f16,
         sfm_bn3_apply_f16, sfm_bn3_backward_f16 (csrc/bn3.hip)

HIP-event time of forward plus backward (into the parameters and the cost
volume), arms alternating, WARMUP warm-ups, then mean / min / max of REPEATS
repeats per arm (ms per step).  Peak memory is torch.cuda.max_memory_allocated
over one step of the arm, above what the inputs and parameters hold.  The HIP
arm is timed once more with the library's own events: per kernel name the time
per launch and the achieved bytes/s against the modelled traffic of one
[B, L, h, w, 32] float16 tensor T -- statistics 1 read; apply 1 read + 1 write,
2 reads with a residual; backward 4 reads + 1 write -- next to the streaming
store figure of profiles/r01_probe_store_bw.txt (row D, 4830 GB/s).  The first
line carries the hash of the kernel sources the run was built from
(bench.src_hash).  One process, one stream: it needs no more than the default 4
hardware queues and sets no thread count.  Run it under a time limit of its
own, e.g.
  timeout -k 10 900 python scripts/stack_norm_ab.py && <next GPU step>
Usage: stack_norm_ab.py [REPEATS=8] [WARMUP=2]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import bench
from sfm_amd import _lib, synth
from sfm_amd.regularize import CostRegularization

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
STORE_PROBE_GBS = 4830.4                      # profiles/r01_probe_store_bw.txt, row D (float4 nt flat stream)
dev = torch.device("cuda", 0)
B, C, L = 1, 64, 128
h, w = synth.feature_hw()

torch.manual_seed(3)
net = CostRegularization(C).to(dev).train()
gen = torch.Generator().manual_seed(5)
cost = torch.randn(B, C, L, h, w, generator=gen).to(dev)
gout = torch.randn(B, 1, L, h, w, generator=gen).to(dev)
stack = list(net.parameters())
T = B * L * h * w * 32 * 2                    # bytes of one float16 activation tensor
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, C = {C}, L = {L}, {h} x {w}; "
      f"cost {cost.numel() * 4 / 1e6:.0f} MB, one activation tensor {T / 1e6:.0f} MB; {REPEATS} alternating repeats "
      f"after {WARMUP} warm-ups; one box, the box-to-box spread is not measured", flush=True)


def forward(norm):
    c = cost.detach().requires_grad_()
    with torch.autocast("cuda", torch.float16):
        out = net.forward_differentiable(c, norm=norm)
    return c, out


def step(norm):
    for p in stack:
        p.grad = None
    c, out = forward(norm)
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
    return sum(ts) / len(ts), min(ts), max(ts)


def peak(norm):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(norm)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


for _ in range(WARMUP):
    gt_ = step("torch")
    gw_t = [p.grad.clone() for p in stack]
    gh = step("hip")
    gw_h = [p.grad.clone() for p in stack]
torch.cuda.synchronize()
diff_in = float((gt_.float() - gh.float()).abs().max() / gt_.float().abs().max())
diff_w = max(float((a.float() - b.float()).abs().max() / a.float().abs().max()) for a, b in zip(gw_t, gw_h))
del gt_, gh, gw_t, gw_h
tt, th = [], []
for rep in range(REPEATS):
    for norm in (("torch", "hip") if rep % 2 == 0 else ("hip", "torch")):
        (th if norm == "hip" else tt).append(timed(lambda: step(norm))[0])
mem_t, mem_h = peak("torch"), peak("hip")

# the HIP arm's kernels, by the library's own events
names = ["conv3_f16", "conv3_wgrad", "bn3_stats", "bn3_apply", "bn3_bwd"]
_lib.profile_select(names)
_lib.profile_reset()
_lib.profile_enable(True)
step("hip")
torch.cuda.synchronize()
_lib.profile_enable(False)
k = {n: _lib.profile_read(n) for n in names}
_lib.profile_select(None)
(tm, tlo, thi), (hm, hlo, hhi) = stats(tt), stats(th)
print(f"torch_ms mean/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} peak_MB={mem_t:.0f}", flush=True)
print(f"hip_ms   mean/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} peak_MB={mem_h:.0f}", flush=True)
total = sum(v[0] for v in k.values())
print("hip_kernels_ms " + " ".join(f"{n}={k[n][0]:.3f} ({k[n][1]} launches)" for n in names) +
      f" torch_remainder={hm - total:.3f} (of the mean step)", flush=True)
# 11 normalised layers: 4 of them add a residual (dres1..4's second)
model = {"bn3_stats": 11 * 1, "bn3_apply": 7 * 2 + 4 * 3, "bn3_bwd": 11 * 5}
for n, tensors in model.items():
    ms, launches = k[n]
    gbs = tensors * T / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    print(f"{n}: {ms / max(launches, 1):.4f} ms per launch, modelled traffic {tensors * T / 1e6:.0f} MB in {launches} "
          f"launches, achieved {gbs:.0f} GB/s = {gbs / STORE_PROBE_GBS:.2f} x the store probe's {STORE_PROBE_GBS:.0f} GB/s",
          flush=True)
print(f"hip/torch={hm / tm:.3f} hip_max_below_torch_min={hhi < tlo} grad_input_max_abs_diff_over_max_abs={diff_in:.3e} "
      f"grad_weight_worst={diff_w:.3e}", flush=True)
