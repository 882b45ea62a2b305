"""Same-process A/B of forward + backward of PSNet's full-resolution refinement
stack (dep_convs; PSNet.py:53-61, 218-221, cfg.PSNET_DEP_CONTEXT) at the KITTI
shape (B = 1, 376 x 1242, features 94 x 311), training mode, float16 autocast:

  torch  PSNet.forward's torch route: feat.float(), the full-resolution fp32 F.interpolate, the 36-channel
         fp32 cat, net.dep_convs as the nn.Conv2d modules (MIOpen), + depth: today's differentiable route
  hip    sfm_amd.context.dep_context_refine_autograd: sfm_dep_context_pack_f16 and seven sfm_conv2_f16
         forward; sfm_conv2_wgrad_f16, sfm_conv2_dgrad_f16 and sfm_dep_context_unpack_grad_f16 backward
         (csrc/context_bwd.hip)

HIP-event time of forward plus backward into the seven weights, feat and depth,
arms alternating, WARMUP warm-ups, then median / min / max of REPEATS repeats
per arm (ms per step); the spread of an arm is (max - min) / median.  Peak
memory is torch.cuda.max_memory_allocated over one step of the arm, above what
the inputs and parameters hold.  The HIP arm is timed once more with the
library's own events (conv2 forward, conv2_dgrad, conv2_wgrad, pack,
unpack-grad) and the remainder of the step is torch's (casts, the ReLU mask of
the last stage, the adds, allocation).  Then the unpack-grad kernel is timed on
its own against its modelled floor: five of the eight 16-byte channel chunks of
the first stage's gradient read once plus the float32 feature gradient written
once, at 6.3 TB/s.  The first line carries the hash of the kernel sources the
run was built from (bench.src_hash).  One process, one stream: it needs no more
than the default 4 hardware queues and sets no thread count.  Run it under a
time limit of its own, e.g.
  timeout -k 10 600 python scripts/dep_context_bwd_ab.py && <next GPU step>
Usage: dep_context_bwd_ab.py [REPEATS=8] [WARMUP=2]"""
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import torch.nn as nn
import torch.nn.functional as F
import bench
from sfm_amd import _lib, context, synth
from sfm_amd.config import defaults
from sfm_amd.psnet import PSNet

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
HBM_TBS = 6.3                                   # achievable HBM bandwidth of an MI355X, TB/s
dev = torch.device("cuda", 0)
B, H, W = 1, 376, 1242
h, w = synth.feature_hw()

cfg = defaults()
cfg.update(PSNET_DEP_CONTEXT=True)
torch.manual_seed(3)
net = PSNet(8, 1.0, cfg=cfg, feature_fn=nn.Conv2d(3, 32, 4, stride=4)).to(dev).train()
gen = torch.Generator().manual_seed(5)
feat0 = torch.randn(B, 32, h, w, generator=gen).half().to(dev)      # float16, as the feature CNN gives under autocast
depth0 = (1.0 + 9.0 * torch.rand(B, 1, H, W, generator=gen)).to(dev)
image0 = torch.rand(B, 3, H, W, generator=gen).to(dev)
gout = torch.randn(B, 1, H, W, generator=gen).to(dev)
params = list(net.dep_convs.parameters())
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, {H} x {W}, features {h} x {w}; "
      f"{REPEATS} alternating repeats after {WARMUP} warm-ups; one box, the box-to-box spread is not measured",
      flush=True)


def forward(hip):
    f = feat0.detach().requires_grad_()
    d = depth0.detach().requires_grad_()
    with torch.autocast("cuda", torch.float16):
        if hip:
            out = context.dep_context_refine_autograd(net.dep_convs, d, f, image0)
        else:
            # PSNet.forward's own lines
            up = F.interpolate(f.float(), [H, W], mode="bilinear", align_corners=True)
            out = net.dep_convs(torch.cat((d.detach(), up, image0.float()), dim=1)) + d
    return f, d, out


def step(hip):
    for q in params:
        q.grad = None
    f, d, out = forward(hip)
    out.float().backward(gout)
    return f.grad, d.grad


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    med = statistics.median(ts)
    return med, min(ts), max(ts), (max(ts) - min(ts)) / med


def peak(hip):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(hip)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / a.float().abs().max())


for _ in range(WARMUP):
    gt_ = step(False)
    gw_t = [q.grad.clone() for q in params]
    gh = step(True)
    gw_h = [q.grad.clone() for q in params]
torch.cuda.synchronize()
diff_feat, depth_same = rel(gt_[0], gh[0]), bool(torch.equal(gt_[1], gh[1]))
diff_w = max(rel(a, b) for a, b in zip(gw_t, gw_h))
del gt_, gh, gw_t, gw_h
tt, th = [], []
for rep in range(REPEATS):
    for hip in ((False, True) if rep % 2 == 0 else (True, False)):
        (th if hip else tt).append(timed(lambda: step(hip))[0])
mem_t, mem_h = peak(False), peak(True)

# the HIP arm's kernels, by the library's own events
NAMES = ["context_conv2", "conv2_dgrad", "conv2_wgrad", "dep_context_pack", "dep_context_unpack_grad"]
_lib.profile_select(NAMES)
_lib.profile_reset()
_lib.profile_enable(True)
step(True)
torch.cuda.synchronize()
_lib.profile_enable(False)
k = {n: _lib.profile_read(n) for n in NAMES}
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
ksum = sum(v[0] for v in k.values())
print(f"torch_ms median/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} peak_MB={mem_t:.0f}", flush=True)
print(f"hip_ms   median/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} peak_MB={mem_h:.0f}", flush=True)
print("hip_kernels_ms " + " ".join(f"{n}={v[0]:.3f} ({v[1]} launches)" for n, v in k.items()) +
      f" torch_remainder={hm - ksum:.3f} (of the median step)", flush=True)
print(f"hip/torch={hm / tm:.3f} hip_max_below_torch_min={hhi < tlo} torch_max_below_hip_min={thi < hlo} "
      f"grad_feat_max_abs_diff_over_max_abs={diff_feat:.3e} grad_depth_bit_equal={depth_same} "
      f"grad_weight_worst={diff_w:.3e}", flush=True)
print(f"wgrad/forward={k['conv2_wgrad'][0] / k['context_conv2'][0]:.2f} "
      f"dgrad/forward={k['conv2_dgrad'][0] / k['context_conv2'][0]:.2f} (the step's kernels, summed over the stages)",
      flush=True)

# the unpack-grad kernel on its own against its modelled floor
g0 = (torch.randn(B, H, W, 64, generator=gen) * 0.01).half().to(dev)
gf = torch.empty(B, 32, h, w, dtype=torch.float32, device=dev)
for _ in range(3):
    context.dep_context_unpack_grad(g0, 0, gf)
_lib.profile_select(["dep_context_unpack_grad"])
_lib.profile_reset()
_lib.profile_enable(True)
ts = []
for _ in range(10):
    before = _lib.profile_read("dep_context_unpack_grad")[0]
    context.dep_context_unpack_grad(g0, 0, gf)
    torch.cuda.synchronize()
    ts.append(_lib.profile_read("dep_context_unpack_grad")[0] - before)
_lib.profile_enable(False)
_lib.profile_select(None)
read_mb, write_mb = B * H * W * 5 * 16 / 1e6, B * 32 * h * w * 4 / 1e6
floor_ms = (read_mb + write_mb) / 1e6 / HBM_TBS * 1e3
um, ulo, uhi, _ = stats(ts)
print(f"dep_context_unpack_grad alone: median/min/max={um:.4f}/{ulo:.4f}/{uhi:.4f} ms; modelled floor "
      f"{floor_ms:.4f} ms ({read_mb:.1f} MB read + {write_mb:.1f} MB written at {HBM_TBS} TB/s); "
      f"measured/floor={um / floor_ms:.1f}", flush=True)
