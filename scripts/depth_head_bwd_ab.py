"""Same-process A/B of the soft-argmin head's forward + backward at the KITTI
shape (B = 1, L = 128, cost 94 x 311 -> depth 376 x 1242, float32):

  hip    depth_head_autograd: sfm_depth_head, then sfm_depth_head_backward (csrc/depth_bwd.hip)
  torch  F.interpolate(trilinear), softmax, the disparity regression and autograd's backward
         (sfm_amd.psnet.torch_depth_head), float32 on the GPU

HIP-event time of forward plus backward, arms alternating, WARMUP warm-ups,
then median / min / max of REPEATS repeats per arm (ms per head); the spread of
an arm is (max - min) / median.  Peak memory is torch.cuda.max_memory_allocated
over one forward + backward of the arm, above what the inputs hold.  The two
arms' gradients are compared (max-abs difference over the max-abs).  The HIP
arm's kernels are timed once more with the library's own events.  The first
line carries the hash of the kernel sources the run was built from
(bench.src_hash).
Usage: depth_head_bwd_ab.py [REPEATS=12] [WARMUP=3]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import bench
from sfm_amd import _lib, synth
from sfm_amd.depth import depth_head_autograd
from sfm_amd.psnet import torch_depth_head

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)
B, L = 1, 128
H, W = synth.KITTI_HW
h, w = synth.feature_hw()
MIN_DEPTH = 1.0


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


gen = torch.Generator().manual_seed(5)
# classify-like logits: O(100) between planes
cost = (100.0 * torch.randn(B, L, h, w, generator=gen)).to(dev)
g = torch.randn(B, 1, H, W, generator=gen).to(dev)
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, L = {L}, {h} x {w} -> {H} x {W}; "
      f"cost {cost.numel() * 4 / 1e6:.1f} MB, upsampled volume {B * L * H * W * 4 / 1e6:.0f} MB; "
      f"{REPEATS} alternating repeats after {WARMUP} warm-ups", flush=True)


def step(head):
    c = cost.detach().requires_grad_()
    head(c, L, MIN_DEPTH, (H, W)).backward(g)
    return c.grad


def arm_hip():
    return timed(lambda: step(depth_head_autograd))


def arm_torch():
    return timed(lambda: step(torch_depth_head))


def peak(arm):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    arm()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


for _ in range(WARMUP):
    _, gt_ = arm_torch()
    _, gh = arm_hip()
torch.cuda.synchronize()
diff = float((gt_ - gh).abs().max() / gt_.abs().max())
del gt_, gh
tt, th = [], []
for rep in range(REPEATS):
    if rep % 2 == 0:
        tt.append(arm_torch()[0])
        th.append(arm_hip()[0])
    else:
        th.append(arm_hip()[0])
        tt.append(arm_torch()[0])
mem_t, mem_h = peak(arm_torch), peak(arm_hip)
_lib.profile_select(None)
_lib.profile_reset()
_lib.profile_enable(True)
arm_hip()
torch.cuda.synchronize()
_lib.profile_enable(False)
kf, ks, kb = (_lib.profile_read(n)[0] for n in ("depth_head", "depth_head_bwd_stats", "depth_head_bwd"))
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
print(f"torch_ms med/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} peak_MB={mem_t:.1f}", flush=True)
print(f"hip_ms   med/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} peak_MB={mem_h:.1f} "
      f"kernels_ms forward={kf:.3f} bwd_stats={ks:.3f} bwd_gather={kb:.3f}", flush=True)
print(f"hip/torch={hm / tm:.3f} hip_max_below_torch_min={hhi < tlo} max_abs_diff_over_max_abs={diff:.3e}", flush=True)
