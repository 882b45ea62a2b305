"""Same-process A/B of the plane sweep's backward at the KITTI shape
(B = 1, C = 32, L = 128, feature map 94 x 311, float32):

  torch  autograd's backward of the same [B, 2C, L, h, w] volume built on the GPU from the per-plane
         F.grid_sample loop (planes stacked, reference rows an expand: no in-place slice copies), into both
         feature maps
  hip    one sfm_plane_sweep_backward call (grad_ref and grad_tgt; csrc/sweep_bwd.hip)

HIP-event time of the whole backward, arms alternating, WARMUP warm-ups, then
median / min / max of REPEATS repeats per arm (ms per pair); the spread of an
arm is (max - min) / median.  The two arms' gradients are compared (max-abs
difference over the RMS).  The HIP arm's kernels are timed once more with the
library's own events.  The first line carries the hash of the kernel sources
the run was built from (bench.src_hash).
Usage: sweep_bwd_ab.py [REPEATS=12] [WARMUP=3] [hip_only=0]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import torch.nn.functional as F
import bench
from oracle import sweep as S
from sfm_amd import _lib, synth
from sfm_amd.sweep import backward_workspace_for, quarter_intrinsics

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
HIP_ONLY = len(sys.argv) > 3 and sys.argv[3] == "1"
dev = torch.device("cuda", 0)
B, C, L = 1, 32, 128
h, w = synth.feature_hw()
MIN_DEPTH = 1.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    s = sorted(ts)
    med = s[len(s) // 2]
    return med, s[0], s[-1], (s[-1] - s[0]) / med


ref, tgt = (t.to(dev) for t in synth.features(B, C, h, w, seed=4))
K = synth.intrinsics(B)
K4, Ki4 = quarter_intrinsics(K, torch.inverse(K))
pose = synth.relative_pose(B, torch.Generator().manual_seed(9))
# the sampling grids of the planes (the reference's float32 expressions), made on the host once
grids = [S.warp_grid(torch.ones(B, h, w) * (MIN_DEPTH * L) / (i + 1), pose, K4, Ki4, h, w).to(dev) for i in range(L)]
g = torch.randn(B, 2 * C, L, h, w, generator=torch.Generator().manual_seed(3)).to(dev)
pose_d, K4_d, Ki4_d = pose.to(dev).contiguous(), K4.to(dev).contiguous(), Ki4.to(dev).contiguous()
ws = backward_workspace_for(B, C, h, w, L, dev)
grad_ref, grad_tgt = torch.empty_like(ref), torch.empty_like(tgt)
lib = _lib.load()
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, C = {C}, L = {L}, {h} x {w}; "
      f"gradient volume {g.numel() * 4 / 1e6:.0f} MB; {REPEATS} alternating repeats after {WARMUP} warm-ups",
      flush=True)


def torch_graph():
    r, t = ref.clone().requires_grad_(), tgt.clone().requires_grad_()
    warped = torch.stack([F.grid_sample(t, grids[i], mode="bilinear", padding_mode="zeros", align_corners=True)
                          for i in range(L)], 2)
    return r, t, torch.cat([r.unsqueeze(2).expand(B, C, L, h, w), warped], 1)


def arm_torch():
    r, t, cost = torch_graph()
    torch.cuda.synchronize()
    ms = timed(lambda: cost.backward(g))
    return ms, r.grad, t.grad


def hip_call():
    _lib.check(lib.sfm_plane_sweep_backward(_lib.ptr(g), 0, B, C, h, w, _lib.ptr(pose_d), _lib.ptr(K4_d),
                                            _lib.ptr(Ki4_d), L, MIN_DEPTH, 0, _lib.ptr(grad_ref), _lib.ptr(grad_tgt),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
               "sfm_plane_sweep_backward")


def arm_hip():
    return timed(hip_call), grad_ref, grad_tgt


if HIP_ONLY:
    for _ in range(WARMUP + REPEATS):
        arm_hip()
    torch.cuda.synchronize()
    print(f"hip_only {_lib.last_sweep()} ran {WARMUP + REPEATS} times", flush=True)
    sys.exit(0)

for _ in range(WARMUP):
    _, tr, tt_ = arm_torch()
    _, hr, ht = arm_hip()
torch.cuda.synchronize()
rms = float(tt_.double().pow(2).mean().sqrt())
diff_tgt = float((tt_ - ht).abs().max()) / rms
diff_ref = float((tr - hr).abs().max()) / float(tr.double().pow(2).mean().sqrt())
del tr, tt_
tt, th = [], []
for rep in range(REPEATS):
    if rep % 2 == 0:
        tt.append(arm_torch()[0])
        th.append(arm_hip()[0])
    else:
        th.append(arm_hip()[0])
        tt.append(arm_torch()[0])
_lib.profile_select(None)
_lib.profile_reset()
_lib.profile_enable(True)
hip_call()
torch.cuda.synchronize()
_lib.profile_enable(False)
kp, kr, kt = (_lib.profile_read(n)[0] for n in ("sweep_bwd_prep", "sweep_bwd_ref", "sweep_bwd"))
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
spread = max(tsp, hsp)
print(f"torch_ms med/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f}", flush=True)
print(f"hip_ms   med/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} form={_lib.last_sweep()} "
      f"kernels_ms prep={kp:.3f} grad_ref={kr:.3f} grad_tgt={kt:.3f} "
      f"grad_tgt_read_TBps={g.numel() * 2 / (kt * 1e-3) / 1e12:.2f}", flush=True)
print(f"hip/torch={hm / tm:.3f} max_abs_diff_over_rms grad_tgt={diff_tgt:.3e} grad_ref={diff_ref:.3e} "
      f"hip_faster_beyond_spread={hm < tm * (1.0 - spread)}", flush=True)
