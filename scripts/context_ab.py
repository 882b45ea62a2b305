"""Same-process A/B of PSNet's per-plane context stack at the KITTI shape
(B = 1, L = 128, feature map 94 x 311) under float16 autocast:

  torch  net.convs on the B*L-image batch (MIOpen), plus the "+ plane", as PSNet.forward runs it
  hip    sfm_amd.context.context_refine (sfm_context_pack_f16 + 7 x sfm_conv2_f16 per chunk of planes)

HIP-event time of the whole call, arms alternating, WARMUP warm-ups, then
median / min / max of REPEATS repeats per arm (ms per pair); the spread of an
arm is (max - min) / median.  The HIP arm's rate is the stack's algorithmic
work (517,536 MAC per pixel and plane, the 33-channel first layer unpadded)
over its median time, as a fraction of the 2.5 PFLOP/s dense f16 peak.  The
two arms' outputs are compared (max-abs difference over max-abs).  The first
line carries the hash of the kernel sources the run was built from
(bench.src_hash).  Usage: context_ab.py [REPEATS=12] [WARMUP=3]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import bench
from sfm_amd import _lib, synth
from sfm_amd.config import defaults
from sfm_amd.context import context_refine, planes_per_chunk
from sfm_amd.psnet import PSNet

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)
B, L, h, w = 1, 128, 94, 311
MAC = sum(9 * a * b for a, b in ((33, 128), (128, 128), (128, 128), (128, 96), (96, 64), (64, 32), (32, 1)))
assert MAC == 517536
FLOP = 2.0 * MAC * B * L * h * w
PEAK = 2.5e15


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


c = defaults()
c.update(MIXED_PREC=True)
torch.manual_seed(1)
net = PSNet(L, 1.0, cfg=c, feature_fn=lambda img: img).to(dev).eval()
ctx = synth.features(B, 32, h, w, seed=2, device=dev)[0].half()
costs = torch.randn(B, 1, L, h, w, generator=torch.Generator().manual_seed(3)).to(dev)
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, L = {L}, {h} x {w}; "
      f"{FLOP / 1e12:.2f} TFLOP per pair; {REPEATS} alternating repeats after {WARMUP} warm-ups; "
      f"planes per chunk {planes_per_chunk(B, h, w, L, 1 << 30)}", flush=True)


def arm_torch():
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        f = ctx.float()
        planes = costs[:, 0].permute(1, 0, 2, 3).reshape(L * B, 1, h, w)
        x = torch.cat([f.unsqueeze(0).expand(L, B, 32, h, w).reshape(L * B, -1, h, w), planes], 1)
        return (net.convs(x) + planes).reshape(L, B, h, w).permute(1, 0, 2, 3).unsqueeze(1)


def arm_hip():
    return context_refine(net.convs, ctx, costs)


for _ in range(WARMUP):
    yt = arm_torch()
    yh = arm_hip()
torch.cuda.synchronize()
diff = float((yt - yh).abs().max() / yt.abs().max())
del yt, yh
tt, th = [], []
for r in range(REPEATS):
    if r % 2 == 0:
        tt.append(timed(arm_torch))
        th.append(timed(arm_hip))
    else:
        th.append(timed(arm_hip))
        tt.append(timed(arm_torch))
_lib.profile_select(None)
_lib.profile_reset()
_lib.profile_enable(True)
arm_hip()
torch.cuda.synchronize()
_lib.profile_enable(False)
kc, kp = _lib.profile_read("context_conv2"), _lib.profile_read("context_pack")
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
spread = max(tsp, hsp)
faster = hm < tm * (1.0 - spread)
print(f"torch_ms med/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} "
      f"TFLOPs={FLOP / tm / 1e9:.1f}", flush=True)
print(f"hip_ms   med/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} "
      f"TFLOPs={FLOP / hm / 1e9:.1f} fraction_of_f16_peak={FLOP / (hm * 1e-3) / PEAK:.4f} "
      f"conv2_ms={kc[0]:.3f}/{kc[1]} launches pack_ms={kp[0]:.3f}/{kp[1]} launches", flush=True)
print(f"hip/torch={hm / tm:.3f} max_abs_diff_over_max_abs={diff:.3e} "
      f"hip_faster_beyond_spread={faster}", flush=True)
print(f"# default rule (HIP faster than MIOpen by more than the larger spread): "
      f"context_precision 'auto' -> {'fp16' if faster else 'torch'} under float16 autocast", flush=True)
