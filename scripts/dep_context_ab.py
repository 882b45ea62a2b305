"""Same-process A/B of PSNet's full-resolution depth refinement (dep_convs,
models/PSNet.py:218-221, cfg.PSNET_DEP_CONTEXT) at the KITTI shape (B = 1,
image 376 x 1242, feature map 94 x 311) under float16 autocast:

  torch  features.float(), F.interpolate, torch.cat, net.dep_convs (MIOpen), "+ depth", as PSNet.forward
         runs it with dep_context_precision="torch"
  hip    sfm_amd.context.dep_context_refine (sfm_dep_context_pack_f16 + 7 x sfm_conv2_f16 per chunk of pairs)

HIP-event time of the whole call, arms alternating, WARMUP warm-ups, then
median / min / max of REPEATS repeats per arm (ms per pair); the spread of an
arm is (max - min) / median.  The HIP arm's rate is the stack's algorithmic
work (520,992 MAC per pixel, the 36-channel first layer unpadded) over its
median time, as a fraction of the 2.5 PFLOP/s dense f16 peak; its pack
kernel's time is reported on its own, with the rate of its 128 bytes per pixel
of writes.  The two arms' outputs are compared (max-abs difference over
max-abs).  The first line carries the hash of the kernel sources the run was
built from (bench.src_hash).  Usage: dep_context_ab.py [REPEATS=12] [WARMUP=3]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import torch.nn.functional as F
import bench
from sfm_amd import _lib, synth
from sfm_amd.config import defaults
from sfm_amd.context import dep_context_refine, pairs_per_chunk
from sfm_amd.psnet import PSNet

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)
B, H, W, h, w = 1, 376, 1242, 94, 311
MAC = sum(9 * a * b for a, b in ((36, 128), (128, 128), (128, 128), (128, 96), (96, 64), (64, 32), (32, 1)))
assert MAC == 520992
FLOP = 2.0 * MAC * B * H * W
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
c.update(MIXED_PREC=True, PSNET_DEP_CONTEXT=True)
torch.manual_seed(1)
net = PSNet(8, 1.0, cfg=c, feature_fn=lambda img: img).to(dev).eval()
g = torch.Generator().manual_seed(3)
fea = synth.features(B, 32, h, w, seed=2, device=dev)[0].half()
depth = (1.0 + 79.0 * torch.rand(B, 1, H, W, generator=g)).to(dev)
image = torch.rand(B, 3, H, W, generator=g).to(dev)
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, {H} x {W}, features "
      f"{h} x {w}; {FLOP / 1e12:.3f} TFLOP per pair; {REPEATS} alternating repeats after {WARMUP} warm-ups; "
      f"pairs per chunk {pairs_per_chunk(B, H, W, 1 << 30)}", flush=True)


def arm_torch():
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        up = F.interpolate(fea.float(), [H, W], mode="bilinear", align_corners=True)
        return net.dep_convs(torch.cat((depth.detach(), up, image.float()), dim=1)) + depth


def arm_hip():
    return dep_context_refine(net.dep_convs, depth, fea, image)


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
kc, kp = _lib.profile_read("context_conv2"), _lib.profile_read("dep_context_pack")
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
faster = hm < tm * (1.0 - tsp) and hm < tm * (1.0 - hsp)
print(f"torch_ms med/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} "
      f"TFLOPs={FLOP / tm / 1e9:.1f}", flush=True)
print(f"hip_ms   med/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} "
      f"TFLOPs={FLOP / hm / 1e9:.1f} fraction_of_f16_peak={FLOP / (hm * 1e-3) / PEAK:.4f} "
      f"conv2_ms={kc[0]:.3f}/{kc[1]} launches pack_ms={kp[0]:.3f}/{kp[1]} launches "
      f"pack_write_GBps={(B * H * W * 128 / (kp[0] * 1e-3) / 1e9) if kp[0] > 0 else 0.0:.0f}", flush=True)
print(f"hip/torch={hm / tm:.3f} max_abs_diff_over_max_abs={diff:.3e} "
      f"hip_faster_beyond_both_spreads={faster}", flush=True)
print(f"# default rule (HIP faster than MIOpen by more than both arms' spreads): "
      f"dep_context_precision 'auto' -> {'fp16' if faster else 'torch'} under float16 autocast", flush=True)
