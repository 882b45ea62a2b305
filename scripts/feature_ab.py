"""Same-process A/B of PSNet's feature CNN (models/submodule.py:108-184) at
the KITTI shape (a pair: 2 images of 376 x 1242, feature maps 94 x 311) under
float16 autocast:

  torch  net.feature_extraction(image) per image (MIOpen), as PSNet.forward runs it with
         feature_precision="torch"
  hip    sfm_amd.feature.feature_extract on both images as one batch (sfm_image_pack_f16, 61 x sfm_conv2x_f16,
         4 x sfm_avgpool_f16, sfm_spp_pack_f16 per chunk of images)

HIP-event time of the whole call, arms alternating, WARMUP warm-ups, then
median / min / max of REPEATS repeats per arm (ms per pair); the spread of an
arm is (max - min) / median.  The HIP arm's rate is the CNN's algorithmic work
(the 3-channel first layer unpadded) over its median time, as a fraction of
the 2.5 PFLOP/s dense f16 peak; its kernels' times are reported by kind.  The
two arms' outputs are compared (max-abs difference over max-abs).  The first
line carries the hash of the kernel sources the run was built from
(bench.src_hash).  Usage: feature_ab.py [REPEATS=12] [WARMUP=3]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import torch.nn as nn
import bench
from sfm_amd import _lib
from sfm_amd.feature import feature_extract, feature_hw, images_per_chunk
from sfm_amd.psnet import FeatureExtraction, _Residual

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)
B, H, W = 2, 376, 1242
h, w = feature_hw((H, W))
PEAK = 2.5e15


def conv_macs(net, image_hw):
    """MACs per image, from the output size of every Conv2d (hooks on one CPU run)."""
    total = [0]

    def hook(m, i, o):
        total[0] += o.shape[2] * o.shape[3] * m.out_channels * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        net(torch.zeros(1, 3, *image_hw))
    for x in hs:
        x.remove()
    return total[0]


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


torch.manual_seed(1)
net = FeatureExtraction().eval()
for m in net.modules():
    if isinstance(m, nn.Conv2d):
        nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    elif isinstance(m, _Residual):
        m.conv2[1].weight.data.fill_(0.25)      # keeps 25 "+ x" in a row inside float16
FLOP = 2.0 * conv_macs(net, (H, W)) * B
net = net.to(dev)
image = (torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; {B} images of {H} x {W}, features "
      f"{h} x {w}; {FLOP / 1e12:.3f} TFLOP per pair; {REPEATS} alternating repeats after {WARMUP} warm-ups; "
      f"images per chunk {images_per_chunk(B, H, W, 1 << 30)}", flush=True)


def arm_torch():
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        return torch.cat([net(image[:1]), net(image[1:])])


def arm_hip():
    return feature_extract(net, image)


for _ in range(WARMUP):
    yt = arm_torch()
    yh = arm_hip()
torch.cuda.synchronize()
assert bool(torch.isfinite(yt).all()) and bool(torch.isfinite(yh).all())
diff = float((yt.float() - yh.float()).abs().max() / yt.float().abs().max())
del yt, yh
tt, th = [], []
for r in range(REPEATS):
    if r % 2 == 0:
        tt.append(timed(arm_torch))
        th.append(timed(arm_hip))
    else:
        th.append(timed(arm_hip))
        tt.append(timed(arm_torch))
KINDS = ("feature_conv2x", "feature_image_pack", "feature_avgpool", "feature_spp_pack")
_lib.profile_select(None)
_lib.profile_reset()
_lib.profile_enable(True)
arm_hip()
torch.cuda.synchronize()
_lib.profile_enable(False)
kinds = " ".join(f"{k[8:]}_ms={_lib.profile_read(k)[0]:.3f}/{_lib.profile_read(k)[1]}" for k in KINDS)
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
faster = hm < tm * (1.0 - tsp) and hm < tm * (1.0 - hsp)
print(f"torch_ms med/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} "
      f"TFLOPs={FLOP / tm / 1e9:.1f}", flush=True)
print(f"hip_ms   med/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} "
      f"TFLOPs={FLOP / hm / 1e9:.1f} fraction_of_f16_peak={FLOP / (hm * 1e-3) / PEAK:.4f} "
      f"kernel time / launches: {kinds}", flush=True)
print(f"hip/torch={hm / tm:.3f} max_abs_diff_over_max_abs={diff:.3e} hip_median_below_torch_median={hm < tm} "
      f"hip_faster_beyond_both_spreads={faster}", flush=True)
print(f"# default rule (HIP arm's median below the torch arm's): "
      f"feature_precision 'auto' -> {'fp16' if hm < tm else 'torch'} under float16 autocast", flush=True)
