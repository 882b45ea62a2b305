"""Times of the three float16 BatchNorm2d entry points (csrc/bn2.hip:
sfm_bn2_stats_f16, sfm_bn2_apply_f16, sfm_bn2_backward_f16) at the feature
CNN's own maps at batch 2 of a KITTI image: 2 x 188 x 621 x 32 (firstconv,
layer1), 2 x 94 x 311 x 64 (layer2) and 2 x 94 x 311 x 128 (layer3, layer4).

Training mode, ReLU on, with a residual: the widest form of each entry.  Per
map and entry WARMUP warm-up calls, then the median of REPEATS calls, each
timed by the library's own events (the profile scopes bn2_stats, bn2_apply,
bn2_bwd).  Each time is set against the entry's modelled traffic in tensors T
of the map's size -- statistics 1 T read; apply 2 T read (x and the residual) +
1 T write; backward 4 T read (x and grad_out, twice) + 1 T write -- over the
streaming-store probe's 4830 GB/s (profiles/r01_probe_store_bw.txt, row D).
These maps are 5 to 15 MB: they fit the 256 MB Infinity Cache, and a launch is a
few microseconds, so the ratio says how close a call is to the memory system's
rate at this size, not to HBM's.  No torch arm: torch's batch_norm on these
tensors is the call this route replaces.  One process, one stream.  Run it
under a time limit of its own, e.g.
  timeout -k 10 300 python scripts/bn2_time.py > profiles/bn2_kernels.txt
Usage: bn2_time.py [REPEATS=12] [WARMUP=3]"""
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import bench
from sfm_amd import _lib
from sfm_amd.feature import bn2_apply_f16, bn2_backward_f16, bn2_stats_f16

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
STORE_PROBE_GBS = 4830.4                      # profiles/r01_probe_store_bw.txt, row D (float4 nt flat stream)
MAPS = [(2, 188, 621, 32), (2, 94, 311, 64), (2, 94, 311, 128)]
dev = torch.device("cuda", 0)
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; training mode, relu, residual; median of "
      f"{REPEATS} calls after {WARMUP} warm-ups, by the library's events; one box, the box-to-box spread is not measured",
      flush=True)


def timed(scope, fn):
    ms = []
    for i in range(WARMUP + REPEATS):
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        ms.append(_lib.profile_read(scope)[0])
    return statistics.median(ms[WARMUP:]), min(ms[WARMUP:]), max(ms[WARMUP:])


gen = torch.Generator().manual_seed(7)
_lib.profile_select(["bn2_stats", "bn2_apply", "bn2_bwd"])
_lib.profile_enable(True)
try:
    for shape in MAPS:
        C = shape[3]
        x = torch.randn(shape, generator=gen).half().to(dev)
        res = torch.randn(shape, generator=gen).half().to(dev)
        gout = torch.randn(shape, generator=gen).half().to(dev)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        st = bn2_stats_f16(x, gamma, beta, 1e-5, rm, rv, 0.1, True)
        T = x.numel() * 2
        rows = [("bn2_stats", 1, lambda: bn2_stats_f16(x, gamma, beta, 1e-5, rm, rv, 0.1, True)),
                ("bn2_apply", 3, lambda: bn2_apply_f16(x, st, res, True)),
                ("bn2_bwd", 5, lambda: bn2_backward_f16(x, gout, st, True, True))]
        for scope, tensors, fn in rows:
            med, lo, hi = timed(scope, fn)
            gbs = tensors * T / (med * 1e-3) / 1e9
            print(f"map={'x'.join(map(str, shape))} T_MB={T / 1e6:.2f} entry={scope} ms median/min/max="
                  f"{med:.4f}/{lo:.4f}/{hi:.4f} modelled={tensors}T achieved_GBs={gbs:.0f} "
                  f"x_probe={gbs / STORE_PROBE_GBS:.2f}", flush=True)
finally:
    _lib.profile_enable(False)
    _lib.profile_select(None)
