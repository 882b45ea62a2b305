"""Same-process A/B of the channels-last sweep with float16 features in hand
(what SFMnet holds under cfg.MIXED_PREC): KITTI features 94 x 311, C = 32,
L = 128, B = 1 and 4, outputs f16 and f32.

  parent  the two .float() casts, then sfm_plane_sweep_cl (k_tgt_quads + k_sweep_cl)
  new     sfm_plane_sweep_cl_f16 on the features as they come (k_tgt_octets + k_sweep_cl, octet form)

Per cell: HIP-event time of the whole call (casts included), arms alternating,
WARMUP warm-ups, then median / min / max of REPEATS repeats per arm (ms); the
spread of an arm is (max - min) / median.  The two volumes must be bit-equal
(torch.equal on integer views).  Peak allocation of each arm from a pass of
its own (output and workspace allocated inside the call, as the depth stage
does).  Per-kernel times from the library's event profiler, 10 launches.
Usage: sweep_cl_f16feat_ab.py [REPEATS=24] [WARMUP=4]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
from sfm_amd import _lib, synth
from sfm_amd import sweep as SW

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 24
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 4
assert REPEATS >= 24
dev = torch.device("cuda", 0)
C, L, h, w = 32, 128, 94, 311
IVIEW = {torch.float16: torch.int16, torch.float32: torch.int32}
SCOPES = ("sweep_tgt_quads", "plane_sweep_cl", "sweep_tgt_octets", "plane_sweep_cl_f16")


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def kernel_ms(fn):
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    return {k: (lambda ms, n: ms / n if n else None)(*_lib.profile_read(k)) for k in SCOPES}


print(f"# device {torch.cuda.get_device_name(0)}; {h} x {w}, C = {C}, L = {L}; {REPEATS} alternating repeats after "
      f"{WARMUP} warm-ups; sweep_f16_feat default {_lib.tune_get('sweep_f16_feat')}", flush=True)
verdict = []
for B in (1, 4):
    _, K, pose, _ = synth.kitti_pair_batch(B, seed=1000, device=dev)
    ref32, tgt32 = synth.features(B, C, h, w, device=dev)
    ref16, tgt16 = ref32.half(), tgt32.half()
    del ref32, tgt32
    K4, Ki4 = SW.quarter_intrinsics(K, torch.inverse(K))
    P = pose[:, :3, :4].float().contiguous().to(dev)
    ws = SW.workspace_for(B, C, h, w, dev)
    for dtype, name in ((torch.float16, "f16"), (torch.float32, "f32")):
        out_p = torch.empty(B, L, h, w, 2 * C, device=dev, dtype=dtype)
        out_n = torch.empty_like(out_p)

        def parent(out=out_p, workspace=ws):
            return SW.plane_sweep_cost_channels_last(ref16.float(), tgt16.float(), P, K4, Ki4, L, 1.0, dtype=dtype,
                                                     out=out, workspace=workspace)

        def new(out=out_n, workspace=ws):
            return SW.plane_sweep_cost_channels_last(ref16, tgt16, P, K4, Ki4, L, 1.0, dtype=dtype, out=out,
                                                     workspace=workspace)
        out_p.fill_(float("nan"))
        out_n.fill_(float("nan"))
        for _ in range(WARMUP):
            parent()
            new()
        torch.cuda.synchronize()
        equal = torch.equal(out_p.view(IVIEW[dtype]), out_n.view(IVIEW[dtype]))
        tp, tn = [], []
        for r in range(REPEATS):
            if r % 2 == 0:
                tp.append(timed(parent))
                tn.append(timed(new))
            else:
                tn.append(timed(new))
                tp.append(timed(parent))
        kp, kn = kernel_ms(parent), kernel_ms(new)
        assert kp["plane_sweep_cl_f16"] is None and kn["plane_sweep_cl"] is None      # each arm ran its own kernels
        del out_p, out_n
        mp = peak_mb(lambda: parent(None, None))
        mn = peak_mb(lambda: new(None, None))
        (pm, plo, phi, psp), (nm, nlo, nhi, nsp) = stats(tp), stats(tn)
        not_slower = nm <= pm * (1.0 + psp)
        verdict.append((B, name, not_slower))
        print(f"B={B} {name} parent_ms med/min/max={pm:.4f}/{plo:.4f}/{phi:.4f} spread={psp:.3f} "
              f"k_tgt_quads={kp['sweep_tgt_quads']:.4f} k_sweep_cl={kp['plane_sweep_cl']:.4f} "
              f"peak_allocated_MB={mp:.1f}", flush=True)
        print(f"B={B} {name} new_ms    med/min/max={nm:.4f}/{nlo:.4f}/{nhi:.4f} spread={nsp:.3f} "
              f"k_tgt_octets={kn['sweep_tgt_octets']:.4f} k_sweep_cl_f16={kn['plane_sweep_cl_f16']:.4f} "
              f"peak_allocated_MB={mn:.1f} bit_equal={equal} new/parent={nm / pm:.3f} "
              f"not_slower_beyond_parent_spread={not_slower}", flush=True)
        assert equal, "the two arms' volumes differ"
ok = all(v for B, name, v in verdict if name == "f16")
print(f"# default rule (every f16-output cell not slower than the parent beyond the parent's spread): "
      f"sweep_f16_feat = {1 if ok else 0}", flush=True)
