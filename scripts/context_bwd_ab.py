"""Same-process A/B of forward + backward of PSNet's per-plane context stack
(convs; PSNet.py:17-26, 64-71, 175-190) at the KITTI shape (B = 1, L = 128,
94 x 311), training mode, float16 autocast:

  torch  net.convs as the nn.Conv2d modules on the B L images (MIOpen): today's differentiable route
  hip    sfm_amd.context.context_refine_autograd: sfm_context_pack_f16 and seven sfm_conv2_f16 forward;
         sfm_conv2_wgrad_f16, sfm_conv2_dgrad_f16 and sfm_context_unpack_grad_f16 backward
         (csrc/context_bwd.hip)

HIP-event time of forward plus backward into the seven weights, ctx and costs,
arms alternating, WARMUP warm-ups, then mean / min / max of REPEATS repeats per
arm (ms per step); the spread of an arm is (max - min) / mean.  Peak memory is
torch.cuda.max_memory_allocated over one step of the arm, above what the inputs
and parameters hold.  The HIP arm is timed once more with the library's own
events (conv2 forward, conv2_dgrad, conv2_wgrad, pack / unpack) and the
remainder of the step is torch's (casts, the ReLU mask of the last stage, the
adds, allocation).  Then every stage's three kernels are timed on their own at
the step's shape: the weight gradient's modelled floor is the stage's forward
time (the same FLOPs), and the table gives the measured multiple of it.  The
first line carries the hash of the kernel sources the run was built from
(bench.src_hash).  One process, one stream: it needs no more than the default 4
hardware queues and sets no thread count.  Run it under a time limit of its
own, e.g.
  timeout -k 10 900 python scripts/context_bwd_ab.py && <next GPU step>
Usage: context_bwd_ab.py [REPEATS=8] [WARMUP=2]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-sfm-revisited_amd"))
import torch
import torch.nn as nn
import bench
from sfm_amd import _lib, context, synth
from sfm_amd.psnet import PSNet

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dev = torch.device("cuda", 0)
B, L = 1, 128
h, w = synth.feature_hw()

torch.manual_seed(3)
net = PSNet(L, 1.0, feature_fn=nn.Conv2d(3, 32, 4, stride=4)).to(dev).train()
gen = torch.Generator().manual_seed(5)
ctx0 = torch.randn(B, 32, h, w, generator=gen).to(dev)
costs0 = torch.randn(B, 1, L, h, w, generator=gen).to(dev)
gout = torch.randn(B, 1, L, h, w, generator=gen).to(dev)
params = list(net.convs.parameters())
print(f"# device {torch.cuda.get_device_name(0)}; src_hash {bench.src_hash()}; B = {B}, L = {L}, {h} x {w}; "
      f"{REPEATS} alternating repeats after {WARMUP} warm-ups; one box, the box-to-box spread is not measured",
      flush=True)


def forward(hip):
    c = ctx0.detach().requires_grad_()
    p = costs0.detach().requires_grad_()
    with torch.autocast("cuda", torch.float16):
        if hip:
            out = context.context_refine_autograd(net.convs, c, p)
        else:
            # PSNet.forward's own application of the modules: one batch of L B images
            planes = p[:, 0].permute(1, 0, 2, 3).reshape(L * B, 1, h, w)
            x = torch.cat([c.unsqueeze(0).expand(L, B, 32, h, w).reshape(L * B, -1, h, w), planes], 1)
            out = (net.convs(x) + planes).reshape(L, B, h, w).permute(1, 0, 2, 3).unsqueeze(1)
    return c, p, out


def step(hip):
    for q in params:
        q.grad = None
    c, p, out = forward(hip)
    out.float().backward(gout)
    return c.grad, p.grad


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    mean = sum(ts) / len(ts)
    return mean, min(ts), max(ts), (max(ts) - min(ts)) / mean


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
diff_ctx, diff_costs = rel(gt_[0], gh[0]), rel(gt_[1], gh[1])
diff_w = max(rel(a, b) for a, b in zip(gw_t, gw_h))
del gt_, gh, gw_t, gw_h
tt, th = [], []
for rep in range(REPEATS):
    for hip in ((False, True) if rep % 2 == 0 else (True, False)):
        (th if hip else tt).append(timed(lambda: step(hip))[0])
mem_t, mem_h = peak(False), peak(True)

# the HIP arm's kernels, by the library's own events
NAMES = ["context_conv2", "conv2_dgrad", "conv2_wgrad", "context_pack", "context_unpack_grad"]
_lib.profile_select(NAMES)
_lib.profile_reset()
_lib.profile_enable(True)
step(True)
torch.cuda.synchronize()
_lib.profile_enable(False)
k = {n: _lib.profile_read(n) for n in NAMES}
(tm, tlo, thi, tsp), (hm, hlo, hhi, hsp) = stats(tt), stats(th)
ksum = sum(v[0] for v in k.values())
print(f"torch_ms mean/min/max={tm:.3f}/{tlo:.3f}/{thi:.3f} spread={tsp:.3f} peak_MB={mem_t:.0f}", flush=True)
print(f"hip_ms   mean/min/max={hm:.3f}/{hlo:.3f}/{hhi:.3f} spread={hsp:.3f} peak_MB={mem_h:.0f}", flush=True)
print("hip_kernels_ms " + " ".join(f"{n}={v[0]:.3f} ({v[1]} launches)" for n, v in k.items()) +
      f" torch_remainder={hm - ksum:.3f} (of the mean step)", flush=True)
print(f"hip/torch={hm / tm:.3f} hip_max_below_torch_min={hhi < tlo} grad_ctx_max_abs_diff_over_max_abs={diff_ctx:.3e} "
      f"grad_costs={diff_costs:.3e} grad_weight_worst={diff_w:.3e}", flush=True)

# every stage's three kernels on their own, at the step's shape
packed = context.pack_context_stack(net.convs, dev, "fp16")
n_img = B * L


def kernel_ms(name, fn, reps=3):
    fn()
    _lib.profile_select([name])
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ms, launches = _lib.profile_read(name)
    return ms / max(launches, 1)


tot = [0.0, 0.0, 0.0]
for i, (lay, conv) in enumerate(zip(packed, (blk[0] for blk in net.convs))):
    cip, cop, d = lay["cin_pad"], lay["cout_pad"], lay["dilation"]
    x = torch.randn(n_img, h, w, cip, generator=gen).half().to(dev).relu_()
    g = (torch.randn(n_img, h, w, cop, generator=gen) * 0.01).half().to(dev)
    wd = context.pack_dgrad_weights2(conv.weight.detach().float()).half().contiguous()
    fwd = kernel_ms("context_conv2", lambda: context.conv2_f16(x, lay["w"], lay["scale"], lay["bias"], d, True,
                                                               lay["cout"]))
    dg = kernel_ms("conv2_dgrad", lambda: context.conv2_dgrad_f16(g, wd, d, x))
    wg = kernel_ms("conv2_wgrad", lambda: context.conv2_wgrad_f16(x, g, d))
    tot = [tot[0] + fwd, tot[1] + dg, tot[2] + wg]
    print(f"stage{i} {cip}->{lay['cout']} d{d}: forward_ms={fwd:.3f} dgrad_ms={dg:.3f} wgrad_ms={wg:.3f} "
          f"wgrad/forward={wg / fwd:.2f} (the modelled floor: the same FLOPs)", flush=True)
    del x, g
print(f"stages_total forward_ms={tot[0]:.3f} dgrad_ms={tot[1]:.3f} wgrad_ms={tot[2]:.3f} "
      f"wgrad/forward={tot[2] / tot[0]:.2f}", flush=True)
_lib.profile_select(None)
