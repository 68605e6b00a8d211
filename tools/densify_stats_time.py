#!/usr/bin/env python3
"""What the screen-space densification statistics cost: on the config-3 scene at an orbit camera,
  * the two kernels alone, on device events: gsplat_densify_stats behind a raster backward (the frame's own project_state and
    grad2d, through ops internals) and gsplat_densify_stats_merge of a fully touched record;
  * the backward pass of a deferred frame (composite entries) without and inside ops.densify_stats;
  * Trainer.step with densify_rule "reference" and "screen" (one view, no densification inside the timed window).
Prints one JSON line (microseconds, medians).
    python tools/densify_stats_time.py [config] [iterations]
A kernel trace of the same run: rocprofv3 --kernel-trace --stats -- python tools/densify_stats_time.py"""
import ctypes as C
import importlib
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import bench
from oracle import scenes

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
ops = importlib.import_module(PKG + ".ops")
abi = importlib.import_module(PKG + "._abi")
model_mod = importlib.import_module(PKG + ".model")
training = importlib.import_module(PKG + ".training")
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
params, cam = bench.synthetic_scene(cfg)
dev = torch.device("cuda:0")
c2w = torch.tensor(scenes.orbit_c2w(1, 24), device=dev)
gimg = torch.rand(cam["H"], cam["W"], 3, device=dev)
pdev = {k: v.to(dev) for k, v in params.items()}
n = int(params["pos"].shape[0])
camargs = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def backward_us(rec):
    p = {k: v.detach().requires_grad_(True) for k, v in pdev.items()}
    with gs.deferred_checks() as chk:
        with (gs.densify_stats(rec) if rec is not None else torch.enable_grad()):
            img = gs.render_gaussians(*[p[k] for k in bench.NAMES], c2w, *camargs)
        torch.cuda.synchronize()
        t = timed(lambda: img.backward(gimg))
    chk.verify()
    return t


res = {"config": cfg, "n": n, "iterations": iters}
rec, total = gs.DensifyStats(n, dev), gs.DensifyStats(n, dev)
with torch.no_grad():                    # warm-up: pair capacity, allocator, code objects
    gs.render_gaussians(*[pdev[k] for k in bench.NAMES], c2w, *camargs)
for r in (None, rec):
    backward_us(r)
res["backward_us"] = round(statistics.median(backward_us(None) for _ in range(iters)), 1)
res["backward_with_stats_us"] = round(statistics.median(backward_us(rec) for _ in range(iters)), 1)

# the kernels alone: a waited frame keeps project_state and grad2d as separate buffers
lib = abi.lib()
p = {k: v.detach().requires_grad_(True) for k, v in pdev.items()}
spec = ops._frame_spec(True, *camargs, 0.01, 100.0, 32, 16, 1e-6, 6.25, 0.99, 1 / 128.)
view = spec.view
(img, _, _), fr, counts = ops._forward_impl(spec, c2w, {k: p[k] for k in spec.names}, False, True)
grad2d, state, pairs = fr.grad2d if fr.grad2d is not None else torch.zeros(n, 16, device=dev), fr.proj_state, fr.n_pairs
ops._backward_impl(fr, gimg)             # leaves the frame's grad2d filled (the tensor above is the frame's own)
torch.cuda.synchronize()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())
stats_call = lambda: abi.check(lib.gsplat_densify_stats(n, pairs, C.byref(view), ptr(state), ptr(grad2d), ptr(rec.data), st), "gsplat_densify_stats")
stats_call()
res["visible"] = int((rec.count > 0).sum())
res["densify_stats_kernel_us"] = round(statistics.median(timed(stats_call) for _ in range(iters)), 1)


def merge_us():
    stats_call()                         # every visible row touched again (the merge clears what it consumes)
    torch.cuda.synchronize()
    return timed(lambda: total.merge_(rec))


merge_us()
res["densify_stats_merge_kernel_us"] = round(statistics.median(merge_us() for _ in range(iters)), 1)
res["densify_stats_merge_untouched_us"] = round(statistics.median(timed(lambda: total.merge_(rec)) for _ in range(iters)), 1)

# the training iteration, one view
target = torch.rand(cam["H"], cam["W"], 3)
views = [dict(image=target.to(dev), c2w=c2w, H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])]
for rule in ("reference", "screen"):
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = training.Trainer(model, training.TrainConfig(densify_rule=rule, densification_interval=10 ** 6, opacity_reset_interval=10 ** 9))
    for it in (1, 2, 3):
        tr.step(it, views)
    torch.cuda.synchronize()
    ts = []
    for it in range(4, 4 + iters):
        ts.append(timed(lambda: tr.step(it, views)))
    res[f"train_step_{rule}_us"] = round(statistics.median(ts), 1)
res["train_step_screen_extra_us"] = round(res["train_step_screen_us"] - res["train_step_reference_us"], 1)
print(json.dumps(res))
