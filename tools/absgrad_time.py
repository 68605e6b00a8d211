#!/usr/bin/env python3
"""What the absolute-gradient statistic costs: on the config-3 scene at orbit camera 1 of 24, medians on device events,
  * the raster backward alone, gsplat_rasterize_backward against gsplat_rasterize_backward_abs on the same waited frame;
  * the backward pass of a deferred frame (composite entries) inside ops.densify_stats(rec) and ops.densify_stats(rec, absgrad=True);
  * Trainer.step with densify_rule "screen", without and with densify_absgrad (one view, no densification inside the timed window).
Prints one JSON line (microseconds) and writes it to the file given as the third argument.
    python tools/absgrad_time.py [config] [iterations] [out.json]"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else None
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


def median_us(fn):
    fn()
    return round(statistics.median(fn() for _ in range(iters)), 1)


res = {"config": cfg, "n": n, "iterations": iters}
with torch.no_grad():                    # warm-up: pair capacity, allocator, code objects
    gs.render_gaussians(*[pdev[k] for k in bench.NAMES], c2w, *camargs)

# the raster backward alone: a waited frame keeps project_state, bin_state, accum and grad2d as separate buffers
lib = abi.lib()
p = {k: v.detach().requires_grad_(True) for k, v in pdev.items()}
spec = ops._frame_spec(True, *camargs, 0.01, 100.0, 32, 16, 1e-6, 6.25, 0.99, 1 / 128.)
view = spec.view
(img, _, _), fr, counts = ops._forward_impl(spec, c2w, {k: p[k] for k in spec.names}, False, True)
grad2d = torch.empty(n, 16, device=dev)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())
res["pairs"] = int(fr.n_pairs)
for name, key in (("gsplat_rasterize_backward", "raster_backward_us"), ("gsplat_rasterize_backward_abs", "raster_backward_abs_us")):
    call = lambda: abi.check(getattr(lib, name)(n, fr.n_pairs, C.byref(view), ptr(fr.proj_state), ptr(fr.bin_state), ptr(fr.accum), ptr(gimg),
                                                ptr(grad2d), 0, None, 0, st), name)       # (grad2d_zeroed = 0: the call clears grad2d itself, in both)
    res[key] = median_us(lambda: timed(call))
res["raster_backward_abs_ratio"] = round(res["raster_backward_abs_us"] / res["raster_backward_us"], 3)


def backward_us(rec, absgrad):
    q = {k: v.detach().requires_grad_(True) for k, v in pdev.items()}
    with gs.deferred_checks() as chk:
        with gs.densify_stats(rec, absgrad=absgrad):
            im = gs.render_gaussians(*[q[k] for k in bench.NAMES], c2w, *camargs)
        torch.cuda.synchronize()
        t = timed(lambda: im.backward(gimg))
    chk.verify()
    return t


rec = gs.DensifyStats(n, dev)
res["backward_with_stats_us"] = median_us(lambda: backward_us(rec, False))
res["backward_with_abs_stats_us"] = median_us(lambda: backward_us(rec, True))

# the training iteration, one view
target = torch.rand(cam["H"], cam["W"], 3)
views = [dict(image=target.to(dev), c2w=c2w, H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])]
for absgrad, key in ((False, "train_step_screen_us"), (True, "train_step_screen_absgrad_us")):
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = training.Trainer(model, training.TrainConfig(densify_rule="screen", densify_absgrad=absgrad, densification_interval=10 ** 6,
                                                      opacity_reset_interval=10 ** 9))
    for it in (1, 2, 3):
        tr.step(it, views)
    torch.cuda.synchronize()
    ts = []
    for it in range(4, 4 + iters):
        ts.append(timed(lambda: tr.step(it, views)))
    res[key] = round(statistics.median(ts), 1)
res["train_step_absgrad_extra_us"] = round(res["train_step_screen_absgrad_us"] - res["train_step_screen_us"], 1)
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
