#!/usr/bin/env python3
"""What per-view bilateral grids cost: at the image size of a bench config (default 3: 1920 x 1080) and the default
grid (16, 16, 8),
  * the launches alone through the C ABI with arguments built once -- the forward, the backward in its three combinations (both
    gradients, g_image alone, the gather of g_grids alone), the TV launch over a table of 100 grids (gradient + loss) -- on device
    events, medians after warm-up, next to the bytes each is budgeted (24 B/pixel forward, 36 B/pixel for the g_image half, 24 B/pixel
    per visit and about four visits for the gather);
  * Trainer.step, one view: the default against bilagrid=True, alternating in the same process.
Prints one JSON line (microseconds) and writes it to a file when one is named.
    python tools/bilagrid_time.py [config] [iterations] [out.json]
    python tools/bilagrid_time.py --step-only [config] [iterations]      only Trainer.step with the mode OFF; GSPLAT_TREE=<checkout> runs
                                                                         another checkout's package (the parent commit, built beside
                                                                         this one: the A/B of the mode-off iteration on ONE box)
A kernel trace of the same run: rocprofv3 --kernel-trace --stats -- python tools/bilagrid_time.py"""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

args = [a for a in sys.argv[1:] if a != "--step-only"]
step_only = "--step-only" in sys.argv[1:]
sys.path.insert(0, os.environ.get("GSPLAT_TREE") or __file__.rsplit("/", 2)[0])
import bench
from oracle import scenes

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
abi = importlib.import_module(PKG + "._abi")
model_mod = importlib.import_module(PKG + ".model")
training = importlib.import_module(PKG + ".training")
config = int(args[0]) if len(args) > 0 else 3
iters = int(args[1]) if len(args) > 1 else 30
dev = torch.device("cuda:0")
X, Y, L = 16, 16, 8
V_TV = 100


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


params, cam = bench.synthetic_scene(config)
H, W = cam["H"], cam["W"]
c2w = torch.tensor(scenes.orbit_c2w(1, 24), device=dev)
views = [dict(image=torch.rand(H, W, 3).to(dev), c2w=c2w, H=H, W=W, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], idx=0)]


def step_times(modes):
    """Medians of Trainer.step, one view, for each named config -- alternating between them in this process."""
    trainers = {}
    for name, kw in modes:
        model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
        tr = trainers[name] = training.Trainer(model, training.TrainConfig(densify_until_iter=0, opacity_reset_interval=10 ** 9, **kw),
                                               **(dict(bilagrid_views=V_TV) if kw else {}))
        for it in (1, 2, 3):
            tr.step(it, views)
    torch.cuda.synchronize()
    ts = {name: [] for name in trainers}
    for it in range(4, 4 + iters):
        for name, tr in trainers.items():
            ts[name].append(timed(lambda: tr.step(it, views)))
    return ({name: round(statistics.median(v), 1) for name, v in ts.items()},
            {name: [round(x, 1) for x in np.percentile(v, [10, 90])] for name, v in ts.items()})


if step_only:
    med, spread = step_times([("default", {})])
    print(json.dumps({"tree": os.environ.get("GSPLAT_TREE") or "this", "config": config, "iterations": iters,
                      "train_step_default_us": med["default"], "p10_p90_us": spread["default"]}))
    sys.exit(0)

lib = abi.lib()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
image, g_out = torch.rand(1, H, W, 3, device=dev), torch.randn(1, H, W, 3, device=dev)
eye = torch.eye(3, 4, device=dev).reshape(1, 12, 1, 1, 1)
G = (eye + 0.05 * torch.randn(1, 12, L, Y, X, device=dev)).contiguous()
out, g_image, g_grids = torch.empty_like(image), torch.empty_like(image), torch.zeros_like(G)
table = (eye + 0.05 * torch.randn(V_TV, 12, L, Y, X, device=dev)).contiguous()
tv_grad, tv_loss = torch.zeros_like(table), torch.zeros((), device=dev)
scratch = torch.empty(lib.gsplat_bilagrid_tv_scratch_bytes(V_TV, X, Y, L), dtype=torch.uint8, device=dev)


def backward(gi, gg):
    return lambda: abi.check(lib.gsplat_bilagrid_backward(p(image), p(G), p(g_out), 1, H, W, X, Y, L, p(gi), p(gg), None, 0, st),
                             "gsplat_bilagrid_backward")


launches = {
    "forward": lambda: abi.check(lib.gsplat_bilagrid_forward(p(image), p(G), 1, H, W, X, Y, L, p(out), st), "gsplat_bilagrid_forward"),
    "backward": backward(g_image, g_grids),
    "backward_image_only": backward(g_image, None),
    "backward_grids_only": backward(None, g_grids),
    "tv_100_grids": lambda: abi.check(lib.gsplat_bilagrid_tv(p(table), V_TV, X, Y, L, 10.0, p(tv_loss), p(tv_grad), abi.GSPLAT_BILAGRID_ACCUMULATE,
                                                             p(scratch), st), "gsplat_bilagrid_tv"),
}
pixels = H * W
budget = {"forward": 24 * pixels, "backward_image_only": 36 * pixels, "backward_grids_only": 4 * 24 * pixels,
          "backward": (36 + 4 * 24) * pixels, "tv_100_grids": 3 * 4 * table.numel()}
res = {"config": config, "H": H, "W": W, "grid": [X, Y, L], "iterations": iters, "pixels": pixels, "budget_bytes": budget,
       "launch_us": {}, "launch_p10_p90_us": {}, "budget_tb_per_s": {}}
for _ in range(3):                           # warm-up: code objects, clocks
    for fn in launches.values():
        fn()
torch.cuda.synchronize()
ts = {name: [] for name in launches}
for _ in range(iters):
    for name, fn in launches.items():
        ts[name].append(timed(fn))
for name, v in ts.items():
    med = statistics.median(v)
    res["launch_us"][name] = round(med, 1)
    res["launch_p10_p90_us"][name] = [round(x, 1) for x in np.percentile(v, [10, 90])]
    res["budget_tb_per_s"][name] = round(budget[name] / med / 1e6, 2)
res["empty_event_pair_us"] = round(statistics.median([timed(lambda: None) for _ in range(iters)]), 1)

# the training iteration, one view: the default against bilagrid=True (a table of 100 grids: the dense TV launch and Adam step)
res["train_step_us"], res["train_step_p10_p90_us"] = step_times([("default", {}), ("bilagrid", dict(bilagrid=True))])
res["train_step_bilagrid_minus_default_us"] = round(res["train_step_us"]["bilagrid"] - res["train_step_us"]["default"], 1)
line = json.dumps(res)
print(line)
if len(args) > 2:
    with open(args[2], "w") as f:
        f.write(line + "\n")
