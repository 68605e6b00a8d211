#!/usr/bin/env python3
"""What the SH degree is worth: on the config-3 scene at an orbit camera, one view, device events, medians,
  * the forward pass and the backward pass of a deferred frame (composite entries, gradients wanted) at degrees 0, 1, 2, 3;
  * Trainer.step (one view: the folded f_rest step) at degree 0 and at degree 3.
Next to the times stand the bytes per Gaussian the projection forward reads (44 B of geometry + 12 B of f_dc, + 180 B of f_rest
from degree 1 on: whole rows are staged) and the f_rest bytes the projection backward moves.
Prints one JSON line (microseconds) and writes it to the output file.
    python tools/sh_degree_time.py [config] [iterations] [output.json]
A kernel trace of the same run: rocprofv3 --kernel-trace --stats -- python tools/sh_degree_time.py"""
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
import bench
from oracle import scenes

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
model_mod = importlib.import_module(PKG + ".model")
training = importlib.import_module(PKG + ".training")
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"sh_degree_time_config{cfg}.json")
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
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, out


def frame_us(degree):
    """(forward, backward) of one deferred frame with gradients."""
    p = {k: v.detach().requires_grad_(True) for k, v in pdev.items()}
    with gs.deferred_checks() as chk:
        torch.cuda.synchronize()
        fwd, img = timed(lambda: gs.render_gaussians(*[p[k] for k in bench.NAMES], c2w, *camargs, sh_degree=degree))
        bwd, _ = timed(lambda: img.backward(gimg))
    chk.verify()
    return fwd, bwd


res = {"config": cfg, "n": n, "iterations": iters, "H": cam["H"], "W": cam["W"]}
with torch.no_grad():                    # warm-up: pair capacity, allocator, code objects
    gs.render_gaussians(*[pdev[k] for k in bench.NAMES], c2w, *camargs)
for degree in (0, 1, 2, 3):
    frame_us(degree)
    ts = [frame_us(degree) for _ in range(iters)]
    res[f"forward_degree{degree}_us"] = round(statistics.median(t[0] for t in ts), 1)
    res[f"backward_degree{degree}_us"] = round(statistics.median(t[1] for t in ts), 1)
    # what the projection kernels move per Gaussian (from the code: whole f_rest rows from degree 1 on)
    res[f"forward_input_bytes_degree{degree}"] = 56 + (180 if degree else 0)
    res[f"backward_f_rest_gradient_bytes_degree{degree}"] = 180        # every row is written: zeros at degree 0, not formed

# the training iteration, one view (the Adam step of f_rest folded into the backward); degree 0 = a schedule that never leaves it
target = torch.rand(cam["H"], cam["W"], 3)
views = [dict(image=target.to(dev), c2w=c2w, H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])]
for degree, interval in ((0, 10 ** 9), (3, 0)):
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = training.Trainer(model, training.TrainConfig(densification_interval=10 ** 6, opacity_reset_interval=10 ** 9, sh_degree_interval=interval))
    for it in (1, 2, 3):
        assert tr.step(it, views)["sh_degree"] == degree
    torch.cuda.synchronize()
    ts = [timed(lambda: tr.step(it, views))[0] for it in range(4, 4 + iters)]
    res[f"train_step_degree{degree}_us"] = round(statistics.median(ts), 1)
line = json.dumps(res)
print(line)
with open(out_path, "w") as f:
    f.write(line + "\n")
