#!/usr/bin/env python3
"""What the screen-space low-pass costs: on the config-3 scene at an orbit camera, one view, device events, medians,
  * the forward pass and the backward pass of a deferred frame (composite entries, gradients wanted),
  * Trainer.step (one view: the folded f_rest step),
  * the reference's pair count P, the pairs actually binned and the visible Gaussians,
for the default mode, (lowpass 0.3, antialias off) and (lowpass 0.3, antialias on).
Prints one JSON line (microseconds) and writes it to the output file.
    python tools/filter_time.py [config] [iterations] [output.json]
Per-kernel times of the same run: rocprofv3 --kernel-trace --stats -- python tools/filter_time.py   (the filtered instantiations of
project_kernel / project_backward_kernel carry a trailing `true` template argument)."""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"filter_time_config{cfg}.json")
params, cam = bench.synthetic_scene(cfg)
dev = torch.device("cuda:0")
c2w = torch.tensor(scenes.orbit_c2w(1, 24), device=dev)
gimg = torch.rand(cam["H"], cam["W"], 3, device=dev)
pdev = {k: v.to(dev) for k, v in params.items()}
n = int(params["pos"].shape[0])
camargs = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
MODES = (("default", {}), ("lowpass", dict(lowpass=0.3)), ("antialias", dict(lowpass=0.3, antialias=True)))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, out


def frame_us(kw):
    """(forward, backward) of one deferred frame with gradients."""
    p = {k: v.detach().requires_grad_(True) for k, v in pdev.items()}
    with gs.deferred_checks() as chk:
        torch.cuda.synchronize()
        fwd, img = timed(lambda: gs.render_gaussians(*[p[k] for k in bench.NAMES], c2w, *camargs, **kw))
        bwd, _ = timed(lambda: img.backward(gimg))
    chk.verify()
    return fwd, bwd


res = {"config": cfg, "n": n, "iterations": iters, "H": cam["H"], "W": cam["W"]}
target = torch.rand(cam["H"], cam["W"], 3)
views = [dict(image=target.to(dev), c2w=c2w, H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])]
for tag, kw in MODES:
    with torch.no_grad():                # an eager frame: the counts, and a pair capacity for the mode
        img = gs.render_gaussians(*[pdev[k] for k in bench.NAMES], c2w, *camargs, **kw)
    _, visible, pairs = gs.render_stats(img)
    res[f"{tag}_visible"], res[f"{tag}_P"], res[f"{tag}_binned"] = int(visible), int(pairs), int(gs.ops.binned_pairs())
    frame_us(kw)
    ts = [frame_us(kw) for _ in range(iters)]
    res[f"{tag}_forward_us"] = round(statistics.median(t[0] for t in ts), 1)
    res[f"{tag}_backward_us"] = round(statistics.median(t[1] for t in ts), 1)
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = training.Trainer(model, training.TrainConfig(densification_interval=10 ** 6, opacity_reset_interval=10 ** 9, **kw))
    for it in (1, 2, 3):
        tr.step(it, views)
    torch.cuda.synchronize()
    ts = [timed(lambda: tr.step(it, views))[0] for it in range(4, 4 + iters)]
    res[f"{tag}_train_step_us"] = round(statistics.median(ts), 1)
line = json.dumps(res)
print(line)
with open(out_path, "w") as f:
    f.write(line + "\n")
