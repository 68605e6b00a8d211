#!/usr/bin/env python3
"""What the MCMC density control costs: on the config-3 scene (1 M Gaussians), medians on device events of
  * the noise launch (mcmc.add_noise) -- with the scene's own opacities, and with every Gaussian transparent (every row written);
  * the regulariser launch (mcmc.regularise, gradients added);
  * one refinement with 5 % of the rows dead (mcmc.relocate with the twelve Adam moments: six launches), the parameters restored
    outside the timed interval.
Each after a warm-up call, per measuring-on-mi355x: events around one call, a synchronise between samples.
Prints one JSON line (microseconds, medians) and, with a third argument, writes it to that file.
    python tools/mcmc_time.py [config] [iterations] [out.json]"""
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import bench

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
params, _ = bench.synthetic_scene(cfg)
dev = torch.device("cuda:0")
model = gs.model.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
n = model.get_num_gaussians()
opt = gs.optim.GaussianAdam(gs.optim.reference_param_groups(model), lr=0.01, eps=1e-15)
for p in model.get_params().values():
    p.grad = torch.randn_like(p)
    opt._state(p)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def median_us(fn, before=None):
    ts = []
    for _ in range(iters + 1):                     # (the first call is the warm-up: code objects, the scratch)
        if before is not None:
            before()
            torch.cuda.synchronize()
        ts.append(timed(fn))
    return round(statistics.median(ts[1:]), 1)


res = {"config": cfg, "n": n, "iterations": iters}
with torch.no_grad():
    scale = 1.6e-4 * 5e5
    res["opaque_fraction"] = round(float((torch.sigmoid(model.opacity_raw) > 0.9).float().mean()), 3)
    res["noise_us"] = median_us(lambda: gs.mcmc.add_noise(model, scale, 0, 1))
    saved = model.opacity_raw.detach().clone()
    model.opacity_raw.fill_(-5.0)
    res["noise_all_rows_written_us"] = median_us(lambda: gs.mcmc.add_noise(model, scale, 0, 1))
    model.opacity_raw.copy_(saved)
    res["regularise_us"] = median_us(lambda: gs.mcmc.regularise(model, 0.01, 0.01))
    g = torch.Generator(device=dev).manual_seed(1)
    dead = torch.rand(n, device=dev, generator=g) < 0.05
    model.opacity_raw[dead] = -20.0
    backup = {k: p.detach().clone() for k, p in model.get_params().items()}
    res["dead_rows"] = int(dead.sum())

    def restore():
        for k, p in model.get_params().items():
            p.copy_(backup[k])

    res["refine_5pct_dead_us"] = median_us(lambda: gs.mcmc.relocate(model, opt, 0.005, 0, 100), before=restore)
    res["noise_bytes_per_row"] = 56
    res["noise_gbytes_per_s_all_rows"] = round(56 * n / res["noise_all_rows_written_us"] / 1e3, 1)
print(json.dumps(res))
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    with open(sys.argv[3], "w") as f:
        f.write(json.dumps(res) + "\n")
