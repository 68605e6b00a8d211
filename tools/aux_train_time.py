#!/usr/bin/env python3
"""What training with a background, an opacity target and depth maps costs: Trainer.step on the config-3 scene, one view, timed on
device events in steady state -- with the default config and with each of background=(1, 1, 1), lambda_alpha, lambda_depth and all
three on (an aux pass: the separate library calls, no folded f_rest step); and the two new kernels alone at the
frame's size (gsplat_aux_loss_forward + _backward through losses.aux_loss, gsplat_composite_target through losses.composite_over).
Prints one JSON line (microseconds, medians).
    python tools/aux_train_time.py [config] [iterations]"""
import importlib
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import bench
from oracle import scenes

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
losses = importlib.import_module(PKG + ".losses")
model_mod = importlib.import_module(PKG + ".model")
training = importlib.import_module(PKG + ".training")
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
params, cam = bench.synthetic_scene(cfg)
dev = torch.device("cuda:0")
H, W = cam["H"], cam["W"]
g = torch.Generator().manual_seed(1)
view = dict(image=torch.rand(H, W, 3, generator=g).to(dev), alpha=torch.rand(H, W, generator=g).to(dev),
            depth=(1.0 + 4.0 * torch.rand(H, W, generator=g)).to(dev), c2w=torch.tensor(scenes.orbit_c2w(1, 24)), H=H, W=W, fx=cam["fx"],
            fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def step_time(**kw):
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = training.Trainer(model, training.TrainConfig(densify_until_iter=0, opacity_reset_interval=10 ** 9, **kw))
    for it in (1, 2, 3):                 # warm-up: pair capacity, allocator, code objects
        tr.step(it, [view])
    return round(statistics.median(timed(lambda it=it: tr.step(it, [view])) for it in range(4, 4 + iters)), 1)


res = {"step_default_us": step_time(),
       "step_background_us": step_time(background=(1.0, 1.0, 1.0)),
       "step_lambda_alpha_us": step_time(lambda_alpha=0.1),
       "step_lambda_depth_us": step_time(lambda_depth=0.1),
       "step_all_us": step_time(background=(1.0, 1.0, 1.0), lambda_alpha=0.1, lambda_depth=0.1)}
depth, alpha = (view["depth"] * view["alpha"]).requires_grad_(True), view["alpha"].clone().requires_grad_(True)
target_alpha = torch.rand(H, W, generator=g).to(dev)


def aux_loss_call():
    depth.grad = alpha.grad = None
    losses.aux_loss(depth, alpha, view["depth"], target_alpha, 0.1, 0.1)[0].backward()


for fn in (aux_loss_call, lambda: losses.composite_over(view["image"], view["alpha"], (1.0, 1.0, 1.0))):
    for _ in range(3):
        fn()
res["aux_loss_forward_backward_us"] = round(statistics.median(timed(aux_loss_call) for _ in range(iters)), 1)
res["composite_over_us"] = round(statistics.median(timed(lambda: losses.composite_over(view["image"], view["alpha"], (1.0, 1.0, 1.0)))
                                                   for _ in range(iters)), 1)
res.update(config=cfg, n=int(params["pos"].shape[0]), H=H, W=W, iterations=iters)
print(json.dumps(res))
