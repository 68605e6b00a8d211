#!/usr/bin/env python3
"""What per-view pose corrections cost: at a bench config (default 3),
  * the three launches alone through the C ABI with arguments built once -- the forward and the backward of one view, the backward of
    64 views, the decay of a table of 200 rows -- on device events, after warm-up;
  * Trainer.step, one view, alternating in the same process: the default (composite entries, folded f_rest step); no_fold
    (fold_rest_step=False: what leaving the folded step costs); separate_calls (the same with the composite entries switched off:
    what leaving them costs); and pose_opt=True (a pose frame through the separate library calls, the table's launches and its Adam).
Prints one JSON line (microseconds) and writes it to profiles/pose_opt_times.json, or to the file named.
    python tools/pose_opt_time.py [config] [iterations] [out.json]
A kernel trace of the same run: rocprofv3 --kernel-trace --stats -- python tools/pose_opt_time.py"""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
import bench
from oracle import scenes

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
abi = importlib.import_module(PKG + "._abi")
model_mod = importlib.import_module(PKG + ".model")
training = importlib.import_module(PKG + ".training")
config = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 30
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pose_opt_times.json")
dev = torch.device("cuda:0")


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
lib = abi.lib()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
c2w = torch.tensor(np.stack([scenes.orbit_c2w(k, 64) for k in range(64)]), dtype=torch.float32, device=dev).contiguous()
delta, g_out = 0.01 * torch.randn(64, 9, device=dev), torch.randn(64, 4, 4, device=dev)
out, g_c2w, g_delta = torch.empty_like(c2w), torch.empty_like(c2w), torch.zeros(64, 9, device=dev)
table, table_grad = 0.01 * torch.randn(200, 9, device=dev), torch.zeros(200, 9, device=dev)
launches = {
    "forward_1": lambda: abi.check(lib.gsplat_pose_delta_forward(p(c2w), p(delta), 1, p(out), st), "gsplat_pose_delta_forward"),
    "backward_1": lambda: abi.check(lib.gsplat_pose_delta_backward(p(c2w), p(delta), p(g_out), 1, p(g_c2w), p(g_delta), None, 0, st),
                                    "gsplat_pose_delta_backward"),
    "backward_1_delta_only": lambda: abi.check(lib.gsplat_pose_delta_backward(p(c2w), p(delta), p(g_out), 1, None, p(g_delta), None, 0, st),
                                               "gsplat_pose_delta_backward"),
    "backward_64": lambda: abi.check(lib.gsplat_pose_delta_backward(p(c2w), p(delta), p(g_out), 64, p(g_c2w), p(g_delta), None, 0, st),
                                     "gsplat_pose_delta_backward"),
    "decay_200": lambda: abi.check(lib.gsplat_pose_delta_decay(p(table), 200, 1e-6, p(table_grad), st), "gsplat_pose_delta_decay"),
}
res = {"config": config, "H": H, "W": W, "iterations": iters, "launch_us": {}, "launch_p10_p90_us": {}}
for _ in range(3):                           # warm-up: code objects, clocks
    for fn in launches.values():
        fn()
torch.cuda.synchronize()
ts = {name: [] for name in launches}
for _ in range(iters):
    for name, fn in launches.items():
        ts[name].append(timed(fn))
for name, v in ts.items():
    res["launch_us"][name] = round(statistics.median(v), 1)
    res["launch_p10_p90_us"][name] = [round(x, 1) for x in np.percentile(v, [10, 90])]
res["empty_event_pair_us"] = round(statistics.median([timed(lambda: None) for _ in range(iters)]), 1)

# the training iteration, one view
view_c2w = torch.tensor(scenes.orbit_c2w(1, 24), device=dev)
views = [dict(image=torch.rand(H, W, 3).to(dev), c2w=view_c2w, H=H, W=W, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], idx=0)]
trainers = {}
composite = {"default": True, "no_fold": True, "separate_calls": False, "pose_opt": True}


def step(name, it):
    gs.ops._composite = composite[name]        # (the ablation switch of ops.py: a deferred frame then takes the separate library calls)
    try:
        return trainers[name].step(it, views)
    finally:
        gs.ops._composite = True


for name, kw in (("default", {}), ("no_fold", dict(fold_rest_step=False)), ("separate_calls", dict(fold_rest_step=False)), ("pose_opt", dict(pose_opt=True))):
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = trainers[name] = training.Trainer(model, training.TrainConfig(densify_until_iter=0, opacity_reset_interval=10 ** 9, **kw),
                                           pose_views=200 if kw.get("pose_opt") else None)
    for it in (1, 2, 3):
        step(name, it)
torch.cuda.synchronize()
ts = {name: [] for name in trainers}
for it in range(4, 4 + iters):
    for name in trainers:
        ts[name].append(timed(lambda: step(name, it)))
res["train_step_us"] = {name: round(statistics.median(v), 1) for name, v in ts.items()}
res["train_step_p10_p90_us"] = {name: [round(x, 1) for x in np.percentile(v, [10, 90])] for name, v in ts.items()}
res["train_step_pose_opt_minus_default_us"] = round(res["train_step_us"]["pose_opt"] - res["train_step_us"]["default"], 1)
res["train_step_no_fold_minus_default_us"] = round(res["train_step_us"]["no_fold"] - res["train_step_us"]["default"], 1)
res["train_step_separate_calls_minus_no_fold_us"] = round(res["train_step_us"]["separate_calls"] - res["train_step_us"]["no_fold"], 1)
res["train_step_pose_opt_minus_separate_calls_us"] = round(res["train_step_us"]["pose_opt"] - res["train_step_us"]["separate_calls"], 1)
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
