#!/usr/bin/env python3
"""What per-view exposure compensation costs: at the image size of a bench config (default 3),
  * the three launches alone through the C ABI with arguments built once -- the forward, the backward with both gradients (two
    launches: the sums and their finish), each half of the backward alone -- on device events, after warm-up, next to the bytes each
    moves (24 B/pixel forward, 36 B/pixel backward);
  * Trainer.step, one view: the default against exposure=True, alternating in the same process.
Prints one JSON line (microseconds) and writes it to a file when one is named.
    python tools/exposure_time.py [config] [iterations] [out.json]
A kernel trace of the same run: rocprofv3 --kernel-trace --stats -- python tools/exposure_time.py"""
import ctypes as C
import importlib
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import bench
from oracle import scenes

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
abi = importlib.import_module(PKG + "._abi")
model_mod = importlib.import_module(PKG + ".model")
training = importlib.import_module(PKG + ".training")
config = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 30
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
image, g_out = torch.rand(1, H, W, 3, device=dev), torch.randn(1, H, W, 3, device=dev)
E = (torch.eye(3, 4, device=dev) + 0.05 * torch.randn(3, 4, device=dev)).reshape(1, 12).contiguous()
out, g_image, g_params = torch.empty_like(image), torch.empty_like(image), torch.zeros(1, 12, device=dev)
scratch = torch.empty(lib.gsplat_exposure_scratch_bytes(1, H, W), dtype=torch.uint8, device=dev)
launches = {
    "forward": lambda: abi.check(lib.gsplat_exposure_forward(p(image), p(E), 1, H, W, p(out), st), "gsplat_exposure_forward"),
    "backward": lambda: abi.check(lib.gsplat_exposure_backward(p(image), p(E), p(g_out), 1, H, W, p(g_image), p(g_params), None, 0, p(scratch), st),
                                  "gsplat_exposure_backward"),
    "backward_image_only": lambda: abi.check(lib.gsplat_exposure_backward(p(image), p(E), p(g_out), 1, H, W, p(g_image), None, None, 0, None, st),
                                             "gsplat_exposure_backward"),
    "backward_params_only": lambda: abi.check(lib.gsplat_exposure_backward(p(image), p(E), p(g_out), 1, H, W, None, p(g_params), None, 0, p(scratch), st),
                                              "gsplat_exposure_backward"),
}
pixels = H * W
res = {"config": config, "H": H, "W": W, "iterations": iters, "pixels": pixels,
       "bytes": {"forward": 24 * pixels, "backward": 36 * pixels, "backward_image_only": 24 * pixels, "backward_params_only": 24 * pixels},
       "launch_us": {}, "launch_p10_p90_us": {}, "launch_tb_per_s": {}}
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
    res["launch_tb_per_s"][name] = round(res["bytes"][name] / med / 1e6, 2)
res["empty_event_pair_us"] = round(statistics.median([timed(lambda: None) for _ in range(iters)]), 1)

# the training iteration, one view: the default against exposure=True
c2w = torch.tensor(scenes.orbit_c2w(1, 24), device=dev)
views = [dict(image=torch.rand(H, W, 3).to(dev), c2w=c2w, H=H, W=W, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], idx=0)]
trainers = {}
for name, kw in (("default", {}), ("exposure", dict(exposure=True))):
    model = model_mod.GaussianModel({k: v.clone() for k, v in params.items()}, device=dev)
    tr = trainers[name] = training.Trainer(model, training.TrainConfig(densify_until_iter=0, opacity_reset_interval=10 ** 9, **kw),
                                           exposure_views=200 if kw else None)
    for it in (1, 2, 3):
        tr.step(it, views)
torch.cuda.synchronize()
ts = {name: [] for name in trainers}
for it in range(4, 4 + iters):
    for name, tr in trainers.items():
        ts[name].append(timed(lambda: tr.step(it, views)))
res["train_step_us"] = {name: round(statistics.median(v), 1) for name, v in ts.items()}
res["train_step_p10_p90_us"] = {name: [round(x, 1) for x in np.percentile(v, [10, 90])] for name, v in ts.items()}
res["train_step_exposure_minus_default_us"] = round(res["train_step_us"]["exposure"] - res["train_step_us"]["default"], 1)
line = json.dumps(res)
print(line)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write(line + "\n")
