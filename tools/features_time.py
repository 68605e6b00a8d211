#!/usr/bin/env python3
"""What the feature kernels cost: on the config-3 scene at one orbit camera, medians on device events of
  * raster_features_kernel (gsplat_features_forward) and raster_features_adjoint_kernel (gsplat_features_adjoint, into a table zeroed
    outside the timed interval) at C = 3, 8, 32, 128, beside
  * raster_forward_kernel<false> (gsplat_rasterize_forward without accum) of the SAME frame -- one project_state / bin_state, through
    ops internals -- in the same run, on the same box;
  * the whole features.render under torch.no_grad() and the whole features.lift per pose, at C = 8 (projection, the host's wait for
    the pair count, binning, the kernel), as tools/contribution_time.py times ops.contribution.
Prints one JSON line (microseconds, medians) and, with a third argument, writes it to that file.
    python tools/features_time.py [config] [iterations] [out.json]
A kernel trace of the same run (no counters in it): rocprofv3 --kernel-trace --stats -- python tools/features_time.py"""
import ctypes as C
import importlib
import json
import os
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
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
CHANNELS = (3, 8, 32, 128)
params, cam = bench.synthetic_scene(cfg)
dev = torch.device("cuda:0")
c2w = torch.tensor(scenes.orbit_c2w(1, 24), device=dev)
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


res = {"config": cfg, "n": n, "H": cam["H"], "W": cam["W"], "iterations": iters, "device": torch.cuda.get_device_name(dev),
       "command": "python tools/features_time.py " + " ".join(sys.argv[1:])}
lib = abi.lib()
with torch.no_grad():
    # one waited frame: its project_state and bin_state as separate buffers (also the warm-up: allocator, code objects)
    spec = ops._frame_spec(True, *camargs, 0.01, 100.0, 32, 16, 1e-6, 6.25, 0.99, 1 / 128.)
    (image, _, _), fr, counts = ops._forward_impl(spec, c2w, dict(zip(spec.names, [pdev[k] for k in spec.names])), False, False)
    torch.cuda.synchronize()
    view, state, bins, pairs = spec.view, fr.proj_state, fr.bin_state, fr.n_pairs
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    forward = lambda: abi.check(lib.gsplat_rasterize_forward(n, pairs, C.byref(view), ptr(state), ptr(bins), ptr(image), None, None, st),
                                "gsplat_rasterize_forward")
    forward()
    res["pairs"] = int(pairs)
    res["gaussians_in_lists"] = int(counts.n_visible)
    gen = torch.Generator(device=dev).manual_seed(7)
    for ch in CHANNELS:
        feats = torch.randn((n, ch), device=dev, generator=gen)
        G = torch.randn((cam["H"], cam["W"], ch), device=dev, generator=gen)
        out = torch.empty((cam["H"], cam["W"], ch), device=dev)
        table = torch.zeros((n, ch), device=dev)
        fwd = lambda: abi.check(lib.gsplat_features_forward(n, pairs, C.byref(view), ptr(state), ptr(bins), ptr(feats), ch, ptr(out), st),
                                "gsplat_features_forward")
        adj = lambda: abi.check(lib.gsplat_features_adjoint(n, pairs, C.byref(view), ptr(state), ptr(bins), ptr(G), ch, ptr(table), st),
                                "gsplat_features_adjoint")
        fwd()
        adj()
        torch.cuda.synchronize()
        ts_f, ts_a, ts_r = [], [], []
        for _ in range(iters):                 # alternating, so that all three see the same clocks
            table.zero_()
            torch.cuda.synchronize()
            ts_f.append(timed(fwd))
            ts_a.append(timed(adj))
            ts_r.append(timed(forward))
        raster = statistics.median(ts_r)
        res[f"C{ch}"] = {"groups": (ch + 7) // 8, "features_forward_us": round(statistics.median(ts_f), 1),
                         "features_adjoint_us": round(statistics.median(ts_a), 1), "raster_forward_kernel_us": round(raster, 1),
                         "forward_over_raster": round(statistics.median(ts_f) / raster, 2), "adjoint_over_raster": round(statistics.median(ts_a) / raster, 2),
                         "adjoint_rows_written": int((table != 0).any(1).sum())}
        del feats, G, out, table
    # the whole call per pose (device events round the call; C = 8)
    geometry = [pdev[k] for k in ("pos", "opacity_raw", "scale_raw", "q_raw")]
    feats8 = torch.randn((n, 8), device=dev, generator=gen)
    map8 = torch.randn((cam["H"], cam["W"], 8), device=dev, generator=gen)
    render = lambda: gs.features.render(geometry[0], feats8, *geometry[1:], c2w, *camargs)
    lift = lambda: gs.features.lift(*geometry, [c2w], [map8], *camargs)
    render()
    lift()
    res["render_no_grad_per_pose_us"] = round(statistics.median(timed(render) for _ in range(iters)), 1)
    res["lift_per_pose_us"] = round(statistics.median(timed(lift) for _ in range(iters)), 1)
print(json.dumps(res))
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    with open(sys.argv[3], "w") as f:
        f.write(json.dumps(res) + "\n")
