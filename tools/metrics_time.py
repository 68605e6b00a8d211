#!/usr/bin/env python3
"""What the image metrics cost: metrics.image_metrics at 1920 x 1080, B = 1, without and with the colour correction,
beside the forward half of losses.compute_loss_device at the same shape AS TRAINING RUNS IT -- the prediction requires a gradient,
so the statistics kernel also writes the three partial-derivative maps the backward half reads (36 B/pixel, 75 MB here); no backward
is run.  That is the yardstick: the value-only statistics kernel of the metrics writes no maps.  The loss's value-only forward (a
prediction without a gradient: no maps) is timed too, for information -- it is the metrics kernel's nearest relative and does
slightly LESS per pixel (no squared-error sum, no mask, fp32 sums, two reciprocals for a division).

Two kinds of window, every sample `reps` calls between two device events after a warm-up of every call, the calls alternating in
one process on the same device:
  entry_us   the library entries alone (gsplat_metrics_forward, gsplat_loss_forward) on buffers allocated once: one ctypes call per
             launch pair, so the device is the bottleneck and this is the device time of the launches of a call
  call_us    the Python calls a user makes (allocation of outputs and scratch, argument checks, the autograd node of the loss)
  host_enqueue_us   how long the host takes to QUEUE one Python call (host clock, no synchronise inside the window): where this is
             below call_us the window was bound by the device, where it is not, call_us measures the host
Prints one JSON line (microseconds per call) and writes it to the file named.
    python tools/metrics_time.py [samples] [reps] [out.json]
A kernel trace of the same run: rocprofv3 --kernel-trace --stats -- python tools/metrics_time.py"""
import ctypes as C
import importlib
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
abi = importlib.import_module(PKG + "._abi")
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
if not torch.cuda.is_available():
    sys.exit("metrics_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
H, W = 1080, 1920


def window(fn):
    """(device microseconds per call, host microseconds to queue one call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = (time.perf_counter() - t0) * 1e6 / reps
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


g = torch.Generator().manual_seed(3)
target = torch.rand(H, W, 3, generator=g)
pred = (0.9 * target + 0.05 + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1).to(dev)
target = target.to(dev)
pred_grad = pred.clone().requires_grad_()          # what training hands the loss: the forward keeps the maps for a backward
lib = abi.lib()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
CC = abi.GSPLAT_METRICS_COLOUR_CORRECT
out, affine = torch.empty(1, 4, device=dev), torch.empty(1, 12, device=dev)
values, total = torch.empty(3, device=dev), torch.empty((), device=dev)
m_scratch = torch.empty(lib.gsplat_metrics_scratch_bytes(1, H, W, CC), dtype=torch.uint8, device=dev)
l_scratch = torch.empty(lib.gsplat_loss_scratch_bytes(1, H, W, 1), dtype=torch.uint8, device=dev)
entries = {
    "metrics": lambda: abi.check(lib.gsplat_metrics_forward(p(pred), p(target), None, 1, H, W, 0, None, p(out), p(m_scratch), st), "metrics"),
    "metrics_colour_correct": lambda: abi.check(lib.gsplat_metrics_forward(p(pred), p(target), None, 1, H, W, CC, p(affine), p(out), p(m_scratch), st),
                                                "metrics"),
    "loss_forward": lambda: abi.check(lib.gsplat_loss_forward(p(pred), p(target), 1, H, W, 0.8, 0.2, 1.0, p(values), p(total), p(l_scratch), 1, st),
                                      "loss"),
    "loss_forward_value_only": lambda: abi.check(lib.gsplat_loss_forward(p(pred), p(target), 1, H, W, 0.8, 0.2, 1.0, p(values), p(total),
                                                                         p(l_scratch), 0, st), "loss"),
}
calls = {
    "metrics": lambda: gs.metrics.image_metrics(pred, target),
    "metrics_colour_correct": lambda: gs.metrics.image_metrics(pred, target, colour_correct=True),
    "loss_forward": lambda: gs.losses.compute_loss_device(pred_grad, target),
    "loss_forward_value_only": lambda: gs.losses.compute_loss_device(pred, target),
}
for _ in range(3):                               # warm-up: code objects, the allocator's blocks, clocks
    for fn in list(entries.values()) + list(calls.values()):
        window(fn)
te, tc, th = ({name: [] for name in calls} for _ in range(3))
for _ in range(samples):
    for name in calls:
        te[name].append(window(entries[name])[0])
        dev_us, host_us = window(calls[name])
        tc[name].append(dev_us)
        th[name].append(host_us)


def med(ts):
    return {k: round(statistics.median(v), 2) for k, v in ts.items()}


def spread(ts):
    return {k: [round(x, 2) for x in np.percentile(v, [10, 90])] for k, v in ts.items()}


res = {"H": H, "W": W, "B": 1, "samples": samples, "calls_per_sample": reps,
       "entry_us": med(te), "entry_p10_p90_us": spread(te), "call_us": med(tc), "call_p10_p90_us": spread(tc), "host_enqueue_us": med(th),
       "launches_per_call": {"metrics": 2, "metrics_colour_correct": 4, "loss_forward": 2, "loss_forward_value_only": 2},
       "loss_forward_writes_maps_bytes": 36 * H * W}
res["metrics_over_loss_forward_entry"] = round(res["entry_us"]["metrics"] / res["entry_us"]["loss_forward"], 3)
res["metrics_over_loss_forward_call"] = round(res["call_us"]["metrics"] / res["call_us"]["loss_forward"], 3)
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
