#!/usr/bin/env python3
"""What the 3-nearest-neighbour scale initialisation costs, on device events, medians after warm-up:
  * gs.knn.mean_dist2 at 100 k, 1 M and 10 M points (--sizes), on two clouds: `uniform` in the unit cube, and `clustered` -- 256 tight
    clusters in the unit cube plus 1 % outliers spread over 100 x the core's extent, the shape of an SfM cloud;
  * at 100 k, the library route the kernel replaces: torch.cdist in chunks of 4096 rows + topk(4), with the largest relative
    difference between the two results (the library route rounds differently; it is not a reference).
No time here is a pass/fail condition.  Writes profiles/knn_times.json (or --out) and prints it (microseconds)."""
import argparse
import importlib
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--cdist-at", type=int, default=100_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
gs = importlib.import_module(PKG)
if not torch.cuda.is_available():
    sys.exit("knn_time.py measures on the GPU; there is none here")
dev = torch.device("cuda:0")


def cloud(kind, n, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "uniform":
        return torch.rand(n, 3, generator=g).to(dev)
    centres = torch.rand(256, 3, generator=g)
    p = centres[torch.randint(0, 256, (n,), generator=g)] + 0.01 * torch.randn(n, 3, generator=g)
    far = torch.rand(n, generator=g) < 0.01
    p[far] = (torch.rand(int(far.sum()), 3, generator=g) - 0.5) * 100.0 + 0.5
    return p.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def median_us(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn) for _ in range(iters)]
    return round(statistics.median(t), 1), [round(float(x), 1) for x in np.percentile(t, [10, 90])]


def cdist_topk(p, chunk=4096):
    out = torch.empty(p.shape[0], device=p.device)
    for a in range(0, p.shape[0], chunk):
        d = torch.cdist(p[a:a + chunk], p)
        out[a:a + chunk] = (d.topk(4, dim=1, largest=False).values[:, 1:] ** 2).mean(dim=1)
    return out


res = {"device": torch.cuda.get_device_name(0), "box": gs.knn.BOX, "iterations": args.iterations, "sizes": {}}
for n in args.sizes:
    row = {}
    for kind in ("uniform", "clustered"):
        p = cloud(kind, n)
        out = torch.empty(n, device=dev)
        iters = args.iterations if n <= 1_000_000 else max(3, args.iterations // 2)
        us, spread = median_us(lambda: gs.knn.mean_dist2(p, out=out), iters)
        row[kind] = {"mean_dist2_us": us, "p10_p90_us": spread, "points_per_us": round(n / us, 1)}
        if n == args.cdist_at:
            lib_us, lib_spread = median_us(lambda: cdist_topk(p), max(3, args.iterations // 2), warm=1)
            ref = cdist_topk(p)
            rel = ((out - ref).abs() / ref.clamp_min(1e-30)).max()
            row[kind].update(cdist_topk_us=lib_us, cdist_topk_p10_p90_us=lib_spread, cdist_over_kernel=round(lib_us / us, 1),
                             largest_relative_difference=float(rel))
        del p, out
    row["clustered_over_uniform"] = round(row["clustered"]["mean_dist2_us"] / row["uniform"]["mean_dist2_us"], 2)
    res["sizes"][str(n)] = row
    print(f"{n}: {json.dumps(row)}", flush=True)
path = args.out or os.path.join(HERE, "profiles", "knn_times.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
