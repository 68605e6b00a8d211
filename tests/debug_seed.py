#!/usr/bin/env python3
"""For one seed of tests/test_gpu_parity.py::test_random_scenes_vs_oracle, or -- with a row of tests/mode_scenes.MODES -- one case of
tests/test_gpu_mode_scenes.py: the errors of the HIP path AND of the oracle run in float32 (= the reference's own fp32 arithmetic),
both against the float64 oracle, for the image, the maps and every gradient (diagnostic; needs a GPU).
    python tests/debug_seed.py <seed> [row] [det]"""
import importlib
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from tests import mode_scenes as ms
from tests import util

args = [a for a in sys.argv[1:] if a != "det"]
seed = int(args[0])
gs = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd")
if len(args) > 1:
    row = int(args[1])
    d, m = ms.mode_scene(seed), ms.MODES[row]
    print("row", row, m)
else:
    d, m = ms.parity_scene(seed), ms.MODES[0]
if "det" in sys.argv[1:]:                                # fixed-order sums instead of float atomics (is an error an accumulation error?)
    m = m._replace(route=ms.DETERMINISTIC)
print("H W n", d["H"], d["W"], len(d["pos"]))
res = {"f64": ms.oracle(d, m, ms.F64), "f32": ms.oracle(d, m, ms.F32), "hip": ms.render_hip(gs, d, m)}
ref = res["f64"]
names = ms.grad_names(m)
for tag in ("f32", "hip"):
    for what, im, r in zip(("image", "depth / max", "alpha"), res[tag][:3], ref[:3]):
        if im is not None:
            scale = max(np.abs(r).max(), 1e-30) if what.startswith("depth") else 1.0
            dd = np.abs(im - r) / scale
            y, x = np.unravel_index(int(dd.reshape(dd.shape[0], dd.shape[1], -1).max(-1).argmax()), dd.shape[:2])
            print(tag, "%-11s mean %.2e max %.2e at pixel (%d, %d) frac>1e-5 %.2e  >5e-3: %d" %
                  (what + ":", dd.mean(), dd.max(), y, x, (dd > util.IMG_TOL_BULK).mean(), int((dd > util.IMG_TOL_REST).sum())))
    for k in names:
        e = util.grad_errors(res[tag][3][k], ref[3][k])
        print("   %-12s rel-L2 %.3e  max/max %.3e" % (k, e["l2"], e["mx"]))
# where the largest error of every gradient sits, and what the float32 oracle does at the same Gaussian
for k in names:
    if k == "c2w":
        continue
    n = len(ref[3][k])
    e = np.abs(res["hip"][3][k] - ref[3][k]).reshape(n, -1).max(1)
    i = int(e.argmax())
    e32 = np.abs(res["f32"][3][k] - ref[3][k]).reshape(n, -1).max(1)
    print("   worst %-12s Gaussian %5d: |err| hip %.3e, f32 oracle %.3e there (its own worst %.3e at %d); |ref| there %.3e, max |ref| %.3e"
          % (k, i, e[i], e32[i], e32.max(), int(e32.argmax()), np.abs(ref[3][k]).reshape(n, -1).max(1)[i], np.abs(ref[3][k]).max()))
# what moving the chi-square clip and alpha_cutoff by -+ 1e-4 (relative) does to the gradients in float64, beside the HIP error
for thr in ("chi_square_clip", "alpha_cutoff"):
    band = ms.threshold_band(d, m, 1e-4, (thr,))
    for k in names:
        e = np.abs(res["hip"][3][k] - ref[3][k])
        out = np.maximum(e - util.K_CAL * band[k], 0.0)
        print("   %s -+1e-4 %-12s band max %.3e; |hip err| max %.3e, outside K_CAL x band %.3e (max |ref| %.3e)"
              % (thr, k, band[k].max(), e.max(), out.max(), np.abs(ref[3][k]).max()))
