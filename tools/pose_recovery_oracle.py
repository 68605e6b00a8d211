"""Choose K and the table learning rate of the pose-recovery test (tests/test_gpu_pose_training.py) on the CPU, and
write what that test reads: tests/golden/pose_recovery.npz.

A frozen model of 300 Gaussians at 64 x 64, two views whose GIVEN poses are off the true ones by about 0.5 degrees and 0.02 units;
targets are the float64 oracle's renders at the true poses.  K pose-only iterations -- loss = mean squared error per view, one row
of a [2, 9] table per view (tests/pose_delta_oracle.torch_compose), torch.optim.Adam at a fixed rate with eps = 1e-8 -- on the
float64 oracle and on the float32 oracle (oracle/torch_port.py).  The file holds the scene, the cameras, the targets, K, the rate and
both error trajectories (rotation angle in radians and translation distance per iteration and view, entry 0 = the start).

    python tools/pose_recovery_oracle.py [--steps K] [--lr RATE] [--out FILE]

Chosen: K = 300 at 1e-3.  The float64 loop goes from (8.73e-3 rad, 2.0e-2) to (4.6e-5, 2.1e-4) and (6.7e-5, 3.3e-4) for the two views,
falling all the way, and ends well above fp32's noise floor: the float32 loop ends within 1 % of it.  Tried and left: 120 at 3e-4
stops at a quarter of the start; 300 at 2e-3 reaches 6e-8 rad, where two fp32 runs differ by more than their error.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import scenes  # noqa: E402
from oracle import torch_port as tp  # noqa: E402
from tests import pose_delta_oracle as po  # noqa: E402

NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")


def build():
    """(scene, camera tuple, true poses [2, 4, 4], given poses [2, 4, 4]) in float64."""
    rng = np.random.default_rng(129)
    s = scenes._base(rng, 300, 64, 64, 70.0, 70.0, 32.0, 32.0, mu_s=-1.9)
    true = np.stack([np.asarray(s["c2w"], dtype=np.float64), np.asarray(scenes._camera(rng, tilt=0.1), dtype=np.float64)])
    given = true.copy()
    for k, (axis, shift) in enumerate((((1.0, 2.0, -1.5), (0.012, -0.016, 0.0)), ((-2.0, 1.0, 1.0), (-0.01, 0.01, 0.0141)))):
        axis = np.asarray(axis) / np.linalg.norm(axis) * np.deg2rad(0.5)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        a = np.deg2rad(0.5)
        rot = np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K
        given[k, :3, :3] = rot @ true[k, :3, :3]
        given[k, :3, 3] += shift
    return s, (s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"]), true, given


def errors(c2w, true):
    """(rotation angle in radians, translation distance) of each pose of c2w [B, 4, 4] from true [B, 4, 4], in float64."""
    c2w, true = np.asarray(c2w, dtype=np.float64), np.asarray(true, dtype=np.float64)
    r = np.einsum("bij,bkj->bik", c2w[:, :3, :3], true[:, :3, :3])
    sin = 0.5 * np.linalg.norm(np.stack([r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]], 1), axis=1)
    return np.arctan2(sin, (np.trace(r, axis1=1, axis2=2) - 1) / 2), np.linalg.norm(c2w[:, :3, 3] - true[:, :3, 3], axis=1)


def loop(s, cam, true, given, targets, steps, lr, dtype):
    p = [torch.tensor(np.asarray(s[k]), dtype=dtype) for k in NAMES]
    table = torch.zeros(2, 9, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([table], lr=lr, eps=1e-8)
    g = torch.tensor(given, dtype=dtype)
    tgt = [torch.tensor(t, dtype=dtype) for t in targets]
    rot, tr = [], []
    for it in range(steps + 1):
        c2w = po.torch_compose(g, table)
        e = errors(c2w.detach().double().numpy(), true)
        rot.append(e[0]); tr.append(e[1])
        if it == steps:
            break
        opt.zero_grad()
        loss = sum(((tp.render_fused(*p, c2w[k], *cam) - tgt[k]) ** 2).mean() for k in range(2))
        loss.backward()
        opt.step()
    return np.stack(rot), np.stack(tr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pose_recovery.npz"))
    a = ap.parse_args()
    s, cam, true, given = build()
    with torch.no_grad():
        p64 = [torch.tensor(np.asarray(s[k]), dtype=torch.float64) for k in NAMES]
        targets = [tp.render_fused(*p64, torch.tensor(true[k]), *cam).numpy() for k in range(2)]
    res = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        rot, tr = loop(s, cam, true, given, targets, a.steps, a.lr, dtype)
        res["rot_" + name], res["trans_" + name] = rot, tr
        print(name, "rotation", rot[0], "->", rot[-1], "translation", tr[0], "->", tr[-1])
        for it in range(0, a.steps + 1, max(1, a.steps // 8)):
            print("   ", it, rot[it], tr[it])
    np.savez_compressed(a.out, steps=a.steps, lr=a.lr, cam=np.asarray(cam, dtype=np.float64), true=true, given=given,
                        targets=np.stack(targets).astype(np.float32), **{k: np.asarray(s[k], dtype=np.float32) for k in NAMES}, **res)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
