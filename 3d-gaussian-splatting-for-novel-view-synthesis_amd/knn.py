"""Scale initialisation from the three nearest neighbours (not in the reference): the rule of the paper, of the INRIA
trainer (`distCUDA2` of simple_knn) and of gsplat (`knn(points, 4)`).  Every Gaussian starts as an isotropic blob whose size is the
root mean squared distance to its three nearest neighbours: dense regions start fine, sparse ones coarse.

    mean_dist2(points, out=None)                   dist2 [N]: the mean squared distance to the 3 nearest neighbours
    init_scale_raw(points, scale=1.0, floor=1e-7)  scale_raw [N, 3]: log(scale sqrt(max(dist2, floor))) in all three columns

    g = gs.data.initialize_gaussians_from_pointcloud(points, scale_init="knn", device="cuda")

The definition (csrc/gs_knn.h).  For N points p_i (fp32, [N, 3]), dist2[i] is the mean of the m = min(3, F - 1) smallest values of
d2(i, j):
  * j ranges over the finite rows j != i; F is the number of finite rows;
  * d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) of the three fp32 differences: one function for the device and the host test build;
  * the m values are summed in ascending order and scaled by a float constant per m (1, 1/2, 1/3): no division;
  * j != i is by index, not by distance: a duplicate of a point is its neighbour at distance 0 (as in simple_knn and sklearn);
  * a row with a NaN or an infinity is nobody's neighbour and gets 0;  F <= 1 gives 0 everywhere.
The search is exact, so the result is a function of the multiset of the other points only: the same bits on every call, stream and
data-parallel rank, and under any permutation of the rows (the output permutes with them).

ctypes calls into csrc/gsplat_knn.hip on the current stream, in the style of filter3d.py; nothing here reads the device.  There is no
CPU fallback.
"""
import math

import torch

from . import _abi
from ._dev import _gpu_f32, _p, _stream_ptr

BOX = _abi.GSPLAT_KNN_BOX


def mean_dist2(points, out=None):
    """dist2 [N] fp32 of points [N, 3] (the module docstring has the definition).  One library call on the current stream; the scratch
    (about 40 N bytes) is a fresh block from the caching allocator per call, so that calls on different streams never share one."""
    points = _gpu_f32(points.detach() if isinstance(points, torch.Tensor) else points, "points", "knn")
    n = points.shape[0] if points.dim() > 0 else 0
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points has shape {tuple(points.shape)}, expected [N, 3]")
    dev = points.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=dev)
        elif _gpu_f32(out, "out", "knn").shape != (n,) or out.device != dev:
            raise ValueError(f"out has shape {tuple(out.shape)} on {out.device}, expected ({n},) on {dev}")
        lib = _abi.lib()
        size = int(lib.gsplat_knn_scratch_bytes(n))
        if size < 0:
            raise ValueError(f"points has {n} rows, more than gsplat_knn_mean_dist2 takes")
        scratch = torch.empty(max(size, 256), dtype=torch.uint8, device=dev)
        _abi.check(lib.gsplat_knn_mean_dist2(n, _p(points), _p(out), _p(scratch), _stream_ptr(dev)), "gsplat_knn_mean_dist2")
    return out


def _positive(x, name):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not (x > 0 and math.isfinite(x)):
        raise ValueError(f"{name} must be a finite number > 0, not {x!r}")
    return float(x)


def init_scale_raw(points, scale=1.0, floor=1e-7):
    """scale_raw [N, 3]: log(scale sqrt(max(dist2, floor))) in all three columns -- the INRIA trainer's
    log(sqrt(clamp_min(distCUDA2(points), 1e-7))) and gsplat's init_scale.  The epilogue is three elementwise torch calls on [N]."""
    scale, floor = _positive(scale, "scale"), _positive(floor, "floor")
    d2 = mean_dist2(points)
    return torch.log(torch.sqrt(torch.clamp_min(d2, floor)) * scale)[:, None].repeat(1, 3)
