"""The scenes of the list / record checks (tests/test_listcheck_cpu.py, tests/test_gpu_lists.py), as plain float32 arrays, and the
oracle's float64 per-Gaussian stages for them.  The synthetic ones are the scenes of tests/test_gpu_parity.py, seed for seed."""
import numpy as np
import torch

from oracle import scenes
from oracle import torch_port as tp
from tests import util

NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")


def _pack(s, H, W, fx, fy, cx, cy, c2w=None, **kwargs):
    out = {k: np.ascontiguousarray(np.asarray(s[k], np.float32)) for k in NAMES}
    out.update(H=int(H), W=int(W), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), kwargs=kwargs,
               c2w=np.ascontiguousarray(np.eye(4) if c2w is None else c2w, np.float32))
    return out


def golden(name):
    d = util.load(name)
    return _pack(d, *util.cam_args(d), c2w=d["c2w"], **d["kwargs"])


def _distinct_depths(z):
    zs, order = torch.sort(z)
    keep = torch.ones(len(z), dtype=torch.bool)
    keep[order[1:][(zs[1:] - zs[:-1]) < 2e-5]] = False
    return keep


def hot_spot(n, hw):
    """test_long_lists_take_the_large_sort_paths: thousands of Gaussians on the same pixels."""
    (H, W), f = hw, 40.0
    g = torch.Generator().manual_seed(11)
    z = torch.rand(n, generator=g, dtype=torch.float64) * 4 + 2
    keep = _distinct_depths(z)
    uv = torch.rand(n, 2, generator=g, dtype=torch.float64) * 7.0 + 4.5
    pos = torch.stack([(uv[:, 0] - W / 2) / f * z, (uv[:, 1] - H / 2) / f * z, z], 1).float()
    s = dict(pos=pos, scale_raw=torch.randn(n, 3, generator=g) * 0.2 - 1.6, q_raw=torch.randn(n, 4, generator=g),
             opacity_raw=torch.randn(n, generator=g) * 0.3 - 3.6, f_dc=torch.randn(n, 3, generator=g),
             f_rest=torch.randn(n, 45, generator=g) * 0.2)
    return _pack({k: v[keep].numpy() for k, v in s.items()}, H, W, f, f, W / 2.0, H / 2.0)


def equal_depths():
    """test_equal_depths_are_ordered_by_index: every Gaussian at camera depth 4."""
    n, H, W, f = 3000, 32, 48, 40.0
    g = torch.Generator().manual_seed(21)
    z = torch.full((n,), 4.0, dtype=torch.float64)
    uv = torch.stack([torch.rand(n, generator=g, dtype=torch.float64) * (W - 8) + 4,
                      torch.rand(n, generator=g, dtype=torch.float64) * (H - 8) + 4], 1)
    pos = torch.stack([(uv[:, 0] - W / 2) / f * z, (uv[:, 1] - H / 2) / f * z, z], 1).float()
    s = dict(pos=pos, scale_raw=torch.randn(n, 3, generator=g) * 0.2 - 1.2, q_raw=torch.randn(n, 4, generator=g),
             opacity_raw=torch.randn(n, generator=g) * 0.3 - 3.4, f_dc=torch.randn(n, 3, generator=g),
             f_rest=torch.randn(n, 45, generator=g) * 0.2)
    return _pack({k: v.numpy() for k, v in s.items()}, H, W, f, f, W / 2.0, H / 2.0)


def huge_gaussians():
    """test_huge_gaussians_cover_many_lists: every 8th Gaussian spans more than 32 lists."""
    n, H, W, f = 400, 120, 160, 100.0
    g = torch.Generator().manual_seed(22)
    z = torch.rand(n, generator=g, dtype=torch.float64) * 3 + 3
    keep = _distinct_depths(z)
    uv = torch.stack([torch.rand(n, generator=g, dtype=torch.float64) * W, torch.rand(n, generator=g, dtype=torch.float64) * H], 1)
    pos = torch.stack([(uv[:, 0] - W / 2) / f * z, (uv[:, 1] - H / 2) / f * z, z], 1).float()
    scale = torch.randn(n, 3, generator=g) * 0.3 - 2.0
    scale[::8] += 2.3
    s = dict(pos=pos, scale_raw=scale, q_raw=torch.randn(n, 4, generator=g), opacity_raw=torch.randn(n, generator=g) - 1.0,
             f_dc=torch.randn(n, 3, generator=g), f_rest=torch.randn(n, 45, generator=g) * 0.2)
    return _pack({k: v[keep].numpy() for k, v in s.items()}, H, W, f, f * 1.1, W / 2.0 + 1.5, H / 2.0 - 2.0, c2w=scenes.orbit_c2w(0, 8))


def config(cfg):
    s = scenes.synthetic_scene(cfg)
    return _pack(s, s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"])


def cam_args(s):
    return (s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"])


def oracle_stages(s, dtype=torch.float64):
    """The oracle's per-Gaussian stages (F4 - F13, no compositing) as float64 numpy arrays, evaluated in `dtype`:
    ids, u, v, conic [V, 3], cond (2-D condition number), tile_rect, opacity."""
    st = {}
    torch.set_num_threads(16)
    tp.render_fused(*[torch.tensor(s[k]).to(dtype) for k in NAMES], torch.tensor(s["c2w"]).to(dtype), *cam_args(s), stages=st,
                    stop_after_binning=True, **s["kwargs"])
    ev = st["evals"].double().numpy()
    return dict(ids=st["ids"].numpy(), u=st["u"].double().numpy(), v=st["v"].double().numpy(), conic=st["conic"].double().numpy(),
                cond=ev[:, 1] / ev[:, 0], tile_rect=st["tile_rect"].numpy(), opacity=st["opacity"].double().numpy())
