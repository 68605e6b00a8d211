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


def stacked(n=300, hw=(8, 16)):
    """The scene of the capped-queue path (tests/test_gpu_aux.py, tests/test_gpu_raster.py): ONE 16 x 8 list holding 300 low-opacity
    Gaussians -- 5 chunks, and every central sub-tile queue is cut at the backward kernel's cap.  n < 300: its first n Gaussians (the
    draws are the same); hw: another image size around the same principal point (8, 4)."""
    rng = np.random.default_rng(5)
    m, f = 300, 20.0
    z = rng.uniform(3, 6, m)
    pos = np.stack([rng.uniform(-0.3, 0.3, m), rng.uniform(-0.15, 0.15, m), z], 1)
    d = dict(pos=pos, scale_raw=np.log(rng.uniform(0.3, 0.7, (m, 3))), q_raw=rng.normal(0, 1, (m, 4)),
             opacity_raw=rng.uniform(-4.2, -3.4, m), f_dc=0.5 * rng.normal(0, 1, (m, 3)), f_rest=0.1 * rng.normal(0, 1, (m, 45)))
    return _pack({k: v[:n] for k, v in d.items()}, hw[0], hw[1], f, f, 16 / 2, 8 / 2)


def clamps():
    """Both clamps of the compositing, for the un-fused entry: 60 Gaussians on 16 x 32 pixels with opacity_raw up to +8 (opacity
    0.999 > alpha_max near the centres) and colours from [-0.5, 1.5] (the composited colour leaves [0, 1] on either side).  Beside
    the usual arrays: color [n, 3] and sigma [n, 3, 3] (float32) for Frame(s, unfused=(color, sigma))."""
    n, H, W, f = 60, 16, 32, 30.0
    rng = np.random.default_rng(31)
    z = rng.uniform(3, 6, n)
    uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    pos = np.stack([(uv[:, 0] - W / 2) / f * z, (uv[:, 1] - H / 2) / f * z, z], 1)
    d = dict(pos=pos, scale_raw=np.log(rng.uniform(0.15, 0.6, (n, 3))), q_raw=rng.normal(0, 1, (n, 4)),
             opacity_raw=rng.uniform(-3.0, 8.0, n), f_dc=np.zeros((n, 3)), f_rest=np.zeros((n, 45)))
    s = _pack(d, H, W, f, f, W / 2.0, H / 2.0)
    s["color"] = np.ascontiguousarray(rng.uniform(-0.5, 1.5, (n, 3)), np.float32)
    s["sigma"] = np.ascontiguousarray(tp.covariance_from_params(torch.tensor(s["scale_raw"], dtype=torch.float64),
                                                                torch.tensor(s["q_raw"], dtype=torch.float64)).numpy(), np.float32)
    return s


RASTER_GOLDENS = ("g1_generic", "g2_ragged", "g3_occlusion", "g4_thresholds", "g6_huge", "g7_tiny", "g12_kwargs")
RASTER_SCENES = RASTER_GOLDENS + ("stacked", "stacked63", "stacked64", "stacked65", "stacked128", "stacked129", "stacked_5x13", "hot_spot",
                                  "equal_depths", "huge", "clamps")


def raster_scene(name):
    """The scenes of the raster-kernel tests (tests/test_raster_oracle_cpu.py, tests/test_gpu_raster.py): the smallest at which each
    path of the two kernels exists."""
    if name in RASTER_GOLDENS:
        return golden(name)
    if name == "stacked_5x13":
        return stacked(hw=(5, 13))
    if name.startswith("stacked"):
        return stacked(int(name[7:] or 300))
    return dict(hot_spot=lambda: hot_spot(6000, (32, 48)), equal_depths=equal_depths, huge=huge_gaussians, clamps=clamps)[name]()


def thresholds(s, as_float32=False):
    """chi_square_clip, alpha_max, alpha_cutoff of the scene; as_float32: the values the kernels receive (gsplat_view holds floats)."""
    kw = s["kwargs"]
    th = (kw.get("chi_square_clip", 6.25), kw.get("alpha_max", 0.99), kw.get("alpha_cutoff", 1 / 128.))
    return tuple(float(np.float32(x)) for x in th) if as_float32 else th


def upstream(s, seed=3, left_half_zero=False):
    """Seeded normal upstream gradients of the image, the depth map and the opacity map (float32)."""
    rng = np.random.default_rng(seed)
    H, W = s["H"], s["W"]
    g = [rng.normal(0, 1, shape).astype(np.float32) for shape in ((H, W, 3), (H, W), (H, W))]
    if left_half_zero:
        for a in g:
            a[:, :W // 2] = 0
    return g


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
