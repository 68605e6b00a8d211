"""Oracle of the screen-space densification statistics (helper, not a test).

Built on oracle/torch_port.py: the oracle renders with `stages`, the projected centres u, v keep their
gradients (retain_grad), and after the backward pass of sum(image * w)

    g[i]   = sqrt((dL/du_i W/2)^2 + (dL/dv_i H/2)^2)                        (NDC units)
    ext[i] = min(max(sqrt(chi k22 / D), sqrt(chi k11 / D)), 250),  D = k11 k22 - k12^2     (half-extents of {q <= chi}, pixels)

scattered to the input rows through st["ids"]; `seen` marks the rows the oracle keeps on screen (its own AABB test: a superset of
the Gaussians the HIP path bins into a list).  Everything in the dtype asked for.
"""
import numpy as np
import torch

from oracle import torch_port as tp

NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
EXTENT_MAX = 250.0


def frame_stats(s, w, dtype=torch.float64, c2w=None, lowpass=0.0, antialias=False):
    """s: a scene (util.load(...) or tests/list_scenes.py); w [H, W, 3]: the upstream gradient of the image; c2w: another camera
    than the scene's; lowpass, antialias: the oracle's filter.  Returns float64 numpy arrays g [N], ext [N], seen [N] (bool)."""
    torch.set_num_threads(16)
    p = {k: torch.tensor(np.asarray(s[k])).to(dtype).requires_grad_(True) for k in NAMES}
    cam = torch.tensor(np.asarray(s["c2w"] if c2w is None else c2w)).to(dtype)
    H, W = int(s["H"]), int(s["W"])
    n = p["pos"].shape[0]
    g, ext, seen = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    st = {}
    sigma = tp.covariance_from_params(p["scale_raw"], p["q_raw"])
    color = tp.sh_colour(p["f_dc"], p["f_rest"], p["pos"], cam)
    img = tp.render(p["pos"], color, p["opacity_raw"], sigma, cam, H, W, s["fx"], s["fy"], s["cx"], s["cy"], stages=st, lowpass=lowpass,
                    antialias=antialias, **s["kwargs"])
    if "u" not in st:                                   # no survivor: the zero image, nothing on screen
        return g, ext, seen
    st["u"].retain_grad()
    st["v"].retain_grad()
    (img * torch.as_tensor(np.asarray(w)).to(dtype)).sum().backward()
    ids = st["ids"].numpy()
    gu = st["u"].grad.double().numpy() if st["u"].grad is not None else np.zeros(len(ids))
    gv = st["v"].grad.double().numpy() if st["v"].grad is not None else np.zeros(len(ids))
    g[ids] = np.sqrt((gu * W / 2) ** 2 + (gv * H / 2) ** 2)
    chi = float(s["kwargs"].get("chi_square_clip", 6.25))
    k = st["conic"].detach()
    det = k[:, 0] * k[:, 2] - k[:, 1] * k[:, 1]
    e = torch.maximum(torch.sqrt(chi * k[:, 2] / det), torch.sqrt(chi * k[:, 0] / det)).clamp(max=EXTENT_MAX)
    ext[ids] = e.double().numpy()
    seen[ids] = True
    return g, ext, seen


def upstream(s, seed=0):
    """A seeded upstream gradient of the image, float32 [H, W, 3] in [0, 1)."""
    return np.random.default_rng(seed).uniform(0, 1, (int(s["H"]), int(s["W"]), 3)).astype(np.float32)
