"""float64 numpy oracle of the 3D smoothing filter, independent of csrc/gs_filter3d.h: the sampling interval per
Gaussian with a band for the float32 decisions next to a threshold, the filter in raw-parameter space from its plain closed forms, and
its vector-Jacobian product from the closed-form partial derivatives.

    compute(pos, cams, near, margin)      -> dict(t_sure, t_possible, seen_sure, seen_possible)      (t = min z / max(fx, fy), no sqrt(s))
    fill(t, seen)                         -> t with the unseen rows set to the maximum of the seen ones (0 if none)
    apply(scale_raw, opacity_raw, filt)   -> (scale_raw', opacity_raw')
    apply_vjp(scale_raw, opacity_raw, filt, g_scale_out, g_opacity_out) -> (g_scale_raw, g_opacity_raw)
    scene(seed, n, n_cams)                -> (pos float32 [n, 3], view dicts): the fixed test scene of the GPU tests
    inputs / plain_float32 / errors       the rows, the float32 yardstick and the error measure of the filter's tolerance rule

cams: a list of view dicts (c2w [4, 4], H, W, fx, fy, cx, cy), as Trainer.step takes them.
"""
import numpy as np
import torch

REL = 1e-4            # relative margin of the three inequalities: sure = inside by REL, possible = inside when relaxed by REL


def _camera_space(pos, v):
    c2w = np.asarray(v['c2w'], dtype=np.float64)
    d = np.asarray(pos, dtype=np.float64) - c2w[:3, 3]
    return d @ c2w[:3, :3]                                   # R^T (p - t), row by row


def compute(pos, cams, near=0.2, margin=0.15, rel=REL):
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    out = {}
    finite = np.isfinite(pos).all(axis=1)
    for name, sign in (("sure", +1.0), ("possible", -1.0)):
        t = np.full(n, np.inf)
        for v in cams:
            with np.errstate(all="ignore"):
                pc = _camera_space(pos, v)
                x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
                fx, fy, cx, cy, W, H = (float(v[k]) for k in ("fx", "fy", "cx", "cy", "W", "H"))
                u, w = fx * x / z + cx, fy * y / z + cy
                du, dv = sign * rel * (1 + 2 * margin) * W, sign * rel * (1 + 2 * margin) * H          # REL of the widened image's size
                seen = (finite & (z > near * (1 + sign * rel)) & (u >= -margin * W + du) & (u <= (1 + margin) * W - du)
                        & (w >= -margin * H + dv) & (w <= (1 + margin) * H - dv))
                t = np.where(seen, np.minimum(t, z / max(fx, fy)), t)
        out["seen_" + name] = np.isfinite(t)
        out["t_" + name] = t
    return out


def fill(t, seen):
    top = t[seen].max() if seen.any() else 0.0
    return np.where(seen, t, top)


def _terms(scale_raw, filt):
    e = np.exp(np.asarray(scale_raw, dtype=np.float64))
    clamped = e < 1e-6
    s2 = np.where(clamped, 1e-6, e) ** 2
    f2 = np.asarray(filt, dtype=np.float64)[:, None] ** 2
    return s2, f2, clamped


def apply(scale_raw, opacity_raw, filt):
    s2, f2, _ = _terms(scale_raw, filt)
    o = np.asarray(opacity_raw, dtype=np.float64).reshape(-1)
    scale_out = 0.5 * np.log(s2 + f2)
    c = np.sqrt(np.prod(s2 / (s2 + f2), axis=1))
    sigma = 1.0 / (1.0 + np.exp(-o))
    x = c * sigma
    return scale_out, (np.log(x) - np.log1p(-x)).reshape(np.shape(opacity_raw))


def apply_vjp(scale_raw, opacity_raw, filt, g_scale_out, g_opacity_out):
    s2, f2, clamped = _terms(scale_raw, filt)
    o = np.asarray(opacity_raw, dtype=np.float64).reshape(-1)
    go = np.asarray(g_opacity_out, dtype=np.float64).reshape(-1)
    c = np.sqrt(np.prod(s2 / (s2 + f2), axis=1))
    sigma = 1.0 / (1.0 + np.exp(-o))
    w = np.where(clamped, 0.0, s2 / (s2 + f2))               # d scale_raw'_j / d scale_raw_j
    qw = np.where(clamped, 0.0, f2 / (s2 + f2))              # d log c / d scale_raw_j
    one_minus = 1.0 - c * sigma
    g_o = go * (1.0 - sigma) / one_minus
    g_log_c = go / one_minus
    g_s = np.asarray(g_scale_out, dtype=np.float64) * w + g_log_c[:, None] * qw
    return g_s, g_o.reshape(np.shape(opacity_raw))


def inputs(n, seed):
    """float32 rows over the ranges the filter meets in training: scale_raw in [-12, 3], opacity_raw in [-12, 12], f in [1e-5, 1]
    (log-uniform), upstream gradients of order one."""
    rng = np.random.default_rng(seed)
    scale_raw = rng.uniform(-12.0, 3.0, (n, 3)).astype(np.float32)
    opacity_raw = rng.uniform(-12.0, 12.0, n).astype(np.float32)
    filt = np.exp(rng.uniform(np.log(1e-5), 0.0, n)).astype(np.float32)
    return scale_raw, opacity_raw, filt, rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=n).astype(np.float32)


def plain_float32(scale_raw, opacity_raw, filt, gs_out, go_out):
    """The closed forms as written, evaluated by torch in float32, with autograd's gradients: the yardstick of the tolerance."""
    s_raw = torch.tensor(scale_raw, requires_grad=True)
    o_raw = torch.tensor(opacity_raw, requires_grad=True)
    s = torch.clamp_min(torch.exp(s_raw), 1e-6)
    f2 = (torch.tensor(filt) ** 2)[:, None]
    so = torch.log(torch.sqrt(s * s + f2))
    c = torch.sqrt(torch.prod(s * s / (s * s + f2), dim=1))
    oo = torch.logit(c * torch.sigmoid(o_raw))
    ((so * torch.tensor(gs_out)).sum() + (oo * torch.tensor(go_out)).sum()).backward()
    return so.detach().numpy(), oo.detach().numpy(), s_raw.grad.numpy(), o_raw.grad.numpy()


def errors(scale_raw, opacity_raw, filt, gs_out, go_out, so, oo, g_s, g_o):
    """(scale, opacity, g_scale, g_opacity): the largest relative error against the float64 oracle, forward in activated space, a
    gradient entry relative to the sum of the magnitudes of its two terms."""
    ref_so, ref_oo = apply(scale_raw, opacity_raw, filt)
    ref_gs, ref_go = apply_vjp(scale_raw, opacity_raw, filt, gs_out, go_out)
    e_s = np.abs(np.exp(so.astype(np.float64) - ref_so) - 1.0).max()
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    e_o = np.abs(sig(oo.astype(np.float64)) / sig(ref_oo) - 1.0).max()
    one = np.ones_like(go_out, dtype=np.float64)
    only_s, _ = apply_vjp(scale_raw, opacity_raw, filt, np.abs(gs_out), 0.0 * one)
    only_o, mag_o = apply_vjp(scale_raw, opacity_raw, filt, 0.0 * np.abs(gs_out), np.abs(go_out))
    e_gs = (np.abs(g_s - ref_gs) / (np.abs(only_s) + np.abs(only_o) + 1e-300)).max()
    e_go = (np.abs(g_o - ref_go) / (np.abs(mag_o) + 1e-300)).max()
    return e_s, e_o, e_gs, e_go


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """c2w of a camera at `eye` whose +z axis points at `target` (the project's convention: x right, y down, z forward)."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    return c2w


def scene(seed, n, n_cams):
    """pos float32 [n, 3] and n_cams view dicts with mixed intrinsics (every value exact in float32).  The cameras stand on an arc of
    +-1 rad of a circle of radius 4 around the origin and look at it; every fifth one has a long lens.  Most points lie in
    [-1.5, 1.5]^3; the first n // 8 are 60 units above (outside every margin), the next n // 8 around (12, 0, 0), behind every camera
    of the arc, and the last row (n >= 3) has a NaN."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.5, 1.5, (n, 3))
    k = n // 8
    pos[:k] = rng.uniform(-0.5, 0.5, (k, 3)) + np.array([0.0, 60.0, 0.0])
    pos[k:2 * k] = rng.uniform(-0.5, 0.5, (k, 3)) + np.array([12.0, 0.0, 0.0])
    pos = pos.astype(np.float32)
    if n >= 3:
        pos[n - 1, 1] = np.nan
    views = []
    for c in range(n_cams):
        a = -1.0 + 2.0 * (c + 0.5) / n_cams
        eye = np.array([4.0 * np.cos(a), 0.5 * np.sin(3 * a), 4.0 * np.sin(a)])
        W, H = (96, 64) if c % 2 == 0 else (80, 80)
        f = 240.0 if c % 5 == 4 else 70.0 + 10.0 * (c % 3)
        views.append(dict(c2w=look_at(eye, rng.uniform(-0.3, 0.3, 3)).astype(np.float32), H=H, W=W, fx=f, fy=f + 4.0 * (c % 2),
                          cx=W / 2 + 0.5 * (c % 3), cy=H / 2 - 0.25 * (c % 2)))
    return pos, views
