"""The pose correction in numpy float64: out = compose(c2w, delta) and its two gradients.  The yardstick of
tests/test_pose_delta_cpu.py and tests/test_gpu_pose_delta.py; it reads nothing but its arguments.

    delta = (d[3], p[3], s[3]);  a1 = p + e_x, a2 = s + e_y;  b1 = a1 / max(|a1|, eps);  u2 = a2 - (b1.a2) b1;  b2 = u2 / max(|u2|, eps);
    b3 = b1 x b2;  D = rows b1, b2, b3;  out[:3,:3] = R D,  out[:3,3] = R d + e,  out[3] = c2w[3]

An active clamp (a norm below eps) treats its denominator as a constant in the backward, as torch.nn.functional.normalize does.

The magnitudes (`magnitude`, `backward_magnitude`) are the same formulas with every term replaced by its absolute value and every
subtraction by an addition -- the sum of the absolute values of the terms, carried through the intermediate results: what a rounding
bound of the fp32 arithmetic is a multiple of.

torch_compose is the same forward written with torch functions, in the dtype of its arguments: its float64 autograd is the authority
for the gradients (tests/test_pose_delta_cpu.py holds backward() against it), and the oracle loops of the trainer tests compose
their poses with it."""
import numpy as np

EPS = 1e-12


def _batched(c2w, delta, g_out=None):
    c2w, delta = np.asarray(c2w, dtype=np.float64), np.asarray(delta, dtype=np.float64)
    single = c2w.ndim == 2
    if single:
        c2w, delta = c2w[None], delta[None]
    assert c2w.ndim == 3 and c2w.shape[1:] == (4, 4) and delta.shape == (c2w.shape[0], 9), (c2w.shape, delta.shape)
    if g_out is not None:
        g_out = np.asarray(g_out, dtype=np.float64).reshape(c2w.shape)
    return c2w, delta, g_out, single


def _dot(a, b):
    return (a * b).sum(axis=-1, keepdims=True)


def _cross(a, b, sign):
    """a x b (sign = -1), or the sum of the absolute values of its terms for non-negative a, b (sign = +1)."""
    return np.stack([a[:, 1] * b[:, 2] + sign * a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + sign * a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + sign * a[:, 1] * b[:, 0]], axis=1)


def _rotation(delta, sign, norms=None):
    """(D [B, 3, 3] with rows b1, b2, b3; a2; b1.a2; n1; n2; clamp 1 active; clamp 2 active).  sign = +1: the magnitudes, with the
    norms and clamps of the true run (`norms`)."""
    ex, ey = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    if sign < 0:
        a1, a2 = delta[:, 3:6] + ex, delta[:, 6:9] + ey
        l1 = np.sqrt(_dot(a1, a1))
    else:
        a1, a2 = np.abs(delta[:, 3:6]) + ex, np.abs(delta[:, 6:9]) + ey
        l1 = None
    if norms is None:
        c1 = l1 < EPS
        n1 = np.where(c1, EPS, l1)
    else:
        n1, _, c1, _ = norms
    b1 = a1 / n1
    dot = _dot(b1, a2)
    u2 = a2 + sign * dot * b1
    if norms is None:
        l2 = np.sqrt(_dot(u2, u2))
        c2 = l2 < EPS
        n2 = np.where(c2, EPS, l2)
    else:
        _, n2, _, c2 = norms
    b2 = u2 / n2
    b3 = _cross(b1, b2, sign)
    return np.stack([b1, b2, b3], axis=1), a2, dot, n1, n2, c1, c2


def _forward(c2w, delta, sign, norms=None):
    D = _rotation(delta, sign, norms)[0]
    out = c2w.copy()
    out[:, :3, :3] = np.einsum("bik,bkj->bij", c2w[:, :3, :3], D)
    out[:, :3, 3] = np.einsum("bik,bk->bi", c2w[:, :3, :3], delta[:, :3]) + c2w[:, :3, 3]
    return out


def _true_norms(delta):
    _, _, _, n1, n2, c1, c2 = _rotation(delta, -1.0)
    return n1, n2, c1, c2


def forward(c2w, delta):
    """compose(c2w, delta): c2w [4, 4] with delta [9], or [B, 4, 4] with [B, 9]."""
    c, t, _, single = _batched(c2w, delta)
    out = _forward(c, t, -1.0)
    return out[0] if single else out


def magnitude(c2w, delta):
    """The sum of the absolute values of the terms of every element of forward(c2w, delta)."""
    c, t, _, single = _batched(c2w, delta)
    out = _forward(np.abs(c), np.abs(t), 1.0, _true_norms(t))
    return out[0] if single else out


def _backward(c2w, delta, G, sign, norms=None):
    D, a2, dot, n1, n2, c1, c2 = _rotation(delta, sign, norms)
    R, d = c2w[:, :3, :3], delta[:, :3]
    g_c2w = G.copy()
    g_c2w[:, :3, :3] = np.einsum("bij,bkj->bik", G[:, :3, :3], D) + G[:, :3, 3:4] * d[:, None, :]
    g_d = np.einsum("bik,bi->bk", R, G[:, :3, 3])
    gD = np.einsum("bik,bij->bkj", R, G[:, :3, :3])
    b1, b2 = D[:, 0], D[:, 1]
    gb1, gb2, gb3 = gD[:, 0], gD[:, 1], gD[:, 2]
    gb1 = gb1 + _cross(b2, gb3, sign)
    gb2 = gb2 + _cross(gb3, b1, sign)
    gu2 = (gb2 + sign * np.where(c2, 0.0, _dot(gb2, b2)) * b2) / n2
    q = _dot(gu2, b1)
    g_s = gu2 + sign * q * b1
    gb1 = gb1 + sign * (q * a2 + dot * gu2)
    g_p = (gb1 + sign * np.where(c1, 0.0, _dot(gb1, b1)) * b1) / n1
    return g_c2w, np.concatenate([g_d, g_p, g_s], axis=1)


def backward(c2w, delta, g_out):
    """(g_c2w, g_delta) of g_out = dL/dout, shaped like c2w and delta."""
    c, t, g, single = _batched(c2w, delta, g_out)
    a, b = _backward(c, t, g, -1.0)
    return (a[0], b[0]) if single else (a, b)


def backward_magnitude(c2w, delta, g_out):
    """The sum of the absolute values of the terms of every element of backward(c2w, delta, g_out)."""
    c, t, g, single = _batched(c2w, delta, g_out)
    a, b = _backward(np.abs(c), np.abs(t), np.abs(g), 1.0, _true_norms(t))
    return (a[0], b[0]) if single else (a, b)


def torch_compose(c2w, delta):
    """compose(c2w, delta) with torch functions (any float dtype, differentiable): c2w [..., 4, 4], delta [..., 9]."""
    import torch
    F = torch.nn.functional
    d, p, s = delta[..., 0:3], delta[..., 3:6], delta[..., 6:9]
    a1 = p + torch.tensor([1.0, 0.0, 0.0], dtype=delta.dtype)
    a2 = s + torch.tensor([0.0, 1.0, 0.0], dtype=delta.dtype)
    b1 = F.normalize(a1, dim=-1, eps=EPS)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1, eps=EPS)
    b3 = torch.cross(b1, b2, dim=-1)
    D = torch.stack([b1, b2, b3], dim=-2)
    R, e = c2w[..., :3, :3], c2w[..., :3, 3]
    top = torch.cat([R @ D, (R @ d[..., None]) + e[..., None]], dim=-1)
    return torch.cat([top, c2w[..., 3:4, :]], dim=-2)
