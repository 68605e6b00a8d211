"""Oracle of the absolute-gradient sums of the raster backward (helper, not a test).  Plain numpy, float64, no GPU.

In the notation of tests/raster_oracle.py: for Gaussian i and pixel p of a list it is binned into, a_p = dL/dalpha exp(-q / 2), zero
unless alive, passed and o g <= alpha_max (the quantity whose moments the backward kernel takes).  With du = px - u, dv = py - v, over
all pixels of all its lists:

    Sx = sum_p |a_p (A11 du + A12 dv)|      Sy = sum_p |a_p (A12 du + A22 dv)|         (columns 10, 11 of grad2d behind the _abs entries)
    signed twins: the same sums without the absolute value (= A11 Mx + A12 My and A12 Mx + A22 My of the moments)
    scale_x = sum_p (|A11 du| + |A12 dv|) sa_p,  scale_y = sum_p (|A12 du| + |A22 dv|) sa_p,   sa = raster_oracle's absolute-term bound of a
    allow: for every band (pair, pixel) of raster_oracle.composite the pixel's column is recomputed with that one decision inverted
           and the absolute change of every touched Gaussian's contribution is added -- nothing is left out.

Every pixel's column comes from raster_oracle._columns on that one pixel (P = 1), whose M0 column is a_p and whose M0 scale is sa_p."""
import numpy as np

from tests import raster_oracle as ro


def _pixel_terms(o, r):
    """Per entry of one pixel's column o (P = 1): (|a lu|, |a lv|, a lu, a lv, scale_x, scale_y)."""
    a, sa = o["rows"][:, 5], o["scale"][:, 5]
    du, dv = o["du"][:, 0], o["dv"][:, 0]
    a11, a12, a22 = r[:, 2], r[:, 3], r[:, 4]
    lu, lv = a11 * du + a12 * dv, a12 * du + a22 * dv
    return (np.abs(a * lu), np.abs(a * lv), a * lu, a * lv, (np.abs(a11 * du) + np.abs(a12 * dv)) * sa, (np.abs(a12 * du) + np.abs(a22 * dv)) * sa)


class AbsReference:
    """S [n,2] = (Sx, Sy), signed [n,2], scale [n,2], allow [n,2]; in_list [n]."""


def absgrad(ref, rec, g_img=None, g_depth=None, g_alpha=None, bg=None, chi=None, alpha_max=None, alpha_cutoff=None):
    """ref: raster_oracle.composite(...) of the same records, lists, thresholds and upstream gradients (its lists, its band); rec [n,16];
    chi, alpha_max, alpha_cutoff: the thresholds given to composite()."""
    rec = np.asarray(rec, np.float64)
    if not ref.aux:
        assert g_depth is None and g_alpha is None and bg is None
        rec = rec.copy()
        rec[:, 11] = 0.0
    th = (float(chi), float(alpha_max), float(alpha_cutoff))
    H, W, n = ref.H, ref.W, ref.n
    gi, gd, ga = ro._upstream(H, W, g_img, g_depth, g_alpha)
    out = AbsReference()
    S, signed, scale, allow = (np.zeros((n, 2)) for _ in range(4))
    for l_ in np.nonzero(ref.ranges[:, 1] > ref.ranges[:, 0])[0]:
        s0, s1 = ref.ranges[l_]
        g = ref.sorted_ids[s0:s1]
        r = rec[g]
        px, py = ro._list_pixels(l_, ref.lists_x)
        valid = (px < W) & (py < H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)

        def column(p, force=None):
            vf = np.array([float(valid[p])])
            return ro._columns(r, np.array([float(px[p])]), np.array([float(py[p])]), vf, th, gi[cy[p], cx[p]][None, :] * vf[0],
                               gd[cy[p], cx[p]][None] * vf[0], ga[cy[p], cx[p]][None] * vf[0], bg, force=force)

        base = {}
        for p in np.nonzero(valid)[0]:
            base[p] = t = _pixel_terms(column(p), r)
            np.add.at(S[:, 0], g, t[0]); np.add.at(S[:, 1], g, t[1])
            np.add.at(signed[:, 0], g, t[2]); np.add.at(signed[:, 1], g, t[3])
            np.add.at(scale[:, 0], g, t[4]); np.add.at(scale[:, 1], g, t[5])
        flips = [(k, int(i), int(p)) for k in ("q", "cut", "max", "alive") for i, p in np.argwhere(ref.band[k][s0:s1])]
        b_col = ref.band["col"][cy, cx] & valid[:, None]
        flips += [("col", 0, int(p), int(c)) for p, c in np.argwhere(b_col)]
        for f in flips:
            p = f[2]
            if not valid[p]:
                continue
            t = _pixel_terms(column(p, force=(f[0], f[1]) + tuple(f[3:])), r)
            np.add.at(allow[:, 0], g, np.abs(t[0] - base[p][0]))
            np.add.at(allow[:, 1], g, np.abs(t[1] - base[p][1]))
    out.S, out.signed, out.scale, out.allow, out.in_list = S, signed, scale, allow, ref.in_list.copy()
    return out


def magnitude(S, opacity, H, W):
    """What one frame adds to grad_sum in absolute mode: sqrt((o Sx W/2)^2 + (o Sy H/2)^2)."""
    return np.sqrt((opacity * S[:, 0] * W / 2) ** 2 + (opacity * S[:, 1] * H / 2) ** 2)


def cancellation_frame():
    """ONE Gaussian centred on pixel (8, 4) of an 8 x 16 image whose per-pixel centre gradients a_p (A11 du + A12 dv) are ODD in
    (du, dv) about that centre: they cancel in the signed sums and add up in the absolute ones.  a_p = (c . G_p) exp(-q / 2) for a
    single Gaussian, and the linear term is odd already, so the upstream gradient G itself is EVEN about the centre (an odd G would
    make the terms even, and nothing would cancel); the row y = 0 and the column x = 0, whose mirror images lie outside the image,
    get no gradient.  Returns (rec [1,16], ranges, sorted_ids, lists_x, H, W, thresholds, g_img)."""
    H, W = 8, 16
    rec = np.zeros((1, 16), np.float32)
    rec[0, :8] = (8.0, 4.0, 0.125, 0.03125, 0.25, 0.5, 12.0, 9.0)          # u, v, A11, A12, A22, opacity, ex, ey (all exact in float32)
    rec[0, 8:11] = (0.5, 0.25, 0.75)
    ys, xs = np.mgrid[0:H, 0:W]
    du, dv = xs - 8.0, ys - 4.0
    even = 0.5 + (du * du + du * dv + 2.0 * dv * dv) / 64.0
    even[(xs == 0) | (ys == 0)] = 0.0
    g_img = np.stack([even, 0.5 * even, -0.25 * even], -1).astype(np.float32)
    return rec, np.array([[0, 1]], np.uint32), np.array([0], np.uint32), 1, H, W, (6.25, float(np.float32(0.99)), 1 / 128.0), g_img


def cancellation_scene():
    """The same frame for the device: one Gaussian on the optical axis of a camera whose principal point is pixel (8, 4), so that the
    projection puts its centre on that pixel exactly; g_img as above."""
    from tests import list_scenes
    d = dict(pos=np.array([[0.0, 0.0, 4.0]]), scale_raw=np.log(np.array([[0.5, 0.3, 0.4]])), q_raw=np.array([[0.9, 0.1, -0.2, 0.3]]),
             opacity_raw=np.array([0.0]), f_dc=np.array([[0.3, -0.2, 0.5]]), f_rest=np.zeros((1, 45)))
    return list_scenes._pack(d, 8, 16, 20.0, 20.0, 8.0, 4.0), cancellation_frame()[-1]
