"""Reference of the two raster kernels alone (K6 raster_forward_kernel, K7 raster_backward_kernel): a float64 composite of the SAME
records and lists the kernels read, so that what is compared is the raster arithmetic and nothing else.  Plain numpy, no torch, no GPU.

Inputs: rec [n,16] (u, v, A11, A12 | A22, opacity, ex, ey | r, g, b, z | ...), ranges [lists,2], sorted_ids, lists_x, H, W and the three
thresholds, as tests/device_frame.Frame.arrays() or tests/cpu_frame.cpu_state() give them (or float64 from elsewhere); upstream
gradients g_img [H,W,3] and optionally g_depth, g_alpha [H,W] and a background bg[3].

Rule (include/gsplat_mi355x.h, render.py), per list over its 16 x 8 pixels inside the image, entries in list order:
    q = A11 du^2 + 2 A12 du dv + A22 dv^2,  og = o exp(-q / 2),  pass = (q <= chi) and (og >= cutoff),  alpha = pass ? min(og, alpha_max) : 0,
    T_i = prod_{k<i} (1 - alpha_k),  alive = T_i > 5e-5,  w = alive ? alpha T : 0,
    C = sum w c,  A = sum w,  D = sum w z,  image = clamp(C + (1 - A) bg).
Rows of grad2d (per Gaussian, summed over its lists): with G+ = (G_r, G_g, G_b, G_D, G_A - sum_c G_c bg_c), G_c masked by the clamp of the
shown colour, s_i = c+_i . G+ and dL/dalpha_i = T_i s_i - (sum_{k>i} w_k s_k) / (1 - alpha_i), the moments Mx, My, Mxx, Mxy, Myy, M0 of
a = dL/dalpha exp(-q / 2) [alive and pass and og <= alpha_max], then sum w G_r, sum w G_g, sum w G_b, and column 9 = sum w G_D.

scale [n,NS]: the same sums with every term replaced by its absolute value; the dL/dalpha term by
    |T s| + (sum_k |w_k s_k| + |G . C|) / (1 - alpha)       over the whole pixel
-- the kernel forms the suffix sum as total - prefix, so an occluded row carries an absolute error of eps times that.  Per pixel
scale_img = 1 + sum w |c| (+ A |bg| under a background), and 1 + sum w |z|, 1 + sum w for D and A.

The band: a (pair, pixel) is in the band when one of its decisions lies within fp32's reach of its threshold,
    |q - chi| <= K_B 2^-24 (|A11| du^2 + 2 |A12 du dv| + |A22| dv^2 + 1)                              (= qb)
    |og - cutoff| or |og - alpha_max| <= og (K_B 2^-24 + qb / 2)
    |T_i - 5e-5| <= 5e-5 K_B 2^-24 (i + 1)
    |shown colour - 0| or |shown colour - 1| <= K_B 2^-24 scale_img,
K_B = 16 from the rounding count of the kernel's expression (q: two differences, five products, two sums and the pre-scaling of the
conic, each half an ulp of its own term: <= 8 x 2^-24 of the sum of absolute terms, and as much again for the threshold's own product
with the same constant; T_i: one product and one difference per layer).  Decisions on a pixel that is neither alive nor in the band of
the alive test decide nothing and are not counted, nor are the two tests of o g on a pixel that is the Gaussian's centre (du = dv = 0: o g = o
without a rounding, so a tie there is decided by the comparison operator alone -- `<` for `<=` must show), nor is the colour clamp of a pixel that no Gaussian reaches (A = 0).  For every band (pair, pixel) that one pixel's column is recomputed with that one
decision inverted; the absolute change of the pixel's outputs goes to allow_img, that of every touched Gaussian's row contributions
to allow [n,NS].  Nothing is left out of a comparison: a band pixel is compared with its allowance added to the bound.

Float32 mode (composite_f32): the same in the kernel's order -- conic pre-scaled by -0.5 log2 e, exp2, sequential T = T - alpha T, suffix
= total - running prefix, fp32 sums per sub-tile, per pair, per Gaussian.  It is the calibration: check() is given K = 3 x its largest
|delta| / (2^-24 scale)."""
import numpy as np

LIST_W, LIST_H = 16, 8
EPS = 2.0 ** -24
K_B = 16.0
T_MIN = 5e-5
CHUNK, MAXQ_BWD = 64, 24
KINDS = ("image", "moments", "colour")       # output kinds a K is measured for: maps | columns 0-5 | columns 6-8 (and 9)


class RasterError(AssertionError):
    pass


def f32_thresholds(chi, alpha_max, alpha_cutoff):
    """The kernels get the three thresholds as floats: a reference FOR THE KERNELS is given those values (composite() itself takes
    the thresholds as they come: alpha_max = 0.99 and float(0.99f) differ by 1e-8, which a saturated pixel shows)."""
    return tuple(float(np.float32(x)) for x in (chi, alpha_max, alpha_cutoff))


def _list_pixels(l_, lists_x):
    ox, oy = (l_ % lists_x) * LIST_W, (l_ // lists_x) * LIST_H
    px = ox + np.tile(np.arange(LIST_W), LIST_H)
    py = oy + np.repeat(np.arange(LIST_H), LIST_W)
    return px, py


def _upstream(H, W, g_img, g_depth, g_alpha, dtype=np.float64):
    z2 = np.zeros((H, W), dtype)
    return (np.zeros((H, W, 3), dtype) if g_img is None else np.asarray(g_img, dtype),
            z2 if g_depth is None else np.asarray(g_depth, dtype), z2 if g_alpha is None else np.asarray(g_alpha, dtype))


def _columns(r, px, py, valid, th, gi, gd, ga, bg, force=None):
    """The rule on the pixels (px, py) [P] of one list with entries r [L,16] (float64).  gi [P,3], gd, ga [P]: upstream gradients.
    force = (kind, entry[, channel]) inverts that one decision (P = 1).  Returns a dict of [L,P] / [P] arrays and the per-entry rows and
    scales [L,10] summed over the P pixels."""
    chi, amax, cut = th
    du, dv = px[None, :] - r[:, 0:1], py[None, :] - r[:, 1:2]
    a11, a12, a22, o = r[:, 2:3], r[:, 3:4], r[:, 4:5], r[:, 5:6]
    col, z = r[:, 8:11], r[:, 11]
    q = a11 * du * du + 2 * a12 * du * dv + a22 * dv * dv
    gs = np.exp(-0.5 * np.minimum(q, 4 * chi + 100.0))
    og = o * gs
    pq, po, pc = q <= chi, og >= cut, og <= amax
    if force is not None and force[0] in ("q", "cut", "max"):
        m = dict(q=pq, cut=po, max=pc)[force[0]]
        m[force[1], 0] = not m[force[1], 0]
    pas = pq & po
    alpha = np.where(pas, np.where(pc, og, amax), 0.0)
    T = np.cumprod(1.0 - alpha, 0)
    T = np.concatenate([np.ones_like(T[:1]), T[:-1]], 0) * valid[None, :]
    alive = T > T_MIN
    if force is not None and force[0] == "alive":
        i = force[1]
        if alive[i, 0]:
            alive[i:, 0] = False
        else:
            alive[:i + 1, 0] = bool(valid[0])
    w = np.where(alive, alpha * T, 0.0)
    C, A, D = w.T @ col, w.sum(0), w.T @ z
    has_bg = bg is not None
    shown = C + (1.0 - A)[:, None] * np.asarray(bg, np.float64)[None, :] if has_bg else C
    cm = (shown >= 0.0) & (shown <= 1.0)
    if force is not None and force[0] == "col":
        cm[0, force[2]] = not cm[0, force[2]]
    Gc = gi * cm
    Ga = ga - (Gc @ np.asarray(bg, np.float64) if has_bg else 0.0)
    sdot = col @ Gc.T + z[:, None] * gd[None, :] + Ga[None, :]
    ws = w * sdot
    total = ws.sum(0)
    suffix = total[None, :] - np.cumsum(ws, 0)
    mask = alive & pas & pc
    inv = 1.0 / (1.0 - alpha)
    a = np.where(mask, (T * sdot - suffix * inv) * gs, 0.0)
    sa = np.where(mask, (np.abs(T * sdot) + (np.abs(ws).sum(0) + np.abs(total))[None, :] * inv) * gs, 0.0)
    rows, scale = np.empty((len(r), 10)), np.empty((len(r), 10))
    for k, m in enumerate((du, dv, du * du, du * dv, dv * dv, np.ones_like(du))):
        rows[:, k], scale[:, k] = (m * a).sum(1), (np.abs(m) * sa).sum(1)
    for c in range(3):
        rows[:, 6 + c], scale[:, 6 + c] = w @ Gc[:, c], w @ np.abs(Gc[:, c])
    rows[:, 9], scale[:, 9] = w @ gd, w @ np.abs(gd)
    s_col = 1.0 + w.T @ np.abs(col) + (A[:, None] * np.abs(np.asarray(bg, np.float64))[None, :] if has_bg else 0.0)
    return dict(du=du, dv=dv, q=q, og=og, pq=pq, po=po, pc=pc, T=T, alive=alive, C=C, A=A, D=D, shown=shown, cm=cm, rows=rows, scale=scale,
                s_col=s_col, s_D=1.0 + w.T @ np.abs(z), s_A=1.0 + A, image=np.clip(shown, 0.0, 1.0),
                qb=K_B * EPS * (np.abs(a11) * du * du + 2 * np.abs(a12 * du * dv) + np.abs(a22) * dv * dv + 1.0))


class Reference:
    """What composite() returns: the maps image / accum (= C) [H,W,3], depth, alpha [H,W]; rows [n,16] (columns ns .. 15 zero), scale,
    allow [n,ns]; scale_img / allow_img (dicts by map name); in_list [n]; pair_scale [pairs,ns] by position in sorted_ids; the decisions
    (dec: q, cut, max, alive [capacity,128] bool, col [H,W,3]) and the band (band: [capacity,128] bool per kind, band_upto: some decision
    of the pixel at or before the entry is in the band); band_pixels [H,W]."""


def composite(rec, ranges, sorted_ids, lists_x, H, W, chi, alpha_max, alpha_cutoff, g_img=None, g_depth=None, g_alpha=None, bg=None,
              aux=False, allowances=True):
    rec = np.asarray(rec, np.float64)
    n, ns = len(rec), 10 if aux else 9
    th = (float(chi), float(alpha_max), float(alpha_cutoff))
    gi, gd, ga = _upstream(H, W, g_img, g_depth, g_alpha)
    if not aux:
        assert g_depth is None and g_alpha is None and bg is None
        rec = rec.copy()
        rec[:, 11] = 0.0
    ref = Reference()
    ref.H, ref.W, ref.n, ref.ns, ref.lists_x, ref.aux = H, W, n, ns, lists_x, aux
    ref.ranges, ref.sorted_ids = np.asarray(ranges, np.int64), np.asarray(sorted_ids, np.int64)
    ref.image, ref.accum = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    ref.depth, ref.alpha = np.zeros((H, W)), np.zeros((H, W))
    if bg is not None:
        ref.image[:] = np.clip(np.asarray(bg, np.float64), 0, 1)
    ref.has_bg = bg is not None
    ref.scale_img = dict(image=np.ones((H, W, 3)), accum=np.ones((H, W, 3)), depth=np.ones((H, W)), alpha=np.ones((H, W)))
    ref.allow_img = dict(image=np.zeros((H, W, 3)), accum=np.zeros((H, W, 3)), depth=np.zeros((H, W)), alpha=np.zeros((H, W)))
    rows, scale, allow = np.zeros((n, 10)), np.zeros((n, 10)), np.zeros((n, 10))
    cap = len(ref.sorted_ids)
    ref.pair_scale = np.zeros((cap, 10))
    ref.pair_list = np.full(cap, -1, np.int64)
    ref.dec = {k: np.zeros((cap, 128), bool) for k in ("q", "cut", "max", "alive")}
    ref.dec["col"] = np.ones((H, W, 3), bool)
    ref.band = {k: np.zeros((cap, 128), bool) for k in ("q", "cut", "max", "alive")}
    ref.band["col"] = np.zeros((H, W, 3), bool)
    ref.band_upto = np.zeros((cap, 128), bool)
    ref.band_pixels = np.zeros((H, W), bool)
    ref.in_list = np.zeros(n, bool)
    ref.n_flips = 0
    for l_ in np.nonzero(ref.ranges[:, 1] > ref.ranges[:, 0])[0]:
        s0, s1 = ref.ranges[l_]
        g = ref.sorted_ids[s0:s1]
        ref.in_list[g] = True
        ref.pair_list[s0:s1] = l_
        px, py = _list_pixels(l_, lists_x)
        valid = (px < W) & (py < H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        vf = valid.astype(np.float64)
        r = rec[g]
        o = _columns(r, px.astype(np.float64), py.astype(np.float64), vf, th, gi[cy, cx] * vf[:, None], gd[cy, cx] * vf, ga[cy, cx] * vf, bg)
        yv, xv = py[valid], px[valid]
        ref.image[yv, xv], ref.accum[yv, xv] = o["image"][valid], o["C"][valid]
        ref.depth[yv, xv], ref.alpha[yv, xv] = o["D"][valid], o["A"][valid]
        ref.scale_img["image"][yv, xv] = ref.scale_img["accum"][yv, xv] = o["s_col"][valid]
        ref.scale_img["depth"][yv, xv], ref.scale_img["alpha"][yv, xv] = o["s_D"][valid], o["s_A"][valid]
        np.add.at(rows, g, o["rows"])
        np.add.at(scale, g, o["scale"])
        ref.pair_scale[s0:s1] = o["scale"]
        # decisions and band
        idx = np.arange(len(g))[:, None]
        b_alive = (np.abs(o["T"] - T_MIN) <= T_MIN * K_B * EPS * (idx + 1)) & valid[None, :]
        eff = (o["alive"] | b_alive) & valid[None, :]                    # the pixel still decides something
        b_q = (np.abs(o["q"] - th[0]) <= o["qb"]) & eff
        rel = o["og"] * (K_B * EPS + 0.5 * o["qb"])
        inexact = (o["du"] != 0) | (o["dv"] != 0)                        # at the centre exp(-q / 2) = 1 and o g = o in any arithmetic
        b_cut = (np.abs(o["og"] - th[2]) <= rel) & eff & (o["pq"] | b_q) & inexact
        b_max = (np.abs(o["og"] - th[1]) <= rel) & eff & (o["pq"] | b_q) & inexact
        b_col = ((np.abs(o["shown"]) <= K_B * EPS * o["s_col"]) | (np.abs(o["shown"] - 1.0) <= K_B * EPS * o["s_col"])) & (valid & (o["A"] > 0))[:, None]
        for k, b in (("q", b_q), ("cut", b_cut), ("max", b_max), ("alive", b_alive)):
            ref.band[k][s0:s1] = b
        ref.dec["q"][s0:s1], ref.dec["cut"][s0:s1], ref.dec["max"][s0:s1], ref.dec["alive"][s0:s1] = o["pq"], o["po"], o["pc"], o["alive"]
        ref.dec["col"][yv, xv], ref.band["col"][yv, xv] = o["cm"][valid], b_col[valid]
        any_b = b_q | b_cut | b_max | b_alive
        ref.band_upto[s0:s1] = np.maximum.accumulate(any_b, 0)
        bp = any_b.any(0) | b_col.any(1)
        ref.band_pixels[yv, xv] = bp[valid]
        if not allowances:
            continue
        flips = [(k, int(i), int(p)) for k, b in (("q", b_q), ("cut", b_cut), ("max", b_max), ("alive", b_alive)) for i, p in np.argwhere(b)]
        flips += [("col", 0, int(p), int(c)) for p, c in np.argwhere(b_col)]
        base = {}
        for f in flips:
            p = f[2]
            args = (r, np.array([float(px[p])]), np.array([float(py[p])]), vf[p:p + 1], th, gi[cy[p], cx[p]][None, :] * vf[p], gd[cy[p], cx[p]][None] * vf[p],
                    ga[cy[p], cx[p]][None] * vf[p], bg)
            if p not in base:
                base[p] = _columns(*args)
            b0, b1 = base[p], _columns(*args, force=(f[0], f[1]) + tuple(f[3:]))
            np.add.at(allow, g, np.abs(b1["rows"] - b0["rows"]))
            y, x = py[p], px[p]
            ref.allow_img["image"][y, x] += np.abs(b1["image"][0] - b0["image"][0])
            ref.allow_img["accum"][y, x] += np.abs(b1["C"][0] - b0["C"][0])
            ref.allow_img["depth"][y, x] += abs(b1["D"][0] - b0["D"][0])
            ref.allow_img["alpha"][y, x] += abs(b1["A"][0] - b0["A"][0])
            ref.n_flips += 1
    ref.rows = np.zeros((n, 16))
    ref.rows[:, :ns] = rows[:, :ns]
    ref.scale, ref.allow = scale[:, :ns], allow[:, :ns]
    ref.pair_scale = ref.pair_scale[:, :ns]
    ref.band_share = float(ref.band_pixels.mean())
    return ref


# ---- the float32 mode ---------------------------------------------------------------------------------------------------------------

QK = np.float32(-0.72134752044448170368)


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def composite_f32(rec, ranges, sorted_ids, lists_x, H, W, chi, alpha_max, alpha_cutoff, g_img=None, g_depth=None, g_alpha=None, bg=None,
                  aux=False, strict_clamp=False, ignore_image_clamp=False, ragged_bug=False):
    """The rule in float32, in the kernels' order of operations; all lists advance together, one entry per step.  Returns a dict: image,
    accum, depth, alpha, accum_aux, grad2d [n,16] (float32), pair_sub [capacity,8,ns] (the sums of every (pair, sub-tile)), dec (the
    decisions, as in Reference.dec).  The last three switches restate three kernel faults for tests/test_raster_oracle_cpu.py: `og < alpha_max`
    in the clamp gradient, the image clamp mask ignored, the pixel column right of a ragged image composited."""
    f = np.float32
    rec = np.asarray(rec, f)
    n, ns = len(rec), 10 if aux else 9
    ranges, sorted_ids = np.asarray(ranges, np.int64), np.asarray(sorted_ids, np.int64)
    chi, amax, cut = (f(x) for x in (chi, alpha_max, alpha_cutoff))
    chik, tmin = f(chi * QK), f(T_MIN)
    gi, gd, ga = _upstream(H, W, g_img, g_depth, g_alpha, f)
    ln = ranges[:, 1] - ranges[:, 0]
    ls = np.argsort(-ln, kind="stable")
    ls = ls[ln[ls] > 0]
    nl, cap = len(ls), len(sorted_ids)
    px = np.stack([_list_pixels(l_, lists_x)[0] for l_ in ls]) if nl else np.zeros((0, 128), np.int64)
    py = np.stack([_list_pixels(l_, lists_x)[1] for l_ in ls]) if nl else np.zeros((0, 128), np.int64)
    valid = (px < (W + 1 if ragged_bug else W)) & (py < H)
    cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
    fpx, fpy = px.astype(f), py.astype(f)
    dec = {k: np.zeros((cap, 128), bool) for k in ("q", "cut", "max", "alive")}

    def staged(i, m):
        pos = ranges[ls[:m], 0] + i
        r = rec[sorted_ids[pos]]
        return pos, r, QK * r[:, 2:3], (f(2) * QK) * r[:, 3:4], QK * r[:, 4:5]

    def quad(r, k11, k12, k22, m):
        du, dv = fpx[:m] - r[:, 0:1], fpy[:m] - r[:, 1:2]
        q = (k11 * du * du) + dv * ((k12 * du) + k22 * dv)
        return du, dv, q, np.exp2(q)

    # forward
    T = valid.astype(f)
    C = np.zeros((nl, 128, 3), f)
    D, A = np.zeros((nl, 128), f), np.zeros((nl, 128), f)
    for i in range(int(ln.max(initial=0))):
        m = int((ln[ls] > i).sum())
        pos, r, k11, k12, k22 = staged(i, m)
        du, dv, q, g = quad(r, k11, k12, k22, m)
        al = np.minimum(r[:, 5:6] * g, amax)
        al = np.where((q >= chik) & (al >= cut) & (T[:m] > tmin), al, f(0))
        w = al * T[:m]
        T[:m] = T[:m] - al * T[:m]
        C[:m] += w[:, :, None] * r[:, None, 8:11]
        if aux:
            D[:m] += w * r[:, 11:12]
            A[:m] += w
    has_bg = bg is not None
    bgf = np.asarray(bg if has_bg else (0, 0, 0), f)
    shown = np.stack([_fma(f(1) - A, bgf[c], C[:, :, c]) for c in range(3)], -1) if has_bg else C
    out = dict(image=np.zeros((H, W, 3), f), accum=np.zeros((H, W, 3), f), depth=np.zeros((H, W), f), alpha=np.zeros((H, W), f))
    if has_bg:
        out["image"][:] = np.clip(bgf, 0, 1)
    v = valid & (px < W)
    out["image"][py[v], px[v]], out["accum"][py[v], px[v]] = np.clip(shown[v], f(0), f(1)), C[v]
    out["depth"][py[v], px[v]], out["alpha"][py[v], px[v]] = D[v], A[v]
    out["accum_aux"] = np.stack([out["depth"], out["alpha"]], -1)
    if not aux:
        out["depth"] = out["alpha"] = out["accum_aux"] = None
    dec["col"] = np.ones((H, W, 3), bool)
    cm = (shown >= 0) & (shown <= 1)
    dec["col"][py[v], px[v]] = cm[v]
    if ignore_image_clamp:
        cm = np.ones_like(cm)
    # backward
    G = np.where(cm, gi[cy, cx], f(0)) * valid[:, :, None]
    Gd, Ga = gd[cy, cx] * valid, ga[cy, cx] * valid
    suffix = np.zeros((nl, 128), f)
    for c in range(3):
        suffix += G[:, :, c] * C[:, :, c]
        if has_bg:
            Ga = Ga - G[:, :, c] * bgf[c]
    if aux:
        suffix += Gd * D + Ga * A
    T = valid.astype(f)
    pair_sub = np.zeros((cap, 8, ns), f)

    def sub(x):                    # [m,128] -> [m,8]: the sums over the 16 pixels of each 4 x 4 sub-tile (bit 4 (y / 4) + x / 4)
        return x.reshape(-1, 2, 4, 4, 4).sum((2, 4), dtype=f).reshape(-1, 8)

    for i in range(int(ln.max(initial=0))):
        m = int((ln[ls] > i).sum())
        pos, r, k11, k12, k22 = staged(i, m)
        du, dv, q, g = quad(r, k11, k12, k22, m)
        og = r[:, 5:6] * g
        iq, io = q >= chik, og >= cut
        ic = (og < amax) if strict_clamp else (og <= amax)
        p = iq & io
        al = np.where(p, np.minimum(og, amax), f(0))
        alive = T[:m] > tmin
        dec["q"][pos], dec["cut"][pos], dec["max"][pos], dec["alive"][pos] = iq, io, og <= amax, alive
        w = np.where(alive, al * T[:m], f(0))
        sdot = r[:, 8:9] * G[:m, :, 0] + r[:, 9:10] * G[:m, :, 1] + r[:, 10:11] * G[:m, :, 2]
        if aux:
            sdot = sdot + (r[:, 11:12] * Gd[:m] + Ga[:m])
        suffix[:m] -= w * sdot
        om = f(1) / (f(1) - al)
        dal = np.where(alive & p & ic, T[:m] * sdot - suffix[:m] * om, f(0))
        ao = dal * g
        dva = dv * ao
        cols = [du * ao, dva, du * (du * ao), du * dva, dv * dva, ao, w * G[:m, :, 0], w * G[:m, :, 1], w * G[:m, :, 2]]
        if aux:
            cols.append(w * Gd[:m])
        for k, x in enumerate(cols):
            pair_sub[pos, :, k] = sub(x)
        T[:m] = T[:m] - al * T[:m]
    out.update(pair_sub=pair_sub, dec=dec, grad2d=rows_from_pairs(pair_sub, ranges, sorted_ids, n))
    return out


def rows_from_pairs(pair_sub, ranges, sorted_ids, n):
    """grad2d [n,16] float32 from the sums of every (pair, sub-tile): sub-tiles added in order, then the Gaussian's lists in list order."""
    f = np.float32
    per_pair = np.zeros(pair_sub.shape[::2], f)
    for t in range(8):
        per_pair += pair_sub[:, t]
    g2d = np.zeros((n, 16), f)
    ranges = np.asarray(ranges, np.int64)
    for l_ in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        s0, s1 = ranges[l_]
        g2d[np.asarray(sorted_ids[s0:s1], np.int64), :per_pair.shape[1]] += per_pair[s0:s1]          # (a Gaussian is in a list once)
    return g2d


def chunk_layout(ranges, pair_mask):
    """How the backward kernel cuts every list into chunks (stage_chunk with the queue cap): per pair position in sorted_ids the chunk
    number and the position inside the chunk; and the list of (list, first, n, cut) per chunk.  A chunk offers min(64, rest) entries and
    is cut by 4 at a time, not below 24, until no sub-tile queue holds more than 24."""
    ranges = np.asarray(ranges, np.int64)
    chunk_no, chunk_pos = np.zeros(len(pair_mask), np.int64), np.zeros(len(pair_mask), np.int64)
    chunks = []
    bits = ((np.asarray(pair_mask, np.uint8)[:, None] >> np.arange(8)[None, :]) & 1).astype(np.int64)
    for l_ in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        base, end, c = ranges[l_, 0], ranges[l_, 1], 0
        while base < end:
            n0 = n = int(min(end - base, CHUNK))
            while bits[base:base + n].sum(0).max() > MAXQ_BWD:
                n = max(n - 4, MAXQ_BWD)
            chunk_no[base:base + n], chunk_pos[base:base + n] = c, np.arange(n)
            chunks.append((int(l_), int(base), n, n < n0))
            base, c = base + n, c + 1
    return chunk_no, chunk_pos, chunks


# ---- the comparison -------------------------------------------------------------------------------------------------------------------

MAPS = ("image", "accum", "depth", "alpha")


def _where_pair(ref, gauss, col, pair_mask):
    """The (list, entry) that carries most of column `col` of Gaussian `gauss`, for the failure message."""
    pos = np.nonzero((ref.sorted_ids == gauss) & (ref.pair_list >= 0))[0]
    lists = ref.pair_list[pos]
    if len(pos) == 0:
        return "in no list"
    k = int(np.argmax(ref.pair_scale[pos, col]))
    rank = int(pos[k] - ref.ranges[lists[k], 0])
    txt = f"list {int(lists[k])}, entry {rank}"
    if pair_mask is not None:
        cn, cp, _ = chunk_layout(ref.ranges, pair_mask)
        txt += f" (backward chunk {int(cn[pos[k]])}, position {int(cp[pos[k]])} in the chunk)"
    else:
        txt += f" (position {rank % CHUNK} of forward chunk {rank // CHUNK})"
    return txt


def ratios(dev, ref):
    """Largest (|delta| - allowance)+ / (2^-24 scale) per output kind, over what `dev` holds (maps by name, grad2d [n,16])."""
    out = {}
    for name in MAPS:
        if dev.get(name) is not None:
            d = np.abs(np.asarray(dev[name], np.float64) - getattr(ref, name))
            x = np.maximum(d - ref.allow_img[name], 0.0) / (EPS * ref.scale_img[name])
            out["image"] = max(out.get("image", 0.0), float(x.max(initial=0.0)))
    if dev.get("grad2d") is not None:
        d = np.maximum(np.abs(np.asarray(dev["grad2d"], np.float64)[:, :ref.ns] - ref.rows[:, :ref.ns]) - ref.allow, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(d > 0, d / (EPS * ref.scale), 0.0)
        out["moments"] = float(x[:, :6].max(initial=0.0))
        out["colour"] = float(x[:, 6:].max(initial=0.0))
    return out


def check(dev, ref, K, what="", pair_mask=None):
    """dev: dict with any of image, accum, depth, alpha, accum_aux [H,W,2] (= depth, alpha), grad2d [n,16].  Every value within
    K[kind] 2^-24 scale + allowance of the reference; grad2d's columns ns .. 15 and the rows of Gaussians in no list exact zeros.  Raises
    RasterError naming the pixel, or the Gaussian, its column and the (list, entry) that carries most of it.  Returns ratios(dev, ref)."""
    dev = dict(dev)
    if dev.get("accum_aux") is not None:
        aa = np.asarray(dev["accum_aux"])
        for k, name in enumerate(("depth", "alpha")):
            if dev.get(name) is not None and not np.array_equal(np.asarray(dev[name]), aa[..., k]):
                y, x = np.argwhere(np.asarray(dev[name]) != aa[..., k])[0]
                raise RasterError(f"{what}: pixel ({y}, {x}): accum_aux holds {aa[y, x, k]!r}, the {name} map {np.asarray(dev[name])[y, x]!r}")
            dev.setdefault(name, aa[..., k])
    for name in MAPS:
        if dev.get(name) is None:
            continue
        got = np.asarray(dev[name], np.float64)
        want = getattr(ref, name)
        if got.shape != want.shape or not np.isfinite(got).all():
            raise RasterError(f"{what}: {name}: shape {got.shape} (expected {want.shape}) or non-finite values")
        bound = K["image"] * EPS * ref.scale_img[name] + ref.allow_img[name]
        bad = np.argwhere(np.abs(got - want) > bound)
        if len(bad):
            i = tuple(bad[np.argmax((np.abs(got - want) / bound)[tuple(bad.T)])])
            raise RasterError(f"{what}: pixel ({i[0]}, {i[1]}){' channel ' + str(i[2]) if len(i) > 2 else ''} of {name}: {got[i]!r}, reference {want[i]!r}: "
                              f"|delta| {abs(got[i] - want[i]):.3e} > {bound[i]:.3e} (= {K['image']:.1f} x 2^-24 x {ref.scale_img[name][i]:.3e} + {ref.allow_img[name][i]:.3e})")
    if dev.get("image") is not None and dev.get("accum") is not None and bg_free(ref):
        a = np.asarray(dev["accum"])
        if not np.array_equal(np.asarray(dev["image"]), np.clip(a, 0, 1)):
            y, x, c = np.argwhere(np.asarray(dev["image"]) != np.clip(a, 0, 1))[0]
            raise RasterError(f"{what}: pixel ({y}, {x}) channel {c}: image {np.asarray(dev['image'])[y, x, c]!r} is not the clamp of accum {a[y, x, c]!r}")
    if dev.get("grad2d") is not None:
        g = np.asarray(dev["grad2d"], np.float64)
        if g.shape != (ref.n, 16) or not np.isfinite(g).all():
            bad = np.argwhere(~np.isfinite(g)) if g.shape == (ref.n, 16) else []
            raise RasterError(f"{what}: grad2d: shape {g.shape} or non-finite values" + (f" (Gaussian {bad[0][0]}, column {bad[0][1]})" if len(bad) else ""))
        bad = np.argwhere(g[:, ref.ns:] != 0)
        if len(bad):
            raise RasterError(f"{what}: Gaussian {bad[0][0]}, padding column {ref.ns + bad[0][1]}: {g[bad[0][0], ref.ns + bad[0][1]]!r}, must be an exact zero")
        bad = np.argwhere((g != 0) & ~ref.in_list[:, None])
        if len(bad):
            raise RasterError(f"{what}: Gaussian {bad[0][0]} is in no list, column {bad[0][1]} of its row is {g[tuple(bad[0])]!r}")
        kk = np.array([K["moments"]] * 6 + [K["colour"]] * (ref.ns - 6))
        bound = kk[None, :] * EPS * ref.scale + ref.allow
        d = np.abs(g[:, :ref.ns] - ref.rows[:, :ref.ns])
        bad = np.argwhere(d > bound)
        if len(bad):
            with np.errstate(divide="ignore", invalid="ignore"):
                over = np.where(bound > 0, d / bound, np.inf)
            i, c = bad[np.argmax(over[tuple(bad.T)])]
            raise RasterError(f"{what}: Gaussian {i}, column {c}: {g[i, c]!r}, reference {ref.rows[i, c]!r}: |delta| {d[i, c]:.3e} > {bound[i, c]:.3e} "
                              f"(= {kk[c]:.1f} x 2^-24 x {ref.scale[i, c]:.3e} + {ref.allow[i, c]:.3e}); {len(bad)} values beyond their bounds; "
                              f"most of it from {_where_pair(ref, i, c, pair_mask)}")
    return ratios(dev, ref)


def bg_free(ref):
    return not ref.has_bg


def decisions_outside_band(ref, dec):
    """How many decisions `dec` (composite_f32's, or any other evaluation's) takes differently from the reference outside the band.  A
    decision counts where the pixel decides something (see the module docstring) and no decision of the same pixel at or before that
    entry is in the band (a flip there moves every T behind it)."""
    n = 0
    gate = ~ref.band_upto
    alive = ref.dec["alive"]
    n += int(((dec["q"] != ref.dec["q"]) & gate & alive).sum())
    both = ref.dec["q"] & dec["q"] & gate & alive
    n += int(((dec["cut"] != ref.dec["cut"]) & both).sum())
    n += int(((dec["max"] != ref.dec["max"]) & both).sum())
    n += int(((dec["alive"] != ref.dec["alive"]) & gate).sum())
    n += int(((dec["col"] != ref.dec["col"]) & ~ref.band["col"] & ~ref.band_pixels[:, :, None]).sum())
    return n
