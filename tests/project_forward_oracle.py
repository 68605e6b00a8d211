"""Float64 reference of K1 / K1b (project_kernel, colour_kernel) for any of their modes, Gaussian by Gaussian (helper, not a test).

Built on project_backward_oracle.Stage: Stage.out [V,10] (u, v, A11, A12, A22, opacity_record, r, g, b, z) is the record's columns
0..5 and 8..11 of the V Gaussians the oracle keeps.  check() holds every value to

    |got - ref| <= K[group, kind] * 2^-24 * scale + floor,      floor = 2^-24 * 2^-24 * the group's largest scale in the scene,

scale = |out_j| + sum_k |d out_j / d theta_k| |theta_k| over the Gaussian's own parameters and the twelve entries of c2w: what one
float32 rounding of an input moves the value by -- its forward condition scale (one autograd pass per column; Gaussians are
independent, so the pass of column j hands every parameter entry its own derivative).  max(|u|, 1) would not do: u = fx x / z + cx
with (x, y, z) = W (p - e), a difference that the naive scale does not see.  Groups: uv, conic, opacity, rgb, z, kj.  K = util.K_CAL x
the largest ratio of the FLOAT32 ORACLE (Stage(dtype=torch.float32)) in that (group, kind) of the same scene and mode; a kind with
fewer than MIN_ROWS rows in a scene takes the largest K of the scenes of the same mode (`other`).  Kinds: pbo.kinds.

kj [V,12], the saved SH Jacobian: kj[:3] = c (1 - c) of the colour, kj[3 + 3 ch + m] = d logit_ch / d p_m, by float64 autograd through
torch_port's SH basis over the active bands; its scale by a second pass through the same graph.

Derived columns are checked against float64 formulas evaluated on THE RECORD'S OWN float32 values, so that what is left is the
arithmetic of that expression alone.  In units of 2^-24 relative (one rounding to nearest; GS_RCP_FAST and GS_SQRT_FAST 1 ulp = 2):

    D  = A11 A22 - A12^2          one rounding per product, one of the difference:   1 + kappa,  kappa = (A11 A22 + A12^2) / D
    ex = sqrt(chi rcp(D) A22) 1.0001 + 0.01:   under the root  (1 + kappa) + 2 (rcp) + 1 + 1 = 5 + kappa,  halved by the root,
         + 2 (sqrt) + 1 (x 1.0001f) + 1 (+ 0.01f)  =  6.5 + 0.5 kappa             ->  C0_EXT = 7 (the half for the second-order terms), C1_EXT = 0.5
    bk4[0] = -A12 rcp(A11), bk4[1] = chi_pad rcp(A11):   2 + 1 = 3
    bk4[2] = D rcp(A11) rcp(A11):   (1 + kappa) + 2 + 1 + 2 + 1 = 7 + kappa
    bk4[3] = A12 rcp(A22) ex:   2 + 1 + 1 = 4
(1.0001f, 0.01f, chi and chi_pad are the float32 constants the kernels hold.)  A conic that is not positive definite has ex = ey = 1e30.
"""
import numpy as np
import torch

from oracle import torch_port as tp
from tests import project_backward_oracle as pbo
from tests import util

EPS = pbo.EPS
MIN_ROWS = 4
GROUPS = {"uv": (0, 1), "conic": (2, 3, 4), "opacity": (5,), "rgb": (6, 7, 8), "z": (9,)}
REC_COLS = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)           # the record column of Stage.out's column j
C0_EXT, C1_EXT = 7.0, 0.5
BK4_C = ((3.0, 0.0), (3.0, 0.0), (7.0, 1.0), (4.0, 0.0))
MAX_BOUNDARY_SHARE = 0.03
SCENES = tuple(f"synth{n}" for n in pbo.SIZES) + pbo.GOLDENS


def scene(name):
    """pbo.scene with the synthetic scenes' added cull reasons (more_culls), and `synth200u`: the un-fused twin of synth200."""
    if name == "synth200u":
        s = pbo.synthetic(200, more_culls=True)
        return (s,) + unfused_inputs(s)
    if name.startswith("synth"):
        return pbo.synthetic(int(name[5:]), more_culls=True), None, None
    return pbo.scene(name)


def unfused_inputs(s):
    """(color, sigma) of a fused scene for the un-fused entry: the oracle's build_sigma / evaluate_sh in float64, rounded once."""
    t = {k: torch.tensor(s[k], dtype=torch.float64) for k in ("pos", "f_dc", "f_rest", "scale_raw", "q_raw", "c2w")}
    sigma = tp.covariance_from_params(t["scale_raw"], t["q_raw"]).numpy()
    color = tp.sh_colour(t["f_dc"], t["f_rest"], t["pos"], t["c2w"]).numpy()
    return np.ascontiguousarray(color, np.float32), np.ascontiguousarray(sigma, np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------

def _logits(f_dc, f_rest, pos, eye, degree):
    if degree < 3:
        f_rest = f_rest * torch.tensor(~tp.inactive_columns(degree), dtype=f_rest.dtype)
    coeff = torch.cat([f_dc.unsqueeze(1), f_rest.reshape(-1, 3, 15).transpose(1, 2)], 1)
    d = pos - eye
    d = d / (d.norm(dim=-1, keepdim=True) + 1e-8)
    return (coeff * tp.sh_basis(d).unsqueeze(-1)).sum(1)


def _kj(s, ids, degree, dtype, scale):
    """kj [V,12] of the Gaussians ids in dtype (as float64 numpy), and with `scale` its condition scale [V,12]."""
    V = len(ids)
    t = lambda a: torch.tensor(np.asarray(a, np.float64)[ids], dtype=dtype, requires_grad=True)
    f_dc, f_rest, pos = t(s["f_dc"]), t(s["f_rest"]), t(s["pos"])
    eye = torch.tensor(np.tile(np.asarray(s["c2w"], np.float64)[:3, 3], (V, 1)), dtype=dtype, requires_grad=True)
    lg = _logits(f_dc, f_rest, pos, eye, degree)
    c = torch.sigmoid(lg)
    rows = [torch.autograd.grad(lg[:, ch].sum(), pos, create_graph=True, allow_unused=True)[0] for ch in range(3)]
    rows = [r if r is not None else torch.zeros_like(pos) for r in rows]
    val = torch.cat([c * (1 - c)] + rows, 1)
    out = val.detach().double().numpy()
    if not scale:
        return out, None
    leaves = [f_dc, f_rest, pos, eye]
    sc = np.abs(out)
    for j in range(12):
        if not val[:, j].requires_grad:
            continue
        for lf, g in zip(leaves, torch.autograd.grad(val[:, j].sum(), leaves, retain_graph=True, allow_unused=True)):
            if g is not None:
                sc[:, j] += (g.detach().abs() * lf.detach().abs()).sum(1).double().numpy()
    return out, sc


class Reference:
    """n, ids [V] (the Gaussians the oracle keeps, VIS_OK), out / scale [n,10], kj / kj_scale [n,12] (fused; NaN outside ids), kind [n],
    tile_rect [V,4], n_survivors, n_visible, n_pairs, lam_max [V] (the clamped larger eigenvalue), s (the scene), fused, degree."""


def reference(s, degree=3, lowpass=0.0, antialias=False, color=None, sigma=None, dtype=torch.float64, scale=True):
    """The forward reference of a scene and mode.  dtype = torch.float32 (scale = False): the same evaluation in the reference's own
    arithmetic -- the calibration."""
    stg = pbo.Stage(s, degree, lowpass, antialias, color, sigma, dtype)
    ref = Reference()
    ref.s, ref.n, ref.ids, ref.fused, ref.degree = s, stg.n, stg.ids, stg.fused, degree
    ref.kind = pbo.kinds(stg) if dtype == torch.float64 else None
    ref.out = np.full((stg.n, 10), np.nan)
    ref.scale = np.full((stg.n, 10), np.nan)
    ref.kj = np.full((stg.n, 12), np.nan)
    ref.kj_scale = np.full((stg.n, 12), np.nan)
    ref.n_survivors = int(stg.st.get("n_survivors", 0))
    ref.n_visible = len(stg.ids)
    ref.tile_rect = np.zeros((0, 4), np.int64)
    ref.n_pairs = 0
    ref.lam_max = np.zeros(0)
    if not len(stg.ids):
        return ref
    ids = stg.ids
    ref.out[ids] = stg.out.detach().double().numpy()
    ref.tile_rect = stg.st["tile_rect"].numpy()
    tr = ref.tile_rect
    ref.n_pairs = int(((tr[:, 2] - tr[:, 0] + 1) * (tr[:, 3] - tr[:, 1] + 1)).sum())
    ref.lam_max = stg.st["evals"].detach().double().numpy()[:, 1]
    if scale:
        assert dtype == torch.float64
        sc = np.abs(ref.out[ids])
        names = list(stg.names)
        leaves = [stg.leaves[k] for k in names]
        for j in range(10):
            if not stg.out[:, j].requires_grad:
                continue
            for lf, g in zip(leaves, torch.autograd.grad(stg.out[:, j].sum(), leaves, retain_graph=True, allow_unused=True)):
                if g is not None:
                    sc[:, j] += (g.detach().abs() * lf.detach().abs()).reshape(stg.n, -1).sum(1).numpy()[ids]
        for (r, c), col in stg.jacobian_c2w().items():
            sc += np.abs(col.numpy()) * abs(float(s["c2w"][r, c]))
        ref.scale[ids] = sc
    if stg.fused:
        kj, ksc = _kj(s, ids, degree, dtype, scale)
        ref.kj[ids] = kj
        if scale:
            ref.kj_scale[ids] = ksc
    return ref


def radius_ties(ref):
    """The visible Gaussians (indices into ids) whose 2.5 sqrt(lambda_max) lies within 4 ulp of an integer: float32 may round the
    radius the other way, and n_pairs may then differ by that Gaussian's tiles (the rule of tests/test_gpu_fullsize.py).  Not an
    eigenvalue AT the clamp: 1e4 is the same number in both precisions, its radius 250 exactly."""
    r = 2.5 * np.sqrt(np.clip(ref.lam_max, 1e-12, 1e4))
    return np.nonzero((np.abs(r - np.round(r)) <= 4 * 2.0 ** -23 * r) & (ref.lam_max != 1e4))[0]


# ---- the record, value by value ------------------------------------------------------------------------------------------------

def _group_arrays(rec, kj, ref):
    """{group: (got [n,c], want [n,c], scale [n,c], column names)}"""
    rec = np.asarray(rec, np.float64)
    out = {}
    for g, cols in GROUPS.items():
        out[g] = (rec[:, [REC_COLS[j] for j in cols]], ref.out[:, cols], ref.scale[:, cols], [pbo.COLUMNS[j] for j in cols])
    if kj is not None and ref.fused:
        out["kj"] = (np.asarray(kj, np.float64), ref.kj, ref.kj_scale, [f"kj{j}" for j in range(12)])
    return out


def ratios(rec, kj, ref):
    """{group: (ratio [n] -- the largest of the Gaussian's values in the group, inf for a non-finite one, 0 outside ids --, worst
    column index [n])}: (|got - ref| - floor)+ / (2^-24 scale)."""
    out = {}
    vis = np.zeros(ref.n, bool)
    vis[ref.ids] = True
    for g, (got, want, sc, _) in _group_arrays(rec, kj, ref).items():
        r = np.zeros(got.shape)
        if vis.any():
            floor = EPS * EPS * np.nanmax(sc[vis])
            with np.errstate(divide="ignore", invalid="ignore"):
                excess = np.maximum(np.abs(got[vis] - want[vis]) - floor, 0.0)
                rv = np.where(excess == 0.0, 0.0, excess / (EPS * sc[vis]))
            rv[~np.isfinite(got[vis])] = np.inf
            r[vis] = rv
        out[g] = (r.max(1), r.argmax(1))
    return out


def worst(rat, ref):
    """{(group, kind): (the largest ratio, rows)} over the compared rows (no boundary rows, no culled ones)."""
    out = {}
    for g, (r, _) in rat.items():
        for kd in set(ref.kind.tolist()) - {"boundary", "culled"}:
            m = ref.kind == kd
            out[(g, kd)] = (float(r[m].max()), int(m.sum()))
    return out


def calibrate(ref, ref32):
    """(K, rows): K[group, kind] = util.K_CAL x the float32 oracle's largest ratio; rows[group, kind] the rows it was taken over.  The
    float32 oracle must keep the same Gaussians."""
    assert np.array_equal(np.sort(ref.ids), np.sort(ref32.ids)), "the float32 oracle culls differently from float64"
    rec = np.zeros((ref.n, 16))
    rec[:, list(REC_COLS)] = np.nan_to_num(ref32.out)
    w = worst(ratios(rec, np.nan_to_num(ref32.kj) if ref.fused else None, ref), ref)
    return {k: util.K_CAL * v[0] for k, v in w.items()}, {k: v[1] for k, v in w.items()}


def merge_K(Ks):
    return pbo.merge_K(Ks)


def bound_of(K, rows, other, key):
    k = K.get(key, 0.0)
    if rows.get(key, 0) < MIN_ROWS:
        k = max(k, (other or {}).get(key, 0.0))
    return k


# Rows held to the K of their group over ALL kinds of the same scene and mode (still K_CAL x the float32 oracle, never the code under
# test), each with its cause: {(scene, degree, filter): {(group, Gaussian)}}.  The kinds sort by the covariance's clamps and condition,
# which the colour, kj, (u, v) and z do not depend on: a kind of a few rows is then one draw of the float32 oracle's rounding of a
# quantity whose error is the same in every kind.
KNOWN_ROWS = {
    # kj5 at 9.4 roundings against the 2.8 of its kind's five rows; the float32 oracle reaches 28 in the same scene (host build: 19)
    ("synth129", 2, "off"): {("kj", 42)}, ("synth129", 2, "lowpass"): {("kj", 42)}, ("synth129", 2, "antialias"): {("kj", 42)},
    # kj5 = d logit_r / d p_z of a Gaussian near the optical axis: the component along the view direction, what g - d (d . g) leaves, 1 / 13
    # of the row's other entries.  The float32 oracle sits at 11.9 on this row (the largest of its kind's five) and reaches 18.1 in the
    # scene; the host build 27.0, the device's contracted arithmetic 45.9
    ("synth200", 2, "off"): {("kj", 152)}, ("synth200", 2, "lowpass"): {("kj", 152)}, ("synth200", 2, "antialias"): {("kj", 152)},
    # kj8 at 8.9 against the 2.2 of the thirteen scale-clamped rows; the float32 oracle reaches 25 in the same scene
    ("g7_tiny", 1, "off"): {("kj", 489)},
    # b at 1.1 roundings: the only `free c2` row of any scene, where the float32 oracle happens to sit at 0.25; it reaches 1.3 in the scene
    ("g7_tiny", 3, "off"): {("rgb", 236)},
}


def check_records(got, ref, K, rows, what, other=None, known=None):
    """Every value of every compared row within its bound; returns ({(group, kind): largest ratio}, failures)."""
    rat = ratios(got["rec"], got.get("kj"), ref)
    arrs = _group_arrays(got["rec"], got.get("kj"), ref)
    bad = []
    for g, (r, col) in rat.items():
        for i in ref.ids:
            kd = ref.kind[i]
            if kd == "boundary":
                continue
            bound = bound_of(K, rows, other, (g, kd))
            if (g, int(i)) in (known or ()):
                bound = max(v for (gg, _), v in K.items() if gg == g)
            if not r[i] <= bound:
                gv, wv, _, names = arrs[g]
                bad.append((r[i] / max(bound, 1e-300), f"{what}: {g}[{i}] (kind {kd}, lane {i % 64}, column {names[col[i]]}): {gv[i, col[i]]!r} against "
                            f"{wv[i, col[i]]!r}, ratio {r[i]:.3g} > K = {bound:.3g}"))
    return {k: v[0] for k, v in worst(rat, ref).items()}, bad


# ---- derived columns: the expression's own arithmetic ---------------------------------------------------------------------------

def unpack_rect(rect):
    rect = np.asarray(rect).astype(np.int64)
    return rect[:, 0] & 0xFFFF, rect[:, 0] >> 16, rect[:, 1] & 0xFFFF, rect[:, 1] >> 16


def check_derived(got, ref, what):
    """ex, ey (record columns 6, 7) from both sides, bk4 (12..15) and depth[] against the record's own float32 values."""
    rec32 = np.asarray(got["rec"], np.float32)
    rec = rec32.astype(np.float64)
    kw = ref.s["kwargs"]
    chi = float(np.float32(kw.get("chi_square_clip", 6.25)))
    chi_pad = float(np.float32(float(np.float32(kw.get("chi_square_clip", 6.25))) * 1.001 + 1e-4))
    k1, k0 = float(np.float32(1.0001)), float(np.float32(0.01))
    bad = []
    ids = ref.ids
    a11, a12, a22 = rec[ids, 2], rec[ids, 3], rec[ids, 4]
    D = a11 * a22 - a12 * a12
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = (a11 * a22 + a12 * a12) / D
        sure_pd = (D > 2 * EPS * (a11 * a22 + a12 * a12)) & (a11 > 0) & (a22 > 0)
        sure_not = (D < -2 * EPS * (a11 * a22 + a12 * a12)) | (a11 <= 0) | (a22 <= 0)
        for col, name, num in ((6, "ex", a22), (7, "ey", a11)):
            want = np.minimum(np.sqrt(chi * num / D) * k1 + k0, 1e30)
            tol = EPS * (C0_EXT + C1_EXT * kappa) * want
            g = rec[ids, col]
            for k, i in enumerate(ids):
                ok_pd = abs(g[k] - want[k]) <= tol[k] if np.isfinite(want[k]) else False
                ok_not = rec32[i, col] == np.float32(1e30)
                if not ((sure_pd[k] and ok_pd) or (sure_not[k] and ok_not) or (not sure_pd[k] and not sure_not[k] and (ok_pd or ok_not))):
                    bad.append((np.inf, f"{what}: {name}[{i}] (kind {ref.kind[i]}, lane {i % 64}, column {col}): {g[k]!r} against {want[k]!r} "
                                f"of the record's own conic, allowance {tol[k]:.3g}"))
    # bk4: the rows whose binned rectangle has more than 32 lists; exact zeros elsewhere
    x0, y0, x1, y1 = unpack_rect(got["rect"])
    area = (x1 - x0 + 1) * (y1 - y0 + 1)
    tiles = np.asarray(got["tiles"])
    for k, i in enumerate(ids):
        row = rec[i, 12:16]
        if tiles[i] and area[i] > 32:
            with np.errstate(divide="ignore", invalid="ignore"):
                pd = D[k] > 0 and a11[k] > 0 and a22[k] > 0 and rec[i, 6] < 1e30
                want = [-a12[k] / a11[k], chi_pad / a11[k] if pd else -1.0, D[k] / (a11[k] * a11[k]), a12[k] / a22[k] * rec[i, 6]]
            for c in range(4):
                if c == 1 and not (sure_pd[k] or sure_not[k]):
                    continue
                tol = EPS * (BK4_C[c][0] + BK4_C[c][1] * abs(kappa[k])) * abs(want[c])
                if not abs(row[c] - want[c]) <= tol:
                    bad.append((np.inf, f"{what}: bk4[{i}] (kind {ref.kind[i]}, lane {i % 64}, column {12 + c}): {row[c]!r} against {want[c]!r} of "
                                f"the record's own conic, allowance {tol:.3g}"))
        elif tiles[i] and rec32[i, 12:16].view(np.uint32).any():
            bad.append((np.inf, f"{what}: bk4[{i}] (kind {ref.kind[i]}, lane {i % 64}): {row!r} in a rectangle of {area[i]} lists, not exact zeros"))
    d = np.asarray(got["depth"], np.float32)
    for i in ids[d[ids].view(np.uint32) != rec32[ids, 11].view(np.uint32)]:
        bad.append((np.inf, f"{what}: depth[{i}] (kind {ref.kind[i]}, lane {i % 64}): {d[i]!r} is not the record's z {rec32[i, 11]!r}"))
    return bad


# ---- integers ---------------------------------------------------------------------------------------------------------------

def expected_counts(got, ref):
    """(n_survivors, n_visible, n_pairs, max_tiles_per_gaussian, n_binned): the first three from float64, the last two from tiles[]."""
    tiles = np.asarray(got["tiles"]).astype(np.int64)
    return (ref.n_survivors, ref.n_visible, ref.n_pairs, int(tiles.max()) if len(tiles) else 0, int(tiles.sum()))


def check_integers(got, ref, what, pairs_slack=0):
    """tiles == 0 (and record, rect, mask, kj exact zeros) for every row the float64 stage does not keep; a kept row has a record; the
    counters exact (pairs_slack: what the radius ties of a golden may move n_pairs by)."""
    bad = []
    keep = np.zeros(ref.n, bool)
    keep[ref.ids] = True
    tiles = np.asarray(got["tiles"])
    rec = np.asarray(got["rec"], np.float32).view(np.uint32)
    for i in np.nonzero(~keep & (tiles != 0))[0]:
        bad.append((np.inf, f"{what}: tiles[{i}] (kind culled, lane {i % 64}): {tiles[i]} lists for a Gaussian the oracle culls -- it is visible"))
    for k in ("rec", "rect", "mask", "kj"):
        if got.get(k) is not None:
            a = np.ascontiguousarray(got[k]).view(np.uint32).reshape(ref.n, -1)
            for i in np.nonzero(~keep & a.any(1))[0]:
                bad.append((np.inf, f"{what}: {k}[{i}] (kind culled, lane {i % 64}): the row of a culled Gaussian is not exact zeros"))
    for i in ref.ids[~rec[ref.ids].any(1)]:
        bad.append((np.inf, f"{what}: rec[{i}] (kind {ref.kind[i]}, lane {i % 64}): a visible Gaussian is reported culled (no record)"))
    if got.get("counts") is not None:
        want = expected_counts(got, ref)
        for name, g, w in zip(("n_survivors", "n_visible", "n_pairs", "max_tiles_per_gaussian", "n_binned"), got["counts"], want):
            if abs(int(g) - w) > (pairs_slack if name == "n_pairs" else 0):
                bad.append((np.inf, f"{what}: counter {name}: {int(g)} against {w}"))
    return bad


def check(got, ref, K, rows, what, other=None, known=None, pairs_slack=0):
    """got: rec [n,16], kj [n,12] or None, rect [n,2], depth [n], tiles [n], mask [n], counts (5-tuple) or None.  Raises AssertionError
    naming tensor, Gaussian, kind and column; returns the largest ratio per (group, kind)."""
    w, bad = check_records(got, ref, K, rows, what, other, known)
    bad += check_derived(got, ref, what)
    bad += check_integers(got, ref, what, pairs_slack)
    if bad:
        bad.sort(key=lambda t: -t[0])
        raise AssertionError(f"{len(bad)} values beyond their bound; the worst: " + "; then ".join(b[1] for b in bad[:4]))
    return w


def boundary_share(ref):
    return pbo.boundary_share(ref)


# ---- the non-finite scene -----------------------------------------------------------------------------------------------------
# (parameter, column, value, stays visible in the oracle)
POISONS = (("scale_raw", 0, np.nan, False), ("scale_raw", 0, np.inf, False), ("scale_raw", 1, -np.inf, True), ("q_raw", 0, np.nan, False),
           ("q_raw", 0, np.inf, False), ("pos", 0, np.nan, False), ("pos", 1, np.inf, False), ("pos", 2, -np.inf, False),
           ("opacity_raw", 0, np.nan, False), ("opacity_raw", 0, np.inf, True))
POISONS_UNFUSED = (("sigma", 0, np.nan, False), ("sigma", 4, np.inf, False), ("pos", 0, np.nan, False), ("opacity_raw", 0, np.nan, False))


def nonfinite(unfused=False):
    """(poisoned, twin, rows, stays): synthetic(200) with one ordinary visible row per entry of POISONS (POISONS_UNFUSED) given that
    value, and the twin with opacity_raw = -30 instead on the rows that must be culled; each as (scene, color, sigma)."""
    def fresh():
        s = pbo.synthetic(200)
        color, sigma = unfused_inputs(s) if unfused else (None, None)
        return s, color, sigma
    bad, twin = fresh(), fresh()
    s = bad[0]
    cand = [i for i in range(129, 200) if not s["culled"][i] and i % 5 and i % 11 not in (4, 9)]
    poisons = POISONS_UNFUSED if unfused else POISONS
    rows = cand[:len(poisons)]
    assert len(rows) == len(poisons)
    for i, (k, c, v, stays) in zip(rows, poisons):
        for which, (sc, color, sigma) in enumerate((bad, twin)):
            arr = dict(sc, color=color, sigma=sigma)[k].reshape(200, -1)
            if which == 0 or stays:
                arr[i, c] = v
            else:
                sc["opacity_raw"][i] = -30.0
    return bad, twin, np.array(rows), np.array([p[3] for p in poisons])
