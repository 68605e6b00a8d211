"""Float64 reference of K8 (project_backward_kernel) for any of its modes, Gaussian by Gaussian (helper, not a test).

Built on the stages of oracle/torch_port.py (any SH degree, low-pass and antialiasing).  The rows of grad2d -- columns 0..8 the moments and
colour sums of the raster backward, column 9 dL/dz -- become cotangents of the oracle's per-Gaussian stage
(u, v, conic, opacity_record, colour, z) by the relation documented at project_backward_core (csrc/gs_body.h); then autograd runs,
ONE PASS PER STAGE COLUMN.  Gaussians are independent, so the pass of column j hands every parameter entry its own term
d out_j / d theta_ik * ct_j: their sum is the gradient, the sum of their absolute values is the entry's `scale` -- what the entry
is the result of adding up, and so what one float32 rounding of it is proportional to.  For c2w the terms are summed over the
Gaussians as well (the Jacobian columns come from a second backward pass per entry of c2w).

check() holds every entry of every row to

    |got - ref| <= K[tensor, kind] * 2^-24 * scale_row + floor,

scale_row the largest scale of the row within the tensor, floor = 2^-24 * 2^-24 * the tensor's largest scale.  Rows are sorted into
kinds from float64 quantities alone (kinds()); K comes from the same evaluation in float32 (calibrate()): 3 x (util.K_CAL) the
largest ratio of the float32 oracle in that (tensor, kind) of the same scene and mode, never above util.GRAD_TOL_MAX / 2^-24.
"""
import numpy as np
import torch

from oracle import torch_port as tp
from tests import list_scenes, util

EPS = 2.0 ** -24
K_CAP = util.GRAD_TOL_MAX / EPS
FUSED = ("pos", "opacity_raw", "scale_raw", "q_raw", "f_dc", "f_rest")
UNFUSED = ("pos", "opacity_raw", "color", "sigma")
COLUMNS = ("u", "v", "A11", "A12", "A22", "opacity", "r", "g", "b", "z")
NEAR = 1e-3               # a row within this (relative) of a threshold is a `boundary` row
ISO = 1e-2                # a free row whose three scales differ by less (relative) is `free iso`
SIZES = (1, 63, 64, 65, 129, 200)
GOLDENS = ("g1_generic", "g6_huge", "g7_tiny")
FILTERS = {"off": (0.0, False), "lowpass": (0.3, False), "antialias": (0.3, True)}


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def _c2w():
    """A camera that is not the identity, so that the pose terms are all alive."""
    a, b = 0.3, -0.2
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = [0.4, -0.3, 0.2]
    return m


def _subpixel(z, f, jitter):
    """scale_raw of a splat 0.023 px wide at depth z (jitter: three log-scale offsets, halved): its 2-D variances are 5e-4 px^2, and
    under the 0.3 px^2 low-pass rho^2 = det Sigma / det(Sigma + s I) = 3e-6 -- the middle of a decade, so that the sub-pixel rows of
    a scene share one kind."""
    return np.log(0.023 * z / f) + 0.5 * np.asarray(jitter)


def synthetic(n, more_culls=False):
    """n Gaussians on a view of 32 x 48 pixels, with the edge rows of tests/test_gpu_pieces.py _sigma_inputs mixed in (every 3rd row
    below 64 rows, every 5th above): clamped scales, |q_raw| around 1e-6, 1e-4 and 1e-2, q_raw = 0, near-isotropic, sub-pixel (and
    every 11th ordinary row as well: _subpixel), huge (an eigenvalue beyond 1e4), saturated opacity -- and culled Gaussians (behind the camera, opacity below the cut, off screen):
    every 7th row of an ordinary block; n = 129: block 1 is invisible as a whole; n = 200: block 0 has lane 0 alone visible and
    block 1 lane 63 alone.  The last block of every size but 64 is partial.
    more_culls (the forward tests): the culled rows take ten reasons in turn instead of three -- also inside the near plane, beyond the
    far plane, beyond each of the four guard-band sides, and (s["offscreen"]) a SURVIVOR: inside the guard band with its AABB outside
    the image, counted in n_survivors and not in n_visible.  The rows that are culled and every other row stay what they are."""
    H, W, f = 32, 48, 40.0
    rng = np.random.default_rng(100 + n)
    z = rng.uniform(3, 6, n)
    uv = np.stack([rng.uniform(3, W - 3, n), rng.uniform(3, H - 3, n)], 1)
    sr = rng.normal(-2.0, 0.4, (n, 3))
    qr = rng.normal(0, 1, (n, 4))
    op = rng.uniform(-2.0, 2.0, n)
    unit = qr / np.linalg.norm(qr, axis=1, keepdims=True)
    step = 3 if n < 64 else 5
    for i in range(0, n, step):
        j = (i // step) % 13
        if j == 0:
            sr[i] = [-15.0, -16.5, -14.0] if n > 1 else sr[i]                  # all three below log 1e-6
        elif j == 1:
            sr[i] = [-15.0, -2.0, -2.3] if (i // step) % 2 else [np.log(1e-6) + 0.4, -2.2, -1.9]     # below the clamp / just above it
        elif j == 2:
            qr[i] = unit[i] * 1e-6
        elif j == 3:
            qr[i] = 0.0
        elif j == 4:
            qr[i] = unit[i] * 0.99e-4
        elif j == 5:
            qr[i] = unit[i] * 1.01e-4
        elif j == 6:
            qr[i] = unit[i] * 0.99e-2                                          # either side of the branch to the torque form
        elif j == 7:
            qr[i] = unit[i] * 1.01e-2
        elif j == 8:
            sr[i] = sr[i, 0] + rng.normal(0, 1e-3, 3)                          # nearly isotropic
        elif j == 9:
            sr[i] = _subpixel(z[i], f, rng.normal(-6.0, 0.2, 3) + 6.0)
        elif j == 10:
            sr[i] = [3.0, 1.0, 0.5]                                            # huge: an eigenvalue beyond 1e4 px^2
        elif j == 11:
            op[i] = 30.0                                                       # sigmoid beyond the 0.999 clamp (and not within 1e-3 of it)
        else:
            sr[i] = [-9.0, -2.0, -2.5]                                         # a needle
    # more sub-pixel rows, on ordinary rows (every 11th from row 4 that is no edge row, a generator of their own, so the other rows
    # are what they were): a kind of one row would be calibrated by a single draw of the float32 oracle's rounding
    sub = np.random.default_rng(7000 + n)
    for i in range(4, n, 11):
        if i % step:
            sr[i] = _subpixel(z[i], f, sub.normal(0, 0.2, 3))
    for i in range(9, n, 11):                                                  # and more nearly isotropic ones, likewise
        if i % step:
            sr[i] = sr[i, 0] + sub.normal(0, 1e-3, 3)
    culled = np.zeros(n, bool)
    culled[6::7] = True
    if n == 129:
        culled[64:128] = True
    if n == 200:
        culled[:128] = True
        culled[0] = culled[127] = False
        sr[0], sr[127], qr[0], qr[127], op[0], op[127] = [-2.0, -2.3, -1.8], [-2.2, -1.9, -2.4], unit[0], unit[127], 0.5, -0.5
    x = (uv[:, 0] - W / 2) / f * z
    y = (uv[:, 1] - H / 2) / f * z
    offscreen = np.zeros(n, bool)
    for k, i in enumerate(np.nonzero(culled)[0]):
        r = k % 10 if more_culls else k % 3
        if r == 0:
            z[i] = -z[i]                                                       # behind the camera
        elif r == 1:
            op[i] = -10.0                                                      # below the opacity cut
        elif r == 2:
            x[i] = (W + 200.0 - W / 2) / f * z[i]                              # beyond the guard band
        elif r == 3:
            x[i] = (W + 20.0 - W / 2) / f * z[i]                               # inside the guard band, its AABB (radius 1 px) off the image
            sr[i] = np.log(0.2 * z[i] / f)
            offscreen[i] = True
        elif r in (4, 5):
            z[i] = 0.005 if r == 4 else 150.0                                  # inside the near plane (0.01) / beyond the far plane (100)
            x[i], y[i] = (uv[i, 0] - W / 2) / f * z[i], (uv[i, 1] - H / 2) / f * z[i]
        elif r == 6:
            x[i] = (-40.0 - W / 2) / f * z[i]                                  # beyond the guard band (32 px) on the left,
        elif r == 7:
            y[i] = (-40.0 - H / 2) / f * z[i]                                  # at the top,
        elif r == 8:
            y[i] = (H + 40.0 - H / 2) / f * z[i]                               # at the bottom,
        else:
            x[i] = (W + 40.0 - W / 2) / f * z[i]                               # and just beyond it on the right
    c2w = _c2w()
    pos = np.stack([x, y, z], 1) @ c2w[:3, :3].T + c2w[:3, 3]
    d = dict(pos=pos, scale_raw=sr, q_raw=qr, opacity_raw=op, f_dc=0.5 * rng.normal(0, 1, (n, 3)), f_rest=0.2 * rng.normal(0, 1, (n, 45)))
    s = list_scenes._pack(d, H, W, f, f * 1.1, W / 2.0 + 0.5, H / 2.0 - 0.25, c2w=c2w)
    s["culled"] = culled
    s["offscreen"] = offscreen
    return s


def assert_block_layout(name, tiles):
    """The blocks of 64 the synthetic scenes are built for, in the tiles[n] of a projection: n = 129, block 1 invisible as a whole
    and the one row of block 2 visible; n = 200, lane 0 alone visible in block 0 and lane 63 alone in block 1."""
    vis = np.asarray(tiles) != 0
    if name == "synth129":
        assert vis[:64].any() and not vis[64:128].any() and vis[128], name
    if name == "synth200":
        assert vis[0] and not vis[1:64].any() and vis[127] and not vis[64:127].any() and vis[128:192].any() and vis[192:].any(), name


def scene(name):
    """(scene, color, sigma): `synthN`, a fused golden, or g11_unfused (its color_in / sigma_in; else None, None)."""
    if name.startswith("synth"):
        return synthetic(int(name[5:])), None, None
    s = list_scenes.golden(name)
    if name == "g11_unfused":
        d = util.load(name)
        return s, np.ascontiguousarray(d["color_in"], np.float32), np.ascontiguousarray(d["sigma_in"], np.float32)
    return s, None, None


# ---- the stage -------------------------------------------------------------------------------------------------------------

class Stage:
    """The oracle's per-Gaussian stage of scene s in `dtype`, with the parameters (and c2w) as leaves: names, leaves{}, c2w, st
    (the oracle's stages), ids, out [V,10] (COLUMNS), lam0 [V,2] (unfiltered, unclamped eigenvalues), s (the low-pass)."""

    def __init__(self, s, degree=3, lowpass=0.0, antialias=False, color=None, sigma=None, dtype=torch.float64):
        self.fused = color is None
        self.n = len(s["pos"])
        self.s, self.degree, self.antialias = s, degree, antialias
        self.lowpass = tp.lowpass_value(lowpass)
        kw = s["kwargs"]
        t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
        self.c2w = t(s["c2w"])
        st = {}
        mode = dict(lowpass=lowpass, antialias=antialias, stages=st, stop_after_binning=True)
        if self.fused:
            self.names = FUSED
            self.leaves = {k: t(s[k]) for k in FUSED}
            p = self.leaves
            early = tp.render_fused(p["pos"], p["f_dc"], p["f_rest"], p["opacity_raw"], p["scale_raw"], p["q_raw"], self.c2w,
                                    *list_scenes.cam_args(s), sh_degree=degree, **mode, **kw)
        else:
            assert degree == 3
            self.names = UNFUSED
            self.leaves = dict(pos=t(s["pos"]), opacity_raw=t(s["opacity_raw"]), color=t(color), sigma=t(sigma))
            p = self.leaves
            early = tp.render(p["pos"], p["color"], p["opacity_raw"], p["sigma"], self.c2w, *list_scenes.cam_args(s), **mode, **kw)
        self.st = st
        if early is not None or "ids" not in st:                 # no survivor
            self.ids = np.zeros(0, np.int64)
            self.out = torch.zeros((0, 10), dtype=dtype)
            self.lam0 = np.zeros((0, 2))
            return
        self.ids = st["ids"].numpy()
        self.out = torch.cat([st["u"].unsqueeze(1), st["v"].unsqueeze(1), st["conic"], st["opacity_record"].unsqueeze(1), st["color"],
                              st["z"].unsqueeze(1)], 1)
        self.lam0 = st["evals_unfiltered"].detach().double().numpy()

    def jacobian_c2w(self):
        """{(r, c): d out / d c2w[r, c] as [V,10]}, computed once: (J^T v) is linear in v, so the gradient of its entry (r, c) w.r.t. v
        is that column of J."""
        if not hasattr(self, "_jac"):
            self._jac = {}
            v = torch.zeros_like(self.out, requires_grad=True)
            jt = torch.autograd.grad(self.out, self.c2w, v, create_graph=True)[0]
            for r in range(3):
                for c in range(4):
                    col = torch.autograd.grad(jt[r, c], v, retain_graph=True, allow_unused=True)[0]
                    if col is not None:
                        self._jac[(r, c)] = col.detach()
        return self._jac

    def cotangents(self, g2d, moments=True):
        """[V,10] in the stage's dtype: the rows of grad2d (float32 values) as cotangents of COLUMNS.  moments = False: columns 0..4
        are the 2-D gradients themselves."""
        dt = self.out.dtype
        m = torch.tensor(np.asarray(g2d)[self.ids, :10].astype(np.float64)).to(dt)
        if not moments:
            return m
        o, c = self.st["opacity_record"].detach(), self.st["conic"].detach()
        a11, a12, a22 = c[:, 0], c[:, 1], c[:, 2]
        return torch.stack([o * (a11 * m[:, 0] + a12 * m[:, 1]), o * (a12 * m[:, 0] + a22 * m[:, 1]), -0.5 * o * m[:, 2], -o * m[:, 3],
                            -0.5 * o * m[:, 4], m[:, 5], m[:, 6], m[:, 7], m[:, 8], m[:, 9]], 1)


def kinds(stage):
    """One label per Gaussian [n] from float64 quantities: `culled` (not a survivor of the oracle's stage), `boundary` (a quantity
    within NEAR of its threshold), `eigen-clamped`, `conic-floor`, `scale-clamped`, `saturated`, else `free c<d>` with d the decade
    of the 2-D condition number of the covariance that is clamped (Sigma + s I under the filter; c4 = 1e4 and beyond) and, under
    a low-pass, ` r<d>` the decade of rho^2 (r-8 = 1e-8 and below); `free iso` where the three scales are within ISO of each other: there
    the gradient of the rotation is a difference of nearly equal terms that the float32 oracle loses, and the kind's K with it, which
    the other free rows must not inherit."""
    assert stage.out.dtype == torch.float64
    s, st = stage.s, stage.st
    out = np.full(stage.n, "culled", dtype=object)
    if not len(stage.ids):
        return out
    ids = stage.ids
    lam = stage.lam0 + stage.lowpass
    near = lambda x, t: np.abs(np.asarray(x, np.float64) / t - 1.0) < NEAR
    cov = st["cov2d"].detach().numpy()
    a, b, d = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    det = np.maximum(a * d - b * b, 1e-12)
    k11, k22 = d / det, a / det
    mc = s["kwargs"].get("min_conis", 1e-6)
    sig = 1.0 / (1.0 + np.exp(-s["opacity_raw"][ids].astype(np.float64)))
    bnd = near(lam[:, 0], 1e-6) | near(lam[:, 1], 1e-6) | near(lam[:, 0], 1e4) | near(lam[:, 1], 1e4) | near(k11, mc) | near(k22, mc) | near(sig, 0.999)
    bnd |= near(stage.lam0[:, 0] * stage.lam0[:, 1], 1e-30)
    eig = (lam[:, 0] < 1e-6) | (lam[:, 1] > 1e4)
    floor = (k11 < mc) | (k22 < mc)
    sat = sig > 0.999
    small = np.zeros(len(ids), bool)
    if stage.fused:
        sc = np.exp(s["scale_raw"][ids].astype(np.float64))
        small = (sc < 1e-6).any(1)
        bnd |= near(sc, 1e-6).any(1) | near(np.linalg.norm(s["q_raw"][ids].astype(np.float64), axis=1), 1e-2)
    cond = np.clip(np.floor(np.log10(lam[:, 1] / np.maximum(lam[:, 0], 1e-300))), 0, 4).astype(int)
    gap = np.full(len(ids), np.inf)                                      # (un-fused: no scales, no such kind)
    if stage.fused:
        gap = sc.max(1) / np.maximum(sc.min(1), 1e-300) - 1.0
        bnd |= near(gap, ISO)
    # rho^2 = det Sigma / det(Sigma + s I), whether or not the opacity is scaled by rho: under the low-pass alone the float32 oracle
    # loses a sub-pixel splat's own eigenvalues just the same, and its rows must not calibrate the ordinary ones
    rho2 = stage.lam0.prod(1) / np.maximum(lam.prod(1), 1e-300)
    rho2 = np.clip(np.floor(np.log10(np.maximum(rho2, 1e-300))), -8, 0).astype(int)
    for k, i in enumerate(ids):
        if bnd[k]:
            out[i] = "boundary"
        elif eig[k]:
            out[i] = "eigen-clamped"
        elif floor[k]:
            out[i] = "conic-floor"
        elif small[k]:
            out[i] = "scale-clamped"
        elif sat[k]:
            out[i] = "saturated"
        else:
            out[i] = ("free iso" if gap[k] < ISO else f"free c{cond[k]}") + (f" r{rho2[k]}" if stage.lowpass > 0 else "")
    return out


def moment_rows(stage, tiles, seed=0):
    """Seeded grad2d [n,16] (float32): moment rows (Mx, My, Mxx, Mxy, Myy, M0, r, g, b) and dL/dz for the Gaussians that both the
    oracle and `tiles` (the device's, or the host build's) see, every term at a similar magnitude; every 9th of them an all-zero row
    (`zero`, bool [n])."""
    rng = np.random.default_rng(seed)
    ids = stage.ids
    g2d = np.zeros((stage.n, 16), np.float32)
    zero = np.zeros(stage.n, bool)
    if len(ids):
        rows = rng.normal(0, 1, (len(ids), 10))
        conic = stage.st["conic"].detach().double().numpy()
        rows[:, :5] /= np.abs(conic).max(1, keepdims=True) + 1.0
        rows[np.asarray(tiles)[ids] == 0] = 0
        if len(ids) > 9:
            rows[4::9] = 0
            zero[ids[4::9]] = True
        g2d[ids, :10] = rows.astype(np.float32)
    return g2d, zero


# ---- the reference ---------------------------------------------------------------------------------------------------------

class Reference:
    """terms[name][j] = the gradient of `name` through stage column j alone ([10, n, ...]; c2w [10, 4, 4]); abs_c2w [10, 4, 4] the sum
    over the Gaussians of the absolute terms (float64 with scale=True only); kind [n]; ids; rho [n] (1 where not visible)."""

    def grad(self, depth=False):
        """Gradients by name (the parameters' and c2w's), float64; depth: with column 9."""
        j = 10 if depth else 9
        return {k: v[:j].sum(0) for k, v in self.terms.items()}

    def scale(self, depth=False):
        j = 10 if depth else 9
        out = {k: np.abs(v[:j]).sum(0) for k, v in self.terms.items()}
        out["c2w"] = self.abs_c2w[:j].sum(0)
        return out


def reference(s, g2d, degree=3, lowpass=0.0, antialias=False, color=None, sigma=None, dtype=torch.float64, scale=True, stage=None,
              moments=True):
    """The per-column gradients of the rows g2d (moments = False: columns 0..4 hold the 2-D gradients, not moment sums; stage: a
    Stage of the same scene and mode to evaluate on, instead of a new one).  dtype = torch.float32 (scale = False): the same evaluation in the reference's own
    arithmetic -- the calibration."""
    stg = stage if stage is not None else Stage(s, degree, lowpass, antialias, color, sigma, dtype)
    ref = Reference()
    ref.names, ref.ids, ref.n, ref.fused, ref.degree = stg.names, stg.ids, stg.n, stg.fused, degree
    shapes = {k: tuple(v.shape) for k, v in stg.leaves.items()}
    ref.terms = {k: np.zeros((10,) + shapes[k]) for k in stg.names}
    ref.terms["c2w"] = np.zeros((10, 4, 4))
    ref.abs_c2w = np.zeros((10, 4, 4))
    ref.rho = np.ones(stg.n)
    ref.kind = kinds(stg) if dtype == torch.float64 else None
    if not len(stg.ids):
        return ref
    ref.rho[stg.ids] = stg.st["rho"].detach().double().numpy()
    ct = stg.cotangents(g2d, moments)
    leaves = [stg.leaves[k] for k in stg.names] + [stg.c2w]
    for j in range(10):
        gr = torch.autograd.grad(stg.out[:, j], leaves, ct[:, j], retain_graph=True, allow_unused=True)
        for k, g in zip(stg.names + ("c2w",), gr):
            if g is not None:
                ref.terms[k][j] = g.double().numpy()
    if scale:
        assert dtype == torch.float64
        for (r, c), col in stg.jacobian_c2w().items():
            t = (col * ct).detach().numpy()
            ref.abs_c2w[:, r, c] = np.abs(t).sum(0)
            assert np.allclose(t.sum(0), ref.terms["c2w"][:, r, c], rtol=1e-9, atol=1e-12 * (np.abs(t).sum() + 1e-300))
    if not stg.fused:       # the projection sees sym(Sigma) only
        ref.terms["sigma"] = 0.5 * (ref.terms["sigma"] + ref.terms["sigma"].transpose(0, 1, 3, 2))
    return ref


# ---- the checker -----------------------------------------------------------------------------------------------------------

def _rows(a, n):
    return np.asarray(a, np.float64).reshape(n, -1)


def ratios(got, ref, depth=False, names=None):
    """{tensor: (ratio [n] -- the largest of the row, inf for a non-finite entry --, worst column [n])} of got against ref.grad(depth):
    (|got - ref| - floor)+ / (2^-24 scale_row); a row whose scale is an exact zero has ratio 0 within the floor and inf beyond.
    c2w is one row."""
    want, sc = ref.grad(depth), ref.scale(depth)
    out = {}
    for k in (names if names is not None else got.keys()):
        n = 1 if k == "c2w" else ref.n
        g, w, s = _rows(got[k], n), _rows(want[k], n), _rows(sc[k], n)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if k == "sigma":
            g = 0.5 * (g + g.reshape(n, 3, 3).transpose(0, 2, 1).reshape(n, 9))
        srow = s.max(1, keepdims=True)
        floor = EPS * EPS * (s.max() if s.size else 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            excess = np.maximum(np.abs(g - w) - floor, 0.0)
            r = np.where(excess == 0.0, 0.0, excess / (EPS * srow))
        r[~np.isfinite(g)] = np.inf
        out[k] = (r.max(1), r.argmax(1))
    return out


def worst(rat, ref, known=None):
    """{(tensor, kind): the largest ratio} over the rows that are compared with the kind's K (no boundary rows, no KNOWN_ROWS)."""
    out = {}
    for k, (r, _) in rat.items():
        kind = np.array(["all"], dtype=object) if k == "c2w" else ref.kind.copy()
        for (kk, i) in (known or {}):
            if kk == k:
                kind[i] = "boundary"
        for kd in set(kind.tolist()):
            if kd != "boundary":
                out[(k, kd)] = float(r[kind == kd].max())
    return out


def calibrate(ref, ref32):
    """K[tensor, kind] = min(K_CAL x the float32 oracle's largest ratio in that (tensor, kind), GRAD_TOL_MAX / 2^-24); the ratio is
    the larger of the gradient's with and without the depth column (the scale differs)."""
    out = {}
    for depth in (False, True):
        for key, r in worst(ratios(ref32.grad(depth), ref, depth), ref).items():
            out[key] = max(out.get(key, 0.0), min(util.K_CAL * r, K_CAP))
    return out


CAL_SEEDS = tuple(range(12))


def calibration(s, tiles, st64, st32, rows=(), seeds=CAL_SEEDS, **mode):
    """K of a scene and mode: the float32 oracle against the float64 one on the seeded moment rows of CAL_SEEDS (and on `rows`, pairs
    (g2d, moments) of the caller's own) -- the largest ratio over all of them, so that a kind of one or two Gaussians is not calibrated
    by a single draw of their cotangents."""
    Ks = []
    for g2d, moments in [(moment_rows(st64, tiles, seed)[0], True) for seed in seeds] + list(rows):
        r64 = reference(s, g2d, stage=st64, moments=moments, **mode)
        r32 = reference(s, g2d, stage=st32, moments=moments, dtype=torch.float32, scale=False, **mode)
        Ks.append(calibrate(r64, r32))
    return merge_K(Ks)


def merge_K(Ks):
    """The largest K per (tensor, kind) over several calibrations: what a kind with no calibration rows in a scene takes."""
    out = {}
    for K in Ks:
        for key, v in K.items():
            out[key] = max(out.get(key, 0.0), v)
    return out


# Rows whose arithmetic no float32 evaluation of the kernel's form resolves, each with its cause and its own K (at most five):
# {(scene, filter): {(tensor, Gaussian): K}}
KNOWN_ROWS = {
    # a disc seen edge-on (2-D eigenvalues 9.7e-6 and 1.43 px^2, rho = 5e-3): the compensation's d det0 = d da + a dd - 2 b db is formed
    # from the rounded (a, b, d), where det0 is 1 / 1.5e5 of a d -- float32 keeps eps * l1 / l0 of the term.  K = K_CAL * l1 / l0.
    ("g7_tiny", "antialias"): {("scale_raw", 69): 3.0 * 1.43279297 / 9.65882536e-06},
}


def check(got, ref, K, what, depth=False, names=None, other=None, known=None):
    """Every entry of every compared row within K[tensor, kind] * 2^-24 * scale_row + floor; the failure names the tensor, the
    Gaussian, its kind and its lane.  other: K of the other scenes of the run, for a (tensor, kind) this scene's K lacks.  known:
    {(tensor, Gaussian): K} of the scene and filter from KNOWN_ROWS.  Returns the largest ratio per (tensor, kind)."""
    rat = ratios(got, ref, depth, names)
    bad = []
    for k, (r, col) in rat.items():
        for i in range(len(r)):
            kd = "all" if k == "c2w" else ref.kind[i]
            if kd == "boundary":
                continue
            bound = K.get((k, kd), (other or {}).get((k, kd), 0.0))
            bound = max(bound, (known or {}).get((k, i), 0.0))
            if not r[i] <= bound:
                bad.append((r[i] / max(bound, 1e-300), f"{what}: {k}[{i}] (kind {kd}, lane {i % 64}, column {col[i]}): "
                            f"{_rows(got[k], len(r))[i, col[i]]!r} against {_rows(ref.grad(depth)[k], len(r))[i, col[i]]!r}, "
                            f"ratio {r[i]:.3g} > K = {bound:.3g}"))
    if "f_rest" in rat and ref.degree < 3:      # (below the floor, but structural: the degree's inactive columns are exact zeros)
        cols = tp.inactive_columns(ref.degree)
        g = _rows(got["f_rest"], ref.n)
        for i in np.nonzero((g[:, cols] != 0).any(1))[0]:
            bad.append((np.inf, f"{what}: f_rest[{i}] (kind {ref.kind[i]}, lane {i % 64}): an inactive column of degree {ref.degree} holds "
                        f"{g[i, cols][g[i, cols] != 0][0]!r}, not an exact zero"))
    if bad:
        bad.sort(key=lambda t: -t[0])
        raise AssertionError(f"{len(bad)} rows beyond their bound; the worst: " + "; then ".join(b[1] for b in bad[:4]))
    return worst(rat, ref, known)


def boundary_share(ref):
    """The share of the visible rows that are boundary rows (not compared)."""
    vis = ref.kind != "culled"
    return float((ref.kind == "boundary").sum()) / max(int(vis.sum()), 1)


def acc_K(ref, prior, K, depth=False):
    """K for GSPLAT_BACKWARD_ACCUMULATE, checked as (result - prior) against the reference: the sum prior + gradient is rounded once
    more, by half an ulp of the sum <= 2^-24 (|prior| + |gradient|) per entry -- in units of 2^-24 * scale_row that is at most
    (|prior|_row + scale_row) / scale_row, added to the K of the row's kind (the largest over the kind's rows; a row of scale 0 is not
    touched by the accumulation)."""
    sc = ref.scale(depth)
    out = dict(K)
    for k, p in prior.items():
        srow = sc[k].reshape(ref.n, -1).max(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            extra = np.where(srow > 0, (np.abs(np.asarray(p, np.float64).reshape(ref.n, -1)).max(1) + srow) / srow, 0.0)
        for kd in set(ref.kind.tolist()):
            out[(k, kd)] = K.get((k, kd), 0.0) + float(extra[ref.kind == kd].max())
    return out
