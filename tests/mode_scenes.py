"""Seeded random scenes and the table of render modes they are swept through (tests/test_mode_scenes_cpu.py, tests/test_gpu_mode_scenes.py,
tests/debug_seed.py, tests/stress_random_scenes.py), and the one copy of what the oracle-parity tests share: the scene builder of
test_gpu_parity.test_random_scenes_vs_oracle, the loss over (image, depth, alpha), and the checks of maps, gradient sets and the
pose gradient (tests/test_gpu_aux.py, tests/test_gpu_pose_grad.py).  Nothing here needs a GPU; render_hip() is handed the package.

Every bound is tests/util.py's.  The float64 oracle (oracle/torch_port.py) is the reference, its float32 run the calibration."""
import collections
import functools
import itertools

import numpy as np
import torch

from oracle import scenes
from oracle import torch_port as tp
from tests import util

F32, F64 = torch.float32, torch.float64
NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
UNFUSED = ("pos", "color", "opacity_raw", "sigma")
BG = (1.0, 0.5, 0.25)


# ---- the scene builder -------------------------------------------------------------------------------------------------------------

def random_scene(seed, rng_base, h_max, w_max, n_max):
    """Randomised image size, camera, anisotropy and opacity: {six float32 parameter tensors, `c2w`, `cam` = (H, W, fx, fy, cx, cy), H, W,
    and the loss weights w_img [H, W, 3], w_depth [H, W] (uniform / 8), w_alpha [H, W] (uniform in [-1, 1]), float32 numpy}.  The draws
    come in a fixed order from default_rng(rng_base + seed), the weights last: tests/golden/random_scene_digests.json pins the arrays
    of four seeds of test_random_scenes_vs_oracle (rng_base 1000, sizes below 150 x 200, fewer than 1800 Gaussians)."""
    rng = np.random.default_rng(rng_base + seed)
    H, W = int(rng.integers(9, h_max)), int(rng.integers(9, w_max))
    n = int(rng.integers(1, n_max))
    f = float(rng.uniform(40, 160))
    cam = (H, W, f, f * float(rng.uniform(0.9, 1.1)), W / 2 + float(rng.uniform(-5, 5)), H / 2 + float(rng.uniform(-5, 5)))
    c2w = torch.tensor(scenes._camera(rng, tilt=0.3))
    s = scenes._base(rng, n, H, W, cam[2], cam[3], cam[4], cam[5], mu_s=float(rng.uniform(-3.2, -1.2)), sd_s=float(rng.uniform(0.2, 1.0)),
                     op_mu=float(rng.uniform(-2, 3)), op_sd=1.5, spread=1.3, c2w=c2w.numpy())
    t = {k: torch.tensor(s[k]) for k in util.PARAMS}
    # drop near depth ties (fp32 cannot order them; the reference's argsort is unstable there)
    zc = tp.to_camera(t["pos"].double(), c2w.double())[2]
    zs, order = torch.sort(zc)
    keep = torch.ones(n, dtype=torch.bool)
    keep[order[1:][(zs[1:] - zs[:-1]) < 2e-5]] = False
    d = {k: v[keep].contiguous() for k, v in t.items()}
    d.update(seed=seed, cam=cam, H=H, W=W, c2w=c2w)
    d["w_img"] = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    d["w_depth"] = (rng.uniform(0, 1, (H, W)) / 8).astype(np.float32)
    d["w_alpha"] = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    return d


def parity_scene(seed):
    """The scene of test_gpu_parity.test_random_scenes_vs_oracle for `seed`."""
    return random_scene(seed, 1000, 150, 200, 1800)


@functools.lru_cache(maxsize=None)
def mode_scene(seed):
    """The scene of the mode sweep: the smallest sizes that still give several 16 x 8 lists per row, ragged edges and more than one
    chunk per list.  Shared and never written to."""
    return random_scene(seed, 5000, 80, 112, 700)


def scene_arrays(d):
    """name -> numpy array of everything the builder drew (what the digests cover)."""
    out = {k: d[k].numpy() for k in util.PARAMS}
    out.update(cam=np.array(d["cam"], dtype=np.float64), c2w=d["c2w"].numpy(), w_img=d["w_img"])
    return out


# ---- the loss and the checks (shared with test_gpu_aux.py and test_gpu_pose_grad.py) -------------------------------------------------

def loss(out, d, dtype, device, which="all"):
    """L = sum image * w_img + sum depth * w_depth + sum alpha * w_alpha, or one of the three terms.  `out` = (image, depth, alpha)."""
    terms = dict(image=(out[0], "w_img"), depth=(out[1], "w_depth"), alpha=(out[2], "w_alpha"))
    use = terms if which == "all" else {which: terms[which]}
    return sum((t * torch.as_tensor(np.asarray(d[w]), dtype=dtype, device=device)).sum() for t, w in use.values())


def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def check_maps(out, ref, cal, what):
    """(image, depth, alpha) against the float64 frame `ref`, calibrated by the float32 frame `cal`: image and alpha as they are,
    depth after dividing both sides by max|depth| of the float64 frame (one chi-square flip is then worth what it is worth in the image)."""
    assert all(t.dtype == F32 for t in out[:3] if isinstance(t, torch.Tensor))       # (a device frame: float32 outputs)
    img, depth, alpha = (_np(t) for t in out[:3])
    assert depth.shape == alpha.shape == img.shape[:2]
    util.check_image(img, ref[0], cal=None if cal is None else cal[0], what=f"{what} image")
    util.check_image(alpha, ref[2], cal=None if cal is None else cal[2], what=f"{what} alpha")
    scale = max(float(np.abs(ref[1]).max()), 1e-30)
    util.check_image(depth / scale, ref[1] / scale, cal=None if cal is None else cal[1] / scale, what=f"{what} depth / max")


def check_pose(g, ref, what, cal=None, band=None):
    """dL/dc2w [4, 4]: the 3 x 3 rotation block on its own (the translation column is the larger), then the whole."""
    g, ref = _np(g), _np(ref)
    util.check_grad(g[:3, :3], ref[:3, :3], f"{what} c2w[:3,:3]", cal=None if cal is None else cal[:3, :3], band=None if band is None else band[:3, :3])
    util.check_grad(g, ref, f"{what} c2w", cal=cal, band=band)


def check_grads(grads, ref, cal, what, names=NAMES + ("c2w",), band=None):
    """The gradients `names` of `grads` against ref[k], calibrated by cal[k] (None: the bounds as they stand); a tensor whose
    float64 gradient is all zero must be exactly zero (util.check_grad)."""
    for k in names:
        b = None if band is None else band[k]
        if k == "c2w":
            check_pose(grads[k], ref[k], what, cal=None if cal is None else cal[k], band=b)
        else:
            util.check_grad(_np(grads[k]), ref[k], f"{what} {k}", cal=None if cal is None else cal[k], band=b)


def check_case(got, ref, cal, m, what, band=None, grads=True):
    """Everything row `m` asserts of one (image, depth, alpha, gradients) against the float64 one: the image -- with aux the three maps --
    and (`grads`) the row's gradients.  cal: the float32 oracle's, or None for the bounds as they stand."""
    if m.aux:
        check_maps(got, ref, cal, what)
    else:
        util.check_image(got[0], ref[0], cal=None if cal is None else cal[0], what=f"{what} image")
    if grads:
        check_grads(got[3], ref[3], None if cal is None else cal[3], what, names=grad_names(m), band=band)


def case_errors(got, ref, m):
    """{what: (error, detail)} of one result against the float64 one, as check_case measures them: max |delta| and the fraction beyond
    1e-5 of every map (depth / max|depth|), the worst rel-L2 and max/max over the row's gradients."""
    out = {}
    for what, im, r in zip(("image", "depth", "alpha"), got[:3], ref[:3]):
        if im is not None:
            scale = max(float(np.abs(r).max()), 1e-30) if what == "depth" else 1.0
            e = util.image_errors(im / scale, r / scale)
            out[what + " max"], out[what + " frac > 1e-5"] = (e["max"], ""), (e["bad"], "")
    g = {k: util.grad_errors(got[3][k], ref[3][k]) for k in grad_names(m) if np.abs(ref[3][k]).max() > 0}
    for key, name in (("l2", "grad rel-L2"), ("mx", "grad max/max")):
        out[name] = max(((e[key], k) for k, e in g.items()), default=(0.0, ""))
    return out


# ---- the mode table ----------------------------------------------------------------------------------------------------------------

Mode = collections.namedtuple("Mode", "entry sh_degree lowpass antialias aux background pose thresholds route")
FUSED, PLAIN = "render_gaussians", "render"
EAGER, DEFERRED, DETERMINISTIC = "eager", "deferred", "deterministic"
DEFAULT, G12 = "default", "g12"
FILTERS = ((0.0, False), (0.3, False), (0.3, True), (0.1, True))
OUTPUTS = ((False, None), (True, None), (False, BG), (True, BG))
ROUTES = (EAGER, DEFERRED, DETERMINISTIC)
# every value of every axis; a row's place on an axis is axes(row)[axis]
AXES = dict(entry=(FUSED, PLAIN), sh_degree=(0, 1, 2, 3), filter=FILTERS, output=OUTPUTS, pose=(False, True), thresholds=(DEFAULT, G12),
            route=ROUTES)


def axes(m):
    return dict(entry=m.entry, sh_degree=m.sh_degree, filter=(m.lowpass, m.antialias), output=(m.aux, m.background), pose=m.pose,
                thresholds=m.thresholds, route=m.route)


def refused(pair):
    """The pairs of axis values the code refuses by design: render() takes a colour, so it has no SH degree below 3."""
    p = dict(pair)
    return p.get("entry") == PLAIN and p.get("sh_degree", 3) != 3


def _row(entry, degree, filt, output, pose, thresholds, route):
    return Mode(entry, degree, *FILTERS[filt], *OUTPUTS[output], bool(pose), (DEFAULT, G12)[thresholds], ROUTES[route])


# Row 0 is the default call (the mode of test_random_scenes_vs_oracle).  Rows 1-16 are an orthogonal array of strength 2: degree and
# filter index the 4 x 4 square, output = degree + filter, (pose, thresholds) = degree + 2 filter and the route = degree + 3 filter in
# GF(4) (relabelled; the route's fourth label is `deferred` again), and the four rows of degree 3 go through render().  A table that holds
# every (degree, filter) pair has 16 rows at least; this one holds every pair of values of two axes but the refused ones
# (test_mode_scenes_cpu.py computes that).  Rows 6 and 11 -- deferred, the image alone, no pose -- take the composite entries.
#          entry  degree filter output pose thresholds route
MODES = (_row(FUSED, 3, 0, 0, 0, 0, 0),
         _row(FUSED, 0, 0, 0, 1, 0, 0),
         _row(FUSED, 0, 1, 1, 1, 1, 1),
         _row(FUSED, 0, 2, 2, 0, 1, 2),
         _row(FUSED, 0, 3, 3, 0, 0, 1),
         _row(FUSED, 1, 0, 1, 0, 0, 2),
         _row(FUSED, 1, 1, 0, 0, 1, 1),
         _row(FUSED, 1, 2, 3, 1, 1, 0),
         _row(FUSED, 1, 3, 2, 1, 0, 1),
         _row(FUSED, 2, 0, 2, 1, 1, 1),
         _row(FUSED, 2, 1, 3, 1, 0, 2),
         _row(FUSED, 2, 2, 0, 0, 0, 1),
         _row(FUSED, 2, 3, 1, 0, 1, 0),
         _row(PLAIN, 3, 0, 3, 0, 1, 1),
         _row(PLAIN, 3, 1, 2, 0, 0, 0),
         _row(PLAIN, 3, 2, 1, 1, 0, 1),
         _row(PLAIN, 3, 3, 0, 1, 1, 2))
# 24 seeds on which the float32 oracle alone meets the uncalibrated bounds in every row (test_mode_scenes_cpu.py asserts it; of the first
# 26, seeds 12 and 24 do not: 4e-4 and 1e-3 of their image values lie beyond 1e-5 in float32)
SEEDS = tuple(s for s in range(26) if s not in (12, 24))


def uncovered_pairs(modes=MODES):
    """Every pair of values of two different axes that no row holds and the code does not refuse."""
    have = set()
    for m in modes:
        have |= set(itertools.combinations(sorted(axes(m).items(), key=lambda kv: kv[0]), 2))
    want = set()
    for (a, va), (b, vb) in itertools.combinations(sorted(AXES.items()), 2):
        want |= {((a, x), (b, y)) for x in va for y in vb}
    return sorted((p for p in want - have if not refused(p)), key=repr)


def takes_composite_entries(m):
    """A deferred frame goes through gsplat_forward_deferred / gsplat_backward unless it is a pose or an aux frame."""
    return m.route == DEFERRED and not m.pose and not m.aux and m.background is None


@functools.lru_cache(maxsize=None)
def thresholds(name):
    """The positional threshold arguments of a row: none, or the non-default ones of golden g12_kwargs."""
    return dict(util.load("g12_kwargs")["kwargs"]) if name == G12 else {}


def render_kwargs(m):
    """The mode arguments of the device call (ops.render / ops.render_gaussians)."""
    kw = dict(thresholds(m.thresholds), lowpass=m.lowpass, antialias=m.antialias, aux=m.aux)
    if m.background is not None:
        kw["background"] = m.background
    if m.entry == FUSED:
        kw["sh_degree"] = m.sh_degree
    return kw


def neighbours(m):
    """{what: row}: the row with one axis the oracle can see moved one step (degree +-1, lowpass 0.3 <-> 0.1 -- off -> 0.1 --, antialias
    flipped, background <-> none, g12 thresholds <-> default)."""
    out = {}
    if m.entry == FUSED:
        for d in (m.sh_degree - 1, m.sh_degree + 1):
            if 0 <= d <= 3:
                out[f"degree {m.sh_degree}->{d}"] = m._replace(sh_degree=d)
    lp = {0.0: 0.1, 0.1: 0.3, 0.3: 0.1}[m.lowpass]
    out[f"lowpass {m.lowpass}->{lp}"] = m._replace(lowpass=lp)
    if m.lowpass > 0:
        out[f"antialias {m.antialias}->{not m.antialias}"] = m._replace(antialias=not m.antialias)
    out["background " + ("off" if m.background else "on")] = m._replace(background=None if m.background else BG)
    out["thresholds " + (DEFAULT if m.thresholds == G12 else G12)] = m._replace(thresholds=DEFAULT if m.thresholds == G12 else G12)
    return out


# ---- the oracle and the device, in one shape -------------------------------------------------------------------------------------------

def grad_names(m):
    return (NAMES if m.entry == FUSED else UNFUSED) + (("c2w",) if m.pose else ())


def _inputs(d, m, dtype, device, nan_inactive=False):
    """The leaves of a row's call: the six parameters, or -- render() -- the colour and Sigma of the float64 oracle rounded to float32,
    the same values for every dtype and device.  nan_inactive: NaN in the f_rest columns the row's degree ignores."""
    if m.entry == FUSED:
        vals = {k: d[k] for k in NAMES}
        if nan_inactive and m.sh_degree < 3:
            vals["f_rest"] = d["f_rest"].clone()
            vals["f_rest"][:, torch.tensor(tp.inactive_columns(m.sh_degree))] = float("nan")
    else:
        q = {k: d[k].double() for k in NAMES}
        vals = dict(pos=q["pos"], color=tp.sh_colour(q["f_dc"], q["f_rest"], q["pos"], d["c2w"].double()), opacity_raw=q["opacity_raw"],
                    sigma=tp.covariance_from_params(q["scale_raw"], q["q_raw"]))
    p = {k: v.detach().to(F32).to(dtype).to(device).contiguous().requires_grad_(True) for k, v in vals.items()}
    return p, d["c2w"].detach().to(dtype).to(device).requires_grad_(True)


def _result(out, m, p, c):
    out = out if m.aux else (out, None, None)
    grads = {k: (np.zeros(v.shape) if v.grad is None else _np(v.grad)) for k, v in p.items()}
    grads["c2w"] = np.zeros((4, 4)) if c.grad is None else _np(c.grad)
    return tuple(None if t is None else _np(t) for t in out) + (grads,)


def _backward(out, d, m, dtype, device):
    (loss(out, d, dtype, device) if m.aux else loss((out, None, None), d, dtype, device, "image")).backward()


def oracle(d, m, dtype, backward=True, **threshold_overrides):
    """(image, depth, alpha, gradients incl. c2w) of the oracle in `dtype` for row `m` of scene `d`, float64 numpy arrays (the maps None
    without aux; the gradients None with backward=False).  The oracle's c2w is always a leaf.  threshold_overrides: chi_square_clip=, alpha_cutoff= ... in place of the row's."""
    p, c = _inputs(d, m, dtype, "cpu")
    kw = dict(thresholds(m.thresholds), lowpass=m.lowpass, antialias=m.antialias, background=m.background, maps=m.aux)
    kw.update(threshold_overrides)
    if m.entry == FUSED:
        out = tp.render_fused(*[p[k] for k in NAMES], c, *d["cam"], sh_degree=m.sh_degree, **kw)
    else:
        out = tp.render(p["pos"], p["color"], p["opacity_raw"], p["sigma"], c, *d["cam"], **kw)
    if not backward:
        return tuple(None if t is None else _np(t) for t in (out if m.aux else (out, None, None))) + (None,)
    _backward(out, d, m, dtype, "cpu")
    return _result(out, m, p, c)


def _oracle_key(m):
    return m._replace(pose=False, route=EAGER)         # (what the oracle's result depends on)


@functools.lru_cache(maxsize=None)
def _reference(seed, key, dtype, backward=True):
    try:
        return oracle(mode_scene(seed), key, dtype, backward=backward)
    except Exception as e:                              # "all off-screen": kept, and raised again for every row that shares the key
        return e


def reference(seed, m, dtype, backward=True):
    """oracle(mode_scene(seed), m, dtype, backward), computed once for all rows that differ in the pose flag or the route only; shared, never
    written to.  Raises what the oracle raised."""
    r = _reference(seed, _oracle_key(m), dtype, backward)
    if isinstance(r, Exception):
        raise r
    return r


def threshold_band(d, m, rel, what=("chi_square_clip", "alpha_cutoff")):
    """What moving a hard threshold by -+ rel (relative) does to every gradient entry in float64: {name: |hi - lo|}, the bands of the
    thresholds in `what` added."""
    base = dict(chi_square_clip=6.25, alpha_cutoff=1 / 128.)
    base.update({k: v for k, v in thresholds(m.thresholds).items() if k in base})
    band = None
    for k in what:
        lo, hi = (oracle(d, m, F64, **{k: base[k] * (1 + s * rel)})[3] for s in (-1, 1))
        b = {n: np.abs(hi[n] - lo[n]) for n in lo}
        band = b if band is None else {n: band[n] + b[n] for n in b}
    return band


def render_hip(gs, d, m, dev="cuda:0"):
    """The same structure from the device, through the row's entry and route.  The f_rest columns below the row's degree hold
    NaN.  A deferred row renders once without gradients first (the frame that sizes the pair capacity waits) and then inside
    deferred_checks(), repeated by run_deferred if the kept buffers were too small; the off-screen exception comes from its verify()."""
    def frame(grad=True):
        p, c = _inputs(d, m, F32, dev, nan_inactive=True)
        c.requires_grad_(m.pose)
        kw = render_kwargs(m)
        with torch.set_grad_enabled(grad):
            if m.entry == FUSED:
                out = gs.render_gaussians(*[p[k] for k in NAMES], c, *d["cam"], **kw)
            else:
                out = gs.render(p["pos"], p["color"], p["opacity_raw"], p["sigma"], c, *d["cam"], **kw)
        if grad:
            _backward(out, d, m, F32, dev)
        return out, p, c

    if m.route == DETERMINISTIC:
        old = gs.set_deterministic(True)
        try:
            out, p, c = frame()
        finally:
            gs.set_deterministic(old)
    elif m.route == DEFERRED:
        frame(grad=False)
        before = gs.ops.forward_modes["deferred"]
        out, p, c = gs.run_deferred(frame)
        assert gs.ops.forward_modes["deferred"] > before, "the frame was waited for"
    else:
        out, p, c = frame()
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    return _result(out, m, p, c)
