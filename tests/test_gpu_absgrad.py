"""The absolute-gradient densification statistic on the device: raster_backward_kernel<DET, AUX, ABS> through the two
_abs raster entries against the existing entries (columns 0-9) and tests/absgrad_oracle.py (columns 10-11), densify_stats_kernel<ABS>
against float64 on the device's own records, ops.densify_stats(rec, absgrad=True) behind every backward route, the statistic end to
end against oracle/torch_port.py pixel by pixel, a frame whose signed statistic cancels, and Trainer(densify_absgrad=True).

Bound of columns 10-11, per Gaussian: |delta| <= (K_moments + 8) 2^-24 scale + allowance.  K_moments = 3 x the largest ratio of the raster
oracle's own float32 evaluation, as tests/test_gpu_raster.py derives it; 8 = the roundings of the linear term formed from the pre-scaled
conic (two products, one sum, the rescale, the product with a: each half an ulp of the absolute terms, counted twice as K_B is); scale and
allowance: tests/absgrad_oracle.py.  Each check prints the device's largest ratio (pytest -s)."""
import ctypes as C
import functools
import importlib
import types

import numpy as np
import pytest
import torch

from oracle import scenes
from oracle import torch_port as tp
from tests import absgrad_oracle as ao
from tests import device_frame as dfm
from tests import list_scenes
from tests import raster_oracle as ro

pytestmark = pytest.mark.gpu
PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
abi = dfm.abi
DEV = dfm.DEV
NAMES = list_scenes.NAMES
BG = (1.0, 0.5, 0.25)
MODES = ("atomic", "deterministic", "aux atomic", "aux deterministic")
SCENES = ("stacked", "stacked65", "stacked_5x13", "clamps", "huge", "g1_generic", "g3_occlusion")
K_LINEAR = 8.0
SENTINEL = -123.0
_RUNS = {}


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _abs_backward(fr, g_img, g_depth=None, g_alpha=None, aux=False, det=False, bg=None):
    """gsplat_rasterize_backward[_aux]_abs behind fr.forward(accum=True, aux=aux), on a grad2d full of 0xFF bytes and (det) a scratch
    of exactly the size the library asks for, each followed by a canary.  Returns grad2d [n,16]."""
    assert fr.fwd_aux == aux and "accum" in fr.bufs
    dev = {k: torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV) for k, a in (("gi", g_img), ("gd", g_depth), ("ga", g_alpha)) if a is not None}
    g2d = fr._buf("grad2d", fr.n * 64)
    nbytes = (fr.lib.gsplat_rasterize_backward_aux_abs_scratch_bytes if aux else fr.lib.gsplat_rasterize_backward_abs_scratch_bytes)(fr.n, fr.capacity)
    scratch = fr._buf("det_scratch", nbytes) if det else None
    acc = _vp(fr.bufs["accum"][0])
    if not aux:
        abi.check(fr.lib.gsplat_rasterize_backward_abs(fr.n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), acc, _vp(dev["gi"]), g2d, 0,
                                                       scratch, nbytes if det else 0, fr.st), "gsplat_rasterize_backward_abs")
    else:
        bgp = None if bg is None else (C.c_float * 3)(*bg)
        abi.check(fr.lib.gsplat_rasterize_backward_aux_abs(fr.n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), acc,
                                                           _vp(fr.bufs["accum_aux"][0]), _vp(dev["gi"]), _vp(dev["gd"]), _vp(dev["ga"]), bgp, g2d, 0,
                                                           scratch, nbytes if det else 0, fr.st), "gsplat_rasterize_backward_aux_abs")
    torch.cuda.synchronize()
    return fr._floats("grad2d", (fr.n, 16))


class _Run:
    """Everything of one scene, computed once: the device's state, grad2d of the existing and of the _abs entries in the four modes
    (the deterministic _abs ones twice), the raster oracle with its K and the absolute-gradient oracle (plain / aux)."""

    def __init__(self, name):
        s = self.s = list_scenes.raster_scene(name)
        unfused = (s["color"], s["sigma"]) if "color" in s else None
        fr = self.fr = dfm.Frame(s, unfused=unfused)
        counts = fr.project(0 if unfused else dfm.F)
        assert counts.n_binned > 0
        fr.bin(counts.n_binned)
        up = list_scenes.upstream(s)
        self.plain, self.abs, self.abs2, self.intact = {}, {}, {}, []
        for aux in (False, True):
            kw = dict(aux=aux, bg=BG if aux else None)
            fr.forward(accum=True, **kw)
            for det in (False, True):
                mode = ("aux " if aux else "") + ("deterministic" if det else "atomic")
                bk = dict(g_img=up[0], g_depth=up[1] if aux else None, g_alpha=up[2] if aux else None, det=det, **kw)
                self.plain[mode] = fr.backward(**bk)
                self.abs[mode] = _abs_backward(fr, **bk)
                self.intact.append(fr.canaries_intact())
                if det:
                    self.abs2[mode] = _abs_backward(fr, **bk)
                    self.intact.append(fr.canaries_intact())
        a = self.arr = fr.arrays()
        th = list_scenes.thresholds(s, as_float32=True)
        self.args = (a["rec"], a["ranges"], a["sorted_ids"], a["lists_x"], s["H"], s["W"]) + th
        self.ref, self.K, self.ab = {}, {}, {}
        for aux in (False, True):
            kw = dict(g_img=up[0], g_depth=up[1], g_alpha=up[2], bg=BG, aux=True) if aux else dict(g_img=up[0])
            self.ref[aux] = ro.composite(*self.args, **kw)
            cal = ro.ratios(ro.composite_f32(*self.args, **kw), self.ref[aux])
            self.K[aux] = {k: 3.0 * cal.get(k, 0.0) for k in ro.KINDS}
            kw.pop("aux", None)
            self.ab[aux] = ao.absgrad(self.ref[aux], a["rec"], chi=th[0], alpha_max=th[1], alpha_cutoff=th[2], **kw)


def _run(name):
    """(A failed set-up is kept and raised again: nothing runs on the device a second time.)"""
    if name not in _RUNS:
        try:
            _RUNS[name] = _Run(name)
        except Exception as e:
            _RUNS[name] = e
    if isinstance(_RUNS[name], Exception):
        raise _RUNS[name]
    return _RUNS[name]


def _abs_ratio(g, ab, K):
    """Columns 10-11 of grad2d g against the oracle ab: (largest (|delta| - allowance)+ / (2^-24 scale), the indices beyond the bound)."""
    d = np.abs(g[:, 10:12].astype(np.float64) - ab.S)
    over = np.maximum(d - ab.allow, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(over > 0, over / (ro.EPS * ab.scale), 0.0)
    return float(ratio.max(initial=0.0)), np.argwhere(d > (K + K_LINEAR) * ro.EPS * ab.scale + ab.allow), d


# ---- 1. the ABS kernel computes the plain gradients -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_abs_entries_give_the_plain_gradients(name, mode):
    run = _run(name)
    aux = mode.startswith("aux")
    ns = 10 if aux else 9
    g, plain = run.abs[mode], run.plain[mode]
    assert np.isfinite(g).all()
    assert not g[:, 12:].any() and (aux or not g[:, 9].any()), "columns 12-15 (and 9 without aux) are exact zeros"
    if "deterministic" in mode:
        diff = np.argwhere(g[:, :ns].view(np.uint32) != plain[:, :ns].view(np.uint32))
        assert not len(diff), f"{name} {mode}: {len(diff)} values of columns 0-{ns - 1} differ from the existing entry, first at {diff[0]}"
    else:
        low = g.copy()
        low[:, 10:12] = 0.0
        r = ro.check(dict(grad2d=low), run.ref[aux], run.K[aux], f"{name} _abs backward {mode}", pair_mask=run.arr["pair_mask"])
        print(f"{name} _abs backward {mode}: columns 0-{ns - 1}, device |delta| / (2^-24 scale) {r}; K {run.K[aux]}")


# ---- 2. columns 10-11 against the oracle -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_absolute_sums_against_the_oracle(name, mode):
    run = _run(name)
    aux = mode.startswith("aux")
    ab, K = run.ab[aux], run.K[aux]["moments"]
    g = run.abs[mode]
    assert (g[:, 10:12] >= 0).all()
    assert not g[~ab.in_list].any(), "the row of a Gaussian in no list must keep zeros"
    assert (ab.S > 0).any()
    ratio, bad, d = _abs_ratio(g, ab, K)
    print(f"{name} {mode}: columns 10-11, device |delta| / (2^-24 scale) {ratio:.1f} (allowed K_moments {K:.1f} + {K_LINEAR:.0f}); "
          f"{int((ab.S[:, 0] > 0).sum())} Gaussians, {int((ab.allow > 0).any(1).sum())} with an allowance")
    assert not len(bad), (f"{name} {mode}: Gaussian {bad[0][0]}, column {10 + bad[0][1]}: {g[bad[0][0], 10 + bad[0][1]]!r}, oracle {ab.S[tuple(bad[0])]!r}, "
                          f"|delta| {d[tuple(bad[0])]:.3e}, scale {ab.scale[tuple(bad[0])]:.3e}, allowance {ab.allow[tuple(bad[0])]:.3e}; {len(bad)} beyond the bound")
    if "deterministic" in mode:
        assert np.array_equal(g.view(np.uint32), run.abs2[mode].view(np.uint32)), "deterministic mode: two runs differ"


@pytest.mark.parametrize("name", SCENES)
def test_canaries(name):
    run = _run(name)
    assert len(run.intact) == 6 and all(run.intact)


# ---- 3. the statistics kernel --------------------------------------------------------------------------------------------------------

def _cut(name, n):
    s = list_scenes.golden(name)
    for k in NAMES:
        s[k] = np.ascontiguousarray(s[k][:n])
    return s


def _behind_camera():
    s = list_scenes.golden("g1_generic")
    eye = s["c2w"][:3, 3]
    s["pos"] = s["pos"].copy()
    s["pos"][::3] = 2 * eye - s["pos"][::3]
    return s


KERNEL_SCENES = {
    "g1_generic": lambda: list_scenes.golden("g1_generic"),
    "g6_huge": lambda: list_scenes.golden("g6_huge"),                   # the extent cap is reached
    "g1_cut_300": lambda: _cut("g1_generic", 300),                       # the last block of 256 is ragged
    "behind_camera": _behind_camera,
}


def _sentinel_record(n, seed, tail=64):
    rng = np.random.default_rng(seed)
    rec = np.full((n + tail, 4), SENTINEL, np.float32)
    rec[:n, 0] = rng.uniform(0, 1e-3, n)
    rec[:n, 1] = rng.integers(0, 4, n)
    rec[:n, 2] = rng.uniform(0, 300, n)
    rec[:n, 3] = 7.0
    return rec


@pytest.mark.parametrize("name", list(KERNEL_SCENES))
def test_abs_stats_kernel_against_the_device_records(name):
    s = KERNEL_SCENES[name]()
    fr = dfm.Frame(s)
    c = fr.project(dfm.F | dfm.L | dfm.J)
    fr.bin(max(int(c.n_binned), 1))
    fr.rasterize()
    gi = torch.tensor(np.random.default_rng(1).normal(0, 1, (s["H"], s["W"], 3)).astype(np.float32), device=DEV)
    g2d = torch.empty(fr.n, 16, device=DEV)
    abi.check(fr.lib.gsplat_rasterize_backward_abs(fr.n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), _vp(fr.accum), _vp(gi),
                                                   _vp(g2d), 0, None, 0, fr.st), "gsplat_rasterize_backward_abs")
    torch.cuda.synchronize()
    n, H, W = fr.n, s["H"], s["W"]
    a = fr.arrays(lists=False)
    rec, g = a["rec"].astype(np.float64), g2d.cpu().numpy().astype(np.float64)
    vis = a["tiles"] != 0
    assert vis.any() and (name != "behind_camera" or not vis[::3].any())
    before = _sentinel_record(n, 3)
    dev, plain = torch.tensor(before, device=DEV), torch.tensor(before, device=DEV)
    calls = 2
    for _ in range(calls):
        abi.check(fr.lib.gsplat_densify_stats_abs(n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(g2d), _vp(dev), fr.st), "gsplat_densify_stats_abs")
        abi.check(fr.lib.gsplat_densify_stats(n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(g2d), _vp(plain), fr.st), "gsplat_densify_stats")
    torch.cuda.synchronize()
    got, pl = dev.cpu().numpy(), plain.cpu().numpy()
    assert got[n:].tobytes() == before[n:].tobytes(), "canary rows behind the record were written"
    assert got[:n][~vis].tobytes() == before[:n][~vis].tobytes(), "the row of a Gaussian that is not visible was touched"
    assert got[:, 1:].tobytes() == pl[:, 1:].tobytes(), "count, extent_max and column 3 must be what the plain kernel writes"
    assert np.array_equal(got[:n, 1], before[:n, 1] + calls * vis)
    per_call = ao.magnitude(g[:, 10:12], rec[:, 5], H, W)
    want = before[:n, 0].astype(np.float64) + calls * per_call * vis
    tol = calls * 1e-5 * per_call + calls * 2.0 ** -24 * np.abs(want)           # 1e-5 relative per call + the two float32 additions into the sum
    err = np.abs(got[:n, 0] - want)
    worst = int(np.argmax(np.where(vis, err / np.maximum(tol, 1e-300), 0.0)))
    print(f"{name}: {int(vis.sum())} of {n} visible, non-zero statistic {(per_call[vis] > 0).sum()}, worst row {worst}: err {err[worst]:.3e} tol {tol[worst]:.3e}")
    assert (per_call[vis] > 0).any() and (err <= tol)[vis].all(), (worst, err[worst], tol[worst])
    signed = (pl[:n, 0] - before[:n, 0]).astype(np.float64)
    assert ((got[:n, 0] - before[:n, 0]) >= signed * (1 - 1e-5) - calls * 2.0 ** -23 * np.abs(want))[vis].all(), "the absolute statistic is below the signed one"
    if a["counts"].n_binned > 1:              # a frame whose pairs outgrew the capacity it is called with adds nothing
        keep = dev.clone()
        abi.check(fr.lib.gsplat_densify_stats_abs(n, int(a["counts"].n_binned) - 1, C.byref(fr.view), _vp(fr.state), _vp(g2d), _vp(dev), fr.st),
                  "gsplat_densify_stats_abs")
        torch.cuda.synchronize()
        assert torch.equal(dev, keep)


# ---- 4. routes -----------------------------------------------------------------------------------------------------------------------

def _second_camera(c2w):
    c = np.array(c2w, np.float32).copy()
    c[:3, 3] += c[:3, :3] @ np.array([0.05, -0.03, 0.02], np.float32)
    return c


def _upstream01(s, seed):
    return np.random.default_rng(seed).uniform(0, 1, (int(s["H"]), int(s["W"]), 3)).astype(np.float32)


def _views(s):
    return [(np.asarray(s["c2w"], np.float32), _upstream01(s, 0)), (_second_camera(s["c2w"]), _upstream01(s, 1))]


def _params(s):
    return {k: torch.tensor(s[k], device=DEV, requires_grad=True) for k in NAMES}


def _go(gs, p, s, c2w, w, **extra):
    c = c2w if isinstance(c2w, torch.Tensor) else torch.tensor(c2w, device=DEV)
    out = gs.render_gaussians(*[p[k] for k in NAMES], c, *list_scenes.cam_args(s), **s["kwargs"], **extra)
    img = out[0] if isinstance(out, tuple) else out
    (img * torch.tensor(w, device=DEV)).sum().backward()


ROUTES = ("waited", "deferred", "accumulate", "fused_rest", "aux", "pose")


def _route(gs, s, route, absgrad):
    """One pass through `route` inside ops.densify_stats(rec, absgrad=absgrad).  Returns ({name: gradient or stepped parameter}, record)."""
    ops = gs.ops
    views = _views(s)
    p = _params(s)
    rec = gs.DensifyStats(len(s["pos"]), DEV)
    kw = dict(absgrad=True) if absgrad else {}
    out = {}
    before = dict(ops.absgrad_calls)
    if route in ("waited", "aux", "pose"):
        c2w, w = views[0]
        cam = torch.tensor(c2w, device=DEV, requires_grad=(route == "pose"))
        with gs.densify_stats(rec, **kw):
            _go(gs, p, s, cam, w, **(dict(aux=True, background=BG) if route == "aux" else {}))
        if route == "pose":
            out["c2w"] = cam.grad.clone()
        n_frames, kind = 1, "separate"
    else:
        with torch.no_grad():                                            # a pair capacity for this size: the frames below do not wait
            for c2w, _ in views:
                gs.render_gaussians(*[p[k] for k in NAMES], torch.tensor(c2w, device=DEV), *list_scenes.cam_args(s), **s["kwargs"])
        calls = ops.composite_calls["backward"]
        if route == "deferred":
            with gs.deferred_checks() as chk, gs.densify_stats(rec, **kw):
                _go(gs, p, s, *views[0])
            n_frames = 1
        elif route == "accumulate":
            with gs.deferred_checks() as chk, ops.accumulate_grads(p) as acc, gs.densify_stats(rec, **kw):
                for c2w, w in views:
                    _go(gs, p, s, c2w, w)
                acc.assign()
            assert acc.count == 2
            n_frames = 2
        else:
            optim = importlib.import_module(PKG + ".optim")
            opt = optim.GaussianAdam(optim.reference_param_groups(types.SimpleNamespace(**p)), lr=0.01, eps=1e-15)
            with gs.deferred_checks() as chk, opt.fused_rest_update(p["f_rest"]) as hook, gs.densify_stats(rec, **kw):
                _go(gs, p, s, *views[0])
            assert hook.applied
            out["f_rest stepped"] = p["f_rest"].detach().clone()
            n_frames = 1
        chk.verify()
        assert ops.composite_calls["backward"] == calls + n_frames
        kind = "arena"
    torch.cuda.synchronize()
    after = ops.absgrad_calls
    assert after[kind] - before[kind] == (n_frames if absgrad else 0) and sum(after.values()) - sum(before.values()) == (n_frames if absgrad else 0)
    for k in NAMES:
        if p[k].grad is not None:
            out[k] = p[k].grad.clone()
    return out, rec.data.clone()


@functools.lru_cache(maxsize=None)
def _waited_views(name):
    """grad_sum of each of the two views alone, waited, absolute mode, deterministic."""
    gs = importlib.import_module(PKG)
    s = list_scenes.golden(name)
    out = []
    for c2w, w in _views(s):
        rec = gs.DensifyStats(len(s["pos"]), DEV)
        with gs.densify_stats(rec, absgrad=True):
            _go(gs, _params(s), s, c2w, w)
        torch.cuda.synchronize()
        out.append(rec.data.clone())
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["g1_generic", "g7_tiny"])
def test_absgrad_behind_every_backward_route(gs, name, route):
    s = list_scenes.golden(name)
    old = gs.set_deterministic(True)
    try:
        ga, ra = _route(gs, s, route, True)
        gp, rp = _route(gs, s, route, False)
        waited = _waited_views(name)
        if route == "waited":
            assert torch.equal(ra, waited[0]), "deterministic mode: two waited runs differ"
    finally:
        gs.set_deterministic(old)
    assert set(ga) == set(gp) and len(ga) >= 5
    for k in ga:
        assert torch.equal(ga[k], gp[k]), f"{route}: {k} differs between a frame with and without absgrad"
    assert ra[:, 0].any() and torch.equal(ra[:, 1:], rp[:, 1:]), "count, extent_max and column 3 are the signed record's"
    assert (ra[:, 0] >= rp[:, 0] * (1 - 1e-5)).all(), "an absolute statistic below the signed one"
    print(f"{name} {route}: sum of grad_sum absolute {float(ra[:, 0].sum()):.4e}, signed {float(rp[:, 0].sum()):.4e}")
    if route != "aux":                   # (over a background the frame is another frame: G_A = -sum_c G_c bg_c joins the gradient)
        want = waited[0][:, 0].double() + (waited[1][:, 0].double() if route == "accumulate" else 0.0)
        err = (ra[:, 0].double() - want).abs()
        assert (err <= 1e-5 * want).all(), f"{route}: grad_sum differs from the waited route's by {float((err / want.clamp(min=1e-30)).max()):.2e} relative"


# ---- 5. end to end against the oracle, pixel by pixel -----------------------------------------------------------------------------

def _pixelwise(s, w, dtype):
    """sum over the pixels p of |d(sum_c w_pc image_pc) / du|, the same for v, as the NDC magnitude per input row, from
    oracle/torch_port.py evaluated in dtype; float64 numpy [N].  The oracle renders with `stages` (tests/densify_stats_oracle.py).  One
    autograd pass per pixel through its graph takes 25 ms (75 s for the 3072 pixels of g7_tiny, and a batched autograd.grad is no
    faster: cumprod's backward has no batching rule), so the per-tile compositing (torch_port.render, F14) is evaluated once more on
    the oracle's own stages with ONE LEAF per (pair, pixel) for u and v: a single backward pass then holds every pixel's gradient
    separately.  That second evaluation is held to the oracle: its image must be the oracle's, and its per-pixel gradients must add
    up to the oracle's own dL/du, dL/dv."""
    torch.set_num_threads(16)
    p = {k: torch.tensor(np.asarray(s[k])).to(dtype).requires_grad_(True) for k in NAMES}
    cam = torch.tensor(np.asarray(s["c2w"])).to(dtype)
    H, W = int(s["H"]), int(s["W"])
    kw = s["kwargs"]
    T, chi, amax, cut = int(kw.get("T", 16)), kw.get("chi_square_clip", 6.25), kw.get("alpha_max", 0.99), kw.get("alpha_cutoff", 1 / 128.)
    st = {}
    sigma = tp.covariance_from_params(p["scale_raw"], p["q_raw"])
    color = tp.sh_colour(p["f_dc"], p["f_rest"], p["pos"], cam)
    img = tp.render(p["pos"], color, p["opacity_raw"], sigma, cam, H, W, s["fx"], s["fy"], s["cx"], s["cy"], stages=st, **kw)
    wt = torch.as_tensor(np.asarray(w)).to(dtype)
    st["u"].retain_grad()
    st["v"].retain_grad()
    (img * wt).sum().backward()
    V = len(st["ids"])
    u, v, conic, record, col = (st[k].detach() for k in ("u", "v", "conic", "opacity_record", "color"))
    tiles_x = (W + T - 1) // T
    su, sv, tu, tv = (torch.zeros(V, dtype=torch.float64) for _ in range(4))
    again = torch.zeros(H, W, 3, dtype=dtype)
    for t, s0, s1 in zip(st["tile_ids"].tolist(), st["tile_start"].tolist(), st["tile_end"].tolist()):
        gx, gy = (t % tiles_x) * T, (t // tiles_x) * T
        w_t, h_t = min(gx + T, W) - gx, min(gy + T, H) - gy
        if w_t <= 0 or h_t <= 0:
            continue
        px = torch.arange(gx, gx + w_t, dtype=dtype).repeat(h_t)
        py = torch.arange(gy, gy + h_t, dtype=dtype).repeat_interleave(w_t)
        g = st["pair_gauss"][s0:s1]
        U = u[g].unsqueeze(1).expand(-1, len(px)).clone().requires_grad_(True)            # one leaf per (pair, pixel)
        Vv = v[g].unsqueeze(1).expand(-1, len(px)).clone().requires_grad_(True)
        du, dv = px.unsqueeze(0) - U, py.unsqueeze(0) - Vv
        q = conic[g, 0].unsqueeze(1) * du * du + 2 * conic[g, 1].unsqueeze(1) * du * dv + conic[g, 2].unsqueeze(1) * dv * dv
        fall = torch.exp(-0.5 * q.clamp(max=chi))
        fall = torch.where(q <= chi, fall, torch.zeros_like(fall))
        alpha = (record[g].unsqueeze(1) * fall).clamp_max(amax)
        alpha = torch.where(alpha >= cut, alpha, torch.zeros_like(alpha))
        trans = torch.cumprod(1 - alpha, 0)
        trans = torch.cat([torch.ones_like(trans[:1]), trans[:-1]], 0)
        wgt = alpha * trans * (trans > 5e-5).to(dtype)
        pix = (wgt.unsqueeze(-1) * col[g].unsqueeze(1)).sum(0).clamp(0, 1)
        iy, ix = py.long(), px.long()
        again[iy, ix] = pix.detach()
        (pix * wt[iy, ix]).sum().backward()
        su.index_add_(0, g, U.grad.double().abs().sum(1))
        sv.index_add_(0, g, Vv.grad.double().abs().sum(1))
        tu.index_add_(0, g, U.grad.double().sum(1))
        tv.index_add_(0, g, Vv.grad.double().sum(1))
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert float((again - img.detach()).abs().max()) <= tol, "the second evaluation of the compositing is not the oracle's image"
    for mine, theirs in ((tu, st["u"].grad), (tv, st["v"].grad)):
        theirs = theirs.double()
        assert float((mine - theirs).abs().max()) <= tol * max(float(theirs.abs().max()), 1e-30) * (1 if dtype == torch.float64 else 10), "per-pixel gradients do not add up to the oracle's"
    g = np.zeros(len(s["pos"]))
    g[st["ids"].numpy()] = np.sqrt((su.numpy() * W / 2) ** 2 + (sv.numpy() * H / 2) ** 2)
    return g


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _e2e_oracles():
    out = {}
    for name in ("g7_tiny", "stacked"):
        s = list_scenes.raster_scene(name)
        w = _upstream01(s, 0)
        out[name] = (s, w, _pixelwise(s, w, torch.float64), _pixelwise(s, w, torch.float32))
    return out


@pytest.mark.parametrize("name", ["g7_tiny", "stacked"])
def test_statistic_end_to_end_against_the_oracle(gs, name):
    orc = _e2e_oracles()
    cal = {k: _rel_l2(v[3], v[2]) for k, v in orc.items()}
    bound = 3.0 * max(cal.values())
    s, w, g64, g32 = orc[name]
    rec = gs.DensifyStats(len(s["pos"]), DEV)
    with gs.densify_stats(rec, absgrad=True):
        _go(gs, _params(s), s, s["c2w"], w)
    torch.cuda.synchronize()
    got = rec.data[:, 0].double().cpu().numpy()
    e = _rel_l2(got, g64)
    print(f"{name}: grad_sum (absolute) against the float64 oracle pixel by pixel: rel-L2 {e:.2e}; the oracle in float32 {cal[name]:.2e} "
          f"(both scenes: {cal}); allowed {bound:.2e}")
    assert np.isfinite(got).all() and g64.any()
    assert e <= bound


# ---- 6. the cancellation frame -------------------------------------------------------------------------------------------------------

def test_cancellation_frame_on_the_device():
    s, gi = ao.cancellation_scene()
    fr = dfm.Frame(s)
    c = fr.project(dfm.F)
    assert c.n_binned == 1
    fr.bin(c.n_binned)
    fr.forward(accum=True)
    g = _abs_backward(fr, gi, det=True)
    assert fr.canaries_intact()
    a = fr.arrays()
    assert a["rec"][0, 0] == 8.0 and a["rec"][0, 1] == 4.0, "the projected centre must be pixel (8, 4) exactly"
    th = list_scenes.thresholds(s, as_float32=True)
    args = (a["rec"], a["ranges"], a["sorted_ids"], a["lists_x"], s["H"], s["W"]) + th
    ref = ro.composite(*args, g_img=gi)
    K = 3.0 * ro.ratios(ro.composite_f32(*args, g_img=gi), ref).get("moments", 0.0)
    ab = ao.absgrad(ref, a["rec"], g_img=gi, chi=th[0], alpha_max=th[1], alpha_cutoff=th[2])
    assert (ab.S > 0).all() and (np.abs(ab.signed) < 1e-12 * ab.S).all()
    ratio, bad, d = _abs_ratio(g, ab, K)
    print(f"cancellation frame: columns 10-11 {g[0, 10:12]}, oracle {ab.S[0]}, |delta| / (2^-24 scale) {ratio:.1f} (allowed {K:.1f} + {K_LINEAR:.0f})")
    assert not len(bad), (g[0, 10:12], ab.S[0], d)
    recs = {}
    g2d = torch.tensor(g, device=DEV)
    for name in ("gsplat_densify_stats", "gsplat_densify_stats_abs"):
        recs[name] = torch.zeros(1, 4, device=DEV)
        abi.check(getattr(fr.lib, name)(1, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(g2d), _vp(recs[name]), fr.st), name)
    torch.cuda.synchronize()
    signed, absolute = float(recs["gsplat_densify_stats"][0, 0]), float(recs["gsplat_densify_stats_abs"][0, 0])
    want = float(ao.magnitude(ab.S, a["rec"][:, 5].astype(np.float64), s["H"], s["W"])[0])
    print(f"cancellation frame: signed statistic {signed:.3e}, absolute {absolute:.6e} (oracle {want:.6e})")
    assert absolute > 0 and signed < 1e-4 * absolute
    assert abs(absolute - want) <= 1e-5 * want + ao.magnitude((K + K_LINEAR) * ro.EPS * ab.scale + ab.allow, a["rec"][:, 5].astype(np.float64), s["H"], s["W"])[0]


# ---- 7. Trainer ----------------------------------------------------------------------------------------------------------------------

TNAMES = ("pos", "opacity_raw", "f_dc", "f_rest", "scale_raw", "q_raw")


def _train_scene():
    """The scene of tests/test_gpu_densify_stats.py: three views, the third 16 pixels wider (a pair capacity of its own)."""
    s = scenes.case_g1()
    rng = np.random.default_rng(5)
    cams = [s["c2w"], scenes._camera(rng), scenes._camera(rng)]
    views = []
    for k, c in enumerate(cams):
        W = s["W"] + (16 if k == 2 else 0)
        views.append(dict(image=rng.uniform(0, 1, (s["H"], W, 3)).astype(np.float32), c2w=c, H=s["H"], W=W, fx=s["fx"], fy=s["fy"],
                          cx=s["cx"], cy=s["cy"]))
    return s, views


def _trainer(s, **cfg):
    model_mod = importlib.import_module(PKG + ".model")
    training = importlib.import_module(PKG + ".training")
    model = model_mod.GaussianModel({k: torch.tensor(s[k]) for k in TNAMES}, device=DEV)
    cfg = dict(dict(densify_rule="screen", densification_interval=10 ** 6, opacity_reset_interval=10 ** 9), **cfg)
    return training.Trainer(model, training.TrainConfig(**cfg))


def _merged_by_hand(gs, s, views, **kw):
    """One pass record per view, made with ops.densify_stats(..., **kw) on the initial parameters, merged in view order."""
    losses = importlib.import_module(PKG + ".losses")
    p = {k: torch.tensor(s[k], device=DEV, requires_grad=True) for k in TNAMES}
    total = gs.DensifyStats(len(s["pos"]), DEV)
    for v in views:
        rec = gs.DensifyStats(len(s["pos"]), DEV)
        with gs.densify_stats(rec, **kw):
            img = gs.render_gaussians(p["pos"], p["f_dc"], p["f_rest"], p["opacity_raw"], p["scale_raw"], p["q_raw"],
                                      torch.tensor(v["c2w"], dtype=torch.float32, device=DEV), v["H"], v["W"], v["fx"], v["fy"], v["cx"], v["cy"])
            loss, _ = losses.compute_loss_device(img, torch.tensor(v["image"], device=DEV), 0.8, 0.2, scale=1.0 / len(views))
            loss.backward()
        total.merge_(rec)
    torch.cuda.synchronize()
    return total.data.clone()


def test_trainer_accumulates_the_absolute_statistics_of_its_views(gs):
    ops = gs.ops
    s, views = _train_scene()
    old = gs.set_deterministic(True)
    try:
        ref = _merged_by_hand(gs, s, views, absgrad=True)
        signed = _merged_by_hand(gs, s, views)
        assert (ref[:, 1] == 3).any() and ref[:, 0].any() and torch.equal(ref[:, 1:], signed[:, 1:]) and not torch.equal(ref[:, 0], signed[:, 0])
        got = {}
        for streams in (1, 2):
            tr = _trainer(s, view_streams=streams, densify_absgrad=True)
            before = sum(ops.absgrad_calls.values())
            out = tr.step(1, views)
            torch.cuda.synchronize()
            assert not out["densified"] and sum(ops.absgrad_calls.values()) == before + len(views)
            got[streams] = tr.densify_stats.data.clone()
        assert torch.equal(got[1], ref), "one step: the merge, in view order, of the three views' absolute statistics, bit for bit"
        assert torch.equal(got[2], got[1]), "view_streams = 2 differs from view_streams = 1"
        # the default configuration queues no _abs call, and its column 0 is the signed run's
        tr = _trainer(s)
        before = sum(ops.absgrad_calls.values())
        tr.step(1, views)
        torch.cuda.synchronize()
        assert sum(ops.absgrad_calls.values()) == before
        assert torch.equal(tr.densify_stats.data, signed)
    finally:
        gs.set_deterministic(old)
