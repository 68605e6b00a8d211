"""Screen-space densification statistics on the device: the two kernels through the C ABI against numpy float64 on
the device's own records, ops.densify_stats behind every backward route against the float64 oracle
(tests/densify_stats_oracle.py), and Trainer(densify_rule="screen")."""
import contextlib
import ctypes as C
import functools
import importlib
import types

import numpy as np
import pytest
import torch

from oracle import scenes
from tests import densify_stats_oracle as dso
from tests import device_frame as dfm
from tests import list_scenes, util

pytestmark = pytest.mark.gpu
PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
abi = dfm.abi
DEV = dfm.DEV
NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
SENTINEL = -123.0            # the canary rows behind a record


def _vp(t):
    return C.c_void_p(t.data_ptr())


# ---- kernel level -------------------------------------------------------------------------------------------------------------

def _behind_camera():
    """g1_generic with every third Gaussian mirrored through the camera centre: camera-space z < 0, culled."""
    s = list_scenes.golden("g1_generic")
    eye = s["c2w"][:3, 3]
    s["pos"] = s["pos"].copy()
    s["pos"][::3] = 2 * eye - s["pos"][::3]
    return s


def _cut(name, n):
    s = list_scenes.golden(name)
    for k in NAMES:
        s[k] = np.ascontiguousarray(s[k][:n])
    return s


KERNEL_SCENES = {
    "g1_generic": lambda: list_scenes.golden("g1_generic"),
    "g6_huge": lambda: list_scenes.golden("g6_huge"),
    "g1_cut_300": lambda: _cut("g1_generic", 300),                       # the last block of 256 is ragged
    "hot_spot": lambda: list_scenes.hot_spot(3000, (32, 48)),            # more than one block, long lists
    "huge_gaussians": list_scenes.huge_gaussians,                        # rectangles of more than 32 lists
    "behind_camera": _behind_camera,
}


def _frame_with_grad2d(s, seed=1):
    """project, bin, rasterise, gsplat_rasterize_backward with a seeded grad_image; returns (frame, grad2d tensor)."""
    fr = dfm.Frame(s)
    c = fr.project(dfm.F | dfm.L | dfm.J)
    fr.bin(max(int(c.n_binned), 1))
    fr.rasterize()
    gi = torch.tensor(np.random.default_rng(seed).normal(0, 1, (s["H"], s["W"], 3)).astype(np.float32), device=DEV)
    g2d = torch.empty(fr.n, 16, device=DEV)
    abi.check(fr.lib.gsplat_rasterize_backward(fr.n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), _vp(fr.accum), _vp(gi),
                                               _vp(g2d), 0, None, 0, fr.st), "gsplat_rasterize_backward")
    torch.cuda.synchronize()
    return fr, g2d


def _sentinel_record(n, seed, tail=64):
    """n rows of plausible earlier statistics (counts 0-3, some extents above the cap, a marker in column 3) followed by canary rows."""
    rng = np.random.default_rng(seed)
    rec = np.full((n + tail, 4), SENTINEL, np.float32)
    rec[:n, 0] = rng.uniform(0, 1e-3, n)
    rec[:n, 1] = rng.integers(0, 4, n)
    rec[:n, 2] = rng.uniform(0, 300, n)
    rec[:n, 3] = 7.0
    return rec


@pytest.mark.parametrize("name", list(KERNEL_SCENES))
def test_stats_kernel_against_the_device_records(name):
    s = KERNEL_SCENES[name]()
    fr, g2d = _frame_with_grad2d(s)
    n, H, W = fr.n, s["H"], s["W"]
    a = fr.arrays(lists=False)
    rec, tiles, g = a["rec"].astype(np.float64), a["tiles"], g2d.cpu().numpy().astype(np.float64)
    vis = tiles != 0
    assert vis.any() and (name != "behind_camera" or not vis[::3].any())
    before = _sentinel_record(n, 3)
    dev = torch.tensor(before, device=DEV)
    calls = 2
    for _ in range(calls):
        abi.check(fr.lib.gsplat_densify_stats(n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(g2d), _vp(dev), fr.st), "gsplat_densify_stats")
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    # rows of Gaussians that are binned nowhere, column 3 and the canary keep their bits
    assert got[n:].tobytes() == before[n:].tobytes(), "canary rows behind the record were written"
    assert got[:n][~vis].tobytes() == before[:n][~vis].tobytes(), "the row of a Gaussian that is not visible was touched"
    assert np.array_equal(got[:n, 3], before[:n, 3])
    # count: exactly k per visible Gaussian
    assert np.array_equal(got[:n, 1], before[:n, 1] + calls * vis)
    # extent_max: bitwise max(before, min(max(ex, ey), 250)) in float32
    ext = np.minimum(np.maximum(a["rec"][:, 6], a["rec"][:, 7]), np.float32(250.0))
    want_ext = np.where(vis, np.maximum(before[:n, 2], ext), before[:n, 2]).astype(np.float32)
    assert got[:n, 2].tobytes() == want_ext.tobytes()
    if name == "g6_huge":
        assert (ext[vis] == 250.0).any()                  # the cap is reached
    # grad_sum: float64 from the copied-back float32 record and moments
    o, a11, a12, a22, mx, my = rec[:, 5], rec[:, 2], rec[:, 3], rec[:, 4], g[:, 0], g[:, 1]
    gu, gv = o * (a11 * mx + a12 * my), o * (a12 * mx + a22 * my)
    per_call = np.sqrt((gu * W / 2) ** 2 + (gv * H / 2) ** 2)
    want = before[:n, 0].astype(np.float64) + calls * per_call * vis
    # about ten float32 roundings against the cancellation-free magnitude per call (room for fused multiply-adds and a fast square
    # root), plus the two float32 additions into the running sum (2^-24 of the sum each)
    tol = calls * 1e-5 * o * (np.abs(a11 * mx) + np.abs(a12 * my) + np.abs(a12 * mx) + np.abs(a22 * my)) * max(W, H) / 2 + calls * 2.0 ** -24 * np.abs(want)
    err = np.abs(got[:n, 0] - want)
    worst = int(np.argmax(np.where(vis, err / np.maximum(tol, 1e-300), 0.0)))
    print(f"{name}: {int(vis.sum())} of {n} visible, non-zero gradient {(per_call[vis] > 0).sum()}, worst row {worst}: err {err[worst]:.3e} tol {tol[worst]:.3e}")
    assert (per_call[vis] > 0).any()
    assert (err <= tol)[vis].all(), (worst, err[worst], tol[worst])
    # a frame whose pairs outgrew the capacity it is called with adds nothing (decided on the device from the frame's counters)
    if a["counts"].n_binned > 1:
        keep = dev.clone()
        abi.check(fr.lib.gsplat_densify_stats(n, int(a["counts"].n_binned) - 1, C.byref(fr.view), _vp(fr.state), _vp(g2d), _vp(dev), fr.st),
                  "gsplat_densify_stats")
        torch.cuda.synchronize()
        assert torch.equal(dev, keep)


def test_merge_kernel_on_hand_made_records():
    lib = abi.lib()
    n, tail = 257, 64
    rng = np.random.default_rng(8)
    p, t = _sentinel_record(n, 11, tail), _sentinel_record(n, 12, tail)
    p[:n, 3] = 0.0
    p[::3, :3] = 0.0                                   # rows the pass did not touch
    p[1, 1], p[1, 0] = 0.0, 0.5                        # count 0 decides, whatever the other columns hold
    t[4] = 0.0
    p[:n, 2] = rng.uniform(0, 250, n) * (p[:n, 1] > 0)
    dp_, dt_ = torch.tensor(p, device=DEV), torch.tensor(t, device=DEV)
    abi.check(lib.gsplat_densify_stats_merge(n, _vp(dp_), _vp(dt_), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gsplat_densify_stats_merge")
    torch.cuda.synchronize()
    gp, gt = dp_.cpu().numpy(), dt_.cpu().numpy()
    used = p[:n, 1] > 0
    assert used.any() and not used.all()
    want = t.copy()
    want[:n, 0] = np.where(used, t[:n, 0] + p[:n, 0], t[:n, 0])          # float32 sums: exact to the bit
    want[:n, 1] = np.where(used, t[:n, 1] + p[:n, 1], t[:n, 1])
    want[:n, 2] = np.where(used, np.maximum(t[:n, 2], p[:n, 2]), t[:n, 2])
    assert gt.tobytes() == want.tobytes()                                # (rows the pass did not touch, column 3 and the canary included)
    wp = p.copy()
    wp[:n][used] = 0.0
    assert gp.tobytes() == wp.tobytes()                                  # exactly the consumed rows are zero; the canary is intact


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _second_camera(c2w):
    c = np.array(c2w, np.float32).copy()
    c[:3, 3] += c[:3, :3] @ np.array([0.05, -0.03, 0.02], np.float32)
    return c


def _views(s):
    return [(np.asarray(s["c2w"], np.float32), dso.upstream(s, 0)), (_second_camera(s["c2w"]), dso.upstream(s, 1))]


@functools.lru_cache(maxsize=None)
def _oracle(name, n_views):
    """Per view: the float64 and the float32 oracle and the device's own tiles (a projection of its own through the C ABI)."""
    s = list_scenes.golden(name)
    out = []
    for c2w, w in _views(s)[:n_views]:
        g64, e64, _ = dso.frame_stats(s, w, torch.float64, c2w)
        g32, e32, _ = dso.frame_stats(s, w, torch.float32, c2w)
        fr = dfm.Frame(dict(s, c2w=c2w))
        fr.project(dfm.F | dfm.L)
        out.append((g64, g32, e64, e32, fr.arrays(lists=False)["tiles"] != 0))
    return out


def _check(name, got, n_views, what):
    per_view = _oracle(name, n_views)
    got = got.detach().cpu().numpy()
    vis = np.stack([v[4] for v in per_view])
    g64, g32 = sum(v[0] for v in per_view), sum(v[1] for v in per_view)
    assert np.array_equal(got[:, 1], vis.sum(0).astype(np.float32)), f"{what}: count differs from the device's own tiles != 0"
    assert not got[:, 3].any()
    util.check_grad(got[:, 0], g64, f"grad_sum ({name}, {what})", cal=g32)
    assert not got[~vis.any(0)].any(), f"{what}: the row of a Gaussian no view binned is not zero"
    if name in ("g1_generic", "g2_ragged"):
        e64 = np.max([np.where(v[4], v[2], 0.0) for v in per_view], 0)
        e32 = np.max([np.where(v[4], v[3], 0.0) for v in per_view], 0)
        # the record's padding (x 1.0001 + 0.01 px) plus K_CAL x the float32 oracle's own deviation -- the largest relative one over the
        # frame, as tests/util.py calibrates every bound by an aggregate of the float32 reference (row by row that deviation is zero
        # by chance for many rows, and no float32 evaluation could meet it there)
        seen = e64 > 0
        cal = float((np.abs(e32 - e64)[seen] / e64[seen]).max())
        slack = e64 * 1e-4 + 0.01 + util.K_CAL * cal * e64
        err = np.abs(got[:, 2] - e64)
        print(f"extent_max ({name}, {what}): max |delta| {err.max():.3e} px, beyond the padding at most {((err - e64 * 1e-4 - 0.01) / np.maximum(e64, 1e-30))[seen].max():.2e} "
              f"relative (allowed {util.K_CAL * cal:.2e}, float32 oracle {cal:.2e})")
        bad = err > slack
        assert not bad.any(), (what, int(bad.sum()), err.max())


def _params(s):
    return {k: torch.tensor(s[k], device=DEV, requires_grad=True) for k in NAMES}


def _go(gs, p, s, c2w, w, **extra):
    c = c2w if isinstance(c2w, torch.Tensor) else torch.tensor(c2w, device=DEV)
    out = gs.render_gaussians(*[p[k] for k in NAMES], c, *list_scenes.cam_args(s), **s["kwargs"], **extra)
    img = out[0] if isinstance(out, tuple) else out
    (img * torch.tensor(w, device=DEV)).sum().backward()


E2E_SCENES = ["g1_generic", "g2_ragged", "g5_guardband", "g6_huge", "g7_tiny"]


@pytest.mark.parametrize("mode", ["waited", "deferred", "accumulate", "fused_rest"])
@pytest.mark.parametrize("name", E2E_SCENES)
def test_stats_behind_every_backward_route(gs, name, mode):
    ops = gs.ops
    s = list_scenes.golden(name)
    views = _views(s)
    rec = gs.DensifyStats(len(s["pos"]), DEV)
    p = _params(s)
    if mode == "waited":
        before = dict(ops.forward_modes)
        with gs.densify_stats(rec):
            _go(gs, p, s, *views[0])
        assert ops.forward_modes["waited"] == before["waited"] + 1
        n_views = 1
    else:
        with torch.no_grad():                                            # a pair capacity for this size: the frames below do not wait
            for c2w, _ in views:
                gs.render_gaussians(*[p[k] for k in NAMES], torch.tensor(c2w, device=DEV), *list_scenes.cam_args(s), **s["kwargs"])
        calls = ops.composite_calls["backward"]
        if mode == "deferred":
            with gs.deferred_checks() as chk, gs.densify_stats(rec):
                _go(gs, p, s, *views[0])
            n_views = 1
        elif mode == "accumulate":
            with gs.deferred_checks() as chk, ops.accumulate_grads(p) as acc, gs.densify_stats(rec):
                for c2w, w in views:
                    _go(gs, p, s, c2w, w)
                acc.assign()
            assert acc.count == 2
            n_views = 2
        else:
            optim = importlib.import_module(PKG + ".optim")
            model = types.SimpleNamespace(**p)
            opt = optim.GaussianAdam(optim.reference_param_groups(model), lr=0.01, eps=1e-15)
            with gs.deferred_checks() as chk, opt.fused_rest_update(p["f_rest"]) as hook, gs.densify_stats(rec):
                _go(gs, p, s, *views[0])
            assert hook.applied
            n_views = 1
        chk.verify()
        assert ops.composite_calls["backward"] == calls + n_views
    torch.cuda.synchronize()
    _check(name, rec.data, n_views, mode)


@pytest.mark.parametrize("kind", ["aux", "pose"])
def test_aux_and_pose_frames_give_the_plain_statistics(gs, kind):
    s = list_scenes.golden("g1_generic")
    c2w, w = _views(s)[0]
    rec = gs.DensifyStats(len(s["pos"]), DEV)
    with gs.densify_stats(rec):
        if kind == "aux":
            _go(gs, _params(s), s, c2w, w, aux=True)                     # the loss reads only the image
        else:
            _go(gs, _params(s), s, torch.tensor(c2w, device=DEV, requires_grad=True), w)
    torch.cuda.synchronize()
    _check("g1_generic", rec.data, 1, kind)


def test_deterministic_mode_gives_equal_bits(gs):
    s = list_scenes.golden("g2_ragged")
    old = gs.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            rec = gs.DensifyStats(len(s["pos"]), DEV)
            with gs.densify_stats(rec):
                for c2w, w in _views(s):
                    _go(gs, _params(s), s, c2w, w)
            torch.cuda.synchronize()
            runs.append(rec.data.clone())
    finally:
        gs.set_deterministic(old)
    assert runs[0].any() and torch.equal(runs[0], runs[1])
    _check("g2_ragged", runs[0], 2, "deterministic")


def _sentinel_stats(gs, n):
    rec = gs.DensifyStats(n, DEV)
    rec.data.copy_(torch.tensor(_sentinel_record(n, 5, 0)))
    return rec, rec.data.clone()


def test_a_frame_that_overflows_its_pair_capacity_adds_nothing(gs):
    """The set-up of the overflow test of the folded Adam step: the capacity kept from earlier frames is far below the frame's pairs."""
    optim = importlib.import_module(PKG + ".optim")
    s = list_scenes.golden("g1_generic")
    c2w, w = _views(s)[0]
    p = _params(s)
    with torch.no_grad():
        gs.render_gaussians(*[p[k] for k in NAMES], torch.tensor(c2w, device=DEV), *list_scenes.cam_args(s), **s["kwargs"])
    rec, before = _sentinel_stats(gs, len(s["pos"]))
    for folded in (False, True):
        with util.forced_pair_capacity(gs, s["H"], s["W"], len(s["pos"]), 100):          # far below the ~1600 pairs of the frame
            p = _params(s)
            opt = optim.GaussianAdam(optim.reference_param_groups(types.SimpleNamespace(**p)), lr=0.01, eps=1e-15)
            route = opt.fused_rest_update(p["f_rest"]) if folded else contextlib.nullcontext()
            with gs.deferred_checks() as chk, route, gs.densify_stats(rec):
                _go(gs, p, s, c2w, w)
            with pytest.raises(gs.PairCapacityExceeded):
                chk.verify()
            torch.cuda.synchronize()
            assert torch.equal(rec.data, before), "an overflowed frame touched the record"


@pytest.mark.parametrize("name", util.EMPTY_CASES)
def test_empty_scenes_leave_the_record_untouched(gs, name):
    s = list_scenes.golden(name)
    rec, before = _sentinel_stats(gs, len(s["pos"]))
    with gs.densify_stats(rec):
        _go(gs, _params(s), s, s["c2w"], dso.upstream(s))
    torch.cuda.synchronize()
    assert torch.equal(rec.data, before)


def test_no_grad_renders_add_nothing(gs):
    s = list_scenes.golden("g1_generic")
    rec, before = _sentinel_stats(gs, len(s["pos"]))
    p = _params(s)
    with gs.densify_stats(rec), torch.no_grad():
        gs.render_gaussians(*[p[k] for k in NAMES], torch.tensor(s["c2w"], device=DEV), *list_scenes.cam_args(s), **s["kwargs"])
    torch.cuda.synchronize()
    assert torch.equal(rec.data, before)


# ---- Trainer ------------------------------------------------------------------------------------------------------------------

TNAMES = ("pos", "opacity_raw", "f_dc", "f_rest", "scale_raw", "q_raw")


def _train_scene():
    """The scene of tests/test_gpu_training.py with three views; the third is 16 pixels wider, so that it has a pair capacity of
    its own (one view of a pass can overflow while the others are valid)."""
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


def _reference_record(gs, s, views):
    """The same views on the initial parameters, one after the other, inside ONE ops.densify_stats block."""
    losses = importlib.import_module(PKG + ".losses")
    p = {k: torch.tensor(s[k], device=DEV, requires_grad=True) for k in TNAMES}
    rec = gs.DensifyStats(len(s["pos"]), DEV)
    with gs.densify_stats(rec):
        for v in views:
            img = gs.render_gaussians(p["pos"], p["f_dc"], p["f_rest"], p["opacity_raw"], p["scale_raw"], p["q_raw"],
                                      torch.tensor(v["c2w"], dtype=torch.float32, device=DEV), v["H"], v["W"], v["fx"], v["fy"], v["cx"], v["cy"])
            loss, _ = losses.compute_loss_device(img, torch.tensor(v["image"], device=DEV), 0.8, 0.2, scale=1.0 / len(views))
            loss.backward()
    torch.cuda.synchronize()
    return rec.data.clone()


def test_trainer_accumulates_the_statistics_of_its_views(gs):
    ops = gs.ops
    s, views = _train_scene()
    old = gs.set_deterministic(True)
    try:
        ref = _reference_record(gs, s, views)
        assert (ref[:, 1] == 3).any() and ref[:, 0].any()
        got = {}
        for streams in (1, 2):
            tr = _trainer(s, view_streams=streams)
            assert tr.densify_stats is None
            out = tr.step(1, views)
            torch.cuda.synchronize()
            assert not out["densified"]
            got[streams] = tr.densify_stats.data.clone()
            assert all(not r.data.any() for r in tr._pass_stats), "the pass records must be zero again after the merge"
        assert torch.equal(got[1], ref), "one step: the statistics of the three views, bit for bit"
        assert torch.equal(got[2], got[1]), "view_streams = 2 differs from view_streams = 1"
        # a step whose first pass overflows: the third view's capacity is far too small, the other two views are valid -- and must
        # not count twice when the pass is repeated
        with util.forced_pair_capacity(gs, views[2]["H"], views[2]["W"], len(s["pos"]), 100):
            tr = _trainer(s)
            before = dict(ops.forward_modes)
            tr.step(1, views)
            torch.cuda.synchronize()
            assert ops.forward_modes["deferred"] == before["deferred"] + 6 and ops.forward_modes["waited"] == before["waited"]
            assert torch.equal(tr.densify_stats.data, ref), "a repeated pass changed the statistics"
    finally:
        gs.set_deterministic(old)


def test_trainer_densifies_from_the_statistics(gs):
    s, views = _train_scene()
    n0 = len(s["pos"])
    old = gs.set_deterministic(True)
    try:
        a = _trainer(s, densification_interval=2)
        b = _trainer(s)                                    # the same two iterations, densified by hand afterwards
        for it in (1, 2):
            oa, ob = a.step(it, views), b.step(it, views)
            assert oa["densified"] == (it == 2) and not ob["densified"]
        torch.cuda.synchronize()
        assert (b.densify_stats.count.max() == 6) and b.densify_stats.data.shape[0] == n0
        c = b.cfg
        b.model.densify_and_prune_screen(b.densify_stats, opacity_threshold=c.prune_opacity_threshold, grad_threshold=c.densify_grad_threshold,
                                         scale_threshold=c.scale_threshold, max_screen_size=None, generator=b._densify_generator(2))
        n1 = a.model.get_num_gaussians()
        assert n1 != n0 and n1 == b.model.get_num_gaussians() and oa["gaussians"] == n1
        for k in TNAMES:
            assert torch.equal(getattr(a.model, k).detach(), getattr(b.model, k).detach()), k
        assert a.densify_stats.data.shape == (n1, 4) and not a.densify_stats.data.any()
        out = a.step(3, views)                             # the next window, on the new set of Gaussians
        torch.cuda.synchronize()
        assert np.isfinite(float(out["loss"])) and a.densify_stats.data.shape == (n1, 4) and a.densify_stats.count.max() == 3
    finally:
        gs.set_deterministic(old)


def test_reference_rule_keeps_no_statistics(gs):
    s, views = _train_scene()
    training = importlib.import_module(PKG + ".training")
    assert training.TrainConfig().densify_rule == "reference"
    tr = _trainer(s, densify_rule="reference")
    tr.step(1, views)
    torch.cuda.synchronize()
    assert tr.densify_stats is None and tr._pass_stats == []
    with pytest.raises(ValueError, match="densify_rule"):
        _trainer(s, densify_rule="paper")
