"""Per-Gaussian feature vectors on the device.

Kernel level: raster_features_kernel and raster_features_adjoint_kernel through ctypes on tests/device_frame.Frame, with canaries
behind `out` and `grad_features`, against tests/feature_oracle.py's float64 evaluation of the records and lists THE DEVICE left:
    |delta| <= K 2^-24 scale + allowance,
K = 3 x the largest ratio of the oracle's OWN float32 evaluation against its float64 (per scene; never measured against the kernel).
Each check prints the device's own ratio beside the calibration (pytest -s).  Features and upstream values are signed, seeded, random.

Channel counts 1, 3, 8, 9, 17 -- below a group, a full group, a group and one channel, two groups and one -- on the light scenes (a
golden case with a ragged image, the 300-entry list, the 5 x 13 image); C = 9 on the heavy ones (more than 24 entries in one sub-tile,
huge Gaussians, equal depths), whose references cost seconds per slab of three channels; C = 512 once, on 65 Gaussians.

Op level: gs.features.render / lift against the same oracle on the records a Frame of the same pose leaves, against
render_gaussians(sh_degree=0), against the adjoint entry and against gs.contribution."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import scenes
from tests import device_frame as dfm
from tests import feature_oracle as fo
from tests import list_scenes

pytestmark = pytest.mark.gpu
abi = dfm.abi
DEV = dfm.DEV
NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
GEOMETRY = ("pos", "opacity_raw", "scale_raw", "q_raw")
SENTINEL = 12345.0               # rows the adjoint may not touch: Gaussians in no list, and the tail behind the table
TAIL = 64
POISON = 3                       # floats of NaN behind every table and map the kernels read
LIGHT, HEAVY = ("g2_ragged", "stacked", "stacked_5x13"), ("hot_spot", "huge", "equal_depths")
CHANNELS = (1, 3, 8, 9, 17)
CASES = [(n, c) for n in LIGHT for c in CHANNELS] + [(n, 9) for n in HEAVY]
SH_C0 = 0.28209479177387814


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _scene(name):
    if name == "hot_spot":                   # 1500 Gaussians on the same 7 x 7 pixels: every chunk of 64 puts more than 24 into one sub-tile
        return list_scenes.hot_spot(1500, (16, 32))
    if name == "stacked65_5x13":
        return list_scenes.stacked(65, (5, 13))
    return list_scenes.raster_scene(name)


def _poisoned(a, lead=0):
    """The float32 array `a` flat in a device buffer of lead + a.size + POISON floats, NaN before and behind it; returns (buffer, view)."""
    buf = torch.full((lead + a.size + POISON,), float("nan"), dtype=torch.float32, device=DEV)
    buf[lead:lead + a.size] = torch.tensor(np.ascontiguousarray(a, np.float32).ravel(), device=DEV)
    return buf, buf[lead:lead + a.size]


def _forward(fr, feats, ch, lead=0):
    """gsplat_features_forward of the table feats [n, ch] on the frame: the map [H, W, ch] from a buffer of 0xFF bytes + canary."""
    H, W = fr.s["H"], fr.s["W"]
    keep, view = _poisoned(feats, lead)
    out = fr._buf("feature_map", H * W * ch * 4)
    abi.check(fr.lib.gsplat_features_forward(fr.n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), _vp(view), ch, out, fr.st),
              "gsplat_features_forward")
    torch.cuda.synchronize()
    return fr._floats("feature_map", (H, W, ch))


def _table(n, ch, untouched):
    t = np.zeros((n * ch + TAIL,), np.float32)
    t[n * ch:] = SENTINEL
    t[:n * ch].reshape(n, ch)[untouched] = SENTINEL
    return torch.tensor(t, device=DEV)


def _adjoint(fr, G, ch, table, lead=0):
    keep, view = _poisoned(G, lead)
    abi.check(fr.lib.gsplat_features_adjoint(fr.n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), _vp(view), ch, _vp(table), fr.st),
              "gsplat_features_adjoint")
    torch.cuda.synchronize()
    return table.cpu().numpy().copy()


def _rows(got, n, ch, untouched):
    """The [n, ch] rows of a table with the untouched rows (checked to hold the sentinel still) read as the zeros a caller starts from."""
    assert (got[n * ch:] == SENTINEL).all(), "the tail behind grad_features was written"
    rows = got[:n * ch].reshape(n, ch).copy()
    assert (rows[untouched] == SENTINEL).all(), "the row of a Gaussian in no list was written"
    rows[untouched] = 0
    return rows


def _frame(s, flags=dfm.F):
    fr = dfm.Frame(s)
    counts = fr.project(flags)
    assert counts.n_binned > 0
    fr.bin(counts.n_binned)
    a = fr.arrays()
    return fr, a, (a["rec"], a["ranges"], a["sorted_ids"], a["lists_x"], s["H"], s["W"]) + list_scenes.thresholds(s, as_float32=True)


class _Run:
    """Everything of one scene at its largest channel count, computed once: the device's state, the float64 references of the device's
    records and lists, and K.  A smaller channel count reads the first channels of the same table and maps: the references are slices."""

    def __init__(self, name, cmax):
        s = self.s = _scene(name)
        self.fr, self.arr, self.args = _frame(s)
        self.n, self.cmax = self.fr.n, cmax
        rng = np.random.default_rng(23)
        self.feats = rng.normal(0, 1, (self.n, cmax)).astype(np.float32)
        self.G = rng.normal(0, 1, (s["H"], s["W"], cmax)).astype(np.float32)
        self.K_map, self.K_rows, self.fwd, self.adj = fo.calibration(self.args, self.feats, self.G)
        self.untouched = self.arr["tiles"] == 0

    def refs(self, ch):
        return (fo.Ref(self.fwd.value[..., :ch], self.fwd.scale[..., :ch], self.fwd.allow[..., :ch]),
                fo.Ref(self.adj.value[:, :ch], self.adj.scale[:, :ch], self.adj.allow[:, :ch], self.adj.in_list))


_RUNS = {}


def _run(name, cmax=None):
    """(A failed set-up is kept and raised again: nothing runs on the device a second time.)"""
    if name not in _RUNS:
        try:
            _RUNS[name] = _Run(name, cmax or (max(CHANNELS) if name in LIGHT else 9))
        except Exception as e:
            _RUNS[name] = e
    if isinstance(_RUNS[name], Exception):
        raise _RUNS[name]
    return _RUNS[name]


def _kernels_against_the_oracle(run, name, ch):
    fr, n = run.fr, run.n
    fwd, adj = run.refs(ch)
    assert np.array_equal(run.untouched, ~adj.in_list)
    feats, G = np.ascontiguousarray(run.feats[:, :ch]), np.ascontiguousarray(run.G[..., :ch])
    got = _forward(fr, feats, ch)
    assert fr.canaries_intact()
    r_map = fo.check(got, fwd, run.K_map, f"{name} C={ch} forward")
    unreached = (fwd.scale == 1.0) & (fwd.allow == 0.0)                  # no Gaussian has a weight there (the features are never 0)
    assert unreached.any() or name != "g2_ragged"
    assert (got[unreached] == 0.0).all(), "a pixel no Gaussian reaches must be exactly 0.0"
    table = _table(n, ch, run.untouched)
    once = _rows(_adjoint(fr, G, ch, table), n, ch, run.untouched)
    twice = _rows(_adjoint(fr, G, ch, table), n, ch, run.untouched)
    r_rows = fo.check(once, adj, run.K_rows, f"{name} C={ch} adjoint")
    fo.check(twice, adj, run.K_rows, f"{name} C={ch} adjoint, two calls", calls=2)
    assert once.any() and got.any()
    print(f"{name} C={ch}: device |delta| / (2^-24 scale) map {r_map:.2f}, rows {r_rows:.2f}; float32 mode {run.K_map / 3:.2f}, {run.K_rows / 3:.2f} "
          f"(bounds: 3 x); {int(adj.in_list.sum())} of {n} Gaussians in lists, longest list {int((run.arr['ranges'][:, 1] - run.arr['ranges'][:, 0]).max())}")


@pytest.mark.parametrize("name,ch", CASES, ids=[f"{n}-C{c}" for n, c in CASES])
def test_kernels_against_the_oracle_of_the_device_records(name, ch):
    run = _run(name)
    if name == "hot_spot":
        m = _box_masks(run)
        assert ((m[:64, None] >> np.arange(8)) & 1).sum(0).max() > 24, "the first chunk of the longest list must overflow a sub-tile queue"
    if name == "stacked":
        assert (run.arr["ranges"][:, 1] - run.arr["ranges"][:, 0]).max() == 300
    if name in ("g2_ragged", "stacked_5x13"):
        assert run.s["H"] % 8 and run.s["W"] % 16
    _kernels_against_the_oracle(run, name, ch)


def _box_masks(run):
    """The box-test sub-tile masks (gs_raster.h: subtile_mask) of the entries of the longest list, in list order."""
    a = run.arr
    ln = a["ranges"][:, 1].astype(np.int64) - a["ranges"][:, 0]
    l_ = int(np.argmax(ln))
    ids = a["sorted_ids"][a["ranges"][l_, 0]:a["ranges"][l_, 1]].astype(np.int64)
    r = a["rec"][ids].astype(np.float64)
    ox, oy = (l_ % a["lists_x"]) * 16, (l_ // a["lists_x"]) * 8
    x0, x1, y0, y1 = r[:, 0] - r[:, 6] - ox, r[:, 0] + r[:, 6] - ox, r[:, 1] - r[:, 7] - oy, r[:, 1] + r[:, 7] - oy
    cm = sum(((x1 >= 4 * k) & (x0 <= 4 * k + 3)).astype(np.int64) << k for k in range(4))
    return np.where((y1 >= 0) & (y0 <= 3), cm, 0) | np.where((y1 >= 4) & (y0 <= 7), cm << 4, 0)


def test_512_channels_on_the_smallest_scene():
    run = _run("stacked65_5x13", 512)
    _kernels_against_the_oracle(run, "stacked65_5x13", 512)


def test_an_overflowed_frame_leaves_the_map_and_the_table_untouched():
    s = _scene("g2_ragged")
    fr = dfm.Frame(s)
    counts = fr.project(dfm.F)
    fr.bin(int(counts.n_binned) - 1)                        # the lists of this frame are garbage: the kernels must not read them
    rng = np.random.default_rng(2)
    ch = 9
    got = _forward(fr, rng.normal(0, 1, (fr.n, ch)).astype(np.float32), ch)
    assert (got.view(np.uint32) == 0xFFFFFFFF).all() and fr.canaries_intact()
    table = torch.full((fr.n * ch + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    after = _adjoint(fr, rng.normal(0, 1, (s["H"], s["W"], ch)).astype(np.float32), ch, table)
    assert (after == SENTINEL).all() and fr.canaries_intact()


@pytest.mark.parametrize("ch", [8, 9])
def test_poison_around_the_table_changes_nothing_and_alignment_does_not_matter(ch):
    """The tables of every test here lie in buffers with NaNs behind them (a [N, C + 3]-like padded allocation read as rows of C); here
    also with a NaN in front, which moves the table off its 16-byte alignment: C = 8 then takes the float-by-float path, and the map
    must have the bits of the aligned call."""
    run = _run("g2_ragged")
    fr, n = run.fr, run.n
    feats, G = np.ascontiguousarray(run.feats[:, :ch]), np.ascontiguousarray(run.G[..., :ch])
    aligned, shifted = _forward(fr, feats, ch), _forward(fr, feats, ch, lead=1)
    assert np.isfinite(aligned).all() and np.array_equal(aligned.view(np.uint32), shifted.view(np.uint32))
    clean = torch.tensor(feats, device=DEV)                  # an exact allocation, nothing behind it that belongs to the test
    out = fr._buf("feature_map", run.s["H"] * run.s["W"] * ch * 4)
    abi.check(fr.lib.gsplat_features_forward(n, fr.capacity, C.byref(fr.view), _vp(fr.state), _vp(fr.bin_state), _vp(clean), ch, out, fr.st),
              "gsplat_features_forward")
    torch.cuda.synchronize()
    assert np.array_equal(fr._floats("feature_map", aligned.shape).view(np.uint32), aligned.view(np.uint32)) and fr.canaries_intact()
    _, adj = run.refs(ch)
    rows = _rows(_adjoint(fr, G, ch, _table(n, ch, run.untouched), lead=1), n, ch, run.untouched)
    fo.check(rows, adj, run.K_rows, f"g2_ragged C={ch} adjoint, map off its alignment")


# ---- op level -------------------------------------------------------------------------------------------------------------------

OP_SCENE = "g1_generic"


def _poses(s):
    """The golden's pose and one more: the same camera moved a twelfth of a turn round the scene centre."""
    return [np.asarray(s["c2w"], np.float32), (scenes.orbit_c2w(1, 12).astype(np.float64) @ np.asarray(s["c2w"], np.float64)).astype(np.float32)]


class _Op:
    """The op-level scene, once: its tensors, per pose the Frame at SH degree 0, the oracle's references for one table / one map, K."""

    def __init__(self):
        s = self.s = list_scenes.golden(OP_SCENE)
        self.t = {k: torch.tensor(s[k], device=DEV) for k in NAMES}
        self.geo = [self.t[k] for k in GEOMETRY]
        self.cam, self.kw = list_scenes.cam_args(s), s["kwargs"]
        self.n, self.ch = len(s["pos"]), 5
        rng = np.random.default_rng(41)
        self.feats = rng.normal(0, 1, (self.n, self.ch)).astype(np.float32)
        self.G = rng.normal(0, 1, (s["H"], s["W"], self.ch + 1)).astype(np.float32)
        self.G[..., self.ch] = 1.0                                                  # (channel C of lift: the weight)
        self.poses, self.frames = _poses(s), []
        for k, c2w in enumerate(self.poses):
            fr, a, args = _frame(dict(s, c2w=c2w), dfm.F | abi.GSPLAT_PROJECT_SH_DEGREE(0))
            f = dict(fr=fr, arr=a, args=args)
            if k == 0:       # (the map of the table, and the adjoint of all six channels of G, the weight channel included)
                f["K_map"], f["fwd"] = fo.calibrate_render(args, self.feats)
                f["K_rows"], f["adj"] = fo.calibrate_adjoint(args, self.G)
            self.frames.append(f)

    def render(self, gs, feats, pose=0, **mode):
        return gs.features.render(self.t["pos"], feats, *self.geo[1:], torch.tensor(self.poses[pose], device=DEV), *self.cam, **self.kw, **mode)

    def lift(self, gs, poses, maps, **kw):
        return gs.features.lift(*self.geo, [torch.tensor(self.poses[p], device=DEV) for p in poses], maps, *self.cam, **self.kw, **kw)


_OP = []


def _op():
    if not _OP:
        try:
            _OP.append(_Op())
        except Exception as e:
            _OP.append(e)
    if isinstance(_OP[0], Exception):
        raise _OP[0]
    return _OP[0]


def test_render_against_the_oracle_and_the_sh_degree_0_image(gs):
    op = _op()
    f0 = op.frames[0]
    got = op.render(gs, torch.tensor(op.feats, device=DEV))
    torch.cuda.synchronize()
    assert got.shape == (op.s["H"], op.s["W"], op.ch) and got.dtype == torch.float32 and not got.requires_grad
    r = fo.check(got.cpu().numpy(), f0["fwd"], f0["K_map"], "features.render")
    print(f"features.render C={op.ch}: device ratio {r:.2f}, float32 mode {f0['K_map'] / 3:.2f}")
    # the SH-degree-0 colours as a table, formed in torch by the reference's rule (spherical_harmonics.py:118-166, oracle/torch_port.sh_colour):
    # sigmoid(SH_C0 f_dc), in float64 and rounded once
    colours = torch.sigmoid(SH_C0 * op.t["f_dc"].double()).float().contiguous()
    with torch.no_grad():
        image = gs.render_gaussians(*[op.t[k] for k in NAMES], torch.tensor(op.poses[0], device=DEV), *op.cam, sh_degree=0, **op.kw).cpu().numpy()
    fmap = op.render(gs, colours).cpu().numpy()
    K, ref = fo.calibrate_render(f0["args"], colours.cpu().numpy())
    fo.check(fmap, ref, K, "features.render of the colours")
    inside = (image > 0.0) & (image < 1.0)
    assert inside.mean() > 0.3
    bound = 2.0 * (K * fo.EPS * ref.scale + ref.allow)
    d = np.abs(fmap.astype(np.float64) - image)
    assert (d[inside] <= bound[inside]).all(), f"largest excess {float((d - bound)[inside].max()):.3e}"
    print(f"colours against render_gaussians(sh_degree=0): largest |delta| / bound {float((d[inside] / bound[inside]).max()):.3f} over {int(inside.sum())} values")
    # a channel of ones renders the opacity map
    ones = op.render(gs, torch.ones((op.n, 1), device=DEV))
    with torch.no_grad():
        alpha = gs.render_gaussians(*[op.t[k] for k in NAMES], torch.tensor(op.poses[0], device=DEV), *op.cam, sh_degree=0, aux=True, **op.kw)[2]
    K1, ref1 = fo.calibrate_render(f0["args"], np.ones((op.n, 1), np.float32))
    fo.check(ones[..., 0].cpu().numpy()[..., None], ref1, K1, "a channel of ones")
    assert (np.abs(ones[..., 0].cpu().numpy().astype(np.float64) - alpha.cpu().numpy()) <= 2.0 * (K1 * fo.EPS * ref1.scale + ref1.allow)[..., 0]).all()


def test_autograd_is_the_adjoint_entry_and_grad_accumulates(gs):
    op = _op()
    f0 = op.frames[0]
    fr, ch = f0["fr"], op.ch
    G = np.ascontiguousarray(op.G[..., :ch])
    adj = fo.Ref(f0["adj"].value[:, :ch], f0["adj"].scale[:, :ch], f0["adj"].allow[:, :ch], f0["adj"].in_list)
    untouched = f0["arr"]["tiles"] == 0
    entry = _rows(_adjoint(fr, G, ch, _table(op.n, ch, untouched)), op.n, ch, untouched)
    fo.check(entry, adj, f0["K_rows"], "the adjoint entry")
    feats = torch.tensor(op.feats, device=DEV, requires_grad=True)
    Gd = torch.tensor(G, device=DEV)
    out = op.render(gs, feats)
    assert out.requires_grad
    (g,) = torch.autograd.grad((out * Gd).sum(), feats)
    torch.cuda.synchronize()
    r = fo.check(g.cpu().numpy(), adj, f0["K_rows"], "autograd.grad of features.render")
    bound = f0["K_rows"] * fo.EPS * adj.scale + adj.allow
    assert (np.abs(g.cpu().numpy().astype(np.float64) - entry) <= 2.0 * bound).all()
    print(f"autograd through features.render C={ch}: device ratio {r:.2f}, float32 mode {f0['K_rows'] / 3:.2f}")
    for _ in range(2):
        (op.render(gs, feats) * Gd).sum().backward()
    torch.cuda.synchronize()
    fo.check(feats.grad.cpu().numpy(), adj, f0["K_rows"], "feats.grad after two backward passes", calls=2)
    # the frozen geometry and the deterministic mode are refused on the device as on the host
    with pytest.raises(ValueError, match="geometry is frozen"):
        gs.features.render(op.t["pos"].clone().requires_grad_(True), feats, *op.geo[1:], torch.tensor(op.poses[0], device=DEV), *op.cam)
    old = gs.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="no deterministic adjoint"):
            op.render(gs, feats)
    finally:
        gs.set_deterministic(old)


def test_lowpass_and_antialias_change_the_map_and_agree_with_the_oracle(gs):
    op = _op()
    s = op.s
    feats = torch.tensor(op.feats, device=DEV)
    plain = op.render(gs, feats).cpu().numpy()
    got = op.render(gs, feats, lowpass=0.3, antialias=True).cpu().numpy()
    assert not np.array_equal(got, plain) and np.abs(got - plain).max() > 1e-3
    fr, a, args = _frame(dict(s, c2w=op.poses[0]), dfm.F | abi.GSPLAT_PROJECT_SH_DEGREE(0) | abi.filter_bits(0.3, True))
    K, ref = fo.calibrate_render(args, op.feats)
    r = fo.check(got, ref, K, "features.render lowpass=0.3 antialias")
    print(f"features.render lowpass=0.3 antialias=True: device ratio {r:.2f}, float32 mode {K / 3:.2f}")
    with pytest.raises(fo.FeatureError):
        fo.check(plain, ref, K, "the unfiltered map against the filtered records")


def test_lift_over_two_poses_is_the_sum_of_two_calls_and_its_weight_is_contributions(gs):
    op = _op()
    ch = op.ch
    maps = [torch.tensor(np.ascontiguousarray(op.G[..., :ch]), device=DEV), torch.tensor(np.ascontiguousarray(op.G[::-1, :, :ch]), device=DEV)]
    refs = []
    for k, f in enumerate(op.frames):
        if k == 0:
            refs.append((f["adj"], f["K_rows"]))
        else:                                                                 # (the second pose lifts the map upside down)
            Gk = np.concatenate([op.G[::-1, :, :ch], np.ones_like(op.G[..., :1])], -1)
            refs.append(fo.calibrate_adjoint(f["args"], Gk)[::-1])
    both, w_both = op.lift(gs, [0, 1], maps)
    a, wa = op.lift(gs, [0], maps[:1])
    b, wb = op.lift(gs, [1], torch.stack(maps[1:]))                          # ([V, H, W, C] as one tensor)
    torch.cuda.synchronize()
    assert both.shape == (op.n, ch) and w_both.shape == (op.n,) and both.is_contiguous() and w_both.is_contiguous()
    value = sum(r.value for r, _ in refs)
    bound = sum(K * fo.EPS * r.scale + r.allow for r, K in refs)
    full = lambda s_, w_: np.concatenate([s_.cpu().numpy().astype(np.float64), w_.cpu().numpy().astype(np.float64)[:, None]], 1)
    for what, got, want, bnd in (("pose 0", full(a, wa), refs[0][0].value, refs[0][1] * fo.EPS * refs[0][0].scale + refs[0][0].allow),
                                 ("pose 1", full(b, wb), refs[1][0].value, refs[1][1] * fo.EPS * refs[1][0].scale + refs[1][0].allow),
                                 ("both poses", full(both, w_both), value, bound), ("the sum of two calls", full(a, wa) + full(b, wb), value, bound)):
        d = np.abs(got - want)
        assert (d <= bnd).all(), f"lift, {what}: Gaussian {np.unravel_index(np.argmax(d - bnd), d.shape)}: excess {float((d - bnd).max()):.3e}"
    assert (np.abs(full(both, w_both) - full(a, wa) - full(b, wb)) <= 2.0 * bound).all()
    # accumulation into `out`: the second pose added to the first call's pair
    acc = op.lift(gs, [1], maps[1:], out=(a.clone(), wa.clone()))
    assert (np.abs(full(*acc) - value) <= bound + fo.EPS * np.abs(full(*acc))).all()       # (the one float32 addition into `out`: half an ulp of its result)
    # the weight against gs.contribution: two independent kernels, the same pixels
    st = gs.contribution(*[op.t[k] for k in NAMES], [torch.tensor(p, device=DEV) for p in op.poses], *op.cam, sh_degree=0, **op.kw)
    torch.cuda.synchronize()
    pairs = sum(f["arr"]["tiles"].astype(np.float64) for f in op.frames)
    tol = bound[:, ch] + pairs * 2.0 ** -32
    wsum, pix = st.weight_sum.cpu().numpy().astype(np.float64), st.pixels.cpu().numpy()
    d = np.abs(w_both.cpu().numpy().astype(np.float64) - wsum)
    assert (d <= tol).all(), f"weight against contribution: Gaussian {int(np.argmax(d - tol))}: |delta| {float(d.max()):.3e}"
    assert (pix > 0).any() and (pix == 0).any() and (w_both.cpu().numpy()[pix == 0] == 0.0).all() and (w_both.cpu().numpy()[pix > 0] > 0.0).all()
    print(f"lift weight against contribution: largest |delta| / tolerance {float((d / np.maximum(tol, 1e-300)).max()):.3f}; {int((pix > 0).sum())} of {op.n} Gaussians weighted")


def test_a_culled_pose_gives_zeros_and_an_offscreen_pose_raises(gs):
    op = _op()
    s = op.s
    feats = torch.tensor(op.feats, device=DEV, requires_grad=True)
    behind = np.array(s["c2w"], np.float32)
    behind[:3, :3] = behind[:3, :3] @ np.diag([-1.0, 1.0, -1.0]).astype(np.float32)          # turned right round: no survivor, no error
    out = gs.features.render(op.t["pos"], feats, *op.geo[1:], torch.tensor(behind, device=DEV), *op.cam, **op.kw)
    assert out.shape == (s["H"], s["W"], op.ch) and not out.any()
    (g,) = torch.autograd.grad(out.sum(), feats, allow_unused=True)
    assert g is None or not g.any()
    sums, weight = gs.features.lift(*op.geo, [torch.tensor(behind, device=DEV)], [torch.ones((s["H"], s["W"], 2), device=DEV)], *op.cam, **op.kw)
    assert sums.shape == (op.n, 2) and not sums.any() and not weight.any()
    a = np.deg2rad(75.0)                 # the camera turned 75 degrees about its own y axis: survivors, none of them on screen
    away = np.array(s["c2w"], np.float64)
    away[:3, :3] = away[:3, :3] @ np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    away = torch.tensor(away.astype(np.float32), device=DEV)
    with pytest.raises(Exception) as e:
        gs.features.render(op.t["pos"], feats, *op.geo[1:], away, *op.cam, **op.kw)
    assert str(e.value) == gs.ops.OFFSCREEN_MSG
    with pytest.raises(Exception) as e:
        gs.features.lift(*op.geo, [away], [torch.ones((s["H"], s["W"], 2), device=DEV)], *op.cam, **op.kw)
    assert str(e.value) == gs.ops.OFFSCREEN_MSG
    # inside deferred_checks() the op still waits: the frame is whole when the call returns, and the block has nothing to verify
    with gs.deferred_checks() as chk:
        inside = op.render(gs, feats.detach())
    assert chk.verify() == [] and torch.equal(inside, op.render(gs, feats.detach()))


def test_features_share_the_waited_front_end_and_keep_it_unchanged(gs):
    """The front end features.render / lift share with ops.contribution, seen from outside, on the golden scene case_g1
    at its own image size (tests/test_gpu_contrib.py has the sibling for contribution): the pair capacity a waited pose leaves under
    the features' own key; render_stats() and binned_pairs() untouched; "project" and "bin" counted once per pose that bins; a
    backward pass on another stream, which may not change the front end the node saved."""
    op, ops = _op(), gs.ops
    s, g1 = op.s, scenes.case_g1()
    assert all(np.array_equal(g1[k], s[k]) for k in NAMES + ("c2w", "H", "W")) and not op.kw
    c2w, moved = (torch.tensor(p, device=DEV) for p in op.poses)
    behind = c2w.clone()
    behind[:3, :3] = c2w[:3, :3] @ torch.diag(torch.tensor([-1.0, 1.0, -1.0], device=DEV))      # flipped: every z is below near
    dev = op.t["pos"].device
    key = ops.capacity_key(dev, ops._frame_spec(True, *op.cam, 0.01, 100.0, 32, 16, 1e-6, 6.25, 0.99, 1 / 128., sh_degree=0), op.n)
    feats = torch.tensor(op.feats, device=DEV)
    maps = [torch.tensor(np.ascontiguousarray(op.G[..., :op.ch]), device=DEV)] * 3
    saved = dict(ops._ws.capacity)
    try:
        ops._ws.capacity.pop(key, None)                                   # (the key holds no SH degree: the render's entry too)
        waited = ops.forward_modes["waited"]
        with torch.no_grad():                                             # the waited render of the same pose: what the counters say
            gs.render_gaussians(*[op.t[k] for k in NAMES], c2w, *op.cam)
        assert ops.forward_modes["waited"] == waited + 1
        stats = ops.render_stats()
        ops._ws.capacity.pop(key)
        first = op.render(gs, feats)
        binned = ops.binned_pairs()
        assert binned > 0 and stats[0] > 0 and ops._ws.pair_capacity(key) == int(binned * 1.25) + 4096
        timer = ops.StageTimer()
        ops.set_stage_timer(timer)
        try:
            sums, weight = gs.features.lift(*op.geo, [moved, behind, c2w], maps, *op.cam)
            torch.cuda.synchronize()
        finally:
            ops.set_stage_timer(None)
        assert {k: v[0] for k, v in timer.totals_ms().items()} == {"project": 3, "bin": 2}      # (the culled pose projects and bins nothing)
        assert ops.render_stats() == stats and ops.binned_pairs() == binned and sums.any() and weight.any()
    finally:
        ops._ws.capacity.clear()
        ops._ws.capacity.update(saved)
    # one channel, upstream ones: the gradient is the weight column of the adjoint's reference (channel C of op.G is all ones)
    adj, K = op.frames[0]["adj"], op.frames[0]["K_rows"]
    ref = fo.Ref(adj.value[:, op.ch:], adj.scale[:, op.ch:], adj.allow[:, op.ch:], adj.in_list)
    table = [torch.tensor(op.feats[:, :1].copy(), device=DEV, requires_grad=True) for _ in range(2)]
    op.render(gs, table[0]).sum().backward()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = op.render(gs, table[1])
        out.sum().backward(retain_graph=True)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    r0 = fo.check(table[0].grad.cpu().numpy(), ref, K, "feats.grad, default stream")
    r1 = fo.check(table[1].grad.cpu().numpy(), ref, K, "feats.grad, render and backward on a side stream")
    bound = K * fo.EPS * ref.scale + ref.allow
    assert (np.abs(table[1].grad.cpu().numpy().astype(np.float64) - table[0].grad.cpu().numpy()) <= 2.0 * bound).all()
    print(f"backward on a side stream: device ratio {r1:.2f} (default stream {r0:.2f}), float32 mode {K / 3:.2f}")
    # a second backward pass through the same node, now on the default stream: the saved front end serves it as it is
    out.sum().backward()
    torch.cuda.synchronize()
    fo.check(table[1].grad.cpu().numpy(), ref, K, "feats.grad after a second backward pass on the default stream", calls=2)
    again = op.render(gs, table[1].detach())
    assert torch.equal(again, out.detach()) and torch.equal(op.render(gs, feats), first)
