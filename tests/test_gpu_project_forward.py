"""K1 / K1b (gsplat_project: project_kernel, colour_kernel) on the device, Gaussian by Gaussian: every record value against the float64
reference of tests/project_forward_oracle.py under its per-value bound, the derived columns against their own expression, the
integers and counters exactly -- in every instantiation the host dispatch (gsplat_kernels.hip gsplat_project) can select.
(The host build of the same body is held to the same check in tests/test_project_forward_oracle_cpu.py.)

project_kernel<FUSED, COLOUR, JAC, TOTALS, NB, FILTER> behind project_kernel_for (TOTALS = no GSPLAT_PROJECT_COUNTS_LATE), and
colour_kernel<JAC, NB>; F = COLOUR_FUSED, L = COUNTS_LATE, J = SAVE_SH_JACOBIAN, NB = (degree + 1)^2, filter `off` is FILTER = 0,
`lowpass` and `antialias` are FILTER = 1 with vk.antialias 0 / 1:

    form                                          flags            instantiations   reached by
    <0,1,0,TOTALS,16,FILTER>  un-fused            0, L             2 x 2 = 4        test_every_unfused_form_...[scene-filter]
    <1,1,JAC,TOTALS,NB,FILTER>  colour inside     F, F|J, F|L,     2 x 2 x 4 x 2    test_every_fused_form_...[scene-degree-filter]: the four
                                                  F|L|J            = 32             flag sets at its (degree, filter)
    <1,0,0,TOTALS,16,FILTER>  geometry only       0, J, L, L|J     2 x 2 = 4        the same test (J goes to colour_kernel), any degree
    colour_kernel<JAC, NB>                        0 / L, J / L|J   2 x 4 = 8        the same test, its degree
  48 in all.  F|L|J is held to the float64 reference; the other seven flag sets are held bit-identical to it ("One
  rounding for every kernel variant").  The non-finite test runs the 8 fused flag sets and the 2 un-fused ones under the three filters.

Measured on an MI355X (largest ratio of the device per group over the scenes, degrees and filters, in roundings of the value's
condition scale, beside the float32 oracle's): see DESIGN.md section 8(i).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import device_frame as dfm
from tests import list_scenes
from tests import project_backward_oracle as pbo
from tests import project_forward_oracle as pfo

pytestmark = pytest.mark.gpu
abi = dfm.abi
F, L, J = dfm.F, dfm.L, dfm.J
M = abi.GSPLAT_PROJECT_COUNTS_MAPPED
BASE = F | L | J
FUSED_FLAGS = (F | L | J, F | L, F | J, F, L | J, L, J, 0)
UNFUSED_SCENES = ("g11_unfused", "synth200u")
PER_GAUSSIAN = ("rect", "depth", "tiles", "mask")


def _threads():
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


def _project(fr, flags):
    """One projection: what it left behind, with the counters the host received as a tuple."""
    c = fr.project(flags)
    got = fr.arrays(lists=False)
    assert dfm.counts_tuple(got["counts"]) == dfm.counts_tuple(c), "the counters in the state are not the ones the host received"
    got["counts"] = dfm.counts_tuple(c)
    return got


def _same(a, b, what, colour_everywhere):
    """rec / rect / depth / tiles / mask and the counters bit for bit; the colour of a visible Gaussian that is binned nowhere is left
    out where one of the two evaluates it in colour_kernel."""
    n = a["n"]
    for k in PER_GAUSSIAN:
        bad = np.nonzero((a[k].reshape(n, -1).view(np.uint32) != b[k].reshape(n, -1).view(np.uint32)).any(1))[0]
        assert not len(bad), f"{what}: {k} of Gaussian {bad[0]} differs: {a[k][bad[0]]} / {b[k][bad[0]]}"
    ra, rb = a["rec"].view(np.uint32).copy(), b["rec"].view(np.uint32).copy()
    if not colour_everywhere:
        ra[a["tiles"] == 0, 8:11] = 0
        rb[a["tiles"] == 0, 8:11] = 0
    bad = np.nonzero((ra != rb).any(1))[0]
    assert not len(bad), f"{what}: record of Gaussian {bad[0]} differs: {a['rec'][bad[0]]} / {b['rec'][bad[0]]}"
    assert a["counts"] == b["counts"], f"{what}: counters {a['counts']} / {b['counts']}"


class _Case:
    """The float64 reference of (scene, degree, filter), its K from the float32 oracle, and what n_pairs may move by."""

    def __init__(self, name, degree, filt):
        _threads()
        self.name, self.degree, self.filt = name, degree, filt
        lowpass, aa = pbo.FILTERS[filt]
        self.s, self.color, self.sigma = pfo.scene(name)
        self.fused = self.color is None
        self.bits = abi.filter_bits(lowpass, aa) | (abi.GSPLAT_PROJECT_SH_DEGREE(degree) if self.fused else 0)
        kw = dict(degree=degree, lowpass=lowpass, antialias=aa, color=self.color, sigma=self.sigma)
        self.ref = pfo.reference(self.s, **kw)
        self.K, self.rows = pfo.calibrate(self.ref, pfo.reference(self.s, dtype=torch.float32, scale=False, **kw))
        self.known = pfo.KNOWN_ROWS.get((name, degree, filt))
        ties = pfo.radius_ties(self.ref)
        tr = self.ref.tile_rect[ties]
        self.pairs_slack = int(((tr[:, 2] - tr[:, 0] + 2) * (tr[:, 3] - tr[:, 1] + 2)).sum())
        if name.startswith("synth"):
            assert not len(ties), f"{name}: rows {self.ref.ids[ties]} have a radius within 4 ulp of an integer"


@functools.lru_cache(maxsize=None)
def _case(name, degree, filt):
    return _Case(name, degree, filt)


@functools.lru_cache(maxsize=None)
def _mode_K(degree, filt, fused=True):
    """The largest K per (group, kind) over the scenes of the mode: what a kind of fewer than pfo.MIN_ROWS rows takes."""
    return pfo.merge_K([_case(n, degree, filt).K for n in (pfo.SCENES if fused else UNFUSED_SCENES)])


def _layout(c, got):
    share = pfo.boundary_share(c.ref)
    if c.name.startswith("synth"):
        assert share == 0 and not got["tiles"][c.s["culled"]].any()
        pbo.assert_block_layout(c.name[:8], got["tiles"])
        off = c.s["offscreen"]
        assert c.ref.n_survivors == c.ref.n_visible + int(off.sum()) and (c.name == "synth1" or off.any())
    assert share <= pfo.MAX_BOUNDARY_SHARE, f"{c.name}: {share:.3%} of the visible rows are boundary rows"


def _report(c, dev):
    for key in sorted(dev):
        print(f"{c.name} degree {c.degree} {c.filt}: {key[0]:8s} {key[1]:18s} rows {c.rows.get(key, 0):3d}   float32 oracle "
              f"{c.K.get(key, float('nan')) / 3.0:8.3g}   device {dev[key]:8.3g}")


@pytest.mark.parametrize("filt", list(pbo.FILTERS))
@pytest.mark.parametrize("degree", (0, 1, 2, 3))
@pytest.mark.parametrize("name", pfo.SCENES)
def test_every_fused_form_gaussian_by_gaussian(name, degree, filt):
    c = _case(name, degree, filt)
    ref = c.ref
    fr = dfm.Frame(c.s)
    tag = f"{name} degree {degree} {filt}"
    base = _project(fr, BASE | c.bits)
    _layout(c, base)
    dev = pfo.check(base, ref, c.K, c.rows, f"{tag} F|L|J", other=_mode_K(degree, filt), known=c.known, pairs_slack=c.pairs_slack)
    _report(c, dev)
    nowhere = base["tiles"] == 0
    kj_bits = base["kj"].view(np.uint32)
    for flags in FUSED_FLAGS[1:]:
        what = f"{tag} flags {flags:#x}"
        got = _project(fr, flags | c.bits)
        _same(got, base, what, colour_everywhere=bool(flags & F))
        if not flags & J:                                    # no stray stores: the kj bytes of the cleared state stay zero
            assert not got["kj"].view(np.uint32).any(), f"{what}: kj was written without SAVE_SH_JACOBIAN"
            continue
        if flags & F:                                        # the same kernel code with other counters: the same bits
            assert np.array_equal(got["kj"].view(np.uint32), kj_bits), f"{what}: kj differs from F|L|J"
            continue
        # colour_kernel<true, NB>: kj (and the colour) of the Gaussians that are binned somewhere, held to float64 on its own
        assert not got["kj"][nowhere].view(np.uint32).any(), f"{what}: colour_kernel wrote kj of a Gaussian that is binned nowhere"
        own = dict(got, rec=got["rec"].copy(), kj=got["kj"].copy())
        own["rec"][nowhere, 8:11] = base["rec"][nowhere, 8:11]
        own["kj"][nowhere] = base["kj"][nowhere]
        pfo.check(own, ref, c.K, c.rows, f"{what} (colour_kernel)", other=_mode_K(degree, filt), known=c.known, pairs_slack=c.pairs_slack)
        # the two producers of kj inline the same sh_colour_jac<NB>: bit for bit
        bad = np.nonzero((got["kj"].view(np.uint32) != kj_bits).any(1) & ~nowhere)[0]
        assert not len(bad), f"{what}: kj of Gaussian {bad[0]} from colour_kernel differs from project_kernel's: {got['kj'][bad[0]]} / {base['kj'][bad[0]]}"
    # inactive coefficients: NaN in every inactive f_rest slot changes no bit of record or kj, in either producer of the colour
    if degree < 3:
        s2 = dict(c.s, f_rest=c.s["f_rest"].copy())
        s2["f_rest"][:, tp.inactive_columns(degree)] = np.nan
        fr2 = dfm.Frame(s2)
        for flags in (BASE, L | J):
            got = _project(fr2, flags | c.bits)
            _same(got, base, f"{tag} flags {flags:#x} with NaN in the inactive slots", colour_everywhere=bool(flags & F))
            rows = slice(None) if flags & F else ~nowhere
            assert np.array_equal(got["kj"].view(np.uint32)[rows], kj_bits[rows]), f"{tag} flags {flags:#x}: NaN in an inactive slot reached kj"


@pytest.mark.parametrize("filt", list(pbo.FILTERS))
@pytest.mark.parametrize("name", UNFUSED_SCENES)
def test_every_unfused_form_gaussian_by_gaussian(name, filt):
    c = _case(name, 3, filt)
    fr = dfm.Frame(c.s, unfused=(c.color, c.sigma))
    base = _project(fr, L | c.bits)
    _layout(c, base)
    assert np.array_equal(base["rec"][c.ref.ids, 8:11].view(np.uint32), c.color[c.ref.ids].view(np.uint32)), "the un-fused colour is copied"
    dev = pfo.check(dict(base, kj=None), c.ref, c.K, c.rows, f"{name} {filt} L", other=_mode_K(3, filt, False), known=c.known, pairs_slack=c.pairs_slack)
    _report(c, dev)
    got = _project(fr, c.bits)
    _same(got, base, f"{name} {filt} flags 0", colour_everywhere=True)
    assert not base["kj"].view(np.uint32).any() and not got["kj"].view(np.uint32).any(), "un-fused inputs have no kj"


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", list(pbo.FILTERS))
@pytest.mark.parametrize("unfused", (False, True))
def test_non_finite_rows_are_culled_as_the_oracle_culls_them(unfused, filt):
    """One ordinary visible row each with NaN / +inf / -inf in scale_raw, NaN / inf in q_raw, NaN / +-inf in pos, NaN / +inf in
    opacity_raw (un-fused: NaN / inf in sigma): culled exactly where the oracle culls (-inf scale and +inf opacity stay visible), and
    every other row's record, rect, tiles, mask bit-identical to the same scene with those rows at opacity_raw = -30; the counters too."""
    _threads()
    lowpass, aa = pbo.FILTERS[filt]
    bits = abi.filter_bits(lowpass, aa)
    bad, twin, rows, stays = pfo.nonfinite(unfused)
    st = pbo.Stage(bad[0], 3, lowpass, aa, bad[1], bad[2])
    assert np.array_equal(np.isin(rows, st.ids), stays)
    want = (int(st.st["n_survivors"]), len(st.ids))
    fa, fb = (dfm.Frame(s, unfused=None if not unfused else (color, sigma)) for s, color, sigma in (bad, twin))
    for flags in ((0, L) if unfused else FUSED_FLAGS):
        what = f"{'un-fused' if unfused else 'fused'} {filt} flags {flags:#x}"
        a, b = _project(fa, flags | bits), _project(fb, flags | bits)
        for i, keep in zip(rows, stays):
            assert (a["tiles"][i] != 0) == keep, f"{what}: poisoned row {i} is {'culled' if keep else 'visible'} ({a['tiles'][i]} lists)"
        assert a["counts"][:2] == want, f"{what}: (n_survivors, n_visible) = {a['counts'][:2]}, the oracle's {want}"
        _same(a, b, what, colour_everywhere=True)
        assert np.array_equal(a["kj"].view(np.uint32), b["kj"].view(np.uint32)), f"{what}: kj"


# ---- the counters --------------------------------------------------------------------------------------------------------------------

def _counters_scene(n):
    """n cheap rows on 32 x 48 pixels under the identity camera, eight kinds in turn (i % 8), the expected counts by construction:
    0: 0.2 px wide at (8.3, 4.2): radius 1, one tile, one list;  1: 0.5 px wide at (15.5, 4.2): radius 2, tiles 0..1 and lists 0..1 of
    row 0;  2: behind the camera;  3: below the opacity cut;  4: a survivor off the image (20 px inside the guard band, radius 1);
    5: inside the near plane;  6: beyond the far plane;  7: beyond the guard band."""
    H, W, f, z = 32, 48, 40.0, 4.0
    kind = np.arange(n) % 8
    u = np.select([kind == 1, kind == 4, kind == 7], [15.5, W + 20.0, W + 60.0], 8.3)
    zz = np.select([kind == 2, kind == 5, kind == 6], [-z, 0.005, 150.0], z)
    pos = np.stack([(u - W / 2) / f * zz, np.full(n, (4.2 - H / 2) / f) * zz, zz], 1)
    sr = np.where(kind == 1, np.log(0.5 * z / f), np.log(0.2 * z / f))
    d = dict(pos=pos, scale_raw=np.repeat(sr[:, None], 3, 1), q_raw=np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)), opacity_raw=np.where(kind == 3, -10.0, 1.0),
             f_dc=np.zeros((n, 3)), f_rest=np.zeros((n, 45)))
    na, nb, noff = int((kind == 0).sum()), int((kind == 1).sum()), int((kind == 4).sum())
    return list_scenes._pack(d, H, W, f, f, W / 2.0, H / 2.0), (na + nb + noff, na + nb, na + 2 * nb, 2, na + 2 * nb)


@pytest.mark.parametrize("n", (256 * 64 + 1, 300 * 64 + 7))
def test_counters_are_exact_in_every_variant_on_one_counter_block(n):
    """256 * 64 + 1 rows: 257 waves on the 256 counter shards -- shard 0 alone holds two waves, the wrap of the arrival arithmetic
    (waves_of_shard); 300 * 64 + 7: ragged.  Totalled by the projection or by the first binning kernel, handed over by copy or by mapped
    store, alternating on ONE counter block, which every call leaves zeroed (Frame.project asserts it)."""
    s, want = _counters_scene(n)
    fr = dfm.Frame(s)
    seq = (F, F | L, F | M, F | L | M, F | L, F, L | M, M, 0, L, F | L | J, F | J | M)
    for k, flags in enumerate(seq + seq[::-1]):
        c = dfm.counts_tuple(fr.project(flags))
        assert c == want, f"n = {n}, call {k} (flags {flags:#x}): counters {c}, by construction {want}"
    tiles = fr.arrays(lists=False)["tiles"]
    assert int(tiles.max()) == want[3] and int(tiles.astype(np.int64).sum()) == want[4]
