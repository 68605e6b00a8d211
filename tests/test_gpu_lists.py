"""What the projection, binning, sort and raster kernels leave on the DEVICE, looked at directly: the per-Gaussian records (K1),
the (list, Gaussian) pairs, their order and the launch plan (K3a - K5, K4), and the per-pair sub-tile masks (K6).  Integer
quantities are checked exactly, floats against the float64 oracle; tests/listcheck.py is the checker (tests/test_listcheck_cpu.py
shows that it rejects broken lists), tests/device_frame.py drives the C ABI.  A failure names the list and the Gaussian."""
import numpy as np
import pytest

from tests import device_frame as dfm
from tests import list_scenes, listcheck, util

pytestmark = pytest.mark.gpu
BASE = dfm.F | dfm.L | dfm.J
FLAG_VARIANTS = (0, dfm.F | dfm.L, BASE)
PER_GAUSSIAN = ("rect", "depth", "tiles", "mask")
MANY_PAIRS = 500_000          # above this the pair masks are checked on a seeded sample of lists, the coverage on 2 000 Gaussians


def _golden_stages(d):
    con, ev = d["im_conic"], d["im_evals"]
    return dict(ids=d["im_ids"], u=d["im_u"].astype(np.float64), v=d["im_v"].astype(np.float64),
                conic=np.stack([con[:, 0, 0], con[:, 0, 1], con[:, 1, 1]], 1).astype(np.float64), cond=ev[:, 1] / ev[:, 0],
                tile_rect=d["im_tile_rect"])


def _visible(a):
    return np.nonzero(a["rec"][:, 5] > 0)[0]          # (project_state was cleared: a row the kernel did not write has opacity 0)


def _same_records(a, b, what):
    """rec / rect / depth / tiles / mask bit for bit ("One rounding for every kernel variant").  The colour of a
    visible Gaussian that is binned nowhere is only evaluated when the colour pass runs inside the projection: left out."""
    for k in PER_GAUSSIAN:
        bad = np.nonzero(a[k].reshape(a["n"], -1).view(np.uint32) != b[k].reshape(a["n"], -1).view(np.uint32))[0]
        assert not len(bad), f"{what}: {k} of Gaussian {bad[0]} differs: {a[k][bad[0]]} / {b[k][bad[0]]}"
    ra, rb = a["rec"].view(np.uint32).copy(), b["rec"].view(np.uint32).copy()
    nowhere = a["tiles"] == 0
    ra[nowhere, 8:11] = 0
    rb[nowhere, 8:11] = 0
    bad = np.nonzero((ra != rb).any(1))[0]
    assert not len(bad), f"{what}: record of Gaussian {bad[0]} differs: {a['rec'][bad[0]]} / {b['rec'][bad[0]]}"


def _same_lists(a, b, what):
    nb = int(a["counts"].n_binned)
    for k in ("ranges", "class_bounds"):
        bad = np.nonzero((a[k] != b[k]).reshape(len(a[k]), -1).any(1))[0]
        assert not len(bad), f"{what}: {k}[{bad[0]}] differs: {a[k][bad[0]]} / {b[k][bad[0]]}"
    # `order`: lists of one bucket are appended by LDS atomics, in whatever order the waves arrive (the launch order inside a bucket
    # is immaterial) -- the sequence of buckets is what a plan fixes; that both are permutations is check 6
    ln = a["ranges"][:, 1].astype(np.int64) - a["ranges"][:, 0]
    ba, bb = listcheck.work_bucket(ln[a["order"]]), listcheck.work_bucket(ln[b["order"]])
    bad = np.nonzero(ba != bb)[0]
    assert not len(bad), f"{what}: list {b['order'][bad[0]]}: order[{bad[0]}] is of bucket {bb[bad[0]]}, not {ba[bad[0]]}"
    for k in ("sorted_ids", "pair_mask"):
        bad = np.nonzero(a[k][:nb] != b[k][:nb])[0]
        if len(bad):
            l_ = int(np.nonzero((a["ranges"][:, 0] <= bad[0]) & (a["ranges"][:, 1] > bad[0]))[0][0])
            raise AssertionError(f"{what}: list {l_}: {k} at position {bad[0]} differs: {a[k][bad[0]]} / {b[k][bad[0]]}")


def _check_frame(s, o, a, fr, seed=0):
    """Checks 1 - 9 of tests/listcheck.py on one frame's arrays `a`; o = the float64 stages."""
    c = a["counts"]
    nb = int(c.n_binned)
    assert c.n_visible == len(o["ids"]) or s.get("knife_edge_ok"), (c.n_visible, len(o["ids"]))
    assert c.max_tiles_per_gaussian == int(a["tiles"].max(initial=0))
    p = listcheck.check_lists(a["n"], a["rect"], a["depth"], a["tiles"], a["mask"], a["ranges"], a["sorted_ids"], a["order"], a["class_bounds"],
                              nb, a["lists_x"], a["lists_y"])
    kw = s["kwargs"]
    chi, T = kw.get("chi_square_clip", 6.25), int(kw.get("T", 16))
    rng = np.random.default_rng(seed)
    big = nb > MANY_PAIRS
    sample = np.sort(rng.choice(len(o["ids"]), 2000, replace=False)) if big and len(o["ids"]) > 2000 else None
    n_px = listcheck.check_coverage(p, a["n"], o["ids"], o["u"], o["v"], o["conic"], o["tile_rect"], chi, T, s["H"], s["W"], a["lists_x"], sample=sample)
    full = np.nonzero(p.len > 0)[0]
    only = np.sort(rng.choice(full, 150, replace=False)) if big and len(full) > 150 else None
    written = listcheck.written_pairs(p, a["rec"], a["ranges"], s["H"], s["W"], a["lists_x"], chi, kw.get("alpha_max", 0.99),
                                      kw.get("alpha_cutoff", 1 / 128.), len(a["sorted_ids"]), only_lists=only)
    n_low, n_up = listcheck.check_pair_masks(p, a["pair_mask"], written, a["n"], o["ids"], o["u"], o["v"], o["conic"], o["cond"], chi, s["H"], s["W"],
                                             a["lists_x"], util.K_CAL, only_lists=only)
    print(f"{nb} pairs in {len(full)} lists (longest {int(p.len.max())}); coverage: {n_px} pixels of {len(o['ids']) if sample is None else len(sample)} "
          f"Gaussians; masks: {n_low} pairs")
    assert n_px > 0 and n_low > 0
    return p


def _variants(s, o, records=None):
    """The base frame checked in full; then the other projection flags (records bit-identical, same counters, same lists) and the
    larger pair capacities (same lists: the split kernels take their grids from the capacity)."""
    fr = dfm.Frame(s)
    c = fr.project(BASE)
    nb = int(c.n_binned)
    assert nb > 0
    fr.bin(nb)
    fr.rasterize()
    assert fr.canaries_intact()
    base = fr.arrays()
    assert dfm.counts_tuple(base["counts"]) == dfm.counts_tuple(c), "device copy of the counters / what the host received"
    if records is not None:
        records(base)
    _check_frame(s, o, base, fr)
    for flags in FLAG_VARIANTS[:2]:
        other = dfm.Frame(s)
        c2 = other.project(flags)
        assert dfm.counts_tuple(c2) == dfm.counts_tuple(c), (flags, dfm.counts_tuple(c2), dfm.counts_tuple(c))
        other.bin(nb)
        other.rasterize()
        assert other.canaries_intact()
        b = other.arrays()
        _same_records(base, b, f"projection flags {flags} / {BASE}")
        _same_lists(base, b, f"projection flags {flags} / {BASE}")
        assert bool((other.image == fr.image).all())
    for cap in (nb + 1, int(np.ceil(1.25 * nb))):
        assert dfm.counts_tuple(fr.project(BASE)) == dfm.counts_tuple(c)
        fr.bin(cap)
        fr.rasterize()
        assert fr.canaries_intact()
        _same_lists(base, fr.arrays(), f"pair_capacity {cap} / {nb}")
    return base


@pytest.mark.parametrize("name", util.RENDER_CASES)
def test_goldens_records_lists_and_masks(name):
    """Every render golden with its own kwargs: the float assertions of test_forward_records_vs_reference_intermediates on the DEVICE
    records (the same helper, the same bounds), then the lists, the plan and the pair masks, for three sets of projection flags and
    three pair capacities."""
    d = util.load(name)
    s = list_scenes.golden(name)

    def records(a):
        r = a["rec"]
        listcheck.check_records(d, r[:, 0:4], r[:, 4:8], r[:, 8:12], a["tiles"], _visible(a), a["rect"], a["tiles"], a["mask"])
        assert np.array_equal(a["depth"][d["im_ids"]], r[d["im_ids"], 11])

    _variants(s, _golden_stages(d), records)


@pytest.mark.parametrize("n,longest,hw", [(6000, 4096, (32, 48)), (11000, 8192, (32, 48)), (6000, 4096, (512, 640))])
def test_hot_spot_lists_of_every_sort_class(n, longest, hw):
    """The scenes of test_long_lists_take_the_large_sort_paths: a list of 4096+ entries (largest LDS class), of 8192+ (global-memory
    path), and the long list in a large empty image (no launch for the 4096+ class: the next class takes it)."""
    s = list_scenes.hot_spot(n, hw)
    a = _variants(s, list_scenes.oracle_stages(s))
    ln = a["ranges"][:, 1] - a["ranges"][:, 0]
    assert ln.max() > longest and a["class_bounds"][0] >= 1


def test_equal_depths_lists_are_in_index_order():
    """test_equal_depths_are_ordered_by_index's scene (the dense-bucket fallback of the list sort): every list ascends in the index."""
    s = list_scenes.equal_depths()
    a = _variants(s, list_scenes.oracle_stages(s))
    assert len(np.unique(a["depth"][a["tiles"] > 0])) == 1
    for l_ in np.nonzero(a["ranges"][:, 1] > a["ranges"][:, 0])[0]:
        ids = a["sorted_ids"][a["ranges"][l_, 0]:a["ranges"][l_, 1]].astype(np.int64)
        assert np.all(np.diff(ids) > 0), f"list {l_}: not in index order"
    assert (a["ranges"][:, 1] - a["ranges"][:, 0]).max() > 1000


@pytest.mark.parametrize("which", ["huge", "config6"])
def test_large_gaussians_lists(which):
    """Rectangles of more than 32 lists (binned row span by row span): test_huge_gaussians_cover_many_lists' scene and config 6."""
    s = list_scenes.huge_gaussians() if which == "huge" else list_scenes.config(6)
    a = _variants(s, list_scenes.oracle_stages(s))
    x0, y0, x1, y1 = listcheck.unpack_rect(a["rect"])
    assert ((a["tiles"] > 0) & ((x1 - x0 + 1) * (y1 - y0 + 1) > 32)).sum() >= 40


@pytest.mark.parametrize("cfg", [2, 3])
def test_full_size_configs_lists(cfg):
    """BASELINE.json configs 2 and 3 at full size: every integer check on every pair; coverage and pair masks on seeded samples."""
    s = list_scenes.config(cfg)
    s["knife_edge_ok"] = True             # (a knife-edge cull may differ between fp32 and float64 among 10^6 Gaussians: counted elsewhere)
    o = list_scenes.oracle_stages(s)
    fr = dfm.Frame(s)
    c = fr.project(BASE)
    assert abs(c.n_visible - len(o["ids"])) <= 1e-5 * len(o["ids"]) + 1
    fr.bin(int(c.n_binned))
    fr.rasterize()
    assert fr.canaries_intact()
    a = fr.arrays()
    vis = np.zeros(a["n"], bool)
    vis[_visible(a)] = True
    keep = vis[o["ids"]]                  # the float64 stages of the Gaussians the device kept, too
    o = {k: v[keep] for k, v in o.items()}
    _check_frame(s, o, a, fr)


@pytest.mark.parametrize("which", ["g1_generic", "huge"])
def test_too_small_pair_capacity_stays_inside_the_buffers(which):
    """The contract of gsplat_bin for a frame with more pairs than pair_capacity: nothing is written out of bounds (a canary behind
    bin_state and one behind the bin scratch, each inside the test's own allocation, are unchanged), every range stays inside
    [0, capacity], and the counters report n_binned > capacity."""
    s = list_scenes.golden(which) if which != "huge" else list_scenes.huge_gaussians()
    fr = dfm.Frame(s)
    nb = int(fr.project(BASE).n_binned)
    for cap in (nb - 1, nb // 2, 1):
        assert int(fr.project(BASE).n_binned) == nb
        fr.bin(cap)
        assert fr.canaries_intact(), f"pair_capacity {cap}: a canary behind bin_state / the bin scratch was overwritten"
        a = fr.arrays()
        assert int(a["counts"].n_binned) == nb > cap
        bad = np.nonzero((a["ranges"][:, 0] > a["ranges"][:, 1]) | (a["ranges"][:, 1] > cap))[0]
        assert not len(bad), f"list {bad[0]}: range {a['ranges'][bad[0]]} leaves [0, {cap}]"
