"""The binning front end at the sizes where its two block layouts can go wrong (tests/listcheck.py is the checker, tests/device_frame.py
drives the C ABI): the sharded coarse-bin totals -- more blocks of 2048 Gaussians than shards, a short last block, a bin whose region
holds several shards and a large part, a pair capacity below the count -- and the sort launches for the lists below 4096 entries at
the edges of their size classes: every kind of block in one frame, one kind missing, and equal depths in every kind."""
import functools

import numpy as np
import pytest

from tests import device_frame as dfm
from tests import list_scenes, listcheck

pytestmark = pytest.mark.gpu
BASE = dfm.F | dfm.L | dfm.J
BIN_GAUSS, BIN_LISTS = 2048, 64                      # csrc/gs_layout.h: Gaussians per binning block, lists per coarse bin
SIZES = (1, 2049, 9 * 2048 + 5)                      # one block | two | more blocks than shards of the bin totals, the last one short
IMAGES = ((64, 128), (136, 272))                     # (H, W): 8 x 8 = 64 lists in one bin | 17 x 17 = 289 lists, five bins, the last partial


def _up(x):
    return (x + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def _small_scene(n, hw, f=40.0):
    """n Gaussians of 1 - 2 pixels sigma spread over the image (4 pixels at the most: rectangles of up to 3 x 4 lists); Gaussian 0 sits
    on a corner of four lists, so that even n = 1 bins more than one pair.  f: the focal length (the world scales shrink with it)."""
    H, W = hw
    rng = np.random.default_rng(100 + n)
    z = rng.uniform(3.0, 6.0, n)
    uv = np.stack([rng.uniform(2, W - 2, n), rng.uniform(2, H - 2, n)], 1)
    uv[0], z[0] = (64.0, 32.0), 4.0
    pos = np.stack([(uv[:, 0] - W / 2) / f * z, (uv[:, 1] - H / 2) / f * z, z], 1)
    d = dict(pos=pos, scale_raw=np.clip(rng.normal(0, 0.2, (n, 3)), -0.8, 0.8) - 2.0 + np.log(40.0 / f), q_raw=rng.normal(0, 1, (n, 4)),
             opacity_raw=rng.normal(0, 0.3, n) - 1.0,
             f_dc=rng.normal(0, 1, (n, 3)), f_rest=rng.normal(0, 0.2, (n, 45)))
    return list_scenes._pack(d, H, W, f, f, W / 2.0, H / 2.0)


def _single_list_scene(lengths, hw=(64, 64), seed=7):
    """lengths[l] Gaussians of 0.8 pixels sigma within half a pixel of the centre of list l: each lies in exactly that list (its
    3-sigma box ends a pixel inside the 16 x 8 region)."""
    (H, W), f = hw, 40.0
    lists_x = W // listcheck.LIST_W
    rng = np.random.default_rng(seed)
    which = np.repeat(np.arange(len(lengths)), lengths)
    which = which[rng.permutation(len(which))]          # (a list's Gaussians come from every block of 2048)
    n = len(which)
    z = rng.uniform(3.9, 4.1, n)
    u = (which % lists_x) * listcheck.LIST_W + 8 + rng.uniform(-0.5, 0.5, n)
    v = (which // lists_x) * listcheck.LIST_H + 4 + rng.uniform(-0.5, 0.5, n)
    pos = np.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], 1)
    d = dict(pos=pos, scale_raw=np.full((n, 3), np.log(0.08)), q_raw=rng.normal(0, 1, (n, 4)), opacity_raw=np.full(n, -1.0),
             f_dc=rng.normal(0, 1, (n, 3)), f_rest=rng.normal(0, 0.2, (n, 45)))
    return list_scenes._pack(d, H, W, f, f, W / 2.0, H / 2.0)


def _bin_start(fr):
    """bin_start[0 .. bins] of the frame's project_state.  The layout call does not name it; it lies three parts in front of `ranges`
    (csrc/gs_layout.h carve_project: bin_start | block_off | list_count | ranges, each part a multiple of 256 bytes)."""
    nl = int(fr.lay.lists)
    nb = (nl + BIN_LISTS - 1) // BIN_LISTS
    assert fr.n < 2 * BIN_GAUSS * 1024                  # (one batch of 2048 Gaussians per block)
    blocks = (fr.n + BIN_GAUSS - 1) // BIN_GAUSS
    off = fr.lay.ranges - _up(nb * BIN_LISTS * 4) - _up(blocks * nb * 4) - _up((nb + 1) * 4)
    assert off >= fr.lay.mask + _up(fr.n * 4)
    return fr.state[off:off + (nb + 1) * 4].cpu().numpy().view(np.uint32).copy()


def _frame(s):
    fr = dfm.Frame(s)
    c = fr.project(BASE)
    nb = int(c.n_binned)
    assert nb > 0
    fr.bin(nb)
    assert fr.canaries_intact()
    return fr, fr.arrays(), nb


def _check(a, nb):
    assert int(a["counts"].n_binned) == nb
    return listcheck.check_lists(a["n"], a["rect"], a["depth"], a["tiles"], a["mask"], a["ranges"], a["sorted_ids"], a["order"], a["class_bounds"],
                                 nb, a["lists_x"], a["lists_y"])


def _areas(a):
    x0, y0, x1, y1 = listcheck.unpack_rect(a["rect"])
    return (x1 - x0 + 1) * (y1 - y0 + 1)


def _lengths(a):
    return a["ranges"][:, 1].astype(np.int64) - a["ranges"][:, 0]


@pytest.mark.parametrize("hw", IMAGES)
@pytest.mark.parametrize("n", SIZES)
def test_shards_wrap_and_blocks_differ_in_size(n, hw):
    """Small Gaussians only: the lists are complete and ordered, and the bin regions end where the counter says."""
    fr, a, nb = _frame(_small_scene(n, hw))
    binned = a["tiles"] > 0
    assert binned[0] and binned.sum() >= 0.9 * n and _areas(a)[binned].max() <= 32
    assert nb >= 2
    _check(a, nb)
    bs = _bin_start(fr)
    assert bs[0] == 0 and np.all(np.diff(bs.astype(np.int64)) >= 0) and int(bs[-1]) == nb, (bs, nb)
    # every bin's region holds exactly the pairs of its 64 lists
    ln = np.zeros((len(bs) - 1) * BIN_LISTS, np.int64)
    ln[:len(a["ranges"])] = _lengths(a)
    assert np.array_equal(np.diff(bs.astype(np.int64)), ln.reshape(-1, BIN_LISTS).sum(1))


def test_more_than_1024_bins():
    """An image beyond 4 M pixels (2176 x 4096: 69 632 lists, 1088 bins): a thread of the scatter owns five bins, and the fifth takes
    the path that loads its shards by itself."""
    fr, a, nb = _frame(_small_scene(SIZES[-1], (2176, 4096), f=4000.0))
    assert (int(fr.lay.lists) + BIN_LISTS - 1) // BIN_LISTS > 1024
    binned = a["tiles"] > 0
    assert binned.sum() >= 0.9 * a["n"] and _areas(a)[binned].max() <= 32
    _check(a, nb)
    bs = _bin_start(fr).astype(np.int64)
    ln = np.zeros((len(bs) - 1) * BIN_LISTS, np.int64)
    ln[:len(a["ranges"])] = _lengths(a)
    assert int(bs[-1]) == nb and np.array_equal(np.diff(bs), ln.reshape(-1, BIN_LISTS).sum(1))


def test_small_and_large_parts_of_one_bin():
    """list_scenes.huge_gaussians() and, in the same bins, twelve jittered copies of each of its small Gaussians: three blocks of small
    ones (three shards) and the large part in every bin's region."""
    s = dict(list_scenes.huge_gaussians())
    n0 = len(s["pos"])
    small = np.nonzero(s["scale_raw"].mean(1) < -1.0)[0]                # (the scene adds 2.3 to the log scales of the large ones, around -2.0;
    rng = np.random.default_rng(9)                                       #  which rectangles ARE large is read from the device below)
    idx = np.concatenate([np.arange(n0), np.tile(small, 12)])
    for k in list_scenes.NAMES:
        s[k] = np.ascontiguousarray(s[k][idx])
    s["pos"][n0:] += rng.normal(0, 0.02, (len(idx) - n0, 3)).astype(np.float32)
    fr, a, nb = _frame(s)
    area, binned = _areas(a), a["tiles"] > 0
    big = binned & (area > 32)
    assert big.sum() >= 40 and (binned & ~big).sum() > 2 * BIN_GAUSS and a["n"] > 2 * BIN_GAUSS
    p = _check(a, nb)
    # bins that hold pairs of large Gaussians and of small ones from every block
    bin_of = p.list // BIN_LISTS
    is_big = big[p.id]
    blocks = p.id // BIN_GAUSS
    mixed = [b for b in np.unique(bin_of) if is_big[bin_of == b].any() and len(np.unique(blocks[(bin_of == b) & ~is_big])) >= 3]
    assert len(mixed) >= 1
    assert int(_bin_start(fr)[-1]) == nb


@pytest.mark.parametrize("hw", IMAGES)
@pytest.mark.parametrize("n", SIZES)
def test_too_small_pair_capacity_on_the_sharded_regions(n, hw):
    """test_too_small_pair_capacity_stays_inside_the_buffers' contract with several shards per bin: canaries unchanged, every range
    inside [0, capacity], the counters report n_binned > capacity."""
    s = _small_scene(n, hw)
    fr = dfm.Frame(s)
    nb = int(fr.project(BASE).n_binned)
    assert nb >= 2
    for cap in sorted({nb - 1, max(nb // 2, 1), 1}, reverse=True):
        assert int(fr.project(BASE).n_binned) == nb
        fr.bin(cap)
        assert fr.canaries_intact(), f"pair_capacity {cap}: a canary behind bin_state / the bin scratch was overwritten"
        a = fr.arrays()
        assert int(a["counts"].n_binned) == nb > cap
        bad = np.nonzero((a["ranges"][:, 0] > a["ranges"][:, 1]) | (a["ranges"][:, 1] > cap))[0]
        assert not len(bad), f"list {bad[0]}: range {a['ranges'][bad[0]]} leaves [0, {cap}]"


EDGES = (1, 63, 64, 255, 256, 1023, 1024, 4095)        # either side of: one wave's slice | short / mid | mid / class 1 | class 1 / class 0
FILL = (2, 7, 100, 300, 31, 129, 511, 17)


@pytest.mark.parametrize("which,lengths", [("all_kinds", EDGES + FILL), ("no_class1", EDGES[:6] + FILL),
                                           ("no_short", (256, 1023, 1024, 4095, 300, 511, 700, 2000))])
def test_every_block_kind_in_one_frame(which, lengths):
    """Lists of exactly these lengths in one frame: class-1, mid and short blocks of the sort all have work; then a frame without a list
    of 1024 .. 4095 entries and one without a list below 256 (there the 4096+ class gets its launch, with nothing in it)."""
    s = _single_list_scene(lengths)
    fr, a, nb = _frame(s)
    ln = _lengths(a)
    assert np.array_equal(ln[:len(lengths)], np.asarray(lengths)) and not ln[len(lengths):].any(), ln
    cb = a["class_bounds"]
    want = [int((ln >= m).sum()) for m in listcheck.CLASS_MIN_LEN]
    assert list(cb[:4]) == want, (cb, want)
    if which == "no_class1":
        assert cb[1] == cb[0] == 0
    if which == "no_short":
        assert cb[3] == cb[2]
    _check(a, nb)
    listcheck.check_plan(a["ranges"], a["order"], a["class_bounds"])


def test_equal_depths_in_every_block_kind():
    """Three copies of list_scenes.equal_depths() (every Gaussian at camera depth 4), thinned from left to right to 100 % / 12 % / 6 %: a list
    of each class whose depths are all equal -- one bucket of the distribution sort holds the whole list and the bitonic network takes
    it, in a class-1 block, a mid block and a wave of a short block.  The ids come out in index order."""
    s = dict(list_scenes.equal_depths())
    u = s["pos"][:, 0] * s["fx"] / s["pos"][:, 2] + s["cx"]
    rng = np.random.default_rng(4)
    keep_p = np.where(u < 11, 1.0, np.where(u < 32, 0.12, 0.06))
    idx = np.concatenate([np.nonzero(rng.uniform(size=len(u)) < keep_p)[0] for _ in range(3)])
    for k in list_scenes.NAMES:
        s[k] = np.ascontiguousarray(s[k][idx])
    fr, a, nb = _frame(s)
    assert len(np.unique(a["depth"][a["tiles"] > 0])) == 1
    ln = _lengths(a)
    dense = 48                                            # csrc/gs_sort.h DENSE_BUCKET: a longer list of one depth takes the network
    assert ((ln >= 1024) & (ln < 4096)).any() and ((ln >= 256) & (ln < 1024)).any() and ((ln > dense) & (ln < 256)).any(), ln
    _check(a, nb)
    for l_ in np.nonzero(ln > 0)[0]:
        ids = a["sorted_ids"][a["ranges"][l_, 0]:a["ranges"][l_, 1]].astype(np.int64)
        assert np.all(np.diff(ids) > 0), f"list {l_}: not in index order"
