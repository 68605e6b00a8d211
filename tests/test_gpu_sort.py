"""The per-list depth sort (K4, csrc/gs_sort.h sort_list) and the launch plan (K5) on the DEVICE, at their edges: every instantiation
of sort_list on every path it has (A: distribution sort in LDS, B: bitonic network in LDS, C: bitonic network in global memory), at the
boundaries of the size classes, at the DENSE_BUCKET threshold, at the transitions of the bucket shift, with the bitonic padding at
2^k - 1 / 2^k / 2^k + 1, in the second grid-stride pass of every launch, and the plan in several rounds and by itself.

tests/sort_scenes.py builds the frames (chosen lengths and depth bits in chosen lists) and models the path choice;
tests/test_sort_scenes_cpu.py shows without a GPU that every frame is what it is meant to be.  Here every frame is projected and
binned through the C ABI (no rasterising) and the device's lists are compared exactly: every comparison is of integers."""
import numpy as np
import pytest

from tests import device_frame as dfm
from tests import listcheck
from tests import sort_scenes as ss

pytestmark = pytest.mark.gpu
BASE = dfm.F | dfm.L | dfm.J


def _project_and_bin(f, n_binned):
    c = f.project(BASE)
    assert int(c.n_binned) == n_binned, (int(c.n_binned), n_binned)
    f.bin(n_binned)
    assert f.canaries_intact()
    return f.arrays()


def _where(fr, list_no):
    k = int(np.searchsorted(fr.lists, list_no))
    return fr.describe(k) if k < len(fr.lists) and fr.lists[k] == list_no else f"frame {fr.name}, list {list_no} (meant to be empty)"


@pytest.mark.parametrize("name", ss.FRAMES)
def test_lists_are_sorted_on_every_path(name):
    fr = ss.frame(name)
    s = fr.scene
    f = dfm.Frame(s)
    a = _project_and_bin(f, fr.n_binned)
    # the lists have the intended lengths
    ln = a["ranges"][:, 1].astype(np.int64) - a["ranges"][:, 0]
    want = np.zeros(fr.n_lists, np.int64)
    want[fr.lists] = fr.length
    bad = np.nonzero(ln != want)[0]
    assert not len(bad), f"{_where(fr, bad[0])}: the device's list holds {ln[bad[0]]} entries"
    # the exact checker: members, strict (depth bits, index) order, class bounds, launch order
    p = listcheck.check_lists(a["n"], a["rect"], a["depth"], a["tiles"], a["mask"], a["ranges"], a["sorted_ids"], a["order"], a["class_bounds"],
                              fr.n_binned, a["lists_x"], a["lists_y"])
    # ... and the one possible answer, entry by entry
    bits = a["depth"].view(np.uint32)
    ids = np.arange(a["n"])
    expect = np.lexsort((ids, bits, s["list_of"]))                 # by list, then (depth bits, index)
    bad = np.nonzero(p.id != expect)[0]
    if len(bad):
        k = bad[0]
        raise AssertionError(f"{_where(fr, p.list[k])}: entry {p.rank[k]} is Gaussian {p.id[k]}, np.lexsort((id, depth_bits)) puts {expect[k]} there")
    # the device's own depths send every list down the intended path
    assert np.array_equal(bits, s["pos"][:, 2].view(np.uint32)), "the device depth is not pos.z bit for bit"
    lists, n, inst, path, shift = ss.sort_paths(p.list, bits[p.id], ss.class0_rule(fr.n_binned, fr.n_lists))
    assert np.array_equal(lists, fr.lists)
    for what, have, intended in (("instantiation", inst, fr.inst), ("path", path, fr.path)):
        bad = np.nonzero(have != intended)[0]
        assert not len(bad), f"{fr.describe(bad[0])}: {what} {have[bad[0]]} with the device's depths"
    bad = np.nonzero((fr.shift >= 0) & (shift != fr.shift))[0]
    assert not len(bad), f"{fr.describe(bad[0])}: shift {shift[bad[0]]} with the device's depths"
    # a second projection and binning: the scatter's arrival order differs, the result must not
    b = _project_and_bin(f, fr.n_binned)
    for k in ("ranges", "class_bounds"):
        assert np.array_equal(a[k], b[k]), f"frame {fr.name}: {k} differs between two runs"
    bad = np.nonzero(a["sorted_ids"][:fr.n_binned] != b["sorted_ids"][:fr.n_binned])[0]
    if len(bad):
        l_ = int(np.nonzero((a["ranges"][:, 0] <= bad[0]) & (a["ranges"][:, 1] > bad[0]))[0][0])
        raise AssertionError(f"{_where(fr, l_)}: sorted_ids at position {bad[0]} differs between two runs: {a['sorted_ids'][bad[0]]} / {b['sorted_ids'][bad[0]]}")
    print(fr.summary())


@pytest.mark.parametrize("hw", ss.EMPTY_IMAGES)
def test_plan_of_a_frame_with_nothing_binned(hw):
    """Every Gaussian behind the camera: gsplat_bin(0) launches plan_kernel alone (one round of plan_body, and more than one)."""
    s = ss.empty(hw)
    f = dfm.Frame(s)
    a = _project_and_bin(f, 0)
    nl = a["lists_x"] * a["lists_y"]
    assert np.all(a["tiles"] == 0)
    bad = np.nonzero(a["ranges"].any(1))[0]
    assert not len(bad), f"list {bad[0]}: range {a['ranges'][bad[0]]} in a frame with nothing binned"
    assert np.all(a["class_bounds"][:4] == 0), a["class_bounds"]
    assert len(a["order"]) == nl and np.array_equal(np.sort(a["order"]), np.arange(nl)), "`order` is not a permutation of the lists"
    listcheck.check_plan(a["ranges"], a["order"], a["class_bounds"])
