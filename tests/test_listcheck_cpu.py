"""tests/listcheck.py checked on the CPU: a consistent set of records, lists, launch plan and pair masks is built without a GPU
(records from the host build of the projection, lists in numpy from its rectangles / masks / row spans, masks from a float64
restatement of the exact sub-tile test), the checker accepts it, and rejects each of eight ways of breaking it by naming the right
list.  This is what shows that tests/test_gpu_lists.py can fail."""
import numpy as np
import pytest

from tests import list_scenes, listcheck, util
from tests.cpu_frame import cpu_state, hm  # noqa: F401  (hm is a fixture)


def run_checker(st, s, o):
    p = listcheck.check_lists(st["n"], st["rect"], st["depth"], st["tiles"], st["mask"], st["ranges"], st["sorted_ids"], st["order"],
                              st["class_bounds"], st["n_binned"], st["lists_x"], st["lists_y"])
    T = int(s["kwargs"].get("T", 16))
    listcheck.check_coverage(p, st["n"], o["ids"], o["u"], o["v"], o["conic"], o["tile_rect"], st["chi"], T, s["H"], s["W"], st["lists_x"])
    listcheck.check_pair_masks(p, st["pair_mask"], np.ones(len(st["sorted_ids"]), bool), st["n"], o["ids"], o["u"], o["v"], o["conic"], o["cond"],
                               st["chi"], s["H"], s["W"], st["lists_x"], util.K_CAL)
    return p


CONTROL_CASES = ["g1_generic", "g6_huge", "g12_kwargs"]


@pytest.fixture(scope="module", params=CONTROL_CASES)
def consistent(hm, request):
    s = list_scenes.golden(request.param)
    return s, cpu_state(hm, s), list_scenes.oracle_stages(s)


def test_checker_accepts_a_consistent_set(consistent):
    s, st, o = consistent
    p = run_checker(st, s, o)
    assert len(p.id) == st["n_binned"] > 0


def _broken(st, **changed):
    out = dict(st)
    out.update({k: v.copy() for k, v in st.items() if isinstance(v, np.ndarray)})
    out.update(changed)
    return out


def _a_list(st, min_len=3):
    """A list with at least min_len entries, not the first in memory (so that its neighbours exist)."""
    ln = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    ls = np.nonzero((ln >= min_len) & (st["ranges"][:, 0] > 0))[0]
    return int(ls[len(ls) // 2])


def _rejects(st, s, o, list_no):
    with pytest.raises(listcheck.ListError, match=rf"^list {list_no}\b"):
        run_checker(st, s, o)


def test_checker_rejects_a_dropped_pair(consistent):
    s, st, o = consistent
    L = _a_list(st)
    a, b = st["ranges"][L]
    ids = np.delete(st["sorted_ids"], a + 1)
    rg = st["ranges"].astype(np.int64)
    rg[rg[:, 0] > a] -= 1
    rg[L, 1] -= 1
    gone = int(st["sorted_ids"][a + 1])
    tiles = st["tiles"].copy()
    tiles[gone] -= 1                      # a list that misses a pair the mask asks for: every count agrees, only the mask says so
    bad = _broken(st, sorted_ids=ids, ranges=rg.astype(np.uint32), tiles=tiles, n_binned=st["n_binned"] - 1, pair_mask=np.delete(st["pair_mask"], a + 1))
    with pytest.raises(listcheck.ListError, match=rf"^list {L} lacks Gaussian {gone}\b|^list \d+: Gaussian {gone} is in"):
        run_checker(bad, s, o)


def test_checker_rejects_a_duplicated_pair(consistent):
    s, st, o = consistent
    L = _a_list(st)
    a, b = st["ranges"][L]
    ids = np.insert(st["sorted_ids"], a + 1, st["sorted_ids"][a + 1])
    rg = st["ranges"].astype(np.int64)
    rg[rg[:, 0] > a] += 1
    rg[L, 1] += 1
    tiles = st["tiles"].copy()
    tiles[st["sorted_ids"][a + 1]] += 1
    bad = _broken(st, sorted_ids=ids, ranges=rg.astype(np.uint32), tiles=tiles, n_binned=st["n_binned"] + 1,
                  pair_mask=np.insert(st["pair_mask"], a + 1, st["pair_mask"][a + 1]))
    _rejects(bad, s, o, L)


def test_checker_rejects_a_pair_outside_its_rectangle(consistent):
    s, st, o = consistent
    x0, y0, x1, y1 = listcheck.unpack_rect(st["rect"])
    p = listcheck.Pairs(st["ranges"], st["sorted_ids"], len(st["ranges"]))
    # move one pair of a Gaussian whose rectangle ends before the last column to the list right of its rectangle (same row)
    k = int(np.nonzero((x1[p.id] < st["lists_x"] - 1) & (p.list % st["lists_x"] == x1[p.id]))[0][0])
    gid, src = int(p.id[k]), int(p.list[k])
    dst = src + 1
    pl = p.list.copy()
    pl[k] = dst
    order_ = np.lexsort((p.id, st["depth"].view(np.uint32)[p.id], pl))
    ln = np.bincount(pl, minlength=len(st["ranges"]))
    end = np.cumsum(ln)
    rg = np.stack([end - ln, end], 1).astype(np.uint32)
    bad = _broken(st, sorted_ids=p.id[order_].astype(np.uint32), ranges=rg, pair_mask=st["pair_mask"][order_],
                  order=np.argsort(-listcheck.work_bucket(ln), kind="stable").astype(np.uint32))
    bad["class_bounds"][:4] = [(ln >= m).sum() for m in listcheck.CLASS_MIN_LEN]
    with pytest.raises(listcheck.ListError, match=rf"^list {dst} = .*holds Gaussian {gid}\b"):
        run_checker(bad, s, o)


def test_checker_rejects_swapped_neighbours(consistent):
    s, st, o = consistent
    L = _a_list(st)
    a = int(st["ranges"][L, 0])
    ids, pm = st["sorted_ids"].copy(), st["pair_mask"].copy()
    ids[[a, a + 1]] = ids[[a + 1, a]]
    pm[[a, a + 1]] = pm[[a + 1, a]]
    _rejects(_broken(st, sorted_ids=ids, pair_mask=pm), s, o, L)


def test_checker_rejects_equal_depths_in_descending_index_order(consistent):
    s, st, o = consistent
    L = _a_list(st)
    a = int(st["ranges"][L, 0])
    i, j = sorted(int(x) for x in st["sorted_ids"][a:a + 2])
    depth = st["depth"].copy()
    depth[[i, j]] = depth[i]                     # a tie: the order must then be the index
    # (only list L is looked at: the tie may have broken the order of other lists that hold both Gaussians)
    for first, second, fine in ((i, j, True), (j, i, False)):
        ids = st["sorted_ids"].copy()
        ids[a], ids[a + 1] = first, second
        p = listcheck.Pairs(st["ranges"][L:L + 1], ids, 1)
        p.list[:] = L
        if fine:
            listcheck.check_pairs_order(p, depth)
        else:
            with pytest.raises(listcheck.ListError, match=rf"^list {L}: entries 0 and 1 \(Gaussians {j}, {i};"):
                listcheck.check_pairs_order(p, depth)


def test_checker_rejects_a_repeated_order_entry(consistent):
    s, st, o = consistent
    order = st["order"].copy()
    order[1] = order[0]
    _rejects(_broken(st, order=order), s, o, int(order[0]))


def test_checker_rejects_a_cleared_mask_bit(consistent):
    s, st, o = consistent
    p = listcheck.Pairs(st["ranges"], st["sorted_ids"], len(st["ranges"]))
    where = np.full(st["n"], -1, np.int64)
    where[o["ids"]] = np.arange(len(o["ids"]))
    k = where[p.id]
    need = listcheck.needed_bits(o["u"][k], o["v"][k], o["conic"][k, 0], o["conic"][k, 1], o["conic"][k, 2], (p.list % st["lists_x"]) * 16,
                                 (p.list // st["lists_x"]) * 8, st["chi"], s["H"], s["W"])
    j = int(np.nonzero(need)[0][len(np.nonzero(need)[0]) // 2])
    bit = int(np.nonzero([(need[j] >> t) & 1 for t in range(8)])[0][0])
    pm = st["pair_mask"].copy()
    pm[p.pos[j]] &= ~np.uint8(1 << bit)
    with pytest.raises(listcheck.ListError, match=rf"^list {p.list[j]}: the sub-tile mask .* of Gaussian {p.id[j]} lacks bit {bit}\b"):
        run_checker(_broken(st, pair_mask=pm), s, o)


def test_checker_rejects_a_shifted_range(consistent):
    s, st, o = consistent
    L = _a_list(st)
    rg = st["ranges"].copy()
    rg[L, 1] += 1                            # reaches into the list behind it
    nxt = int(np.nonzero(st["ranges"][:, 0] == st["ranges"][L, 1])[0][np.nonzero(st["ranges"][np.nonzero(st["ranges"][:, 0] == st["ranges"][L, 1])[0], 1]
                                                                                 > st["ranges"][L, 1])[0][0]])
    _rejects(_broken(st, ranges=rg), s, o, nxt)
    rg = st["ranges"].copy()
    rg[L, 0] += 1                            # leaves one pair to nobody
    _rejects(_broken(st, ranges=rg), s, o, L)


def test_scene_caps_and_the_float32_margin_of_the_pair_mask_upper_bound(hm):
    """Two figures the GPU test relies on, from the oracle alone: (a) at most 1 % of the pairs of every scene belong to Gaussians with a
    2-D condition number above 1e4 (they are left out of check 9); (b) the largest relative excess of the float64 sub-tile minimum
    of q over chi_pad among the candidates the oracle's OWN float32 evaluation (stages and minimum in float32) calls touched:
    listcheck.PAIR_MASK_EXCESS_F32 is that figure.  Candidates: the pairs of the CPU-built lists."""
    import torch
    scene_list = [(n, list_scenes.golden(n)) for n in util.RENDER_CASES]
    scene_list += [("hot4096", list_scenes.hot_spot(6000, (32, 48))), ("hot8192", list_scenes.hot_spot(11000, (32, 48))),
                   ("hot4096 in 512 x 640", list_scenes.hot_spot(6000, (512, 640))), ("equal", list_scenes.equal_depths()),
                   ("huge", list_scenes.huge_gaussians()), ("config 6", list_scenes.config(6))]
    worst = 0.0
    for name, s in scene_list:
        st = cpu_state(hm, s)
        o64, o32 = list_scenes.oracle_stages(s), list_scenes.oracle_stages(s, torch.float32)
        p = listcheck.Pairs(st["ranges"], st["sorted_ids"], len(st["ranges"]))
        w64, w32 = np.full(st["n"], -1, np.int64), np.full(st["n"], -1, np.int64)
        w64[o64["ids"]] = np.arange(len(o64["ids"]))
        w32[o32["ids"]] = np.arange(len(o32["ids"]))
        k64, k32 = w64[p.id], w32[p.id]
        both = (k64 >= 0) & (k32 >= 0)
        ill = both & (o64["cond"][np.maximum(k64, 0)] > listcheck.COND_CAP)
        assert ill.sum() <= 0.01 * len(p.id), (name, int(ill.sum()), len(p.id))
        use = both & ~ill
        k64, k32 = k64[use], k32[use]
        ox, oy = (p.list[use] % st["lists_x"]) * 16, (p.list[use] // st["lists_x"]) * 8
        c64, c32 = o64["conic"][k64], o32["conic"][k32]
        q64 = listcheck.min_q_subtiles(o64["u"][k64], o64["v"][k64], c64[:, 0], c64[:, 1], c64[:, 2], ox, oy)
        q32 = listcheck.min_q_subtiles(o32["u"][k32], o32["v"][k32], c32[:, 0], c32[:, 1], c32[:, 2], ox, oy, dtype=np.float32)
        chi_pad = st["chi"] * 1.001 + 1e-4
        pd = (c64[:, 0] > 0) & (c64[:, 2] > 0) & (c64[:, 0] * c64[:, 2] - c64[:, 1] ** 2 > 0)
        # a candidate the float32 evaluation puts AT chi_pad has its float64 minimum at chi_pad q64 / q32: the excess.  Taken over
        # the candidates whose minimum lies within a factor two of chi_pad (the few that happen to sit within 1e-4 of it are too
        # thin a sample; the relative error of q is what moves the decision, and it is the same at 0.5 and 2 chi_pad)
        near = (q64 >= 0.5 * chi_pad) & (q64 <= 2 * chi_pad) & pd[:, None]
        ex = float((q64[near] / q32[near].astype(np.float64) - 1).max()) if near.any() else 0.0
        print(f"{name}: {len(p.id)} pairs, {int(ill.sum())} above cond 1e4; float32-oracle excess over chi_pad {ex:.3e}")
        worst = max(worst, ex)
    print(f"largest float32-oracle excess {worst:.3e}; listcheck.PAIR_MASK_EXCESS_F32 = {listcheck.PAIR_MASK_EXCESS_F32}")
    assert 0.5 * worst <= listcheck.PAIR_MASK_EXCESS_F32 <= 1.05 * worst, "the constant is no longer the measured figure"
