"""The frames of tests/test_gpu_sort.py, checked without a GPU: the host build of the projection puts every Gaussian into the one list
it was made for, at the requested depth bits; the numpy model of the sort's path choice (tests/sort_scenes.py) sends every list
down the path its pattern was made for, every (instantiation, path) pair and every transition of the bucket shift occurs, and the
many_lists_* frames hold more lists of their class than its launch has groups.  The frames of about 10^6 pairs are placed at a
reduced size (same image, same lists, shorter lists); the path model runs on the full-size depth bits of every frame."""
import numpy as np
import pytest

from tests import listcheck
from tests import sort_scenes as ss
from tests.cpu_frame import cpu_state, hm  # noqa: F401  (hm is a fixture)


@pytest.fixture(scope="module", params=ss.FRAMES)
def placed(hm, request):
    fr = ss.frame(request.param, reduced=request.param in ss.REDUCED)
    return fr, cpu_state(hm, fr.scene)


def test_every_gaussian_lands_in_its_list_at_its_depth_bits(placed):
    fr, st = placed
    s = fr.scene
    assert np.all(st["vis"] == 0), f"{fr.name}: Gaussian {np.nonzero(st['vis'])[0][:1]} is culled"
    assert np.all(st["tiles"] == 1), f"{fr.name}: Gaussian {np.nonzero(st['tiles'] != 1)[0][:1]} is not in exactly one list"
    x0, y0, x1, y1 = listcheck.unpack_rect(st["rect"])
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(y0 * st["lists_x"] + x0, s["list_of"])
    ln = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    want = np.zeros(fr.n_lists, np.int64)
    want[fr.lists] = fr.length
    assert np.array_equal(ln, want) and st["n_binned"] == fr.n_binned
    bits = st["depth"].view(np.uint32)
    assert np.array_equal(bits, s["pos"][:, 2].view(np.uint32))
    o = np.argsort(s["list_of"], kind="stable")                  # by list, then by Gaussian index: the order the patterns are given in
    assert np.array_equal(bits[o], np.concatenate([fr.depths[int(l_)] for l_ in fr.lists]).view(np.uint32))


def test_checker_accepts_the_cpu_built_lists(placed):
    fr, st = placed
    p = listcheck.check_lists(st["n"], st["rect"], st["depth"], st["tiles"], st["mask"], st["ranges"], st["sorted_ids"], st["order"],
                              st["class_bounds"], st["n_binned"], st["lists_x"], st["lists_y"])
    assert len(p.id) == fr.n_binned


def test_checker_rejects_a_swap_inside_a_full_bucket(hm):
    """Two neighbours among the 48 equal keys of a clump48 bucket, exchanged: the error a wrong rank inside a full bucket makes."""
    fr = ss.frame("small")
    st = cpu_state(hm, fr.scene)
    k = [i for i, p in enumerate(fr.pattern) if p == "clump48"][-1]
    L = int(fr.lists[k])
    a = int(st["ranges"][L, 0])
    ids = st["sorted_ids"].copy()
    assert len(np.unique(st["depth"][ids[a:a + 48]])) == 1 and st["depth"][ids[a + 48]] > st["depth"][ids[a]]
    ids[[a + 20, a + 21]] = ids[[a + 21, a + 20]]
    with pytest.raises(listcheck.ListError, match=rf"^list {L}: entries 20 and 21\b"):
        listcheck.check_lists(st["n"], st["rect"], st["depth"], st["tiles"], st["mask"], st["ranges"], ids, st["order"], st["class_bounds"],
                              st["n_binned"], st["lists_x"], st["lists_y"])


@pytest.fixture(scope="module")
def modelled():
    """frame name -> (frame, the model's (lists, length, inst, path, shift)) on the full-size depth bits as requested."""
    out = {}
    for name in ss.FRAMES:
        fr = ss.frame(name)
        bits = np.concatenate([fr.depths[int(l_)] for l_ in fr.lists]).view(np.uint32)
        out[name] = fr, ss.sort_paths(np.repeat(fr.lists, fr.length), bits, fr.class0)
    return out


def test_every_list_takes_the_path_its_pattern_is_made_for(modelled):
    for name, (fr, (lists, n, inst, path, shift)) in modelled.items():
        assert np.array_equal(lists, fr.lists) and np.array_equal(n, fr.length)
        for what, have, want in (("instantiation", inst, fr.inst), ("path", path, fr.path)):
            bad = np.nonzero(have != want)[0]
            assert not len(bad), f"{fr.describe(bad[0])}: the model says {what} {have[bad[0]]}"
        bad = np.nonzero((fr.shift >= 0) & (shift != fr.shift))[0]
        assert not len(bad), f"{fr.describe(bad[0])}: shift {shift[bad[0]]}, intended {fr.shift[bad[0]]}"
        # the one-list restatement agrees with the vectorised one (a sample: the first list of every (pattern, instantiation))
        seen = set()
        for k in range(len(fr.lists)):
            if (fr.pattern[k], fr.inst[k]) not in seen:
                seen.add((fr.pattern[k], fr.inst[k]))
                T, E, L = ss.INST[fr.inst[k]]
                p1, s1 = ss.sort_path(fr.depths[int(fr.lists[k])].view(np.uint32), T, E, L, fr.inst[k] in ("512", "1024"))
                assert p1 == path[k] and (p1 == "C" or s1 == shift[k]), fr.describe(k)
        print(fr.summary())


def test_every_instantiation_and_path_occurs(modelled):
    have = {(i, p) for fr, (_, _, inst, path, _) in modelled.values() for i, p in zip(inst, path)}
    assert have == ss.COMBINATIONS, (ss.COMBINATIONS - have, have - ss.COMBINATIONS)
    # all three paths and all four instantiations in ONE frame
    _, (_, _, inst, path, _) = modelled["mixed"]
    assert set(inst) == set(ss.INST) and set(path) == {"A", "B", "C"}
    # path B with distinct keys, in every instantiation
    for name, want in (("small", "wave"), ("mid", "256"), ("class1", "512"), ("class0", "1024")):
        fr, (_, _, inst, path, _) = modelled[name]
        assert any(p == "two_clumps" and i == want and q == "B" for p, i, q in zip(fr.pattern, inst, path)), name


def test_every_shift_transition_and_the_bucket_threshold_occur(modelled):
    for name, cls in (("small", "wave"), ("mid", "256"), ("class1", "512"), ("class0", "1024")):
        fr, (_, n, inst, path, shift) = modelled[name]
        L = ss.INST[cls][2]
        for k, want in enumerate((0, 1, 1, 2)):
            sel = [j for j, p in enumerate(fr.pattern) if p == f"range{k}" and inst[j] == cls]
            assert sel and all(shift[j] == want and path[j] == "A" for j in sel), (name, k)
            for j in sel:                              # the range is exactly 2^L - 1, 2^L, 2^(L + 1) - 1, 2^(L + 1)
                b = fr.depths[int(fr.lists[j])].view(np.uint32).astype(np.int64)
                assert b.max() - b.min() == ((1 << L) - 1, 1 << L, (1 << (L + 1)) - 1, 1 << (L + 1))[k]
        for pat, want in (("clump48", "A"), ("clump49", "B")):
            sel = [j for j, p in enumerate(fr.pattern) if p == pat and inst[j] == cls]
            assert sel and all(path[j] == want for j in sel), (name, pat)
            for j in sel:                              # the largest bucket holds exactly 48 / 49 entries: the threshold itself
                b = fr.depths[int(fr.lists[j])].view(np.uint32).astype(np.int64)
                assert np.bincount((b - b.min()) >> shift[j]).max() == int(pat[5:]), fr.describe(j)
    fr, (_, n, _, path, shift) = modelled["small"]
    eq = {int(x): (p, s) for x, p, s, pat in zip(n, path, shift, fr.pattern) if pat == "equal"}
    assert eq[48] == ("A", 0) and eq[49] == ("B", 0) and eq[1] == ("A", 0)


def test_class_boundaries_and_padding_sizes_occur(modelled):
    n = np.concatenate([fr.length for fr, _ in modelled.values()])
    for boundary in (256, 1024, 4096, 8192):
        assert boundary - 1 in n and boundary in n and boundary + 1 in n, boundary
    # bitonic padding (path B or C) at 2^k - 1, 2^k, 2^k + 1 in LDS, and at a non-power-of-two above 8192 in global memory
    bitonic = {(int(x), p) for fr, (_, ln, _, path, _) in modelled.values() for x, p in zip(ln, path) if p != "A"}
    for x in (63, 64, 65, 511, 512, 513, 2047, 2048, 4095, 4096, 4097, 8191):
        assert (x, "B") in bitonic, x
    assert (8192, "C") in bitonic and (8193, "C") in bitonic and (12289, "C") in bitonic and (5000, "C") in bitonic


def test_launches_of_every_frame(modelled):
    """gsplat_bin's class0 rule per frame, and the second grid-stride pass of every launch in the many_lists_* frames."""
    want = dict(small=False, mid=False, class1=True, class0=True, no_class0=False, mixed=True, many_lists_4096=True, many_lists_1024=True,
                many_lists_256=False, many_lists_small=False)
    for name, (fr, (_, n, inst, _, _)) in modelled.items():
        la = ss.launches(fr.n_binned, fr.n_lists)
        assert la["class0"] == want[name] == fr.class0, name
        for cls in ss.INST:
            assert not (inst == cls).any() or la[cls] > 0, f"{name}: lists of class {cls} and no launch for them"
        if name in ss.MANY:
            cls, at_least = ss.MANY[name]
            have = int((inst == cls).sum())
            assert have >= at_least and la[cls] < have <= 2 * la[cls], f"{name}: {have} lists of class {cls}, {la[cls]} per pass"
            print(f"{name}: {have} lists sorted by sort_list<{cls}>, {la[cls]} per grid-stride pass")
    fr = modelled["no_class0"][0]
    assert set(fr.inst[fr.length >= 4096]) == {"512"}             # with_class0 = 1: the 512-thread kernel takes the long lists
    assert modelled["many_lists_small"][0].n_lists > 16384       # plan_body in several rounds
    nl = [((W + 15) // 16) * ((H + 7) // 8) for H, W in ss.EMPTY_IMAGES]
    assert nl[0] <= 16384 < nl[1]


@pytest.mark.parametrize("hw", ss.EMPTY_IMAGES)
def test_empty_frames_bin_nothing(hm, hw):
    from tests import cpu_frame
    s = ss.empty(hw)
    _, tiles, vis, _, _, _ = cpu_frame.project(hm, s, s)
    assert np.all(vis != 0) and np.all(tiles == 0)
