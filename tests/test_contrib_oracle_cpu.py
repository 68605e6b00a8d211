"""tests/contrib_oracle.py checked on the CPU, on cpu_state() of every scene of tests/test_gpu_contrib.py: (a) its weight_sum and sum
allowance are column 9 of raster_oracle.composite under g_depth = 1, its total is the sum of the oracle's opacity map, and the simple
bounds hold; (b) the band touches few Gaussians and leaves enough of them compared exactly; (c) check() accepts the float32 mode under
its own calibration (printed: the GPU test multiplies it by 3) and rejects seven restated kernel faults by naming the Gaussian and the
word."""
import functools

import numpy as np
import pytest

from tests import contrib_oracle as co
from tests import list_scenes
from tests import raster_oracle as ro
from tests.cpu_frame import cpu_state, hm  # noqa: F401  (hm is a fixture)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return list_scenes.raster_scene(name)


_STATES, _REFS = {}, {}


def _args(st, s):
    return (st["rec"], st["ranges"], st["sorted_ids"], st["lists_x"], s["H"], s["W"]) + list_scenes.thresholds(s, as_float32=True)


def _setup(hm, name):
    """(s, st, ref, f32, K) of a consistent set: float64 reference, the float32 mode's record, K = 3 x its ratios."""
    if name not in _REFS:
        s = _scene(name)
        st = _STATES.setdefault(name, cpu_state(hm, s))
        ref = co.contribution(*_args(st, s))
        f32 = co.contribution_f32(*_args(st, s))
        r = co.ratios(f32["record"], ref)
        _REFS[name] = (s, st, ref, f32, {k: 3.0 * v for k, v in r.items()}, r)
    return _REFS[name][:5]


def _rebuilt(f32, st, **changed):
    a = dict(f32, **changed)
    return co.record_from_pairs(a["sub_sum"], a["sub_max"], a["sub_cnt"], st["ranges"], st["sorted_ids"], st["n"])


def _rejects(record, ref, K, pattern, **kw):
    with pytest.raises(co.ContribError, match=pattern) as e:
        co.check(record, ref, K, "broken", **kw)
    print(e.value)


def _exact_pairs(ref, f32):
    """Positions in sorted_ids of the pairs with a pixel whose Gaussian has no allowance at all."""
    ok = (ref.gauss >= 0) & (f32["sub_cnt"].sum(1) > 0)
    ok[ok] &= ~ref.any_allowance[ref.gauss[ok]]
    return np.nonzero(ok)[0]


# ---- (a), (b): pinned to raster_oracle; the band ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list_scenes.RASTER_SCENES)
def test_oracle_against_the_raster_oracle_and_float32_calibration(hm, name):
    s, st, ref, f32, K = _setup(hm, name)
    comp = ro.composite(*_args(st, s), aux=True, g_depth=np.ones((s["H"], s["W"])))
    assert np.allclose(ref.weight_sum, comp.rows[:, 9], rtol=1e-12, atol=0.0)
    assert np.allclose(ref.allow_sum, comp.allow[:, 9], rtol=1e-12, atol=0.0)
    assert abs(ref.weight_sum.sum() - comp.alpha.sum()) <= 1e-12 * comp.alpha.sum()
    rec = st["rec"].astype(np.float64)
    amax = list_scenes.thresholds(s, as_float32=True)[1]
    assert (ref.weight_max <= np.minimum(rec[:, 5], amax)).all()
    assert (ref.pixels <= 128 * ref.pairs).all() and (ref.pixels[~ref.in_list] == 0).all()
    assert np.array_equal(ref.in_list, ref.pairs > 0)
    listed = int(ref.in_list.sum())
    share = float((ref.any_allowance & ref.in_list).sum()) / listed
    exact = int((~ref.any_allowance & ref.in_list).sum())
    r = co.ratios(f32["record"], ref)
    print(f"{name}: {st['n_binned']} pairs, {listed} Gaussians in lists, {ref.n_flips} flips; with an allowance {100 * share:.1f} %, compared exactly {exact}; "
          f"zero weight {int((ref.weight_max[ref.in_list] == 0).sum())}; float32 mode needs K_sum {r['sum']:.2f}, K_max {r['max']:.2f}")
    assert share <= 0.15
    assert exact >= 20
    co.check(f32["record"], ref, {k: 1.0001 * v for k, v in r.items()}, name)
    co.check(f32["record"], ref, K, name)


def test_a_second_call_adds(hm):
    s, st, ref, f32, K = _setup(hm, "g1_generic")
    twice = co.record_from_pairs(f32["sub_sum"], f32["sub_max"], f32["sub_cnt"], st["ranges"], st["sorted_ids"], st["n"], record=f32["record"])
    a, b = co.decode(f32["record"]), co.decode(twice)
    assert np.array_equal(b[0], 2 * a[0]) and np.array_equal(b[1], a[1]) and np.array_equal(b[2], 2 * a[2])
    co.check(twice, ref, K, "two calls", calls=2)
    _rejects(f32["record"], ref, K, r"Gaussian \d+, (weight_sum|pixels)", calls=2)          # the second call overwrote instead of adding


def test_decode_reads_words_above_32_bits():
    rec = np.array([[5, 2, 0x3F000000, -1], [0, 0, 0, 0]], np.int64).astype(np.int32)
    sum_q, wmax, pix = co.decode(rec)
    assert int(sum_q[0]) == 2 * 2 ** 32 + 5 and wmax[0] == 0.5 and int(pix[0]) == 2 ** 32 - 1
    assert np.array_equal(co.encode(sum_q, wmax, pix).view(np.int32), rec)


# ---- (c) the checker can fail ---------------------------------------------------------------------------------------------------------

def test_rejects_a_dropped_subtile_slot(hm):
    s, st, ref, f32, K = _setup(hm, "g1_generic")
    k = int(_exact_pairs(ref, f32)[7])
    t = int(np.argmax(f32["sub_cnt"][k]))
    ch = {key: f32[key].copy() for key in ("sub_sum", "sub_max", "sub_cnt")}
    for a in ch.values():
        a[k, t] = 0
    _rejects(_rebuilt(f32, st, **ch), ref, K, rf"Gaussian {st['sorted_ids'][k]}, (weight_sum|weight_max|pixels)")


def test_rejects_the_last_entry_of_a_chunk_dropped(hm):
    s, st, ref, f32, K = _setup(hm, "stacked")
    first = int(st["ranges"][0, 0])
    k = first + 63
    assert f32["sub_cnt"][k].sum() > 0, "entry 63 of the stacked list reaches pixels"
    ch = {key: f32[key].copy() for key in ("sub_sum", "sub_max", "sub_cnt")}
    for a in ch.values():
        a[k] = 0
    _rejects(_rebuilt(f32, st, **ch), ref, K, rf"Gaussian {st['sorted_ids'][k]}, (weight_sum|weight_max|pixels).*entry 63 \(position 63 of chunk 0\)")


def test_rejects_a_pixel_column_right_of_a_ragged_image(hm):
    s, st, ref, f32, K = _setup(hm, "g2_ragged")
    assert s["W"] % 16 and s["H"] % 8
    bad = co.contribution_f32(*_args(st, s), ragged_bug=True)
    _rejects(bad["record"], ref, K, r"Gaussian \d+, (weight_sum|pixels)")


def test_rejects_dead_pixels_counted(hm):
    s, st, ref, f32, K = _setup(hm, "g3_occlusion")
    bad = co.contribution_f32(*_args(st, s), count_dead=True)
    assert np.array_equal(co.decode(bad["record"])[1][ref.weight_max > 0], co.decode(f32["record"])[1][ref.weight_max > 0])
    _rejects(bad["record"], ref, K, r"Gaussian \d+, pixels")


def test_rejects_the_maximum_of_a_lanes_pixel_sum(hm):
    s, st, ref, f32, K = _setup(hm, "g1_generic")
    bad = co.contribution_f32(*_args(st, s), max_of_lane_sum=True)
    assert np.array_equal(co.decode(bad["record"])[0], co.decode(f32["record"])[0])
    _rejects(bad["record"], ref, K, r"Gaussian \d+, weight_max")


def test_rejects_truncation_in_the_quantisation(hm):
    s, st, ref, f32, K = _setup(hm, "hot_spot")           # thousands of Gaussians behind each other: weights down to 1e-7, where 2^-33 shows
    bad = co.contribution_f32(*_args(st, s), truncate=True)
    _rejects(bad["record"], ref, K, r"Gaussian \d+, weight_sum")
