"""tests/absgrad_oracle.py checked on the CPU: its signed twins are the moments of tests/raster_oracle.py, the
absolute sums dominate them, both agree where a Gaussian weights a single pixel, and a hand-made frame whose per-pixel centre
gradients cancel keeps its absolute sums."""
import numpy as np
import pytest

from tests import absgrad_oracle as ao
from tests import list_scenes
from tests import raster_oracle as ro
from tests.cpu_frame import cpu_state, hm  # noqa: F401  (hm is a fixture)

SCENES = ("g1_generic", "stacked", "clamps")
_CACHE = {}


def _scene(hm, name):
    if name not in _CACHE:
        s = list_scenes.raster_scene(name)
        st = cpu_state(hm, s)
        th = list_scenes.thresholds(s, as_float32=True)
        gi = list_scenes.upstream(s)[0]
        ref = ro.composite(st["rec"], st["ranges"], st["sorted_ids"], st["lists_x"], s["H"], s["W"], *th, g_img=gi)
        ab = ao.absgrad(ref, st["rec"], g_img=gi, chi=th[0], alpha_max=th[1], alpha_cutoff=th[2])
        _CACHE[name] = (s, st, ref, ab)
    return _CACHE[name]


@pytest.mark.parametrize("name", SCENES)
def test_signed_twins_are_the_moments(hm, name):
    s, st, ref, ab = _scene(hm, name)
    rec = st["rec"].astype(np.float64)
    a11, a12, a22 = rec[:, 2], rec[:, 3], rec[:, 4]
    want = np.stack([a11 * ref.rows[:, 0] + a12 * ref.rows[:, 1], a12 * ref.rows[:, 0] + a22 * ref.rows[:, 1]], 1)
    err = np.abs(ab.signed - want)
    seen = ab.scale > 0
    assert seen.any() and not err[~seen].any()
    rel = float((err[seen] / ab.scale[seen]).max())
    print(f"{name}: signed twins against the moments: max |delta| / scale {rel:.2e}; {int(seen[:, 0].sum())} Gaussians with a term")
    assert rel <= 1e-12
    assert np.array_equal(ab.in_list, ref.in_list) and not ab.S[~ab.in_list].any()


@pytest.mark.parametrize("name", SCENES)
def test_absolute_sums_dominate_the_signed_ones(hm, name):
    s, st, ref, ab = _scene(hm, name)
    assert (np.abs(ab.signed) <= ab.S * (1 + 1e-12) + 1e-300).all()
    assert (ab.S <= ab.scale * (1 + 1e-12)).all(), "the absolute terms of a bound S"
    assert (ab.S[:, 0] > 2 * np.abs(ab.signed[:, 0])).any(), "no Gaussian of the scene shows any cancellation"
    assert (ab.allow >= 0).all()


def test_a_gaussian_that_weights_one_pixel_has_equal_sums():
    """One small Gaussian between pixel centres, so tight that the chi-square clip leaves it a single pixel."""
    rec = np.zeros((1, 16))
    rec[0, :8] = (5.2, 3.1, 30.0, 1.0, 30.0, 0.6, 1.0, 1.0)
    rec[0, 8:11] = (0.2, 0.7, 0.4)
    H, W, th = 8, 16, (6.25, 0.99, 1 / 128.0)
    gi = np.random.default_rng(2).normal(0, 1, (H, W, 3))
    ref = ro.composite(rec, np.array([[0, 1]]), np.array([0]), 1, H, W, *th, g_img=gi)
    assert int((ref.dec["q"][0] & ref.dec["cut"][0]).sum()) == 1, "the Gaussian must weight exactly one pixel"
    ab = ao.absgrad(ref, rec, g_img=gi, chi=th[0], alpha_max=th[1], alpha_cutoff=th[2])
    assert (ab.S > 0).all() and np.array_equal(ab.S, np.abs(ab.signed))


def test_cancellation_frame():
    rec, ranges, ids, lists_x, H, W, th, gi = ao.cancellation_frame()
    ref = ro.composite(rec, ranges, ids, lists_x, H, W, *th, g_img=gi)
    ab = ao.absgrad(ref, rec, g_img=gi, chi=th[0], alpha_max=th[1], alpha_cutoff=th[2])
    assert (ab.S > 0).all()
    print(f"cancellation frame: S = {ab.S[0]}, signed = {ab.signed[0]}")
    assert (np.abs(ab.signed) < 1e-12 * ab.S).all()
    # and the moments of the raster oracle say the same: the signed statistic of §14 sees nothing here
    assert abs(ref.rows[0, 0]) < 1e-12 * ref.scale[0, 0] and abs(ref.rows[0, 1]) < 1e-12 * ref.scale[0, 1]
