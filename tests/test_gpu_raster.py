"""The two raster kernels alone (raster_forward_kernel<SAVE, AUX>, raster_backward_kernel<DET, AUX>) against tests/raster_oracle.py: a
float64 composite of the records and lists THE DEVICE left (tests/device_frame.Frame through ctypes), so that the projection's fp32
rounding is not in the comparison.  Every pixel and every (Gaussian, column) is held to
    |delta| <= K 2^-24 scale + allowance,
scale = the sum of the absolute terms, allowance = what inverting the decisions within fp32's reach of their thresholds changes
(both defined in raster_oracle's docstring), K = 3 x the largest |delta| / (2^-24 scale) of the oracle's OWN float32 evaluation of the
same records, per scene and per output kind -- measured against the reference's arithmetic, never against the kernel; the factor 3 is
the project's margin over a calibration (hardware exp2 / rcp are ~1 ulp where numpy rounds correctly, and the kernel adds in another
association: 8-lane tree, slots per sub-tile, atomics or the fixed pair order).  Each check prints the device's own largest ratio
(pytest -s); DESIGN.md 8 (g) quotes them."""
import numpy as np
import pytest

from tests import device_frame as dfm
from tests import list_scenes
from tests import raster_oracle as ro

pytestmark = pytest.mark.gpu
BG = (1.0, 0.5, 0.25)
MODES = ("atomic", "deterministic", "aux atomic", "aux deterministic")
_RUNS = {}


class _Run:
    """Everything of one scene, computed once: the device's state and outputs, the two references (plain / aux) and their K."""

    def __init__(self, name):
        s = self.s = list_scenes.raster_scene(name)
        unfused = (s["color"], s["sigma"]) if "color" in s else None
        fr = self.fr = dfm.Frame(s, unfused=unfused)
        counts = fr.project(0 if unfused else dfm.F)
        assert counts.n_binned > 0
        fr.bin(counts.n_binned)
        self.intact = []
        up = list_scenes.upstream(s)
        self.fwd, self.box, self.g2d, self.g2d_zeroed = {}, {}, {}, {}
        for aux in (False, True):
            kw = dict(aux=aux, bg=BG if aux else None)
            self.box[aux] = fr.forward(accum=False, **kw)
            self.intact.append(fr.canaries_intact())
            for det in (False, True):
                mode = ("aux " if aux else "") + ("deterministic" if det else "atomic")
                self.fwd[aux] = fr.forward(accum=True, zero_grad2d=True, **kw)
                self.intact.append(fr.canaries_intact())
                bk = dict(g_img=up[0], g_depth=up[1] if aux else None, g_alpha=up[2] if aux else None, det=det, **kw)
                self.g2d_zeroed[mode] = fr.backward(zeroed=True, **bk)
                self.intact.append(fr.canaries_intact())
                self.g2d[mode] = fr.backward(zeroed=False, **bk)
                self.intact.append(fr.canaries_intact())
        a = self.arr = fr.arrays()
        self.args = (a["rec"], a["ranges"], a["sorted_ids"], a["lists_x"], s["H"], s["W"]) + list_scenes.thresholds(s, as_float32=True)
        self.ref, self.f32, self.K, self.cal = {}, {}, {}, {}
        for aux in (False, True):
            kw = dict(g_img=up[0], g_depth=up[1], g_alpha=up[2], bg=BG, aux=True) if aux else dict(g_img=up[0])
            self.ref[aux] = ro.composite(*self.args, **kw)
            self.f32[aux] = ro.composite_f32(*self.args, **kw)
            self.cal[aux] = ro.ratios(self.f32[aux], self.ref[aux])
            self.K[aux] = {k: 3.0 * self.cal[aux].get(k, 0.0) for k in ro.KINDS}


def _run(name):
    """(A failed set-up is kept and raised again: nothing runs on the device a second time.)"""
    if name not in _RUNS:
        try:
            _RUNS[name] = _Run(name)
        except Exception as e:
            _RUNS[name] = e
    if isinstance(_RUNS[name], Exception):
        raise _RUNS[name]
    return _RUNS[name]


def _report(name, what, r, run, aux):
    print(f"{name} {what}: device |delta| / (2^-24 scale) " + ", ".join(f"{k} {v:.1f}" for k, v in r.items()) + "; float32 mode "
          + ", ".join(f"{k} {v:.1f}" for k, v in run.cal[aux].items()) + f"; band {100 * run.ref[aux].band_share:.2f} % of the pixels")


@pytest.mark.parametrize("name", list_scenes.RASTER_SCENES)
def test_forward(name):
    run = _run(name)
    for aux in (False, True):
        out = run.fwd[aux]
        assert set(out) == ({"image", "accum", "depth", "alpha", "accum_aux"} if aux else {"image", "accum"})
        r = ro.check(out, run.ref[aux], run.K[aux], f"{name} forward{' aux' if aux else ''}")
        _report(name, "forward" + (" aux" if aux else ""), r, run, aux)
    if name == "clamps":
        acc, dec = run.ref[False].accum, run.ref[False].dec
        live = dec["q"] & dec["alive"]
        assert (acc < 0).any() and (acc > 1).any() and ((acc > 0) & (acc < 1)).any(), "pixels on each side of the image clamp"
        assert dec["max"][live].any() and not dec["max"][live].all(), "pixels on each side of the alpha_max clamp"


@pytest.mark.parametrize("name", list_scenes.RASTER_SCENES)
def test_box_test_forward_gives_the_same_bits(name):
    """SAVE = false (box-test queues) against SAVE = true (exact sub-tile test): a Gaussian missing from a queue contributes alpha 0."""
    run = _run(name)
    for aux in (False, True):
        for k in run.box[aux]:
            a, b = run.box[aux][k], run.fwd[aux][k]
            diff = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            assert not len(diff), f"{name}{' aux' if aux else ''} {k}: {len(diff)} values differ, first at {diff[0]}: {a[tuple(diff[0])]!r} != {b[tuple(diff[0])]!r}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list_scenes.RASTER_SCENES)
def test_backward(name, mode):
    run = _run(name)
    aux = mode.startswith("aux")
    ref, K = run.ref[aux], run.K[aux]
    r = ro.check(dict(grad2d=run.g2d[mode]), ref, K, f"{name} backward {mode}", pair_mask=run.arr["pair_mask"])
    _report(name, f"backward {mode}", r, run, aux)
    # grad2d_zeroed = 1 behind a forward that cleared grad2d: the same result (bit for bit where the order of the sums is fixed)
    ro.check(dict(grad2d=run.g2d_zeroed[mode]), ref, K, f"{name} backward {mode}, grad2d_zeroed", pair_mask=run.arr["pair_mask"])
    if "deterministic" in mode:
        assert np.array_equal(run.g2d[mode].view(np.uint32), run.g2d_zeroed[mode].view(np.uint32))
    else:
        other = run.g2d[mode.replace("atomic", "deterministic")]
        kk = np.array([K["moments"]] * 6 + [K["colour"]] * (ref.ns - 6))
        d = np.abs(run.g2d[mode].astype(np.float64) - other)[:, :ref.ns]
        bad = np.argwhere(d > kk[None, :] * ro.EPS * ref.scale + ref.allow)
        assert not len(bad), f"{name} {mode} against deterministic: Gaussian {bad[0][0]}, column {bad[0][1]}: |delta| {d[tuple(bad[0])]:.3e}"


@pytest.mark.parametrize("name", list_scenes.RASTER_SCENES)
def test_canaries(name):
    run = _run(name)
    assert len(run.intact) == 2 + 4 * 3 and all(run.intact)


def test_rows_under_a_zero_upstream_gradient_are_exact_zeros():
    """g_img zero on the left half of the image: the flush skips zeros, and a row whose pixels all lie there is an exact zero."""
    name = "g1_generic"
    run = _run(name)
    s, fr = run.s, run.fr
    gi = list_scenes.upstream(s, left_half_zero=True)[0]
    ref = ro.composite(*run.args, g_img=gi)
    cal = ro.ratios(ro.composite_f32(*run.args, g_img=gi), ref)
    K = {k: 3.0 * cal.get(k, 0.0) for k in ro.KINDS}
    silent = ref.in_list & ~ref.scale.any(1) & ~ref.allow.any(1)
    assert silent.sum() > 20 and (ref.scale.any(1)).sum() > 20
    for det in (False, True):
        fr.forward(accum=True)
        g = fr.backward(gi, det=det)
        assert fr.canaries_intact()
        r = ro.check(dict(grad2d=g), ref, K, f"{name} left half zero, {'deterministic' if det else 'atomic'}", pair_mask=run.arr["pair_mask"])
        assert not g[silent].any()
        print(f"{name} left half zero ({'deterministic' if det else 'atomic'}): {int(silent.sum())} rows exact zeros; device ratios {r}, float32 mode {cal}")
