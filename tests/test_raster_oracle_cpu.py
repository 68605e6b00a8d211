"""tests/raster_oracle.py checked on the CPU: (a) its image is the oracle's on the oracle's own float64 stages, (b) its rows are the
derivatives of a plain torch composite of the same records, (c) its checker rejects ten ways of breaking a consistent set of
"device outputs" (the float32 mode's) by naming the Gaussian or the pixel, (d) on every scene of tests/test_gpu_raster.py the float32
mode takes no decision differently from float64 outside the band, the band holds at most 3 % of the pixels, and the float32 mode's
largest |delta| / (2^-24 scale) is printed (the calibration the GPU test multiplies by 3)."""
import functools

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import list_scenes, util
from tests import raster_oracle as ro
from tests.cpu_frame import cpu_state, hm  # noqa: F401  (hm is a fixture)

BG = (1.0, 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return list_scenes.raster_scene(name)


_STATES = {}


def _state(hm, name):
    if name not in _STATES:
        _STATES[name] = cpu_state(hm, _scene(name))
    return _STATES[name]


def _args(st, s):
    return (st["rec"], st["ranges"], st["sorted_ids"], st["lists_x"], s["H"], s["W"]) + list_scenes.thresholds(s, as_float32=True)


def _grads(s, aux, **kw):
    gi, gd, ga = list_scenes.upstream(s, **kw)
    return dict(g_img=gi, g_depth=gd, g_alpha=ga, bg=BG, aux=True) if aux else dict(g_img=gi)


def _calibration(ref, f32):
    """K per output kind = 3 x the float32 mode's largest ratio."""
    r = ro.ratios(f32, ref)
    return {k: 3.0 * r.get(k, 0.0) for k in ro.KINDS}, r


# ---- (a) pinned to the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list_scenes.RASTER_GOLDENS)
def test_image_on_the_oracles_float64_stages_is_the_golden_image(name):
    d, s = util.load(name), _scene(name)
    st = {}
    dt = torch.float64
    tp.render_fused(*[torch.tensor(s[k], dtype=dt) for k in list_scenes.NAMES], torch.tensor(s["c2w"], dtype=dt), *list_scenes.cam_args(s), stages=st,
                    stop_after_binning=True, **s["kwargs"])
    V, T = len(st["ids"]), int(s["kwargs"].get("T", 16))
    assert T == 16, "a 16 x 8 list lies inside one tile of the reference only for T = 16"
    rec = np.zeros((V, 16))
    rec[:, 0], rec[:, 1], rec[:, 5] = st["u"].numpy(), st["v"].numpy(), st["opacity"].numpy()
    rec[:, 2:5], rec[:, 8:11] = st["conic"].numpy(), st["color"].numpy()
    lists_x, lists_y = (s["W"] + 15) // 16, (s["H"] + 7) // 8
    pl, pi = [], []
    for k, (x0, y0, x1, y1) in enumerate(st["tile_rect"].numpy()):          # stage order = depth order
        ys, xs = np.mgrid[y0 * T // 8:min((y1 * T + T - 1) // 8, lists_y - 1) + 1, x0 * T // 16:min((x1 * T + T - 1) // 16, lists_x - 1) + 1]
        pl.append((ys * lists_x + xs).ravel())
        pi.append(np.full(ys.size, k))
    pl, pi = np.concatenate(pl), np.concatenate(pi)
    o = np.lexsort((pi, pl))
    ln = np.bincount(pl, minlength=lists_x * lists_y)
    end = np.cumsum(ln)
    ref = ro.composite(rec, np.stack([end - ln, end], 1), pi[o], lists_x, s["H"], s["W"], *list_scenes.thresholds(s), allowances=False)
    delta = float(np.abs(ref.image - d["image"]).max())
    print(f"{name}: max |oracle image - golden float64 image| = {delta:.2e}")
    assert d["image"].dtype == np.float64 and delta <= 1e-12


# ---- (b) the rows are derivatives -----------------------------------------------------------------------------------------------------

def _torch_cotangents(st, s, gi, gd, ga, bg):
    """dL/d(u, v, A11, A12, A22, o, r, g, b, z) [n,10] of L = sum image g_img + sum D g_depth + sum A g_alpha, by autograd through a plain
    torch composite of the records (torch_port's F14 on 16 x 8 lists)."""
    dt = torch.float64
    chi, amax, cut = list_scenes.thresholds(s, as_float32=True)
    r = torch.tensor(st["rec"].astype(np.float64)[:, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]], requires_grad=True)
    H, W = s["H"], s["W"]
    loss = torch.zeros((), dtype=dt)
    bgt = None if bg is None else torch.tensor(bg, dtype=dt)
    for l_ in np.nonzero(st["ranges"][:, 1] > st["ranges"][:, 0])[0]:
        g = torch.tensor(st["sorted_ids"][st["ranges"][l_, 0]:st["ranges"][l_, 1]].astype(np.int64))
        px, py = ro._list_pixels(l_, st["lists_x"])
        ok = (px < W) & (py < H)
        px, py = px[ok], py[ok]
        e = r[g]
        du = torch.tensor(px, dtype=dt)[None, :] - e[:, 0:1]
        dv = torch.tensor(py, dtype=dt)[None, :] - e[:, 1:2]
        q = e[:, 2:3] * du * du + 2 * e[:, 3:4] * du * dv + e[:, 4:5] * dv * dv
        fall = torch.where(q <= chi, torch.exp(-0.5 * q.clamp(max=chi)), torch.zeros_like(q))
        og = e[:, 5:6] * fall
        alpha = torch.where(og >= cut, og.clamp_max(amax), torch.zeros_like(og))
        trans = torch.cumprod(1 - alpha, 0)
        trans = torch.cat([torch.ones_like(trans[:1]), trans[:-1]], 0)
        w = alpha * trans * (trans > 5e-5).to(dt)
        C, A, D = w.t() @ e[:, 6:9], w.sum(0), w.t() @ e[:, 9]
        shown = C if bgt is None else C + (1 - A)[:, None] * bgt[None, :]
        loss = loss + (shown.clamp(0, 1) * torch.tensor(gi[py, px], dtype=dt)).sum()
        loss = loss + (D * torch.tensor(gd[py, px], dtype=dt)).sum() + (A * torch.tensor(ga[py, px], dtype=dt)).sum()
    loss.backward()
    return r.grad.numpy()


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux_bg"])
@pytest.mark.parametrize("name", ["g1_generic", "g3_occlusion", "stacked", "clamps"])
def test_rows_are_the_derivatives_of_a_torch_composite(hm, name, aux):
    s, st = _scene(name), _state(hm, name)
    kw = _grads(s, aux)
    ref = ro.composite(*_args(st, s), allowances=False, **kw)
    z = np.zeros((s["H"], s["W"]), np.float32)
    want = _torch_cotangents(st, s, kw["g_img"], kw.get("g_depth", z), kw.get("g_alpha", z), kw.get("bg"))
    m, rec = ref.rows, st["rec"].astype(np.float64)
    o, a11, a12, a22 = rec[:, 5], rec[:, 2], rec[:, 3], rec[:, 4]
    got = np.stack([o * (a11 * m[:, 0] + a12 * m[:, 1]), o * (a12 * m[:, 0] + a22 * m[:, 1]), -0.5 * o * m[:, 2], -o * m[:, 3], -0.5 * o * m[:, 4],
                    m[:, 5], m[:, 6], m[:, 7], m[:, 8], m[:, 9]], 1)
    if name == "clamps":
        assert (ref.accum < 0).any() and (ref.accum > 1).any(), "the scene is there for colours outside [0, 1]"
    for k, col in enumerate(("u", "v", "A11", "A12", "A22", "o", "r", "g", "b", "z")):
        top = np.abs(want[:, k]).max()
        err = np.abs(got[:, k] - want[:, k]).max()
        print(f"{name} {'aux' if aux else 'plain'} d{col}: max |delta| {err:.2e} of max {top:.2e}")
        assert err <= 1e-9 * top, col
    assert aux or not want[:, 9].any()


# ---- (c) the checker can fail ---------------------------------------------------------------------------------------------------------

_SETS = {}


def _setup(hm, name, aux=False, rec=None, **f32_kw):
    """(s, st, kw, ref, f32, K) of a consistent set: float64 reference, float32 "device outputs", K from the calibration."""
    key = (name, aux)
    if key not in _SETS or rec is not None or f32_kw:
        s, st = _scene(name), dict(_state(hm, name))
        if rec is not None:
            st["rec"] = rec
        kw = _grads(s, aux)
        ref = ro.composite(*_args(st, s), **kw) if rec is not None or key not in _SETS else _SETS[key][3]
        f32 = ro.composite_f32(*_args(st, s), **kw, **f32_kw)
        K, _ = _calibration(ref, ro.composite_f32(*_args(st, s), **kw)) if f32_kw else _calibration(ref, f32)
        out = (s, st, kw, ref, f32, K)
        if rec is not None or f32_kw:
            return out
        _SETS[key] = out
    return _SETS[key]


def _rebuilt(f32, st, pair_sub=None, grad2d=None, **maps):
    out = dict(f32)
    if pair_sub is not None:
        grad2d = ro.rows_from_pairs(pair_sub, st["ranges"], st["sorted_ids"], st["n"])
    if grad2d is not None:
        out["grad2d"] = grad2d
    out.update(maps)
    return out


def _rejects(dev, ref, K, pattern, pair_mask=None):
    with pytest.raises(ro.RasterError, match=pattern) as e:
        ro.check(dev, ref, K, "broken", pair_mask=pair_mask)
    print(e.value)


def test_checker_accepts_the_float32_mode(hm):
    for name, aux in (("g1_generic", False), ("stacked", True), ("g2_ragged", False)):
        s, st, kw, ref, f32, K = _setup(hm, name, aux)
        ro.check(f32, ref, K, name, pair_mask=st["pair_mask"])


def test_rejects_a_left_out_subtile_slot(hm):
    s, st, kw, ref, f32, K = _setup(hm, "g1_generic")
    ps = f32["pair_sub"].copy()
    k, t = np.argwhere(np.abs(ps[:, :, 5]) > 0.05 * np.abs(ps[:, :, 5]).max())[7]
    ps[k, t] = 0
    _rejects(_rebuilt(f32, st, ps), ref, K, rf"Gaussian {st['sorted_ids'][k]}, column \d")


def test_rejects_the_last_entry_of_a_cut_chunk_left_out(hm):
    s, st, kw, ref, f32, K = _setup(hm, "stacked", True)
    cn, cp, chunks = ro.chunk_layout(st["ranges"], st["pair_mask"])
    cut = [c for c in chunks if c[3]]
    assert cut, "the stacked scene has chunks cut at the queue cap"
    l_, first, n, _ = cut[0]
    bits = (st["pair_mask"][first:first + n, None] >> np.arange(8)) & 1
    assert bits.sum(0).max() == ro.MAXQ_BWD or n == ro.MAXQ_BWD          # the cut leaves a full queue: its last entry sits at queue position 24
    k = first + n - 1
    ps = f32["pair_sub"].copy()
    ps[k] = 0
    _rejects(_rebuilt(f32, st, ps), ref, K, rf"Gaussian {st['sorted_ids'][k]}, column \d.*backward chunk 0, position {n - 1} in the chunk", st["pair_mask"])


def test_rejects_an_entry_past_kdone_added_in(hm):
    st = _state(hm, "stacked")
    rec = st["rec"].copy()
    rec[:, 2:5] *= 0.02                   # every Gaussian covers the whole list, nearly opaque: all 128 pixels are dead after a few entries
    rec[:, 5] = 0.9
    s, st, kw, ref, f32, K = _setup(hm, "stacked", rec=rec)
    dead = np.nonzero(~ref.dec["alive"].any(1))[0]
    assert len(dead) > 200, "every pixel of the list dies early"
    k = int(dead[0]) + 10                                          # a slot behind the 8-entry block in which the last pixel died
    assert not f32["pair_sub"][k].any()
    ps = f32["pair_sub"].copy()
    ps[k] = f32["pair_sub"][1]                                     # what an earlier entry left in a slot
    _rejects(_rebuilt(f32, st, ps), ref, K, rf"Gaussian {st['sorted_ids'][k]}, column \d")


def _on_the_clamp(hm):
    """g1's consistent state with one Gaussian moved onto a pixel centre and given opacity alpha_max: o g = alpha_max exactly there."""
    st = _state(hm, "g1_generic")
    rec = st["rec"].copy()
    ln = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    l_ = int(np.nonzero(ln >= 3)[0][0])
    i = int(st["sorted_ids"][st["ranges"][l_, 0]])                # first entry of the list: T = 1 on its pixels
    x, y = (l_ % st["lists_x"]) * 16 + 5, (l_ // st["lists_x"]) * 8 + 3
    assert abs(rec[i, 0] - x) < 24 and abs(rec[i, 1] - y) < 12
    rec[i, 0], rec[i, 1], rec[i, 5] = x, y, np.float32(0.99)
    return rec, i, (y, x)


def test_rejects_a_strict_clamp_mask_on_a_row_that_sits_on_the_clamp(hm):
    rec, i, (y, x) = _on_the_clamp(hm)
    s, st, kw, ref, f32, K = _setup(hm, "g1_generic", rec=rec)
    ro.check(f32, ref, K, "on the clamp")
    s, st, kw, ref, bad, K = _setup(hm, "g1_generic", rec=rec, strict_clamp=True)
    _rejects(bad, ref, K, rf"Gaussian {i}, column [0-5]\b")


def test_rejects_an_ignored_image_clamp(hm):
    s, st, kw, ref, f32, K = _setup(hm, "clamps")
    assert (ref.accum < 0).any() and (ref.accum > 1).any()
    _, _, _, _, bad, _ = _setup(hm, "clamps", ignore_image_clamp=True)
    _rejects(bad, ref, K, r"Gaussian \d+, column \d")


def test_rejects_swapped_rows_of_a_flush_group(hm):
    s, st, kw, ref, f32, K = _setup(hm, "g1_generic")
    ln = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    a = int(st["ranges"][int(np.argmax(ln)), 0])
    i, j = (int(x) for x in st["sorted_ids"][a:a + 2])                # rows 0 and 1 of the first flush instruction
    g = f32["grad2d"].copy()
    g[[i, j]] = g[[j, i]]
    _rejects(_rebuilt(f32, st, grad2d=g), ref, K, rf"Gaussian ({i}|{j}), column \d")


def test_rejects_a_composited_pixel_outside_a_ragged_image(hm):
    s, st, kw, ref, f32, K = _setup(hm, "g2_ragged")
    assert s["W"] % 16 and s["H"] % 8
    _, _, _, _, bad, _ = _setup(hm, "g2_ragged", ragged_bug=True)
    _rejects(bad, ref, K, r"Gaussian \d+, column \d")


def test_rejects_column_9_in_column_8_and_a_dirty_padding_column(hm):
    s, st, kw, ref, f32, K = _setup(hm, "stacked", True)
    g = f32["grad2d"].copy()
    g[:, 8] = g[:, 9]
    _rejects(_rebuilt(f32, st, grad2d=g), ref, K, r"Gaussian \d+, column 8\b")
    g = f32["grad2d"].copy()
    i = int(st["sorted_ids"][5])
    g[i, 12] = 1e-30
    _rejects(_rebuilt(f32, st, grad2d=g), ref, K, rf"Gaussian {i}, padding column 12\b")


def test_rejects_a_64th_entry_composited_twice(hm):
    s, st, kw, ref, f32, K = _setup(hm, "stacked", True)
    k = int(st["ranges"][0, 0]) + 63
    ps = f32["pair_sub"].copy()
    ps[k] *= 2
    _rejects(_rebuilt(f32, st, ps), ref, K, rf"Gaussian {st['sorted_ids'][k]}, column \d")


def test_rejects_a_wrong_pixel_and_an_image_that_is_not_the_clamp_of_accum(hm):
    s, st, kw, ref, f32, K = _setup(hm, "clamps")
    img = f32["image"].copy()
    img[3, 7, 1] += 1e-4
    _rejects(_rebuilt(f32, st, image=img), ref, K, r"pixel \(3, 7\) channel 1 of image")
    y, x, c = np.argwhere(f32["accum"] > 1)[0]
    img = f32["image"].copy()
    img[y, x, c] = f32["accum"][y, x, c]
    _rejects(_rebuilt(f32, st, image=img), ref, dict(K, image=1e30), rf"pixel \({y}, {x}\) channel {c}: image")


# ---- (d) the band and the calibration ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list_scenes.RASTER_SCENES)
def test_band_and_float32_calibration(hm, name):
    s, st = _scene(name), _state(hm, name)
    for aux in (False, True):
        kw = _grads(s, aux)
        ref = ro.composite(*_args(st, s), **kw)
        f32 = ro.composite_f32(*_args(st, s), **kw)
        outside = ro.decisions_outside_band(ref, f32["dec"])
        r = ro.ratios(f32, ref)
        print(f"{name} {'aux' if aux else 'plain'}: {st['n_binned']} pairs, longest list {int((st['ranges'][:, 1].astype(np.int64) - st['ranges'][:, 0]).max())}; "
              f"band {int(ref.band_pixels.sum())} of {ref.band_pixels.size} pixels ({100 * ref.band_share:.2f} %), {ref.n_flips} flips; decisions outside "
              f"the band {outside}; float32 mode |delta| / (2^-24 scale): " + ", ".join(f"{k} {v:.1f}" for k, v in r.items()))
        assert outside == 0
        assert ref.band_share <= 0.03
        ro.check(f32, ref, {k: 1.0001 * r.get(k, 0.0) for k in ro.KINDS}, name, pair_mask=st["pair_mask"])
    if name == "clamps":
        rec = st["rec"].astype(np.float64)
        assert (ref.accum < 0).any() and (ref.accum > 1).any() and ((ref.accum > 0) & (ref.accum < 1)).any()
        assert not ref.dec["max"][ref.dec["q"] & ref.dec["alive"]].all() and ref.dec["max"][ref.dec["q"] & ref.dec["alive"]].any()
        assert rec[:, 5].max() > 0.99
