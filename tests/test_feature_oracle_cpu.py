"""tests/feature_oracle.py checked on the CPU, on cpu_state() of two small scenes: (a) the wrapper over raster_oracle agrees with a
direct dense float64 evaluation -- an explicit [entries, pixels] weight matrix per list, built here from the rule in raster_oracle's
docstring -- to 1e-12 relative; (b) the adjoint identity <W f, G> = <f, W^T G> holds to 1e-12 for random signed f, G at C = 5; (c) the
check accepts the float32 twins under their own calibration and rejects eleven deliberately broken outputs."""
import numpy as np
import pytest

from tests import feature_oracle as fo
from tests import list_scenes
from tests.cpu_frame import cpu_state, hm  # noqa: F401  (hm is a fixture)

SCENES = ("g2_ragged", "g3_occlusion")
C_ID, C_BROKEN = 5, 9
_SETUPS = {}


def _dense(args, alive_test=True, clip_test=True):
    """Per non-empty list: (Gaussian ids [L], py [P], px [P], w [L,P]) over its pixels inside the image, from the rule:
    q = A11 du^2 + 2 A12 du dv + A22 dv^2, og = o exp(-q / 2), pass = (q <= chi) and (og >= cutoff), alpha = pass ? min(og, alpha_max) : 0,
    T_i = prod_{k<i} (1 - alpha_k), alive = T_i > 5e-5, w = alive ? alpha T : 0."""
    rec, ranges, ids, lists_x, H, W, chi, amax, cut = args
    rec = np.asarray(rec, np.float64)
    for l_ in range(len(ranges)):
        s0, s1 = int(ranges[l_][0]), int(ranges[l_][1])
        if s1 <= s0:
            continue
        g = np.asarray(ids[s0:s1], np.int64)
        ys, xs = np.meshgrid(np.arange(8) + (l_ // lists_x) * 8, np.arange(16) + (l_ % lists_x) * 16, indexing="ij")
        ys, xs = ys.ravel(), xs.ravel()
        keep = (ys < H) & (xs < W)
        ys, xs = ys[keep], xs[keep]
        r = rec[g]
        du, dv = xs[None, :] - r[:, 0:1], ys[None, :] - r[:, 1:2]
        q = r[:, 2:3] * du * du + 2 * r[:, 3:4] * du * dv + r[:, 4:5] * dv * dv
        og = r[:, 5:6] * np.exp(-0.5 * np.minimum(q, 1e3))
        ok = ((q <= chi) if clip_test else True) & (og >= cut)
        alpha = np.where(ok, np.minimum(og, amax), 0.0)
        T = np.cumprod(1.0 - alpha, 0)
        T = np.concatenate([np.ones_like(T[:1]), T[:-1]], 0)
        w = np.where(T > 5e-5, alpha * T, 0.0) if alive_test else alpha * T
        yield g, ys, xs, w


def _dense_map(args, feats, drop=None, **kw):
    H, W = args[4], args[5]
    out, scale = np.zeros((H, W, feats.shape[1])), np.ones((H, W, feats.shape[1]))
    for k, (g, ys, xs, w) in enumerate(_dense(args, **kw)):
        if drop is not None and drop[0] == k:
            w = w.copy()
            w[drop[1]] = 0.0
        out[ys, xs] = w.T @ feats[g]
        scale[ys, xs] += w.T @ np.abs(feats[g])
    return out, scale


def _dense_rows(args, G, overwrite=False, **kw):
    n = len(args[0])
    rows, scale = np.zeros((n, G.shape[2])), np.zeros((n, G.shape[2]))
    for g, ys, xs, w in _dense(args, **kw):
        if overwrite:
            rows[g] = w @ G[ys, xs]
        else:
            rows[g] += w @ G[ys, xs]                     # (a Gaussian is in a list once)
        scale[g] += w @ np.abs(G[ys, xs])
    return rows, scale


def _setup(hm, name, C):
    if (name, C) not in _SETUPS:
        s = list_scenes.raster_scene(name)
        st = cpu_state(hm, s)
        args = (st["rec"], st["ranges"], st["sorted_ids"], st["lists_x"], s["H"], s["W"]) + list_scenes.thresholds(s, as_float32=True)
        rng = np.random.default_rng(17)
        feats = rng.normal(0, 1, (st["n"], C)).astype(np.float32)
        G = rng.normal(0, 1, (s["H"], s["W"], C)).astype(np.float32)
        _SETUPS[(name, C)] = (s, args, feats.astype(np.float64), G.astype(np.float64)) + fo.calibration(args, feats, G)
    return _SETUPS[(name, C)]


@pytest.mark.parametrize("name", SCENES)
def test_wrapper_against_the_dense_evaluation_and_the_adjoint_identity(hm, name):
    s, args, feats, G, K_map, K_rows, fwd, adj = _setup(hm, name, C_ID)
    want, scale = _dense_map(args, feats)
    assert fwd.value.any() and (np.abs(fwd.value - want) <= 1e-12 * scale).all()
    assert (np.abs(fwd.scale - scale) <= 1e-12 * scale).all()
    rows, rscale = _dense_rows(args, G)
    assert adj.value.any() and (np.abs(adj.value - rows) <= 1e-12 * np.maximum(rscale, 1e-300)).all()
    assert (np.abs(adj.scale - rscale) <= 1e-12 * np.maximum(rscale, 1e-300)).all()
    touched = np.zeros(len(feats), bool)
    for g, _, _, _ in _dense(args):
        touched[g] = True
    assert np.array_equal(adj.in_list, touched) and not adj.value[~touched].any()
    lhs, rhs = float((fwd.value * G).sum()), float((feats * adj.value).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(np.abs(fwd.value * G).sum() + np.abs(feats * adj.value).sum())
    assert (fwd.value < 0).any() and (fwd.value > 0).any(), "signed features give a signed map"


@pytest.mark.parametrize("name", SCENES)
def test_check_accepts_the_float32_twins_and_the_band_is_small(hm, name):
    s, args, feats, G, K_map, K_rows, fwd, adj = _setup(hm, name, C_BROKEN)
    print(f"{name}: float32 twins need K_map {K_map / 3:.2f}, K_rows {K_rows / 3:.2f} (bounds: 3 x); "
          f"{100 * float((fwd.allow > 0).any(2).mean()):.2f} % of the pixels and {int((adj.allow > 0).any(1).sum())} of {int(adj.in_list.sum())} rows carry an allowance")
    assert 0 < K_map < 300 and 0 < K_rows < 300
    assert fo.check(fo.render_f32(args, feats), fwd, K_map, name) <= K_map / 3 + 1e-9
    assert fo.check(fo.adjoint_f32(args, G), adj, K_rows, name) <= K_rows / 3 + 1e-9
    assert (fwd.allow > 0).any(2).mean() < 0.25 and (adj.allow[adj.in_list] == 0).all(1).sum() > 20
    # twice the reference is what two adding calls leave
    fo.check(2 * fo.adjoint_f32(args, G).astype(np.float64), adj, K_rows, name, calls=2)


def _rejects(got, ref, K, pattern):
    with pytest.raises(fo.FeatureError, match=pattern) as e:
        fo.check(got, ref, K, "broken")
    print(e.value)


def test_check_rejects_broken_outputs(hm):
    s, args, feats, G, K_map, K_rows, fwd, adj = _setup(hm, "g3_occlusion", C_BROKEN)
    H, W, C = s["H"], s["W"], C_BROKEN
    good_map, good_rows = fo.render_f32(args, feats).astype(np.float64), fo.adjoint_f32(args, G).astype(np.float64)
    # 1: every channel shifted by one
    _rejects(np.roll(good_map, 1, axis=2), fwd, K_map, "pixel")
    # 2: the tail channel of the partial group dropped
    m = good_map.copy()
    m[..., 8] = 0.0
    _rejects(m, fwd, K_map, "channel 8")
    # 3: a dead pixel's weight counted (no alive test)
    dead, _ = _dense_map(args, feats, alive_test=False)
    assert (dead != _dense_map(args, feats)[0]).any(), "the scene has dead pixels"
    _rejects(dead, fwd, K_map, "pixel")
    # 4: the chi-square clip ignored
    _rejects(_dense_map(args, feats, clip_test=False)[0], fwd, K_map, "pixel")
    # 5: the last pixel column of the image left unwritten
    m = good_map.copy()
    m[:, W - 1] = 0.0
    _rejects(m, fwd, K_map, rf"pixel \(\d+, {W - 1}\)")
    # 6: an entry beside the first chunk boundary lost (the heaviest of positions 56 .. 71 over the lists longer than a chunk)
    cands = [(float(w[p].sum()), k, p) for k, (g, _, _, w) in enumerate(_dense(args)) if len(g) > 64 for p in range(56, min(72, len(g)))]
    assert cands and max(cands)[0] > 0, "a list longer than one chunk with weight at the boundary"
    _rejects(_dense_map(args, feats, drop=max(cands)[1:])[0], fwd, K_map, "pixel")
    # 7: an adjoint that overwrites instead of adding over a Gaussian's lists
    over, _ = _dense_rows(args, G, overwrite=True)
    _rejects(over, adj, K_rows, "Gaussian")
    # 8: the lane's two pixels swapped when G is read (rows y and y + 2 of every sub-tile)
    yy = np.arange(H)
    swapped = np.where(yy % 4 < 2, yy + 2, yy - 2)
    Gs = np.zeros_like(G)
    ok = swapped < H
    Gs[yy[ok]] = G[swapped[ok]]
    _rejects(_dense_rows(args, Gs)[0], adj, K_rows, "Gaussian")
    # 9: the channels of a group leave in the wrong lanes (c -> 7 - c inside the full group)
    r = good_rows.copy()
    r[:, :8] = good_rows[:, 7::-1]
    _rejects(r, adj, K_rows, "Gaussian")
    # 10: one row flushed twice
    i = int(np.argmax(np.abs(adj.value).sum(1)))
    r = good_rows.copy()
    r[i] *= 2
    _rejects(r, adj, K_rows, f"Gaussian {i},")
    # 11: the row of a Gaussian in no list written
    _, args2, _, G2, _, K2, _, adj2 = _setup(hm, "g2_ragged", C_BROKEN)
    assert (~adj2.in_list).any()
    j = int(np.nonzero(~adj2.in_list)[0][0])
    r = fo.adjoint_f32(args2, G2).astype(np.float64)
    fo.check(r, adj2, K2, "g2_ragged")
    r[j, 3] = 1e-30
    _rejects(r, adj2, K2, f"Gaussian {j} is in no list")
    # and a NaN anywhere
    m = good_map.copy()
    m[0, 0, 0] = np.nan
    _rejects(m, fwd, K_map, "non-finite")
