"""The MCMC density control on the device (csrc/gsplat_mcmc.hip) against tests/mcmc_oracle.py: the scan and the draw
bit for bit, the relocation row by row, growth with a carried optimiser, the position noise, the regularisers, and the trainer's
"mcmc" rule end to end.  Every buffer a kernel writes sits between guard margins that are read back."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from oracle import scenes
from tests import mcmc_oracle as mo
from tests.ranks import run_ranks

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
NAMES = ("pos", "opacity_raw", "f_dc", "f_rest", "scale_raw", "q_raw")
ORDER = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")           # the order of the C entry and of gsplat_mcmc_moments
WIDTH = dict(pos=3, f_dc=3, f_rest=45, opacity_raw=1, scale_raw=3, q_raw=4)
COPIED = ("pos", "f_dc", "f_rest", "q_raw")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
RTOL = 1e-6              # the CPU test's bound on the relocation (tests/test_mcmc_cpu.py)

abi = importlib.import_module(PKG + "._abi")


class Guarded:
    """A device array between two margins of GUARD bytes that hold a bit pattern."""

    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.nbytes, self.dtype, self.shape = host.nbytes, host.dtype, host.shape
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + self.nbytes] = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def host(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype).reshape(self.shape)

    def intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.nbytes:] == PATTERN).all())


def _layout(n):
    lay = abi.McmcLayout()
    assert abi.lib().gsplat_mcmc_scratch_layout(n, C.byref(lay)) == abi.GSPLAT_OK
    return lay


def _params(n, sigma, rng, scale=(-5.0, -1.0)):
    """Random rows of the six parameters with the given opacities."""
    sigma = np.asarray(sigma, dtype=np.float64)
    return dict(pos=rng.normal(size=(n, 3)).astype(np.float32), f_dc=rng.normal(size=(n, 3)).astype(np.float32),
                f_rest=rng.normal(size=(n, 45)).astype(np.float32), opacity_raw=np.log(sigma / (1 - sigma)).astype(np.float32),
                scale_raw=rng.uniform(*scale, (n, 3)).astype(np.float32), q_raw=rng.normal(size=(n, 4)).astype(np.float32))


def _refine(P, n, min_opacity, seed, iteration, moments=None):
    """gsplat_mcmc_refine on guarded copies: (params after, moments after, scratch arrays)."""
    lib = abi.lib()
    lay = _layout(n)
    g = {k: Guarded(P[k]) for k in ORDER}
    scratch = Guarded(np.zeros(lay.bytes, np.uint8))
    mo_struct, gm = None, None
    if moments is not None:
        gm = {k: (Guarded(moments[k][0]), Guarded(moments[k][1])) for k in ORDER}
        mo_struct = abi.McmcMoments()
        for k in ORDER:
            getattr(mo_struct, k)[0], getattr(mo_struct, k)[1] = gm[k][0].ptr.value, gm[k][1].ptr.value
    torch.cuda.synchronize()
    status = lib.gsplat_mcmc_refine(*[g[k].ptr for k in ORDER], C.byref(mo_struct) if mo_struct is not None else None, n, min_opacity, seed,
                                    iteration, scratch.ptr, None)
    assert status == abi.GSPLAT_OK, lib.gsplat_last_error()
    torch.cuda.synchronize()
    assert scratch.intact() and all(x.intact() for x in g.values())
    assert gm is None or all(a.intact() and b.intact() for a, b in gm.values())
    raw = scratch.host()
    arrays = dict(w=raw[lay.w:lay.w + n * 4].view(np.uint32), prefix=raw[lay.prefix:lay.prefix + n * 8].view(np.uint64),
                  src=raw[lay.src:lay.src + n * 4].view(np.int32), count=raw[lay.count:lay.count + n * 4].view(np.int32),
                  total=int(raw[lay.total:lay.total + 8].view(np.uint64)[0]))
    assert not raw[lay.reg:lay.reg + 256].any()               # the regulariser's counter is not the refinement's to touch
    after = {k: g[k].host() for k in ORDER}
    m_after = {k: (gm[k][0].host(), gm[k][1].host()) for k in ORDER} if gm is not None else None
    return after, m_after, arrays


def _scan_sizes():
    lay = _layout(1)
    b, c = lay.scan_block, lay.scan_chunk
    return [b - 1, b + 1, 3 * b + 37, b * c + b + 5]


@pytest.mark.parametrize("which", range(4), ids=["one block minus a row", "one block plus a row", "three blocks and a tail", "block sums in two passes"])
def test_scan_and_draw_match_the_integer_oracle(which):
    n = _scan_sizes()[which]
    rng = np.random.default_rng(10 + which)
    sigma = np.where(rng.uniform(size=n) < 0.1, rng.uniform(1e-4, 0.004, n), rng.uniform(0.006, 0.999, n))
    P = _params(n, sigma, rng)
    seed, it = 0x9E3779B97F4A7C15, 700 + which
    _, _, a = _refine(P, n, 0.005, seed, it)
    want, safe = mo.weights(P["opacity_raw"], 0.005)
    dead = a["w"] == 0
    assert 0.05 * n < dead.sum() < 0.15 * n and np.array_equal(dead, want == 0)
    assert np.array_equal(a["w"][safe].astype(np.uint64), want[safe])
    assert (np.abs(a["w"].astype(np.int64) - want.astype(np.int64)) <= 1).all()
    w64 = a["w"].astype(np.uint64)
    inc = np.cumsum(w64, dtype=np.uint64)
    assert np.array_equal(a["prefix"], inc - w64) and a["total"] == int(inc[-1])          # the device's own weights, bit for bit
    _, src, count, _ = mo.draw_fast(a["w"], seed, it)
    assert np.array_equal(a["src"], src) and np.array_equal(a["count"], count)
    assert (a["src"][dead] >= 0).all() and (a["src"][~dead] == -1).all() and a["count"].sum() == dead.sum()


def _moments(n, rng):
    return {k: (rng.normal(size=(n, WIDTH[k])).astype(np.float32), rng.uniform(0.1, 1, (n, WIDTH[k])).astype(np.float32)) for k in ORDER}


def _sigmoid32(raw):
    return mo.sigmoid(np.asarray(raw, np.float32), np.float32).astype(np.float64)


def _check_relocation(P, M, after, m_after, a, min_opacity):
    n = len(P["opacity_raw"])
    src, count = a["src"], a["count"]
    dst = np.nonzero(src >= 0)[0]
    sources = np.nonzero(count > 0)[0]
    touched = np.zeros(n, bool)
    touched[dst] = touched[sources] = True
    for k in COPIED:                                     # destinations: bit copies of the OLD source rows; sources keep these four
        assert np.array_equal(after[k][dst].view(np.uint32), P[k][src[dst]].view(np.uint32)), k
        assert np.array_equal(after[k][sources].view(np.uint32), P[k][sources].view(np.uint32)), k
    worst_o = worst_s = 0.0
    for s in sources:
        o = float(_sigmoid32(P["opacity_raw"][s]))
        _, opp, c, lnc = mo.relocation_exact(o, min(int(count[s]) + 1, 51), min_opacity)
        want_scale = P["scale_raw"][s].astype(np.float64) + lnc
        rows = np.concatenate([[s], dst[src[dst] == s]])
        assert len(rows) == count[s] + 1
        got_o = mo.sigmoid(after["opacity_raw"][rows].astype(np.float64))
        worst_o = max(worst_o, float(np.abs(got_o - opp).max() / opp))
        err_s = np.abs(after["scale_raw"][rows].astype(np.float64) - want_scale) - 2.0 ** -24 * np.maximum(1.0, np.abs(want_scale))
        worst_s = max(worst_s, float(err_s.max()))
        for r in rows[1:]:                               # source and copies carry the same new values, bit for bit
            assert after["opacity_raw"][r] == after["opacity_raw"][s] and np.array_equal(after["scale_raw"][r], after["scale_raw"][s])
    print(f"relocation: {len(dst)} rows onto {len(sources)} sources (max draws {count.max()}), opacity error {worst_o:.2e} relative, "
          f"scale error beyond its rounding {worst_s:.2e}")
    assert worst_o <= RTOL and worst_s <= RTOL
    for k in ORDER:
        assert np.array_equal(after[k][~touched].view(np.uint32), P[k][~touched].view(np.uint32)), k
        for h in range(2):
            assert np.array_equal(m_after[k][h][~touched].view(np.uint32), M[k][h][~touched].view(np.uint32)), (k, h)
            assert not m_after[k][h][touched].view(np.uint32).any(), (k, h)
    return dst, sources


def test_relocation_with_ordinary_weights():
    n, rng = 600, np.random.default_rng(20)
    sigma = rng.uniform(0.01, 0.6, n)
    dead = rng.choice(n, 50, replace=False)
    sigma[dead] = rng.uniform(1e-4, 0.004, 50)
    P, M = _params(n, sigma, rng), _moments(n, rng)
    P["opacity_raw"][dead[:3]] = (-20.0, -80.0, np.float32(np.log(0.005 / 0.995)) - 1e-3)       # an appended row, an extreme one, one just below
    after, m_after, a = _refine(P, n, 0.005, 5, 300, M)
    dst, sources = _check_relocation(P, M, after, m_after, a, 0.005)
    assert sorted(dst.tolist()) == sorted(dead.tolist()) and 20 <= len(sources) <= 50
    assert a["count"].max() >= 2                          # (some source was drawn more than once)


def test_relocation_onto_one_dominant_source_hits_the_cap_of_51():
    n, rng = 600, np.random.default_rng(21)
    sigma = np.full(n, 2e-5)                              # alive at min_opacity = 1e-5, weight 335 each
    dead = rng.choice(np.arange(1, n), 80, replace=False)
    sigma[dead] = 2e-6
    P, M = _params(n, sigma, rng), _moments(n, rng)
    P["opacity_raw"][0] = 0.0                             # sigmoid = 1/2 exactly: weight 2^23 against 174 000 for all the others
    after, m_after, a = _refine(P, n, 1e-5, 6, 301, M)
    assert a["count"][0] >= 70                            # more than 50 draws: n = 51 for the source and every copy
    _check_relocation(P, M, after, m_after, a, 1e-5)
    _, opp, c, _ = mo.relocation_exact(0.5, 51, 1e-5)
    assert abs(float(mo.sigmoid(np.float64(after["opacity_raw"][0]))) - opp) <= RTOL * opp


@pytest.mark.parametrize("sigma", [1e-3, 0.3], ids=["all dead", "none dead"])
def test_nothing_changes_when_all_rows_are_dead_or_none_is(sigma):
    n, rng = 600, np.random.default_rng(22)
    P, M = _params(n, np.full(n, sigma), rng), _moments(n, rng)
    after, m_after, a = _refine(P, n, 0.005, 7, 302, M)
    assert a["total"] == (0 if sigma < 0.005 else int(a["w"].astype(np.uint64).sum())) and (a["src"] == -1).all() and not a["count"].any()
    for k in ORDER:
        assert np.array_equal(after[k].view(np.uint32), P[k].view(np.uint32)), k
        for h in range(2):
            assert np.array_equal(m_after[k][h].view(np.uint32), M[k][h].view(np.uint32)), (k, h)


def _model_from(P):
    model_mod = importlib.import_module(PKG + ".model")
    init = {k: torch.tensor(P[k].reshape(-1) if k == "opacity_raw" else P[k]) for k in NAMES}
    return model_mod.GaussianModel(init, device=DEV)


def test_growth_appends_dead_rows_and_carries_the_optimiser():
    gs = importlib.import_module(PKG)
    n, rng = 100, np.random.default_rng(23)
    model = _model_from(_params(n, rng.uniform(0.05, 0.9, n), rng))
    opt = gs.optim.GaussianAdam(gs.optim.reference_param_groups(model), lr=0.01, eps=1e-15)
    before = {}
    for j, k in enumerate(NAMES):
        st = opt._state(getattr(model, k))
        st['step'] = 5 + j
        st['exp_avg'].copy_(torch.randn_like(st['exp_avg']))
        st['exp_avg_sq'].copy_(torch.rand_like(st['exp_avg_sq']) + 0.1)
        before[k] = (getattr(model, k).detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone())
    groups = [g['lr'] for g in opt.param_groups]
    assert gs.mcmc.refine(model, opt, cap_max=103, min_opacity=0.005, growth=1.05, seed=1, iteration=100) == 3
    torch.cuda.synchronize()
    assert model.get_num_gaussians() == 103 and [g['lr'] for g in opt.param_groups] == groups
    lay = gs.mcmc.layout(103)
    raw = gs.mcmc.scratch(103, model.pos.device).cpu().numpy()
    src, count = raw[lay.src:lay.src + 103 * 4].view(np.int32), raw[lay.count:lay.count + 103 * 4].view(np.int32)
    assert (src[:100] == -1).all() and (src[100:] >= 0).all() and (src[100:] < 100).all() and count.sum() == 3
    touched = torch.tensor(count > 0) | torch.tensor(src >= 0)
    for j, (g, k) in enumerate(zip(opt.param_groups, NAMES)):
        p = getattr(model, k)
        assert g['params'][0] is p and p.shape[0] == 103 and torch.isfinite(p).all() and set(opt.state) >= {p}
        st = opt.state[p]
        keep = ~touched.to(p.device)
        assert st['step'] == 5 + j and st['exp_avg'].shape == p.shape and st['exp_avg_sq'].shape == p.shape
        assert torch.equal(st['exp_avg'][keep], before[k][1][keep[:100]]) and torch.equal(st['exp_avg_sq'][keep], before[k][2][keep[:100]])
        assert not st['exp_avg'][~keep].any() and not st['exp_avg_sq'][~keep].any()
        assert torch.equal(p.detach()[keep], before[k][0][keep[:100]])
    assert len(opt.state) == 6
    # the copies are alive: a second refinement finds nothing dead, appends nothing (the cap) and changes nothing
    snap = {k: getattr(model, k).detach().clone() for k in NAMES}
    ids = {k: id(getattr(model, k)) for k in NAMES}
    assert gs.mcmc.refine(model, opt, cap_max=103, min_opacity=0.005, growth=1.05, seed=1, iteration=200) == 0
    assert model.get_num_gaussians() == 103 and all(id(getattr(model, k)) == ids[k] for k in NAMES)
    assert all(torch.equal(getattr(model, k).detach(), snap[k]) for k in NAMES)
    assert gs.mcmc.refine(model, opt, cap_max=50, min_opacity=0.005, growth=1.05, seed=1, iteration=300) == 0      # above the cap: never shrinks
    assert model.get_num_gaussians() == 103


def _noise(P, n, a, seed, it):
    lib = abi.lib()
    g = {k: Guarded(P[k]) for k in ("pos", "opacity_raw", "scale_raw", "q_raw")}
    torch.cuda.synchronize()
    assert lib.gsplat_mcmc_noise(n, g["pos"].ptr, g["opacity_raw"].ptr, g["scale_raw"].ptr, g["q_raw"].ptr, a, seed, it, None) == abi.GSPLAT_OK
    torch.cuda.synchronize()
    assert all(x.intact() for x in g.values())
    for k in ("opacity_raw", "scale_raw", "q_raw"):
        assert np.array_equal(g[k].host().view(np.uint32), P[k].view(np.uint32))
    return g["pos"].host()


def test_position_noise_against_the_float64_oracle():
    n, rng = 4099, np.random.default_rng(30)
    third = n // 3
    sigma = np.concatenate([rng.uniform(1e-4, 0.004, third), rng.uniform(0.005, 0.02, third), rng.uniform(0.9, 0.9999, n - 2 * third)])
    P = _params(n, sigma, rng)
    P["opacity_raw"][:2], P["opacity_raw"][-2:] = -80.0, 80.0
    P["pos"][:2 * third] = 0.0                            # the rows that move start at 0: what they hold afterwards IS the displacement
    a = float(np.float32(1.6e-4 * 5e5))
    got = _noise(P, n, a, 11, 40)
    assert np.isfinite(got).all()
    opaque = np.arange(n) >= 2 * third
    assert np.array_equal(got[opaque].view(np.uint32), P["pos"][opaque].view(np.uint32))       # g is exactly 0: bit for bit
    moved = ~opaque
    assert (np.abs(got[moved]).max(axis=1) > 0).all()
    ref = mo.noise_displacement(P["opacity_raw"], P["scale_raw"], P["q_raw"], a, 11, 40, gate32=moved)
    f32 = mo.noise_displacement(P["opacity_raw"], P["scale_raw"], P["q_raw"], a, 11, 40, dtype=np.float32, gate32=moved).astype(np.float64)
    size = np.abs(ref).max(axis=1, keepdims=True) + 1e-300
    bound = 4 * (np.abs(f32 - ref) / size)[moved].max()
    err = (np.abs(got.astype(np.float64) - ref) / size)[moved].max()
    print(f"noise: worst error relative to the row's displacement {err:.3e}, bound (4 x numpy float32) {bound:.3e}")
    assert err <= bound < 1e-3
    assert np.array_equal(_noise(P, n, a, 11, 40).view(np.uint32), got.view(np.uint32))        # the same (seed, iteration): the same bits
    for seed, it in ((11, 41), (12, 40)):
        other = _noise(P, n, a, seed, it)
        assert (other[moved] != got[moved]).any(axis=1).mean() > 0.99
        assert np.array_equal(other[opaque].view(np.uint32), P["pos"][opaque].view(np.uint32))
    # added to a position, not stored over it
    P2 = dict(P, pos=rng.normal(size=(n, 3)).astype(np.float32))
    got2 = _noise(P2, n, a, 11, 40)
    assert np.array_equal(got2[moved], P2["pos"][moved] + got[moved])


@pytest.mark.parametrize("n", [4099, 180_001], ids=["a few workgroups", "every workgroup strides"])
def test_regularisers_add_their_gradients_and_sum_reproducibly(n):
    lib = abi.lib()
    rng = np.random.default_rng(31)
    P = _params(n, rng.uniform(1e-4, 0.9999, n), rng, scale=(-6.0, 1.0))
    g_o, g_s = rng.normal(size=n).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    lam_o, lam_s = 0.01, 0.02
    Lo, Ls, d_o, d_s = mo.regularisers(P["opacity_raw"], P["scale_raw"], float(np.float32(lam_o)), float(np.float32(lam_s)))
    lay = _layout(n)
    runs = []
    for base in (None, 0.75, None):
        G = {k: Guarded(v) for k, v in dict(o=P["opacity_raw"], s=P["scale_raw"], go=g_o, gs=g_s, values=np.full(3, np.nan, np.float32),
                                            base=np.array([base or 0.0], np.float32)).items()}
        scratch = Guarded(np.zeros(lay.bytes, np.uint8))
        torch.cuda.synchronize()
        for _ in range(2 if base is None else 1):          # (twice on one scratch: the counter is left at zero)
            status = lib.gsplat_mcmc_regularise(n, G["o"].ptr, G["s"].ptr, G["go"].ptr, G["gs"].ptr, lam_o, lam_s, G["base"].ptr if base else None,
                                                G["values"].ptr, scratch.ptr, None)
            assert status == abi.GSPLAT_OK, lib.gsplat_last_error()
        torch.cuda.synchronize()
        assert scratch.intact() and all(x.intact() for x in G.values())
        assert not scratch.host()[lay.reg:lay.reg + 4].any()
        times = 2 if base is None else 1
        vals = G["values"].host().astype(np.float64)
        for got, want in ((G["go"].host(), g_o + times * d_o), (G["gs"].host(), g_s + times * d_s)):
            assert (np.abs(got.astype(np.float64) - want) <= RTOL * np.abs(want)).all()
        assert abs(vals[0] - Lo) <= RTOL * Lo and abs(vals[1] - Ls) <= RTOL * Ls and abs(vals[2] - ((base or 0.0) + Lo + Ls)) <= RTOL * vals[2]
        runs.append((G["values"].host().copy(), G["go"].host().copy(), G["gs"].host().copy()))
    for x, y in zip(runs[0], runs[2]):                     # a second run: the same bits, values and gradients
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # values only (no gradient arrays): the same values, nothing else written
    vals = Guarded(np.zeros(3, np.float32))
    scratch = Guarded(np.zeros(lay.bytes, np.uint8))
    o, s = Guarded(P["opacity_raw"]), Guarded(P["scale_raw"])
    assert lib.gsplat_mcmc_regularise(n, o.ptr, s.ptr, None, None, lam_o, lam_s, None, vals.ptr, scratch.ptr, None) == abi.GSPLAT_OK
    torch.cuda.synchronize()
    assert np.array_equal(vals.host().view(np.uint32), runs[0][0].view(np.uint32)) and vals.intact() and scratch.intact()


# ---- the trainer's "mcmc" rule ------------------------------------------------------------------------------------------------
def _scene(render_targets=True):
    """The small scene of tests/test_gpu_training.py: case g1 from two cameras; targets = renders of the true scene."""
    gs = importlib.import_module(PKG)
    s = scenes.case_g1()
    rng = np.random.default_rng(5)
    cams = [s["c2w"], scenes._camera(rng)]
    views = [dict(image=None, c2w=c, H=s["H"], W=s["W"], fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"]) for c in cams]
    truth = {k: torch.tensor(s[k], device=DEV) for k in NAMES}
    with torch.no_grad():
        for v in views:
            v["image"] = gs.render_gaussians(truth["pos"], truth["f_dc"], truth["f_rest"], truth["opacity_raw"], truth["scale_raw"], truth["q_raw"],
                                             torch.tensor(v["c2w"], device=DEV), v["H"], v["W"], v["fx"], v["fy"], v["cx"], v["cy"]).cpu().numpy()
    g = torch.Generator().manual_seed(3)
    init = {k: torch.tensor(s[k]) for k in NAMES}
    init["f_dc"] = init["f_dc"] + 0.5 * torch.randn(init["f_dc"].shape, generator=g)
    init["opacity_raw"] = init["opacity_raw"] - 0.5
    return init, views


def _train(views_of, iterations, **cfg_kw):
    model_mod = importlib.import_module(PKG + ".model")
    training = importlib.import_module(PKG + ".training")
    init, views = _scene()
    n0 = init["pos"].shape[0]
    cfg = training.TrainConfig(densify_rule="mcmc", mcmc_start_iter=0, densification_interval=5, cap_max=int(1.2 * n0), **cfg_kw)
    model = model_mod.GaussianModel(init, device=DEV)
    tr = training.Trainer(model, cfg)
    opt = tr.optimizer
    outs = [tr.step(it, views_of(views)) for it in range(iterations)]
    torch.cuda.synchronize()
    assert tr.optimizer is opt
    return model, tr, outs, n0, cfg


def test_mcmc_rule_trains_at_a_fixed_budget_and_keeps_the_optimiser():
    model, tr, outs, n0, cfg = _train(lambda v: v, 30)
    counts = [o["gaussians"] for o in outs]
    assert counts[0] == min(cfg.cap_max, int(1.05 * n0)) > n0
    assert all(b >= a for a, b in zip(counts, counts[1:])) and counts[-1] == cfg.cap_max == max(counts)
    assert [o["densified"] for o in outs] == [it % 5 == 0 for it in range(30)]
    losses = [float(o["loss"]) for o in outs]
    assert all(np.isfinite(losses))
    for o in outs[-3:]:
        total = float(o["l1"]) * cfg.lambda_l1 + float(o["ssim"]) * cfg.lambda_ssim
        assert float(o["reg_opacity"]) > 0 and float(o["reg_scale"]) > 0
        assert abs(float(o["loss"]) - (total + float(o["reg_opacity"]) + float(o["reg_scale"]))) <= 1e-5 * float(o["loss"])
    for k, g in zip(NAMES, tr.optimizer.param_groups):
        p = getattr(model, k)
        assert g['params'][0] is p and p.shape[0] == cfg.cap_max and torch.isfinite(p).all()
        st = tr.optimizer.state[p]
        assert st['step'] == 30 and st['exp_avg'].shape == p.shape and torch.isfinite(st['exp_avg']).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), (losses[:5], losses[-5:])


def test_mcmc_rule_is_bit_reproducible_under_set_deterministic():
    gs = importlib.import_module(PKG)
    old = gs.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            model, tr, outs, _, _ = _train(lambda v: v, 12)
            runs.append(({k: getattr(model, k).detach().cpu() for k in NAMES},
                         {k: (tr.optimizer.state[getattr(model, k)]['exp_avg'].cpu(), tr.optimizer.state[getattr(model, k)]['exp_avg_sq'].cpu())
                          for k in NAMES}, [float(o["loss"]) for o in outs]))
    finally:
        gs.set_deterministic(old)
    assert runs[0][2] == runs[1][2]
    for k in NAMES:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
        assert torch.equal(runs[0][1][k][0], runs[1][1][k][0]) and torch.equal(runs[0][1][k][1], runs[1][1][k][1]), k


@pytest.mark.parametrize("mode", ["one view, folded step", "one view, separate step", "aux pass", "two views on one stream"])
def test_mcmc_rule_runs_with_the_other_routes(mode):
    kw = {"one view, folded step": dict(fold_rest_step=True), "one view, separate step": dict(fold_rest_step=False),
          "aux pass": dict(background=(0.1, 0.2, 0.3)), "two views on one stream": dict(view_streams=1, sum_views_in_kernel=False)}[mode]
    pick = (lambda v: v[:1]) if mode.startswith("one view") else (lambda v: v)
    model, tr, outs, n0, cfg = _train(pick, 7, **kw)
    assert outs[-1]["gaussians"] == min(cfg.cap_max, int(1.05 * int(1.05 * n0))) and outs[5]["densified"] and not outs[6]["densified"]
    assert all(np.isfinite(float(o["loss"])) for o in outs)
    for k in NAMES:
        p = getattr(model, k)
        assert torch.isfinite(p).all() and tr.optimizer.state[p]['step'] == 7, k
    if mode == "aux pass":
        assert "l_alpha" in outs[-1]


def _dp_worker(rank, world):
    model_mod = importlib.import_module(PKG + ".model")
    training = importlib.import_module(PKG + ".training")
    init, views = _scene()
    model = model_mod.GaussianModel(init, device=DEV)
    n0 = init["pos"].shape[0]
    tr = training.Trainer(model, training.TrainConfig(densify_rule="mcmc", mcmc_start_iter=0, densification_interval=3, cap_max=int(1.2 * n0)))
    opt, refined = tr.optimizer, 0
    for it in range(1, 7):                   # iterations 3 and 6 refine: the replicas must stay identical through both
        out = tr.step(it, [views[rank]], global_views=world)
        refined += out["densified"]
    torch.cuda.synchronize()
    return ({k: getattr(model, k).detach().cpu().numpy() for k in NAMES},
            {k: tr.optimizer.state[getattr(model, k)]['exp_avg'].cpu().numpy() for k in NAMES}, out["gaussians"], refined, tr.optimizer is opt)


def test_data_parallel_ranks_stay_bit_identical_through_two_refinements():
    got = run_ranks(_dp_worker, 2)
    n0 = scenes.case_g1()["pos"].shape[0]
    assert got[0][2] == got[1][2] == int(1.05 * int(1.05 * n0)) and got[0][3] == got[1][3] == 2 and got[0][4] and got[1][4]
    for k in NAMES:
        assert np.array_equal(got[0][0][k].view(np.uint32), got[1][0][k].view(np.uint32)), k
        assert np.array_equal(got[0][1][k].view(np.uint32), got[1][1][k].view(np.uint32)), k
        assert np.isfinite(got[0][0][k]).all()
