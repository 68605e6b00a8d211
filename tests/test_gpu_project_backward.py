"""K8 (gsplat_project_backward) on the device, isolated from the raster backward: a hand-made grad2d of moment rows goes in, and the
gradients are compared with float64 autograd through the oracle's per-Gaussian stage.  (The host build of the same body is
checked in tests/test_product_math_cpu.py; there the rows are the 2-D gradients themselves, here they are what K7 accumulates.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import device_frame as dfm
from tests import list_scenes, util

pytestmark = pytest.mark.gpu
abi = dfm.abi
FUSED_OUT = ("pos", "opacity_raw", "scale_raw", "q_raw", "f_dc", "f_rest")


def _moments_and_reference(d, s, tiles, fused=True, color=None, sigma=None, seed=0):
    """Seeded moment rows (Mx, My, Mxx, Mxy, Myy, M0, r, g, b) for the visible Gaussians -- zero where the 2-D condition number
    exceeds 1e4 (as in _oracle_stage_grads: fp32 cannot resolve the small eigenvalue there) and where the device binned the
    Gaussian nowhere (tiles = 0: K8 treats it as culled, and K7 never gives it a gradient) -- and the float64 reference: the rows
    turned into cotangents of (u, v, conic, opacity, colour) by the relation at project_backward_core, with the oracle's conic and
    opacity, then autograd through the oracle's stage."""
    dt = torch.float64
    p = {k: torch.tensor(s[k], dtype=dt, requires_grad=True) for k in util.PARAMS}
    c2w = torch.tensor(s["c2w"], dtype=dt)
    st = {}
    if fused:
        names = list(util.PARAMS)
        leaves = [p[k] for k in names]
        tp.render_fused(p["pos"], p["f_dc"], p["f_rest"], p["opacity_raw"], p["scale_raw"], p["q_raw"], c2w, *list_scenes.cam_args(s), stages=st,
                        stop_after_binning=True, **s["kwargs"])
    else:
        col = torch.tensor(color, dtype=dt, requires_grad=True)
        sig = torch.tensor(sigma, dtype=dt, requires_grad=True)
        names, leaves = ["pos", "opacity_raw", "color", "sigma"], [p["pos"], p["opacity_raw"], col, sig]
        tp.render(p["pos"], col, p["opacity_raw"], sig, c2w, *list_scenes.cam_args(s), stages=st, stop_after_binning=True, **s["kwargs"])
    ids = st["ids"].numpy()
    n = len(s["pos"])
    rng = np.random.default_rng(seed)
    conic = st["conic"].detach().numpy()
    rows = rng.normal(0, 1, (len(ids), 9))
    rows[:, :5] /= np.abs(conic).max(1, keepdims=True) + 1.0            # every term at a similar magnitude
    ev = st["evals"].detach().numpy()
    rows[ev[:, 1] / ev[:, 0] > 1e4] = 0
    rows[tiles[ids] == 0] = 0
    g2d = np.zeros((n, 16), np.float32)
    g2d[ids, :9] = rows.astype(np.float32)
    m = g2d[ids].astype(np.float64)
    o, a11, a12, a22 = st["opacity"].detach().numpy(), conic[:, 0], conic[:, 1], conic[:, 2]
    ct_u, ct_v = o * (a11 * m[:, 0] + a12 * m[:, 1]), o * (a12 * m[:, 0] + a22 * m[:, 1])
    ct_conic = np.stack([-0.5 * o * m[:, 2], -o * m[:, 3], -0.5 * o * m[:, 4]], 1)
    outs = [st["u"], st["v"], st["conic"], st["opacity"], st["color"]]
    cts = [torch.tensor(x) for x in (ct_u, ct_v, ct_conic, m[:, 5], m[:, 6:9])]
    grads = torch.autograd.grad(outs, leaves, cts, allow_unused=True)
    return g2d, {k: (g.numpy() if g is not None else np.zeros(tuple(l_.shape))) for k, g, l_ in zip(names, grads, leaves)}


def _backward(fr, g2d, names, flags, prior=None):
    n = fr.n
    shapes = dict(pos=(n, 3), opacity_raw=(n,), scale_raw=(n, 3), q_raw=(n, 4), f_dc=(n, 3), f_rest=(n, 45), color=(n, 3), sigma=(n, 3, 3))
    out = {k: (torch.full(shapes[k], float("nan"), device=dfm.DEV) if prior is None else prior[k].clone()) for k in names}
    gg = abi.GaussianGrads(*[C.c_void_p(out[k].data_ptr()) if k in out else None
                             for k in ("pos", "opacity_raw", "color", "sigma", "scale_raw", "q_raw", "f_dc", "f_rest")])
    g = torch.tensor(g2d, device=dfm.DEV)
    abi.check(fr.lib.gsplat_project_backward(C.byref(fr.g), C.c_void_p(fr.c2w.data_ptr()), C.byref(fr.view), C.c_void_p(fr.state.data_ptr()),
                                             C.c_void_p(g.data_ptr()), C.byref(gg), flags, fr.st), "gsplat_project_backward")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", util.RENDER_CASES)
def test_project_backward_fused_with_a_known_grad2d(name):
    d = util.load(name)
    s = list_scenes.golden(name)
    fr = dfm.Frame(s)
    fr.project(dfm.F | dfm.L | dfm.J)
    tiles = fr.arrays(lists=False)["tiles"]
    g2d, ref = _moments_and_reference(d, s, tiles)
    assert np.abs(g2d).max() > 0
    plain = _backward(fr, g2d, FUSED_OUT, 0)                                        # reads the SH coefficients
    jac = _backward(fr, g2d, FUSED_OUT, abi.GSPLAT_BACKWARD_SH_JACOBIAN)            # the Jacobian the projection saved
    for tag, got in (("coefficients", plain), ("saved Jacobian", jac)):
        for k in FUSED_OUT:
            util.check_grad(got[k], ref[k], f"{k} ({tag})")
            rows = got[k].reshape(fr.n, -1)[tiles == 0]
            assert not rows.any(), f"{k} ({tag}): the row of a Gaussian that is binned nowhere is not exactly zero"
    # GSPLAT_BACKWARD_ACCUMULATE: prior + gradient, to one rounding (of the gradient, and of the sum)
    gen = torch.Generator().manual_seed(5)
    prior = {k: torch.randn(jac[k].shape, generator=gen).to(dfm.DEV) for k in FUSED_OUT}
    acc = _backward(fr, g2d, FUSED_OUT, abi.GSPLAT_BACKWARD_SH_JACOBIAN | abi.GSPLAT_BACKWARD_ACCUMULATE, prior=prior)
    for k in FUSED_OUT:
        pr = prior[k].cpu().numpy().astype(np.float64)
        want = pr + jac[k].astype(np.float64)
        ulp = 2.0 ** -23 * np.maximum(np.maximum(np.abs(pr), np.abs(jac[k])), np.abs(want))
        bad = np.argwhere(np.abs(acc[k] - want) > ulp)
        assert not len(bad), f"{k}: accumulate at {bad[0]}: {acc[k][tuple(bad[0])]!r} != {pr[tuple(bad[0])]!r} + {jac[k][tuple(bad[0])]!r}"
        assert np.array_equal(acc[k].reshape(fr.n, -1)[tiles == 0], prior[k].cpu().numpy().reshape(fr.n, -1)[tiles == 0]), k


def test_project_backward_unfused_with_a_known_grad2d():
    d = util.load("g11_unfused")
    s = list_scenes.golden("g11_unfused")
    color, sigma = np.ascontiguousarray(d["color_in"], np.float32), np.ascontiguousarray(d["sigma_in"], np.float32)
    fr = dfm.Frame(s, unfused=(color, sigma))
    fr.project(0)
    tiles = fr.arrays(lists=False)["tiles"]
    g2d, ref = _moments_and_reference(d, s, tiles, fused=False, color=color, sigma=sigma)
    names = ("pos", "opacity_raw", "color", "sigma")
    got = _backward(fr, g2d, names, 0)
    for k in names:
        util.check_grad(got[k], ref[k], k)
        assert not got[k].reshape(fr.n, -1)[tiles == 0].any(), f"{k}: the row of a Gaussian that is binned nowhere is not exactly zero"
