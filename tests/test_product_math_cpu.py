"""CPU unit test of the product's per-Gaussian projection math (csrc/gs_math.h, gs_body.h).

The header is compiled for the host (csrc/host_math_check.cpp -> libgsmath_host.so) and compared with
(a) the per-stage intermediates the real reference produced (tests/golden) and (b) autograd through the
oracle's per-Gaussian stage.  This is a test of product code on the CPU, not a product fallback.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import listcheck, util
from tests.cpu_frame import hm, oracle_stage_grads, project, ptr, row_spans  # noqa: F401  (hm is a fixture)

abi = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd._abi")


@pytest.mark.parametrize("name", util.RENDER_CASES)
def test_forward_records_vs_reference_intermediates(hm, name):
    d = util.load(name)
    arrs = {k: np.ascontiguousarray(d[k], np.float32) for k in util.PARAMS}
    rec, tiles, vis, view, *_ = project(hm, d, arrs)
    listcheck.check_records(d, rec[0], rec[1], rec[2], tiles, np.nonzero(vis == 0)[0], rec[4], rec[5], rec[6], ref_rect=rec[3],
                            row_spans=row_spans(hm, rec, view, d["im_ids"]))


@pytest.mark.parametrize("name", util.RENDER_CASES)
def test_backward_fused_vs_oracle_autograd(hm, name):
    d = util.load(name)
    arrs = {k: np.ascontiguousarray(d[k], np.float32) for k in util.PARAMS}
    g2d, ref = oracle_stage_grads(d)
    rec, tiles, vis, view, g, c2w = project(hm, d, arrs)
    out = {k: np.full_like(arrs[k], np.nan) for k in util.PARAMS}
    gg = abi.GaussianGrads(ptr(out["pos"]), ptr(out["opacity_raw"]), None, None, ptr(out["scale_raw"]),
                           ptr(out["q_raw"]), ptr(out["f_dc"]), ptr(out["f_rest"]))
    hm.hm_project_backward(C.byref(g), ptr(c2w), C.byref(view), ptr(tiles), ptr(g2d), C.byref(gg))   # tiles: visibility flag
    for k, r in zip(util.PARAMS, ref):
        util.check_grad(out[k], r, k)


def test_backward_unfused_vs_oracle_autograd(hm):
    d = util.load("g11_unfused")
    arrs = {k: np.ascontiguousarray(d[k], np.float32) for k in util.PARAMS}
    color = np.ascontiguousarray(d["color_in"], np.float32)
    sigma = np.ascontiguousarray(d["sigma_in"], np.float32)
    g2d, ref = oracle_stage_grads(d, fused=False, color=color, sigma=sigma)
    rec, tiles, vis, view, g, c2w = project(hm, d, arrs, fused=False, color=color, sigma=sigma)
    out = dict(pos=np.full_like(arrs["pos"], np.nan), opacity_raw=np.full_like(arrs["opacity_raw"], np.nan),
               color=np.full_like(color, np.nan), sigma=np.full_like(sigma, np.nan))
    gg = abi.GaussianGrads(ptr(out["pos"]), ptr(out["opacity_raw"]), ptr(out["color"]), ptr(out["sigma"]), None, None,
                           None, None)
    hm.hm_project_backward(C.byref(g), ptr(c2w), C.byref(view), ptr(tiles), ptr(g2d), C.byref(gg))   # tiles: visibility flag
    for k, r in zip(("pos", "opacity_raw", "color", "sigma"), ref):
        util.check_grad(out[k], r, k)


def test_pieces_forward_backward(hm):
    d = dict(np.load(util.GOLDEN + "/pieces.npz"))
    n = len(d["scale_raw"])

    def f32(a):
        return np.ascontiguousarray(a, np.float32)

    sr, qr = f32(d["scale_raw"]), f32(d["q_raw"])
    sig = np.zeros((n, 3, 3), np.float32)
    hm.hm_build_sigma(C.c_int64(n), ptr(sr), ptr(qr), ptr(sig))
    assert np.abs(sig - d["sigma"]).max() <= 2e-6 * np.abs(d["sigma"]).max()
    gs, gq = np.zeros_like(sr), np.zeros_like(qr)
    w = f32(d["w_sigma"])
    hm.hm_build_sigma_backward(C.c_int64(n), ptr(sr), ptr(qr), ptr(w), ptr(gs), ptr(gq))
    util.check_grad(gs, d["grad_scale_raw"], "scale_raw", l2=1e-5, mx=1e-5)
    util.check_grad(gq, d["grad_q_raw"], "q_raw", l2=1e-5, mx=1e-5)
    fd, fr, pt, c2w = f32(d["f_dc"]), f32(d["f_rest"]), f32(d["points"]), f32(d["c2w"])
    col = np.zeros((n, 3), np.float32)
    hm.hm_evaluate_sh(C.c_int64(n), ptr(fd), ptr(fr), ptr(pt), ptr(c2w), ptr(col))
    assert np.abs(col - d["color"]).max() < 1e-6
    gfd, gfr, gpt = np.zeros_like(fd), np.zeros_like(fr), np.zeros_like(pt)
    wc = f32(d["w_col"])
    hm.hm_evaluate_sh_backward(C.c_int64(n), ptr(fd), ptr(fr), ptr(pt), ptr(c2w), ptr(wc), ptr(gfd), ptr(gfr), ptr(gpt))
    util.check_grad(gfd, d["grad_f_dc"], "f_dc", l2=1e-5, mx=1e-5)
    util.check_grad(gfr, d["grad_f_rest"], "f_rest", l2=1e-5, mx=1e-5)
    util.check_grad(gpt, d["grad_points"], "points", l2=1e-5, mx=2e-5)


def test_rotation_gradient_of_near_isotropic_gaussians_is_cancellation_free(hm):
    """dL/dq_raw of Sigma = R D R^T vanishes as the scales approach each other; by the plain chain rule through quat_to_rot it is a
    difference of terms of size |G| d, and its relative error grows like 1e-7 / |r_i - r_j| (the reference's own fp32 autograd
    has exactly that: 1e-4 at a log-scale spread of 1e-3).  cov_from_params_backward forms it from the torque
    2 G'_ij (d_i - d_j), d_i - d_j = d_j expm1(2 (r_i - r_j)): accurate to fp32 rounding at every spread, and still the chain rule's
    value where |q_raw| is as small as the reference's eps."""
    rng = np.random.default_rng(0)
    n = 4000
    for spread, bound in ((0.3, 2e-6), (1e-2, 2e-6), (1e-3, 1e-5), (1e-4, 1e-4)):
        sr = (rng.normal(-2, 0.5, (n, 1)) + rng.normal(0, 1, (n, 3)) * spread).astype(np.float32)
        qr = rng.normal(0, 1, (n, 4)).astype(np.float32)
        w = rng.normal(0, 1, (n, 3, 3)).astype(np.float32)
        a = torch.tensor(sr, dtype=torch.float64, requires_grad=True)
        b = torch.tensor(qr, dtype=torch.float64, requires_grad=True)
        (tp.covariance_from_params(a, b) * torch.tensor(w, dtype=torch.float64)).sum().backward()
        gs, gq = np.zeros_like(sr), np.zeros_like(qr)
        hm.hm_build_sigma_backward(C.c_int64(n), ptr(sr), ptr(qr), ptr(w), ptr(gs), ptr(gq))
        ref = b.grad.numpy()
        err = np.linalg.norm(gq - ref) / np.linalg.norm(ref)
        assert err <= bound, (spread, err)
        assert np.linalg.norm(gs - a.grad.numpy()) / np.linalg.norm(a.grad.numpy()) <= 1e-6
    # tiny quaternions: the normalisation's eps matters, R(q) is no rotation -> the chain-rule branch, same values as autograd
    qr = (rng.normal(0, 1, (n, 4)) * 1e-6).astype(np.float32)
    sr = rng.normal(-2, 0.5, (n, 3)).astype(np.float32)
    a = torch.tensor(sr, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(qr, dtype=torch.float64, requires_grad=True)
    (tp.covariance_from_params(a, b) * torch.tensor(w, dtype=torch.float64)).sum().backward()
    gs, gq = np.zeros_like(sr), np.zeros_like(qr)
    hm.hm_build_sigma_backward(C.c_int64(n), ptr(sr), ptr(qr), ptr(w), ptr(gs), ptr(gq))
    assert np.linalg.norm(gq - b.grad.numpy()) / np.linalg.norm(b.grad.numpy()) <= 1e-5
    # clamped scales (exp(scale_raw) < 1e-6): differences of the clamped values
    sr = rng.normal(-14.5, 0.6, (n, 3)).astype(np.float32)
    qr = rng.normal(0, 1, (n, 4)).astype(np.float32)
    a = torch.tensor(sr, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(qr, dtype=torch.float64, requires_grad=True)
    (tp.covariance_from_params(a, b) * torch.tensor(w, dtype=torch.float64)).sum().backward()
    gs, gq = np.zeros_like(sr), np.zeros_like(qr)
    hm.hm_build_sigma_backward(C.c_int64(n), ptr(sr), ptr(qr), ptr(w), ptr(gs), ptr(gq))
    assert np.linalg.norm(gq - b.grad.numpy()) / np.linalg.norm(b.grad.numpy()) <= 1e-4


def test_rotation_gradient_of_small_quaternions_either_side_of_the_branch(hm):
    """cov_from_params_backward takes the torque form (which presumes a unit quaternion) only where the normalisation's eps is
    below fp32 rounding beside |q_raw|: with the branch at 1e-4 the gradient just above it was 4e-5 off (found on the device by
    tests/test_gpu_pieces.py::test_build_sigma_kernels_vs_float64).  1e-5, the bound of test_pieces_forward_backward, at every norm."""
    rng = np.random.default_rng(1)
    n = 2000
    for norm in (1e-6, 0.99e-4, 1.01e-4, 3e-4, 1e-3, 0.99e-2, 1.01e-2, 3e-2, 1.0):
        sr = rng.normal(-2, 0.5, (n, 3)).astype(np.float32)
        qr = rng.normal(0, 1, (n, 4))
        qr = (qr / np.linalg.norm(qr, axis=1, keepdims=True) * norm).astype(np.float32)
        w = rng.normal(0, 1, (n, 3, 3)).astype(np.float32)
        a = torch.tensor(sr, dtype=torch.float64, requires_grad=True)
        b = torch.tensor(qr, dtype=torch.float64, requires_grad=True)
        (tp.covariance_from_params(a, b) * torch.tensor(w, dtype=torch.float64)).sum().backward()
        gs, gq = np.zeros_like(sr), np.zeros_like(qr)
        hm.hm_build_sigma_backward(C.c_int64(n), ptr(sr), ptr(qr), ptr(w), ptr(gs), ptr(gq))
        err = np.linalg.norm(gq - b.grad.numpy()) / np.linalg.norm(b.grad.numpy())
        print(norm, err)
        assert err <= 1e-5, (norm, err)


def test_conic_of_needle_gaussians_has_no_determinant_cancellation(hm):
    """A Gaussian 100 x longer than wide projects to a 2-D covariance whose determinant a d - b^2 cancels 4 digits in float32 (stress
    seed 794: eigenvalues 0.17 and 1200 px^2; the reference's own fp32 conic is 9e-5 off there, a d - b^2 here was 5e-4 off).
    With the fused inputs the determinant is the sum of squares sum_k (s_i s_j (Q^T n)_k)^2: the conic is good to a few ulp at
    every aspect ratio.  The float32 oracle is timed beside it: the bound is not one the reference's arithmetic meets."""
    rng = np.random.default_rng(7)
    n = 3000
    H, W, fx = 200, 300, 250.0
    for aspect_log, bound in ((2.0, 2e-5), (4.0, 2e-5), (5.0, 2e-5)):
        pos = np.concatenate([rng.uniform(-1.0, 1.0, (n, 2)), rng.uniform(3.0, 6.0, (n, 1))], 1).astype(np.float32)
        sr = rng.normal(-4.0, 0.3, (n, 3)).astype(np.float32)
        sr[np.arange(n), rng.integers(0, 3, n)] += aspect_log                  # one long axis
        arrs = dict(pos=pos, scale_raw=sr, q_raw=rng.normal(0, 1, (n, 4)).astype(np.float32), opacity_raw=rng.normal(1, 1, n).astype(np.float32),
                    f_dc=rng.normal(0, 1, (n, 3)).astype(np.float32), f_rest=np.zeros((n, 45), np.float32))
        d = dict(c2w=np.eye(4, dtype=np.float32), H=H, W=W, fx=fx, fy=fx, cx=W / 2, cy=H / 2, kwargs={})
        rec, tiles, vis, *_ = project(hm, d, arrs)
        res = {}
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            st = {}
            tp.render_fused(*[torch.tensor(arrs[k]).to(dt) for k in ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")],
                            torch.eye(4, dtype=dt), H, W, fx, fx, W / 2, H / 2, stages=st, stop_after_binning=True)
            res[tag] = (st["ids"].numpy(), st["conic"].double().numpy(), st["evals"].double().numpy())
        ids, con, ev = res["f64"]
        inside = (ev[:, 0] > 2e-6) & (ev[:, 1] < 0.99e4)                        # the eigen clamp is a different matter (F8)
        assert inside.sum() > n // 8 and (ev[inside, 1] / ev[inside, 0]).max() > 10 ** (0.8 * aspect_log)
        mine = np.stack([rec[0][ids, 2], rec[0][ids, 3], rec[1][ids, 0]], 1).astype(np.float64)
        err = (np.abs(mine - con).max(1) / np.abs(con).max(1))[inside]
        assert err.max() <= bound, (aspect_log, err.max())
        ids32, con32, _ = res["f32"]
        common = np.intersect1d(ids[inside], ids32)
        e32 = np.abs(con32[np.searchsorted(ids32, common) if np.all(np.diff(ids32) > 0) else [list(ids32).index(i) for i in common]] -
                     con[[list(ids).index(i) for i in common]]).max(1) / np.abs(con[[list(ids).index(i) for i in common]]).max(1)
        print(aspect_log, "host build", err.max(), "float32 oracle", e32.max(), "largest condition number", (ev[inside, 1] / ev[inside, 0]).max())
        if aspect_log >= 4.0:
            assert e32.max() > 10 * err.max(), (aspect_log, e32.max(), err.max())


def test_row_spans_of_large_gaussians_cover_every_pixel_inside_the_ellipse(hm):
    """gs_math.h big_row_span against brute force on random large ellipses (blobs and thin rotated needles, centres on and off the
    grid): every list of every row that holds a pixel centre with q <= chi lies inside the row's span, and the spans are tight (a
    span never reaches more than one list beyond the lists the padded ellipse touches)."""
    rng = np.random.default_rng(4)
    H, W = 400, 640
    view = abi.make_view(H, W, 100.0, 100.0, W / 2, H / 2)
    ys, xs = np.mgrid[0:H, 0:W]
    n_extra = n_lists = 0
    for trial in range(300):
        l1 = 10.0 ** rng.uniform(1.0, 3.9)                       # variances: sigma from 3 to 90 px
        l2 = l1 * 10.0 ** rng.uniform(-3.5, 0.0)
        th = rng.uniform(0, np.pi)
        c, s_ = np.cos(th), np.sin(th)
        cov = np.array([[c * c * l1 + s_ * s_ * l2, c * s_ * (l1 - l2)], [c * s_ * (l1 - l2), s_ * s_ * l1 + c * c * l2]])
        K = np.linalg.inv(cov)
        u, v = rng.uniform(-40, W + 40), rng.uniform(-40, H + 40)
        a11, a12, a22 = np.float32(K[0, 0]), np.float32(K[0, 1]), np.float32(K[1, 1])
        D = float(a11) * float(a22) - float(a12) ** 2
        if D <= 0:
            continue
        ex, ey = np.sqrt(6.25 * float(a22) / D) * 1.0001 + 0.01, np.sqrt(6.25 * float(a11) / D) * 1.0001 + 0.01
        lo_u, hi_u, lo_v, hi_v = np.floor(u - ex), np.floor(u + ex), np.floor(v - ey), np.floor(v + ey)
        if hi_u < 0 or lo_u > W - 1 or hi_v < 0 or lo_v > H - 1:
            continue
        bx0, bx1 = int(np.clip(lo_u, 0, W - 1)) // 16, int(np.clip(hi_u, 0, W - 1)) // 16
        by0, by1 = int(np.clip(lo_v, 0, H - 1)) // 8, int(np.clip(hi_v, 0, H - 1)) // 8
        h = by1 - by0 + 1
        xa, xb = np.zeros(h, np.int32), np.zeros(h, np.int32)
        r16 = np.array([u, v, a11, a12, a22, 0.5, ex, ey], np.float32)
        hm.hm_row_spans(ptr(r16), C.c_uint32(bx0 | (by0 << 16)), C.c_uint32(bx1 | (by1 << 16)), C.byref(view), ptr(xa), ptr(xb))
        du, dv = xs - float(np.float32(u)), ys - float(np.float32(v))
        q = float(a11) * du * du + 2 * float(a12) * du * dv + float(a22) * dv * dv
        inside = q <= 6.25
        loose = q <= 6.25 * 1.01 + 0.5                            # the padded region, generously
        for r in range(h):
            band = slice((by0 + r) * 8, (by0 + r) * 8 + 8)
            cols = np.nonzero(inside[band].any(0))[0]
            if len(cols):
                assert xa[r] <= cols.min() // 16 and xb[r] >= cols.max() // 16, (trial, r, xa[r], xb[r], cols.min() // 16, cols.max() // 16)
            if xb[r] >= xa[r]:
                lc = np.nonzero(loose[band].any(0))[0]
                n_lists += xb[r] - xa[r] + 1
                if len(lc):
                    n_extra += max(0, lc.min() // 16 - xa[r]) + max(0, xb[r] - lc.max() // 16)
                else:
                    n_extra += xb[r] - xa[r] + 1
    assert n_lists > 3000 and n_extra <= 0.05 * n_lists, (n_lists, n_extra)
