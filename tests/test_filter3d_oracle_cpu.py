"""The oracle of the 3D smoothing filter (tests/filter3d_oracle.py) against independent evaluations, without a GPU: its closed-form
vector-Jacobian product against torch float64 autograd of the plain formulae, its forward against the same, and its sampling interval
against a brute-force double loop."""
import numpy as np
import torch

from tests import filter3d_oracle as fo


def _plain(scale_raw, opacity_raw, filt):
    """The issue's formulae as written, in whatever dtype the tensors have."""
    s = torch.clamp_min(torch.exp(scale_raw), 1e-6)
    f2 = (filt * filt)[:, None]
    scale_out = torch.log(torch.sqrt(s * s + f2))
    c = torch.sqrt(torch.prod(s * s, dim=1) / torch.prod(s * s + f2, dim=1))
    return scale_out, torch.logit(c * torch.sigmoid(opacity_raw))


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    scale_raw = rng.uniform(-12.0, 3.0, (n, 3))
    scale_raw[:4, 0] = [-14.5, -16.0, -20.0, -13.9]                  # under the 1e-6 clamp: the gradient is zero there
    opacity_raw = rng.uniform(-12.0, 12.0, n)
    filt = np.exp(rng.uniform(np.log(1e-5), 0.0, n))
    filt[4:7] = 0.0
    return scale_raw, opacity_raw, filt


def test_forward_and_vjp_agree_with_float64_autograd_of_the_plain_formulae():
    scale_raw, opacity_raw, filt = _inputs(50, 0)
    rng = np.random.default_rng(1)
    gs_out, go_out = rng.normal(size=(50, 3)), rng.normal(size=50)
    s = torch.tensor(scale_raw, requires_grad=True)
    o = torch.tensor(opacity_raw, requires_grad=True)
    so, oo = _plain(s, o, torch.tensor(filt))
    (so * torch.tensor(gs_out)).sum().backward(retain_graph=True)
    (oo * torch.tensor(go_out)).sum().backward()
    ref_so, ref_oo = fo.apply(scale_raw, opacity_raw, filt)
    np.testing.assert_allclose(ref_so, so.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref_oo, oo.detach().numpy(), rtol=1e-9, atol=1e-9)
    g_s, g_o = fo.apply_vjp(scale_raw, opacity_raw, filt, gs_out, go_out)
    np.testing.assert_allclose(g_s, s.grad.numpy(), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(g_o, o.grad.numpy(), rtol=1e-8, atol=1e-10)
    assert np.all(g_s[:4, 0] == 0.0)                                 # the clamp
    assert np.array_equal(g_s[4:7], gs_out[4:7]) and np.array_equal(g_o[4:7], go_out[4:7])      # f == 0: the identity
    assert np.allclose(ref_so[4:7], scale_raw[4:7], rtol=0, atol=1e-15)


def test_opacity_keeps_its_shape():
    scale_raw, opacity_raw, filt = _inputs(9, 2)
    so, oo = fo.apply(scale_raw, opacity_raw[:, None], filt)
    assert so.shape == (9, 3) and oo.shape == (9, 1)
    g_s, g_o = fo.apply_vjp(scale_raw, opacity_raw[:, None], filt, np.ones((9, 3)), np.ones((9, 1)))
    assert g_s.shape == (9, 3) and g_o.shape == (9, 1)


def test_compute_against_a_brute_force_double_loop():
    pos, views = fo.scene(5, 20, 3)
    got = fo.compute(pos, views, near=0.2, margin=0.15, rel=0.0)     # no band: sure == possible == the plain rule
    assert np.array_equal(got["t_sure"], got["t_possible"])
    want = np.full(20, np.inf)
    for k in range(20):
        p = pos[k].astype(np.float64)
        if not np.isfinite(p).all():
            continue
        for v in views:
            c2w = np.asarray(v["c2w"], dtype=np.float64)
            d = p - c2w[:3, 3]
            x, y, z = (float(sum(c2w[i, j] * d[i] for i in range(3))) for j in range(3))
            if not z > 0.2:
                continue
            u, w = v["fx"] * x / z + v["cx"], v["fy"] * y / z + v["cy"]
            if -0.15 * v["W"] <= u <= 1.15 * v["W"] and -0.15 * v["H"] <= w <= 1.15 * v["H"]:
                want[k] = min(want[k], z / max(v["fx"], v["fy"]))
    np.testing.assert_allclose(got["t_sure"], want, rtol=1e-14)
    assert got["seen_sure"].sum() >= 10 and (~got["seen_sure"]).sum() >= 5 and not got["seen_sure"][19]      # both kinds; the NaN row
    filled = fo.fill(got["t_sure"], got["seen_sure"])
    assert np.all(filled[~got["seen_sure"]] == want[np.isfinite(want)].max())
    assert np.all(fo.fill(want, np.zeros(20, dtype=bool)) == 0.0)
    band = fo.compute(pos, views)
    assert np.all(band["t_possible"] <= band["t_sure"]) and not np.any(band["seen_sure"] & ~band["seen_possible"])
    none = fo.compute(pos, [])
    assert not none["seen_possible"].any()
