"""The float64 oracle of the bilateral grids (tests/bilagrid_oracle.py) against torch float64 autograd through F.grid_sample, the
total variation against a few lines of torch, the identity, and the zero luminance derivative at exactly black and white pixels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bilagrid_oracle as bo


def _torch_slice(image, grids):
    """The issue's definition: grid_sample(G[None], 2 (x, y, z) - 1, bilinear, align_corners, border) and the affine; [H, W, 3]."""
    H, W, _ = image.shape
    x = ((torch.arange(W, dtype=torch.float64) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, dtype=torch.float64) + 0.5) / H)[:, None].expand(H, W)
    lum = 0.299 * image[..., 0] + (0.587 * image[..., 1] + 0.114 * image[..., 2])
    at = 2.0 * torch.stack([x, y, lum.clamp(0.0, 1.0)], dim=-1) - 1.0
    A = F.grid_sample(grids[None], at[None, None], mode="bilinear", align_corners=True, padding_mode="border")[0, :, 0]     # [12, H, W]
    A = A.permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] * image[..., None, :]).sum(-1) + A[..., 3]


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 4), (16, 16, 8)])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (7, 9)])
def test_oracle_matches_torch_float64_autograd_through_grid_sample(h, w, shape):
    image, grids, g_out = (a[0] for a in bo.random_case(11, 1, h, w, shape))
    x = torch.tensor(image, requires_grad=True)
    g = torch.tensor(grids, requires_grad=True)
    out = _torch_slice(x, g)
    out.backward(torch.tensor(g_out))
    assert np.allclose(bo.forward(image, grids), out.detach().numpy(), rtol=0, atol=1e-13)
    g_image, g_grids = bo.backward(image, grids, g_out)
    assert np.allclose(g_image, x.grad.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(g_grids, g.grad.numpy(), rtol=0, atol=1e-12 * h * w)
    # the batched form is the stack of the single ones
    both = bo.random_case(12, 2, h, w, shape)
    out2 = bo.forward(*both[:2])
    gi2, gg2 = bo.backward(*both)
    for b in range(2):
        assert np.array_equal(out2[b], bo.forward(both[0][b], both[1][b]))
        gi, gg = bo.backward(both[0][b], both[1][b], both[2][b])
        assert np.array_equal(gi2[b], gi) and np.array_equal(gg2[b], gg)


def test_the_generator_leaves_no_pixel_near_a_level_and_keeps_clamped_ones():
    image, _, _ = bo.random_case(13, 3, 17, 33, (16, 16, 8))
    lum = bo.luminance(image)
    z = np.clip(lum, 0, 1) * 7
    inner = (lum > 0) & (lum < 1)
    assert (np.abs(z - np.round(z))[inner] >= bo.Z_GUARD).all()
    assert (lum <= 0).any() and (lum >= 1).any()
    again, _, _ = bo.random_case(13, 3, 17, 33, (16, 16, 8))
    assert np.array_equal(image, again)


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 4), (16, 16, 8)])
def test_tv_matches_torch(shape):
    X, Y, L = shape
    table = np.random.default_rng(14).normal(0, 1, (3, 12, L, Y, X))
    t = torch.tensor(table, requires_grad=True)
    want = sum(torch.diff(t, dim=a).pow(2).mean(dim=(1, 2, 3, 4)).sum() for a in (2, 3, 4)) / 3
    want.backward()
    got, grad = bo.tv(table)
    assert abs(got - float(want)) <= 1e-13 * float(want)
    assert np.allclose(grad, t.grad.numpy(), rtol=0, atol=1e-14)
    m, mg = bo.tv_magnitude(table)
    assert m >= got and (mg >= np.abs(grad) - 1e-15).all()
    zero, zgrad = bo.tv(bo.identity(3, shape))
    assert zero == 0.0 and not zgrad.any()


def test_identity_and_magnitudes():
    image, grids, g_out = bo.random_case(15, 2, 5, 7, (3, 5, 4))
    eye = bo.identity(2, (3, 5, 4))
    assert np.allclose(bo.forward(image, eye), image, rtol=0, atol=1e-15)
    g_image, g_grids = bo.backward(image, eye, g_out)
    assert np.allclose(g_image, g_out, rtol=0, atol=1e-15)
    # the eight weights of a pixel add up to one: the grid gradient adds up to the sum of g_o (x) [c, 1]
    assert np.allclose(g_grids.reshape(2, 3, 4, -1).sum(-1)[:, :, 3], g_out.sum(axis=(1, 2)))
    assert (bo.magnitude(image, grids) >= np.abs(bo.forward(image, grids)) - 1e-15).all()
    m_image, m_grids = bo.backward_magnitude(image, grids, g_out)
    gi, gg = bo.backward(image, grids, g_out)
    assert (m_image >= np.abs(gi) - 1e-14).all() and (m_grids >= np.abs(gg) - 1e-12).all()


def test_black_and_white_pixels_get_no_luminance_derivative():
    """grid_sample's rule at the border: where the unclamped luminance is <= 0 or >= 1 the coordinate's gradient is zero -- exactly
    black (luminance 0) and exactly white (luminance exactly 1 in this nesting) included; torch agrees."""
    _, grids, _ = (a[0] for a in bo.random_case(16, 1, 4, 4, (3, 5, 4), spread=0.5))
    image = np.zeros((4, 4, 3))
    image[1] = 1.0
    image[2] = (1.5, 1.2, 0.9)
    image[3] = (0.25, 0.5, 0.75)
    assert (bo.luminance(image)[0] == 0).all() and (bo.luminance(image)[1] == 1).all()
    g_out = np.random.default_rng(17).normal(0, 1, (4, 4, 3))
    g_image, _ = bo.backward(image, grids, g_out)
    A = bo._slice(grids[None], *bo._locate(image[None], 3, 5, 4)[:3])[0][0].reshape(4, 4, 3, 4)
    plain = (A[..., :3] * g_out[..., :, None]).sum(-2)
    assert np.array_equal(g_image[:3], plain[:3])                 # black, white, beyond white: the affine's transpose alone
    assert (np.abs(g_image[3] - plain[3]) > 1e-6).any()           # an inner pixel: the luminance term is there
    x = torch.tensor(image, requires_grad=True)
    _torch_slice(x, torch.tensor(grids)).backward(torch.tensor(g_out))
    assert np.allclose(g_image, x.grad.numpy(), rtol=0, atol=1e-12)
