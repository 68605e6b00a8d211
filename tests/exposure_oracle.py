"""The exposure transform in numpy float64: out = M c + t per pixel, and its two gradients.  The yardstick of
tests/test_exposure_cpu.py and tests/test_gpu_exposure.py; it reads nothing but its arguments."""
import numpy as np


def _batched(image, params, g_out=None):
    image, params = np.asarray(image, dtype=np.float64), np.asarray(params, dtype=np.float64)
    single = image.ndim == 3
    if single:
        image, params = image[None], params[None]
    assert image.ndim == 4 and image.shape[-1] == 3 and params.shape == (image.shape[0], 3, 4), (image.shape, params.shape)
    if g_out is not None:
        g_out = np.asarray(g_out, dtype=np.float64).reshape(image.shape)
    return image, params, g_out, single


def forward(image, params):
    """out[..., r] = sum_k M[r, k] c[k] + t[r]: image [H, W, 3] with params [3, 4], or [B, H, W, 3] with [B, 3, 4]."""
    x, e, _, single = _batched(image, params)
    out = np.einsum("brk,bhwk->bhwr", e[:, :, :3], x) + e[:, None, None, :, 3]
    return out[0] if single else out


def magnitude(image, params):
    """sum_k |M[r, k] c[k]| + |t[r]| per element of out: what the forward's rounding bound is a multiple of."""
    x, e, _, single = _batched(image, params)
    out = np.einsum("brk,bhwk->bhwr", np.abs(e[:, :, :3]), np.abs(x)) + np.abs(e[:, None, None, :, 3])
    return out[0] if single else out


def backward(image, params, g_out):
    """(g_image, g_params): g_image[..., k] = sum_r M[r, k] g_out[..., r];  g_params[r, k] = sum over the pixels of g_out[r] c[k]
    (k < 3) and g_params[r, 3] = sum over the pixels of g_out[r], per image."""
    x, e, g, single = _batched(image, params, g_out)
    g_image = np.einsum("brk,bhwr->bhwk", e[:, :, :3], g)
    g_params = np.concatenate([np.einsum("bhwr,bhwk->brk", g, x), g.sum(axis=(1, 2))[:, :, None]], axis=2)
    return (g_image[0], g_params[0]) if single else (g_image, g_params)


def backward_magnitude(image, params, g_out):
    """(sum_r |M[r, k] g_out[r]| per element of g_image,  sum over the pixels of |g_out[r] c[k]| (|g_out[r]| for k = 3) per parameter)."""
    x, e, g, single = _batched(image, params, g_out)
    a, b = backward(np.abs(x), np.abs(e), np.abs(g))
    return (a[0], b[0]) if single else (a, b)
