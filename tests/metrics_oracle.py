"""float64 numpy restatement of the image metrics, written from the definitions alone:

    l1 = sum_valid |x - y| / (3 n),  mse = sum_valid (x - y)^2 / (3 n),  psnr = -10 log10(mse) (+inf for mse == 0),
    ssim = mean over the valid pixels and the channels of the SSIM map (11 x 11 Gaussian window, sigma 1.5, separable, zero padding,
           C1 = 0.01^2, C2 = 0.03^2, per channel; the map is computed from the whole images),
    n == 0: NaN.  Colour correction: (A + l n D) P = C + l n [I3; 0], A = sum_valid xt xt^T, C = sum_valid xt y^T, xt = [x; 1],
    D = diag(1, 1, 1, 0), l = 1e-8, [M | t] = P^T; the metrics are then those of clamp(M x + t, 0, 1) against y.
The SSIM map is the textbook one (covariances from E[xy]), not the kernels' regrouping."""
import numpy as np

RIDGE = 1e-8
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _band(n):
    """[n, n]: row i holds the window centred on i, cut off at the border (= zero padding)."""
    d = np.arange(n)[None, :] - np.arange(n)[:, None] + 5
    return np.where((d >= 0) & (d < 11), window()[np.clip(d, 0, 10)], 0.0)


def blur(a):
    """The windowed sum of a [H, W, ...] array with zero padding: rows, then columns."""
    a = np.asarray(a, dtype=np.float64)
    return np.moveaxis(np.tensordot(_band(a.shape[1]), np.tensordot(_band(a.shape[0]), a, axes=(1, 0)), axes=(1, 1)), 0, 1)


def ssim_map(x, y):
    """[H, W, 3] -> [H, W, 3]"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mu1, mu2 = blur(x), blur(y)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def normal_equations(x, y, valid):
    """(A [4, 4] with the ridge, C [4, 3] with the ridge, n) of one image."""
    xs, ys = x[valid].reshape(-1, 3), y[valid].reshape(-1, 3)
    n = xs.shape[0]
    xt = np.concatenate([xs, np.ones((n, 1))], 1)
    A, C = xt.T @ xt, xt.T @ ys
    A[:3, :3] += RIDGE * n * np.eye(3)
    C[:3] += RIDGE * n * np.eye(3)
    return A, C, n


def fit_affine(x, y, valid=None):
    """[3, 4] = [M | t] of one image (NaN without a valid pixel)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    valid = np.ones(x.shape[:2], dtype=bool) if valid is None else np.asarray(valid) != 0
    A, C, n = normal_equations(x, y, valid)
    if n == 0:
        return np.full((3, 4), np.nan)
    return np.linalg.solve(A, C).T


def one_image(x, y, valid=None, colour_correct=False):
    """{'psnr', 'ssim', 'l1', 'mse', 'affine', 'map'} of one image [H, W, 3]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    valid = np.ones(x.shape[:2], dtype=bool) if valid is None else np.asarray(valid) != 0
    n = int(valid.sum())
    affine = None
    if colour_correct:
        affine = fit_affine(x, y, valid)
        if n:
            x = np.clip(x @ affine[:, :3].T + affine[:, 3], 0.0, 1.0)
    if n == 0:
        nan = float("nan")
        return dict(psnr=nan, ssim=nan, l1=nan, mse=nan, affine=affine, map=None)
    smap = ssim_map(x, y)
    d = (x - y)[valid]
    mse = float((d * d).sum() / (3 * n))
    with np.errstate(divide="ignore"):
        psnr = float(-10.0 * np.log10(mse)) if mse > 0 else float("inf")
    return dict(psnr=psnr, ssim=float(smap[valid].sum() / (3 * n)), l1=float(np.abs(d).sum() / (3 * n)), mse=mse, affine=affine, map=smap)


def image_metrics(pred, target, mask=None, colour_correct=False):
    """pred, target [B, H, W, 3] (or [H, W, 3]), mask [B, H, W] or None -> dict of [B] float64 arrays (+ 'affine' [B, 3, 4] or None)."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if pred.ndim == 3:
        pred, target, mask = pred[None], target[None], (None if mask is None else np.asarray(mask)[None])
    rows = [one_image(pred[b], target[b], None if mask is None else mask[b], colour_correct) for b in range(pred.shape[0])]
    out = {k: np.array([r[k] for r in rows], dtype=np.float64) for k in ("psnr", "ssim", "l1", "mse")}
    out["affine"] = np.stack([r["affine"] for r in rows]) if colour_correct else None
    return out
