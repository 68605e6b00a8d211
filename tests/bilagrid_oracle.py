"""float64 numpy oracle of the per-view bilateral grids: the slice of a grid of affine colour transforms at
(pixel x, pixel y, pixel luminance), its two gradients, and the total variation of a table with its gradient -- the formulas of the
issue restated, nothing taken from the code under test.

For each result there is a MAGNITUDE: the sum of the absolute values of the terms that make it, plus the terms by which a relative
rounding of u, v or z moves the interpolation weights (|u| |d result / du| with every difference of grid values replaced by the sum
of their absolute values, likewise v and z).  A computation in fp32 that rounds each term, and each coordinate, a bounded number of
times stays within (that number) 2^-24 magnitude of the oracle.

image [B, H, W, 3], grids [B, 12, L, Y, X] (or both without the B), g_out like image.
"""
import numpy as np

LUM = np.array([0.299, 0.587, 0.114])
Z_GUARD = 2.0 ** -10


def luminance(image):
    c = np.asarray(image, dtype=np.float64)
    return 0.299 * c[..., 0] + (0.587 * c[..., 1] + 0.114 * c[..., 2])       # (this nesting gives exactly 1 for a white pixel)


def _batched(image, grids, *more):
    image, grids = np.asarray(image, dtype=np.float64), np.asarray(grids, dtype=np.float64)
    single = image.ndim == 3
    if single:
        image, grids = image[None], grids[None]
        more = tuple(np.asarray(a, dtype=np.float64)[None] for a in more)
    else:
        more = tuple(np.asarray(a, dtype=np.float64) for a in more)
    return (single, image, grids) + more


def _axis(t, n):
    k0 = np.minimum(np.floor(t), n - 2).astype(np.int64)
    return k0, t - k0


def _locate(image, X, Y, L):
    """Per pixel: the cell (z0, y0, x0), the fractions, the coordinates themselves and whether the luminance derivative is live."""
    B, H, W, _ = image.shape
    u = np.broadcast_to(((np.arange(W) + 0.5) / W * (X - 1))[None, None, :], (B, H, W))
    v = np.broadcast_to(((np.arange(H) + 0.5) / H * (Y - 1))[None, :, None], (B, H, W))
    lum = luminance(image)
    z = np.clip(lum, 0.0, 1.0) * (L - 1)
    (x0, fx), (y0, fy), (z0, fz) = _axis(u, X), _axis(v, Y), _axis(z, L)
    return (z0, y0, x0), (fz, fy, fx), (z, v, u), (lum > 0.0) & (lum < 1.0)


def _corners(cell, frac):
    """The 8 corners of every pixel's cell: ((dz, dy, dx), (z, y, x) indices, (wz, wy, wx) weights)."""
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                d = (dz, dy, dx)
                yield d, tuple(k + o for k, o in zip(cell, d)), tuple(f if o else 1.0 - f for f, o in zip(frac, d))


def _gather(grids, idx):
    """grids[b, :, z, y, x] per pixel -> [B, H, W, 12]"""
    b = np.arange(grids.shape[0])[:, None, None]
    return grids[b, :, idx[0], idx[1], idx[2]]


def _slice(grids, cell, frac, coord):
    """A [B, H, W, 12], its abs-sum, and the bound of the weights' movement: sum over axes of |coordinate| |dA / d coordinate|."""
    A = Aabs = move = 0.0
    for d, idx, w in _corners(cell, frac):
        g = _gather(grids, idx)
        A = A + (w[0] * w[1] * w[2])[..., None] * g
        Aabs = Aabs + (w[0] * w[1] * w[2])[..., None] * np.abs(g)
        for a in range(3):                       # the derivative along axis a: +-(the product of the other two weights) g
            others = [w[k] for k in range(3) if k != a]
            move = move + (np.abs(coord[a]) * others[0] * others[1])[..., None] * np.abs(g)
    return A, Aabs, move


def _dz_slice(grids, cell, frac, coord):
    """D = dA / dfz = bilinear in (y, x) of G[z0 + 1] - G[z0]; its abs-sum; the movement bound (u and v only: D is constant in z
    inside a cell)."""
    D = Dabs = move = 0.0
    for d, idx, w in _corners(cell, frac):
        g = _gather(grids, idx)
        sign = 1.0 if d[0] else -1.0
        D = D + sign * (w[1] * w[2])[..., None] * g
        Dabs = Dabs + (w[1] * w[2])[..., None] * np.abs(g)
        move = move + (np.abs(coord[1]) * w[2] + np.abs(coord[2]) * w[1])[..., None] * np.abs(g)
    return D, Dabs, move


def _with_one(image):
    return np.concatenate([image, np.ones(image.shape[:-1] + (1,))], axis=-1)


def forward(image, grids, magnitude=False):
    """out [.., H, W, 3] (or its magnitude)."""
    single, image, grids = _batched(image, grids)
    L, Y, X = grids.shape[-3:]
    cell, frac, coord, _ = _locate(image, X, Y, L)
    A, Aabs, move = _slice(grids, cell, frac, coord)
    c1 = _with_one(image)
    shape = image.shape[:-1] + (3, 4)
    if magnitude:
        out = ((Aabs + move).reshape(shape) * np.abs(c1)[..., None, :]).sum(-1)
        # a rounding of c moves z too, through the luminance: |z| already stands for it (z = (L - 1) lum)
    else:
        out = (A.reshape(shape) * c1[..., None, :]).sum(-1)
    return out[0] if single else out


def magnitude(image, grids):
    return forward(image, grids, magnitude=True)


def backward(image, grids, g_out, magnitude=False):
    """(g_image [.., H, W, 3], g_grids [.., 12, L, Y, X]) (or their magnitudes)."""
    single, image, grids, g_out = _batched(image, grids, g_out)
    B, _, L, Y, X = grids.shape
    cell, frac, coord, inside = _locate(image, X, Y, L)
    A, Aabs, moveA = _slice(grids, cell, frac, coord)
    D, Dabs, moveD = _dz_slice(grids, cell, frac, coord)
    c1 = _with_one(image)
    T = (g_out[..., :, None] * c1[..., None, :]).reshape(image.shape[:-1] + (12,))        # g_o (x) [c, 1], channel 4 r + k
    shape = image.shape[:-1] + (3, 4)
    if magnitude:
        g_image = ((Aabs + moveA).reshape(shape)[..., :3] * np.abs(g_out)[..., :, None]).sum(-2)
        dz = inside * (L - 1) * (np.abs(T) * (Dabs + moveD)).sum(-1)
        g_image = g_image + dz[..., None] * LUM
    else:
        g_image = (A.reshape(shape)[..., :3] * g_out[..., :, None]).sum(-2)
        dz = inside * (L - 1) * (T * D).sum(-1)
        g_image = g_image + dz[..., None] * LUM
    g_grids = np.zeros_like(grids)
    b = np.broadcast_to(np.arange(B)[:, None, None], image.shape[:-1])
    for d, idx, w in _corners(cell, frac):
        if magnitude:
            wt = w[0] * w[1] * w[2] + np.abs(coord[0]) * w[1] * w[2] + np.abs(coord[1]) * w[0] * w[2] + np.abs(coord[2]) * w[0] * w[1]
            val = wt[..., None] * np.abs(T)
        else:
            val = (w[0] * w[1] * w[2])[..., None] * T
        for ch in range(12):
            np.add.at(g_grids[:, ch], (b, idx[0], idx[1], idx[2]), val[..., ch])
    return (g_image[0], g_grids[0]) if single else (g_image, g_grids)


def backward_magnitude(image, grids, g_out):
    return backward(image, grids, g_out, magnitude=True)


def tv(table, magnitude=False):
    """(tv, d tv / d table) of a table [V, 12, L, Y, X] (or their magnitudes): tv = (1 / V) sum_v sum_axis mean(diff^2) over the axes
    L, Y, X, the mean over the 12 channels and all pairs along the axis."""
    G = np.asarray(table, dtype=np.float64)
    V = G.shape[0]
    total, grad = 0.0, np.zeros_like(G)
    for axis in (2, 3, 4):
        d = np.diff(G, axis=axis)
        if magnitude:
            d = np.abs(np.take(G, range(1, G.shape[axis]), axis=axis)) + np.abs(np.take(G, range(G.shape[axis] - 1), axis=axis))
        k = 1.0 / (V * (d.size // V))
        total += k * (d * d).sum()
        hi = [slice(None)] * 5
        lo = [slice(None)] * 5
        hi[axis], lo[axis] = slice(1, None), slice(None, -1)
        grad[tuple(hi)] += 2 * k * d
        grad[tuple(lo)] += (2 * k * d) if magnitude else (-2 * k * d)
    return total, grad


def tv_magnitude(table):
    return tv(table, magnitude=True)


def random_case(seed, b, h, w, shape, spread=0.2, lo=-0.1, hi=1.1):
    """(image [b, h, w, 3], grids [b, 12, L, Y, X], g_out) as float32-representable float64 arrays.  Colours reach a little outside
    [0, 1], so clamped luminances occur.  Any pixel whose z = clamp(lum) (L - 1) lies within 2^-10 of an integer is REDRAWN (from the
    same generator, until none is left): the luminance derivative jumps there, and fp32 and fp64 may land in different cells.  Pixels
    with a luminance outside (0, 1) are kept unless they fall within the guard of 0 or 1 themselves.  Nothing is skipped: every pixel
    of every case is compared."""
    X, Y, L = shape
    rng = np.random.default_rng(seed)
    image = rng.uniform(lo, hi, (b, h, w, 3)).astype(np.float32).astype(np.float64)
    while True:
        lum = luminance(image)
        z = lum * (L - 1)
        bad = (np.abs(z - np.round(z)) < Z_GUARD) & (np.round(z) >= 0) & (np.round(z) <= L - 1)
        if not bad.any():
            break
        image[bad] = rng.uniform(lo, hi, (int(bad.sum()), 3)).astype(np.float32).astype(np.float64)
    eye = np.eye(3, 4).reshape(12, 1, 1, 1)
    grids = (eye + rng.normal(0.0, spread, (b, 12, L, Y, X))).astype(np.float32).astype(np.float64)
    g_out = rng.normal(0.0, 1.0, (b, h, w, 3)).astype(np.float32).astype(np.float64)
    return image, grids, g_out


def identity(b, shape):
    X, Y, L = shape
    return np.broadcast_to(np.eye(3, 4).reshape(1, 12, 1, 1, 1), (b, 12, L, Y, X)).copy()
