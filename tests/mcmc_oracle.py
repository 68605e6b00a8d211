"""Oracle of the MCMC density control: a numpy float64 and Python-integer restatement of the semantics, written for
the tests -- the reference has nothing of this.  Integers (Philox, weights, prefix sums, the draw) are exact; the real-valued
pieces take a `dtype`, so that the SAME formulas evaluated in numpy float32 give the tests their calibration: the error a
float32 evaluation on the same inputs makes against float64."""
import bisect
import fractions
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STREAM_NOISE, STREAM_RELOCATE = 0, 1
MASK32 = 0xFFFFFFFF
RELOCATE_MAX_N = 51


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] unsigned 32-bit -> [..., 4] uint32 (vectorised over the leading axes)."""
    c = [np.asarray(ctr)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) for k in range(2))
    m = np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_python(ctr, key):
    """The same on Python integers, one block: the restatement the known answers were checked with."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
    return c


def row_random(seed, rows, iteration, stream):
    rows = np.asarray(rows, dtype=np.uint64)
    ctr = np.stack([rows & np.uint64(MASK32), rows >> np.uint64(32), np.full_like(rows, iteration), np.full_like(rows, stream)], axis=-1)
    key = np.broadcast_to(np.array([seed & MASK32, (seed >> 32) & MASK32], dtype=np.uint64), rows.shape + (2,))
    return philox4x32_10(ctr, key)


def unit_open(words, dtype=np.float64):
    return ((words >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)


def normals3(words, dtype=np.float64):
    """[..., 4] words -> [..., 3] normals, every operation in `dtype`."""
    u = unit_open(words, dtype)
    two_pi = dtype(2.0 * math.pi)
    r0, r1 = np.sqrt(dtype(-2.0) * np.log(u[..., 0])), np.sqrt(dtype(-2.0) * np.log(u[..., 2]))
    a0, a1 = two_pi * u[..., 1], two_pi * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=-1).astype(dtype)


def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    with np.errstate(over="ignore"):
        return dtype(1.0) / (dtype(1.0) + np.exp(-x))


def weights(opacity_raw, min_opacity):
    """(w, safe) from the float64 sigmoid.  safe = True where that sigmoid is at least 2^-20 away from the min_opacity threshold and
    -- relative to its own size, the way a float32 evaluation errs: a few 2^-24 of the value -- at least 2^-20 away from the
    nearest step of 2^-24: there the float32 weight must be exact, elsewhere within 1.  (From sigmoid = 1/32 on no value is that
    far from a step: one float32 rounding of the sigmoid is then a step or more.)"""
    s = sigmoid(np.asarray(opacity_raw, dtype=np.float32).astype(np.float64))
    thr = np.float64(np.float32(min_opacity))
    x = s * 2.0 ** 24
    w = np.where(s <= thr, 0, np.maximum(1, np.floor(x))).astype(np.uint64)
    frac = x - np.floor(x)
    safe = (np.abs(s - thr) >= 2.0 ** -20) & (np.minimum(frac, 1.0 - frac) >= 2.0 ** -20 * x)
    return w, safe


def draw(w, seed, iteration):
    """Python integers throughout: (prefix, src, count, total) of the draw on weights w."""
    w = [int(x) for x in w]
    n = len(w)
    prefix, total = [], 0
    for x in w:
        prefix.append(total)
        total += x
    src, count = [-1] * n, [0] * n
    if total == 0:
        return prefix, src, count, 0
    dead = [i for i in range(n) if w[i] == 0]
    if dead:
        words = row_random(seed, np.array(dead, dtype=np.uint64), iteration, STREAM_RELOCATE)
        for i, x in zip(dead, words):
            r = (int(x[0]) << 32) | int(x[1])
            t = (r * total) >> 64
            s = bisect.bisect_right(prefix, t) - 1           # the last row with prefix <= t
            assert w[s] > 0 and prefix[s] <= t < prefix[s] + w[s]
            src[i] = s
            count[s] += 1
    return prefix, src, count, total


def draw_fast(w, seed, iteration):
    """The same draw vectorised (numpy uint64 prefix sums are exact below 2^64; the 128-bit product through Python integers in
    object arrays): for the large-N cases of the GPU test."""
    w = np.asarray(w, dtype=np.uint64)
    n = w.shape[0]
    inc = np.cumsum(w, dtype=np.uint64)
    prefix = inc - w
    total = int(inc[-1]) if n else 0
    src, count = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    dead = np.nonzero(w == 0)[0]
    if total == 0 or dead.size == 0:
        return prefix, src, count, total
    words = row_random(seed, dead.astype(np.uint64), iteration, STREAM_RELOCATE)
    r = (words[:, 0].astype(object) << 32) | words[:, 1].astype(object)
    t = np.array([(int(x) * total) >> 64 for x in r], dtype=np.uint64)
    s = np.searchsorted(inc, t, side="right")            # the first row whose inclusive sum exceeds t: prefix <= t < prefix + w
    assert np.all(w[s] > 0) and np.all(prefix[s] <= t) and np.all(t < inc[s])
    src[dead] = s.astype(np.int32)
    np.add.at(count, s, 1)
    return prefix, src, count, total


def relocation_exact(o, n, min_opacity, digits=60):
    """(o', o'', c, ln c) of one Gaussian of opacity o (a float, taken exactly; capped at 1 - 2^-24) split n ways, by the literal
    double sum with exact binomials in `decimal` arithmetic of `digits` digits."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        D_ = decimal.Decimal
        n = min(int(n), RELOCATE_MAX_N)
        od = D_(fractions.Fraction(float(o)).numerator) / D_(fractions.Fraction(float(o)).denominator)
        one = D_(1)
        od = min(od, one - D_(2) ** -24)
        op = od if n == 1 else one - ((one - od).ln() / D_(n)).exp()
        total = D_(0)
        for i in range(1, n + 1):
            for k in range(i):
                total += D_(math.comb(i - 1, k)) * (-1) ** k * op ** (k + 1) / D_(k + 1).sqrt()
        c = od / total
        hi = one - D_(2) ** -24
        opp = min(max(op, D_(float(min_opacity))), hi)
        return float(op), float(opp), float(c), float(c.ln())


def relocation_literal(o, n, dtype):
    """The same double sum in numpy `dtype` arithmetic (binomials rounded to dtype): (o', c).  In float32 this is the evaluation
    that must FAIL at n = 51."""
    o = dtype(o)
    n = min(int(n), RELOCATE_MAX_N)
    op = o if n == 1 else dtype(1) - np.power(dtype(1) - o, dtype(1) / dtype(n), dtype=dtype)
    total = dtype(0)
    for i in range(1, n + 1):
        for k in range(i):
            total = dtype(total + dtype(math.comb(i - 1, k)) * dtype((-1) ** k) * np.power(op, dtype(k + 1), dtype=dtype) / np.sqrt(dtype(k + 1)))
    return op, dtype(o / total)


def quat_to_rot(q, dtype):
    x, y, z, w = (q[..., k] for k in range(4))
    two, one = dtype(2), dtype(1)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                  two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w),
                  two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3)).astype(dtype)


def covariance(scale_raw, q_raw, dtype=np.float64):
    """cov_from_params of gs_math.h: scales clamped at 1e-6, q = q_raw / (|q_raw| + 1e-9), Sigma = R diag(s^2) R^T."""
    sr, q = np.asarray(scale_raw).astype(dtype), np.asarray(q_raw).astype(dtype)
    s = np.maximum(np.exp(sr), dtype(1e-6))
    qn = np.sqrt((q * q).sum(-1, dtype=dtype))
    R = quat_to_rot(q * (dtype(1) / (qn + dtype(1e-9)))[..., None], dtype)
    return np.einsum("nik,nk,njk->nij", R, s * s, R).astype(dtype)


def noise_gate(opacity_raw, dtype=np.float64):
    with np.errstate(over="ignore"):
        return dtype(1) / (dtype(1) + np.exp(dtype(100) * sigmoid(opacity_raw, dtype) - dtype(0.5)))


def noise_displacement(opacity_raw, scale_raw, q_raw, a, seed, iteration, dtype=np.float64, gate32=None):
    """[n, 3] displacement of every row.  `gate32`: the float32 gate's zero pattern may be imposed (float64 never overflows at 99.5)."""
    n = len(opacity_raw)
    z = normals3(row_random(seed, np.arange(n, dtype=np.uint64), iteration, STREAM_NOISE), dtype)
    g = noise_gate(opacity_raw, dtype)
    if gate32 is not None:
        g = np.where(gate32, g, dtype(0))
    v = z * dtype(a) * g[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.einsum("nij,nj->ni", covariance(scale_raw, q_raw, dtype), v)
    return np.where(g[:, None] > 0, d, dtype(0)).astype(dtype)


def regularisers(opacity_raw, scale_raw, lambda_o, lambda_s):
    """float64: (L_o, L_s, d L_o / d opacity_raw, d L_s / d scale_raw)."""
    o, s = np.asarray(opacity_raw, dtype=np.float64), np.asarray(scale_raw, dtype=np.float64)
    n = o.shape[0]
    sg, e = sigmoid(o), np.exp(s)
    em = np.exp(-np.abs(o))
    return lambda_o * sg.mean(), lambda_s * e.mean(), lambda_o / n * em / (1 + em) ** 2, lambda_s / (3 * n) * e
