"""Reference of raster_contrib_kernel alone (csrc/gs_contrib.h): per-Gaussian contribution statistics from the SAME records and lists the
kernel reads, on tests/raster_oracle.py's rule and band machinery.  Plain numpy, no torch, no GPU.

With w_i(p) = alpha_i T_i [T_i > 5e-5] (raster_oracle._columns: the same q, exp, alpha_max clamp, cutoff and alive test as the forward
kernel), over all pixels of all lists a Gaussian is binned into:
    weight_sum = sum_p w,   weight_max = max_p w,   pixels = #{p : w > 0}.

contribution()      float64; also the allowances.  For every band (pair, pixel) of raster_oracle (one of its decisions within fp32's reach
                    of its threshold) the pixel's column is recomputed with that one decision inverted, and every Gaussian of the column gets
                    |delta w| added to its sum allowance, 1 added to its pixel allowance where [w > 0] changes, and its w at that pixel
                    widened to [min, max] of the base and the flipped value (w_lo, w_hi): weight_max lies between max_p w_lo and max_p w_hi.
contribution_f32()  the same in float32 in the kernel's order: conic pre-scaled by -0.5 log2 e, exp2, T = T - alpha T; a lane adds its two
                    pixels, the 8 lanes of a sub-tile add in the tree ((0+7)+(2+5)) + ((1+6)+(3+4)), the sub-tiles of a pair add in index
                    order, and the pair adds rint(pair_sum 2^32) to the uint64 sum_q.  Returns the record [n,4] uint32 the kernel would leave.
check()             a device record [n,4] (32-bit words: sum_q lo, sum_q hi, float bits of weight_max, pixels) against contribution():
    |delta weight_sum| <= K_sum 2^-24 weight_sum + pairs 2^-33 + allowance           (2^-33: half a unit of the per-pair rounding)
    max_p w_lo (1 - K_max 2^-24 (depth index + 2)) <= weight_max <= max_p w_hi (1 + K_max 2^-24 (depth index + 2))
    |delta pixels| <= allowance (exact where it is 0);  rows of Gaussians in no list: all four words zero
    calls = c: the record after c calls on the same frame (sum_q, pairs and pixels c-fold, weight_max the same).
K_sum, K_max are 3 x ratios(contribution_f32's record): measured against the oracle's own float32 arithmetic, never against the kernel."""
import numpy as np

from tests import raster_oracle as ro

EPS = ro.EPS
Q32 = 2.0 ** 32


class ContribError(AssertionError):
    pass


def _w(o, amax):
    """The blending weights [L,P] of a raster_oracle._columns result."""
    alpha = np.where(o["pq"] & o["po"], np.where(o["pc"], o["og"], amax), 0.0)
    return np.where(o["alive"], alpha * o["T"], 0.0)


class Reference:
    """What contribution() returns: weight_sum, weight_max [n] float64, pixels, pairs [n] int64, in_list [n]; allow_sum [n], allow_pix [n];
    per pair position in sorted_ids: w_lo, w_hi [capacity,128] (the base w widened by the flips), depth_index [capacity] (position in its
    list), gauss [capacity] (-1: not in a list); max_lo, max_hi [n] (the interval of weight_max before the float32 widening); n_flips."""


def contribution(rec, ranges, sorted_ids, lists_x, H, W, chi, alpha_max, alpha_cutoff, allowances=True):
    rec = np.asarray(rec, np.float64).copy()
    rec[:, 8:12] = 0.0                       # colours and depth take no part
    n = len(rec)
    th = (float(chi), float(alpha_max), float(alpha_cutoff))
    ranges, sorted_ids = np.asarray(ranges, np.int64), np.asarray(sorted_ids, np.int64)
    cap = len(sorted_ids)
    ref = Reference()
    ref.n, ref.H, ref.W, ref.lists_x, ref.ranges, ref.sorted_ids = n, H, W, lists_x, ranges, sorted_ids
    ref.weight_sum, ref.weight_max = np.zeros(n), np.zeros(n)
    ref.pixels, ref.pairs = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ref.allow_sum, ref.allow_pix = np.zeros(n), np.zeros(n, np.int64)
    ref.in_list = np.zeros(n, bool)
    ref.w_lo, ref.w_hi = np.zeros((cap, 128)), np.zeros((cap, 128))
    ref.depth_index, ref.gauss = np.zeros(cap, np.int64), np.full(cap, -1, np.int64)
    ref.pair_list = np.full(cap, -1, np.int64)
    ref.n_flips = 0
    zero3, zero1 = np.zeros((128, 3)), np.zeros(128)
    for l_ in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        s0, s1 = ranges[l_]
        g = sorted_ids[s0:s1]
        ref.in_list[g] = True
        ref.gauss[s0:s1], ref.depth_index[s0:s1], ref.pair_list[s0:s1] = g, np.arange(len(g)), l_
        np.add.at(ref.pairs, g, 1)
        px, py = ro._list_pixels(l_, lists_x)
        valid = (px < W) & (py < H)
        vf = valid.astype(np.float64)
        r = rec[g]
        fx, fy = px.astype(np.float64), py.astype(np.float64)
        o = ro._columns(r, fx, fy, vf, th, zero3, vf, zero1, None)               # (g_depth = 1 on the image: rows[:, 9] = sum_p w)
        w = _w(o, th[1])
        np.add.at(ref.weight_sum, g, o["rows"][:, 9])
        np.maximum.at(ref.weight_max, g, w.max(1))
        np.add.at(ref.pixels, g, (w > 0).sum(1))
        lo, hi = w.copy(), w.copy()
        if allowances:
            # the band, as raster_oracle.composite forms it
            idx = np.arange(len(g))[:, None]
            b_alive = (np.abs(o["T"] - ro.T_MIN) <= ro.T_MIN * ro.K_B * EPS * (idx + 1)) & valid[None, :]
            eff = (o["alive"] | b_alive) & valid[None, :]
            b_q = (np.abs(o["q"] - th[0]) <= o["qb"]) & eff
            rel = o["og"] * (ro.K_B * EPS + 0.5 * o["qb"])
            inexact = (o["du"] != 0) | (o["dv"] != 0)
            b_cut = (np.abs(o["og"] - th[2]) <= rel) & eff & (o["pq"] | b_q) & inexact
            b_max = (np.abs(o["og"] - th[1]) <= rel) & eff & (o["pq"] | b_q) & inexact
            flips = [(k, int(i), int(p)) for k, b in (("q", b_q), ("cut", b_cut), ("max", b_max), ("alive", b_alive)) for i, p in np.argwhere(b)]
            base = {}
            for kind, i, p in flips:
                args = (r, fx[p:p + 1], fy[p:p + 1], vf[p:p + 1], th, zero3[:1], vf[p:p + 1], zero1[:1], None)
                if p not in base:
                    base[p] = ro._columns(*args)
                b0, b1 = base[p], ro._columns(*args, force=(kind, i))
                w0, w1 = _w(b0, th[1])[:, 0], _w(b1, th[1])[:, 0]
                np.add.at(ref.allow_sum, g, np.abs(b1["rows"][:, 9] - b0["rows"][:, 9]))
                np.add.at(ref.allow_pix, g, ((w1 > 0) != (w0 > 0)).astype(np.int64))
                lo[:, p], hi[:, p] = np.minimum(lo[:, p], w1), np.maximum(hi[:, p], w1)
                ref.n_flips += 1
        ref.w_lo[s0:s1], ref.w_hi[s0:s1] = lo, hi
    ref.max_lo, ref.max_hi = np.zeros(n), np.zeros(n)
    used = ref.gauss >= 0
    np.maximum.at(ref.max_lo, ref.gauss[used], ref.w_lo[used].max(1))
    np.maximum.at(ref.max_hi, ref.gauss[used], ref.w_hi[used].max(1))
    ref.any_allowance = (ref.allow_sum > 0) | (ref.allow_pix > 0) | (ref.max_hi > ref.max_lo)
    return ref


# ---- the float32 mode ---------------------------------------------------------------------------------------------------------------

def _subtile_lanes(x):
    """[m,128] per-pixel values -> [m,8,8,2]: (sub-tile 4 (y / 4) + x / 4, lane j, the lane's two pixels (j & 3, j >> 2) and (j & 3, (j >> 2) + 2))."""
    a = x.reshape(-1, 2, 4, 4, 4)                                  # (ty, yl, tx, xl)
    pair = np.stack([a[:, :, 0:2], a[:, :, 2:4]], -1)              # (ty, j >> 2, tx, j & 3, which)
    return pair.transpose(0, 1, 3, 2, 4, 5).reshape(-1, 8, 8, 2)


def contribution_f32(rec, ranges, sorted_ids, lists_x, H, W, chi, alpha_max, alpha_cutoff, ragged_bug=False, count_dead=False,
                     max_of_lane_sum=False, truncate=False):
    """The rule in float32 in the kernel's order; all lists advance together, one entry per step.  Returns a dict: record [n,4] uint32,
    and per (pair, sub-tile) sub_sum [capacity,8] float32, sub_max [capacity,8] float32, sub_cnt [capacity,8] int64 (record_from_pairs
    rebuilds the record from them).  The switches restate kernel faults for tests/test_contrib_oracle_cpu.py: the pixel column right of a
    ragged image counted, dead pixels counted in `pixels`, the maximum taken of a lane's w.x + w.y, truncation in the quantisation."""
    f = np.float32
    rec = np.asarray(rec, f)
    n = len(rec)
    ranges, sorted_ids = np.asarray(ranges, np.int64), np.asarray(sorted_ids, np.int64)
    chi, amax, cut = (f(x) for x in (chi, alpha_max, alpha_cutoff))
    chik, tmin = f(chi * ro.QK), f(ro.T_MIN)
    ln = ranges[:, 1] - ranges[:, 0]
    ls = np.argsort(-ln, kind="stable")
    ls = ls[ln[ls] > 0]
    nl, cap = len(ls), len(sorted_ids)
    px = np.stack([ro._list_pixels(l_, lists_x)[0] for l_ in ls]) if nl else np.zeros((0, 128), np.int64)
    py = np.stack([ro._list_pixels(l_, lists_x)[1] for l_ in ls]) if nl else np.zeros((0, 128), np.int64)
    valid = (px < (W + 1 if ragged_bug else W)) & (py < H)
    fpx, fpy = px.astype(f), py.astype(f)
    T = valid.astype(f)
    sub_sum, sub_max, sub_cnt = np.zeros((cap, 8), f), np.zeros((cap, 8), f), np.zeros((cap, 8), np.int64)
    for i in range(int(ln.max(initial=0))):
        m = int((ln[ls] > i).sum())
        pos = ranges[ls[:m], 0] + i
        r = rec[sorted_ids[pos]]
        k11, k12, k22 = ro.QK * r[:, 2:3], (f(2) * ro.QK) * r[:, 3:4], ro.QK * r[:, 4:5]
        du, dv = fpx[:m] - r[:, 0:1], fpy[:m] - r[:, 1:2]
        q = (k11 * du * du) + dv * ((k12 * du) + k22 * dv)
        al = np.minimum(r[:, 5:6] * np.exp2(q), amax)
        passed = (q >= chik) & (al >= cut)
        al = np.where(passed & (T[:m] > tmin), al, f(0))
        w = al * T[:m]
        T[:m] = T[:m] - al * T[:m]
        lanes = _subtile_lanes(w)                                                    # [m,8,8,2]
        h = lanes[..., 0] + lanes[..., 1]                                            # a lane's two pixels
        y = h + h[..., ::-1]                                                         # l <-> 7 - l
        z = y + y[..., [2, 3, 0, 1, 6, 7, 4, 5]]                                     # l <-> l ^ 2
        sub_sum[pos] = (z + z[..., [1, 0, 3, 2, 5, 4, 7, 6]])[..., 0]                # l <-> l ^ 1
        sub_max[pos] = (h if max_of_lane_sum else lanes.max(-1)).max(-1)
        hit = (passed & valid[:m]) if count_dead else (w > 0)
        sub_cnt[pos] = _subtile_lanes(hit.astype(np.int64)).sum((2, 3))
    return dict(record=record_from_pairs(sub_sum, sub_max, sub_cnt, ranges, sorted_ids, n, truncate=truncate), sub_sum=sub_sum,
                sub_max=sub_max, sub_cnt=sub_cnt)


def record_from_pairs(sub_sum, sub_max, sub_cnt, ranges, sorted_ids, n, truncate=False, record=None):
    """The record [n,4] uint32 from the values of every (pair, sub-tile): the sub-tiles of a pair in index order (float32), then one integer
    add / max / add per pair with a pixel.  record: add into this one (a second call)."""
    f = np.float32
    tot, mx = np.zeros(len(sub_sum), f), np.zeros(len(sub_sum), f)
    for t in range(8):
        tot = tot + sub_sum[:, t]
        mx = np.maximum(mx, sub_max[:, t])
    cnt = sub_cnt.sum(1)
    scaled = tot.astype(np.float64) * Q32                                            # (exact: a power of two)
    quant = (np.floor(scaled) if truncate else np.rint(scaled)).astype(np.uint64)
    sum_q, wmax, pix = np.zeros(n, np.uint64), np.zeros(n, f), np.zeros(n, np.uint64)
    if record is not None:
        sum_q, wmax, pix = decode(record)[0].copy(), decode(record)[1].copy(), decode(record)[2].astype(np.uint64)
    ranges = np.asarray(ranges, np.int64)
    for l_ in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        s0, s1 = ranges[l_]
        g = np.asarray(sorted_ids[s0:s1], np.int64)
        live = cnt[s0:s1] > 0
        np.add.at(sum_q, g[live], quant[s0:s1][live])
        np.maximum.at(wmax, g[live], mx[s0:s1][live])
        np.add.at(pix, g[live], cnt[s0:s1][live].astype(np.uint64))
    return encode(sum_q, wmax, pix)


def encode(sum_q, weight_max, pixels):
    out = np.zeros((len(sum_q), 4), np.uint32)
    out[:, 0], out[:, 1] = (sum_q & np.uint64(0xFFFFFFFF)).astype(np.uint32), (sum_q >> np.uint64(32)).astype(np.uint32)
    out[:, 2] = np.asarray(weight_max, np.float32).view(np.uint32)
    out[:, 3] = (np.asarray(pixels, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def decode(record):
    """(sum_q uint64, weight_max float32, pixels int64) of a record [n,4] of 32-bit words (int32 or uint32)."""
    w = np.ascontiguousarray(np.asarray(record)).view(np.uint32).reshape(-1, 4)
    sum_q = w[:, 0].astype(np.uint64) | (w[:, 1].astype(np.uint64) << np.uint64(32))
    return sum_q, w[:, 2].copy().view(np.float32), w[:, 3].astype(np.int64)


# ---- the comparison -------------------------------------------------------------------------------------------------------------------

def _max_need(ref, wmax):
    """Per Gaussian the smallest K_max that lets its device weight_max into the widened interval (inf: no K does)."""
    used = ref.gauss >= 0
    g = ref.gauss[used]
    d = EPS * (ref.depth_index[used] + 2.0)[:, None]
    m = np.asarray(wmax, np.float64)[g][:, None]
    lo, hi = ref.w_lo[used], ref.w_hi[used]
    with np.errstate(divide="ignore", invalid="ignore"):
        k_hi = np.where(hi > 0, (m / hi - 1.0) / d, np.inf).min(1)                 # m <= hi (1 + K d) for SOME pixel
        k_lo = np.where(lo > m, (1.0 - m / lo) / d, 0.0).max(1)                    # lo (1 - K d) <= m for EVERY pixel
    need_hi, need_lo = np.full(ref.n, np.inf), np.zeros(ref.n)
    np.minimum.at(need_hi, g, k_hi)
    np.maximum.at(need_lo, g, k_lo)
    need_hi = np.where(np.asarray(wmax) == 0, 0.0, need_hi)
    return np.maximum(np.maximum(need_hi, need_lo), 0.0)


def ratios(record, ref, calls=1):
    """The K_sum and K_max the record needs: largest (|delta weight_sum| - pairs 2^-33 - allowance)+ / (2^-24 weight_sum) and the
    largest widening of the weight_max interval, over the Gaussians in a list."""
    sum_q, wmax, _ = decode(record)
    d = np.abs(sum_q.astype(np.float64) / Q32 - calls * ref.weight_sum) - calls * (ref.pairs * 2.0 ** -33 + ref.allow_sum)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(d > 0, d / (EPS * calls * ref.weight_sum), 0.0)
    need = _max_need(ref, wmax)
    return dict(sum=float(x[ref.in_list].max(initial=0.0)), max=float(need[ref.in_list].max(initial=0.0)))


def _where(ref, i):
    pos = np.nonzero(ref.gauss == i)[0]
    if len(pos) == 0:
        return "in no list"
    k = pos[np.argmax(ref.w_hi[pos].sum(1))]
    return f"most of it in list {int(ref.pair_list[k])}, entry {int(ref.depth_index[k])} (position {int(ref.depth_index[k]) % ro.CHUNK} of chunk {int(ref.depth_index[k]) // ro.CHUNK})"


def check(record, ref, K, what="", calls=1):
    """record [n,4] 32-bit words against contribution()'s reference within K = dict(sum=, max=); see the module docstring.  Raises
    ContribError naming the Gaussian and the word (weight_sum, weight_max, pixels).  Returns ratios(record, ref, calls)."""
    rec = np.asarray(record)
    if rec.shape != (ref.n, 4) or rec.dtype.itemsize != 4:
        raise ContribError(f"{what}: record of shape {rec.shape}, {rec.dtype}: expected ({ref.n}, 4) 32-bit words")
    sum_q, wmax, pix = decode(rec)
    words = np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 4)
    bad = np.nonzero(words.any(1) & ~ref.in_list)[0]
    if len(bad):
        raise ContribError(f"{what}: Gaussian {bad[0]} is in no list, its row is {words[bad[0]].tolist()}")
    if not np.isfinite(wmax).all() or (wmax < 0).any():
        i = int(np.nonzero(~np.isfinite(wmax) | (wmax < 0))[0][0])
        raise ContribError(f"{what}: Gaussian {i}: weight_max {wmax[i]!r} is not a finite non-negative float")
    ws = sum_q.astype(np.float64) / Q32
    want = calls * ref.weight_sum
    bound = K["sum"] * EPS * want + calls * (ref.pairs * 2.0 ** -33 + ref.allow_sum)
    d = np.abs(ws - want)
    bad = np.nonzero(d > bound)[0]
    if len(bad):
        i = int(bad[np.argmax(d[bad] / np.maximum(bound[bad], 1e-300))])
        raise ContribError(f"{what}: Gaussian {i}, weight_sum: {ws[i]!r}, reference {want[i]!r}: |delta| {d[i]:.3e} > {bound[i]:.3e} (= {K['sum']:.1f} x 2^-24 x "
                           f"{want[i]:.3e} + {calls * ref.pairs[i]} pairs x 2^-33 + {calls * ref.allow_sum[i]:.3e}); {len(bad)} Gaussians beyond their bounds; {_where(ref, i)}")
    need = _max_need(ref, wmax)
    bad = np.nonzero(need > K["max"])[0]
    if len(bad):
        i = int(bad[np.argmax(need[bad])])
        raise ContribError(f"{what}: Gaussian {i}, weight_max: {wmax[i]!r} outside [{ref.max_lo[i]!r}, {ref.max_hi[i]!r}] widened by {K['max']:.1f} x 2^-24 x "
                           f"(depth index + 2) (it needs {need[i]:.1f}); {len(bad)} Gaussians outside their intervals; {_where(ref, i)}")
    dp = np.abs(pix - calls * ref.pixels)
    bad = np.nonzero(dp > calls * ref.allow_pix)[0]
    if len(bad):
        i = int(bad[np.argmax(dp[bad])])
        raise ContribError(f"{what}: Gaussian {i}, pixels: {int(pix[i])}, reference {int(calls * ref.pixels[i])} (allowance {int(calls * ref.allow_pix[i])}); "
                           f"{len(bad)} Gaussians with a wrong pixel count; {_where(ref, i)}")
    return ratios(rec, ref, calls)
