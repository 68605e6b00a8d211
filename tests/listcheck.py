"""Checker of what the projection, binning and sort kernels leave on the device: per-Gaussian records, (list, Gaussian) pairs, the
launch plan and the per-pair sub-tile masks.  Plain numpy, no GPU: tests/test_listcheck_cpu.py feeds it arrays built on the CPU (and
broken on purpose), tests/test_gpu_lists.py what the device wrote.  Every failure names the list and the Gaussian.

A "list" is one 16 x 8-pixel region (list L = ly * lists_x + lx); pairs of list L are sorted_ids[ranges[L, 0] : ranges[L, 1]].
"""
import numpy as np

LIST_W, LIST_H = 16, 8
# sort size classes of the launch plan (csrc/gs_sort.h, K5: SORT_CLASSES / class_first_bucket): class c holds the lists of
# CLASS_MIN_LEN[c] <= length < CLASS_MIN_LEN[c - 1]; class_bounds[c] = lists in classes 0 .. c, so class_bounds[3] = the non-empty
# lists, and the empty ones fill the rest of `order`.  (Whether the 4096+ class gets a launch of its own is gsplat_bin's business:
# without one the launch of the next class takes its lists too; the bounds are the same either way.)
CLASS_MIN_LEN = (4096, 1024, 256, 1)
# Check 9 (a set sub-tile bit implies min q <= chi_pad): the largest relative excess of the float64 minimum over chi_pad where the
# ORACLE'S OWN float32 evaluation of the same minimum says "touched", measured over every (Gaussian, sub-tile) candidate of the
# scenes of tests/test_gpu_lists.py with 2-D condition number <= 1e4 (tests/test_listcheck_cpu.py measures and prints it):
#   3.05e-5 (the hot spot in the 512 x 640 image; 1.2e-6 .. 8.5e-6 on the other scenes); the device may exceed chi_pad by K_CAL
#   (tests/util.py) times that.  "Excess" of a candidate = q64 / q32 - 1, the amount by which the float64 minimum lies above chi_pad
#   when the float32 one sits exactly on it, over the candidates within a factor two of chi_pad.
PAIR_MASK_EXCESS_F32 = 3.05e-5
COND_CAP = 1e4


class ListError(AssertionError):
    pass


def _fail(msg):
    raise ListError(msg)


def work_bucket(w):
    """The plan's bucket of a list length (K4 work_bucket): exact below 8, then 8 steps per power of two."""
    w = np.asarray(w, np.int64)
    e = np.floor(np.log2(np.maximum(w, 1))).astype(np.int64)
    return np.where(w < 8, w, (e - 2) * 8 + ((w >> np.maximum(e - 3, 0)) & 7))


def unpack_rect(rect):
    rect = np.asarray(rect, np.uint32)
    return ((rect[:, 0] & 0xFFFF).astype(np.int64), (rect[:, 0] >> 16).astype(np.int64),
            (rect[:, 1] & 0xFFFF).astype(np.int64), (rect[:, 1] >> 16).astype(np.int64))


class Pairs:
    """The pairs of every list, flattened in list order: list, position in sorted_ids, Gaussian."""

    def __init__(self, ranges, sorted_ids, n_lists):
        start, end = ranges[:, 0].astype(np.int64), ranges[:, 1].astype(np.int64)
        ln = end - start
        self.len = ln
        self.list = np.repeat(np.arange(n_lists, dtype=np.int64), ln)
        first = np.cumsum(ln) - ln
        self.pos = start[self.list] + (np.arange(len(self.list), dtype=np.int64) - first[self.list])
        self.id = sorted_ids[self.pos].astype(np.int64)
        self.rank = self.pos - start[self.list]           # position inside the list


def check_ranges(ranges, n_binned, tiles, capacity=None):
    """Check 1.  n_binned: the counter.  Returns nothing; raises ListError naming the list."""
    nl = len(ranges)
    start, end = ranges[:, 0].astype(np.int64), ranges[:, 1].astype(np.int64)
    bad = np.nonzero(end < start)[0]
    if len(bad):
        _fail(f"list {bad[0]}: range [{start[bad[0]]}, {end[bad[0]]}) ends before it starts")
    lim = n_binned if capacity is None else min(n_binned, capacity)
    bad = np.nonzero((end > lim) | (start > lim))[0]
    if len(bad):
        _fail(f"list {bad[0]}: range [{start[bad[0]]}, {end[bad[0]]}) leaves [0, {lim}]")
    full = np.nonzero(end > start)[0]
    o = full[np.argsort(start[full], kind="stable")]
    over = np.nonzero(end[o][:-1] > start[o][1:])[0]
    if len(over):
        a, b = o[over[0]], o[over[0] + 1]
        _fail(f"list {b}: range [{start[b]}, {end[b]}) overlaps list {a}: [{start[a]}, {end[a]})")
    total = int((end - start).sum())
    if total != n_binned:                 # name the first list that does not start where its predecessor ended
        expect = 0
        for l_ in o:
            if start[l_] != expect:
                _fail(f"list {l_}: range starts at {start[l_]}, the lists before it end at {expect} (lengths add up to {total}, the counter says {n_binned})")
            expect = end[l_]
        _fail(f"list {o[-1] if len(o) else 0}: the ranges end at {expect}, the counter says {n_binned}")
    if total != int(np.asarray(tiles, np.int64).sum()):
        _fail(f"list 0: the ranges hold {total} pairs, tiles[] adds up to {int(np.asarray(tiles, np.int64).sum())}")
    assert nl == len(ranges)


def check_pairs(p, n, rect, tiles, mask, depth, lists_x):
    """Checks 2 - 5 on the flattened pairs `p`."""
    tiles = np.asarray(tiles, np.int64)
    bad = np.nonzero(p.id >= n)[0]
    if len(bad):
        _fail(f"list {p.list[bad[0]]}: entry {p.rank[bad[0]]} is Gaussian {p.id[bad[0]]} >= N = {n}")
    bad = np.nonzero(tiles[p.id] == 0)[0]
    if len(bad):
        _fail(f"list {p.list[bad[0]]}: holds Gaussian {p.id[bad[0]]}, which is binned nowhere (tiles = 0)")
    key = p.list * n + p.id
    ks = np.sort(key, kind="stable")
    dup = np.nonzero(ks[1:] == ks[:-1])[0]
    if len(dup):
        _fail(f"list {ks[dup[0]] // n}: holds Gaussian {ks[dup[0]] % n} twice")
    x0, y0, x1, y1 = unpack_rect(rect)
    lx, ly = p.list % lists_x, p.list // lists_x
    out = np.nonzero((lx < x0[p.id]) | (lx > x1[p.id]) | (ly < y0[p.id]) | (ly > y1[p.id]))[0]
    if len(out):
        k = out[0]
        _fail(f"list {p.list[k]} = ({lx[k]}, {ly[k]}): holds Gaussian {p.id[k]}, whose rectangle is x {x0[p.id[k]]}..{x1[p.id[k]]}, y {y0[p.id[k]]}..{y1[p.id[k]]}")
    # 3: small rectangles -- exactly the lists of the mask bits (set equality, sorted keys)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    area = w * h
    small = (tiles > 0) & (area <= 32)
    si = np.nonzero(small)[0]
    bits = (np.asarray(mask, np.uint32)[si][:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
    stray = np.nonzero((bits * (np.arange(32)[None, :] >= area[si][:, None])).any(1))[0]
    if len(stray):
        _fail(f"list 0: Gaussian {si[stray[0]]} has mask bits beyond its rectangle of {area[si[stray[0]]]} lists")
    gi, kk = np.nonzero(bits)
    g = si[gi]
    want = np.sort(((y0[g] + kk // w[g]) * lists_x + x0[g] + kk % w[g]) * n + g)
    have = ks[small[ks % n]]
    if len(want) != len(have) or np.any(want != have):
        miss = np.setdiff1d(want, have)
        if len(miss):
            _fail(f"list {miss[0] // n} lacks Gaussian {miss[0] % n} (its mask bit is set)")
        extra = np.setdiff1d(have, want)
        _fail(f"list {extra[0] // n}: holds Gaussian {extra[0] % n}, whose mask bit for it is clear")
    # the number of pairs of every Gaussian (small ones are settled by the set equality above; this names a large one's list)
    cnt = np.bincount(p.id, minlength=n)
    bad = np.nonzero(cnt != tiles)[0]
    if len(bad):
        i = bad[0]
        where = p.list[p.id == i]
        _fail(f"list {where[0] if len(where) else y0[i] * lists_x + x0[i]}: Gaussian {i} is in {cnt[i]} lists, tiles[] says {tiles[i]}")
    # 4: large rectangles -- one contiguous interval of lists per row
    big = ~small[p.id]
    if big.any():
        bk = np.sort((p.id[big] * 65536 + ly[big]) * 65536 + lx[big])
        same_row = (bk[1:] >> 16) == (bk[:-1] >> 16)
        gap = np.nonzero(same_row & (bk[1:] - bk[:-1] != 1))[0]
        if len(gap):
            k = bk[gap[0]]
            i, yy, xx = k >> 32, (k >> 16) & 0xFFFF, k & 0xFFFF
            _fail(f"list {yy * lists_x + xx + 1} lacks Gaussian {i}: its lists in row {yy} are not one interval (gap behind x = {xx})")
    check_pairs_order(p, depth)


def check_pairs_order(p, depth):
    """Check 5: inside a list (float bits of depth, id) is strictly increasing."""
    dk = (np.asarray(depth, np.float32).view(np.uint32)[p.id].astype(np.uint64) << np.uint64(32)) | p.id.astype(np.uint64)
    inside = p.list[1:] == p.list[:-1]
    bad = np.nonzero(inside & (dk[1:] <= dk[:-1]))[0]
    if len(bad):
        k = bad[0]
        _fail(f"list {p.list[k]}: entries {p.rank[k]} and {p.rank[k] + 1} (Gaussians {p.id[k]}, {p.id[k + 1]}; depths "
              f"{np.asarray(depth)[p.id[k]]!r}, {np.asarray(depth)[p.id[k + 1]]!r}) are not in (depth, index) order")


def check_plan(ranges, order, class_bounds):
    """Check 6."""
    nl = len(ranges)
    ln = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    order = np.asarray(order, np.int64)
    if len(order) != nl or np.any(np.sort(order) != np.arange(nl)):
        cnt = np.bincount(order[order < nl], minlength=nl)
        twice, never = np.nonzero(cnt > 1)[0], np.nonzero(cnt == 0)[0]
        _fail(f"list {twice[0] if len(twice) else never[0]}: launched {'twice' if len(twice) else 'never'} by `order`"
              + (f" (list {never[0]} never)" if len(twice) and len(never) else ""))
    cb = np.asarray(class_bounds, np.int64)[:4]
    if np.any(np.diff(cb) < 0) or cb[0] < 0 or cb[3] > nl:
        _fail(f"list 0: class_bounds {cb.tolist()} are not monotone inside [0, {nl}]")
    if cb[3] != int((ln > 0).sum()):
        _fail(f"list {order[min(cb[3], nl - 1)]}: class_bounds end at {cb[3]}, {int((ln > 0).sum())} lists are non-empty")
    lo = 0
    for c in range(4):
        ls = order[lo:cb[c]]
        hi_len = CLASS_MIN_LEN[c - 1] if c else None
        bad = np.nonzero((ln[ls] < CLASS_MIN_LEN[c]) | ((ln[ls] >= hi_len) if hi_len else False))[0]
        if len(bad):
            _fail(f"list {ls[bad[0]]}: length {ln[ls[bad[0]]]} in sort class {c} (lengths >= {CLASS_MIN_LEN[c]}" + (f", < {hi_len})" if hi_len else ")"))
        lo = cb[c]
    bad = np.nonzero(ln[order[cb[3]:]] != 0)[0]
    if len(bad):
        _fail(f"list {order[cb[3] + bad[0]]}: length {ln[order[cb[3] + bad[0]]]} behind the last sort class")
    b = work_bucket(ln[order])
    up = np.nonzero(b[1:] > b[:-1])[0]
    if len(up):
        _fail(f"list {order[up[0] + 1]}: length {ln[order[up[0] + 1]]} is launched behind list {order[up[0]]} of length {ln[order[up[0]]]}")


def check_lists(n, rect, depth, tiles, mask, ranges, sorted_ids, order, class_bounds, n_binned, lists_x, lists_y):
    """Checks 1 - 6; returns the flattened pairs for the coverage checks."""
    assert len(ranges) == lists_x * lists_y
    check_ranges(ranges, n_binned, tiles)
    p = Pairs(ranges, sorted_ids, len(ranges))
    check_pairs(p, n, rect, tiles, mask, depth, lists_x)
    check_plan(ranges, order, class_bounds)
    return p


# ---- coverage against float64 ------------------------------------------------------------------------------------------
def check_coverage(p, n, ids, u, v, conic, tile_rect, chi, T, H, W, lists_x, sample=None):
    """Check 7.  ids / u / v / conic[:, 3] / tile_rect: the oracle's float64 stages.  Every image pixel with q <= chi (1 - 1e-6) inside
    the reference's tile rectangle lies in a list that holds the Gaussian.  sample: indices into `ids` (default: all)."""
    have = np.sort(p.list * n + p.id)
    det = conic[:, 0] * conic[:, 2] - conic[:, 1] ** 2
    n_px = 0
    for k in (range(len(ids)) if sample is None else sample):
        a, b, c = conic[k]
        x0, x1 = max(int(tile_rect[k, 0]) * T, 0), min(int(tile_rect[k, 2]) * T + T, W)
        y0, y1 = max(int(tile_rect[k, 1]) * T, 0), min(int(tile_rect[k, 3]) * T + T, H)
        if det[k] > 0:                                   # the ellipse's own box, one pixel wider
            ex, ey = np.sqrt(chi * c / det[k]) + 1, np.sqrt(chi * a / det[k]) + 1
            x0, x1 = max(x0, int(np.floor(u[k] - ex))), min(x1, int(np.ceil(u[k] + ex)) + 1)
            y0, y1 = max(y0, int(np.floor(v[k] - ey))), min(y1, int(np.ceil(v[k] + ey)) + 1)
        if x1 <= x0 or y1 <= y0:
            continue
        ys, xs = np.mgrid[y0:y1, x0:x1]
        du, dv = xs - u[k], ys - v[k]
        inside = a * du * du + 2 * b * du * dv + c * dv * dv <= chi * (1 - 1e-6)
        if not inside.any():
            continue
        n_px += int(inside.sum())
        need = np.unique((ys[inside] // LIST_H) * lists_x + xs[inside] // LIST_W) * n + int(ids[k])
        got = have[np.minimum(np.searchsorted(have, need), len(have) - 1)] == need if len(have) else np.zeros(len(need), bool)
        if not got.all():
            l_ = int(need[~got][0] // n)
            _fail(f"list {l_} lacks Gaussian {int(ids[k])}: it holds pixels with q <= chi (centre {u[k]:.3f}, {v[k]:.3f})")
    return n_px


def min_q_subtiles(u, v, a, b, c, ox, oy, dtype=np.float64):
    """Minimum of q = a du^2 + 2 b du dv + c dv^2 over the pixel centres' rectangle of each of the 8 sub-tiles (bit 4 r + k: x in
    [4 k, 4 k + 3], y in [4 r, 4 r + 3] from the list origin), per pair: [P, 8].  q is convex: the minimum is at the centre if it
    lies inside, else on the edge facing it -- the smaller of the two clamped 1-D minima along x = X and y = Y (X, Y: the centre
    clamped to the rectangle).  Evaluated in `dtype` throughout (float32: what the reference's own precision gives)."""
    f = dtype
    u, v, a, b, c = (np.asarray(t, f)[:, None] for t in (u, v, a, b, c))
    k = np.arange(8)
    x0 = (np.asarray(ox, f)[:, None] + (4 * (k % 4)).astype(f)[None, :]) - u
    y0 = (np.asarray(oy, f)[:, None] + (4 * (k // 4)).astype(f)[None, :]) - v
    x1, y1 = x0 + f(3), y0 + f(3)
    X = np.clip(f(0), x0, x1)
    t = np.clip(-b / c * X, y0, y1)
    qx = a * X * X + (f(2) * b * X + c * t) * t
    Y = np.clip(f(0), y0, y1)
    s = np.clip(-b / a * Y, x0, x1)
    qy = c * Y * Y + (f(2) * b * Y + a * s) * s
    return np.minimum(qx, qy)


def needed_bits(u, v, a, b, c, ox, oy, chi, H, W):
    """Check 8's lower bound per pair: bit 4 r + k is needed when a pixel (inside the image) of that sub-tile has q64 <= chi (1 - 1e-6)."""
    need = np.zeros(len(u), np.uint8)
    xs, ys = np.arange(LIST_W), np.arange(LIST_H)
    for s_ in range(8):
        px = ox[:, None, None] + (4 * (s_ % 4) + np.arange(4))[None, None, :]
        py = oy[:, None, None] + (4 * (s_ // 4) + np.arange(4))[None, :, None]
        du, dv = px - u[:, None, None], py - v[:, None, None]
        q = a[:, None, None] * du * du + 2 * b[:, None, None] * du * dv + c[:, None, None] * dv * dv
        hit = ((q <= chi * (1 - 1e-6)) & (px < W) & (py < H)).any((1, 2))
        need |= (hit.astype(np.uint8) << s_).astype(np.uint8)
    del xs, ys
    return need


def check_pair_masks(p, pair_mask, written, n, ids, u, v, conic, cond, chi, H, W, lists_x, k_cal, only_lists=None, block=200_000):
    """Checks 8 and 9.  pair_mask: one byte per pair (indexed like sorted_ids); written[pair position]: did the forward pass reach
    the pair (it stops staging a list once every pixel of it is saturated; see written_pairs).  ids / u / v / conic / cond: the
    oracle's float64 stages.  only_lists: check the pairs of these lists only (a seeded sample of a scene with millions of pairs).
    Returns (pairs checked, set bits checked against the upper bound)."""
    if only_lists is not None:
        take = np.zeros(int(p.list.max(initial=0)) + 1, bool)
        take[only_lists] = True
        keep = take[p.list]
        q = object.__new__(Pairs)
        q.list, q.pos, q.id, q.rank = p.list[keep], p.pos[keep], p.id[keep], p.rank[keep]
        p = q
    where = np.full(n, -1, np.int64)
    where[np.asarray(ids, np.int64)] = np.arange(len(ids))
    chi_pad = chi * 1.001 + 1e-4
    n_low = n_up = 0
    worst = 0.0
    for s0 in range(0, len(p.id), block):
        sl = slice(s0, min(s0 + block, len(p.id)))
        k = where[p.id[sl]]
        ok = (k >= 0) & written[p.pos[sl]]
        k, lst, gid, m = k[ok], p.list[sl][ok], p.id[sl][ok], pair_mask[p.pos[sl][ok]]
        ox, oy = (lst % lists_x) * LIST_W, (lst // lists_x) * LIST_H
        a, b, c = conic[k, 0], conic[k, 1], conic[k, 2]
        need = needed_bits(u[k], v[k], a, b, c, ox, oy, chi, H, W)
        lack = np.nonzero(need & ~m)[0]
        if len(lack):
            j = lack[0]
            bit = int(np.nonzero([(need[j] & ~m[j]) >> t & 1 for t in range(8)])[0][0])
            _fail(f"list {lst[j]}: the sub-tile mask {m[j]:#04x} of Gaussian {gid[j]} lacks bit {bit}: a pixel of that sub-tile has q <= chi (needed {need[j]:#04x})")
        n_low += len(k)
        pd = (a > 0) & (c > 0) & (a * c - b * b > 0) & (cond[k] <= COND_CAP)          # (non-PD: the kernel sets all eight bits)
        qmin = min_q_subtiles(u[k], v[k], a, b, c, ox, oy)
        setb = ((m[:, None] >> np.arange(8)[None, :]) & 1).astype(bool) & pd[:, None]
        ex = np.where(setb, qmin / chi_pad - 1.0, -1.0)
        n_up += int(setb.sum())
        if ex.size and ex.max() > worst:
            worst = float(ex.max())
        over = np.argwhere(ex > k_cal * PAIR_MASK_EXCESS_F32)
        if len(over):
            j, t = over[0]
            _fail(f"list {lst[j]}: bit {t} of the sub-tile mask {m[j]:#04x} of Gaussian {gid[j]} is set, but the smallest q over that sub-tile is "
                  f"{qmin[j, t]:.6g} > chi_pad {chi_pad:.6g} (1 + {k_cal} x {PAIR_MASK_EXCESS_F32})")
    print(f"pair masks: {n_low} pairs against the lower bound, {n_up} set bits against the upper bound; largest excess over chi_pad "
          f"{worst:.2e} (allowed {k_cal * PAIR_MASK_EXCESS_F32:.2e})")
    return n_low, n_up


def written_pairs(p, rec, ranges, H, W, lists_x, chi, alpha_max, alpha_cutoff, capacity, only_lists=None, chunk=64):
    """Which pair-mask bytes gsplat_rasterize_forward writes.  It stages a list in chunks of 64 entries and stops once no pixel of
    the list is alive (T <= 5e-5 everywhere): the bytes of the chunks behind that stay as they were.  From the device's own records,
    composited in float64: chunk j of a list counts as written when, before it, some pixel of the list inside the image has
    T > 5e-5 (1 + 1e-3) -- a pixel nearer the threshold than fp32's reach decides nothing, its chunk is left out of the check."""
    written = np.zeros(capacity, bool)
    ln = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    first = np.cumsum(ln) - ln
    written[p.pos[p.rank < chunk]] = True                      # the first chunk is always staged
    rec = np.asarray(rec, np.float64)
    for l_ in (np.nonzero(ln > chunk)[0] if only_lists is None else [x for x in only_lists if ln[x] > chunk]):
        sl = slice(first[l_], first[l_] + ln[l_])
        g = p.id[sl]
        px = (l_ % lists_x) * LIST_W + np.arange(LIST_W)
        py = (l_ // lists_x) * LIST_H + np.arange(LIST_H)
        px, py = px[px < W], py[py < H]
        du = px[None, None, :] - rec[g, 0][:, None, None]
        dv = py[None, :, None] - rec[g, 1][:, None, None]
        q = rec[g, 2][:, None, None] * du * du + 2 * rec[g, 3][:, None, None] * du * dv + rec[g, 4][:, None, None] * dv * dv
        al = np.minimum(rec[g, 5][:, None, None] * np.exp(-0.5 * np.minimum(q, chi)), alpha_max)
        al = np.where((q <= chi) & (al >= alpha_cutoff), al, 0.0)
        t_after = np.cumprod(1.0 - al, 0).reshape(len(g), -1).max(1)        # the most alive pixel after each entry
        for j in range(1, (ln[l_] + chunk - 1) // chunk):
            if t_after[j * chunk - 1] > 5e-5 * (1 + 1e-3):
                written[p.pos[sl][j * chunk:(j + 1) * chunk]] = True
            else:
                break
    return written


# ---- the float assertions on the per-Gaussian records ---------------------------------------------------------------------
def check_records(d, r0, r1, r2, tiles, visible, brect, btiles, bmask, ref_rect=None, row_spans=None):
    """The assertions of test_forward_records_vs_reference_intermediates, shared by the host build (hm_project) and the device records:
    r0 / r1 / r2 = the three 16-byte rows of the record, visible = indices of the Gaussians the projection kept, brect / btiles /
    bmask = what is binned.  ref_rect [N, 2] (packed like brect): the reference's tile rectangle as the build under test computed
    it -- the host build returns it, the device build does not keep it: then the goldens' own rectangle stands in, and at most 1 %
    of the binned rectangles may leave it (the ceil() discontinuity below).  row_spans(k) -> (xa, xb) of a large Gaussian (index into
    im_ids), or None when the caller checks the lists themselves (listcheck.check_coverage)."""
    ids = d["im_ids"]
    # same visible set as the reference (fp32 vs fp64 may flip a knife-edge cull; none in these fixtures)
    assert set(np.asarray(visible).tolist()) == set(ids.tolist())
    not_vis = np.ones(len(tiles), bool)
    not_vis[ids] = False
    assert np.all(tiles[not_vis] == 0)
    u, v = r0[ids, 0], r0[ids, 1]
    assert np.abs(u - d["im_u"]).max() < 2e-4 and np.abs(v - d["im_v"]).max() < 2e-4
    con = d["im_conic"]
    ref = np.stack([con[:, 0, 0], con[:, 0, 1], con[:, 1, 1]], 1)
    mine = np.stack([r0[ids, 2], r0[ids, 3], r1[ids, 0]], 1)
    scale = np.abs(ref).max(1, keepdims=True)
    # conic = inverse of a possibly ill-conditioned 2x2: fp32 error grows with the condition number
    ev = d["im_evals"]
    cond = (ev[:, 1] / ev[:, 0])[:, None]
    assert (np.abs(mine - ref) <= (2e-6 * cond + 1e-5) * scale).all()
    assert np.abs(r1[ids, 1] - d["im_opacity"]).max() < 1e-6
    rgb = r2[ids, :3]
    assert np.abs(rgb - d["im_color"]).max() < 2e-6
    # tight extents of {q <= chi}: must contain every pixel offset with q <= chi (checked on the reference conic)
    chi = d["kwargs"].get("chi_square_clip", 6.25)
    ex, ey = r1[ids, 2].astype(np.float64), r1[ids, 3].astype(np.float64)
    det = ref[:, 0] * ref[:, 2] - ref[:, 1] ** 2
    ok = det > 0
    assert (ex[ok] >= np.sqrt(chi * ref[ok, 2] / det[ok]) * (1 - 1e-3 * np.minimum(cond[ok, 0], 50))).all()
    assert (ey[ok] >= np.sqrt(chi * ref[ok, 0] / det[ok]) * (1 - 1e-3 * np.minimum(cond[ok, 0], 50))).all()
    T = int(d["kwargs"].get("T", 16))           # the reference's tile size: its rectangle is in T x T tiles, the lists stay 16 x 8 pixels
    bl, bh, bt = brect[ids, 0], brect[ids, 1], btiles[ids]
    br = np.stack([bl & 0xFFFF, bl >> 16, bh & 0xFFFF, bh >> 16], 1).astype(np.int32)
    has = bt > 0
    if ref_rect is not None:
        rl, rh = ref_rect[ids, 0], ref_rect[ids, 1]
        rect = np.stack([rl & 0xFFFF, rl >> 16, rh & 0xFFFF, rh >> 16], 1).astype(np.int32)
        # ceil() in the radius is a discontinuity: a 1-ulp eigenvalue difference can move an AABB edge by one pixel
        # (harmless: pixels with q <= chi_square_clip always lie inside the smaller box), so allow a few mismatches
        bad = (rect != d["im_tile_rect"]).any(1)
        assert bad.mean() <= 0.01, f"{bad.sum()} tile rectangles differ"
        assert np.all(tiles[ids] == (rect[:, 2] - rect[:, 0] + 1) * (rect[:, 3] - rect[:, 1] + 1))
    else:
        rect = np.asarray(d["im_tile_rect"], np.int32)
    # what the kernels bin: 16 x 8 half-tile lists of the tight box, inside the reference rectangle, and containing every
    # pixel of the image with q <= chi (checked by brute force with the reference conic on the integer pixel grid)
    bm = bmask[ids]
    area = (br[:, 2] - br[:, 0] + 1) * (br[:, 3] - br[:, 1] + 1)
    small = has & (area <= 32)
    # large rectangles: no mask; their lists are the row spans of big_row_span, and tiles[] counts exactly those
    assert np.all(bm[has & ~small] == 0xFFFFFFFF) and np.all(bt[has & ~small] <= area[has & ~small])
    spans = {}
    if row_spans is not None:
        for k in np.nonzero(has & ~small)[0]:
            xa, xb = row_spans(k)
            assert int(np.maximum(xb - xa + 1, 0).sum()) == int(bt[k]), k
            assert np.all((xa >= br[k, 0]) | (xa > xb)) and np.all(xb <= br[k, 2])
            spans[int(k)] = (xa, xb)
    assert np.all(bt[small] == [bin(int(x)).count("1") for x in bm[small]])
    assert np.all(bm[small] >> area[small].astype(np.uint32) == 0)
    within = ((br[:, 0] >= rect[:, 0] * T // 16) & (br[:, 2] <= (rect[:, 2] * T + T - 1) // 16) &
              (br[:, 1] >= rect[:, 1] * T // 8) & (br[:, 3] <= (rect[:, 3] * T + T - 1) // 8))
    if ref_rect is not None:
        assert np.all(within[has])
    else:
        assert (~within[has]).mean() <= 0.01, f"{(~within[has]).sum()} binned rectangles leave the reference's tile rectangle"
    H, W = d["H"], d["W"]
    ys, xs = np.mgrid[0:H, 0:W]
    for k in sorted(set(range(0, len(ids), max(1, len(ids) // 200))) | set(np.nonzero(has & ~small)[0][:300].tolist())):
        du, dv = xs - float(d["im_u"][k]), ys - float(d["im_v"][k])
        q = con[k, 0, 0] * du * du + 2 * con[k, 0, 1] * du * dv + con[k, 1, 1] * dv * dv
        inside = q <= chi * (1 - 1e-6)
        # the reference only renders the tiles of its own rectangle
        inside &= (xs // T >= rect[k, 0]) & (xs // T <= rect[k, 2]) & (ys // T >= rect[k, 1]) & (ys // T <= rect[k, 3])
        if not inside.any():
            continue
        assert bt[k] > 0, k
        lx, ly = xs[inside] // 16, ys[inside] // 8
        assert lx.min() >= br[k, 0] and lx.max() <= br[k, 2] and ly.min() >= br[k, 1] and ly.max() <= br[k, 3], k
        if area[k] <= 32:              # every list that holds such a pixel has its mask bit set
            bit = (ly - br[k, 1]) * (br[k, 2] - br[k, 0] + 1) + (lx - br[k, 0])
            assert np.all((int(bm[k]) >> bit) & 1), k
        elif row_spans is not None:    # ... or lies inside its row's span
            xa, xb = spans[int(k)]
            row = ly - br[k, 1]
            assert np.all((lx >= xa[row]) & (lx <= xb[row])), k
