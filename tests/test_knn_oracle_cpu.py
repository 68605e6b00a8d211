"""The host build of csrc/gs_knn.h (libgsknn_host.so: the same d2, key, box distance, insert and mean the kernels inline) without a
GPU: its brute force against the float64 oracle (tests/knn_oracle.py) on every case, the key function's edge cases, the box distance
against the point distance -- the exactness argument of DESIGN.md §28 under test --, and the three-smallest insert against a sort."""
import ctypes as C

import numpy as np
import pytest

from tests import knn_oracle as ko

F3 = C.c_float * 3


@pytest.mark.parametrize("case", ko.CASES)
def test_host_brute_force_lies_within_the_oracles_bound(case):
    """The bound, relative, per value: 1.01 * 9 u with u = 2^-24.

    d2: each of the three differences is one rounding, (a - b)(1 + e), and enters squared: 2 u.  The three squares and the two sums
    that join them are one rounding each, and every term is >= 0, so a term passes through at most its own square and both sums:
    3 u more (the product written as fmaf rounds the square and a sum together: one rounding fewer, never one more).  The three
    smallest d2 are then added in ascending order -- two sums, 2 u -- and scaled once by the constant the definition names, which the
    oracle uses as the same number: 1 u (exact for m = 1 and 2).  Together 8 u to first order for the largest path; the issue's count of
    nine roundings (three differences, three squares, two sums; two sums, one scaling -- the differences once each) is the bound kept
    here, with 1 % on top for the second-order terms.  Choosing another set of three than the oracle can only happen between values
    that are equal in float64 or closer than their own rounding, which the bound on each value covers: the k-th smallest of perturbed
    values is within the perturbation of the k-th smallest.  Where both are 0 (duplicates, non-finite rows, F <= 1) they are equal.

    `lattice`: every coordinate, difference, square and sum is a small integer, exact in float32, so the ONLY rounding left is the
    scaling s * float32(1/3); the oracle's s * float32(1/3) is exact in float64, and the host result must be its float32 rounding,
    bit for bit.  (s / 3 rounded to float32 is a different number for s = 5, 7, ...: the definition multiplies and never divides.)"""
    for n in ko.SIZES:
        p, ref, host = ko.reference(case, n)
        assert host.shape == (n,) and host.dtype == np.float32
        ko.check_against_oracle(host, ref, f"{case} {n}")
        bad = ~np.isfinite(p).all(axis=1)
        assert not host[bad].any()
        if case == "lattice":
            assert np.array_equal(host.view(np.uint32), ref.astype(np.float32).view(np.uint32)), n
        if case == "same" or n <= 1:
            assert not host.any()
        if case == "pairs" and n >= 4:
            uniq, inverse = np.unique(p, axis=0, return_inverse=True)                # the duplicate at distance 0 is a neighbour:
            assert (host < ko.mean_dist2(uniq)[np.asarray(inverse).reshape(-1)]).all()  # closer than in the cloud without duplicates
        if case == "holes":
            assert bad.sum() == min(n, 3) and (host[~bad] > 0).all() == (n - bad.sum() > 1 or n == bad.sum())


def test_oracle_against_a_plain_double_loop():
    for case in ("cube", "holes", "pairs"):
        p = ko.points(case, 40)
        want = np.zeros(40)
        ok = [i for i in range(40) if np.isfinite(p[i]).all()]
        for i in ok:
            d = sorted(float(((p[i].astype(np.float64) - p[j].astype(np.float64)) ** 2).sum()) for j in ok if j != i)[:3]
            want[i] = (d[0] + d[1] + d[2]) * float(np.float32(1.0 / 3.0))
        assert np.allclose(ko.mean_dist2(p), want, rtol=1e-15, atol=0.0)
    two = np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float32)
    assert ko.mean_dist2(two).tolist() == [25.0, 25.0] and ko.mean_dist2(two[:1]).tolist() == [0.0]
    three = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float32)
    assert ko.mean_dist2(three).tolist() == [2.5, 3.0, 4.5]


def test_key_function():
    lib = ko.host()
    top = (1 << 21) - 1
    rng = np.random.default_rng(0)
    for lo, hi in ((-3.0, 4.0), (0.0, 1e-30), (-1e30, 1e30), (-3e38, 3e38), (5.0, 5.0 + 2.0 ** -20)):
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
        xs = np.sort(np.concatenate([[lo, hi], rng.uniform(lo, hi, 2000)]).astype(np.float32).clip(lo, hi))
        q = [lib.hknn_key_axis(float(x), lo, hi) for x in xs]
        assert all(a <= b for a, b in zip(q, q[1:])), (lo, hi)                  # monotone per axis
        assert q[0] == 0 and q[-1] == top and max(q) <= top, (lo, hi)
    assert lib.hknn_key_axis(2.5, 2.5, 2.5) == 0                                # zero extent
    assert lib.hknn_key_axis(0.0, -3e38, 3e38) in (top // 2, top // 2 + 1)      # an extent that overflows: no NaN, still the middle
    # the interleave against a bit loop; the top key is reserved for the non-finite rows
    lo, hi = F3(0, 0, 0), F3(1, 1, 1)
    nonfinite = lib.hknn_key_nonfinite()
    assert nonfinite == 2 ** 64 - 1
    for p in rng.uniform(0, 1, (200, 3)).astype(np.float32).tolist() + [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]:
        axes = [lib.hknn_key_axis(p[a], 0.0, 1.0) for a in range(3)]
        want = sum(((axes[a] >> b) & 1) << (3 * b + a) for a in range(3) for b in range(21))
        got = lib.hknn_key(F3(*p), lo, hi)
        assert got == want and got < 2 ** 63
    assert lib.hknn_key(F3(1, 1, 1), lo, hi) == 2 ** 63 - 1
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        assert lib.hknn_key(F3(*bad), lo, hi) == nonfinite
    # zero extent on every axis, and an infinite extent, through the whole key
    assert lib.hknn_key(F3(2, 2, 2), F3(2, 2, 2), F3(2, 2, 2)) == 0
    assert lib.hknn_key(F3(3e38, -3e38, 0), F3(-3e38, -3e38, -3e38), F3(3e38, 3e38, 3e38)) < 2 ** 63


def test_box_distance_never_exceeds_the_distance_to_a_point_inside():
    """In fp32, on 10^4 random (box, point, query) triples: queries outside, on the faces, at the point itself and inside the box.
    A wave skips a box only when this distance is strictly greater than a lane's third-best, so this is what keeps the search exact."""
    lib = ko.host()
    rng = np.random.default_rng(1)
    worst = 0.0
    for t in range(10_000):
        scale = np.float32(10.0 ** rng.integers(-3, 4))
        a, b = (rng.uniform(-1, 1, (2, 3)) * scale).astype(np.float32)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        p = np.clip((lo + (hi - lo) * rng.uniform(0, 1, 3).astype(np.float32)).astype(np.float32), lo, hi)
        mode = t % 4
        if mode == 0:
            q = (rng.uniform(-2, 2, 3) * scale).astype(np.float32)
        elif mode == 1:
            q = np.where(rng.uniform(size=3) < 0.5, lo, hi).astype(np.float32)
            q[rng.integers(3)] = np.float32(rng.uniform(-2, 2) * scale)
        elif mode == 2:
            q = p.copy()
        else:
            q = np.clip((lo + (hi - lo) * rng.uniform(0, 1, 3).astype(np.float32)).astype(np.float32), lo, hi)
        box, pt = lib.hknn_dist2_box(F3(*q), F3(*lo), F3(*hi)), lib.hknn_dist2(F3(*q), F3(*p))
        assert box <= pt, (t, q, lo, hi, p, box, pt)
        assert pt == lib.hknn_dist2(F3(*p), F3(*q))                             # symmetric bit for bit
        if mode >= 2:
            assert box == 0.0
        worst = max(worst, box / pt if pt > 0 else 0.0)
    assert worst > 0.9                                                          # (the bound is not vacuous: some boxes are nearly as far)


def test_insert3_against_a_sort():
    lib = ko.host()
    rng = np.random.default_rng(2)
    for t in range(500):
        n = int(rng.integers(0, 12))
        d = rng.integers(0, 5, n).astype(np.float32) if t % 2 else rng.uniform(0, 1, n).astype(np.float32)
        best = (C.c_float * 3)()
        lib.hknn_insert3(n, ko.fptr(d), best)
        want = sorted(d.tolist())[:3] + [float("inf")] * (3 - min(n, 3))
        assert list(best) == want
    assert lib.hknn_mean_smallest(1.0, 2.0, 4.0, 3) == np.float32(7.0) * np.float32(1.0 / 3.0)
    assert lib.hknn_mean_smallest(1.0, 2.0, 4.0, 2) == 1.5 and lib.hknn_mean_smallest(1.0, 2.0, 4.0, 1) == 1.0
    assert lib.hknn_mean_smallest(1.0, 2.0, 4.0, 0) == 0.0 and lib.hknn_mean_smallest(1.0, 2.0, 4.0, -1) == 0.0
