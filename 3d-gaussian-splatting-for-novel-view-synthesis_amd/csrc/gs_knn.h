// gs_knn.h -- the arithmetic of the exact 3-nearest-neighbour search that initialises the scales of a point cloud:
// the squared distance, the Morton key, the distance to a box, the three-smallest insert and the mean.
//
// Product code in the style of gs_filter3d.h: `GS_HD` bodies that the kernels of gsplat_knn.hip inline and that g++ compiles into a
// host test library (csrc/host_knn_check.cpp).  The host build is a TEST of this file, never a fallback.
//
// The definition.  For N points p_i (fp32, [N, 3]), dist2[i] is the mean of the m = min(3, F - 1) smallest values of d2(i, j), where
//   * j ranges over the FINITE rows j != i, and F is the number of finite rows;
//   * d2 is dist2_points() below, in fp32, one fixed order of operations with the multiply-adds written out as fmaf (nothing is left
//     to the compiler's contraction; the host build gets -ffp-contract=off as well);
//   * the m values are summed in ascending order and scaled by a float constant per m (1, 1/2, 1/3 rounded once): no division;
//   * j != i is by INDEX, not by distance: a duplicate of a point is its neighbour at distance 0 (as in simple_knn and sklearn);
//   * a row with a NaN or an infinity is nobody's neighbour and gets 0;  F <= 1 gives 0 everywhere.
// The search is exact, so the result is a function of the multiset of the other points only: the same bits on every call, stream and
// rank, and under any permutation of the rows (the output permutes with them).
//
// Not in the reference.  Kerbl et al. 2023 §5.1 / simple_knn's distCUDA2; gsplat's knn(points, 4).
#pragma once
#include "gs_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace gsknn {

constexpr int KEY_BITS = 21;                              // per axis: a 63-bit Morton key
constexpr uint32_t KEY_MAX_AXIS = (1u << KEY_BITS) - 1u;
constexpr uint64_t KEY_NONFINITE = ~0ull;                 // above every key of a finite row (those are < 2^63)

GS_HD uint32_t float_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
GS_HD float bits_float(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
GS_HD bool finite_bits(float x) { return (float_bits(x) & 0x7f800000u) != 0x7f800000u; }
GS_HD bool finite_row(float x, float y, float z) { return finite_bits(x) && finite_bits(y) && finite_bits(z); }

// Floats as unsigned integers that order the same way (-inf < ... < -0 < +0 < ... < +inf): the bounding box is an integer atomic
// min / max of these, so it is the same bits whatever order the workgroups arrive in.
GS_HD uint32_t ordered_bits(float x) { const uint32_t u = float_bits(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
GS_HD float ordered_float(uint32_t o) { return bits_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// d2: three differences, one product, two multiply-adds, each rounded once.  Symmetric bit for bit (fl(a - b) = -fl(b - a)), and
// non-decreasing in each |difference| (rounding is monotone): what the pruning rule rests on.
GS_HD float dist2_diffs(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }
GS_HD float dist2_points(float ax, float ay, float az, float bx, float by, float bz) { return dist2_diffs(ax - bx, ay - by, az - bz); }

// The squared distance from q to the box [lo, hi], never above d2(q, p) of ANY point p inside the box IN THIS ARITHMETIC: per axis
// lo <= p <= hi gives lo - q <= p - q and q - hi <= q - p in the reals, rounding is monotone, so the rounded axis distance is at most
// |fl(q - p)|; then dist2_diffs is non-decreasing in each of them.
GS_HD float axis_gap(float q, float lo, float hi) {
    const float a = lo - q, b = q - hi;
    const float m = a > b ? a : b;
    return m > 0.f ? m : 0.f;
}
GS_HD float dist2_box(float qx, float qy, float qz, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    return dist2_diffs(axis_gap(qx, lox, hix), axis_gap(qy, loy, hiy), axis_gap(qz, loz, hiz));
}

// The three smallest of a stream, ascending in b0 <= b1 <= b2 (start: +inf).  d is never a NaN (finite rows only); d = +inf changes
// nothing.
GS_HD void insert3(float& b0, float& b1, float& b2, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    b2 = __builtin_amdgcn_fmed3f(b1, b2, d);              // the median of (b1, b2, d) = min(b2, max(b1, d)) for b1 <= b2
    b1 = __builtin_amdgcn_fmed3f(b0, b1, d);
    b0 = __builtin_fminf(b0, d);
#else
    const float hi1 = b1 > d ? b1 : d, hi0 = b0 > d ? b0 : d;
    b2 = b2 < hi1 ? b2 : hi1;
    b1 = b1 < hi0 ? b1 : hi0;
    b0 = b0 < d ? b0 : d;
#endif
}

// The mean of the m smallest, m = min(3, others): ascending sum, one scaling by a constant.
GS_HD float mean_smallest(float b0, float b1, float b2, int64_t others) {
    if (others >= 3) return ((b0 + b1) + b2) * 0.333333343f;
    if (others == 2) return (b0 + b1) * 0.5f;
    if (others == 1) return b0;
    return 0.f;
}

// ---- Morton keys (pruning quality only: no result depends on them) ---------------------------------------------------------
// One axis to KEY_BITS bits over [lo, hi] of the finite rows: non-decreasing in x, 0 for an axis of zero extent, and no NaN when
// hi - lo overflows (both halves are taken first).  lo <= x <= hi, all finite.
GS_HD uint32_t key_axis(float x, float lo, float hi) {
    float num = x - lo, ext = hi - lo;
    if (!finite_bits(ext)) { num = 0.5f * x - 0.5f * lo; ext = 0.5f * hi - 0.5f * lo; }
    if (!(ext > 0.f)) return 0u;
    const float t = (num / ext) * (float)KEY_MAX_AXIS;
    if (!(t > 0.f)) return 0u;
    return t >= (float)KEY_MAX_AXIS ? KEY_MAX_AXIS : (uint32_t)t;
}

// bit i of v -> bit 3 i
GS_HD uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// lo / hi: the bounding box of the finite rows.  A non-finite row: KEY_NONFINITE, so that the sort puts it behind all others.
GS_HD uint64_t morton_key(float x, float y, float z, const float lo[3], const float hi[3]) {
    if (!finite_row(x, y, z)) return KEY_NONFINITE;
    return spread3(key_axis(x, lo[0], hi[0])) | (spread3(key_axis(y, lo[1], hi[1])) << 1) | (spread3(key_axis(z, lo[2], hi[2])) << 2);
}

}  // namespace gsknn

#if defined(__clang__)
#pragma clang fp contract(on)     // what gs_math.h set for the headers that follow it
#endif
