"""Reference of the two feature kernels (raster_features_kernel, raster_features_adjoint_kernel): a thin layer over
tests/raster_oracle.py, three channels at a time, on the SAME records and lists the kernels read.  Plain numpy, no torch, no GPU.

`args` is what raster_oracle.composite takes first: (rec, ranges, sorted_ids, lists_x, H, W, chi, alpha_max, alpha_cutoff).

The map F[p, c] = sum_i w_i(p) f_i[c]: a slab of three feature columns is written into the colour columns 8-10 of the records and the
map is composite(...).accum, the unclamped C, so signed features are fine; scale = scale_img["accum"] (1 + sum w |f|), band allowance
= allow_img["accum"].

The adjoint g_i[c] = sum_p w_i(p) G[p, c] does not depend on the features: the colour columns hold the constant 0.5, so the shown colour
is 0.5 A in [0, 0.5] and the clamp mask is always open, and with g_img = a slab of G the columns 6-8 of composite's rows are sum w G;
scale and allowance are the same columns of composite's scale and allow.

The float32 twins (render_f32, adjoint_f32) go through raster_oracle.composite_f32 the same way: the calibration.  A kernel is held to
    |delta| <= K 2^-24 scale + allowance,      K = 3 x the largest ratio of the float32 twin against the float64 reference,
and nothing is left out of a comparison: band pixels and rows are compared with their allowance added, exactly as raster_oracle.check
does."""
import numpy as np

from tests import raster_oracle as ro

EPS = ro.EPS


class FeatureError(AssertionError):
    pass


class Ref:
    """value, scale, allow: arrays of one shape ([H,W,C] for the map, [n,C] for the adjoint); in_list [n] (adjoint)."""

    def __init__(self, value, scale, allow, in_list=None):
        self.value, self.scale, self.allow, self.in_list = value, scale, allow, in_list


def _slabs(C):
    return [(k, min(k + 3, C)) for k in range(0, C, 3)]


def _slab(a, k0, k1):
    """Columns k0:k1 of the last axis, padded with zeros to three."""
    out = np.zeros(a.shape[:-1] + (3,), a.dtype)
    out[..., :k1 - k0] = a[..., k0:k1]
    return out


def _with_colour(rec, colour, dtype):
    r = np.array(rec, dtype)
    r[:, 8:11] = colour
    return r


def render(args, feats):
    """Ref of the map [H,W,C] of the table feats [n,C], in float64."""
    rec, rest = args[0], args[1:]
    feats = np.asarray(feats, np.float64)
    H, W, C = args[4], args[5], feats.shape[1]
    val, scale, allow = np.zeros((H, W, C)), np.ones((H, W, C)), np.zeros((H, W, C))
    for k0, k1 in _slabs(C):
        ref = ro.composite(_with_colour(rec, _slab(feats, k0, k1), np.float64), *rest)
        val[..., k0:k1], scale[..., k0:k1], allow[..., k0:k1] = (a[..., :k1 - k0] for a in (ref.accum, ref.scale_img["accum"], ref.allow_img["accum"]))
    return Ref(val, scale, allow)


def render_f32(args, feats):
    """The map in float32, in the kernels' order of operations (raster_oracle.composite_f32)."""
    rec, rest = args[0], args[1:]
    feats = np.asarray(feats, np.float32)
    H, W, C = args[4], args[5], feats.shape[1]
    val = np.zeros((H, W, C), np.float32)
    for k0, k1 in _slabs(C):
        val[..., k0:k1] = ro.composite_f32(_with_colour(rec, _slab(feats, k0, k1), np.float32), *rest)["accum"][..., :k1 - k0]
    return val


def adjoint(args, G):
    """Ref of the rows [n,C] of the upstream map G [H,W,C], in float64."""
    rec, rest = args[0], args[1:]
    G = np.asarray(G, np.float64)
    n, C = len(rec), G.shape[2]
    half = _with_colour(rec, 0.5, np.float64)
    val, scale, allow = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C))
    in_list = None
    for k0, k1 in _slabs(C):
        ref = ro.composite(half, *rest, g_img=_slab(G, k0, k1))
        assert ref.dec["col"].all(), "the shown colour 0.5 A must leave the clamp mask open"
        val[:, k0:k1], scale[:, k0:k1], allow[:, k0:k1] = (a[:, 6:6 + k1 - k0] for a in (ref.rows, ref.scale, ref.allow))
        in_list = ref.in_list
    return Ref(val, scale, allow, in_list)


def adjoint_f32(args, G):
    rec, rest = args[0], args[1:]
    G = np.asarray(G, np.float32)
    n, C = len(rec), G.shape[2]
    half = _with_colour(rec, 0.5, np.float32)
    val = np.zeros((n, C), np.float32)
    for k0, k1 in _slabs(C):
        val[:, k0:k1] = ro.composite_f32(half, *rest, g_img=_slab(G, k0, k1))["grad2d"][:, 6:6 + k1 - k0]
    return val


def ratio(got, ref, calls=1):
    """Largest (|delta| - allowance)+ / (2^-24 scale) of `got` against `calls` x the reference."""
    d = np.maximum(np.abs(np.asarray(got, np.float64) - calls * ref.value) - calls * ref.allow, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(d > 0, d / (EPS * calls * ref.scale), 0.0)
    return float(x.max(initial=0.0))


def calibrate_render(args, feats):
    """(K, reference) of the map: K = 3 x the ratio of the float32 twin, never measured against a kernel."""
    ref = render(args, feats)
    return 3.0 * ratio(render_f32(args, feats), ref), ref


def calibrate_adjoint(args, G):
    """(K, reference) of the adjoint's rows."""
    ref = adjoint(args, G)
    return 3.0 * ratio(adjoint_f32(args, G), ref), ref


def calibration(args, feats, G):
    """(K_map, K_rows, map reference, rows reference)."""
    (K_map, fwd), (K_rows, adj) = calibrate_render(args, feats), calibrate_adjoint(args, G)
    return K_map, K_rows, fwd, adj


def check(got, ref, K, what="", calls=1, factor=1.0):
    """Every value of `got` within factor x calls x (K 2^-24 scale + allowance) of calls x the reference; the rows of Gaussians in no
    list (adjoint) exact zeros.  Raises FeatureError naming the pixel or the Gaussian and the channel.  Returns ratio(got, ref, calls)."""
    g = np.asarray(got, np.float64)
    if g.shape != ref.value.shape or not np.isfinite(g).all():
        raise FeatureError(f"{what}: shape {g.shape} (expected {ref.value.shape}) or non-finite values")
    if ref.in_list is not None:
        bad = np.argwhere((g != 0) & ~ref.in_list[:, None])
        if len(bad):
            raise FeatureError(f"{what}: Gaussian {bad[0][0]} is in no list, channel {bad[0][1]} of its row is {g[tuple(bad[0])]!r}")
    bound = factor * calls * (K * EPS * ref.scale + ref.allow)
    d = np.abs(g - calls * ref.value)
    bad = np.argwhere(d > bound)
    if len(bad):
        with np.errstate(divide="ignore", invalid="ignore"):
            over = np.where(bound > 0, d / bound, np.inf)
        i = tuple(bad[np.argmax(over[tuple(bad.T)])])
        where = f"pixel ({i[0]}, {i[1]}) channel {i[2]}" if len(i) == 3 else f"Gaussian {i[0]}, channel {i[1]}"
        raise FeatureError(f"{what}: {where}: {g[i]!r}, reference {calls * ref.value[i]!r}: |delta| {d[i]:.3e} > {bound[i]:.3e} "
                           f"(= {factor * calls:g} x ({K:.1f} x 2^-24 x {ref.scale[i]:.3e} + {ref.allow[i]:.3e})); {len(bad)} values beyond their bounds")
    return ratio(got, ref, calls)
