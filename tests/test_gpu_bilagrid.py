"""Per-view bilateral grids on the MI355X: the kernels through the C entries against the float64 oracle
(tests/bilagrid_oracle.py) -- rounding bounds on random floats, bit for bit on dyadic ones --, the identity, bit stability, the flags,
the total variation, the autograd ops against the loss kernel's own gradient, and two ranks against one process.  The rest of the
trainer mode: tests/test_gpu_view_tables.py."""
import ctypes as C
import functools
import importlib
import os
import types

import numpy as np
import pytest
import torch

from tests import bilagrid_oracle as bo
from tests.view_table_harness import (DEV, PKG, ROOT, _dev, _header_constant, _p, _same, _stream, _two_ranks_against_one_process,
                                      deterministic)  # noqa: F401  (deterministic: a fixture)

U = 2.0 ** -24
pytestmark = pytest.mark.gpu

abi = importlib.import_module(PKG + "._abi")
ACC = abi.GSPLAT_BILAGRID_ACCUMULATE


THREADS, WAVE_SPAN, BLOCK_SPAN, SUM_DEPTH_FIXED, LEVEL_GROUP, STAGE_FLOATS = (_header_constant("gs_bilagrid.h", "BILAGRID_" + name) for name in (
    "THREADS", "WAVE_PIX", "BLOCK_PIX", "SUM_DEPTH_FIXED", "LEVEL_GROUP", "STAGE_FLOATS"))
# roundings of one pixel's chain in gs_bilagrid.h, counted from the source (tests/test_bilagrid_cpu.py spells the count out): the slice
# and the affine 9; g_image 14; one term of the grid gradient 7; a coordinate 4 (the magnitudes hold |coordinate| |d / d coordinate|)
PIXEL_DEPTH, IMAGE_GRAD_DEPTH, TERM_DEPTH, COORD_DEPTH = 9, 14, 7, 4
DEFAULT = (16, 16, 8)
# (1, 1), (1, 5); one pixel below, at and above a wave's and a workgroup's span of the per-pixel kernels; an odd frame; several
# workgroups with a ragged last one
SHAPES = [(1, 1), (1, 5), (1, WAVE_SPAN - 1), (1, WAVE_SPAN), (1, WAVE_SPAN + 1), (1, BLOCK_SPAN - 1), (1, BLOCK_SPAN), (1, BLOCK_SPAN + 1),
          (17, 33), (70, 130)]
# every image shape under a small odd grid and under the default one; the two frames under (2, 2, 2) -- one cell covers the frame, so
# one gather workgroup walks every pixel over many loop iterations -- and under a grid of 16 levels (two level groups); an image smaller
# than the grid: most vertices see no pixel.  The per-pixel kernels stage a workgroup's block of vertices in LDS up to STAGE_FLOATS
# and read global memory beyond: most of the above are staged (17 x 33 under the default grid: one workgroup of three); under
# (64, 8, 16) no workgroup of the two frames is, and under (16, 16, 16) some of the 70 x 130 frame are and some are not (_staged_blocks)
CASES = ([(b, h, w, g) for h, w in SHAPES for b in (1, 3) for g in ((3, 5, 4), DEFAULT)]
         + [(b, h, w, g) for h, w in ((17, 33), (70, 130)) for b in (1, 3) for g in ((2, 2, 2), (4, 3, 16), (64, 8, 16))]
         + [(b, 70, 130, (16, 16, 16)) for b in (1, 3)]
         + [(b, 5, 7, DEFAULT) for b in (1, 3)])


def _staged_blocks(h, w, shape):
    """Per workgroup of the per-pixel kernels: does its block of vertices fit the LDS stage?  The kernel's own arithmetic, in fp32."""
    X, Y, L = shape
    f = np.float32

    def cell(k, n, m):
        return min(int((f(k) + f(0.5)) / f(n) * f(m - 1)), m - 2)
    out = []
    for first in range(0, h * w, BLOCK_SPAN):
        last = min(first + BLOCK_SPAN, h * w) - 1
        ny = cell(last // w, h, Y) - cell(first // w, h, Y) + 2
        nx = cell(last % w, w, X) - cell(first % w, w, X) + 2 if first // w == last // w else X
        out.append(12 * L * ((ny * nx) | 1) <= STAGE_FLOATS)       # (a level's block is padded to an odd number of floats)
    return out


def test_the_spans_are_what_the_shapes_assume():
    assert (THREADS, WAVE_SPAN, BLOCK_SPAN, SUM_DEPTH_FIXED, LEVEL_GROUP, STAGE_FLOATS) == (256, 64, 256, 13, 8, 8192)
    assert all(all(_staged_blocks(h, w, g)) for _, h, w, g in CASES if 12 * g[2] * (g[0] * g[1] | 1) <= STAGE_FLOATS)       # a grid that fits whole
    assert all(_staged_blocks(70, 130, DEFAULT)) and all(_staged_blocks(1, BLOCK_SPAN + 1, DEFAULT))
    assert not any(_staged_blocks(17, 33, (64, 8, 16)) + _staged_blocks(70, 130, (64, 8, 16)))
    for mixed in (_staged_blocks(70, 130, (16, 16, 16)), _staged_blocks(17, 33, DEFAULT)):
        assert any(mixed) and not all(mixed)
    assert any(g[2] > LEVEL_GROUP for _, _, _, g in CASES), "a grid with more levels than one group"


@functools.lru_cache(maxsize=None)
def _host():
    lib = C.CDLL(os.path.join(ROOT, PKG, "csrc", "libgsbilagrid_host.so"))
    lib.hbila_gather_thread_pixels.argtypes = [C.c_int32] * 4
    lib.hbila_gather_thread_pixels.restype = C.c_int64
    return lib


def _grid_depth(h, w, shape):
    """fp32 additions between a term of the grid gradient and its sum, from the header's documented chain: the thread's own pixels
    (gather_thread_pixels), the ladder and the waves (BILAGRID_SUM_DEPTH_FIXED)."""
    return int(_host().hbila_gather_thread_pixels(h, w, shape[0], shape[1])) + SUM_DEPTH_FIXED


# ---- the entries, called directly ------------------------------------------------------------------------------------------------
def _xyl(G):
    return G.shape[-1], G.shape[-2], G.shape[-3]


def _forward(x, G):
    b, h, w = x.shape[:3]
    out = torch.empty((b, h, w, 3), dtype=torch.float32, device=DEV)
    abi.check(abi.lib().gsplat_bilagrid_forward(_p(x), _p(G), b, h, w, *_xyl(G), _p(out), _stream()), "gsplat_bilagrid_forward")
    return out


def _backward(x, G, g, image=True, grids=True, dest=None, rows=None, flags=0):
    """(g_image, g_grids).  dest: the [rows, 12, L, Y, X] tensor the grid gradients go to (a fresh NaN-filled [B, ...] by default)."""
    b, h, w = x.shape[:3]
    g_image = torch.full((b, h, w, 3), float("nan"), dtype=torch.float32, device=DEV) if image else None
    if grids and dest is None:
        dest = torch.full(tuple(G.shape), float("nan"), dtype=torch.float32, device=DEV)
    abi.check(abi.lib().gsplat_bilagrid_backward(_p(x), _p(G), _p(g), b, h, w, *_xyl(G), _p(g_image), _p(dest) if grids else None, _p(rows),
                                                 flags, _stream()), "gsplat_bilagrid_backward")
    return g_image, (dest if grids else None)


def _tv(table, scale=1.0, loss=True, grad=True, dest=None, flags=0):
    lib = abi.lib()
    V = table.shape[0]
    X, Y, L = _xyl(table)
    out = torch.full((), float("nan"), dtype=torch.float32, device=DEV) if loss else None
    if grad and dest is None:
        dest = torch.full(tuple(table.shape), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.empty(lib.gsplat_bilagrid_tv_scratch_bytes(V, X, Y, L), dtype=torch.uint8, device=DEV) if loss else None
    abi.check(lib.gsplat_bilagrid_tv(_p(table), V, X, Y, L, scale, _p(out), _p(dest) if grad else None, flags, _p(scratch), _stream()),
              "gsplat_bilagrid_tv")
    return out, (dest if grad else None)


@functools.lru_cache(maxsize=None)
def _random(b, h, w, shape):
    """One random case and everything the oracle says about it, computed once: (image, grids, g_out) fp32 on the host, and the
    float64 results with their magnitudes."""
    image, grids, g_out = bo.random_case(1000 * b + 7 * h + w + 100000 * sum(shape), b, h, w, shape)
    g_image, g_grids = bo.backward(image, grids, g_out)
    m_image, m_grids = bo.backward_magnitude(image, grids, g_out)
    f32 = np.float32
    return types.SimpleNamespace(image=image.astype(f32), grids=grids.astype(f32), g_out=g_out.astype(f32), out=bo.forward(image, grids),
                                 mag=bo.magnitude(image, grids), g_image=g_image, g_grids=g_grids, m_image=m_image, m_grids=m_grids)


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _worst(err, mag):
    return float((err / np.maximum(mag, 1e-300)).max() / U)


def _check_against_oracle(r, out, g_image, g_grids, h, w, shape):
    if out is not None:
        err = np.abs(_f64(out).reshape(r.out.shape) - r.out)
        assert (err <= (PIXEL_DEPTH + COORD_DEPTH) * U * r.mag).all(), _worst(err, r.mag)
    if g_image is not None:
        err = np.abs(_f64(g_image).reshape(r.g_image.shape) - r.g_image)
        assert (err <= (IMAGE_GRAD_DEPTH + COORD_DEPTH) * U * r.m_image).all(), _worst(err, r.m_image)
    if g_grids is not None:
        depth = _grid_depth(h, w, shape) + TERM_DEPTH + COORD_DEPTH
        err = np.abs(_f64(g_grids).reshape(r.g_grids.shape) - r.g_grids)
        print(f"g_grids: worst error {_worst(err, r.m_grids):.2f} x 2^-24 of the magnitude, bound {depth}")
        assert (err <= depth * U * r.m_grids).all(), _worst(err, r.m_grids)
        assert (_f64(g_grids).reshape(r.g_grids.shape)[r.m_grids == 0] == 0).all(), "a vertex no pixel reaches must be an exact zero"


@pytest.mark.parametrize("b,h,w,shape", CASES)
def test_kernels_match_the_oracle_on_random_floats(b, h, w, shape):
    """Forward, g_image and g_grids within (depth + slack) 2^-24 of the oracle's magnitudes, the depths counted from the header's chain;
    each half of the backward alone gives the same bits and leaves the other unwritten."""
    r = _random(b, h, w, shape)
    x, G, g = _dev(r.image, r.grids, r.g_out)
    out = _forward(x, G)
    g_image, g_grids = _backward(x, G, g)
    _check_against_oracle(r, out, g_image, g_grids, h, w, shape)
    if (h, w) == (5, 7):
        assert (r.m_grids == 0).mean() > 0.5, "most vertices of the default grid see no pixel of a 5 x 7 image"
    only_image, none = _backward(x, G, g, grids=False)
    none2, only_grids = _backward(x, G, g, image=False)
    assert none is None and none2 is None and _same(only_image, g_image) and _same(only_grids, g_grids)


def _dyadic(b, h, w, shape, seed):
    """Pixel centres on dyadic fractions of a cell, grey colours 0 and 1 (luminance exactly 0 and 1: on a level), g_o in 64ths: every
    weight, product and partial sum is exact in fp32."""
    rng = np.random.default_rng(seed)
    image = np.repeat(rng.integers(0, 2, (b, h, w, 1)), 3, axis=3).astype(np.float32)
    g_out = (rng.integers(-64, 65, (b, h, w, 3)) / 64).astype(np.float32)
    grids = (bo.identity(b, shape) + rng.integers(-4, 5, (b, 12, shape[2], shape[1], shape[0])) / 8).astype(np.float32)
    return image, grids, g_out


@pytest.mark.parametrize("b,h,w,shape", [(1, 8, 32, (5, 3, 2)), (3, 8, 32, (5, 3, 2)), (3, 16, 32, (3, 3, 3)), (1, 16, 16, (2, 2, 2)),
                                         (3, 4, 4, (16, 16, 8))])
def test_g_grids_is_exact_on_dyadic_inputs(b, h, w, shape):
    """W a power-of-two multiple of X - 1 and H of Y - 1 (or the reverse: 15 cells over 4 pixels): u and v are dyadic and exact, the
    weights are products of dyadic fractions, and with the inputs of _dyadic every sum is exact -- the result equals the float64 sum
    bit for bit, so a dropped or doubled pixel, vertex or level cannot hide in a rounding bound."""
    image, grids, g_out = _dyadic(b, h, w, shape, 5000 + h + w + sum(shape))
    x, G, g = _dev(image, grids, g_out)
    _, g_grids = _backward(x, G, g, image=False)
    want = bo.backward(image, grids, g_out)[1]
    assert want.any() and np.array_equal(_f64(g_grids), want)


@pytest.mark.parametrize("b,h,w,shape", [(1, 1, 1, (2, 2, 2)), (1, 1, 5, DEFAULT), (3, 1, BLOCK_SPAN + 1, (3, 5, 4)), (1, 17, 33, DEFAULT),
                                         (3, 70, 130, (4, 3, 16)), (1, 17, 33, (64, 8, 16)), (3, 70, 130, (16, 16, 16))])
def test_the_identity_table_is_bit_exact(b, h, w, shape):
    rng = np.random.default_rng(9000 + h + w)

    def wide(shape):                              # finite floats over 120 binades, both signs
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-60, 61, shape)).astype(np.float32)
    x, g = _dev(wide((b, h, w, 3)), wide((b, h, w, 3)))
    unit = _dev(rng.uniform(-0.5, 1.5, (b, h, w, 3)))[0]          # colours around [0, 1]: every level is met
    G = _dev(bo.identity(b, shape))[0]
    for image in (x, unit):
        g_image, _ = _backward(image, G, g, grids=False)
        assert _same(_forward(image, G), image) and _same(g_image, g)


@pytest.mark.parametrize("b,h,w,shape", [(1, 70, 130, DEFAULT), (3, 17, 33, (3, 5, 4)), (1, 1, 5, (2, 2, 2))])
def test_a_misaligned_buffer_changes_no_bit(b, h, w, shape):
    """Every array as a view one float into a larger buffer (4 bytes off a 16-byte boundary)."""
    r = _random(b, h, w, shape)
    x, G, g = _dev(r.image, r.grids, r.g_out)

    def shifted(t):
        buf = torch.empty(t.numel() + 5, dtype=torch.float32, device=DEV)
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    xs, Gs, gs_ = shifted(x), shifted(G), shifted(g)
    want_image, want_grids = _backward(x, G, g)
    assert _same(_forward(xs, Gs), _forward(x, G))
    got_image, got_grids = _backward(xs, Gs, gs_, dest=shifted(torch.zeros_like(G)))
    assert _same(got_image, want_image) and _same(got_grids, want_grids)


def test_the_gradient_is_the_same_bits_every_time():
    b, h, w, shape = 3, 70, 130, DEFAULT
    r = _random(b, h, w, shape)
    x, G, g = _dev(r.image, r.grids, r.g_out)
    g_image, g_grids = _backward(x, G, g)
    for _ in range(3):
        again_image, again_grids = _backward(x, G, g)
        assert _same(again_image, g_image) and _same(again_grids, g_grids)
    torch.cuda.synchronize()
    other = torch.cuda.Stream(DEV)
    with torch.cuda.stream(other):
        side_image, side_grids = _backward(x, G, g)
        side_out = _forward(x, G)
    other.synchronize()
    assert _same(side_image, g_image) and _same(side_grids, g_grids) and _same(side_out, _forward(x, G))
    # a batch of three equals three single calls
    for k in range(b):
        one_image, one_grids = _backward(x[k:k + 1], G[k:k + 1], g[k:k + 1])
        assert _same(one_image[0], g_image[k]) and _same(one_grids[0], g_grids[k]), k
        assert _same(_forward(x[k:k + 1], G[k:k + 1])[0], side_out[k])


@pytest.mark.parametrize("h,w,shape", [(17, 33, (3, 5, 4)), (5, 7, DEFAULT)])
def test_the_add_flag_and_the_row_index(h, w, shape):
    b = 3
    r = _random(b, h, w, shape)
    x, G, g = _dev(r.image, r.grids, r.g_out)
    _, stored = _backward(x, G, g)
    # the add flag on pre-filled rows = store, then add on the host; a vertex no pixel reaches is untouched
    filled = torch.tensor(np.random.default_rng(3).normal(0, 1, tuple(G.shape)).astype(np.float32), device=DEV)
    want = (filled.cpu() + stored.cpu())
    _, added = _backward(x, G, g, image=False, dest=filled.clone(), flags=ACC)
    assert _same(added.cpu(), want)
    untouched = torch.tensor(r.m_grids == 0)
    assert _same(added.cpu()[untouched], filled.cpu()[untouched]) and (untouched.any() or shape != DEFAULT)
    # a row_index writes only the rows it names: the others keep their sentinel
    sentinel = -123.25
    table = torch.full((7,) + tuple(G.shape[1:]), sentinel, dtype=torch.float32, device=DEV)
    rows = torch.tensor([5, 0, 2], dtype=torch.int32, device=DEV)
    _backward(x, G, g, image=False, dest=table, rows=rows)
    for k, row in enumerate((5, 0, 2)):
        assert _same(table[row], stored[k]), row
    assert (table[[1, 3, 4, 6]] == sentinel).all()
    _backward(x, G, g, image=False, dest=table, rows=rows, flags=ACC)
    for k, row in enumerate((5, 0, 2)):
        assert _same(table[row], stored[k] + stored[k]), row
    assert (table[[1, 3, 4, 6]] == sentinel).all()
    # a negative entry drops its image
    table.fill_(sentinel)
    _backward(x, G, g, image=False, dest=table, rows=torch.tensor([1, -1, 3], dtype=torch.int32, device=DEV))
    assert _same(table[1], stored[0]) and _same(table[3], stored[2]) and (table[[0, 2, 4, 5, 6]] == sentinel).all()


@pytest.mark.parametrize("shape", [(3, 5, 4), DEFAULT])
def test_black_and_white_pixels_get_no_luminance_derivative(shape):
    """Rows of exactly black, exactly white and beyond-white pixels (and one inner row): the oracle's g_image has no luminance term
    there and neither has its magnitude, so the bound is the affine's transpose alone."""
    h, w = 4, 40
    _, grids, g_out = bo.random_case(77, 1, h, w, shape, spread=0.5)
    image = np.zeros((1, h, w, 3))
    image[0, 1] = 1.0
    image[0, 2] = (1.5, 1.25, 0.875)
    image[0, 3] = (0.25, 0.5, 0.75)
    x, G, g = _dev(image, grids, g_out)
    g_image, _ = _backward(x, G, g, grids=False)
    want, _ = bo.backward(image, grids, g_out)
    mag, _ = bo.backward_magnitude(image, grids, g_out)
    inside = (bo.luminance(image) > 0) & (bo.luminance(image) < 1)
    assert inside[0, 3].all() and not inside[0, :3].any()
    err = np.abs(_f64(g_image) - want)
    assert (err <= (IMAGE_GRAD_DEPTH + COORD_DEPTH) * U * mag).all(), _worst(err, mag)
    # and a black pixel (fz = 0 exactly) reads level 0 alone: with every level a copy of level 0 no bit of its row moves
    flat, _ = _backward(x, _dev(np.broadcast_to(grids[:, :, :1], grids.shape))[0], g, grids=False)
    assert _same(g_image[0, 0], flat[0, 0])


# ---- the total variation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,shape", [(1, (2, 2, 2)), (3, (3, 5, 4)), (5, DEFAULT), (2, (4, 3, 16))])
def test_tv_matches_the_oracle_and_its_bits_are_stable(V, shape):
    X, Y, L = shape
    table = (bo.identity(V, shape) + np.random.default_rng(31 + V).normal(0, 0.2, (V, 12, L, Y, X))).astype(np.float32)
    want, want_grad = bo.tv(table)
    m, m_grad = bo.tv_magnitude(table)
    t = _dev(table)[0]
    loss, grad = _tv(t, scale=10.0)
    # the loss: differences rounded to fp32 (twice in the square), the sums in double, scale and the final rounding to fp32
    assert abs(float(loss) - 10 * want) <= 4 * U * 10 * m
    # the gradient, per axis: the factor, two differences, their difference, the fma = 5; two more additions along the chain of three
    err = np.abs(_f64(grad) - 10 * want_grad)
    assert (err <= 7 * U * 10 * m_grad).all(), _worst(err, 10 * m_grad)
    for _ in range(2):
        loss2, grad2 = _tv(t, scale=10.0)
        assert _same(loss2, loss) and _same(grad2, grad)
    only_loss, none = _tv(t, scale=10.0, grad=False)
    none2, only_grad = _tv(t, scale=10.0, loss=False)
    assert none is None and none2 is None and _same(only_loss, loss) and _same(only_grad, grad)
    filled = torch.tensor(np.random.default_rng(4).normal(0, 1, table.shape).astype(np.float32), device=DEV)
    _, added = _tv(t, scale=10.0, loss=False, dest=filled.clone(), flags=ACC)
    assert _same(added, filled + grad)


def test_tv_is_exactly_zero_on_the_identity_table():
    t = _dev(bo.identity(100, DEFAULT))[0]
    loss, grad = _tv(t, scale=10.0)
    assert float(loss) == 0.0 and not grad.any()


# ---- the autograd ops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
def test_autograd_through_the_loss_matches_the_oracle(gs, batched):
    """compute_loss(bilagrid.slice(img, G), gt).backward(): img.grad and G.grad equal the oracle fed with the loss kernel's own
    gradient, within the bounds of the kernels; the half nobody needs is not computed."""
    b, h, w, shape = (3, 17, 33, (3, 5, 4)) if batched else (1, 70, 130, DEFAULT)
    r = _random(b, h, w, shape)
    ishape = (b, h, w, 3) if batched else (h, w, 3)
    image, grids = r.image.reshape(ishape), (r.grids if batched else r.grids[0])
    gt = torch.tensor(np.random.default_rng(8).uniform(0, 1, ishape).astype(np.float32), device=DEV)
    img = torch.tensor(image, device=DEV, requires_grad=True)
    G = torch.tensor(grids, device=DEV, requires_grad=True)
    out = gs.bilagrid.slice(img, G)
    assert _same(out, _forward(img.detach().view(b, h, w, 3), G.detach().view((b,) + r.grids.shape[1:])).view(ishape))
    gs.compute_loss(out, gt)[0].backward()
    leaf = out.detach().clone().requires_grad_(True)                     # the loss kernel's own gradient at the same image
    gs.compute_loss(leaf, gt)[0].backward()
    g_out = leaf.grad.cpu().numpy()
    want_image, want_grids = bo.backward(image, grids, g_out)
    m_image, m_grids = bo.backward_magnitude(image, grids, g_out)
    assert (np.abs(_f64(img.grad) - want_image) <= (IMAGE_GRAD_DEPTH + COORD_DEPTH) * U * m_image).all()
    assert tuple(G.grad.shape) == tuple(G.shape)
    assert (np.abs(_f64(G.grad) - want_grids) <= (_grid_depth(h, w, shape) + TERM_DEPTH + COORD_DEPTH) * U * m_grids).all()
    # one input alone: the same bits, and the entry is not asked for the other half
    lib, calls = abi.lib(), []
    real = lib.gsplat_bilagrid_backward

    def spy(*args):
        calls.append((args[9] is not None, args[10] is not None))
        return real(*args)
    lib.gsplat_bilagrid_backward = spy
    try:
        img2 = img.detach().clone().requires_grad_(True)
        gs.compute_loss(gs.bilagrid.slice(img2, G.detach()), gt)[0].backward()
        G2 = G.detach().clone().requires_grad_(True)
        gs.compute_loss(gs.bilagrid.slice(img.detach(), G2), gt)[0].backward()
    finally:
        lib.gsplat_bilagrid_backward = real
    assert calls == [(True, False), (False, True)]
    assert _same(img2.grad, img.grad) and _same(G2.grad, G.grad)


def test_other_dtypes_are_converted_and_tv_loss_differentiates(gs):
    shape = (3, 5, 4)
    r = _random(1, 17, 33, shape)
    img = torch.tensor(r.image[0], device=DEV, dtype=torch.float64, requires_grad=True)
    G = torch.tensor(r.grids[0], device=DEV, dtype=torch.float64, requires_grad=True)
    out = gs.bilagrid.slice(img, G)
    assert out.dtype == torch.float64
    out.backward(torch.tensor(r.g_out[0], device=DEV, dtype=torch.float64))
    assert img.grad.dtype == torch.float64 and G.grad.dtype == torch.float64
    _check_against_oracle(types.SimpleNamespace(**{k: v[0] for k, v in vars(r).items()}), out, img.grad, G.grad, 17, 33, shape)
    table = torch.tensor(r.grids, device=DEV, requires_grad=True)
    (3.0 * gs.bilagrid.tv_loss(table)).backward()
    want, want_grad = bo.tv(r.grids)
    m, m_grad = bo.tv_magnitude(r.grids)
    assert (np.abs(_f64(table.grad) - 3 * want_grad) <= 8 * U * 3 * m_grad).all()
    assert abs(float(gs.bilagrid.tv_loss(table)) - want) <= 4 * U * m


# ---- data parallel -----------------------------------------------------------------------------------------------------------------
def test_two_ranks_end_with_the_bits_of_one_process_given_both_views(deterministic):
    """Two ranks (gloo, both on cuda:0), one view each, three iterations with the default TV weight: the table's gradient is
    all-reduced once per iteration and the TV term joins it AFTER that -- counted once, not once per rank: from the second iteration on
    the grids are not flat, and a TV gradient counted twice would change the table's bits.  Table and model are bit for bit those of
    one process given both views, and so is the TV term of every iteration.  (sparse_adam: the route on which one process forms the SH
    gradients as a group of ranks does, so that the MODEL can be compared bit for bit too.)"""
    table, tv = _two_ranks_against_one_process(deterministic, "bilagrid", (1, 2, 3))
    assert tv[0] == 0.0 and tv[1] > 0 and tv[2] > 0
    assert table["grad"][0].any() and table["grad"][2].any()
