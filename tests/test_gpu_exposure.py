"""Per-view exposure compensation on the MI355X: the three kernels through the C entries against the float64 oracle
(tests/exposure_oracle.py) -- rounding bounds on random floats, bit for bit on dyadic ones --, the identity, bit stability, the
autograd op against the loss kernel's own gradient, and two ranks against one process.  The rest of the trainer mode:
tests/test_gpu_view_tables.py."""
import functools
import importlib
import types

import numpy as np
import pytest
import torch

from tests import exposure_oracle as eo
from tests.view_table_harness import (DEV, PKG, _dev, _header_constant, _p, _same, _stream, _two_ranks_against_one_process,
                                      deterministic)  # noqa: F401  (deterministic: a fixture)

U = 2.0 ** -24
pytestmark = pytest.mark.gpu

abi = importlib.import_module(PKG + "._abi")


THREADS, PIX, SUM_DEPTH = (_header_constant("gs_exposure.h", name) for name in ("EXPOSURE_THREADS", "EXPOSURE_PIX", "EXPOSURE_SUM_DEPTH"))
WAVE_SPAN, BLOCK_SPAN = 64 * PIX, THREADS * PIX                      # pixels one wave / one workgroup owns
# (1, 1) .. (1, 5): below, at and above one thread's four pixels; one pixel below, at and above a wave's and a workgroup's span; an
# odd frame; several workgroups with a ragged last one
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 5), (1, WAVE_SPAN - 1), (1, WAVE_SPAN), (1, WAVE_SPAN + 1), (1, BLOCK_SPAN - 1), (1, BLOCK_SPAN),
          (1, BLOCK_SPAN + 1), (17, 33), (70, 130)]
CASES = [(b, h, w) for h, w in SHAPES for b in (1, 3)]


def test_the_spans_are_what_the_shapes_assume():
    assert (WAVE_SPAN, BLOCK_SPAN, SUM_DEPTH) == (256, 1024, 12)


# ---- the entries, called directly ------------------------------------------------------------------------------------------------
def _forward(x, e):
    b, h, w = x.shape[:3]
    out = torch.empty((b, h, w, 3), dtype=torch.float32, device=DEV)
    abi.check(abi.lib().gsplat_exposure_forward(_p(x), _p(e), b, h, w, _p(out), _stream()), "gsplat_exposure_forward")
    return out


def _backward(x, e, g, image=True, params=True, dest=None, rows=None, flags=0):
    """(g_image, g_params).  dest: the [rows, 12] tensor the sums go to (a fresh [B, 12] by default)."""
    lib = abi.lib()
    b, h, w = x.shape[:3]
    g_image = torch.empty((b, h, w, 3), dtype=torch.float32, device=DEV) if image else None
    if params and dest is None:
        dest = torch.full((b, 12), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.empty(lib.gsplat_exposure_scratch_bytes(b, h, w), dtype=torch.uint8, device=DEV) if params else None
    abi.check(lib.gsplat_exposure_backward(_p(x), _p(e), _p(g), b, h, w, _p(g_image), _p(dest) if params else None, _p(rows), flags,
                                           _p(scratch), _stream()), "gsplat_exposure_backward")
    return g_image, (dest if params else None)


@functools.lru_cache(maxsize=None)
def _random(b, h, w):
    """One random case and everything the oracle says about it, computed once: (image, params, g_out) fp32 on the host, and the
    float64 results with their magnitudes."""
    rng = np.random.default_rng(1000 * b + 7 * h + w)
    image = rng.uniform(0.0, 1.0, (b, h, w, 3)).astype(np.float32)
    params = (np.tile(np.eye(3, 4), (b, 1, 1)) + rng.normal(0.0, 0.2, (b, 3, 4))).astype(np.float32)         # three different rows
    g_out = rng.normal(0.0, 1.0, (b, h, w, 3)).astype(np.float32)
    g_image, g_params = eo.backward(image, params, g_out)
    m_image, m_params = eo.backward_magnitude(image, params, g_out)
    return types.SimpleNamespace(image=image, params=params, g_out=g_out, out=eo.forward(image, params), mag=eo.magnitude(image, params),
                                 g_image=g_image, g_params=g_params, m_image=m_image, m_params=m_params)


@pytest.mark.parametrize("b,h,w", CASES)
def test_kernels_match_the_oracle_on_random_floats(b, h, w):
    """Forward and g_image within 4 ulp-halves of the magnitude (a chain of at most four fmas); g_params within (d + 2) of them: d
    additions in fp32 inside one workgroup (gs_exposure.h), the product's rounding, the finish in double rounded once."""
    r = _random(b, h, w)
    x, e, g = _dev(r.image, r.params, r.g_out)
    out = _forward(x, e)
    g_image, g_params = _backward(x, e, g)
    err = np.abs(out.cpu().numpy().astype(np.float64) - r.out)
    assert (err <= 4 * U * r.mag).all(), float((err / r.mag).max() / U)
    err = np.abs(g_image.cpu().numpy().astype(np.float64) - r.g_image)
    assert (err <= 4 * U * r.m_image).all(), float((err / np.maximum(r.m_image, 1e-300)).max() / U)
    err = np.abs(g_params.cpu().numpy().astype(np.float64).reshape(b, 3, 4) - r.g_params)
    print(f"g_params: worst error {float((err / r.m_params).max() / U):.2f} x 2^-24 of the magnitude, bound {SUM_DEPTH + 2}")
    assert (err <= (SUM_DEPTH + 2) * U * r.m_params).all(), float((err / r.m_params).max() / U)
    # each half alone: the same bits, and the other half is not written
    only_image, none = _backward(x, e, g, params=False)
    none2, only_params = _backward(x, e, g, image=False)
    assert none is None and none2 is None and _same(only_image, g_image) and _same(only_params, g_params)


@pytest.mark.parametrize("b,h,w", CASES)
def test_g_params_is_exact_on_dyadic_inputs(b, h, w):
    """c in eighths of [0, 1], g_o in 64ths of [-1, 1]: every product and every partial sum is exact in fp32 (below 2^24 / 512 pixels
    per image), so the result equals the float64 sum bit for bit -- a dropped pixel, workgroup or row cannot hide in a rounding bound."""
    assert h * w * 512 < 2 ** 24
    rng = np.random.default_rng(5000 + 1000 * b + 7 * h + w)
    image = (rng.integers(0, 9, (b, h, w, 3)) / 8).astype(np.float32)
    g_out = (rng.integers(-64, 65, (b, h, w, 3)) / 64).astype(np.float32)
    params = (np.tile(np.eye(3, 4), (b, 1, 1)) + rng.integers(-4, 5, (b, 3, 4)) / 8).astype(np.float32)
    x, e, g = _dev(image, params, g_out)
    g_image, g_params = _backward(x, e, g)
    want_image, want_params = eo.backward(image, params, g_out)
    assert np.array_equal(g_params.cpu().numpy().astype(np.float64).reshape(b, 3, 4), want_params)
    assert np.array_equal(g_image.cpu().numpy().astype(np.float64), want_image)               # (dyadic parameters: exact too)
    assert np.array_equal(_forward(x, e).cpu().numpy().astype(np.float64), eo.forward(image, params))


@pytest.mark.parametrize("b,h,w", [(1, 1, 1), (1, 1, 5), (3, 1, BLOCK_SPAN + 1), (1, 17, 33), (3, 70, 130)])
def test_the_identity_table_is_bit_exact(b, h, w):
    rng = np.random.default_rng(9000 + h + w)

    def wide(shape):                              # finite floats over 120 binades, both signs
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-60, 61, shape)).astype(np.float32)
    x, g = _dev(wide((b, h, w, 3)), wide((b, h, w, 3)))
    e = torch.eye(3, 4, device=DEV).repeat(b, 1, 1).contiguous()
    g_image, _ = _backward(x, e, g)
    assert _same(_forward(x, e), x) and _same(g_image, g)


@pytest.mark.parametrize("b,h,w", [(1, 70, 130), (3, 17, 33), (1, 1, 5), (3, 1, BLOCK_SPAN)])
def test_a_misaligned_buffer_changes_no_bit(b, h, w):
    """Every array as a view one float into a larger buffer (4 bytes off a 16-byte boundary): the element-by-element path, the same
    bits as the 16-byte path of the aligned copies."""
    r = _random(b, h, w)
    x, e, g = _dev(r.image, r.params, r.g_out)

    def shifted(t):
        buf = torch.empty(t.numel() + 5, dtype=torch.float32, device=DEV)
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    xs, gs_ = shifted(x), shifted(g)
    assert _same(_forward(xs, e), _forward(x, e))
    want_image, want_params = _backward(x, e, g)
    got_image, got_params = _backward(xs, e, gs_)
    assert _same(got_image, want_image) and _same(got_params, want_params)
    got_image, got_params = _backward(x, e, gs_)                     # one misaligned array is enough to leave the 16-byte path
    assert _same(got_image, want_image) and _same(got_params, want_params)


def test_the_gradient_is_the_same_bits_every_time():
    b, h, w = 3, 70, 130
    r = _random(b, h, w)
    x, e, g = _dev(r.image, r.params, r.g_out)
    g_image, g_params = _backward(x, e, g)
    again_image, again_params = _backward(x, e, g)
    assert _same(again_image, g_image) and _same(again_params, g_params)
    torch.cuda.synchronize()
    other = torch.cuda.Stream(DEV)
    with torch.cuda.stream(other):
        side_image, side_params = _backward(x, e, g)
        side_out = _forward(x, e)
    other.synchronize()
    assert _same(side_image, g_image) and _same(side_params, g_params) and _same(side_out, _forward(x, e))
    # a batch of three equals three single calls
    for k in range(b):
        one_image, one_params = _backward(x[k:k + 1], e[k:k + 1], g[k:k + 1])
        assert _same(one_image[0], g_image[k]) and _same(one_params[0], g_params[k]), k
        assert _same(_forward(x[k:k + 1], e[k:k + 1])[0], side_out[k])


def test_the_add_flag_and_the_row_index():
    b, h, w = 3, 17, 33
    r = _random(b, h, w)
    x, e, g = _dev(r.image, r.params, r.g_out)
    _, stored = _backward(x, e, g)
    # the add flag on pre-filled rows = store, then add on the host
    filled = torch.tensor(np.random.default_rng(3).normal(0, 1, (b, 12)).astype(np.float32), device=DEV)
    want = (filled.cpu() + stored.cpu())
    _, added = _backward(x, e, g, image=False, dest=filled.clone(), flags=abi.GSPLAT_EXPOSURE_ACCUMULATE)
    assert _same(added.cpu(), want)
    # a row_index writes only the rows it names: the others keep their sentinel
    sentinel = -123.25
    table = torch.full((7, 12), sentinel, dtype=torch.float32, device=DEV)
    rows = torch.tensor([5, 0, 2], dtype=torch.int32, device=DEV)
    _backward(x, e, g, image=False, dest=table, rows=rows)
    for k, row in enumerate((5, 0, 2)):
        assert _same(table[row], stored[k]), row
    assert (table[[1, 3, 4, 6]] == sentinel).all()
    _backward(x, e, g, image=False, dest=table, rows=rows, flags=abi.GSPLAT_EXPOSURE_ACCUMULATE)
    for k, row in enumerate((5, 0, 2)):
        assert _same(table[row], stored[k] + stored[k]), row
    assert (table[[1, 3, 4, 6]] == sentinel).all()
    # a negative entry drops its row
    table.fill_(sentinel)
    _backward(x, e, g, image=False, dest=table, rows=torch.tensor([1, -1, 3], dtype=torch.int32, device=DEV))
    assert _same(table[1], stored[0]) and _same(table[3], stored[2]) and (table[[0, 2, 4, 5, 6]] == sentinel).all()


# ---- the autograd op ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
def test_autograd_through_the_loss_matches_the_oracle(gs, batched):
    """compute_loss(exposure.apply(img, E), gt).backward(): img.grad and E.grad equal the oracle fed with the loss kernel's own
    gradient, within the bounds of the kernels; the half nobody needs is not computed."""
    b, h, w = (3, 17, 33) if batched else (1, 70, 130)
    r = _random(b, h, w)
    shape = (b, h, w, 3) if batched else (h, w, 3)
    image, params = r.image.reshape(shape), (r.params if batched else r.params[0])
    gt = torch.tensor(np.random.default_rng(8).uniform(0, 1, shape).astype(np.float32), device=DEV)
    img = torch.tensor(image, device=DEV, requires_grad=True)
    E = torch.tensor(params, device=DEV, requires_grad=True)
    out = gs.exposure.apply(img, E)
    assert _same(out, _forward(img.detach().view(b, h, w, 3), E.detach().view(b, 12)).view(shape))
    gs.compute_loss(out, gt)[0].backward()
    leaf = out.detach().clone().requires_grad_(True)                     # the loss kernel's own gradient at the same image
    gs.compute_loss(leaf, gt)[0].backward()
    g_out = leaf.grad.cpu().numpy()
    want_image, want_params = eo.backward(image, params, g_out)
    m_image, m_params = eo.backward_magnitude(image, params, g_out)
    assert (np.abs(img.grad.cpu().numpy() - want_image) <= 4 * U * m_image).all()
    assert tuple(E.grad.shape) == tuple(E.shape)
    assert (np.abs(E.grad.cpu().numpy() - want_params) <= (SUM_DEPTH + 2) * U * m_params).all()
    # one input alone: the same bits, and the entry is not asked for the other half
    lib, calls = abi.lib(), []
    real = lib.gsplat_exposure_backward

    def spy(*args):
        calls.append((args[6] is not None, args[7] is not None))
        return real(*args)
    lib.gsplat_exposure_backward = spy
    try:
        img2 = img.detach().clone().requires_grad_(True)
        gs.compute_loss(gs.exposure.apply(img2, E.detach()), gt)[0].backward()
        E2 = E.detach().clone().requires_grad_(True)
        gs.compute_loss(gs.exposure.apply(img.detach(), E2), gt)[0].backward()
    finally:
        lib.gsplat_exposure_backward = real
    assert calls == [(True, False), (False, True)]
    assert _same(img2.grad, img.grad) and _same(E2.grad, E.grad)


def test_other_dtypes_are_converted(gs):
    r = _random(1, 17, 33)
    img = torch.tensor(r.image[0], device=DEV, dtype=torch.float64, requires_grad=True)
    E = torch.tensor(r.params[0], device=DEV, dtype=torch.float64, requires_grad=True)
    out = gs.exposure.apply(img, E)
    assert out.dtype == torch.float64
    out.backward(torch.tensor(r.g_out[0], device=DEV, dtype=torch.float64))
    assert img.grad.dtype == torch.float64 and E.grad.dtype == torch.float64
    assert (np.abs(out.detach().cpu().numpy() - r.out[0]) <= 4 * U * r.mag[0]).all()
    assert (np.abs(E.grad.cpu().numpy() - r.g_params[0]) <= (SUM_DEPTH + 2) * U * r.m_params[0]).all()


# ---- data parallel -----------------------------------------------------------------------------------------------------------------
def test_two_ranks_end_with_the_bits_of_one_process_given_both_views(deterministic):
    """(5) Two ranks (gloo, both on cuda:0), one view each, two iterations: the table's gradient is all-reduced once per iteration, and
    table and model are bit for bit those of one process given both views.  (sparse_adam: the route on which one process forms the SH
    gradients as a group of ranks does, so that the MODEL can be compared bit for bit too.)"""
    table, _ = _two_ranks_against_one_process(deterministic, "exposure", (1, 2))
    assert table["grad"][0].any() and table["grad"][2].any() and not table["grad"][1].any()
