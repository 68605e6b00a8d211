"""Per-view bilateral grids without a GPU: the four C entries exist with the stated argument counts and the ABI version
is still 12; every bad argument comes back as GSPLAT_ERR_BAD_ARG naming the entry before anything is launched; the TV scratch size
against the layout in the source; the host build of the per-pixel functions against the oracle within bounds counted from the header's
chain, the identity bit for bit; what TrainConfig / Trainer refuse; the data-parallel helper over gloo; no CPU fallback."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

from tests import bilagrid_oracle as bo
from tests.abi_checks import check_entries, header_defines, refused
from tests.ranks import run_ranks
from tests.util import zero_model

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = importlib.import_module(PKG + "._abi")
ENTRIES = {"gsplat_bilagrid_forward": 10, "gsplat_bilagrid_backward": 14, "gsplat_bilagrid_tv_scratch_bytes": 4, "gsplat_bilagrid_tv": 11}
HOST_LIB = os.path.join(ROOT, PKG, "csrc", "libgsbilagrid_host.so")
_F = C.POINTER(C.c_float)
U = 2.0 ** -24
# roundings of one pixel's chain in gs_bilagrid.h, counted from the source:
#   the slice: three lerps deep, each a subtraction and an fma = 6; the affine: 3 fmas                                  -> 9
#   g_image: the slice 6 + 3 fmas = 9 for the affine's transpose; the luminance term: D = b1 - b0 (5 up to there + 1),
#            its affine 3, the dot with g_o 3, (L - 1) x 1, the fma onto g_c 1 = 14; the two are added: the larger    -> 14
#   one term of the grid gradient: T 1, 1 - f twice, w_x w_y 1, 1 - fz or fz 1, x w_z 1, the fma 1                      -> 7
#   a coordinate: u and v two roundings (the division, the product), z four (the luminance's 3, x (L - 1)) -- the magnitudes hold
#   |coordinate| |d / d coordinate|, so these join the count                                                           -> 4
PIXEL_DEPTH, IMAGE_GRAD_DEPTH, TERM_DEPTH, COORD_DEPTH = 9, 14, 7, 4


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_mirror_and_library_agree_and_the_version_stays_12():
    check_entries(ENTRIES, family="bilagrid", stubs_in_namespace=True)
    assert header_defines()["GSPLAT_BILAGRID_ACCUMULATE"] == abi.GSPLAT_BILAGRID_ACCUMULATE == 1


def test_entries_refuse_bad_arguments_on_the_host():
    """A NULL required pointer, X, Y or L outside their ranges, H, W or batch <= 0, an unknown flag (first), a missing scratch:
    GSPLAT_ERR_BAD_ARG with a message naming the entry, with host addresses only -- nothing is launched."""
    lib = abi.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)

    def fwd(image=p, grids=p, batch=1, H=4, W=4, X=16, Y=16, L=8, out=p):
        return lib.gsplat_bilagrid_forward(image, grids, batch, H, W, X, Y, L, out, None)

    def bwd(image=p, grids=p, grad_out=p, batch=1, H=4, W=4, X=16, Y=16, L=8, grad_image=p, grad_grids=p, row_index=None, flags=0):
        return lib.gsplat_bilagrid_backward(image, grids, grad_out, batch, H, W, X, Y, L, grad_image, grad_grids, row_index, flags, None)

    def tv(grids=p, V=1, X=16, Y=16, L=8, scale=1.0, loss_out=p, grad=p, flags=0, scratch=p):
        return lib.gsplat_bilagrid_tv(grids, V, X, Y, L, scale, loss_out, grad, flags, scratch, None)

    grid_shapes = (dict(X=1), dict(X=0), dict(X=-5), dict(X=65), dict(Y=1), dict(Y=65), dict(Y=-1), dict(L=1), dict(L=0), dict(L=17), dict(L=-2))
    shapes = (dict(H=0), dict(H=-3), dict(H=(1 << 20) + 1), dict(W=0), dict(W=-1), dict(W=1 << 21), dict(H=1 << 16, W=1 << 16), dict(batch=0), dict(batch=-2), dict(batch=65536), dict(batch=1 << 40)) + grid_shapes
    for arg in ("image", "grids", "out"):
        refused(lib, fwd(**{arg: None}), "gsplat_bilagrid_forward", arg + " is NULL")
    for bad in shapes:
        refused(lib, fwd(**bad), "gsplat_bilagrid_forward", next(iter(bad)))
    for arg in ("image", "grids", "grad_out"):
        refused(lib, bwd(**{arg: None}), "gsplat_bilagrid_backward", arg + " is NULL")
    for bad in shapes:
        refused(lib, bwd(**bad), "gsplat_bilagrid_backward", next(iter(bad)))
    refused(lib, tv(grids=None), "gsplat_bilagrid_tv", "grids is NULL")
    refused(lib, tv(scratch=None), "gsplat_bilagrid_tv", "scratch is NULL")
    for bad in (dict(V=0), dict(V=-1), dict(V=1 << 40)) + grid_shapes:
        refused(lib, tv(**bad), "gsplat_bilagrid_tv", next(iter(bad)))
    for flags in (2, 4, 1 << 5, 3, -2, 1 << 30):
        refused(lib, bwd(flags=flags), "gsplat_bilagrid_backward", "unknown flag")
        refused(lib, bwd(flags=flags, image=None, H=0), "gsplat_bilagrid_backward", "unknown flag")      # refused FIRST
        refused(lib, tv(flags=flags, grids=None), "gsplat_bilagrid_tv", "unknown flag")
    # the defined bit with the same bad arguments gets as far as the argument checks
    refused(lib, bwd(flags=abi.GSPLAT_BILAGRID_ACCUMULATE, image=None), "gsplat_bilagrid_backward", "image is NULL")
    # nothing asked for: nothing to do, nothing launched (and no scratch needed without a loss)
    assert bwd(grad_image=None, grad_grids=None) == abi.GSPLAT_OK
    assert tv(loss_out=None, grad=None, scratch=None) == abi.GSPLAT_OK
    odd = C.c_void_p(p.value + 2)
    refused(lib, fwd(image=odd), "gsplat_bilagrid_forward", "aligned")
    refused(lib, bwd(grad_out=odd), "gsplat_bilagrid_backward", "aligned")
    refused(lib, tv(scratch=C.c_void_p(p.value + 4)), "gsplat_bilagrid_tv", "aligned")
    del buf


def test_tv_scratch_bytes_matches_the_layout_in_the_source():
    """gsplat_bilagrid_tv_scratch_bytes = one double per workgroup -- V 12 planes of ceil(L Y X / 256) -- rounded up to 256 bytes
    (csrc/gsplat_bilagrid.hip); -1 for a size that is none."""
    lib = abi.lib()
    for V, X, Y, L in ((1, 2, 2, 2), (3, 3, 5, 4), (100, 16, 16, 8), (7, 64, 64, 16)):
        blocks = V * 12 * ((L * Y * X + 255) // 256)
        assert lib.gsplat_bilagrid_tv_scratch_bytes(V, X, Y, L) == 256 * ((blocks * 8 + 255) // 256), (V, X, Y, L)
    for V, X, Y, L in ((0, 4, 4, 4), (-1, 4, 4, 4), (1, 1, 4, 4), (1, 4, 65, 4), (1, 4, 4, 17), (1 << 40, 4, 4, 4)):
        assert lib.gsplat_bilagrid_tv_scratch_bytes(V, X, Y, L) == -1


# ---- the host build of the per-pixel functions --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    assert os.path.exists(HOST_LIB), "build the host library first: python __graft_entry__.py"
    lib = C.CDLL(HOST_LIB)
    i32 = C.c_int32
    lib.hbila_forward.argtypes = [i32] * 5 + [_F, _F, _F]
    lib.hbila_backward.argtypes = [i32] * 5 + [_F, _F, _F, _F, _F]
    lib.hbila_forward.restype = lib.hbila_backward.restype = None
    lib.hbila_tv.argtypes = [C.c_int64, i32, i32, i32, C.c_float, _F, _F]
    lib.hbila_tv.restype = C.c_double
    lib.hbila_gather_thread_pixels.argtypes = [i32] * 4
    lib.hbila_gather_thread_pixels.restype = C.c_int64
    return lib


def _fp(a):
    return a.ctypes.data_as(_F)


def _host_run(host, image, grids, g_out):
    image, grids, g_out = (np.ascontiguousarray(a, dtype=np.float32) for a in (image, grids, g_out))
    H, W, _ = image.shape
    _, L, Y, X = grids.shape
    out, g_image, g_grids = np.empty_like(image), np.empty_like(image), np.empty_like(grids)
    host.hbila_forward(H, W, X, Y, L, _fp(image), _fp(grids), _fp(out))
    host.hbila_backward(H, W, X, Y, L, _fp(image), _fp(grids), _fp(g_out), _fp(g_image), _fp(g_grids))
    return out, g_image, g_grids


def test_the_constants_the_gpu_tests_read(host):
    assert (host.hbila_sum_depth_fixed(), host.hbila_wave_pixels(), host.hbila_block_pixels(), host.hbila_level_group()) == (13, 64, 256, 8)
    assert host.hbila_stage_floats() == 8192
    # one cell covers the frame: every vertex walks every pixel -- eight waves share the rows, 64 lanes the columns
    assert host.hbila_gather_thread_pixels(70, 130, 2, 2) == (((70 + 7) // 8) * 130 + 63) // 64
    assert host.hbila_gather_thread_pixels(5, 7, 16, 16) == 1
    # the default grid at 1080p: about 2 W / (X - 1) x 2 H / (Y - 1) pixels a vertex, and the slack of the integer bounds
    n = host.hbila_gather_thread_pixels(1080, 1920, 16, 16)
    assert (144 // 8) * 256 // 64 <= n <= ((144 + 6 + 7) // 8) * (256 + 6) // 64 + 1


@pytest.mark.parametrize("h,w,shape", [(1, 1, (2, 2, 2)), (17, 33, (3, 5, 4)), (17, 33, (16, 16, 8)), (5, 7, (16, 16, 8)), (9, 40, (64, 2, 16))])
def test_host_pixel_functions_match_the_oracle(host, h, w, shape):
    image, grids, g_out = (a[0] for a in bo.random_case(21, 1, h, w, shape))
    out, g_image, g_grids = _host_run(host, image, grids, g_out)
    assert (np.abs(out - bo.forward(image, grids)) <= (PIXEL_DEPTH + COORD_DEPTH) * U * bo.magnitude(image, grids)).all()
    want_image, want_grids = bo.backward(image, grids, g_out)
    m_image, m_grids = bo.backward_magnitude(image, grids, g_out)
    assert (np.abs(g_image - want_image) <= (IMAGE_GRAD_DEPTH + COORD_DEPTH) * U * m_image).all()
    # (the host adds a vertex's pixels one after the other: a chain as long as its support, h w roundings at the most)
    assert (np.abs(g_grids - want_grids) <= (h * w + TERM_DEPTH + COORD_DEPTH) * U * m_grids).all()
    assert (g_grids[m_grids == 0] == 0).all()                       # a vertex no pixel reaches: exactly zero


def test_host_grid_gradient_is_exact_on_dyadic_inputs(host):
    """Pixel centres on vertices or mid-cell (W = 2 (X - 1), H = 2 (Y - 1) ... in powers of two), colours whose luminance is a dyadic
    level fraction (grey c in eighths: lum = c up to the rounding of the coefficients -- so the colours are 0 and 1 only, where it is
    exact), dyadic g_o: every weight and product is exact and so is every sum."""
    X, Y, L = 5, 3, 2
    H, W = 4 * (Y - 1), 8 * (X - 1)
    rng = np.random.default_rng(22)
    image = np.repeat(rng.integers(0, 2, (H, W, 1)), 3, axis=2).astype(np.float32)
    g_out = rng.integers(-64, 65, (H, W, 3)).astype(np.float32) / 64
    grids = bo.identity(1, (X, Y, L))[0] + rng.integers(-4, 5, (12, L, Y, X)) / 8
    _, _, g_grids = _host_run(host, image, grids, g_out)
    assert np.array_equal(g_grids.astype(np.float64), bo.backward(image, grids, g_out)[1])


def test_host_identity_is_bit_exact_on_random_finite_floats(host):
    rng = np.random.default_rng(23)
    bits = rng.integers(0, 2 ** 32, 3 * 4096, dtype=np.uint64).astype(np.uint32)
    vals = bits.view(np.float32)
    vals = vals[np.isfinite(vals) & (bits[:vals.size] != 0x80000000)]          # (-0 comes back as +0: the same number, other bits)
    vals = vals[:vals.size // (3 * 64) * (3 * 64)].reshape(-1, 64, 3)
    assert vals.shape[0] * 64 > 3000 and np.abs(vals).max() > 1e30 and (np.abs(vals)[vals != 0].min() < 1e-30)
    other = np.ascontiguousarray(vals[::-1, ::-1])
    for shape in ((2, 2, 2), (16, 16, 8)):
        out, g_image, _ = _host_run(host, vals, bo.identity(1, shape)[0], other)
        assert np.array_equal(out.view(np.uint32), vals.view(np.uint32))
        assert np.array_equal(g_image.view(np.uint32), other.view(np.uint32))


def test_host_tv_matches_the_oracle(host):
    table = (bo.identity(3, (3, 5, 4)) + np.random.default_rng(24).normal(0, 0.2, (3, 12, 4, 5, 3))).astype(np.float32)
    grad = np.empty_like(table)
    loss = host.hbila_tv(3, 3, 5, 4, 10.0, _fp(table), _fp(grad))
    want, want_grad = bo.tv(table)
    m, m_grad = bo.tv_magnitude(table)
    assert abs(loss - 10 * want) <= 4 * U * 10 * m                 # (differences rounded to fp32, squares and sum in double)
    assert (np.abs(grad - 10 * want_grad) <= 7 * U * 10 * m_grad).all()      # (per axis: the factor, two differences, their difference, the fma = 5; two more additions along the chain of three)
    eye = bo.identity(2, (16, 16, 8)).astype(np.float32)
    grad = np.ones_like(eye)
    assert host.hbila_tv(2, 16, 16, 8, 10.0, _fp(eye), _fp(grad)) == 0.0 and not grad.any()


# ---- TrainConfig / Trainer ---------------------------------------------------------------------------------------------------------
VIEWS = [dict(c2w=torch.eye(4), H=8, W=8, fx=10.0, fy=10.0, cx=4.0, cy=4.0, image=torch.zeros(8, 8, 3), idx=k) for k in range(3)]


def test_the_mode_is_off_by_default_and_a_trainer_with_it_has_a_table(gs):
    training = importlib.import_module(PKG + ".training")
    c = training.TrainConfig()
    assert (c.bilagrid, tuple(c.bilagrid_shape), c.bilagrid_tv) == (False, (16, 16, 8), 10.0)
    assert (c.bilagrid_lr_init, c.bilagrid_lr_final, c.bilagrid_lr_delay_mult, c.bilagrid_lr_max_steps) == (0.002, 0.00002, 0.0, 30000)
    assert training.Trainer(zero_model()).bilagrid is None
    assert training.Trainer(zero_model(), training.TrainConfig(), None, cameras=VIEWS, bilagrid_views=7).bilagrid is None
    tr = training.Trainer(zero_model(), training.TrainConfig(bilagrid=True), cameras=VIEWS)              # (the constructor launches nothing)
    assert isinstance(tr.bilagrid, gs.bilagrid.BilateralGridTable) and tuple(tr.bilagrid.params.shape) == (3, 12, 8, 16, 16)
    assert tr.exposure is None
    assert torch.equal(tr.bilagrid.params, torch.tensor(bo.identity(3, (16, 16, 8)), dtype=torch.float32)) and not tr.bilagrid.grad.any()
    assert tr.bilagrid.optimizer.eps == 1e-15 and tr.bilagrid.optimizer is not tr.optimizer
    tr = training.Trainer(zero_model(), training.TrainConfig(bilagrid=True, bilagrid_shape=(3, 5, 4)), cameras=VIEWS, bilagrid_views=5)
    assert tuple(tr.bilagrid.params.shape) == (5, 12, 4, 5, 3) and tr.bilagrid.shape == (3, 5, 4)
    sd = tr.bilagrid.state_dict()
    assert set(sd) == {"params", "exp_avg", "exp_avg_sq", "step"} and sd["step"] == 0
    sd["params"][2, 7, 1, 3, 2] = 0.25
    sd["step"] = 4
    tr.bilagrid.load_state_dict(sd)
    assert tr.bilagrid.params[2, 7, 1, 3, 2] == 0.25 and tr.bilagrid.state_dict()["step"] == 4
    with pytest.raises(ValueError, match="holds a table"):
        tr.bilagrid.load_state_dict(dict(sd, params=torch.zeros(5, 12, 8, 16, 16)))


@pytest.mark.parametrize("value", [1, 0, "yes", None, 1.0])
def test_trainer_refuses_a_bilagrid_that_is_not_a_bool(value):
    training = importlib.import_module(PKG + ".training")
    with pytest.raises(ValueError, match="bilagrid must be a bool"):
        training.TrainConfig(bilagrid=value)
    cfg = training.TrainConfig()
    cfg.bilagrid = value                                                 # (the fields of a config can be set after it is made)
    with pytest.raises(ValueError, match="bilagrid must be a bool"):
        training.Trainer(zero_model(), cfg, cameras=VIEWS)


@pytest.mark.parametrize("shape", [(16, 16), (1, 16, 8), (16, 65, 8), (16, 16, 17), (16, 16, 1), (16.0, 16, 8), (True, 16, 8), "16x16x8", None, 8])
def test_a_bad_shape_is_refused(gs, shape):
    training = importlib.import_module(PKG + ".training")
    with pytest.raises(ValueError, match="shape"):
        training.TrainConfig(bilagrid_shape=shape)                       # (whether the mode is on or not)
    with pytest.raises(ValueError, match="shape"):
        gs.bilagrid.BilateralGridTable(2, "cpu", shape=shape)


def test_trainer_refuses_the_mode_without_a_number_of_images_or_beside_exposure():
    training = importlib.import_module(PKG + ".training")
    with pytest.raises(ValueError, match="bilagrid_views"):
        training.Trainer(zero_model(), training.TrainConfig(bilagrid=True))
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_views"):
            training.Trainer(zero_model(), training.TrainConfig(bilagrid=True), bilagrid_views=bad)
    with pytest.raises(ValueError, match="not available with exposure=True"):
        training.TrainConfig(bilagrid=True, exposure=True)
    for name, bad in (("bilagrid_tv", -1.0), ("bilagrid_tv", float("nan")), ("bilagrid_lr_init", True), ("bilagrid_lr_max_steps", 0)):
        with pytest.raises(ValueError, match=name):
            training.Trainer(zero_model(), training.TrainConfig(bilagrid=True, **{name: bad}), cameras=VIEWS)
    # the checks keep their order: the exposure section's own messages still come first
    with pytest.raises(ValueError, match="exposure must be a bool"):
        training.TrainConfig(exposure=1, bilagrid=1)
    with pytest.raises(ValueError, match="exposure=True needs the number"):
        training.Trainer(zero_model(), training.TrainConfig(exposure=True, bilagrid_tv=-1.0))


@pytest.mark.parametrize("idx", ["missing", None, -1, 3, 1.0, True, "0"])
def test_step_refuses_a_view_without_a_valid_idx_before_anything_is_queued(idx):
    training = importlib.import_module(PKG + ".training")
    tr = training.Trainer(zero_model(), training.TrainConfig(bilagrid=True), cameras=VIEWS)
    view = dict(VIEWS[0])
    if idx == "missing":
        del view["idx"]
    else:
        view["idx"] = idx
    with pytest.raises(ValueError, match="idx"):                         # (on a CPU model: anything queued would have raised otherwise)
        tr.step(1, [VIEWS[1], view])


def test_ops_have_no_cpu_fallback(gs):
    eye = torch.tensor(bo.identity(1, (3, 5, 4))[0], dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.bilagrid.slice(torch.zeros(4, 4, 3), eye)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.bilagrid.BilateralGridTable(2, "cpu", shape=(3, 5, 4)).apply_view(torch.zeros(4, 4, 3), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.bilagrid.tv_loss(eye[None])
    with pytest.raises(ValueError, match="grids must be"):
        gs.bilagrid.slice(torch.zeros(4, 4, 3), torch.eye(3, 4))
    with pytest.raises(ValueError, match="grids must be"):
        gs.bilagrid.slice(torch.zeros(2, 4, 4, 3), eye[None])
    with pytest.raises(ValueError, match="image must be"):
        gs.bilagrid.slice(torch.zeros(4, 4), eye)
    with pytest.raises(ValueError, match="shape"):
        gs.bilagrid.slice(torch.zeros(4, 4, 3), torch.zeros(12, 1, 5, 3))
    with pytest.raises(ValueError, match="grids must be"):
        gs.bilagrid.tv_loss(eye)


# ---- the data-parallel helper ----------------------------------------------------------------------------------------------------
def _rank_rows(rank, n_views=5):
    """The gradient a rank's views leave: rank 0 used rows 0 and 3, rank 1 rows 1 and 3 (row 3 is shared), the rest are zero."""
    g = torch.Generator().manual_seed(80 + rank)
    grad = torch.zeros(n_views, 12, 4, 5, 3)
    for row in ((0, 3) if rank == 0 else (1, 3)):
        grad[row] = torch.randn(12, 4, 5, 3, generator=g)
    return grad


def _worker(rank, world):
    dp = importlib.import_module(PKG + ".dp")
    grad = _rank_rows(rank)
    assert dp.allreduce_table_grad(grad) is grad
    return grad.numpy().copy()


def test_allreduce_table_grad_over_gloo_gives_the_bits_of_one_process():
    dp = importlib.import_module(PKG + ".dp")
    alone = _rank_rows(0)
    assert dp.allreduce_table_grad(alone) is alone and torch.equal(alone, _rank_rows(0))      # a single process: nothing happens
    got = run_ranks(_worker, 2, answer_s=120, join_s=60)
    a, b = _rank_rows(0), _rank_rows(1)
    want = a.clone()                     # one process given both ranks' views: rank 0's rows, then rank 1's added in view order
    want += b
    assert torch.equal(want[0], a[0]) and torch.equal(want[1], b[1]) and not want[2].any() and not want[4].any()
    for rank, grad in enumerate(got):
        assert np.array_equal(grad.view(np.uint32), want.numpy().view(np.uint32)), rank
