"""Per-view camera-pose corrections without a GPU: the numpy oracle against torch float64 autograd of the forward
formulas; the three C entries exist with the stated argument counts and the ABI version is still 12; every bad argument comes back
as GSPLAT_ERR_BAD_ARG naming the entry before anything is launched; the host build of the per-view functions against the oracle
(random cases, the zero correction, an active clamp); what TrainConfig / Trainer refuse."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

from tests import pose_delta_oracle as po
from tests.abi_checks import check_entries, exported_functions, header_defines, refused
from tests.util import zero_model

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = importlib.import_module(PKG + "._abi")
ENTRIES = {"gsplat_pose_delta_forward": 5, "gsplat_pose_delta_backward": 9, "gsplat_pose_delta_decay": 5}
HOST_LIB = os.path.join(ROOT, PKG, "csrc", "libgsposedelta_host.so")
_F = C.POINTER(C.c_float)
U = 2.0 ** -24
# The rounding bound of the fp32 arithmetic is K_BOUND * 2^-24 * magnitude (pose_delta_oracle.magnitude / backward_magnitude).  Over the
# 10^5 random cases below the host build (g++ -O2, x86-64) reaches at most MEASURED_K of those units -- 4.64 in the forward, 4.34 in
# grad_c2w, 4.20 in grad_delta --; K_BOUND is twice that.  The GPU tests use the same K_BOUND.
MEASURED_K = 4.65
K_BOUND = 2 * MEASURED_K


def random_case(seed, b, spread=0.3):
    """(c2w [b, 4, 4] random rigid poses with |e| <= 10, delta [b, 9] with |d| <= 1 and |p|, |s| <= spread, g_out [b, 4, 4])."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(b, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(b, 3, 3)

    def ball(radius):
        v = rng.normal(size=(b, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.uniform(0, 1, (b, 1)) ** (1 / 3)
    c2w = np.tile(np.eye(4), (b, 1, 1))
    c2w[:, :3, :3] = R
    c2w[:, :3, 3] = ball(10.0)
    delta = np.concatenate([ball(1.0), ball(spread), ball(spread)], axis=1)
    return c2w, delta, rng.normal(size=(b, 4, 4))


torch_forward = po.torch_compose


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
def test_oracle_matches_torch_float64_autograd(b):
    c2w, delta, g_out = random_case(1, b)
    c = torch.tensor(c2w, requires_grad=True)
    t = torch.tensor(delta, requires_grad=True)
    out = torch_forward(c, t)
    out.backward(torch.tensor(g_out))
    g_c2w, g_delta = po.backward(c2w, delta, g_out)
    m_c2w, m_delta = po.backward_magnitude(c2w, delta, g_out)
    assert (np.abs(po.forward(c2w, delta) - out.detach().numpy()) <= 1e-12 * po.magnitude(c2w, delta)).all()
    assert (np.abs(g_c2w - c.grad.numpy()) <= 1e-12 * m_c2w).all()
    assert (np.abs(g_delta - t.grad.numpy()) <= 1e-12 * m_delta).all()
    if b == 1:                                     # the unbatched form is the batch of one
        assert np.array_equal(po.forward(c2w[0], delta[0]), po.forward(c2w, delta)[0])
        a, p = po.backward(c2w[0], delta[0], g_out[0])
        assert np.array_equal(a, g_c2w[0]) and np.array_equal(p, g_delta[0])


def test_oracle_identity_orthonormality_and_magnitudes():
    c2w, delta, g_out = random_case(2, 4)
    assert np.array_equal(po.forward(c2w, np.zeros((4, 9))), c2w)
    out = po.forward(c2w, delta)
    assert np.allclose(np.einsum("bki,bkj->bij", out[:, :3, :3], out[:, :3, :3]), np.tile(np.eye(3), (4, 1, 1)), atol=1e-14)
    assert np.allclose(np.linalg.det(out[:, :3, :3]), 1.0)
    assert (po.magnitude(c2w, delta) >= np.abs(out) - 1e-15).all()
    g_c2w, g_delta = po.backward(c2w, delta, g_out)
    m_c2w, m_delta = po.backward_magnitude(c2w, delta, g_out)
    assert (m_c2w >= np.abs(g_c2w) - 1e-14).all() and (m_delta >= np.abs(g_delta) - 1e-14).all()


def test_oracle_clamp_matches_torch_float64_autograd():
    """p = (-1, 0, 0): a1 = 0 and the first clamp is active -- the denominator is a constant in the backward, as F.normalize has it."""
    c2w, delta, g_out = random_case(3, 2)
    delta[:, 3:6] = (-1.0, 0.0, 0.0)
    c = torch.tensor(c2w, requires_grad=True)
    t = torch.tensor(delta, requires_grad=True)
    out = torch_forward(c, t)
    out.backward(torch.tensor(g_out))
    g_c2w, g_delta = po.backward(c2w, delta, g_out)
    assert np.isfinite(g_delta).all() and np.abs(g_delta[:, 3:6]).max() > 1e9
    assert np.allclose(po.forward(c2w, delta), out.detach().numpy(), rtol=0, atol=1e-13)
    assert np.allclose(g_c2w, c.grad.numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(g_delta, t.grad.numpy(), rtol=1e-12, atol=1e-13)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_mirror_and_library_agree_and_the_version_stays_12():
    check_entries(ENTRIES, family="pose_delta", stubs_in_namespace=True)
    assert header_defines()["GSPLAT_POSE_DELTA_ACCUMULATE"] == abi.GSPLAT_POSE_DELTA_ACCUMULATE == 1
    # the render's own pose gradient (ABI 10) keeps its two names, and nothing else of this unit is exported
    assert {"gsplat_pose_scratch_bytes", "gsplat_project_backward_pose"} <= exported_functions()


def test_entries_refuse_bad_arguments_on_the_host():
    """A NULL required pointer, batch < 1 or beyond 2^30, an unknown flag (first), a misaligned array: GSPLAT_ERR_BAD_ARG with a message
    naming the entry, with host addresses only -- nothing is launched."""
    lib = abi.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)

    def fwd(c2w=p, delta=p, batch=1, out=p):
        return lib.gsplat_pose_delta_forward(c2w, delta, batch, out, None)

    def bwd(c2w=p, delta=p, grad_out=p, batch=1, grad_c2w=p, grad_delta=p, row_index=None, flags=0):
        return lib.gsplat_pose_delta_backward(c2w, delta, grad_out, batch, grad_c2w, grad_delta, row_index, flags, None)

    def decay(delta=p, n_views=1, reg=1e-6, grad=p):
        return lib.gsplat_pose_delta_decay(delta, n_views, reg, grad, None)

    sizes = (0, -2, (1 << 30) + 1, 1 << 40)
    for arg in ("c2w", "delta", "out"):
        refused(lib, fwd(**{arg: None}), "gsplat_pose_delta_forward", arg + " is NULL")
    for bad in sizes:
        refused(lib, fwd(batch=bad), "gsplat_pose_delta_forward", "batch")
    for arg in ("c2w", "delta", "grad_out"):
        refused(lib, bwd(**{arg: None}), "gsplat_pose_delta_backward", arg + " is NULL")
    for bad in sizes:
        refused(lib, bwd(batch=bad), "gsplat_pose_delta_backward", "batch")
    for flags in (2, 4, 1 << 5, 3, -2, 1 << 30):
        refused(lib, bwd(flags=flags), "gsplat_pose_delta_backward", "unknown flag")
        refused(lib, bwd(flags=flags, c2w=None, batch=0), "gsplat_pose_delta_backward", "unknown flag")      # refused FIRST
    refused(lib, bwd(flags=abi.GSPLAT_POSE_DELTA_ACCUMULATE, c2w=None), "gsplat_pose_delta_backward", "c2w is NULL")
    assert bwd(grad_c2w=None, grad_delta=None) == abi.GSPLAT_OK          # neither half asked for: nothing to do, nothing launched
    for arg in ("delta", "grad"):
        refused(lib, decay(**{arg: None}), "gsplat_pose_delta_decay", arg + " is NULL")
    for bad in sizes:
        refused(lib, decay(n_views=bad), "gsplat_pose_delta_decay", "n_views")
    odd = C.c_void_p(p.value + 2)
    refused(lib, fwd(c2w=odd), "gsplat_pose_delta_forward", "aligned")
    refused(lib, bwd(grad_out=odd), "gsplat_pose_delta_backward", "aligned")
    refused(lib, bwd(row_index=odd), "gsplat_pose_delta_backward", "aligned")
    refused(lib, decay(grad=odd), "gsplat_pose_delta_decay", "aligned")
    del buf


# ---- the host build of the per-view functions ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    assert os.path.exists(HOST_LIB), "build the host library first: python __graft_entry__.py"
    lib = C.CDLL(HOST_LIB)
    lib.hpd_forward.argtypes = [C.c_int64, _F, _F, _F]
    lib.hpd_backward.argtypes = [C.c_int64, _F, _F, _F, _F, _F]
    lib.hpd_forward.restype = lib.hpd_backward.restype = None
    return lib


def _fp(a):
    return a.ctypes.data_as(_F) if a is not None else None


def _host_run(host, c2w, delta, g_out, halves=(True, True)):
    c2w, delta, g_out = (np.ascontiguousarray(a, dtype=np.float32) for a in (c2w, delta, g_out))
    n = c2w.size // 16
    out = np.empty_like(c2w)
    g_c2w = np.empty_like(c2w) if halves[0] else None
    g_delta = np.empty_like(delta) if halves[1] else None
    host.hpd_forward(n, _fp(c2w), _fp(delta), _fp(out))
    host.hpd_backward(n, _fp(c2w), _fp(delta), _fp(g_out), _fp(g_c2w), _fp(g_delta))
    return out, g_c2w, g_delta


def ratios(got, c2w, delta, g_out):
    """The largest |got - oracle| / (2^-24 magnitude) of (out, g_c2w, g_delta), the oracle on the fp32 inputs as given."""
    out, g_c2w, g_delta = got
    want_c2w, want_delta = po.backward(c2w, delta, g_out)
    m_c2w, m_delta = po.backward_magnitude(c2w, delta, g_out)
    tiny = np.finfo(np.float64).tiny
    return tuple(float((np.abs(a - b) / (U * np.maximum(m, tiny))).max())
                 for a, b, m in ((out, po.forward(c2w, delta), po.magnitude(c2w, delta)), (g_c2w, want_c2w, m_c2w), (g_delta, want_delta, m_delta)))


def test_host_functions_match_the_oracle_on_1e5_random_cases(host):
    c2w, delta, g_out = (a.astype(np.float32) for a in random_case(4, 100000))
    a1 = delta[:, 3:6] + np.float32([1, 0, 0])
    assert np.linalg.norm(a1, axis=1).min() > 0.4
    got = _host_run(host, c2w, delta, g_out)
    worst = ratios(got, c2w, delta, g_out)
    print("host build, largest error in units of 2^-24 magnitude (out, grad_c2w, grad_delta):", worst)
    assert max(worst) <= K_BOUND, worst
    # either half alone has the bits of both together
    assert np.array_equal(_host_run(host, c2w, delta, g_out, (True, False))[1].view(np.uint32), got[1].view(np.uint32))
    assert np.array_equal(_host_run(host, c2w, delta, g_out, (False, True))[2].view(np.uint32), got[2].view(np.uint32))


def test_host_zero_correction_returns_the_pose(host):
    c2w, _, g_out = (a.astype(np.float32) for a in random_case(5, 4096))
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2 ** 32, c2w.size, dtype=np.uint64).astype(np.uint32).view(np.float32).reshape(c2w.shape)
    wild = np.where(np.isfinite(bits), bits, np.float32(1.0)).astype(np.float32)          # every finite float, not only rigid poses
    for poses in (c2w, wild):
        out, g_c2w, _ = _host_run(host, poses, np.zeros((poses.shape[0], 9), dtype=np.float32), g_out)
        assert np.array_equal(out, poses)                                                  # (as numbers: a -0 may come back as +0)
        assert np.array_equal(g_c2w, g_out)                                                # D = I, d = 0: the gradient passes through
    assert np.array_equal(po.forward(c2w, np.zeros((4096, 9))), c2w.astype(np.float64))


def test_host_active_clamp_is_finite_and_matches_the_oracle(host):
    c2w, delta, g_out = (a.astype(np.float32) for a in random_case(7, 64))
    delta[:, 3:6] = (-1.0, 0.0, 0.0)
    got = _host_run(host, c2w, delta, g_out)
    assert all(np.isfinite(a).all() for a in got)
    worst = ratios(got, c2w, delta, g_out)
    print("host build, active clamp:", worst)
    assert max(worst) <= K_BOUND, worst


# ---- TrainConfig / Trainer ---------------------------------------------------------------------------------------------------------
VIEWS = [dict(c2w=torch.eye(4), H=8, W=8, fx=10.0, fy=10.0, cx=4.0, cy=4.0, image=torch.zeros(8, 8, 3), idx=k) for k in range(3)]


def test_the_mode_is_off_by_default_and_a_trainer_with_it_has_a_table(gs):
    training = importlib.import_module(PKG + ".training")
    c = training.TrainConfig()
    assert (c.pose_opt, c.pose_lr_init, c.pose_lr_final, c.pose_lr_delay_mult, c.pose_lr_max_steps, c.pose_reg) == (False, 1e-5, 1e-7, 0.0, 30000, 1e-6)
    assert training.Trainer(zero_model()).poses is None
    assert training.Trainer(zero_model(), training.TrainConfig(), None, cameras=VIEWS, pose_views=7).poses is None
    tr = training.Trainer(zero_model(), training.TrainConfig(pose_opt=True), cameras=VIEWS)              # (the constructor launches nothing)
    assert isinstance(tr.poses, gs.poses.PoseTable) and tuple(tr.poses.params.shape) == (3, 9) and tr.poses.name == "pose"
    assert not tr.poses.params.any() and not tr.poses.grad.any() and tr.exposure is None and tr.bilagrid is None
    assert tr.poses.optimizer.eps == 1e-8 and tr.poses.optimizer is not tr.optimizer
    tr = training.Trainer(zero_model(), training.TrainConfig(pose_opt=True), cameras=VIEWS, pose_views=5)
    assert tuple(tr.poses.params.shape) == (5, 9)
    sd = tr.poses.state_dict()
    assert set(sd) == {"params", "exp_avg", "exp_avg_sq", "step"} and sd["step"] == 0
    sd["params"][2, 7] = 0.25
    sd["step"] = 4
    tr.poses.load_state_dict(sd)
    assert tr.poses.params[2, 7] == 0.25 and tr.poses.state_dict()["step"] == 4


@pytest.mark.parametrize("other", ["exposure", "bilagrid"])
def test_pose_opt_is_accepted_together_with_a_colour_table(gs, other):
    training = importlib.import_module(PKG + ".training")
    tr = training.Trainer(zero_model(), training.TrainConfig(pose_opt=True, **{other: True}), cameras=VIEWS, pose_views=4)
    assert tuple(tr.poses.params.shape) == (4, 9) and getattr(tr, other) is not None and getattr(tr, other).n_views == 3
    assert tr._tables == [getattr(tr, other), tr.poses]                  # the fixed order of the all-reduces
    with pytest.raises(ValueError, match="idx"):                         # 'idx' must be valid for EVERY table: 3 is a row of the poses only
        tr.step(1, [dict(VIEWS[0], idx=3)])


@pytest.mark.parametrize("value", [1, 0, "yes", None, 1.0])
def test_trainer_refuses_a_pose_opt_that_is_not_a_bool(value):
    training = importlib.import_module(PKG + ".training")
    with pytest.raises(ValueError, match="pose_opt"):
        training.TrainConfig(pose_opt=value)
    cfg = training.TrainConfig()
    cfg.pose_opt = value                                                 # (the fields of a config can be set after it is made)
    with pytest.raises(ValueError, match="pose_opt"):
        training.Trainer(zero_model(), cfg, cameras=VIEWS)


def test_trainer_refuses_the_mode_without_a_number_of_images_and_bad_numbers():
    training = importlib.import_module(PKG + ".training")
    with pytest.raises(ValueError, match="pose_views"):
        training.Trainer(zero_model(), training.TrainConfig(pose_opt=True))
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_views"):
            training.Trainer(zero_model(), training.TrainConfig(pose_opt=True), pose_views=bad)
    for field, bad in (("pose_reg", -1.0), ("pose_lr_init", float("nan")), ("pose_lr_final", float("inf")), ("pose_lr_delay_mult", True),
                       ("pose_lr_max_steps", 0), ("pose_lr_max_steps", 2.5)):
        with pytest.raises(ValueError, match=field):
            training.Trainer(zero_model(), training.TrainConfig(pose_opt=True, **{field: bad}), cameras=VIEWS)
    tr = training.Trainer(zero_model(), training.TrainConfig(), cameras=VIEWS)
    with pytest.raises(ValueError, match="pose_opt"):
        tr.evaluate(VIEWS, refined_poses=True)
    with pytest.raises(ValueError, match="refined_poses"):
        tr.evaluate(VIEWS, refined_poses=1)


@pytest.mark.parametrize("idx", ["missing", None, -1, 3, 1.0, True, "0"])
def test_step_refuses_a_view_without_a_valid_idx_before_anything_is_queued(idx):
    training = importlib.import_module(PKG + ".training")
    tr = training.Trainer(zero_model(), training.TrainConfig(pose_opt=True), cameras=VIEWS)
    view = dict(VIEWS[0])
    if idx == "missing":
        del view["idx"]
    else:
        view["idx"] = idx
    with pytest.raises(ValueError, match="idx"):                         # (on a CPU model: anything queued would have raised otherwise)
        tr.step(1, [VIEWS[1], view])


def test_ops_have_no_cpu_fallback(gs):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.poses.apply(torch.eye(4), torch.zeros(9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.poses.PoseTable(2, "cpu").apply_view(torch.eye(4), 1)
    with pytest.raises(ValueError, match="delta must be"):
        gs.poses.apply(torch.eye(4), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="delta must be"):
        gs.poses.apply(torch.eye(4).expand(2, 4, 4), torch.zeros(9))
    with pytest.raises(ValueError, match="c2w must be"):
        gs.poses.apply(torch.zeros(4, 3), torch.zeros(9))
