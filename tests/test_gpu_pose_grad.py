"""GPU tests of the camera-pose gradient: c2w.requires_grad_() gives c2w.grad, as the reference's plain-PyTorch functions do.
The float64 oracle (oracle/torch_port.py, c2w a leaf) is the reference; the bounds are util.check_grad's, calibrated on the
oracle in float32 where the existing parity tests calibrate the same case."""
import numpy as np
import pytest
import torch

from oracle import scenes
from oracle import torch_port as tp
from tests import util
from tests.mode_scenes import check_pose as _check_pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
NAMES = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")


def _oracle_fused(s, c2w, cam, w, dtype, kw=None):
    """(image, c2w gradient, parameter gradients) of the oracle's fused three-call sequence in `dtype`, L = sum(img * w)."""
    p = {k: torch.tensor(np.asarray(s[k]), dtype=dtype, requires_grad=True) for k in NAMES}
    c = torch.tensor(np.asarray(c2w), dtype=dtype, requires_grad=True)
    img = tp.render_fused(*[p[k] for k in NAMES], c, *cam, **(kw or {}))
    (img * torch.as_tensor(np.asarray(w), dtype=dtype)).sum().backward()
    return img.detach().double().numpy(), c.grad.double().numpy(), {k: v.grad.double().numpy() for k, v in p.items()}


def _render_fused(gs, s, c2w, cam, w, kw=None, c2w_grad=True, param_grad=True, c2w_dtype=F32):
    p = {k: torch.tensor(np.asarray(s[k]), dtype=F32, device=DEV, requires_grad=param_grad) for k in NAMES}
    c = torch.tensor(np.asarray(c2w), dtype=c2w_dtype, device=DEV, requires_grad=c2w_grad)
    img = gs.render_gaussians(*[p[k] for k in NAMES], c, *cam, **(kw or {}))
    (img * torch.as_tensor(np.asarray(w), dtype=F32, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return img, c, p


def _translation_identity(c, pos_grad):
    g = c.grad.double().cpu()
    s = -pos_grad.double().sum(0).cpu()
    assert float((g[:3, 3] - s).abs().max()) <= 1e-5 * float(pos_grad.double().abs().sum()), (g[:3, 3], s)
    assert bool((c.grad[3] == 0).all())


@pytest.mark.parametrize("name", util.RENDER_CASES)
def test_pose_gradient_of_render_gaussians_vs_oracle(gs, name):
    d = util.load(name)
    cam = util.cam_args(d)
    _, ref, _ = _oracle_fused(d, d["c2w"], cam, d["wrand"], torch.float64, d["kwargs"])
    _, cal, _ = _oracle_fused(d, d["c2w"], cam, d["wrand"], torch.float32, d["kwargs"])
    img, c, p = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"])
    assert c.grad is not None and c.grad.dtype == F32 and c.grad.shape == (4, 4)
    _check_pose(c.grad.double().cpu().numpy(), ref, name, cal=cal)
    _translation_identity(c, p["pos"].grad)


def test_pose_gradient_on_the_config1_scene_at_an_orbit_camera(gs):
    s = {k: np.asarray(v) for k, v in scenes.synthetic_scene(1).items() if k in NAMES}
    N, H, W, fx, _ = scenes.CONFIGS[1]
    cam = (H, W, fx, fx, W / 2, H / 2)
    c2w = scenes.orbit_c2w(1, 24)
    w = np.random.default_rng(3).uniform(0, 1, (H, W, 3)).astype(np.float32)
    _, ref, _ = _oracle_fused(s, c2w, cam, w, torch.float64)
    _, cal, _ = _oracle_fused(s, c2w, cam, w, torch.float32)
    img, c, p = _render_fused(gs, s, c2w, cam, w)
    _check_pose(c.grad.double().cpu().numpy(), ref, "config 1", cal=cal)
    _translation_identity(c, p["pos"].grad)


def test_pose_gradient_of_unfused_render_vs_oracle(gs):
    d = util.load("g11_unfused")
    pos = torch.tensor(d["pos"], device=DEV, requires_grad=True)
    opa = torch.tensor(d["opacity_raw"], device=DEV, requires_grad=True)
    col = torch.tensor(d["color_in"], device=DEV, requires_grad=True)
    sig = torch.tensor(d["sigma_in"], device=DEV, requires_grad=True)
    c = torch.tensor(d["c2w"], device=DEV, requires_grad=True)
    img = gs.render(pos, col, opa, sig, c, *util.cam_args(d))
    (img * torch.tensor(d["wrand"], device=DEV)).sum().backward()
    q = [torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("pos", "color_in", "opacity_raw", "sigma_in")]
    cr = torch.tensor(d["c2w"], dtype=torch.float64, requires_grad=True)
    ref = tp.render(q[0], q[1], q[2], q[3], cr, *util.cam_args(d))
    (ref * torch.tensor(d["wrand"], dtype=torch.float64)).sum().backward()
    _check_pose(c.grad.double().cpu().numpy(), cr.grad.numpy(), "g11_unfused")
    _translation_identity(c, pos.grad)
    util.check_grad(pos.grad.cpu().numpy(), d["grad_pos"], "pos")            # the rows are still the ordinary ones


def test_three_call_sequence_gives_the_fused_pose_gradient(gs):
    d = util.load("g1_generic")
    cam = util.cam_args(d)
    old = gs.set_deterministic(True)
    try:
        _, c_fused, _ = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"])
        p = util.tensors(d, F32, device=DEV, grad=True)
        c = torch.tensor(d["c2w"], device=DEV, requires_grad=True)
        sigma = gs.build_sigma_from_params(p["scale_raw"], p["q_raw"])
        color = gs.evaluate_sh(p["f_dc"], p["f_rest"], p["pos"], c)
        img = gs.render(p["pos"], color, p["opacity_raw"], sigma, c, *cam, **d["kwargs"])
        (img * torch.tensor(d["wrand"], device=DEV)).sum().backward()
    finally:
        gs.set_deterministic(old)
    a, b = c.grad.double(), c_fused.grad.double()
    assert float((a - b).norm() / b.norm()) <= 1e-5, (a, b)
    assert bool((c.grad[3] == 0).all())


def test_evaluate_sh_pose_gradient_is_the_translation_column(gs):
    d = util.load("g2_ragged")
    p = util.tensors(d, F32, device=DEV, grad=True)
    c = torch.tensor(d["c2w"], device=DEV, requires_grad=True)
    w = torch.rand(len(d["pos"]), 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    (gs.evaluate_sh(p["f_dc"], p["f_rest"], p["pos"], c) * w).sum().backward()
    pr = torch.tensor(d["pos"], dtype=torch.float64, requires_grad=True)
    cr = torch.tensor(d["c2w"], dtype=torch.float64, requires_grad=True)
    (tp.sh_colour(torch.tensor(d["f_dc"], dtype=torch.float64), torch.tensor(d["f_rest"], dtype=torch.float64), pr, cr) *
     w.double().cpu()).sum().backward()
    util.check_grad(c.grad.cpu().numpy(), cr.grad.numpy(), "evaluate_sh c2w")
    assert bool((c.grad[:, :3] == 0).all()) and bool((c.grad[3] == 0).all())


def test_deferred_frames_give_the_waited_pose_gradient(gs):
    d = util.load("g3_occlusion")
    cam = util.cam_args(d)
    _, c_wait, p_wait = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"])          # (also sizes the kept capacity)
    before = dict(gs.ops.forward_modes), dict(gs.ops.composite_calls)
    with gs.deferred_checks() as chk:
        _, c_def, p_def = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"])
    chk.verify()
    assert gs.ops.forward_modes["deferred"] == before[0]["deferred"] + 1          # not waited for ...
    assert gs.ops.composite_calls == before[1]                                   # ... and through the separate calls
    a, b = c_def.grad.double(), c_wait.grad.double()
    assert float((a - b).norm() / b.norm()) <= 1e-5, (a, b)


def test_pose_gradients_are_reproducible_and_leave_the_parameter_gradients_alone(gs):
    d = util.load("g1_generic")
    cam = util.cam_args(d)
    old = gs.set_deterministic(True)
    try:
        _, c1, p1 = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"])
        _, c2, p2 = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"])
        _, c0, p0 = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"], c2w_grad=False)
        _, c3, _ = _render_fused(gs, d, d["c2w"], cam, d["wrand"], d["kwargs"], param_grad=False)
    finally:
        gs.set_deterministic(old)
    assert torch.equal(c1.grad, c2.grad)
    assert c0.grad is None
    for k in NAMES:
        assert torch.equal(p1[k].grad, p0[k].grad), k          # the pose variant forms the same gradient rows, bit for bit
    assert torch.equal(c3.grad, c1.grad)                       # pose only: no gradient rows, the same sum


def test_float64_camera_gets_a_float64_gradient(gs):
    d = util.load("g2_ragged")
    _, c, _ = _render_fused(gs, d, d["c2w"], util.cam_args(d), d["wrand"], d["kwargs"], c2w_dtype=torch.float64)
    assert c.grad.dtype == torch.float64
    _, ref, _ = _oracle_fused(d, d["c2w"], util.cam_args(d), d["wrand"], torch.float64, d["kwargs"])
    _, cal, _ = _oracle_fused(d, d["c2w"], util.cam_args(d), d["wrand"], torch.float32, d["kwargs"])
    _check_pose(c.grad.cpu().numpy(), ref, "float64 c2w", cal=cal)


@pytest.mark.parametrize("name", util.EMPTY_CASES)
def test_empty_scenes_give_a_zero_pose_gradient(gs, name):
    d = util.load(name)
    img, c, p = _render_fused(gs, d, d["c2w"], util.cam_args(d), d["wrand"], d["kwargs"])
    assert float(img.detach().abs().max()) == 0.0
    assert c.grad is not None and c.grad.shape == (4, 4) and float(c.grad.abs().max()) == 0.0


def test_offscreen_pose_frame_still_raises(gs):
    d = util.load("g10_offscreen")
    with pytest.raises(Exception, match=str(d["raises"])):
        _render_fused(gs, d, d["c2w"], util.cam_args(d), d["wrand"], d["kwargs"])


def test_pose_frame_inside_a_gradient_route_raises(gs):
    d = util.load("g1_generic")
    p = util.tensors(d, F32, device=DEV, grad=True)
    c = torch.tensor(d["c2w"], device=DEV, requires_grad=True)
    with gs.ops.accumulate_grads(p):
        with pytest.raises(RuntimeError, match="gradient_route"):
            gs.render_gaussians(*[p[k] for k in NAMES], c, *util.cam_args(d), **d["kwargs"])
        # the same frame without the pose gradient is routed as before
        gs.render_gaussians(*[p[k] for k in NAMES], c.detach(), *util.cam_args(d), **d["kwargs"])


POSE_STEPS, POSE_LR = 150, 2e-3


def _rotation(omega):
    k = torch.zeros(3, 3, dtype=omega.dtype, device=omega.device)
    k[0, 1], k[0, 2], k[1, 2] = -omega[2], omega[1], -omega[0]
    k[1, 0], k[2, 0], k[2, 1] = omega[2], -omega[1], omega[0]
    return torch.linalg.matrix_exp(k)


def test_pose_refinement_recovers_a_perturbed_camera(gs):
    """Render a target at the true pose; start 1 degree and 0.05 units off; Adam on (axis-angle, translation) composed onto the start
    pose, through c2w.grad alone (the scene is frozen)."""
    s = scenes.synthetic_scene(1)
    N, H, W, fx, _ = scenes.CONFIGS[1]
    cam = (H, W, fx, fx, W / 2, H / 2)
    p = {k: torch.as_tensor(s[k]).to(DEV) for k in NAMES}
    true = torch.tensor(scenes.orbit_c2w(1, 24), device=DEV)
    axis = torch.tensor([1.0, 2.0, -1.5])
    d_rot = _rotation((axis / axis.norm() * np.deg2rad(1.0)).to(DEV))
    start = true.clone()
    start[:3, :3] = d_rot @ true[:3, :3]
    start[:3, 3] += torch.tensor([0.03, -0.04, 0.0], device=DEV)            # 0.05 units

    def errors(c2w):
        r = (c2w[:3, :3].double() @ true[:3, :3].double().T).cpu()
        sin = 0.5 * torch.stack([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]]).norm()
        ang = float(torch.atan2(sin, (r.trace() - 1) / 2))
        return ang, float((c2w[:3, 3].double() - true[:3, 3].double()).norm())

    old = gs.set_deterministic(True)
    try:
        with torch.no_grad():
            target = gs.render_gaussians(*[p[k] for k in NAMES], true, *cam)
        xi = torch.zeros(6, device=DEV, requires_grad=True)
        opt = torch.optim.Adam([xi], lr=POSE_LR)
        rot0, tr0 = errors(start)
        assert abs(rot0 - np.deg2rad(1.0)) < 1e-5 and abs(tr0 - 0.05) < 1e-6
        for it in range(POSE_STEPS):
            c2w = torch.eye(4, device=DEV)
            c2w = torch.cat([torch.cat([_rotation(xi[:3]) @ start[:3, :3], (start[:3, 3] + xi[3:]).unsqueeze(1)], 1), c2w[3:]], 0)
            img = gs.render_gaussians(*[p[k] for k in NAMES], c2w, *cam)
            loss = ((img - target) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            assert xi.grad is not None and bool(torch.isfinite(xi.grad).all())
            opt.step()
            if it % 25 == 0 or it == POSE_STEPS - 1:
                print(it, float(loss.detach()), *errors(c2w.detach()))
    finally:
        gs.set_deterministic(old)
    with torch.no_grad():
        final = torch.cat([torch.cat([_rotation(xi[:3]) @ start[:3, :3], (start[:3, 3] + xi[3:]).unsqueeze(1)], 1),
                           torch.eye(4, device=DEV)[3:]], 0)
    rot, tr = errors(final)
    print("rotation error", rot0, "->", rot, "translation error", tr0, "->", tr)
    assert rot <= 0.3 * rot0 and tr <= 0.3 * tr0, (rot, tr)
