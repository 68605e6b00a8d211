"""GPU tests of TrainConfig(pose_opt=True): Trainer.step against the oracle loop (torch_port.render_fused at poses
composed with a float64 table, torch_port.compute_loss, torch.optim.Adam); a frozen table against the trainer without one; two ranks
against one process, bit for bit; and the recovery of two perturbed cameras against the CPU oracle's recorded trajectories
(tests/golden/pose_recovery.npz, written by tools/pose_recovery_oracle.py)."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import pose_delta_oracle as po
from tests import pose_table_harness as h
from tests import util
from tests.view_table_harness import deterministic  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = h.DEV
NAMES = h.NAMES
RENDER_ORDER = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
POSE_CFG = dict(pose_opt=True, pose_lr_init=1e-3, pose_lr_final=1e-4, pose_reg=1e-3)      # (rates at which three iterations move the rows)


def _mod(name):
    return importlib.import_module(h.PKG + "." + name)


def _cam(v):
    return (v["H"], v["W"], v["fx"], v["fy"], v["cx"], v["cy"])


def _views():
    s, views = h._scene()
    return s, list(views[:2])                          # cameras 0 and 2 of N_CAMERAS


# ---- 4. Trainer.step against the oracle loop -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_loop(dtype):
    """Three iterations of POSE_CFG written with the oracle, in `dtype`: -> (losses, the table's gradient at iteration 1, the model's
    gradients at iteration 1, the table after the three iterations)."""
    optim = _mod("optim")
    s, views = _views()
    P = {k: torch.nn.Parameter(torch.tensor(s[k], dtype=dtype)) for k in NAMES}

    class M:
        pass
    mm = M()
    for k in NAMES:
        setattr(mm, k, P[k])
    opt = torch.optim.Adam(optim.reference_param_groups(mm), lr=0.01, eps=1e-15)
    table = torch.nn.Parameter(torch.zeros(h.N_CAMERAS, 9, dtype=dtype))
    topt = torch.optim.Adam([table], lr=POSE_CFG["pose_lr_init"], eps=1e-8)
    losses, first = [], None
    for it in (1, 2, 3):
        opt.param_groups[0]['lr'] = optim.position_lr(it)
        topt.param_groups[0]['lr'] = optim.position_lr(it, POSE_CFG["pose_lr_init"], POSE_CFG["pose_lr_final"], 0.0, 30000)
        opt.zero_grad()
        topt.zero_grad()
        total = 0
        for v in views:
            c2w = po.torch_compose(torch.tensor(v["c2w"], dtype=dtype), table[v["idx"]])
            img = tp.render_fused(*[P[k] for k in RENDER_ORDER], c2w, *_cam(v))
            total = total + tp.compute_loss(img, torch.tensor(v["image"], dtype=dtype), 0.8, 0.2)[0] / len(views)
        total.backward()
        with torch.no_grad():
            table.grad += POSE_CFG["pose_reg"] * table                    # the decay joins the gradient, as a weight decay inside Adam does
        if first is None:
            first = (table.grad.detach().clone().double().numpy(), {k: P[k].grad.detach().clone().double().numpy() for k in NAMES})
        torch.nn.utils.clip_grad_norm_(P["pos"], max_norm=1.0)
        opt.step()
        topt.step()
        losses.append(float(total.detach()))
    return losses, first[0], first[1], table.detach().clone().double().numpy()


def test_pose_training_iterations_match_the_oracle_loop():
    """The losses within max(2e-5 relative -- the bound of the other oracle-loop tests --, K_CAL x the float32 loop's own error); the
    table's gradient and the model's gradients of iteration 1 within util.check_grad calibrated by the float32 loop."""
    s, views = _views()
    tr = h.trainer(s, **POSE_CFG)
    ref_losses, ref_tg, ref_mg, ref_table = _oracle_loop(torch.float64)
    cal_losses, cal_tg, cal_mg, _ = _oracle_loop(torch.float32)
    for it in (1, 2, 3):
        out = tr.step(it, views)
        got, ref = float(out["loss"]), ref_losses[it - 1]
        allowed = max(2e-5 * abs(ref), util.K_CAL * abs(cal_losses[it - 1] - ref))
        print(f"iteration {it}: loss {got!r} oracle {ref!r} |err| {abs(got - ref):.2e} (allowed {allowed:.2e}) lr_pose {out['lr_pose']:.3e}")
        assert abs(got - ref) <= allowed, (it, got, ref)
        assert set(out) == {"loss", "l1", "ssim", "gaussians", "lr_pos", "densified", "sh_degree", "lr_pose"}
        assert out["lr_pose"] == _mod("optim").position_lr(it, POSE_CFG["pose_lr_init"], POSE_CFG["pose_lr_final"], 0.0, 30000)
        if it == 1:
            torch.cuda.synchronize()
            grad = tr.poses.grad.cpu().numpy()
            used = [v["idx"] for v in views]
            util.check_grad(grad[used], ref_tg[used], "table gradient, iteration 1", cal=cal_tg[used])
            assert not np.delete(grad, used, axis=0).any() and not np.delete(ref_tg, used, axis=0).any()
            for k in NAMES:
                util.check_grad(getattr(tr.model, k).grad.cpu().numpy().reshape(ref_mg[k].shape), ref_mg[k], f"model gradient {k}, iteration 1", cal=cal_mg[k])
    table = tr.poses.params.cpu().numpy()
    print("table rows after three iterations", table[[v["idx"] for v in views]], "oracle", ref_table[[v["idx"] for v in views]])
    assert np.abs(table).max() > 1e-3 and not np.delete(table, [v["idx"] for v in views], axis=0).any()


def test_a_frozen_table_trains_the_model_of_the_trainer_without_one():
    """pose_lr_* = 0 and pose_reg = 0: the table stays exactly zero, and every frame is a pose frame AT the given pose.  The model
    after three iterations against a trainer without pose_opt on the separate-route config (no folded step, no in-kernel sum): not
    bitwise -- the pose instantiation of the projection backward is scheduled differently and the separate calls order the float
    atomics differently -- but within smoke()'s bound between the separate and the composite calls, 1e-5 in relative norm."""
    s, views = _views()
    frozen = h.trainer(s, pose_opt=True, pose_lr_init=0.0, pose_lr_final=0.0, pose_reg=0.0)
    plain = h.trainer(s, fold_rest_step=False, sum_views_in_kernel=False)
    for it in (1, 2, 3):
        a, b = frozen.step(it, views), plain.step(it, views)
        assert a["lr_pose"] == 0.0 and abs(float(a["loss"]) - float(b["loss"])) <= 1e-5 * abs(float(b["loss"]))
    torch.cuda.synchronize()
    assert not frozen.poses.params.any()
    assert frozen.poses.grad[[v["idx"] for v in views]].any()                       # (the gradient was formed; the rate froze the rows)
    for k in NAMES:
        x, y = getattr(frozen.model, k).detach().double(), getattr(plain.model, k).detach().double()
        rel = float((x - y).norm() / (y.norm() + 1e-30))
        print(f"frozen table vs no table, {k}: relative difference {rel:.2e}")
        assert rel < 1e-5, (k, rel)


# ---- 5. two ranks against one process ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [{}, {"exposure": True}], ids=["poses", "poses+exposure"])
def test_two_ranks_give_the_bits_of_one_process(gs, deterministic, extra):
    """gloo, both ranks on cuda:0, one view each, sparse_adam, two iterations: the tables and the model of either rank are those of
    one process given both views, bit for bit -- one all-reduce per table, in the same order on every rank."""
    table = h.two_ranks_against_one_process(gs, extra, (1, 2))
    grad = table["pose", "grad"]
    assert grad[0].any() and grad[1].any() and not grad[2:].any()
    assert table["pose", "params"][:2].any() and not table["pose", "params"][2:].any()
    if extra:
        assert table["exposure", "grad"][:2].any() and not table["exposure", "grad"][2:].any()


# ---- 6. recovery ---------------------------------------------------------------------------------------------------------------------
def _errors(c2w, true):
    c2w, true = np.asarray(c2w, dtype=np.float64), np.asarray(true, dtype=np.float64)
    r = np.einsum("bij,bkj->bik", c2w[:, :3, :3], true[:, :3, :3])
    sin = 0.5 * np.linalg.norm(np.stack([r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]], 1), axis=1)
    return np.arctan2(sin, (np.trace(r, axis1=1, axis2=2) - 1) / 2), np.linalg.norm(c2w[:, :3, 3] - true[:, :3, 3], axis=1)


def test_pose_table_recovers_two_perturbed_cameras(gs, deterministic):
    """The loop of tools/pose_recovery_oracle.py on the GPU: a frozen model, two views given about 0.5 degrees and 0.02 units off,
    targets at the true poses, K pose-only iterations at a fixed table rate (K and the rate were chosen on the CPU oracle and come
    from the file).  The final errors are below the starting ones and within twice the float32 oracle's final errors: fp32 gradient
    noise near the optimum is what separates two fp32 runs.  Recorded on the CPU (K = 300 at 1e-3; views 0 and 1): the float64 oracle
    ends at rotation (4.558e-5, 6.660e-5) rad and translation (2.115e-4, 3.301e-4) from (8.727e-3, 2.0e-2); the float32 oracle at
    (4.566e-5, 6.594e-5) and (2.118e-4, 3.306e-4) -- a float32 / float64 ratio of 1.002, 0.990, 1.001, 1.001, far below two, so the
    margin is two.  (Were that ratio above two, the margin would be twice the ratio: the test computes it from the file.)"""
    g = np.load(os.path.join(util.GOLDEN, "pose_recovery.npz"))
    steps, lr, cam = int(g["steps"]), float(g["lr"]), g["cam"]
    cam = (int(cam[0]), int(cam[1]), *[float(x) for x in cam[2:]])
    p = [torch.tensor(g[k], device=DEV) for k in RENDER_ORDER]
    given = torch.tensor(g["given"], dtype=torch.float32, device=DEV)
    targets = torch.tensor(g["targets"], device=DEV)
    table = gs.poses.PoseTable(2, DEV, lr=lr)
    for it in range(steps):
        table.zero_grad()
        for k in range(2):
            img = gs.render_gaussians(*p, table.apply_view(given[k], k), *cam)
            ((img - targets[k]) ** 2).mean().backward()
        table.step(lr)
    torch.cuda.synchronize()
    rot, tr = _errors(table.c2w(given, [0, 1]).cpu().numpy(), g["true"])
    rot0, tr0 = _errors(g["given"], g["true"])
    for name, got, start, f32, f64 in (("rotation", rot, rot0, g["rot_f32"][-1], g["rot_f64"][-1]), ("translation", tr, tr0, g["trans_f32"][-1], g["trans_f64"][-1])):
        ratio = f32 / f64
        margin = np.where(ratio > 2.0, 2.0 * ratio, 2.0)
        print(f"{name}: start {start} -> {got}; float32 oracle {f32}, float64 oracle {f64}, float32 / float64 {ratio}, margin {margin}")
        assert (got < start).all(), (name, got, start)
        assert (got <= margin * f32).all(), (name, got, f32, margin)


# ---- every route, two streams, the evaluation ------------------------------------------------------------------------------------------
def _route_run(s, views, route, streams):
    from tests.view_table_harness import ROUTES
    tr = h.trainer(s, cameras=views, view_streams=streams, **POSE_CFG, **ROUTES[route])
    losses = [float(tr.step(it, views)["loss"]) for it in (1, 2, 3)]
    torch.cuda.synchronize()
    return tr, losses, h.table_bits(tr), h._model_bits(tr)


@pytest.mark.parametrize("route", ["default", "no_fold_no_kernel_sum", "sparse_adam", "filter3d", "aux", "screen", "reference_densify", "mcmc"])
def test_pose_opt_runs_on_every_route_with_the_same_bits_on_one_stream_and_on_two(gs, deterministic, route):
    """The configs of the colour-table tests (every densify rule, sparse_adam, filter3d, an aux pass) with pose_opt: three views, two of
    them of ONE camera (one row of the table fed from two streams), three iterations.  The losses are finite, the rows of the cameras
    used moved and no other did, and view_streams = 2 leaves the bits of view_streams = 1.  (A first run leaves the pair capacities of
    every model size the run goes through, so that the two compared runs queue the same frames in the same way.)"""
    s, views = h._scene()
    views = [views[0], views[1], dict(views[2], idx=views[0]["idx"])]
    if route == "aux":                                   # (lambda_alpha > 0: every view carries an opacity target)
        rng = np.random.default_rng(9)
        views = [dict(v, alpha=rng.uniform(0.02, 0.98, (v["H"], v["W"])).astype(np.float32)) for v in views]
    h._warm(gs, s, views)
    _route_run(s, views, route, 2)
    tr, losses, table, model = _route_run(s, views, route, 2)
    _, losses1, table1, model1 = _route_run(s, views, route, 1)
    assert np.isfinite(losses).all() and losses == losses1
    used = sorted({v["idx"] for v in views})
    params = table["pose", "params"].cpu().numpy()
    assert all(params[k].any() for k in used) and not np.delete(params, used, axis=0).any()
    for k in table:
        assert torch.equal(table[k].view(torch.int32), table1[k].view(torch.int32)), (route, k)
    for k in model:
        assert model[k].shape == model1[k].shape and torch.equal(model[k].view(torch.int32), model1[k].view(torch.int32)), (route, k)


def test_evaluate_renders_training_views_at_their_corrected_poses_on_request(gs):
    s, views = h._scene()
    tr = h.trainer(s, **POSE_CFG)
    idx = views[0]["idx"]
    tr.poses.params[idx] = torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.005, -0.003, 0.002, 0.007], device=DEV)
    held = {k: v for k, v in views[1].items() if k != "idx"}                  # a held-out view: no row in the table
    before = h.table_bits(tr)
    given = tr.evaluate([views[0], held])
    refined = tr.evaluate([views[0], held], refined_poses=True)
    corrected = tr.poses.c2w(torch.tensor(views[0]["c2w"], dtype=torch.float32, device=DEV), idx)
    by_hand = tr.evaluate([dict(views[0], c2w=corrected), held])
    assert refined["per_view"] == by_hand["per_view"]
    assert refined["per_view"]["psnr"][0] != given["per_view"]["psnr"][0]      # the training view moved ...
    assert refined["per_view"]["psnr"][1] == given["per_view"]["psnr"][1]      # ... the held-out view is at its given pose
    assert tr.evaluate([views[0], held], refined_poses=False) == given
    after = h.table_bits(tr)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert np.asarray(views[0]["c2w"]).shape == (4, 4)                        # the caller's dicts are left as they are
