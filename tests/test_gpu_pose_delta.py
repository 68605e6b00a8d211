"""GPU tests of the per-view camera-pose corrections below the trainer: the three kernels against the float64 oracle
(tests/pose_delta_oracle.py) with the bound the host build was measured for, their row-index / accumulate / NULL-half contracts bit
for bit; gs.poses through the render against the float64 oracle render with c2w composed from a float64 delta leaf; and a pose frame
inside the factored exchange."""
import importlib

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import pose_delta_oracle as po
from tests import pose_table_harness as h
from tests import util
from tests.test_gpu_pose_grad import _check_pose
from tests.test_pose_delta_cpu import K_BOUND, random_case, ratios
from tests.view_table_harness import _same, deterministic  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = h.DEV
F32 = torch.float32
RENDER_ORDER = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
BG = (1.0, 0.5, 0.25)
DELTA = np.array([0.02, -0.015, 0.01, 0.004, -0.006, 0.005, -0.003, 0.002, 0.007])       # about 0.5 degrees and 0.03 units


# ---- 1. the kernels against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 63, 64, 65])
def test_kernels_match_the_oracle(gs, b):
    """One lane, a wave short of one lane, a full wave, a second wave: within K_BOUND * 2^-24 * magnitude, the bound the host build
    was measured for (tests/test_pose_delta_cpu.py)."""
    c2w, delta, g_out = (a.astype(np.float32) for a in random_case(10 + b, b))
    c, t, g = h._dev(c2w, delta, g_out)
    out = h.call_forward(c, t)
    gc, gd = h.call_backward(c, t, g)
    torch.cuda.synchronize()
    worst = ratios((out.cpu().numpy(), gc.cpu().numpy(), gd.cpu().numpy()), c2w, delta, g_out)
    print(f"B = {b}: largest error in units of 2^-24 magnitude (out, grad_c2w, grad_delta): {worst}")
    assert max(worst) <= K_BOUND, worst
    # the public op gives the entries' bits, in both directions
    cc, tt = c.clone().requires_grad_(True), t.clone().requires_grad_(True)
    got = gs.poses.apply(cc, tt)
    got.backward(g)
    assert _same(got, out) and _same(cc.grad, gc) and _same(tt.grad, gd)
    one = gs.poses.apply(c[0], t[0])
    assert one.shape == (4, 4) and _same(one, out[0])


def test_zero_table_is_exact_and_an_active_clamp_is_finite(gs):
    c2w, delta, g_out = (a.astype(np.float32) for a in random_case(20, 65))
    c, g = h._dev(c2w, g_out)
    zero = torch.zeros(65, 9, device=DEV)
    assert torch.equal(h.call_forward(c, zero), c)
    gc, _ = h.call_backward(c, zero, g)
    assert torch.equal(gc, g)
    delta[:, 3:6] = (-1.0, 0.0, 0.0)
    t = h._dev(delta)[0]
    got = (h.call_forward(c, t).cpu().numpy(),) + tuple(x.cpu().numpy() for x in h.call_backward(c, t, g))
    assert all(np.isfinite(a).all() for a in got)
    worst = ratios(got, c2w, delta, g_out)
    print("active clamp:", worst)
    assert max(worst) <= K_BOUND, worst


def test_accumulate_row_index_dropped_rows_and_null_halves_bit_for_bit(gs):
    abi = importlib.import_module(h.PKG + "._abi")
    c2w, delta, g_out = (a.astype(np.float32) for a in random_case(21, 65))
    c, t, g = h._dev(c2w, delta, g_out)
    gc, gd = h.call_backward(c, t, g)
    gc2, gd2 = h.call_backward(c, t, g)
    assert _same(gc, gc2) and _same(gd, gd2)                                          # two calls, the same bits
    assert _same(h.call_backward(c, t, g, grad_delta=False)[0], gc)                    # either half alone: the other half's bits
    assert _same(h.call_backward(c, t, g, grad_c2w=False)[1], gd)
    # rows: view b -> row perm[b] of a table of 80 rows, view 7 dropped; the rows no view names keep their bits
    rng = np.random.default_rng(22)
    perm = rng.permutation(80)[:65].astype(np.int32)
    perm[7] = -1
    rows = torch.tensor(perm, device=DEV)
    start = torch.tensor(rng.normal(size=(80, 9)).astype(np.float32), device=DEV)
    stored = h.call_backward(c, t, g, grad_c2w=False, rows=rows, dest=start.clone())[1]
    added = h.call_backward(c, t, g, grad_c2w=False, rows=rows, flags=abi.GSPLAT_POSE_DELTA_ACCUMULATE, dest=start.clone())[1]
    named = np.zeros(80, dtype=bool)
    for b, r in enumerate(perm):
        if r >= 0:
            named[r] = True
            assert _same(stored[r], gd[b]) and _same(added[r], start[r] + gd[b]), b
    assert named.sum() == 64
    keep = torch.tensor(~named, device=DEV)
    assert _same(stored[keep], start[keep]) and _same(added[keep], start[keep])
    # the decay: grad += reg * delta, one fma per element
    grad = h.call_decay(t, 0.125, start[:65].clone())
    want = torch.tensor(np.float32(0.125) * delta.astype(np.float64) + start[:65].cpu().numpy().astype(np.float64)).float()
    assert torch.equal(grad.cpu(), want)                                               # (0.125 delta is exact: the fma rounds once)


# ---- 2. through the render -----------------------------------------------------------------------------------------------------------
def _oracle_through_render(d, dtype, kw=None, maps_loss=None):
    """(table gradient row, gradient of the composed c2w, parameter gradients) of L = sum(img * w) with c2w = compose(given, delta),
    delta a leaf of `dtype`."""
    p = {k: torch.tensor(np.asarray(d[k]), dtype=dtype, requires_grad=True) for k in RENDER_ORDER}
    delta = torch.tensor(DELTA, dtype=dtype, requires_grad=True)
    c2w = po.torch_compose(torch.tensor(np.asarray(d["c2w"]), dtype=dtype), delta)
    c2w.retain_grad()
    out = tp.render_fused(*[p[k] for k in RENDER_ORDER], c2w, *util.cam_args(d), **dict(d["kwargs"], **(kw or {})))
    loss = (out * torch.as_tensor(d["wrand"], dtype=dtype)).sum() if maps_loss is None else maps_loss(out, dtype)
    loss.backward()
    return delta.grad.double().numpy(), c2w.grad.double().numpy(), {k: v.grad.double().numpy() for k, v in p.items()}


def test_table_gradient_through_the_render_vs_oracle(gs, deterministic):
    d = util.load("g1_generic")
    cam = util.cam_args(d)
    ref, _, _ = _oracle_through_render(d, torch.float64)
    cal, _, _ = _oracle_through_render(d, torch.float32)
    idx = 3
    table = gs.poses.PoseTable(h.N_CAMERAS, DEV)
    table.params[idx] = torch.tensor(DELTA, dtype=F32, device=DEV)
    p = {k: torch.tensor(np.asarray(d[k]), dtype=F32, device=DEV, requires_grad=True) for k in RENDER_ORDER}
    given = torch.tensor(d["c2w"], dtype=F32, device=DEV)
    w = torch.tensor(d["wrand"], dtype=F32, device=DEV)
    img = gs.render_gaussians(*[p[k] for k in RENDER_ORDER], table.apply_view(given, idx), *cam, **d["kwargs"])
    (img * w).sum().backward()
    torch.cuda.synchronize()
    util.check_grad(table.grad[idx].cpu().numpy(), ref, "table.grad[idx]", cal=cal)
    others = [k for k in range(h.N_CAMERAS) if k != idx]
    assert not table.grad[others].any()                                              # every other row is exactly 0
    # the bits of gsplat_pose_delta_backward applied to the c2w.grad of a stand-alone pose frame at the corrected pose
    corrected = table.c2w(given, idx).clone().requires_grad_(True)
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    img2 = gs.render_gaussians(*[q[k] for k in RENDER_ORDER], corrected, *cam, **d["kwargs"])
    assert torch.equal(img2, img)
    (img2 * w).sum().backward()
    abi = importlib.import_module(h.PKG + "._abi")
    direct = h.call_backward(given[None].contiguous(), table.params[idx:idx + 1].contiguous(), corrected.grad[None].contiguous(), grad_c2w=False,
                             flags=abi.GSPLAT_POSE_DELTA_ACCUMULATE, dest=torch.zeros(1, 9, device=DEV))[1]
    assert _same(table.grad[idx], direct[0])
    for k in RENDER_ORDER:
        assert torch.equal(p[k].grad, q[k].grad), k                                  # the table changes nothing of the model's gradients


# ---- 3. a pose frame inside the factored exchange -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("aux", [False, True])
def test_pose_frame_inside_a_factored_exchange(gs, aux):
    """The frame goes through the separate calls, gsplat_logit_grad -> the exchange, gsplat_project_backward_pose with the SH-less
    destination.  c2w.grad against the float64 oracle with the bounds of the pose frame outside; the parameter gradients after
    finish() against the frame outside within util.check_grad (the exchange re-associates the SH sums).  SUMMED still refuses."""
    dp = importlib.import_module(h.PKG + ".dp")
    d = util.load("g1_generic")
    cam = util.cam_args(d)
    kw = dict(d["kwargs"], **(dict(aux=True, background=BG) if aux else {}))
    rng = np.random.default_rng(3)
    wmaps = [rng.uniform(-1, 1, sh) for sh in ((d["H"], d["W"], 3), (d["H"], d["W"]), (d["H"], d["W"]))]

    def loss(out, dtype=F32, device=DEV):
        if not aux:
            return (out * torch.as_tensor(d["wrand"], dtype=dtype, device=device)).sum()
        return sum((t * torch.as_tensor(x, dtype=dtype, device=device)).sum() for t, x in zip(out, wmaps))

    okw = dict(maps=True, background=BG) if aux else {}
    oracle = {dt: _oracle_through_render(d, dt, okw, (lambda out, dtype: loss(out, dtype, "cpu")) if aux else None)[1] for dt in (torch.float64, torch.float32)}
    corrected = po.forward(np.asarray(d["c2w"], dtype=np.float64), DELTA)

    def frame(route):
        p = {k: torch.tensor(np.asarray(d[k]), dtype=F32, device=DEV, requires_grad=True) for k in h.NAMES}
        c = torch.tensor(corrected, dtype=F32, device=DEV, requires_grad=True)
        with (route(p) if route is not None else torch.enable_grad()) as ex:
            loss(gs.render_gaussians(*[p[k] for k in RENDER_ORDER], c, *cam, **kw)).backward()
        return p, c, ex

    ref_p, ref_c, _ = frame(None)
    p, c, ex = frame(lambda params: dp.FactoredExchange(params, world_views=1))
    assert ex.n_added == 1 and p["f_dc"].grad is None and p["f_rest"].grad is None       # the SH gradients went to the exchange
    for what, got in (("outside", ref_c), ("inside", c)):
        _check_pose(got.grad.double().cpu().numpy(), oracle[torch.float64], f"pose frame {what} the exchange, aux={aux}", cal=oracle[torch.float32])
    ex.finish()
    for k in h.NAMES:
        assert float(ref_p[k].grad.abs().max()) > 0, k
        util.check_grad(p[k].grad.cpu().numpy(), ref_p[k].grad.cpu().numpy(), f"factored exchange, pose frame, aux={aux}: {k}")
    q = {k: torch.tensor(np.asarray(d[k]), dtype=F32, device=DEV, requires_grad=True) for k in h.NAMES}
    with gs.ops.accumulate_grads(q):
        with pytest.raises(RuntimeError, match="gradient_route"):
            gs.render_gaussians(*[q[k] for k in RENDER_ORDER], torch.tensor(corrected, dtype=F32, device=DEV, requires_grad=True), *cam, **kw)
