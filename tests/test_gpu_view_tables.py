"""The trainer modes of the two per-view colour tables on the MI355X, in deterministic mode (DESIGN.md §24 exposure, §25 bilateral
grids): one set of tests over both modes; a MODES record carries what differs.  The kernels and the autograd ops have their own files
(tests/test_gpu_exposure.py, tests/test_gpu_bilagrid.py), and each keeps the two-rank test of its mode."""
import contextlib
import importlib
import io
import types

import numpy as np
import pytest
import torch

from tests import bilagrid_oracle as bo
from tests.util import forced_pair_capacity
from tests.view_table_harness import (DEV, N_IMAGES, NAMES, PKG, ROUTES, _assert_same_dict, _model_bits, _same, _scene, _table_bits, _trainer,
                                      _warm, deterministic)  # noqa: F401  (deterministic: a fixture)

pytestmark = pytest.mark.gpu


def _exposure_identity_step(tr, out, views):
    """The rows of the rendered views moved by lr sign(grad) up to Adam's eps, every other row is still the identity, bit for bit."""
    optim = importlib.import_module(PKG + ".optim")
    lr = out["lr_exposure"]
    assert lr == optim.position_lr(1, 0.01, 0.001, 0.0, 30000) and 0.0099 < lr < 0.01
    eye = torch.eye(3, 4)
    table, grad = tr.exposure.params.cpu(), tr.exposure.grad.cpu().double()
    used = [v["idx"] for v in views]
    for row in range(N_IMAGES):
        if row not in used:
            assert _same(table[row], eye) and not grad[row].any(), row
            continue
        g = grad[row]
        assert (g != 0).all(), "a frame of random colours against a random target pulls at every parameter"
        moved = (table[row] - eye).double()
        # first Adam step: -lr g / (|g| + eps); fp32: the bias corrections and the update in a few roundings, 1 - lr near 1
        tol = lr * torch.clamp(1e-8 / g.abs(), max=1.0) + 1e-5 * lr + 1.2e-7
        assert ((moved + lr * torch.sign(g)).abs() <= tol).all(), (row, moved, g)


def _bilagrid_identity_step(tr, out, views):
    """The grids of the rendered views moved, every other grid is still the identity, bit for bit."""
    optim = importlib.import_module(PKG + ".optim")
    assert out["lr_bilagrid"] == optim.position_lr(1, 0.002, 0.00002, 0.0, 30000) and float(out["tv"]) == 0.0
    eye = torch.tensor(bo.identity(1, (16, 16, 8))[0], dtype=torch.float32)
    table, grad = tr.bilagrid.params.cpu(), tr.bilagrid.grad.cpu()
    used = [v["idx"] for v in views]
    for row in range(N_IMAGES):
        if row not in used:
            assert _same(table[row], eye) and not grad[row].any(), row
            continue
        touched = grad[row] != 0
        assert touched.any() and torch.isfinite(table[row]).all()
        assert _same(table[row][~touched], eye[~touched]), "a vertex with a zero gradient does not move in the first Adam step"
        assert (table[row][touched] != eye[touched]).any()


# Per mode: `other` (the table that must stay None), `keys` (what the mode adds to step()'s dict), `identity_cfg` (under which the
# identity table leaves the model's step alone: the grid's TV term off), `identity_step` (the mode's own assertions on that step),
# `identity` (one row at the identity, at the default shape), `state_cfg` / `state_shape` (the table of the state_dict test),
# `unused_rows_get_no_gradient` (the grid's TV term reaches every row of the table, the views' own gradient only theirs).
MODES = {
    "exposure": types.SimpleNamespace(
        other="bilagrid", keys={"lr_exposure"}, identity_cfg=dict(), identity_step=_exposure_identity_step, identity=torch.eye(3, 4),
        state_cfg=dict(), state_shape=(N_IMAGES, 3, 4), unused_rows_get_no_gradient=True),
    "bilagrid": types.SimpleNamespace(
        other="exposure", keys={"lr_bilagrid", "tv"}, identity_cfg=dict(bilagrid_tv=0.0), identity_step=_bilagrid_identity_step,
        identity=torch.tensor(bo.identity(1, (16, 16, 8))[0], dtype=torch.float32),
        state_cfg=dict(bilagrid_shape=(3, 5, 4)), state_shape=(N_IMAGES, 12, 4, 5, 3), unused_rows_get_no_gradient=False),
}
mode_param = pytest.mark.parametrize("mode", sorted(MODES))


@mode_param
@pytest.mark.parametrize("n_views", [1, 2])
def test_a_step_from_the_identity_table_leaves_the_model_as_without_the_mode(deterministic, mode, n_views):
    """(1, 2) The identity (the grid: with bilagrid_tv = 0) returns the frame and its gradient bit for bit, so the model's step is the
    step without the mode -- one view through the folded f_rest step, two through the in-kernel view sum; the rows of the rendered
    views moved (the mode's identity_step says how), every other row is still the identity, bit for bit."""
    gs, M = deterministic, MODES[mode]
    s, views = _scene()
    views = list(views[:n_views])
    _warm(gs, s, views)
    res = {}
    for on in (False, True):
        tr = _trainer(s, **{mode: on}, **M.identity_cfg)
        out = tr.step(1, views)
        torch.cuda.synchronize()
        assert all((k in out) == on for k in M.keys) and (getattr(tr, mode) is not None) == on and getattr(tr, M.other) is None
        assert (tr.model.f_rest.grad is None) == (n_views == 1), "one view takes the folded step, two do not"
        res[on] = (_model_bits(tr), float(out["loss"]), set(out), tr, out)
    _assert_same_dict(res[False][0], res[True][0], "model")
    assert res[False][1] == res[True][1] and res[True][2] == res[False][2] | M.keys
    M.identity_step(res[True][3], res[True][4], views)


@mode_param
def test_a_repeated_pass_counts_the_table_gradient_once(deterministic, mode):
    """(3) The pair capacity is too small for iteration 2: one garbage pass, one good one.  The table's gradient is zeroed at the top
    of every attempt, so the table ends with the bits of an undisturbed iteration."""
    gs = deterministic
    ops = importlib.import_module(PKG + ".ops")
    s, views = _scene()
    views = list(views[:2])
    res = []
    for shrink in (False, True):
        _warm(gs, s, views)
        tr = _trainer(s, **{mode: True})
        tr.step(1, views)
        torch.cuda.synchronize()
        # (100: far below the ~1600 pairs of a view)
        with forced_pair_capacity(gs, views[0]["H"], views[0]["W"], len(s["pos"]), 100) if shrink else contextlib.nullcontext():
            before = dict(ops.forward_modes)
            tr.step(2, views)
            torch.cuda.synchronize()
            assert ops.forward_modes["deferred"] == before["deferred"] + (4 if shrink else 2), "the pass was (not) repeated"
        res.append((_table_bits(tr), _model_bits(tr)))
    assert res[0][0]["grad"][0].any() and res[0][0]["grad"][2].any()
    _assert_same_dict(res[0][0], res[1][0], "table")
    _assert_same_dict(res[0][1], res[1][1], "model")


@mode_param
def test_views_on_two_streams_give_the_bits_of_one_stream(deterministic, mode):
    """(4) Four views, the first two of ONE training image (they land on different streams), two iterations: table and model are bit
    for bit those of the one-stream loop -- a shared row is the views' sum in view order whichever streams they ran on."""
    gs, M = deterministic, MODES[mode]
    s, views = _scene()
    views = [views[0], dict(views[1], idx=views[0]["idx"]), views[2], dict(views[1], idx=views[0]["idx"])]
    _warm(gs, s, views)
    res = []
    for streams in (1, 2):
        tr = _trainer(s, view_streams=streams, **{mode: True})
        for it in (1, 2):
            tr.step(it, views)
        torch.cuda.synchronize()
        res.append((_table_bits(tr), _model_bits(tr)))
    assert res[0][0]["grad"][0].any() and res[0][0]["grad"][4].any()
    if M.unused_rows_get_no_gradient:
        assert not res[0][0]["grad"][2].any()
    _assert_same_dict(res[0][0], res[1][0], "table")
    _assert_same_dict(res[0][1], res[1][1], "model")


@mode_param
def test_state_dict_round_trips_and_the_next_step_is_the_uninterrupted_one(deterministic, mode):
    """(6) Two iterations, the table through torch.save / torch.load into a scrambled table, a third iteration: the bits of three
    iterations in a row."""
    gs, M = deterministic, MODES[mode]
    s, views = _scene()
    views = list(views[:2])
    _warm(gs, s, views)
    res = []
    for interrupt in (False, True):
        tr = _trainer(s, **{mode: True}, **M.state_cfg)
        table = getattr(tr, mode)
        for it in (1, 2):
            tr.step(it, views)
        if interrupt:
            buf = io.BytesIO()
            torch.save(table.state_dict(), buf)
            saved = _table_bits(tr)
            table.load_state_dict(dict(params=torch.zeros(M.state_shape), exp_avg=torch.ones(M.state_shape), exp_avg_sq=torch.ones(M.state_shape),
                                       step=0))
            assert not table.params.any()
            buf.seek(0)
            table.load_state_dict(torch.load(buf))
            back = _table_bits(tr)
            assert all(_same(saved[k], back[k]) for k in ("params", "exp_avg", "exp_avg_sq")) and table.state_dict()["step"] == 2
        tr.step(3, views)
        torch.cuda.synchronize()
        res.append((_table_bits(tr), _model_bits(tr)))
    _assert_same_dict(res[0][0], res[1][0], "table")
    _assert_same_dict(res[0][1], res[1][1], "model")


@mode_param
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n_views", [1, 2])
def test_every_route_keeps_working_with_the_mode_on(gs, mode, route, n_views):
    """The op sits outside the render: every route of the gradients and every densify rule trains with it, the table learns, and a
    fresh model optimiser after a densification leaves the table and its moments alone."""
    M = MODES[mode]
    s, views = _scene()
    views = [dict(v, alpha=np.full((v["H"], v["W"]), 0.5, np.float32)) for v in views[:n_views]]
    tr = _trainer(s, cameras=views, **{mode: True}, **ROUTES[route])
    table = getattr(tr, mode)
    table_opt = table.optimizer
    for it in (1, 2, 3):
        out = tr.step(it, views)
        assert np.isfinite(float(out["loss"])) and out["lr_" + mode] > 0
        assert all(np.isfinite(float(out[k])) for k in M.keys)
    if "tv" in M.keys:
        assert float(out["tv"]) > 0, "after two steps the grids of the rendered views are no longer flat"
    torch.cuda.synchronize()
    st = table_opt._state(table.params)
    assert table.optimizer is table_opt and st["step"] == 3
    eye = M.identity.to(DEV)
    for row in range(N_IMAGES):
        used = row in [v["idx"] for v in views]
        assert torch.isfinite(table.params[row]).all()
        assert (not torch.equal(table.params[row], eye)) == used and bool(st["exp_avg_sq"][row].any()) == used, row
    for k in NAMES:
        assert torch.isfinite(getattr(tr.model, k)).all(), k
