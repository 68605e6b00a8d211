"""What the GPU tests of the pose table share (tests/test_gpu_pose_delta.py, tests/test_gpu_pose_training.py): direct calls into the
three entries, the bits of a trainer's tables, and the two-rank run.  The plumbing is tests/view_table_harness.py's; its _table_bits
and its workers know the two colour tables only, so the ones here are their pose-aware twins."""
import importlib

import numpy as np
import torch

from tests.ranks import run_ranks
from tests.view_table_harness import DEV, NAMES, PKG, _dev, _model_bits, _p, _scene, _stream, _warm  # noqa: F401  (shared with the test files)

N_CAMERAS = 5


def _lib():
    return importlib.import_module(PKG + "._abi").lib()


def _ok(status, what):
    assert status == 0, (what, status, _lib().gsplat_last_error())


def call_forward(c2w, delta):
    out = torch.empty_like(c2w)
    _ok(_lib().gsplat_pose_delta_forward(_p(c2w), _p(delta), c2w.shape[0], _p(out), _stream()), "forward")
    return out


def call_backward(c2w, delta, g_out, grad_c2w=True, grad_delta=True, rows=None, flags=0, dest=None):
    """-> (grad_c2w or None, the destination of grad_delta or None): `dest` is the buffer the nine floats go to (fresh if None)."""
    gc = torch.empty_like(c2w) if grad_c2w else None
    gd = (dest if dest is not None else torch.empty_like(delta)) if grad_delta else None
    _ok(_lib().gsplat_pose_delta_backward(_p(c2w), _p(delta), _p(g_out), c2w.shape[0], _p(gc), _p(gd), _p(rows), flags, _stream()), "backward")
    return gc, gd


def call_decay(delta, reg, grad):
    _ok(_lib().gsplat_pose_delta_decay(_p(delta), delta.shape[0], float(reg), _p(grad), _stream()), "decay")
    return grad


# ---- the trainer mode ------------------------------------------------------------------------------------------------------------
def trainer(s, cameras=None, **cfg):
    """A trainer on the scene's model; every table it has N_CAMERAS rows."""
    model_mod = importlib.import_module(PKG + ".model")
    training = importlib.import_module(PKG + ".training")
    model = model_mod.GaussianModel({k: torch.tensor(s[k]) for k in NAMES}, device=DEV)
    cfg = dict(dict(densify_until_iter=0, opacity_reset_interval=10 ** 9), **cfg)
    return training.Trainer(model, training.TrainConfig(**cfg), cameras=cameras, exposure_views=N_CAMERAS if cfg.get("exposure") else None,
                            bilagrid_views=N_CAMERAS if cfg.get("bilagrid") else None, pose_views=N_CAMERAS if cfg.get("pose_opt") else None)


def table_bits(tr):
    """params, grad and both moments of every table of the trainer, keyed by (table name, what)."""
    out = {}
    for table in tr._tables:
        st = table.optimizer._state(table.params)
        out.update({(table.name, "params"): table.params.clone(), (table.name, "grad"): table.grad.clone(),
                    (table.name, "exp_avg"): st["exp_avg"].clone(), (table.name, "exp_avg_sq"): st["exp_avg_sq"].clone()})
    return out


# ---- data parallel -----------------------------------------------------------------------------------------------------------------
DP_CFG = dict(sparse_adam=True, pose_opt=True, pose_lr_init=1e-3, pose_lr_final=1e-4)       # (a rate at which two iterations move the rows)


def _dp_worker(rank, world, extra, iterations):
    gs = importlib.import_module(PKG)
    gs.set_deterministic(True)
    s, views = dp_views()
    _warm(gs, s, views)
    tr = trainer(s, **DP_CFG, **extra)
    for it in iterations:
        tr.step(it, [views[rank]], global_views=world)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in table_bits(tr).items()}, {k: v.cpu().numpy() for k, v in _model_bits(tr).items()}


def dp_views():
    """The scene of the colour-table tests and its first two views, as cameras 0 and 1 of N_CAMERAS."""
    s, views = _scene()
    return s, [dict(v, idx=k) for k, v in enumerate(views[:2])]


def two_ranks_against_one_process(gs, extra, iterations):
    """Two ranks (gloo, both on cuda:0) with one view each against one process given both views, DP_CFG plus `extra`: asserts that the
    tables and the model of either rank are those of the one process, bit for bit, and returns the one process's table bits."""
    got = run_ranks(_dp_worker, 2, extra, iterations)
    s, views = dp_views()
    _warm(gs, s, views)
    tr = trainer(s, **DP_CFG, **extra)
    for it in iterations:
        tr.step(it, list(views))
    torch.cuda.synchronize()
    table, model = table_bits(tr), _model_bits(tr)

    def i32(a):
        return np.ascontiguousarray(a).view(np.int32)
    for rank in (0, 1):
        for k, v in table.items():
            assert np.array_equal(i32(got[rank][0][k]), i32(v.cpu().numpy())), (rank, "table", k)
        for k, v in model.items():
            assert np.array_equal(i32(got[rank][1][k]), i32(v.cpu().numpy())), (rank, "model", k)
    return table
