"""What the GPU tests of the per-view colour tables share (tests/test_gpu_exposure.py, tests/test_gpu_bilagrid.py,
tests/test_gpu_view_tables.py): the plumbing of a direct call into the library, bit comparison, and the small scene and trainers of
the trainer-level tests."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

from oracle import scenes
from tests.ranks import run_ranks
from tests.util import bits

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAMES = ("pos", "opacity_raw", "f_dc", "f_rest", "scale_raw", "q_raw")
N_IMAGES = 5


def _header_constant(header, name):
    txt = open(os.path.join(ROOT, PKG, "csrc", header)).read()
    value = re.search(rf"constexpr int {name} = (\w+);", txt).group(1)
    return int(value) if value.isdigit() else _header_constant(header, value)          # (a constant defined as another one)


# ---- the entries, called directly ------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _same(a, b):
    return torch.equal(bits(a), bits(b))


def _dev(*arrays):
    return [torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV) for a in arrays]


# ---- the trainer mode ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    """oracle.scenes.case_g1 seen by three cameras; the views name images 0, 2 and 4 of a training set of five."""
    s = scenes.case_g1()
    rng = np.random.default_rng(5)
    cams = [s["c2w"], scenes._camera(rng), scenes._camera(rng)]
    views = [dict(image=rng.uniform(0, 1, (s["H"], s["W"], 3)).astype(np.float32), c2w=c, H=s["H"], W=s["W"], fx=s["fx"], fy=s["fy"],
                  cx=s["cx"], cy=s["cy"], idx=2 * k) for k, c in enumerate(cams)]
    return s, views


def _warm(gs, s, views):
    """A pair capacity for the views' size, so that no frame of a trainer waits for its counters (every trainer takes the same path)."""
    p = {k: torch.tensor(s[k], device=DEV) for k in NAMES}
    with torch.no_grad():
        for v in views:
            gs.render_gaussians(*[p[k] for k in ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")], torch.tensor(v["c2w"], device=DEV),
                                v["H"], v["W"], v["fx"], v["fy"], v["cx"], v["cy"])


def _trainer(s, cameras=None, **cfg):
    """A trainer on the scene's model; with exposure=True or bilagrid=True its table has N_IMAGES rows."""
    model_mod = importlib.import_module(PKG + ".model")
    training = importlib.import_module(PKG + ".training")
    model = model_mod.GaussianModel({k: torch.tensor(s[k]) for k in NAMES}, device=DEV)
    cfg = dict(dict(densify_until_iter=0, opacity_reset_interval=10 ** 9), **cfg)
    return training.Trainer(model, training.TrainConfig(**cfg), cameras=cameras, exposure_views=N_IMAGES if cfg.get("exposure") else None,
                            bilagrid_views=N_IMAGES if cfg.get("bilagrid") else None)


def _model_bits(tr):
    return {k: getattr(tr.model, k).detach().clone() for k in NAMES}


def _table_bits(tr):
    table = tr.exposure if tr.exposure is not None else tr.bilagrid
    st = table.optimizer._state(table.params)
    return dict(params=table.params.clone(), grad=table.grad.clone(), exp_avg=st["exp_avg"].clone(), exp_avg_sq=st["exp_avg_sq"].clone())


def _assert_same_dict(a, b, what):
    for k in a:
        assert _same(a[k], b[k]), (what, k)


@pytest.fixture()
def deterministic(gs):
    old = gs.set_deterministic(True)
    yield gs
    gs.set_deterministic(old)


ROUTES = {
    "default": dict(),
    "no_fold_no_kernel_sum": dict(fold_rest_step=False, sum_views_in_kernel=False),
    "sparse_adam": dict(sparse_adam=True),
    "filter3d": dict(filter3d=0.2, lowpass=0.3, antialias=True),
    "aux": dict(background=(0.2, 0.4, 0.6), lambda_alpha=0.1),
    "screen": dict(densify_rule="screen", densify_absgrad=True, densify_until_iter=100, densification_interval=2),
    "reference_densify": dict(densify_until_iter=100, densification_interval=2, max_grad=1e-4),
    "mcmc": dict(densify_rule="mcmc", densify_until_iter=100, densification_interval=2, mcmc_start_iter=0, cap_max=700),
}


# ---- data parallel -----------------------------------------------------------------------------------------------------------------
def _steps(tr, iterations, views, **kw):
    """The iterations in a row; the 'tv' of each as a float, where the mode has one."""
    tv = []
    for it in iterations:
        out = tr.step(it, views, **kw)
        if "tv" in out:
            tv.append(float(out["tv"]))
    return tv


def _dp_worker(rank, world, mode, iterations):
    gs = importlib.import_module(PKG)
    gs.set_deterministic(True)
    s, views = _scene()
    _warm(gs, s, views[:2])
    tr = _trainer(s, sparse_adam=True, **{mode: True})
    tv = _steps(tr, iterations, [views[rank]], global_views=world)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in _table_bits(tr).items()}, {k: v.cpu().numpy() for k, v in _model_bits(tr).items()}, tv


def _two_ranks_against_one_process(gs, mode, iterations):
    """Two ranks (gloo, both on cuda:0) with one view each against one process given both views, `iterations` with `mode` on and
    sparse_adam: asserts that table, model and the per-iteration 'tv' of either rank are those of the one process, bit for bit, and
    returns the one process's (table bits, tv list) for the mode's own assertions."""
    got = run_ranks(_dp_worker, 2, mode, iterations)
    s, views = _scene()
    _warm(gs, s, views[:2])
    tr = _trainer(s, sparse_adam=True, **{mode: True})
    tv = _steps(tr, iterations, list(views[:2]))
    torch.cuda.synchronize()
    table, model = _table_bits(tr), _model_bits(tr)

    def i32(a):
        return np.ascontiguousarray(a).view(np.int32)
    for rank in (0, 1):
        assert got[rank][2] == tv, (rank, "the TV term")
        for k, v in table.items():
            assert np.array_equal(i32(got[rank][0][k]), i32(v.cpu().numpy())), (rank, "table", k)
        for k, v in model.items():
            assert np.array_equal(i32(got[rank][1][k]), i32(v.cpu().numpy())), (rank, "model", k)
    return table, tv
