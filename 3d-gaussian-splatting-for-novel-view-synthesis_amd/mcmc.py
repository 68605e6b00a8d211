"""Density control at a fixed budget (not in the reference): the MCMC formulation of Kheradmand et al. 2024.

    add_noise(model_or_tensors, scale, seed, iteration)      pos += Sigma (z scale g) after the optimiser step
    regularise(model_or_tensors, lambda_opacity, lambda_scale, base=None)
                                                             L_o, L_s as device scalars, their gradients ADDED to .grad
    relocate(model_or_tensors, optimizer, min_opacity, seed, iteration)
                                                             dead rows become copies of live ones, in place (one library call)
    refine(model, optimizer, cap_max, min_opacity, growth, seed, iteration)
                                                             growth towards cap_max (GaussianModel.refine_mcmc), then relocate

ctypes calls into csrc/gsplat_mcmc.hip on the current stream, in the style of optim.py; nothing here reads the device.  Random
numbers are a function of (seed, iteration, row) and the sampling weights integers, so data-parallel ranks that hold the same
parameters compute the same bits without a message.  There is no CPU fallback.
"""
import ctypes as C

import torch

from . import _abi
from ._dev import _launch, _p, _stream_ptr

PARAMS = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")
_WIDTH = {"pos": 3, "f_dc": 3, "f_rest": 45, "opacity_raw": 1, "scale_raw": 3, "q_raw": 4}
_scratch = {}          # per device: the zero-initialised scratch of the regulariser and the refinement, grown on demand


def _tensors(model_or_tensors):
    """{name: tensor} of the six parameters: a GaussianModel (or anything with those attributes) or a dict."""
    get = model_or_tensors.__getitem__ if isinstance(model_or_tensors, dict) else (lambda k: getattr(model_or_tensors, k))
    t = {k: get(k) for k in PARAMS}
    n = t["pos"].shape[0]
    for k, v in t.items():
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
            raise RuntimeError(f"mcmc needs contiguous fp32 GPU parameters ({k}; there is no CPU fallback)")
        if v.shape[0] != n or v.numel() != n * _WIDTH[k] or v.device != t["pos"].device:
            raise ValueError(f"{k} has shape {tuple(v.shape)}, expected {n} rows of {_WIDTH[k]} on {t['pos'].device}")
    return t, n


def _check_seed(seed, iteration):
    if type(seed) is not int or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), not {seed!r}")
    if type(iteration) is not int or not 0 <= iteration < 2 ** 32:
        raise ValueError(f"iteration must be an integer in [0, 2^32), not {iteration!r}")


def scratch(n, dev):
    """The device scratch for n rows (gsplat_mcmc_scratch_bytes; zeroed when it is made, as the regulariser's counter needs)."""
    need = _abi.lib().gsplat_mcmc_scratch_bytes(n)
    if need < 0:
        raise ValueError(f"mcmc handles fewer than 2^31 rows, not {n}")
    key = (dev.type, dev.index)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < need:
        buf = _scratch[key] = torch.zeros(need + need // 4, dtype=torch.uint8, device=dev)
    return buf


def layout(n):
    """The byte offsets inside scratch(n) (tests and tools)."""
    lay = _abi.McmcLayout()
    _abi.check(_abi.lib().gsplat_mcmc_scratch_layout(n, C.byref(lay)), "gsplat_mcmc_scratch_layout")
    return lay


@torch.no_grad()
def add_noise(model_or_tensors, scale, seed, iteration):
    """pos_i += Sigma_i (z_i scale g_i) in place: z three normals of (seed, iteration, i), g the opacity gate (0 for an opaque
    Gaussian, whose row is not written).  `scale` = position learning rate x noise_lr.  One launch."""
    _check_seed(seed, iteration)
    t, n = _tensors(model_or_tensors)
    dev = t["pos"].device
    _launch("gsplat_mcmc_noise", dev, n, _p(t["pos"]), _p(t["opacity_raw"]), _p(t["scale_raw"]), _p(t["q_raw"]), float(scale), seed, iteration)


@torch.no_grad()
def regularise(model_or_tensors, lambda_opacity, lambda_scale, base=None, grads=True):
    """values = (L_o, L_s, base + L_o + L_s) as a [3] device tensor, L_o = lambda_opacity mean sigmoid(opacity_raw), L_s =
    lambda_scale mean exp(scale_raw); with `grads` their gradients are added to opacity_raw.grad and scale_raw.grad (which must
    exist).  `base`: a device scalar (a loss) or None.  One launch, the same bits every call."""
    t, n = _tensors(model_or_tensors)
    dev = t["pos"].device
    go = gs = None
    if grads:
        go, gs = t["opacity_raw"].grad, t["scale_raw"].grad
        for k, g in (("opacity_raw", go), ("scale_raw", gs)):
            if g is None or not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
                raise RuntimeError(f"mcmc.regularise adds to {k}.grad: it must be a contiguous fp32 GPU tensor")
    if base is not None and not (base.is_cuda and base.dtype == torch.float32 and base.numel() == 1):
        raise RuntimeError("base must be an fp32 GPU scalar")
    with torch.cuda.device(dev):
        values = torch.zeros(3, dtype=torch.float32, device=dev) if n == 0 else torch.empty(3, dtype=torch.float32, device=dev)
        _abi.check(_abi.lib().gsplat_mcmc_regularise(n, _p(t["opacity_raw"]), _p(t["scale_raw"]), _p(go), _p(gs), float(lambda_opacity),
                                                     float(lambda_scale), _p(base), _p(values), _p(scratch(n, dev)), _stream_ptr(dev)),
                   "gsplat_mcmc_regularise")
    return values


def _moments(optimizer, t):
    mo = _abi.McmcMoments()
    if optimizer is None:
        return None
    for k in PARAMS:
        st = optimizer._state(t[k])
        getattr(mo, k)[0], getattr(mo, k)[1] = st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()
    return mo


@torch.no_grad()
def relocate(model_or_tensors, optimizer, min_opacity, seed, iteration):
    """One library call (six launches, no host read): every row with sigmoid(opacity_raw) <= min_opacity draws a live row in
    proportion to the opacities and becomes a copy of it; source and copies get the opacity and scale that keep the image; the
    Adam moments of `optimizer` (a GaussianAdam over these very tensors, or None) are zeroed on the rows that changed."""
    _check_seed(seed, iteration)
    t, n = _tensors(model_or_tensors)
    dev = t["pos"].device
    mo = _moments(optimizer, t)
    with torch.cuda.device(dev):
        _abi.check(_abi.lib().gsplat_mcmc_refine(*[_p(t[k]) for k in PARAMS], C.byref(mo) if mo is not None else None, n, float(min_opacity),
                                                 seed, iteration, _p(scratch(n, dev)), _stream_ptr(dev)), "gsplat_mcmc_refine")


def refine(model, optimizer, cap_max, min_opacity=0.005, growth=1.05, seed=0, iteration=0):
    """GaussianModel.refine_mcmc: grow towards cap_max with dead rows (the optimiser keeps its state), then relocate."""
    return model.refine_mcmc(optimizer, cap_max=cap_max, min_opacity=min_opacity, growth=growth, seed=seed, iteration=iteration)
