"""Per-view exposure compensation (not in the reference): photographs of one scene differ in exposure and white
balance, and a model trained against them without compensation pays for the difference with floaters and view-dependent colour it
should not have.  As in the INRIA trainer (its 2024 update) and gsplat, every training image gets a small learned colour transform
that the rendered frame goes through before the loss:

    E = [M | t], 3 x 4:    out = M c + t   per pixel colour c,  no clamp;   the identity at the start

    apply(image, params)                     the transform, differentiable with respect to both
    ExposureTable(n_views, device)           one E per training image, their gradient buffer and an Adam state of their own
    table.apply_view(image, idx)             the transform of view idx; its backward adds into table.grad[idx]

    out = exposure.apply(rendered, E)                                 # [H, W, 3] with [3, 4], or [B, H, W, 3] with [B, 3, 4]
    loss, _ = gs.compute_loss(out, photograph)

TrainConfig.exposure switches it on in Trainer.step.  Novel views are rendered without it, as the INRIA trainer does.

ctypes calls into csrc/gsplat_exposure.hip on the current stream, in the style of filter3d.py; nothing here reads the device.  The
gradient of the parameters is a full-frame sum formed in a fixed order without float atomics: the same bits on every call, every
stream and every launch, with or without gs.set_deterministic(True).  There is no CPU fallback.
"""
import torch

from . import _abi
from ._viewtable import ViewFn, ViewOp, ViewTable
from ._dev import _p


def _shapes(image, params):
    shape = tuple(image.shape)
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise ValueError(f"image must be [H, W, 3] or [B, H, W, 3], got {shape}")
    b = shape[0] if len(shape) == 4 else 1
    want = (b, 3, 4) if len(shape) == 4 else (3, 4)
    if tuple(params.shape) != want:
        raise ValueError(f"params must be {list(want)} for an image of {list(shape)}, got {list(params.shape)}")
    if min(shape) < 1:
        raise ValueError(f"image has an empty dimension: {shape}")
    return shape, (b, shape[-3], shape[-2])


def _forward(x, e, dims, out, stream):
    _abi.check(_abi.lib().gsplat_exposure_forward(_p(x), _p(e), *dims, _p(out), stream), "gsplat_exposure_forward")


def _backward(x, e, g, dims, g_image, target, rows, flags, stream):
    lib = _abi.lib()
    # the twelve sums are a full-frame reduction: its partial sums live in a scratch buffer, wanted only with the gradient of params
    scratch = torch.empty(lib.gsplat_exposure_scratch_bytes(*dims), dtype=torch.uint8, device=x.device) if target is not None else None
    _abi.check(lib.gsplat_exposure_backward(_p(x), _p(e), _p(g), *dims, _p(g_image), _p(target), _p(rows), flags, _p(scratch), stream),
               "gsplat_exposure_backward")


# out = E c over gsplat_exposure_forward / gsplat_exposure_backward, in the skeleton of _viewtable.ViewFn
_OP = ViewOp("params", _shapes, _forward, _backward, _abi.GSPLAT_EXPOSURE_ACCUMULATE)


def apply(image, params):
    """out = M c + t per pixel: image [H, W, 3] with params [3, 4] = [M | t], or [B, H, W, 3] with [B, 3, 4] (one transform per
    image).  Nothing is clamped; the identity returns the image bit for bit.  Differentiable with respect to both; the half that is
    not needed is not computed.  fp32 is computed directly, other dtypes are converted.  One launch forward, one or two backward."""
    return ViewFn.apply(_OP, image, params, None, None)


class ExposureTable(ViewTable):
    """One transform per training image: `params` [V, 3, 4] at the identity, `grad` a buffer of the same shape, and an Adam state of
    its own -- a second optim.GaussianAdam over the one tensor (eps = 1e-8 and a dense step, as in the INRIA trainer), apart from the
    model's optimiser: restarts of that one after a densification touch neither the table nor its moments.

    The step is DENSE: a row no view of the iteration used has a zero gradient, and still moves by the momentum earlier iterations
    left in its moments (with a zero gradient both moments decay, and the row drifts by lr m / (sqrt(v) + eps) until they are gone).

        table.zero_grad()
        out = table.apply_view(rendered, idx); loss(out).backward()          # adds into table.grad[idx]
        table.step(lr)
    """

    name, op = 'exposure', _OP

    def __init__(self, n_views, device, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(n_views, device, lr, betas, eps)

    def _identity(self, device):
        return torch.eye(3, 4, dtype=torch.float32, device=device)
