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
import numbers

import torch

from . import _abi, optim
from .ops import _f32, _p, _stream_ptr


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
    return shape, b, shape[-3], shape[-2]


class _ApplyFn(torch.autograd.Function):
    """out = E c over gsplat_exposure_forward / gsplat_exposure_backward.  `dest` is None (the gradient of params is returned to
    autograd) or (grad buffer [V, 12 floats], row [1] int32 on the device): the backward then ADDS the view's twelve sums into that
    row of the buffer itself and returns no gradient for params -- no dense [V, 12] tensor per view.  `anchor`: a scalar leaf that
    requires a gradient (it never gets one), so that the backward runs for the table even where the image needs none."""

    @staticmethod
    def forward(ctx, image, params, dest, anchor):
        if not isinstance(image, torch.Tensor) or not isinstance(params, torch.Tensor):
            raise TypeError("image and params must be torch.Tensors")
        shape, b, h, w = _shapes(image, params)
        x, e = _f32(image, shape, "image"), _f32(params, tuple(params.shape), "params")
        if e.device != x.device:
            raise ValueError(f"image is on {x.device}, params on {e.device}")
        dev = x.device
        with torch.cuda.device(dev):
            out = torch.empty(shape, dtype=torch.float32, device=dev)
            _abi.check(_abi.lib().gsplat_exposure_forward(_p(x), _p(e), b, h, w, _p(out), _stream_ptr(dev)), "gsplat_exposure_forward")
        need_image = ctx.needs_input_grad[0]
        need_params = ctx.needs_input_grad[1] if dest is None else True
        ctx.saved = (x, e, b, h, w, dest) if need_image or need_params else None
        ctx.need = (need_image, need_params)
        ctx.dtypes = (image.dtype, params.dtype)
        ctx.params_shape = tuple(params.shape)
        return out if image.dtype == torch.float32 else out.to(image.dtype)

    @staticmethod
    def backward(ctx, g_out):
        need_image, need_params = ctx.need
        if ctx.saved is None:
            return None, None, None, None
        lib = _abi.lib()
        x, e, b, h, w, dest = ctx.saved
        dev = x.device
        g = _f32(g_out, tuple(x.shape), "grad_out")
        with torch.cuda.device(dev):
            g_image = torch.empty_like(x) if need_image else None
            g_params = scratch = rows = None
            flags = 0
            if need_params:
                scratch = torch.empty(lib.gsplat_exposure_scratch_bytes(b, h, w), dtype=torch.uint8, device=dev)
                if dest is None:
                    g_params = target = torch.empty((b, 12), dtype=torch.float32, device=dev)
                else:
                    target, rows = dest
                    flags = _abi.GSPLAT_EXPOSURE_ACCUMULATE
            _abi.check(lib.gsplat_exposure_backward(_p(x), _p(e), _p(g), b, h, w, _p(g_image), _p(target) if need_params else None, _p(rows),
                                                    flags, _p(scratch), _stream_ptr(dev)), "gsplat_exposure_backward")
        if g_image is not None and ctx.dtypes[0] != torch.float32:
            g_image = g_image.to(ctx.dtypes[0])
        if g_params is not None:
            g_params = g_params.view(ctx.params_shape)
            if ctx.dtypes[1] != torch.float32:
                g_params = g_params.to(ctx.dtypes[1])
        return g_image, g_params, None, None


def apply(image, params):
    """out = M c + t per pixel: image [H, W, 3] with params [3, 4] = [M | t], or [B, H, W, 3] with [B, 3, 4] (one transform per
    image).  Nothing is clamped; the identity returns the image bit for bit.  Differentiable with respect to both; the half that is
    not needed is not computed.  fp32 is computed directly, other dtypes are converted.  One launch forward, one or two backward."""
    return _ApplyFn.apply(image, params, None, None)


class ExposureTable:
    """One transform per training image: `params` [V, 3, 4] at the identity, `grad` a buffer of the same shape, and an Adam state of
    its own -- a second optim.GaussianAdam over the one tensor (eps = 1e-8 and a dense step, as in the INRIA trainer), apart from the
    model's optimiser: restarts of that one after a densification touch neither the table nor its moments.

    The step is DENSE: a row no view of the iteration used has a zero gradient, and still moves by the momentum earlier iterations
    left in its moments (with a zero gradient both moments decay, and the row drifts by lr m / (sqrt(v) + eps) until they are gone).

        table.zero_grad()
        out = table.apply_view(rendered, idx); loss(out).backward()          # adds into table.grad[idx]
        table.step(lr)
    """

    def __init__(self, n_views, device, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
        if type(n_views) is not int or n_views < 1:
            raise ValueError(f"n_views must be an integer >= 1, not {n_views!r}")
        device = torch.device(device)
        self.n_views = n_views
        self.params = torch.eye(3, 4, dtype=torch.float32, device=device).repeat(n_views, 1, 1).contiguous()
        self.grad = torch.zeros_like(self.params)
        self.optimizer = optim.GaussianAdam([{'params': [self.params], 'lr': float(lr), 'name': 'exposure'}], betas=betas, eps=eps)
        # row k of the table names itself: the address of element k is the one-entry row_index of view k (nothing is copied per view)
        self._rows = torch.arange(n_views, dtype=torch.int32, device=device)
        self._anchor = torch.zeros((), dtype=torch.float32, device=device, requires_grad=True)

    def check_index(self, idx):
        """idx as an int in [0, V) (bool, float and anything out of range: ValueError)."""
        if isinstance(idx, bool) or not isinstance(idx, numbers.Integral) or not 0 <= idx < self.n_views:
            raise ValueError(f"a view's 'idx' must be an integer in [0, {self.n_views}), not {idx!r}")
        return int(idx)

    def zero_grad(self):
        self.grad.zero_()

    def apply_view(self, image, idx):
        """The transform of view `idx` applied to image [H, W, 3].  Differentiable with respect to the image; the backward ADDS the
        twelve sums of the view into grad[idx] (gsplat_exposure_backward with a row_index and GSPLAT_EXPOSURE_ACCUMULATE): no dense
        [V, 12] tensor is produced or added per view.  Two views with the same idx must run their backward passes in one stream
        order (Trainer.step sees to it)."""
        idx = self.check_index(idx)
        return _ApplyFn.apply(image, self.params[idx], (self.grad, self._rows[idx:idx + 1]), self._anchor)

    @torch.no_grad()
    def step(self, lr=None):
        """One dense Adam step of the whole table on `grad` (one launch; nothing read back)."""
        if lr is not None:
            self.optimizer.param_groups[0]['lr'] = float(lr)
        self.params.grad = self.grad
        self.optimizer.step()

    def state_dict(self):
        st = self.optimizer._state(self.params)
        return {'params': self.params.detach().clone(), 'exp_avg': st['exp_avg'].clone(), 'exp_avg_sq': st['exp_avg_sq'].clone(),
                'step': int(st['step'])}

    @torch.no_grad()
    def load_state_dict(self, state):
        p = torch.as_tensor(state['params'])
        if tuple(p.shape) != tuple(self.params.shape):
            raise ValueError(f"the state holds a table of {tuple(p.shape)}, this one is {tuple(self.params.shape)}")
        st = self.optimizer._state(self.params)
        self.params.copy_(p)
        st['exp_avg'].copy_(torch.as_tensor(state['exp_avg']))
        st['exp_avg_sq'].copy_(torch.as_tensor(state['exp_avg_sq']))
        st['step'] = int(state['step'])
