"""Optimiser step of the reference's training loop on the MI355X ("next" row 2).

Mirrors the call sites of scripts/train.py: `optim.Adam([...six groups...], lr=lr, eps=1e-15)` (:394-401), the position
learning-rate schedule (:446-457), `clip_grad_norm_(model.pos, max_norm=1.0)` (:536) and `optimizer.step()` (:538).
`GaussianAdam` takes torch-style param groups; `step()` runs ONE fused HIP kernel for all of them (csrc/gsplat_optim.hip); the
clip coefficient is computed and applied on the device, so a training step has no host synchronisation here.
"""
import ctypes as C

import torch

from . import _abi, ops
from ._dev import _p, _stream_ptr
from ._timing import _stage


def position_lr(iteration, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                position_lr_max_steps=30000):
    """Exponential decay with the initial x0.01 delay phase (scripts/train.py:446-457)."""
    if iteration < position_lr_max_steps:
        lr = position_lr_init * (position_lr_final / position_lr_init) ** (iteration / position_lr_max_steps)
    else:
        lr = position_lr_final
    if iteration < position_lr_delay_mult * position_lr_max_steps:
        lr *= 0.01
    return lr


def reference_param_groups(model, position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005,
                           rotation_lr=0.001):
    """The six groups of scripts/train.py:394-401; `model` has pos, opacity_raw, f_dc, f_rest, scale_raw, q_raw."""
    return [{'params': [model.pos], 'lr': position_lr_init, 'name': 'pos'},
            {'params': [model.opacity_raw], 'lr': opacity_lr, 'name': 'opacity'},
            {'params': [model.f_dc], 'lr': feature_lr, 'name': 'f_dc'},
            {'params': [model.f_rest], 'lr': feature_lr / 20.0, 'name': 'f_rest'},
            {'params': [model.scale_raw], 'lr': scaling_lr, 'name': 'scale'},
            {'params': [model.q_raw], 'lr': rotation_lr, 'name': 'rotation'}]


class _RestUpdate:
    """What ops._backward_impl needs to fold the Adam step of one parameter (f_rest) into the backward pass."""
    route_kind = "folded"

    def __init__(self, opt, param, lr):
        self.opt, self.param, self.lr, self.applied = opt, param, lr, False

    def matches(self, f_rest32, src_ptr):
        p = self.param
        return (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and src_ptr == p.data_ptr()
                and f_rest32.data_ptr() == p.data_ptr() and p.data_ptr() % 16 == 0)

    def begin(self):
        """(AdamGroup, beta1, beta2, eps) of the optimiser's next step of the parameter; commit() counts it once the call is queued."""
        st = self.opt._state(self.param)
        group = _abi.AdamGroup(self.param.numel(), _p(self.param).value, None, _p(st['exp_avg']).value, _p(st['exp_avg_sq']).value,
                               float(self.lr), int(st['step']) + 1, None)
        return group, float(self.opt.betas[0]), float(self.opt.betas[1]), float(self.opt.eps)

    def commit(self):
        self.opt._state(self.param)['step'] += 1
        self.applied = True

    def rollback(self):
        """The frame turned out to have outgrown its buffers (or to be off screen): the kernel stepped nothing, so nothing counts."""
        if self.applied:
            self.opt._state(self.param)['step'] -= 1
            self.applied = False


class GaussianAdam:
    """torch.optim.Adam (amsgrad off, no weight decay) restricted to what the reference uses, fused per tensor.

    `clip` = (parameter tensor, max_norm): clip_grad_norm_ on that tensor before the step, fused into its update."""

    def __init__(self, param_groups, lr=0.01, betas=(0.9, 0.999), eps=1e-15):
        self.param_groups = []
        for g in param_groups:
            g = dict(g)
            g.setdefault('lr', lr)
            g['params'] = list(g['params'])
            self.param_groups.append(g)
        self.betas, self.eps = betas, eps
        self.state = {}
        self._clip_buf = None

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g['params']:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def _state(self, p):
        st = self.state.get(p)
        if st is None:
            st = self.state[p] = {'step': 0, 'exp_avg': torch.zeros_like(p, memory_format=torch.contiguous_format),
                                  'exp_avg_sq': torch.zeros_like(p, memory_format=torch.contiguous_format)}
        return st

    @torch.no_grad()
    def grow_rows(self, old_param, new_param):
        """`new_param` is `old_param` with rows appended (density control that keeps the optimiser, model.refine_mcmc): the state moves
        to the new tensor -- both moments padded with zero rows, `step` kept -- and the parameter group holds the new tensor."""
        if new_param.shape[1:] != old_param.shape[1:] or new_param.shape[0] < old_param.shape[0]:
            raise ValueError(f"grow_rows: {tuple(old_param.shape)} cannot grow into {tuple(new_param.shape)}")
        found = False
        for g in self.param_groups:
            for k, p in enumerate(g['params']):
                if p is old_param:
                    g['params'][k], found = new_param, True
        if not found:
            raise ValueError("grow_rows: the old parameter is not one of this optimiser's")
        st = self.state.pop(old_param, None)
        if st is not None:
            extra = new_param.shape[0] - old_param.shape[0]
            for key in ('exp_avg', 'exp_avg_sq'):
                m = st[key]
                st[key] = torch.cat([m, m.new_zeros((extra,) + tuple(m.shape[1:]))], dim=0) if extra else m
            self.state[new_param] = st
        if getattr(self, "_pending_clip", None) is not None and self._pending_clip[0] is old_param:
            self._pending_clip = None

    def fused_rest_update(self, param):
        """For an iteration of ONE view rendered inside ops.deferred_checks(): the backward pass applies this optimiser's step of
        `param` (the model's f_rest: 81 % of all parameters) as the gradient is formed, param.grad stays None and step() skips it.
        A context (ops.gradient_route) that yields the hook: call hook.rollback() when the frame's checks fail afterwards
        (ops.PairCapacityExceeded, off-screen) -- the kernel itself stepped nothing in that case."""
        lr = next(g['lr'] for g in self.param_groups if any(p is param for p in g['params']))
        return ops.gradient_route(_RestUpdate(self, param, lr))

    @torch.no_grad()
    def clip_grad_norm_(self, param, max_norm=1.0):
        """Device-side clip_grad_norm_ for one tensor; returns the [coef, norm] device tensor (no host read)."""
        lib = _abi.lib()
        g = param.grad
        if g is None:
            return None
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
            raise RuntimeError("GaussianAdam needs contiguous fp32 GPU gradients (there is no CPU fallback)")
        dev = g.device
        with torch.cuda.device(dev):
            if self._clip_buf is None or self._clip_buf[0].device != dev:
                self._clip_buf = (torch.empty(2, dtype=torch.float32, device=dev),
                                  torch.empty(lib.gsplat_clip_scratch_bytes(), dtype=torch.uint8, device=dev))
            out, scratch = self._clip_buf
            _abi.check(lib.gsplat_clip_grad_norm(g.numel(), _p(g), float(max_norm), _p(out), _p(scratch), _stream_ptr(dev)),
                       "gsplat_clip_grad_norm")
        self._pending_clip = (param, out)
        return out

    @torch.no_grad()
    def step(self, visible=None):
        """One launch per device for all parameter groups (gsplat_adam_step_multi, eight tensors per launch).

        visible (an ops.VisibleSet or its uint8 [N] tensor): the sparse step -- every stepped tensor has N rows
        (shape[0] == N, else ValueError) and only the rows whose byte is non-zero are stepped (gsplat_adam_step_rows): exactly as
        above, with the tensor's own `step` in the bias corrections; every other row keeps its parameter, gradient and moments bit for
        bit.  `step` counts once per call either way, and clip_grad_norm_ composes unchanged."""
        lib = _abi.lib()
        pending = getattr(self, "_pending_clip", None)
        mask = None
        if visible is not None:
            mask = self._row_mask(visible)
        per_device = {}
        for g in self.param_groups:
            for p in g['params']:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()):
                    raise RuntimeError("GaussianAdam needs contiguous fp32 GPU parameters (there is no CPU fallback)")
                st = self._state(p)
                st['step'] += 1
                scale = pending[1] if pending is not None and pending[0] is p else None
                per_device.setdefault(p.device, []).append(
                    _abi.AdamGroup(p.numel(), _p(p).value, _p(p.grad).value, _p(st['exp_avg']).value, _p(st['exp_avg_sq']).value,
                                   float(g['lr']), int(st['step']), _p(scale).value if scale is not None else None))
        with _stage("adam"):
            for dev, groups in per_device.items():
                with torch.cuda.device(dev):
                    for k in range(0, len(groups), 8):
                        chunk = groups[k:k + 8]
                        arr = (_abi.AdamGroup * len(chunk))(*chunk)
                        if mask is None:
                            _abi.check(lib.gsplat_adam_step_multi(len(chunk), arr, float(self.betas[0]), float(self.betas[1]), float(self.eps),
                                                                  _stream_ptr(dev)), "gsplat_adam_step_multi")
                            continue
                        n = mask.shape[0]
                        if n == 0:                # (no rows: nothing to step, and an empty tensor has no address to give)
                            continue
                        widths = (C.c_int32 * len(chunk))(*[q.n // n for q in chunk])
                        _abi.check(lib.gsplat_adam_step_rows(len(chunk), arr, widths, n, _p(mask), float(self.betas[0]), float(self.betas[1]),
                                                             float(self.eps), _stream_ptr(dev)), "gsplat_adam_step_rows")
        self._pending_clip = None

    def _row_mask(self, visible):
        """The uint8 [N] tensor of step(visible=...), checked against every tensor the step will touch before anything is counted."""
        mask = visible.data if isinstance(visible, ops.VisibleSet) else visible
        if not isinstance(mask, torch.Tensor):
            raise TypeError("step(visible=...) takes an ops.VisibleSet or its uint8 [N] tensor")
        if mask.dtype != torch.uint8 or mask.dim() != 1 or not mask.is_contiguous():
            raise ValueError(f"step(visible=...): the mask is {mask.dtype} {tuple(mask.shape)}; it must be a contiguous uint8 [N] tensor")
        n = mask.shape[0]
        for g in self.param_groups:
            for p in g['params']:
                if p.grad is None:
                    continue
                if p.dim() < 1 or p.shape[0] != n:
                    raise ValueError(f"step(visible=...): a parameter of shape {tuple(p.shape)} does not have the mask's {n} rows")
                if p.device != mask.device:
                    raise ValueError(f"step(visible=...): the mask is on {mask.device}, a parameter on {p.device}")
        return mask
