"""What the per-view tables share (exposure.ExposureTable, bilagrid.BilateralGridTable, poses.PoseTable): one
autograd skeleton for an op `out = f(image, table row)` over a pair of library entries (for the pose table the "image" is the camera
pose), and one table of such rows with its gradient buffer and its own Adam.  An op plugs its three parts into the skeleton as a
ViewOp; a table names its op, its identity and its Adam defaults.
Nothing here reads the device, and there is no CPU fallback."""
import collections
import numbers

import torch

from . import optim
from ._dev import _f32, _stream_ptr

# The parts of an op.  `arg`: what its second argument is called in messages.  shapes(image, table) -> (the image's shape, the integers
# both entries take after the arrays); ValueError for a pair that does not fit.  forward(x, t, dims, out, stream) and
# backward(x, t, g, dims, g_image, target, rows, flags, stream) make the library calls (target None: the table's gradient is not wanted;
# whatever scratch the call needs is allocated there).  `accumulate`: the entry's flag for "ADD into the rows `rows` names".  `first`:
# what the first argument is called in messages.
ViewOp = collections.namedtuple("ViewOp", "arg shapes forward backward accumulate first", defaults=("image",))


class ViewFn(torch.autograd.Function):
    """out = op(image, table).  `dest` is None (the gradient of the table argument is returned to autograd) or (grad buffer [V, ...],
    row [1] int32 on the device): the backward then ADDS the view's gradient into that row of the buffer itself and returns none -- no
    dense table-sized tensor per view.  `anchor`: a scalar leaf that requires a gradient (it never gets one), so that the backward runs
    for the table even where the image needs none."""

    @staticmethod
    def forward(ctx, op, image, table, dest, anchor):
        if not isinstance(image, torch.Tensor) or not isinstance(table, torch.Tensor):
            raise TypeError(f"{op.first} and {op.arg} must be torch.Tensors")
        shape, dims = op.shapes(image, table)
        x, t = _f32(image, shape, op.first), _f32(table, tuple(table.shape), op.arg)
        if t.device != x.device:
            raise ValueError(f"{op.first} is on {x.device}, {op.arg} on {t.device}")
        dev = x.device
        with torch.cuda.device(dev):
            out = torch.empty(shape, dtype=torch.float32, device=dev)
            op.forward(x, t, dims, out, _stream_ptr(dev))
        need_image = ctx.needs_input_grad[1]
        need_table = ctx.needs_input_grad[2] if dest is None else True
        ctx.saved = (op, x, t, dims, dest) if need_image or need_table else None
        ctx.need = (need_image, need_table)
        ctx.dtypes = (image.dtype, table.dtype)
        return out if image.dtype == torch.float32 else out.to(image.dtype)

    @staticmethod
    def backward(ctx, g_out):
        need_image, need_table = ctx.need
        if ctx.saved is None:
            return None, None, None, None, None
        op, x, t, dims, dest = ctx.saved
        dev = x.device
        g = _f32(g_out, tuple(x.shape), "grad_out")
        with torch.cuda.device(dev):
            g_image = torch.empty_like(x) if need_image else None
            g_table = target = rows = None
            flags = 0
            if need_table:
                if dest is None:
                    g_table = target = torch.empty_like(t)
                else:
                    target, rows = dest
                    flags = op.accumulate
            op.backward(x, t, g, dims, g_image, target, rows, flags, _stream_ptr(dev))
        if g_image is not None and ctx.dtypes[0] != torch.float32:
            g_image = g_image.to(ctx.dtypes[0])
        if g_table is not None and ctx.dtypes[1] != torch.float32:
            g_table = g_table.to(ctx.dtypes[1])
        return None, g_image, g_table, None, None


class ViewTable:
    """One row of parameters per training image: `params` [V, ...] at the identity, `grad` a buffer of the same shape, and an Adam state
    of its own -- a second optim.GaussianAdam over the one tensor (a dense step), apart from the model's optimiser: restarts of that one
    after a densification touch neither the table nor its moments.

    A subclass has `name` ('exposure', 'bilagrid', 'pose': its optimiser group, and the prefix of its TrainConfig fields), `op` (the ViewOp
    apply_view calls) and _identity(device) (one row at the identity); it may override regularise()."""

    def __init__(self, n_views, device, lr, betas, eps):
        if type(n_views) is not int or n_views < 1:
            raise ValueError(f"n_views must be an integer >= 1, not {n_views!r}")
        device = torch.device(device)
        self.n_views = n_views
        row = self._identity(device)
        self.params = row.expand(n_views, *row.shape).contiguous()
        self.grad = torch.zeros_like(self.params)
        self.optimizer = optim.GaussianAdam([{'params': [self.params], 'lr': float(lr), 'name': self.name}], betas=betas, eps=eps)
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
        """The op of view `idx` on image [H, W, 3].  Differentiable with respect to the image; the backward ADDS the view's gradient into
        grad[idx] (the backward entry with a row_index and its ACCUMULATE flag): no dense table-sized tensor is produced or added per
        view.  Two views with the same idx must run their backward passes in one stream order (Trainer.step sees to it)."""
        idx = self.check_index(idx)
        return ViewFn.apply(self.op, image, self.params[idx], (self.grad, self._rows[idx:idx + 1]), self._anchor)

    def regularise(self, cfg):
        """The table's once-per-iteration term, for Trainer.step after the all-reduce of `grad`: adds it to `grad` and returns what it
        contributes to step()'s dict (device scalars).  Here: nothing."""
        return {}

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
