"""Per-view bilateral grids (not in the reference): a global affine per image (exposure.py) absorbs exposure and white
balance, not what an in-camera ISP does LOCALLY -- tone mapping, vignetting, highlight roll-off vary over the frame and with
brightness.  As in gsplat (use_bilateral_grid, after "Bilateral Guided Radiance Field Processing"), every training image gets a
low-resolution grid of affine colour transforms, sliced at (pixel x, pixel y, pixel luminance) and applied to the rendered frame
before the loss; a total-variation term keeps it smooth:

    G[12, L, Y, X]: channel 4 r + k = entry (r, k) of [M | t];   out = A(x, y, lum(c)) [c, 1],  A the trilinear slice;  no clamp

    slice(image, grids)                      the op, differentiable with respect to both
    tv_loss(grids)                           the total variation of a table [V, 12, L, Y, X]
    BilateralGridTable(n_views, device)      one grid per training image at the identity, their gradient buffer, an Adam of their own
    table.apply_view(image, idx)             the slice of view idx; its backward adds into table.grad[idx]
    table.add_tv_grad(weight)                grad += weight dtv/dG; returns weight tv

TrainConfig.bilagrid switches it on in Trainer.step.  Novel views are rendered without it.

ctypes calls into csrc/gsplat_bilagrid.hip on the current stream, in the style of exposure.py; nothing here reads the device.  The
gradient of a grid is gathered per vertex in a fixed order without float atomics: the same bits on every call, every stream and every
launch, with or without gs.set_deterministic(True).  There is no CPU fallback.
"""
import torch

from . import _abi
from ._viewtable import ViewFn, ViewOp, ViewTable
from ._dev import _f32, _p, _stream_ptr

DEFAULT_SHAPE = (16, 16, 8)      # (X, Y, L)


def check_shape(shape):
    """(X, Y, L) as three ints with 2 <= X, Y <= 64 and 2 <= L <= 16 (anything else: ValueError)."""
    try:
        ok = len(shape) == 3 and all(type(s) is int for s in shape)
    except TypeError:
        ok = False
    if not ok or not (2 <= shape[0] <= 64 and 2 <= shape[1] <= 64 and 2 <= shape[2] <= 16):
        raise ValueError(f"a bilateral grid's shape must be three integers (X, Y, L) with 2 <= X, Y <= 64 and 2 <= L <= 16, not {shape!r}")
    return tuple(shape)


def _shapes(image, grids):
    shape, gshape = tuple(image.shape), tuple(grids.shape)
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise ValueError(f"image must be [H, W, 3] or [B, H, W, 3], got {shape}")
    b = shape[0] if len(shape) == 4 else 1
    lead = (b, 12) if len(shape) == 4 else (12,)
    if len(gshape) != len(lead) + 3 or gshape[:len(lead)] != lead:
        raise ValueError(f"grids must be {list(lead)} + [L, Y, X] for an image of {list(shape)}, got {list(gshape)}")
    if min(shape) < 1:
        raise ValueError(f"image has an empty dimension: {shape}")
    L, Y, X = gshape[-3:]
    check_shape((X, Y, L))
    return shape, (b, shape[-3], shape[-2], X, Y, L)


def _forward(x, g, dims, out, stream):
    _abi.check(_abi.lib().gsplat_bilagrid_forward(_p(x), _p(g), *dims, _p(out), stream), "gsplat_bilagrid_forward")


def _backward(x, g, go, dims, g_image, target, rows, flags, stream):
    _abi.check(_abi.lib().gsplat_bilagrid_backward(_p(x), _p(g), _p(go), *dims, _p(g_image), _p(target), _p(rows), flags, stream),
               "gsplat_bilagrid_backward")


# out = A [c, 1] over gsplat_bilagrid_forward / gsplat_bilagrid_backward, in the skeleton of _viewtable.ViewFn
_OP = ViewOp("grids", _shapes, _forward, _backward, _abi.GSPLAT_BILAGRID_ACCUMULATE)


def slice(image, grids):
    """The grid sliced at every pixel's (x, y, luminance) and applied to its colour: image [H, W, 3] with grids [12, L, Y, X], or
    [B, H, W, 3] with [B, 12, L, Y, X] (one grid per image).  Nothing is clamped; the identity grid returns the image bit for bit.
    Differentiable with respect to both; the half that is not needed is not computed.  fp32 is computed directly, other dtypes are
    converted.  One launch forward, one per gradient backward."""
    return ViewFn.apply(_OP, image, grids, None, None)


def _tv(grids, scale, want_loss, grad, accumulate):
    """gsplat_bilagrid_tv on a contiguous fp32 table; returns the device scalar scale tv (None unless want_loss)."""
    V, _, L, Y, X = grids.shape
    lib, dev = _abi.lib(), grids.device
    with torch.cuda.device(dev):
        loss = scratch = None
        if want_loss:
            loss = torch.empty((), dtype=torch.float32, device=dev)
            scratch = torch.empty(lib.gsplat_bilagrid_tv_scratch_bytes(V, X, Y, L), dtype=torch.uint8, device=dev)
        _abi.check(lib.gsplat_bilagrid_tv(_p(grids), V, X, Y, L, float(scale), _p(loss), _p(grad),
                                          _abi.GSPLAT_BILAGRID_ACCUMULATE if accumulate else 0, _p(scratch), _stream_ptr(dev)), "gsplat_bilagrid_tv")
    return loss


def _table(grids):
    if not isinstance(grids, torch.Tensor):
        raise TypeError("grids must be a torch.Tensor")
    shape = tuple(grids.shape)
    if len(shape) != 5 or shape[1] != 12 or shape[0] < 1:
        raise ValueError(f"grids must be [V, 12, L, Y, X], got {list(shape)}")
    check_shape((shape[4], shape[3], shape[2]))
    return _f32(grids, shape, "grids")


class _TvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        g = _table(grids)
        ctx.saved = g if ctx.needs_input_grad[0] else None
        ctx.dtype = grids.dtype
        return _tv(g, 1.0, True, None, False)

    @staticmethod
    def backward(ctx, g_loss):
        if ctx.saved is None:
            return None
        grad = torch.empty_like(ctx.saved)
        _tv(ctx.saved, 1.0, False, grad, False)
        grad = grad * g_loss.to(torch.float32)
        return grad if ctx.dtype == torch.float32 else grad.to(ctx.dtype)


def tv_loss(grids):
    """The total variation of a table grids [V, 12, L, Y, X]: (1 / V) sum_v sum_axis mean((G shifted by one along the axis - G)^2)
    over the axes L, Y, X -- a device scalar, differentiable.  The loss is added in a fixed order in double; the gradient is a gather."""
    return _TvFn.apply(grids)


class BilateralGridTable(ViewTable):
    """One grid per training image: `params` [V, 12, L, Y, X] at the identity, `grad` a buffer of the same shape, and an Adam state of
    its own -- a second optim.GaussianAdam over the one tensor (eps = 1e-15 and a dense step, as gsplat's trainer), apart from the
    model's optimiser: restarts of that one after a densification touch neither the table nor its moments.

        table.zero_grad()
        out = table.apply_view(rendered, idx); loss(out).backward()          # adds into table.grad[idx]
        tv = table.add_tv_grad(10.0)                                         # grad += 10 dtv/dG; returns 10 tv
        table.step(lr)
    """

    name, op = 'bilagrid', _OP

    def __init__(self, n_views, device, shape=DEFAULT_SHAPE, lr=0.002, betas=(0.9, 0.999), eps=1e-15):
        self.shape = shape                          # (checked in _identity: n_views is refused first)
        super().__init__(n_views, device, lr, betas, eps)

    def _identity(self, device):
        X, Y, L = self.shape = check_shape(self.shape)
        return torch.eye(3, 4, dtype=torch.float32, device=device).reshape(12, 1, 1, 1).expand(12, L, Y, X)

    @torch.no_grad()
    def add_tv_grad(self, weight):
        """grad += weight dtv/dG over the whole table (one library call; nothing read back).  Returns the device scalar weight tv."""
        return _tv(self.params, weight, True, self.grad, True)

    def regularise(self, cfg):
        """grad += cfg.bilagrid_tv dtv/dG; {'tv': the weighted term}."""
        return {'tv': self.add_tv_grad(cfg.bilagrid_tv)}
