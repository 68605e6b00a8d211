"""Training loss of the reference (gaussian_splatting/losses.py) on the MI355X: L1 + SSIM, value and gradient from two
fused HIP kernels (csrc/gsplat_loss.hip) -- SURVEY.md §8(f), "next" row 1.

Same names, arguments and return values as the reference:
    l1_loss(pred, target)                                              losses.py:27
    ssim_loss(pred, target, window_size=11, size_average=True)         losses.py:44
    compute_loss(pred, target, lambda_l1=0.8, lambda_ssim=0.2)         losses.py:158  -> (total, {'l1', 'ssim', 'total'})
pred / target: [H, W, 3] or [B, H, W, 3].  Differentiable w.r.t. `pred` (the reference never needs d/d target).

Not in the reference: aux_loss, the loss on the depth / opacity maps of an aux render against a target depth and a
target opacity, and composite_over, a target image with an alpha channel over a background colour -- one HIP kernel each way.
"""
import ctypes as C

import torch

from . import _abi
from ._dev import _f32, _p, _stream_ptr
from ._timing import _stage


class _LossFn(torch.autograd.Function):
    """(total, values): total = scale * (l1w * l1 + sw * (1 - ssim)), differentiable w.r.t. pred; values = scale * (l1, 1 - ssim,
    total), detached.  The forward leaves the SSIM term's partial-derivative maps in scratch; the gradient is written by the backward,
    with the upstream scalar multiplied in by the kernel (gsplat_loss_forward / gsplat_loss_backward)."""

    @staticmethod
    def forward(ctx, pred, target, l1w, sw, scale=1.0):
        lib = _abi.lib()
        shape = tuple(pred.shape)
        if len(shape) not in (3, 4) or shape[-1] != 3 or tuple(target.shape) != shape:
            raise ValueError(f"pred/target must both be [H, W, 3] or [B, H, W, 3], got {shape} and {tuple(target.shape)}")
        b = shape[0] if len(shape) == 4 else 1
        h, w = shape[-3], shape[-2]
        x, y = _f32(pred, shape, "pred"), _f32(target, shape, "target")
        dev = x.device
        need = ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            values = torch.empty(3, dtype=torch.float32, device=dev)
            total = torch.empty((), dtype=torch.float32, device=dev)
            scratch = torch.empty(lib.gsplat_loss_scratch_bytes(b, h, w, 1 if need else 0), dtype=torch.uint8, device=dev)
            with _stage("loss"):
                _abi.check(lib.gsplat_loss_forward(_p(x), _p(y), b, h, w, float(l1w), float(sw), float(scale), _p(values), _p(total),
                                                   _p(scratch), 1 if need else 0, _stream_ptr(dev)), "gsplat_loss_forward")
        ctx.saved = (x, y, scratch, b, h, w, float(l1w), float(sw), float(scale)) if need else None
        ctx.dtype = pred.dtype
        ctx.mark_non_differentiable(values)
        return total, values

    @staticmethod
    def backward(ctx, g_total, _g_values):
        lib = _abi.lib()
        x, y, scratch, b, h, w, l1w, sw, scale = ctx.saved
        dev = x.device
        up = g_total.detach().to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            grad = torch.empty_like(x)
            with _stage("loss"):
                _abi.check(lib.gsplat_loss_backward(_p(x), _p(y), b, h, w, l1w, sw, scale, _p(up), _p(grad), _p(scratch), _stream_ptr(dev)),
                           "gsplat_loss_backward")
        return (grad if ctx.dtype == torch.float32 else grad.to(ctx.dtype)), None, None, None, None


def compute_loss(pred, target, lambda_l1=0.8, lambda_ssim=0.2):
    """lambda_l1 * L1 + lambda_ssim * (1 - SSIM); returns (total_loss, dict of floats) like the reference."""
    total, v = _LossFn.apply(pred, target, lambda_l1, lambda_ssim)
    l1, ssim, tot = v.tolist()                       # ONE host read instead of the reference's three .item() calls
    return (total if pred.dtype == torch.float32 else total.to(pred.dtype)), {'l1': l1, 'ssim': ssim, 'total': tot}


def l1_loss(pred, target):
    return _LossFn.apply(pred, target, 1.0, 0.0)[0].to(pred.dtype)


def ssim_loss(pred, target, window_size=11, size_average=True):
    if window_size != 11 or not size_average:
        raise NotImplementedError("the fused kernel implements the reference defaults: window_size=11, size_average=True")
    return _LossFn.apply(pred, target, 0.0, 1.0)[0].to(pred.dtype)


def compute_loss_device(pred, target, lambda_l1=0.8, lambda_ssim=0.2, scale=1.0):
    """compute_loss without the host read: returns (total_loss, values) with values = device tensor scale * [l1, 1 - ssim, total]
    (the training step keeps the loss on the GPU and reads it only when the caller logs it).  `scale` (1 / batch size in the
    training loop) is applied by the kernels: the value comes out scaled and so does the gradient."""
    total, v = _LossFn.apply(pred, target, lambda_l1, lambda_ssim, scale)
    return (total if pred.dtype == torch.float32 else total.to(pred.dtype)), v


class _AuxLossFn(torch.autograd.Function):
    """(total, values) of the auxiliary loss, differentiable w.r.t. depth and alpha (gsplat_aux_loss_forward / _backward); the
    gradient of a map whose term is off is None."""

    @staticmethod
    def forward(ctx, depth, alpha, target_depth, target_alpha, lambda_depth, lambda_alpha, scale):
        lib = _abi.lib()
        shape = tuple(alpha.shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"alpha must be [H, W] or [B, H, W], got {shape}")
        b = shape[0] if len(shape) == 3 else 1
        h, w = shape[-2], shape[-1]
        a = _f32(alpha, shape, "alpha")
        z = _f32(target_depth, shape, "target_depth") if target_depth is not None else None
        m = _f32(target_alpha, shape, "target_alpha") if target_alpha is not None else None
        if z is not None and depth is None:
            raise ValueError("a target depth needs the render's depth map")
        d = _f32(depth, shape, "depth") if z is not None else None
        dev = a.device
        need_d = depth is not None and ctx.needs_input_grad[0] and z is not None
        need_a = ctx.needs_input_grad[1] and (z is not None or m is not None)
        with torch.cuda.device(dev):
            values = torch.empty(3, dtype=torch.float32, device=dev)
            total = torch.empty((), dtype=torch.float32, device=dev)
            scratch = torch.empty(lib.gsplat_aux_loss_scratch_bytes(b, h, w), dtype=torch.uint8, device=dev)
            with _stage("loss"):
                _abi.check(lib.gsplat_aux_loss_forward(_p(d), _p(a), _p(z), _p(m), b, h, w, float(lambda_depth), float(lambda_alpha), float(scale),
                                                       _p(values), _p(total), _p(scratch), _stream_ptr(dev)), "gsplat_aux_loss_forward")
        ctx.saved = (d, a, z, m, scratch, b, h, w, float(lambda_depth), float(lambda_alpha), float(scale)) if need_d or need_a else None
        ctx.need = (need_d, need_a)
        ctx.dtypes = (depth.dtype if depth is not None else None, alpha.dtype)
        ctx.mark_non_differentiable(values)
        return total, values

    @staticmethod
    def backward(ctx, g_total, _g_values):
        need_d, need_a = ctx.need
        if ctx.saved is None:
            return (None,) * 7
        lib = _abi.lib()
        d, a, z, m, scratch, b, h, w, ld, la, scale = ctx.saved
        dev = a.device
        up = g_total.detach().to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            gd = torch.empty_like(a) if z is not None else None          # (the entry writes both maps of a depth term)
            ga = torch.empty_like(a)
            with _stage("loss"):
                _abi.check(lib.gsplat_aux_loss_backward(_p(d), _p(a), _p(z), _p(m), b, h, w, ld, la, scale, _p(up), _p(gd), _p(ga), _p(scratch),
                                                        _stream_ptr(dev)), "gsplat_aux_loss_backward")
        gd = None if not need_d else gd if ctx.dtypes[0] == torch.float32 else gd.to(ctx.dtypes[0])
        ga = None if not need_a else ga if ctx.dtypes[1] == torch.float32 else ga.to(ctx.dtypes[1])
        return gd, ga, None, None, None, None, None


def aux_loss(depth, alpha, target_depth=None, target_alpha=None, lambda_depth=1.0, lambda_alpha=1.0, scale=1.0):
    """The loss on the maps of an aux render (ops.render / render_gaussians with aux=True): depth = D, alpha = A, [H, W] or
    [B, H, W].  target_depth = Z in camera-space z, the unit of D (<= 0 or non-finite: no data there), target_alpha = M:

        L_alpha = mean |A - M|,   L_depth = sum over valid Z of |D - A Z| / max(1, number of valid Z)
        total = scale * (lambda_alpha L_alpha + lambda_depth L_depth)

    |D - A Z| is the composited depth residual |sum w_i (z_i - Z)|: un-normalised like the maps, exactly zero with a zero gradient on
    an empty pixel (a loss on D / A is one line of autograd for a caller who wants it).  Returns (total, values): total is
    differentiable w.r.t. depth and alpha (None for a map whose term is off: target None), values = scale * [L_alpha, L_depth,
    lambda_alpha L_alpha + lambda_depth L_depth], a detached device tensor.  A term whose target is None is off and its value 0;
    depth may then be None."""
    total, v = _AuxLossFn.apply(depth, alpha, target_depth, target_alpha, lambda_depth, lambda_alpha, scale)
    return (total if alpha.dtype == torch.float32 else total.to(alpha.dtype)), v


@torch.no_grad()
def composite_over(rgb, alpha, background):
    """rgb * alpha + (1 - alpha) * background: a target image with an alpha channel over a background colour.  rgb [H, W, 3] or
    [B, H, W, 3] is straight colour (not pre-multiplied), alpha [H, W] or [B, H, W], background 3 numbers; values in [0, 1], nothing
    is clamped.  fp32 out, no gradient."""
    lib = _abi.lib()
    shape = tuple(rgb.shape)
    if len(shape) not in (3, 4) or shape[-1] != 3 or tuple(alpha.shape) != shape[:-1]:
        raise ValueError(f"rgb must be [H, W, 3] or [B, H, W, 3] and alpha its [H, W] or [B, H, W], got {shape} and {tuple(alpha.shape)}")
    vals = background.detach().reshape(-1).tolist() if isinstance(background, torch.Tensor) else list(background)
    if len(vals) != 3:
        raise ValueError("background must hold 3 numbers (r, g, b)")
    b = shape[0] if len(shape) == 4 else 1
    c, a = _f32(rgb, shape, "rgb"), _f32(alpha, shape[:-1], "alpha")
    dev = c.device
    with torch.cuda.device(dev):
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        _abi.check(lib.gsplat_composite_target(_p(c), _p(a), (C.c_float * 3)(*map(float, vals)), b, shape[-3], shape[-2], _p(out),
                                               _stream_ptr(dev)), "gsplat_composite_target")
    return out
