"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024; not in the reference): the companion of the
screen-space low-pass (`lowpass=`, `antialias=`).  Every Gaussian is convolved with an isotropic Gaussian whose standard deviation is
sqrt(s) times the smallest world-space distance between two samples that any training camera took of it, so that no Gaussian gets
thinner than anything a training view could have observed.

    pack_cameras(views, device)                         the camera array of the training set (poses and intrinsics only)
    compute(pos, cameras, s=0.2, near=0.2, margin=0.15) filt [N]: the filter's standard deviation per Gaussian
    apply(scale_raw, opacity_raw, filt)                 (scale_raw', opacity_raw'), differentiable: what the render is given
    bake(params_or_model, filt)                         the six tensors with the two filtered ones, no grad: renders, orbits, checkpoints

    s, o = filter3d.apply(m.scale_raw, m.opacity_raw, filt)
    image = gs.render_gaussians(m.pos, m.f_dc, m.f_rest, o, s, m.q_raw, c2w, H, W, fx, fy, cx, cy, lowpass=0.3, antialias=True)

The filter acts in raw-parameter space: with s_j = max(exp(scale_raw_j), 1e-6), sigma = sigmoid(opacity_raw) and f = filt[k],
scale_raw'_j = log sqrt(s_j^2 + f^2) and opacity_raw' = logit(c sigma), c = sqrt(prod s_j^2 / prod (s_j^2 + f^2)) -- the projection
kernel and its structs do not know about it.  The render's own clamp of the opacity at 0.999 then acts on c sigma.  A baked dict is an
ordinary model: saved with harness.save_checkpoint it is in the reference's format, and any viewer shows the filtered Gaussians.

ctypes calls into csrc/gsplat_filter3d.hip on the current stream, in the style of mcmc.py; nothing here reads the device.  The
result of compute() is the same bits every call, on every stream and on every data-parallel rank that holds the same positions.
There is no CPU fallback.
"""
import torch

from . import _abi
from ._dev import _gpu_f32, _launch, _p, _stream_ptr

CAMERA_FLOATS = _abi.GSPLAT_FILTER3D_CAMERA_FLOATS
PARAMS = ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")


def _real(x, name):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= x < float("inf"):
        raise ValueError(f"{name} must be a finite number >= 0, not {x!r}")
    return float(x)


def pack_cameras(views, device):
    """[len(views), CAMERA_FLOATS] fp32 on `device` from the view dicts Trainer.step takes (c2w, H, W, fx, fy, cx, cy; anything else
    in them is ignored): per camera c2w[:3, :4] row-major, fx, fy, cx, cy, W, H, padding (include/gsplat_mi355x.h).  Built on the host
    with one copy to the device."""
    rec = torch.zeros((len(views), CAMERA_FLOATS), dtype=torch.float32)
    for k, v in enumerate(views):
        c2w = torch.as_tensor(v['c2w']).detach().to("cpu", torch.float32)
        if tuple(c2w.shape) != (4, 4):
            raise ValueError(f"view {k}: c2w has shape {tuple(c2w.shape)}, expected (4, 4)")
        rec[k, :12] = c2w[:3, :4].reshape(12)
        rec[k, 12:18] = torch.tensor([float(v['fx']), float(v['fy']), float(v['cx']), float(v['cy']), float(v['W']), float(v['H'])])
    return rec.to(device)


def compute(pos, cameras, s=0.2, near=0.2, margin=0.15, out=None):
    """filt [N] = sqrt(s) min over the cameras that see Gaussian k of z / max(fx, fy) (a Gaussian no camera sees: the largest value of
    the seen ones; no camera, or nobody seen: 0).  `cameras`: pack_cameras(...).  A camera sees k iff z > near and its projection lies
    inside the image widened by `margin` of its size on every side.  One library call (a 4-byte memset and two launches)."""
    s, near, margin = _real(s, "s"), _real(near, "near"), _real(margin, "margin")
    pos = _gpu_f32(pos.detach() if isinstance(pos, torch.Tensor) else pos, "pos", "filter3d")
    cameras = _gpu_f32(cameras, "cameras", "filter3d")
    n = pos.shape[0]
    if pos.numel() != n * 3:
        raise ValueError(f"pos has shape {tuple(pos.shape)}, expected [N, 3]")
    if cameras.dim() != 2 or cameras.shape[1] != CAMERA_FLOATS or cameras.device != pos.device:
        raise ValueError(f"cameras has shape {tuple(cameras.shape)} on {cameras.device}, expected [C, {CAMERA_FLOATS}] on {pos.device} (pack_cameras)")
    dev = pos.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=dev)
        elif _gpu_f32(out, "out", "filter3d").shape != (n,) or out.device != dev:
            raise ValueError(f"out has shape {tuple(out.shape)} on {out.device}, expected ({n},) on {dev}")
        lib = _abi.lib()
        # the maximum's word: a fresh block from the caching allocator per call, so that calls on different streams never share one
        scratch = torch.empty(max(int(lib.gsplat_filter3d_scratch_bytes(n)), 256), dtype=torch.uint8, device=dev)
        _abi.check(lib.gsplat_filter3d_compute(n, _p(pos), cameras.shape[0], _p(cameras), near, margin, s, _p(out), _p(scratch),
                                               _stream_ptr(dev)), "gsplat_filter3d_compute")
    return out


def _check_triple(scale_raw, opacity_raw, filt):
    scale_raw, opacity_raw, filt = _gpu_f32(scale_raw, "scale_raw", "filter3d"), _gpu_f32(opacity_raw, "opacity_raw", "filter3d"), _gpu_f32(filt, "filt", "filter3d")
    n = scale_raw.shape[0]
    if scale_raw.numel() != n * 3 or opacity_raw.numel() != n or filt.numel() != n:
        raise ValueError(f"scale_raw {tuple(scale_raw.shape)}, opacity_raw {tuple(opacity_raw.shape)}, filt {tuple(filt.shape)}: expected "
                         f"[N, 3], [N] or [N, 1], [N]")
    if opacity_raw.device != scale_raw.device or filt.device != scale_raw.device:
        raise ValueError("scale_raw, opacity_raw and filt must be on one device")
    return n


class _ApplyFn(torch.autograd.Function):
    """(scale_raw, opacity_raw) -> (scale_raw', opacity_raw') over gsplat_filter3d_apply / _apply_backward.  The backward recomputes c
    and sigma from the inputs: the forward saves nothing but the three tensors themselves."""

    @staticmethod
    def forward(ctx, scale_raw, opacity_raw, filt):
        n = _check_triple(scale_raw, opacity_raw, filt)
        dev = scale_raw.device
        with torch.cuda.device(dev):
            scale_out, opacity_out = torch.empty_like(scale_raw), torch.empty_like(opacity_raw)
            _abi.check(_abi.lib().gsplat_filter3d_apply(n, _p(scale_raw), _p(opacity_raw), _p(filt), _p(scale_out), _p(opacity_out),
                                                        _stream_ptr(dev)), "gsplat_filter3d_apply")
        ctx.save_for_backward(scale_raw, opacity_raw, filt)
        return scale_out, opacity_out

    @staticmethod
    def backward(ctx, g_scale_out, g_opacity_out):
        scale_raw, opacity_raw, filt = ctx.saved_tensors
        if g_scale_out is None:
            g_scale_out = torch.zeros_like(scale_raw)
        if g_opacity_out is None:
            g_opacity_out = torch.zeros_like(opacity_raw)
        g_scale_out, g_opacity_out = g_scale_out.contiguous(), g_opacity_out.contiguous()
        g_scale, g_opacity = torch.empty_like(scale_raw), torch.empty_like(opacity_raw)
        backward_into(scale_raw, opacity_raw, filt, g_scale_out, g_opacity_out, g_scale, g_opacity)
        return g_scale, g_opacity, None


def apply(scale_raw, opacity_raw, filt):
    """(scale_raw', opacity_raw'): the raw parameters of the Gaussians convolved with their filter, differentiable with respect to
    scale_raw and opacity_raw (filt gets no gradient).  opacity_raw keeps its shape ([N] or [N, 1]).  A row with filt == 0 comes back
    bit for bit.  One launch each way."""
    return _ApplyFn.apply(scale_raw, opacity_raw, filt.detach())


@torch.no_grad()
def backward_into(scale_raw, opacity_raw, filt, g_scale_out, g_opacity_out, g_scale_raw, g_opacity_raw, accumulate=False):
    """The vector-Jacobian product of apply() written to (accumulate: added to) g_scale_raw / g_opacity_raw: one launch.  The map is
    linear in the gradient and row-local, so the trainer runs it ONCE on the gradients summed over views and ranks."""
    n = _check_triple(scale_raw, opacity_raw, filt)
    for name, t, ref in (("g_scale_out", g_scale_out, scale_raw), ("g_opacity_out", g_opacity_out, opacity_raw),
                         ("g_scale_raw", g_scale_raw, scale_raw), ("g_opacity_raw", g_opacity_raw, opacity_raw)):
        if _gpu_f32(t, name, "filter3d").numel() != ref.numel() or t.device != ref.device:
            raise ValueError(f"{name} has shape {tuple(t.shape)} on {t.device}, expected {tuple(ref.shape)} on {ref.device}")
    dev = scale_raw.device
    _launch("gsplat_filter3d_apply_backward", dev, n, _p(scale_raw), _p(opacity_raw), _p(filt), _p(g_scale_out), _p(g_opacity_out),
            _p(g_scale_raw), _p(g_opacity_raw), 1 if accumulate else 0)


@torch.no_grad()
def bake(params_or_model, filt):
    """{name: tensor} of the six parameters with scale_raw / opacity_raw replaced by the filtered ones, detached: an ordinary model for
    render_frames, the harness orbits and harness.save_checkpoint (whose formats stay as they are: the filter is IN the numbers)."""
    get = params_or_model.__getitem__ if isinstance(params_or_model, dict) else (lambda k: getattr(params_or_model, k))
    t = {k: get(k).detach() for k in PARAMS}
    t["scale_raw"], t["opacity_raw"] = apply(t["scale_raw"].contiguous(), t["opacity_raw"].contiguous(), filt)
    return t
