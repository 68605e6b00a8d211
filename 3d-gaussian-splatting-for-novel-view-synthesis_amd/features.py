"""Per-Gaussian feature vectors through the rasteriser (not in the reference): N-channel maps and their adjoint.

    render(pos, feats, opacity_raw, scale_raw, q_raw, c2w, H, W, fx, fy, cx, cy, ...)   map [H, W, C]:  F[p, c] = sum_i w_i(p) feats[i, c]
    lift(pos, opacity_raw, scale_raw, q_raw, c2ws, maps, H, W, fx, fy, cx, cy, ...)     (sums [N, C], weight [N]):
                                                                                        sums[i, c] = sum_views sum_p w_i(p) maps[v][p, c]

w_i(p) = alpha_i T_i [T_i > 5e-5] is the blending weight of Gaussian i at pixel p, the very weight the image is composited with: the
same projection, lists, thresholds and arithmetic (csrc/gs_features.h walks the lists with the forward rasteriser's own pieces).  What
is blended is the caller's table instead of the SH colour: segmentation masks, language or feature fields, labels, a per-Gaussian
scalar.  The map is neither clamped nor normalised, and features may have either sign; a channel of ones renders the opacity map A
(the `alpha` of render_gaussians(aux=True)).  A table of C channels costs ceil(C / 8) traversals of the lists.

`render` is differentiable with respect to `feats` ONLY -- its backward pass is the adjoint kernel, g[i, c] = sum_p w_i(p) G[p, c] --
and the geometry is frozen: a pos, opacity_raw, scale_raw, q_raw or c2w that requires grad is refused (ValueError), not given a silent
zero.  The adjoint adds with float atomics, in arrival order; there is no deterministic variant, and under set_deterministic(True)
`render` raises ValueError.  `lift` is the same adjoint used forwards: it carries 2D maps onto the Gaussians in closed form.

Rows follow the Gaussians' index.  Densification, pruning and relocation do not carry a feature table along: these ops are for a
model that has stopped changing.

Every call is a waited frame (the host waits once per pose for the pair count, so the binning buffers are exact), inside
deferred_checks() too.  ctypes calls on the current stream; there is no CPU fallback.
"""
import ctypes as C

import torch

from . import _abi, ops
from ._dev import _f32, _p

MAX_CHANNELS = _abi.GSPLAT_FEATURES_MAX_CHANNELS


def _spec(H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff, lowpass, antialias):
    return ops._frame_spec(True, H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff,
                           sh_degree=0, lowpass=lowpass, antialias=antialias)


def _check_geometry(who, tensors):
    """pos ... q_raw are tensors; pos is [N, 3].  Returns (n, device).  Queues nothing."""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    pos = tensors["pos"]
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"{who}: pos has shape {tuple(pos.shape)}, expected [N, 3]")
    return pos.shape[0], pos.device


def _check_table(who, name, t, shape, dev, cmax):
    """`t` is a contiguous float32 tensor of `shape` (None: any length) on `dev`, its last dimension C in 1 .. cmax."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    want = "[" + ", ".join("C" if s is None else str(s) for s in shape) + "]"
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {want}")
    if not 1 <= t.shape[-1] <= cmax:
        raise ValueError(f"{who}: {name} has {t.shape[-1]} channels, expected 1 .. {cmax}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 tensor {want}, not {t.dtype}{'' if t.is_contiguous() else ' (not contiguous)'}")
    if t.device != dev:
        raise ValueError(f"{who}: {name} is on {t.device}, pos on {dev}")


def _need_gpu(who, name, t):
    """(the last check: what is wrong with the arguments themselves is said first, on any device)"""
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} is on {t.device}: the MI355X rasterizer needs GPU tensors (there is no CPU fallback)")


def _front(spec, tensors, n, dev):
    """(front, held): ops._WaitedFront over the converted geometry (None for n == 0) and the tensors behind its addresses, which the
    caller keeps until its last frame is queued: the geometry in fp32, a zero f_dc of the op's own (degree 0 reads no f_rest: f_dc again)."""
    opa = tensors["opacity_raw"]
    ins = dict(pos=_f32(tensors["pos"], (n, 3), "pos"), opacity_raw=_f32(opa if opa.dim() == 1 else opa.reshape(-1), (n,), "opacity_raw"),
               scale_raw=_f32(tensors["scale_raw"], (n, 3), "scale_raw"), q_raw=_f32(tensors["q_raw"], (n, 4), "q_raw"))
    if n == 0:
        return None, ins
    f_dc = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    g = _abi.Gaussians(n, _p(ins["pos"]), _p(ins["opacity_raw"]), None, None, _p(ins["scale_raw"]), _p(ins["q_raw"]), _p(f_dc), _p(f_dc))
    return ops._WaitedFront(spec, g, n, dev, ops._PROJECT_DEGREE[0] | spec.filter), (ins, f_dc)


def _call(name, front, fr, src, channels, dst, st):
    """The library's `name` (gsplat_features_forward / _adjoint) on the frame fr = (pairs, bin_state) of `front`, on the stream `st`."""
    _abi.check(getattr(_abi.lib(), name)(front.n, fr[0], C.byref(front.view), _p(front.proj_state), _p(fr[1]), _p(src), channels, _p(dst), st), name)


class _FeatureFn(torch.autograd.Function):
    """apply(feats, spec, front, c2w): the map [H, W, C].  The node keeps the front end with its project_state and the frame's
    bin_state (neither run again nor changed) and its backward pass is gsplat_features_adjoint into a zeroed
    [N, C], on the backward pass's own current stream."""

    @staticmethod
    def forward(ctx, feats, spec, front, c2w):
        dev, ch = feats.device, feats.shape[1]
        ctx.frame = None
        ctx.shape = feats.shape
        fr = front.frame(c2w) if front is not None else None
        if fr is None:                           # no survivor: the zero map, and a zero gradient
            return torch.zeros((spec.H, spec.W, ch), dtype=torch.float32, device=dev)
        out = torch.empty((spec.H, spec.W, ch), dtype=torch.float32, device=dev)
        _call("gsplat_features_forward", front, fr, feats, ch, out, front.st)
        ctx.frame = (front, fr, torch.cuda.current_stream(dev))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad = torch.zeros(ctx.shape, dtype=torch.float32, device=grad_out.device)
        if ctx.frame is not None:
            front, fr, stream = ctx.frame
            g = grad_out.detach()
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
            here, _, st = ops._stream_key(g.device)                  # (the backward pass's own current stream)
            if here != stream:
                here.wait_stream(stream)
            _call("gsplat_features_adjoint", front, fr, g, ctx.shape[1], grad, st)
        return grad, None, None, None


def render(pos, feats, opacity_raw, scale_raw, q_raw, c2w, H, W, fx, fy, cx, cy, near=0.01, far=100.0, pix_guard=32, T=16,
           min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1 / 128., *, lowpass=0.0, antialias=False):
    """The map [H, W, C] float32 of the table `feats` [N, C] (contiguous float32 on pos.device, 1 <= C <= 512) under the camera c2w:
    F[p, c] = sum_i w_i(p) feats[i, c], the weights of render_gaussians() with the same geometry, camera and thresholds (arguments as
    there; lowpass, antialias: DESIGN.md §16).  Not clamped, not normalised, no background; a pixel no Gaussian reaches is 0.0.  A
    channel of ones renders the opacity map A.

    Differentiable with respect to `feats` only (the adjoint kernel; float atomics).  ValueError: a geometry tensor or c2w that
    requires grad (the geometry is frozen here); set_deterministic(True) (there is no deterministic adjoint); a feats that is not a
    contiguous float32 [N, C] on pos.device, or C outside 1 .. 512.  RuntimeError: CPU tensors (no CPU fallback).  Always a waited
    frame, inside deferred_checks() too.  No survivor: the zero map; survivors but none on screen: the reference's off-screen
    Exception."""
    who = "features.render"
    spec = _spec(H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff, lowpass, antialias)
    geometry = dict(pos=pos, opacity_raw=opacity_raw, scale_raw=scale_raw, q_raw=q_raw)
    n, dev = _check_geometry(who, geometry)
    if not isinstance(c2w, torch.Tensor):
        c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev)
    frozen = [k for k, t in dict(geometry, c2w=c2w).items() if t.requires_grad]
    if frozen:
        raise ValueError(f"{who}: the geometry is frozen here -- {', '.join(frozen)} requires grad, and this op differentiates with respect "
                         "to feats only (detach it; render_gaussians() has the gradients of the geometry)")
    if ops._deterministic:
        raise ValueError(f"{who}: there is no deterministic adjoint (float atomics add in arrival order): not available under set_deterministic(True)")
    _check_table(who, "feats", feats, (n, None), dev, MAX_CHANNELS)
    _need_gpu(who, "feats", feats)
    front, held = _front(spec, geometry, n, dev)
    return _FeatureFn.apply(feats, spec, front, _f32(c2w, (4, 4), "c2w"))


@torch.no_grad()
def lift(pos, opacity_raw, scale_raw, q_raw, c2ws, maps, H, W, fx, fy, cx, cy, near=0.01, far=100.0, pix_guard=32, T=16,
         min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1 / 128., *, lowpass=0.0, antialias=False, out=None):
    """Carry the 2D maps of the poses `c2ws` onto the Gaussians: (sums [N, C], weight [N]), float32,
        sums[i, c] = sum_v sum_p w_i(p; v) maps[v][p, c]        weight[i] = sum_v sum_p w_i(p; v),
    for maps [V, H, W, C] or a list of V maps [H, W, C] (contiguous float32 on pos.device, 1 <= C <= 511).  Per pose: project -> bin ->
    the adjoint kernel on that view's map; the weight is the adjoint of a map of ones, carried as channel C of the same launches.
    Accumulates into `out` = (sums, weight) of an earlier call, or into a fresh zeroed pair; returns it.  The caller divides:

        mean = sums / weight.clamp_min(eps)[:, None]

    Forward-only: nothing is saved for a backward pass.  Float atomics: the last bits differ from run to run; under
    set_deterministic(True) it raises ValueError.  A pose without a survivor adds nothing; one with survivors but none on screen
    raises the reference's off-screen Exception, and the pair then holds the poses before it.  There is no CPU fallback."""
    who = "features.lift"
    spec = _spec(H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff, lowpass, antialias)
    geometry = dict(pos=pos, opacity_raw=opacity_raw, scale_raw=scale_raw, q_raw=q_raw)
    n, dev = _check_geometry(who, geometry)
    if ops._deterministic:
        raise ValueError(f"{who}: there is no deterministic adjoint (float atomics add in arrival order): not available under set_deterministic(True)")
    c2ws, maps = list(c2ws), (list(maps) if not isinstance(maps, torch.Tensor) else maps)
    if len(maps) != len(c2ws):
        raise ValueError(f"{who}: {len(maps)} maps for {len(c2ws)} poses")
    if len(c2ws) == 0:
        raise ValueError(f"{who}: no pose given")
    if isinstance(maps, torch.Tensor):
        _check_table(who, "maps", maps, (len(c2ws), spec.H, spec.W, None), dev, MAX_CHANNELS - 1)
    else:
        for k, m in enumerate(maps):
            _check_table(who, f"maps[{k}]", m, (spec.H, spec.W, None), dev, MAX_CHANNELS - 1)
            if m.shape[-1] != maps[0].shape[-1]:
                raise ValueError(f"{who}: maps[{k}] has {m.shape[-1]} channels, maps[0] {maps[0].shape[-1]}")
    ch = maps[0].shape[-1]
    if out is not None:
        if not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise ValueError(f"{who}: out must be the pair (sums, weight) of an earlier call")
        _check_table(who, "out[0]", out[0], (n, ch), dev, MAX_CHANNELS - 1)
        _check_table(who, "out[1]", out[1].unsqueeze(-1) if isinstance(out[1], torch.Tensor) and out[1].dim() == 1 else out[1], (n, 1), dev, 1)
    _need_gpu(who, "maps" if isinstance(maps, torch.Tensor) else "maps[0]", maps if isinstance(maps, torch.Tensor) else maps[0])
    cams = ops._convert_cameras(c2ws, dev)
    front, held = _front(spec, geometry, n, dev)
    table = torch.zeros((n, ch + 1), dtype=torch.float32, device=dev)          # (sums | weight): one table, one launch sequence per pose
    for c2w, m in zip(cams, maps):
        fr = front.frame(c2w) if n else None
        if fr is None:
            continue
        g = torch.cat([m, torch.ones((spec.H, spec.W, 1), dtype=torch.float32, device=dev)], dim=-1)
        _call("gsplat_features_adjoint", front, fr, g, ch + 1, table, front.st)
    if out is None:
        return table[:, :ch].contiguous(), table[:, ch].contiguous()
    out[0].add_(table[:, :ch])
    out[1].add_(table[:, ch])
    return out[0], out[1]
