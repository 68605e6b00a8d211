"""PyTorch-ROCm host side of the hot path: autograd surface over the C ABI (ctypes, raw device pointers).

Mirrors the reference's operator interface (same names, argument meaning, defaults and error behaviour):

    render(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, near=0.01, far=100.0, pix_guard=32, T=16,
           min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1/128.)      reference render.py:62-64
           (+ keyword-only aux=False, background=None: depth and opacity maps, a background colour -- not in the reference)
    build_sigma_from_params(scale_raw, q_raw)                                               reference gaussian.py:71
    evaluate_sh(f_dc, f_rest, points, c2w)                                   reference spherical_harmonics.py:70

plus the fused entry `render_gaussians(...)`, which takes the six raw parameter tensors and folds the covariance build
and the SH evaluation into the projection kernel (the Sigma[N,3,3] and colour[N,3] tensors are never materialised); its
keyword sh_degree (0..3, default 3) renders with the first (sh_degree + 1)^2 SH bases only.  Every render entry
takes the keywords lowpass=0.0, antialias=False: the screen-space low-pass of the paper's rasteriser and the opacity compensation of
its antialiased variant.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); all arithmetic runs in the HIP library.
There is no CPU path: CPU tensors, or a missing library, raise.

The render entries turn their arguments into ONE immutable FrameSpec (_frame_spec: camera, mode, input names), which the forward
pass keeps on the frame (_Frame.spec) for the backward pass; the facts of one autograd call (pose, need_grad, route) lie beside it.

This file holds the frame (spec, forward halves, backward pass, gradient routes, public entries) and the switches that tests and tools
assign (_composite, _sh_jacobian, _deterministic: read here only, at call time).  What outlives a frame lives in modules that never
import this one -- _dev, _timing, _workspace, records -- and is re-exported here under the names it always had.
"""
import contextlib
import contextvars
import ctypes as C
import dataclasses

import torch

from . import _abi, _timing
from ._dev import _f32, _launch, _p, _stream_ptr  # noqa: F401
from ._timing import StageTimer, _stage, set_stage_timer  # noqa: F401
from ._workspace import (OFFSCREEN_MSG, PINNED_SLOTS, DeferredChecks, PairCapacityExceeded, _deferred_stack, _note_counts, _Unread,  # noqa: F401
                         _Workspace, _ws, binned_pairs, capacity_key, deferred_checks, forward_modes, read_counts, render_stats, reset_pair_capacity, run_deferred)
from .records import (ContributionStats, DensifyStats, VisibleSet, _stats, _stats_absgrad, _visible, absgrad_calls, add_frame_records,  # noqa: F401
                      densify_stats, frame_records, visible_set)

composite_calls = {"forward": 0, "backward": 0}  # passes queued through ONE library call (gsplat_forward_deferred / gsplat_backward)

_sh_jacobian = True      # tests / ablations switch it off: the backward then reads the SH coefficients again (same gradients)
_composite = True        # tests / ablations switch it off: a deferred frame then goes through the separate library calls
_FUSED_NAMES = ("pos", "opacity_raw", "scale_raw", "q_raw", "f_dc", "f_rest")
_PLAIN_NAMES = ("pos", "opacity_raw", "color", "sigma")
_ROW_SHAPE = dict(pos=(3,), color=(3,), sigma=(3, 3), scale_raw=(3,), q_raw=(4,), f_dc=(3,), f_rest=(45,))      # per Gaussian
_SH = ("f_dc", "f_rest")
_GRAD_FIELDS = tuple(name for name, _ in _abi.GaussianGrads._fields_)
_INPUT_FIELDS = tuple(name for name, _ in _abi.Gaussians._fields_[1:])        # (behind n: one address per input, NULL where the entry has none)


@dataclasses.dataclass(frozen=True, eq=False)
class FrameSpec:
    """The render mode of one public call: built once, by _frame_spec(), and never changed -- the forward pass, the frame and every
    backward route read the same object, so they cannot disagree.  `view` carries the C fields only."""
    __slots__ = ("view", "fused", "grad_mode", "aux", "background", "sh_degree", "filter", "names")
    view: _abi.View
    fused: bool            # render_gaussians / render_frames (six raw parameter tensors) or render (colour and Sigma given)
    grad_mode: bool        # torch.is_grad_enabled() of the caller (the autograd node's forward() always runs with grad disabled)
    aux: bool              # the call also returns the depth and the opacity map
    background: tuple      # (r, g, b) the image is composited over, or None
    sh_degree: int         # of the forward pass; 3 when not fused
    filter: int            # the GSPLAT_FILTER_* bits (lowpass, antialias): the same bits in the flags of every projection entry
    names: tuple           # the tensor inputs of the entry, in the order _RenderFn takes them and returns their gradients
    H = property(lambda self: self.view.H)
    W = property(lambda self: self.view.W)
    is_aux = property(lambda self: self.aux or self.background is not None)      # the aux variant of the raster kernels

    def __eq__(self, other):                           # (a ctypes structure compares by identity: compare the camera's bytes)
        key = lambda s: (bytes(s.view),) + tuple(getattr(s, k) for k in FrameSpec.__slots__[1:])
        return isinstance(other, FrameSpec) and key(self) == key(other)


def _frame_spec(fused, H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff, *,
                aux=False, background=None, sh_degree=3, lowpass=0.0, antialias=False):
    """The FrameSpec of a public call, for all three entries; every bad mode argument is refused here (ValueError), in one order: SH
    degree (fused entries), filter, T, background.  Needs no GPU and queues nothing."""
    if fused:
        _abi.sh_bands_dropped(sh_degree)
    bits = _abi.filter_bits(lowpass, antialias)
    # every T of the reference is accepted: the image does not depend on it; T only sets the reference's
    # tile rectangles, i.e. the reported pair count P.  The kernels always bin 16 x 8-pixel lists.
    if int(T) < 1:
        raise ValueError("tile size T must be >= 1")
    # H, W may arrive as 0-d tensors from DataLoader collate (reference scripts/train.py:499)
    view = _abi.make_view(H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff)
    if background is not None:             # a constant (3 numbers, a sequence or a tensor): it gets no gradient
        vals = background.detach().reshape(-1).tolist() if isinstance(background, torch.Tensor) else list(background)
        if len(vals) != 3:
            raise ValueError("background must hold 3 numbers (r, g, b)")
        background = tuple(float(x) for x in vals)
    return FrameSpec(view, fused, torch.is_grad_enabled(), bool(aux), background, sh_degree if fused else 3, bits,
                     _FUSED_NAMES if fused else _PLAIN_NAMES)


class _Frame:
    """Everything the backward pass needs from one forward call: the call's FrameSpec (`spec`: camera and mode), the converted inputs
    by name, and the facts of this autograd call -- `need_grad`, `pose` (the backward also forms dL/dc2w), `stats` (the
    densify_stats() record, if any; `absgrad`: its mode; `visible`: the visible_set() record, if any) and the gradient route (`route`, `route_kind`: _route_of).  A frame queued by
    gsplat_forward_deferred keeps ONE arena (project_state | bin_state | accum | grad2d, carved by the library); one that went
    through the separate calls keeps them as separate buffers."""
    __slots__ = ("spec", "n", "n_pairs", "proj_state", "bin_state", "accum", "inputs", "c2w", "empty", "grad2d", "sh_jacobian", "arena",
                 "gaussians", "dirty", "src_ptrs", "route", "route_kind", "pose", "need_grad", "accum_aux", "stats", "absgrad", "visible")


def _forward_begin(spec, c2w, tensors, pose=False, need_grad=False):
    """First half of the forward pass of `tensors` ({name: tensor} for spec.names): everything up to (not including) the host's wait
    for the counters.  Returns (pending, None), or (None, (result, frame, counts)) when nothing is left to do: zero Gaussians, or --
    inside a deferred_checks() block once a pair capacity is known for this image size -- the whole forward pass was queued by ONE
    library call (gsplat_forward_deferred) and the result is there.  The result is always (image, depth, alpha), the maps None where
    the frame has none (_deliver turns it into what the caller gets).  pose (from _RenderFn): the backward pass will also form
    dL/dc2w -- a pose frame: always the separate library calls, and no gradient route but the factored exchange.  spec.is_aux: an aux frame -- depth and
    opacity maps, or an image over a background -- which takes the separate library calls like a pose frame."""
    route = _route.get()
    # (the factored exchange takes a pose frame as it takes an aux frame, below: the separate calls, gsplat_logit_grad -> route.add,
    #  then gsplat_project_backward_pose with the SH-less destination -- the kernel's factored branches do not depend on the pose)
    if pose and route is not None and route.route_kind != FACTORED:
        raise RuntimeError("a camera-pose gradient (c2w.requires_grad) is not available inside a gradient_route() block "
                           "(factored exchange, folded f_rest step, accumulate_grads): render the pose frame outside it")
    auxf = spec.is_aux
    # (the factored exchange takes an aux frame: it goes through the separate calls, whose backward forms the logit gradients from
    #  grad2d whatever filled it; the other two routes live on the composite entries, which have no aux variant)
    if auxf and route is not None and route.route_kind != FACTORED:
        raise RuntimeError("depth / opacity maps and a background (aux=True, background=...) are not available inside a gradient_route() "
                           "block (factored exchange, folded f_rest step, accumulate_grads): render the frame outside it")
    pos = tensors["pos"]
    dev, n, view = pos.device, pos.shape[0], spec.view
    fr = _Frame()
    # (the records are checked before anything else: a wrong one is refused even where nothing is rendered)
    fr.stats, fr.absgrad, fr.visible = frame_records(pos, need_grad)
    fr.spec, fr.pose, fr.need_grad, fr.n = spec, pose, need_grad, n
    fr.route, fr.route_kind = None, PLAIN       # (until _route_of finds a consumer for this frame)
    fr.inputs, g = _convert_inputs(spec.names, tensors, n)
    c2w32 = fr.c2w = _f32(c2w, (4, 4), "c2w")
    fr.arena = fr.gaussians = fr.proj_state = fr.bin_state = fr.accum = fr.grad2d = fr.accum_aux = None
    fr.empty = fr.sh_jacobian = fr.dirty = False
    # the caller's own SH tensors (before any dtype / layout conversion): what dp.FactoredExchange.owns() compares
    fr.src_ptrs = (tensors["f_dc"].data_ptr(), tensors["f_rest"].data_ptr()) if spec.fused else None
    if n == 0:      # nothing survives by construction: the reference returns the zero image (render.py:109-112)
        fr.empty = True
        _route_of(fr, False)
        return None, (_empty_result(spec, dev), fr, _abi.Counts(0, 0, 0, 0, 0, 0))
    fr.gaussians = g                            # (addresses of fr.inputs, which the frame keeps)
    ckey = capacity_key(dev, spec, n)
    capacity = _ws.pair_capacity(ckey) if _deferred_stack else 0
    deferred = capacity > 0
    _, key, st = _stream_key(dev)               # looked up ONCE per forward pass
    fr.sh_jacobian = bool(spec.fused and need_grad and _sh_jacobian)   # 48 bytes per Gaussian that spare the backward the 192 bytes of SH coefficients
    chk = _deferred_stack[-1] if deferred else None
    composite = deferred and _composite and not _timing.wants(_FORWARD_STAGES) and not pose and not auxf
    _route_of(fr, composite)
    lib = _abi.lib()
    if composite:
        # ---- the whole forward pass in one call, on one arena
        counters, pinned, slot, ready = _ws.counter_set(dev, key, chk, True)
        flags = (_abi.GSPLAT_FRAME_BACKWARD if need_grad else 0) | (0 if _sh_jacobian else _abi.GSPLAT_FRAME_NO_SH_JACOBIAN)
        frame_bytes, scratch_bytes = _ws.frame_sizes(lib, n, capacity, view, flags)
        flags |= _FRAME_DEGREE[spec.sh_degree] | spec.filter
        fr.arena, fr.n_pairs = torch.empty(frame_bytes, dtype=torch.uint8, device=dev), capacity
        image = torch.empty((spec.H, spec.W, 3), dtype=torch.float32, device=dev)
        scratch = _ws.get_scratch(dev, scratch_bytes, key)
        _abi.check(lib.gsplat_forward_deferred(g, c2w32.data_ptr(), view, fr.arena.data_ptr(), frame_bytes, capacity, counters.data_ptr(),
                                               counters.numel(), scratch.data_ptr(), scratch.numel(), pinned.data_ptr(), ready.cuda_event,
                                               image.data_ptr(), flags, st), "gsplat_forward_deferred")
        forward_modes["deferred"] += 1
        composite_calls["forward"] += 1
        chk.add(pinned, ready, capacity, dev, ckey, (key, slot))
        return None, ((image, None, None), fr, None)
    fr.proj_state = torch.empty(lib.gsplat_project_state_bytes(n, C.byref(view)), dtype=torch.uint8, device=dev)
    # a frame that will not wait for its counters evaluates the SH colour inside the projection kernel and lets the first binning
    # kernel total the counters (the projection's waves then retire without waiting for their stores)
    flags = (_abi.GSPLAT_PROJECT_COLOUR_FUSED | _abi.GSPLAT_PROJECT_COUNTS_LATE) if deferred else 0
    if fr.sh_jacobian:
        flags |= _abi.GSPLAT_PROJECT_SAVE_SH_JACOBIAN
    flags |= _PROJECT_DEGREE[spec.sh_degree] | spec.filter
    pinned, slot, ready = _queue_project(g, c2w32, view, fr.proj_state, flags, dev, key, st, chk, deferred)
    return (fr, _Unread(pinned, ready, capacity if deferred else None, dev, ckey, (key, slot))), None


# ---- the front end of a frame, shared by the forward pass and contribution(): convert, project, (read_counts,) bin.  The pieces take
# the ring key and the stream handle of _stream_key(), which their caller looks up once.

def _convert_inputs(names, tensors, n):
    """(inputs by name in fp32, the C struct of their addresses -- the caller keeps the former alive) of the entry's inputs `names`."""
    opa = tensors["opacity_raw"]
    ins = dict(pos=_f32(tensors["pos"], (n, 3), "pos"), opacity_raw=_f32(opa if opa.dim() == 1 else opa.reshape(-1), (n,), "opacity_raw"))
    for name in names[2:]:
        ins[name] = _f32(tensors[name], (n,) + _ROW_SHAPE[name], name)
    return ins, _abi.Gaussians(n, *map(_p, map(ins.get, _INPUT_FIELDS)))


def _stream_key(dev):
    """(stream, key, st) of the current stream of `dev`, made the current device: the key of the workspace's per-stream buffers and the
    handle the library takes.  Looking the stream up is the costliest thing a pass does on the host: once per pass and direction."""
    if torch.cuda.current_device() != dev.index:
        torch.cuda.set_device(dev)            # (a context manager per call costs more than the call: the one-process-per-GPU host never switches)
    stream = torch.cuda.current_stream(dev)
    return stream, (dev.type, dev.index, stream.cuda_stream), C.c_void_p(stream.cuda_stream)


def _queue_project(g, c2w32, view, proj_state, flags, dev, key, st, owner=None, fresh_event=False):
    """Queue gsplat_project; returns (pinned, slot, ready): the counters go straight into the pinned block (mapped into the device's
    address space: no copy operation), and `ready` is recorded behind them."""
    counters, pinned, slot, ready = _ws.counter_set(dev, key, owner, fresh_event)
    with _stage("project"):
        _abi.check(_abi.lib().gsplat_project(C.byref(g), _p(c2w32), C.byref(view), _p(proj_state), _p(counters), counters.numel(),
                                             C.c_void_p(pinned.data_ptr()), C.c_void_p(ready.cuda_event),
                                             flags | _abi.GSPLAT_PROJECT_COUNTS_MAPPED, st), "gsplat_project")
    return pinned, slot, ready


def _queue_bin(n, pairs, view, proj_state, dev, key, st):
    """Queue gsplat_bin of `pairs` pairs; returns the frame's bin_state (the scratch is the stream's own)."""
    lib = _abi.lib()
    bin_state = torch.empty(lib.gsplat_bin_state_bytes(pairs, C.byref(view)), dtype=torch.uint8, device=dev)
    scratch = _ws.get_scratch(dev, lib.gsplat_bin_scratch_bytes(pairs, C.byref(view)), key)
    with _stage("bin"):
        _abi.check(lib.gsplat_bin(n, pairs, C.byref(view), _p(proj_state), _p(bin_state), _p(scratch), scratch.numel(), st), "gsplat_bin")
    return bin_state


def _convert_cameras(c2ws, dev):
    """The poses `c2ws` (tensors, or what torch.as_tensor takes) as fp32 [4, 4] on `dev`."""
    return [_f32(c if isinstance(c, torch.Tensor) else torch.as_tensor(c, dtype=torch.float32, device=dev), (4, 4), "c2w") for c in c2ws]


class _WaitedFront:
    """The waited front end of contribution() and features.render / lift, for one model `g` (n > 0; the caller keeps its tensors): one
    project_state for all poses, the current stream looked up once.  frame(c2w) queues project, waits for the pair count, bins with
    exact buffers: (pairs, bin_state), None for a pose without a survivor, the reference's off-screen Exception for survivors none of
    which is on screen.  `proj_state`, `view`, `st`: for the caller's own library call.  (Not _forward_end's waited branch, which
    drains the deferred block between reading the counters and raising.)"""

    def __init__(self, spec, g, n, dev, flags):
        self.g, self.n, self.dev, self.flags, self.view = g, n, dev, flags, spec.view
        _, self.key, self.st = _stream_key(dev)
        self.proj_state = torch.empty(_abi.lib().gsplat_project_state_bytes(n, C.byref(self.view)), dtype=torch.uint8, device=dev)
        self.ckey = capacity_key(dev, spec, n)

    def frame(self, c2w):
        pinned, _, ready = _queue_project(self.g, c2w, self.view, self.proj_state, self.flags, self.dev, self.key, self.st)
        ready.synchronize()                      # the one host wait of a frame: the pair count sizes the binning buffers
        counts, scene = read_counts(pinned, self.ckey)
        if scene == _abi.GSPLAT_SCENE_ALL_OFFSCREEN:
            raise Exception(OFFSCREEN_MSG)
        if scene == _abi.GSPLAT_SCENE_ALL_CULLED:
            return None
        pairs = int(counts.n_binned)
        return pairs, _queue_bin(self.n, pairs, self.view, self.proj_state, self.dev, self.key, self.st)


def _empty_result(spec, dev):
    """(image, depth, alpha) of a frame without a survivor: the zero image -- the clamped background where one is given -- and zero
    maps (None without aux=True)."""
    H, W = spec.H, spec.W
    if spec.background is None:
        image = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    else:
        image = torch.tensor(spec.background, dtype=torch.float32, device=dev).clamp_(0.0, 1.0).expand(H, W, 3).contiguous()
    if not spec.aux:
        return image, None, None
    return image, torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.float32, device=dev)


def _deliver(spec, result, dtype=torch.float32):
    """The one place the (image, depth, alpha) of the forward pass becomes what the caller gets: the image, or the triple with
    aux=True (in `dtype`, the caller's)."""
    out = tuple(t if t is None or t.dtype == dtype else t.to(dtype) for t in result)
    return out if spec.aux else out[0]


def _background_arg(background):
    """The 3 host floats the aux entries read during the call (NULL = no background)."""
    return (C.c_float * 3)(*background) if background is not None else None


# the flag bits of an SH degree, per entry family (index = degree; 0 for degree 3)
_PROJECT_DEGREE = tuple(_abi.GSPLAT_PROJECT_SH_DEGREE(d) for d in range(4))
_FRAME_DEGREE = tuple(_abi.GSPLAT_FRAME_SH_DEGREE(d) for d in range(4))
_BACKWARD_DEGREE = tuple(_abi.GSPLAT_BACKWARD_SH_DEGREE(d) for d in range(4))
_FORWARD_STAGES = frozenset(("project", "bin", "raster_forward"))
_BACKWARD_STAGES = frozenset(("raster_backward", "project_backward"))


def _forward_end(fr, unread):
    """Second half, of a call between its halves (projection queued, counters `unread`): wait for the counters, size the pair
    buffers, bin, rasterise.  Must run with the same current stream as the first half.  Returns ((image, depth, alpha), frame, counts)."""
    lib = _abi.lib()
    spec, n, need_grad, dev = fr.spec, fr.n, fr.need_grad, unread.device
    view, H, W = spec.view, spec.H, spec.W
    key = unread.slot[0]                         # (device, stream) of the first half: the same current stream is the caller's contract
    st = C.c_void_p(key[2])
    # the one host wait of the forward pass: the pair count sizes the binning buffers, and the reference's empty /
    # off-screen conventions need the survivor counts.  Only the counters are waited for: the first binning kernel and
    # (fused inputs) the SH colour pass are queued behind them and run during this round trip.
    if unread.capacity is not None:
        # deferred: no wait.  Buffers of the capacity kept from earlier frames; the kernels read the real count on the
        # device; the host looks at the counters in DeferredChecks.verify()
        counts = None
        fr.n_pairs = int(unread.capacity)
        forward_modes["deferred"] += 1
        _deferred_stack[-1].add(*unread)
    else:
        unread.event.synchronize()
        forward_modes["waited"] += 1
        counts, scene = read_counts(unread.pinned, unread.ckey)
        if _deferred_stack:                      # a frame that had to wait inside a deferred block (first of its size): verify() still
            chk = _deferred_stack[-1]            # returns one entry per frame, in frame order (the earlier frames are done by now)
            chk._drain(len(chk.pending))
            chk.counts.append(counts)
        if scene == _abi.GSPLAT_SCENE_ALL_OFFSCREEN:
            raise Exception(OFFSCREEN_MSG)
        if scene == _abi.GSPLAT_SCENE_ALL_CULLED:
            fr.empty = True
            fr.proj_state = None
            return _empty_result(spec, dev), fr, counts
        fr.n_pairs = int(counts.n_binned)        # pairs actually binned (16 x 8 lists); counts.n_pairs = the reference's P
    image = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    fr.bin_state = _queue_bin(n, fr.n_pairs, view, fr.proj_state, dev, key, st)
    fr.accum = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if need_grad else None
    # the forward rasterizer clears the backward's accumulation buffer on the side (its waves are VALU-bound), unless
    # there are so few lists that a wave's share would be long
    lists = ((W + 15) // 16) * ((H + 7) // 8)
    fr.grad2d = torch.empty((n, 16), dtype=torch.float32, device=dev) if need_grad and n <= 256 * lists else None
    depth = alpha = None
    if spec.is_aux:
        # depth and opacity beside the colour (and the colour over the background): the aux variant of the raster kernel
        if spec.aux:
            depth, alpha = (torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2))
        fr.accum_aux = torch.empty((H, W, 2), dtype=torch.float32, device=dev) if need_grad else None
        with _stage("raster_forward"):
            _abi.check(lib.gsplat_rasterize_forward_aux(n, fr.n_pairs, C.byref(view), _p(fr.proj_state), _p(fr.bin_state), _p(image),
                                                        _p(depth), _p(alpha), _p(fr.accum), _p(fr.accum_aux), _p(fr.grad2d),
                                                        _background_arg(spec.background), st), "gsplat_rasterize_forward_aux")
    else:
        with _stage("raster_forward"):
            _abi.check(lib.gsplat_rasterize_forward(n, fr.n_pairs, C.byref(view), _p(fr.proj_state), _p(fr.bin_state),
                                                    _p(image), _p(fr.accum), _p(fr.grad2d), st), "gsplat_rasterize_forward")
    return (image, depth, alpha), fr, counts


def _forward_impl(spec, c2w, tensors, pose, need_grad):
    pend, done = _forward_begin(spec, c2w, tensors, pose, need_grad)
    return done if pend is None else _forward_end(*pend)


def _flat_like(ins):
    """One flat fp32 buffer holding a gradient for every input (each view 256-byte aligned inside it).  The data-parallel
    helper recognises the shared base and all-reduces the six gradients with ONE in-place collective, no flatten copy."""
    sizes = [(v.numel() + 63) // 64 * 64 for v in ins.values()]
    any_in = next(iter(ins.values()))
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=any_in.device)
    parts = flat.split(sizes)                                   # one call for all the pieces
    return {k: (piece if piece.numel() == v.numel() else piece[:v.numel()]).view(v.shape) for (k, v), piece in zip(ins.items(), parts)}


_deterministic = False


def set_deterministic(flag=True):
    """Bitwise reproducible gradients: the raster backward stores its per-(list, Gaussian) sums and adds them per Gaussian in a
    fixed order instead of using float atomics (whose order of arrival changes the last bits from run to run).  Slower by the
    cost of a 36-byte row per pair written and read once.  Returns the previous setting."""
    global _deterministic
    old, _deterministic = _deterministic, bool(flag)
    return old


class GradAccumulation:
    """with ops.accumulate_grads(params) as acc: ... several render(...).backward() ...; acc.assign()

    The gradients of the views of ONE iteration are summed by the projection backward itself (GSPLAT_BACKWARD_ACCUMULATE) in one flat
    buffer: the first view writes, the others add -- instead of autograd's AccumulateGrad pass per view (read two, write one: 0.4 ms
    per view at 3 M Gaussians).  `params`: dict name -> the leaf tensors the renders are called with (fp32, contiguous, .grad None).
    A render of other tensors, a frame that waited for its counters or a timed pass keep the ordinary backward.  assign()
    sets param.grad (views of the buffer) -- summing in what the ordinary backward may have produced for some views."""

    NAMES = _FUSED_NAMES
    route_kind = "summed"

    def __init__(self, params):
        self.params = {k: params[k] for k in self.NAMES}
        self.buffers = None
        self.count = 0
        self.event = None
        self.ptrs = {k: v.data_ptr() for k, v in self.params.items()}

    def matches(self, ins):
        return all(k in ins and ins[k].data_ptr() == self.ptrs[k] for k in self.NAMES)

    def begin(self, stream):
        """(buffers, accumulate?) for the next backward pass, ordered behind the previous one whatever stream that ran on."""
        if self.buffers is None:
            self.buffers = _flat_like({k: self.params[k] for k in self.NAMES})
        if self.event is not None:
            stream.wait_event(self.event)
        return self.buffers, self.count > 0

    def done(self, stream):
        self.count += 1
        if self.event is None:
            self.event = torch.cuda.Event(enable_timing=False)
        self.event.record(stream)

    def assign(self):
        if self.count == 0:
            return
        stream = torch.cuda.current_stream(self.params["pos"].device)
        stream.wait_event(self.event)
        for k, p in self.params.items():
            g = self.buffers[k]
            g.record_stream(stream)
            p.grad = g if p.grad is None else p.grad.add_(g)


def accumulate_grads(params):
    return gradient_route(GradAccumulation(params))


# The route of a frame's gradients: at most one consumer takes them in place of autograd's .grad, for the frames rendered inside
# its gradient_route() block.  A consumer names its kind (`route_kind`): dp.FactoredExchange is FACTORED (data parallel: 3 colour-logit
# gradients per Gaussian instead of 48 SH ones), GradAccumulation SUMMED (the views of an iteration summed by the
# backward), optim._RestUpdate FOLDED (the Adam step of f_rest inside the backward).  The slot is read once, in the caller's thread,
# when a frame is rendered (_route_of): the backward pass, on autograd's thread, reads fr.route and fr.route_kind only.
_route = contextvars.ContextVar("gsplat_gradient_route", default=None)
PLAIN, FACTORED, SUMMED, FOLDED = "plain", "factored", "summed", "folded"       # PLAIN: no consumer, autograd gets every gradient


@contextlib.contextmanager
def gradient_route(consumer):
    if _route.get() is not None:
        raise RuntimeError("a gradient route is already active: routes do not nest")
    token = _route.set(consumer)
    try:
        yield consumer
    finally:
        _route.reset(token)


def _route_of(fr, composite):
    """Decide, once, where the gradients of a frame go (composite: queued by gsplat_forward_deferred): fr.route = the active route's
    consumer and fr.route_kind = its kind if it takes them, else (None, PLAIN)."""
    r = _route.get()
    if r is None or not (fr.need_grad and fr.spec.fused):
        return
    kind = r.route_kind
    if kind == FACTORED:
        takes = r.owns(fr.inputs, fr.src_ptrs)
    else:                                             # the other two routes live on the composite entries and the saved Jacobian
        takes = composite and fr.sh_jacobian and (r.matches(fr.inputs) if kind == SUMMED else r.matches(fr.inputs["f_rest"], fr.src_ptrs[1]))
    if takes:
        fr.route, fr.route_kind = r, kind


# the raster backward of a frame: (aux variant?, absolute-gradient statistics? -- rows of 11 / 12) -> (entry, its scratch-size entry)
_RASTER_BACKWARD = {(aux, absgrad): (name, name + "_scratch_bytes") for aux in (False, True) for absgrad in (False, True)
                    for name in ["gsplat_rasterize_backward" + "_aux" * aux + "_abs" * absgrad]}


class _BackwardPass:
    """What _backward_impl prepares for either call sequence: the route kind of THIS pass, timed pass?, fp32 grad_image, the stream and
    its handle, deterministic scratch, destination buffers (dict and C struct), SUMMED: add to them?, flag bits of the projection backward."""
    __slots__ = ("kind", "staged", "gi", "stream", "st", "det", "dst", "gg", "add", "jac")


def _backward_impl(fr, grad_image, need_params=True, grad_depth=None, grad_alpha=None):
    """Returns a dict name -> fp32 gradient tensor of the inputs of the forward call (a missing name: fr.route took that gradient);
    a pose frame adds "c2w" (fp32 [4, 4]).  need_params = False (pose frames): only the pose gradient is wanted.  An aux frame:
    grad_image, grad_depth, grad_alpha are the upstream gradients of its three outputs, None where the loss does not read one.
    Here: the prologue that the two call sequences share."""
    spec, ins = fr.spec, fr.inputs
    if fr.empty or fr.n == 0 or (spec.is_aux and grad_image is None and grad_depth is None and grad_alpha is None):
        return _backward_empty(fr)
    dev = ins["pos"].device
    bp = _BackwardPass()
    bp.gi = _f32(grad_image, (spec.H, spec.W, 3), "grad_image") if grad_image is not None else None
    stream, key, bp.st = _stream_key(dev)
    bp.stream, bp.det = stream, None
    if _deterministic:
        det_bytes = getattr(_abi.lib(), _RASTER_BACKWARD[spec.is_aux, fr.absgrad][1])
        bp.det = _ws.get_scratch(dev, det_bytes(fr.n, fr.n_pairs), key)
    staged = bp.staged = _timing.wants(_BACKWARD_STAGES)
    # only known now, each sending the frame down the ordinary backward: a timed pass (phase by phase), a second pass through the
    # frame (views' sum), a step of f_rest already applied (folded step)
    kind = fr.route_kind
    if kind == SUMMED and (staged or fr.dirty) or kind == FOLDED and (staged or fr.route.applied):
        kind = PLAIN
    bp.kind, bp.add = kind, False
    if kind == SUMMED:
        bp.dst, bp.add = fr.route.begin(stream)
    elif fr.pose and not need_params:
        bp.dst = {}
    else:
        bp.dst = _flat_like({k: v for k, v in ins.items() if not (kind == FACTORED and k in _SH or kind == FOLDED and k == "f_rest")})
    bp.gg = _abi.GaussianGrads(*map(_p, map(bp.dst.get, _GRAD_FIELDS)))
    # (`jac` goes into the flags of every projection backward: the saved Jacobian, the degree and the filter of the frame's forward pass)
    bp.jac = (_abi.GSPLAT_BACKWARD_SH_JACOBIAN if fr.sh_jacobian else 0) | _BACKWARD_DEGREE[spec.sh_degree] | spec.filter
    if fr.arena is None:
        return _backward_separate(fr, bp, grad_depth, grad_alpha, need_params)
    return _backward_arena(fr, bp)


def _backward_empty(fr):
    """A frame without a survivor, or an aux frame none of whose outputs the loss reads: zero gradients, nothing queued but them."""
    dev = fr.inputs["pos"].device
    factored = fr.route_kind == FACTORED
    if factored:
        fr.route.add(torch.zeros((fr.n, 3), dtype=torch.float32, device=dev), fr.c2w[:3, 3], fr.spec.sh_degree)
    out = {k: torch.zeros_like(v) for k, v in fr.inputs.items() if not (factored and k in _SH)}
    if fr.pose:
        out["c2w"] = torch.zeros((4, 4), dtype=torch.float32, device=dev)
    return out


def _backward_separate(fr, bp, grad_depth, grad_alpha, need_params):
    """The frame went through the separate calls (waited, timed, pose and aux frames): raster backward, statistics, logit gradients
    for a factored exchange, projection backward.  Its route is FACTORED or PLAIN."""
    lib = _abi.lib()
    spec, dst, gg, jac, st, det = fr.spec, bp.dst, bp.gg, bp.jac, bp.st, bp.det
    view, dev = spec.view, fr.inputs["pos"].device
    zeroed = fr.grad2d is not None
    grad2d = fr.grad2d if zeroed else torch.empty((fr.n, 16), dtype=torch.float32, device=dev)
    fr.grad2d = None                       # a second backward through the same graph must not reuse a dirty buffer
    gd = _f32(grad_depth, (spec.H, spec.W), "grad_depth") if grad_depth is not None else None
    ga = _f32(grad_alpha, (spec.H, spec.W), "grad_alpha") if grad_alpha is not None else None
    name = _RASTER_BACKWARD[spec.is_aux, fr.absgrad][0]
    if spec.is_aux:
        # (z, 1) as two more colour channels; column 9 of grad2d = dL/dz, which the projection backward picks up (DEPTH)
        upstream = (_p(fr.accum_aux), _p(bp.gi), _p(gd), _p(ga), _background_arg(spec.background))
        jac |= _abi.GSPLAT_BACKWARD_DEPTH
    else:
        upstream = (_p(bp.gi),)
    with _stage("raster_backward"):
        _abi.check(getattr(lib, name)(fr.n, fr.n_pairs, C.byref(view), _p(fr.proj_state), _p(fr.bin_state), _p(fr.accum), *upstream,
                                      _p(grad2d), int(zeroed), _p(det), det.numel() if det is not None else 0, st), name)
    add_frame_records(fr, st, grad2d)
    if bp.kind == FACTORED:
        # logit gradients first: the exchange may start on them while the projection backward runs
        glogit = torch.empty((fr.n, 3), dtype=torch.float32, device=dev)
        _abi.check(lib.gsplat_logit_grad(fr.n, C.byref(view), _p(fr.proj_state), _p(grad2d), _p(glogit), st), "gsplat_logit_grad")
        fr.route.add(glogit, fr.c2w[:3, 3], spec.sh_degree)
    if fr.pose:
        # the same chain rule plus dL/dc2w: per-block rows of the pose terms, added in a fixed order (no gradient rows if
        # nothing but the pose is wanted)
        gc2w = torch.empty((4, 4), dtype=torch.float32, device=dev)
        nbytes = lib.gsplat_pose_scratch_bytes(fr.n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _stage("project_backward"):
            _abi.check(lib.gsplat_project_backward_pose(C.byref(fr.gaussians), _p(fr.c2w), C.byref(view), _p(fr.proj_state), _p(grad2d),
                                                        C.byref(gg) if need_params else None, _p(gc2w), _p(scratch), nbytes, jac,
                                                        st), "gsplat_project_backward_pose")
        return dict(dst, c2w=gc2w)
    with _stage("project_backward"):
        _abi.check(lib.gsplat_project_backward(C.byref(fr.gaussians), _p(fr.c2w), C.byref(view), _p(fr.proj_state), _p(grad2d),
                                               C.byref(gg), jac, st), "gsplat_project_backward")
    return dst


def _backward_call(fr, bp, flags, det=None, glogit=None, rest=None):
    """gsplat_backward on the frame's arena, or gsplat_backward_adam_rest with rest = (AdamGroup, beta1, beta2, eps)."""
    lib = _abi.lib()
    args = (fr.gaussians, fr.c2w.data_ptr(), fr.spec.view, fr.arena.data_ptr(), fr.arena.numel(), fr.n_pairs, bp.gi.data_ptr(), bp.gg)
    scratch = (det.data_ptr(), det.numel()) if det is not None else (None, 0)
    if rest is None:
        _abi.check(lib.gsplat_backward(*args, _p(glogit), *scratch, flags, bp.st), "gsplat_backward")
    else:
        group, b1, b2, eps = rest
        _abi.check(lib.gsplat_backward_adam_rest(*args, *scratch, flags, C.byref(group), b1, b2, eps, bp.st), "gsplat_backward_adam_rest")


def _backward_arena(fr, bp):
    """The frame was queued by gsplat_forward_deferred: one call for the whole backward pass (two, phase by phase, for a factored
    exchange or a timed pass)."""
    kind, route, jac, det = bp.kind, fr.route, bp.jac, bp.det
    flags = jac | (_abi.GSPLAT_BACKWARD_GRAD2D_DIRTY if fr.dirty else 0) | (_abi.GSPLAT_BACKWARD_ABSGRAD if fr.absgrad else 0)
    fr.dirty = True                            # a second backward through the same graph must not reuse a dirty buffer
    if kind == FACTORED or bp.staged:
        glogit = torch.empty((fr.n, 3), dtype=torch.float32, device=fr.arena.device) if kind == FACTORED else None
        with _stage("raster_backward"):
            _backward_call(fr, bp, flags | _abi.GSPLAT_BACKWARD_PHASE_RASTER, det, glogit)
        if kind == FACTORED:                   # logit gradients first: the exchange may start on them while the projection backward runs
            route.add(glogit, fr.c2w[:3, 3], fr.spec.sh_degree)
        add_frame_records(fr, bp.st)
        with _stage("project_backward"):
            _backward_call(fr, bp, jac | _abi.GSPLAT_BACKWARD_PHASE_PROJECT)
    else:
        if kind == SUMMED:
            # the views of an iteration summed in the accumulation's own buffer by the projection backward: autograd gets no gradient
            _backward_call(fr, bp, flags | (_abi.GSPLAT_BACKWARD_ACCUMULATE if bp.add else 0), det)
            route.done(bp.stream)
        elif kind == FOLDED:
            # the Adam step of f_rest inside the projection backward: its 192 bytes of gradient per Gaussian are never written
            _backward_call(fr, bp, flags, det, rest=route.begin())
            route.commit()
        else:
            _backward_call(fr, bp, flags, det)
        add_frame_records(fr, bp.st)           # (the projection phase only reads grad2d)
    composite_calls["backward"] += 1
    return {} if kind == SUMMED else bp.dst


@torch.no_grad()
def contribution(pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw, c2ws, H, W, fx, fy, cx, cy, near=0.01, far=100.0, pix_guard=32, T=16,
                 min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1 / 128., sh_degree=3, *, lowpass=0.0, antialias=False,
                 stats=None):
    """The contribution statistics (ContributionStats) of the camera poses `c2ws`, arguments as for render_frames(): for every pose
    project -> bin -> gsplat_contribution through the separate library calls; nothing is rasterised and no image exists.  Every
    frame waits for its pair count like render_gaussians(), so its buffers are exact and nothing is repeated or counted twice.
    Adds into `stats` (a ContributionStats of pos.shape[0] rows on pos.device; anything else raises ValueError before anything is
    queued), or into a fresh record; returns it.  A pose without a survivor adds nothing; a pose with survivors but none on screen
    raises the reference's off-screen Exception, and `stats` then holds the poses before it."""
    spec = _frame_spec(True, H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff,
                       sh_degree=sh_degree, lowpass=lowpass, antialias=antialias)
    if not isinstance(pos, torch.Tensor):
        raise TypeError("pos must be a torch.Tensor")
    n, dev = pos.shape[0], pos.device
    if stats is not None:
        data = getattr(stats, "data", None)
        if not isinstance(stats, ContributionStats) or not stats.fits(data, n, dev):
            raise ValueError(f"contribution: stats must be a ContributionStats of {n} rows (contiguous int32 {(n, 4)}) on {dev}, not "
                             f"{type(stats).__name__}" + (f" {data.dtype} {tuple(data.shape)} on {data.device}" if isinstance(data, torch.Tensor) else ""))
    ins, g = _convert_inputs(spec.names, dict(pos=pos, opacity_raw=opacity_raw, scale_raw=scale_raw, q_raw=q_raw, f_dc=f_dc, f_rest=f_rest), n)
    cams = _convert_cameras(c2ws, dev)
    if stats is None:
        stats = ContributionStats(n, dev)
    if n == 0:                                  # nothing survives by construction
        stats.frames += len(cams)
        return stats
    front = _WaitedFront(spec, g, n, dev, _PROJECT_DEGREE[spec.sh_degree] | spec.filter)
    for c2w in cams:
        fr = front.frame(c2w)                    # (an off-screen pose raises: not counted)
        stats.frames += 1
        if fr is not None:
            _abi.check(_abi.lib().gsplat_contribution(n, fr[0], C.byref(front.view), _p(front.proj_state), _p(fr[1]), _p(stats.data), front.st),
                       "gsplat_contribution")
    return stats


def sh_accumulate(pos, eyes, grad_logit, scale=1.0, sh_degree=3):
    """(grad_f_dc [N,3], grad_f_rest [N,45]) = scale * sum over views of grad_logit[v] (x) Y(direction from eyes[v] to pos).
    sh_degree: the degree the views were rendered at; the columns of the inactive bases are zeros."""
    _abi.sh_bands_dropped(sh_degree)
    n, v = pos.shape[0], grad_logit.shape[0]
    pos32, eyes32, gl32 = _f32(pos, (n, 3), "pos"), _f32(eyes, (v, 3), "eyes"), _f32(grad_logit, (v, n, 3), "grad_logit")
    off = (n * 3 + 63) // 64 * 64                     # both views 256-byte aligned inside one buffer
    flat = torch.empty(off + n * 45, dtype=torch.float32, device=pos32.device)
    g_dc, g_rest = flat[:n * 3].view(n, 3), flat[off:off + n * 45].view(n, 45)
    _launch("gsplat_sh_accumulate_degree", pos32.device, n, v, _p(pos32), _p(eyes32), _p(gl32), float(scale), _p(g_dc), _p(g_rest), sh_degree)
    return g_dc, g_rest


class _RenderFn(torch.autograd.Function):
    """Autograd node for both entry points: apply(spec, c2w, *tensors) with exactly the tensors of spec.names; gradients for c2w and
    for the tensors, in that order.  One output, the image -- or, with spec.aux, the three outputs (image, depth, alpha)."""

    @staticmethod
    def forward(ctx, spec, c2w, *tensors):
        # needs_input_grad ignores the grad mode (and forward() itself always runs with grad disabled): the caller's grad mode
        # travels in spec.grad_mode.  Under torch.no_grad() nothing is saved for a backward that cannot come.
        need = spec.grad_mode and any(ctx.needs_input_grad)
        pose = bool(spec.grad_mode and ctx.needs_input_grad[1])          # a pose frame: c2w wants a gradient too
        result, fr, counts = _forward_impl(spec, c2w, dict(zip(spec.names, tensors)), pose, need)
        if spec.is_aux:
            ctx.set_materialize_grads(False)     # an output the loss does not read: None, not a map of zeros
        ctx.frame = fr
        ctx.c2w_dtype = c2w.dtype
        ctx.dtypes = [t.dtype for t in tensors]
        ctx.opa_shape = tensors[1].shape         # (opacity_raw: second of both entries' names)
        if counts is not None:                   # (a deferred frame's counters are read in DeferredChecks.verify())
            ctx.counts = _note_counts(counts)
        return _deliver(spec, result, tensors[0].dtype)

    @staticmethod
    def backward(ctx, grad_image, grad_depth=None, grad_alpha=None):
        fr = ctx.frame
        wanted = ctx.needs_input_grad[2:]
        g = _backward_impl(fr, grad_image, any(wanted), grad_depth, grad_alpha)
        outs = []
        for nm, dtype, want in zip(fr.spec.names, ctx.dtypes, wanted):
            t = g.get(nm) if want else None      # (None also where the frame's route took the gradient)
            if t is not None and nm == "opacity_raw":
                t = t.reshape(ctx.opa_shape)
            outs.append(t if t is None or dtype == torch.float32 else t.to(dtype))
        gc2w = g.get("c2w") if ctx.needs_input_grad[1] else None
        if gc2w is not None and ctx.c2w_dtype != torch.float32:
            gc2w = gc2w.to(ctx.c2w_dtype)
        return (None, gc2w, *outs)


def render(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, near=0.01, far=100.0, pix_guard=32, T=16,
           min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1 / 128., *, aux=False, background=None, lowpass=0.0,
           antialias=False):
    """Drop-in for the reference render() (gaussian_splatting/render.py:62-410).

    Returns the image [H, W, 3] in [0, 1], same dtype/device as `pos`, differentiable w.r.t. pos, color, opacity_raw,
    sigma and the camera pose c2w (c2w.requires_grad: dL/dc2w [4, 4] in c2w's dtype, last row 0; such a frame always takes
    the separate library calls and may not be rendered inside a gradient_route() block other than a factored exchange).  No opacity / frustum / finite
    survivor -> zero image with zero gradients; survivors but none on screen -> Exception("All projected points are
    off-screen"), as in the reference.

    Beyond the reference (keyword-only; the defaults are the reference's call).  With w_i = alpha_i T_i [T_i > 5e-5] of the
    composite, C = sum w_i c_i, A = sum w_i, D = sum w_i z_i (z_i = camera-space depth of Gaussian i):
      aux=True          returns (image, depth, alpha): depth = D and alpha = A, [H, W] each in pos.dtype, neither clamped nor
                        normalised (the expected depth is depth / alpha), differentiable like the image, c2w included.
      background=(r, g, b)   image = clamp(C + (1 - A) * background, 0, 1); a constant (sequence or tensor of 3 numbers), no
                        gradient.  No survivor: the clamped background, zero maps.
    Such a frame takes the separate library calls and may not be rendered inside a gradient_route() block.
      lowpass=s         (a multiple of 0.01 in [0, 2.55], px^2; the paper's rasteriser uses 0.3) the eigen clamp is applied to the
                        projected covariance + s I: radius, rectangles, pair count, conic and the densification extent follow.
      antialias=True    (a bool; needs lowpass > 0) the opacity of every splat is scaled by sqrt(det Sigma / det(Sigma + s I)), so a
                        sub-pixel splat keeps its energy; differentiable through Sigma.
    Anything else raises ValueError before anything is queued.  The mode is kept on the frame: the backward pass cannot be given
    another one.  The default is the reference's render, bit for bit.
    """
    spec = _frame_spec(False, H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff,
                       aux=aux, background=background, lowpass=lowpass, antialias=antialias)
    return _RenderFn.apply(spec, c2w, pos, opacity_raw, color, sigma)


def render_gaussians(pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw, c2w, H, W, fx, fy, cx, cy, near=0.01, far=100.0,
                     pix_guard=32, T=16, min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1 / 128., *, aux=False,
                     background=None, sh_degree=3, lowpass=0.0, antialias=False):
    """Fused entry: render(pos, evaluate_sh(f_dc, f_rest, pos, c2w), opacity_raw, build_sigma_from_params(scale_raw,
    q_raw), c2w, ...) in one pass (the reference's three-call sequence, scripts/train.py:463,502,505-508).  Differentiable
    w.r.t. the six parameter tensors and c2w (through the camera transform, the covariance rotation and the SH view
    direction), as render() is.  aux, background, lowpass, antialias: as for render().

    sh_degree (one of the integers 0, 1, 2, 3; anything else raises ValueError before anything is queued): the colour is
    sigmoid(sum_{k < (sh_degree + 1)^2} f_k Y_k).  f_rest stays [N, 45]; its inactive entries -- columns ch * 15 + j with
    j >= (sh_degree + 1)^2 - 1 -- are ignored: their values (a NaN included) change no output bit, their gradient is exactly
    zero on every backward route, and the image equals the default render of the same scene with zeros there.  The degree
    is kept on the frame, so the backward pass cannot be given another one."""
    spec = _frame_spec(True, H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff,
                       aux=aux, background=background, sh_degree=sh_degree, lowpass=lowpass, antialias=antialias)
    return _RenderFn.apply(spec, c2w, pos, opacity_raw, scale_raw, q_raw, f_dc, f_rest)


@torch.no_grad()
def render_frames(pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw, c2ws, H, W, fx, fy, cx, cy, near=0.01, far=100.0,
                  pix_guard=32, T=16, min_conis=1e-6, chi_square_clip=6.25, alpha_max=0.99, alpha_cutoff=1 / 128., on_frame=None, sh_degree=3,
                  *, lowpass=0.0, antialias=False, aux=False, background=None):
    """Forward-only rendering of a sequence of camera poses with the frames software-pipelined over two HIP streams:
    frame k + 1's projection / binning front (latency- and bandwidth-bound) overlaps frame k's rasterisation (VALU-bound).
    Same images as render_gaussians() frame by frame.  Returns the list of images (or calls on_frame(k, image) and returns
    None); the caller's current stream waits for all of them.  Without on_frame, and once a pair capacity is known for the
    device, no frame waits for its counters either (deferred_checks: the per-frame checks are made after the last frame is
    queued; a sequence that outgrows the buffers is rendered again).  sh_degree, lowpass, antialias: as for render_gaussians().
    aux, background: as for render_gaussians() -- every element of the result (and the argument of on_frame) is then what
    render_gaussians() returns for the same arguments, bit for bit: (image, depth, alpha) with aux=True, the image over the
    background with a background alone."""
    spec = _frame_spec(True, H, W, fx, fy, cx, cy, near, far, pix_guard, T, min_conis, chi_square_clip, alpha_max, alpha_cutoff,
                       aux=aux, background=background, sh_degree=sh_degree, lowpass=lowpass, antialias=antialias)
    dev = pos.device
    cams = [torch.as_tensor(c, dtype=torch.float32, device=dev) if not isinstance(c, torch.Tensor) else c for c in c2ws]
    tensors = dict(zip(spec.names, (pos, opacity_raw, scale_raw, q_raw, f_dc, f_rest)))
    if on_frame is not None or _ws.pair_capacity(capacity_key(dev, spec, pos.shape[0])) == 0 or _deferred_stack:
        return _render_frames(spec, dev, cams, tensors, on_frame)
    return run_deferred(lambda: _render_frames(spec, dev, cams, tensors, None))


def _render_frames(spec, dev, cams, tensors, on_frame):
    main = torch.cuda.current_stream(dev)
    streams = _pipeline_streams(dev)
    for st in streams:
        st.wait_stream(main)                                   # parameters and camera matrices produced on the caller's stream

    def begin(k):
        with torch.cuda.stream(streams[k % 2]):
            return _forward_begin(spec, cams[k], tensors)

    images = []
    started = begin(0) if cams else None
    for k in range(len(cams)):
        nxt = begin(k + 1) if k + 1 < len(cams) else None      # queue the next frame's front before waiting for this one's counters
        pend, done = started
        with torch.cuda.stream(streams[k % 2]):
            result = (done if pend is None else _forward_end(*pend))[0]
        started = nxt
        for t in result:
            if t is not None:
                t.record_stream(main)                          # allocated on a side stream, consumed on the caller's
        image = _deliver(spec, result)
        if on_frame is not None:
            main.wait_stream(streams[k % 2])                   # GPU-side dependency only: the host does not block
            on_frame(k, image)
        else:
            images.append(image)
    for st in streams:
        main.wait_stream(st)
    return None if on_frame is not None else images


_pipe_streams = {}


def _pipeline_streams(dev):
    key = (dev.type, dev.index)
    if key not in _pipe_streams:
        _pipe_streams[key] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    return _pipe_streams[key]



class _BuildSigmaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scale_raw, q_raw):
        n = scale_raw.shape[0]
        sr, qr = _f32(scale_raw, (n, 3), "scale_raw"), _f32(q_raw, (n, 4), "q_raw")
        out = torch.empty((n, 3, 3), dtype=torch.float32, device=sr.device)
        _launch("gsplat_build_sigma", sr.device, n, _p(sr), _p(qr), _p(out))
        ctx.save_for_backward(sr, qr)
        ctx.dtypes = (scale_raw.dtype, q_raw.dtype)
        return out if scale_raw.dtype == torch.float32 else out.to(scale_raw.dtype)

    @staticmethod
    def backward(ctx, grad_sigma):
        sr, qr = ctx.saved_tensors
        n = sr.shape[0]
        gs = _f32(grad_sigma, (n, 3, 3), "grad_sigma")
        gsr, gqr = torch.empty_like(sr), torch.empty_like(qr)
        _launch("gsplat_build_sigma_backward", sr.device, n, _p(sr), _p(qr), _p(gs), _p(gsr), _p(gqr))
        return gsr.to(ctx.dtypes[0]), gqr.to(ctx.dtypes[1])


def build_sigma_from_params(scale_raw, q_raw):
    """Drop-in for the reference build_sigma_from_params (gaussian_splatting/gaussian.py:71-127): Sigma = R S S R^T."""
    return _BuildSigmaFn.apply(scale_raw, q_raw)


class _EvaluateShFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f_dc, f_rest, points, c2w):
        n = points.shape[0]
        if f_rest.shape[-1] != 45:
            # the reference raises RuntimeError for any other width
            raise RuntimeError(f"evaluate_sh needs f_rest of width 45 (degree-3 SH), got {tuple(f_rest.shape)}")
        dc, rest = _f32(f_dc, (n, 3), "f_dc"), _f32(f_rest, (n, 45), "f_rest")
        pts, cam = _f32(points, (n, 3), "points"), _f32(c2w, (4, 4), "c2w")
        out = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
        _launch("gsplat_evaluate_sh", pts.device, n, _p(dc), _p(rest), _p(pts), _p(cam), _p(out))
        ctx.save_for_backward(dc, rest, pts, cam)
        ctx.dtypes = (f_dc.dtype, f_rest.dtype, points.dtype, c2w.dtype)
        return out if points.dtype == torch.float32 else out.to(points.dtype)

    @staticmethod
    def backward(ctx, grad_color):
        dc, rest, pts, cam = ctx.saved_tensors
        n = pts.shape[0]
        gc = _f32(grad_color, (n, 3), "grad_color")
        gdc, grest, gpts = torch.empty_like(dc), torch.empty_like(rest), torch.empty_like(pts)
        _launch("gsplat_evaluate_sh_backward", pts.device, n, _p(dc), _p(rest), _p(pts), _p(cam), _p(gc), _p(gdc), _p(grest), _p(gpts))
        gc2w = None
        if ctx.needs_input_grad[3]:
            # the colour depends on c2w only through the direction p - c2w[:3,3]: dL/dc2w[:3,3] = -sum dL/dp, the rest is 0
            gc2w = torch.zeros((4, 4), dtype=ctx.dtypes[3], device=pts.device)
            gc2w[:3, 3] = -gpts.double().sum(0).to(ctx.dtypes[3])
        return gdc.to(ctx.dtypes[0]), grest.to(ctx.dtypes[1]), gpts.to(ctx.dtypes[2]), gc2w


def evaluate_sh(f_dc, f_rest, points, c2w):
    """Drop-in for the reference evaluate_sh (gaussian_splatting/spherical_harmonics.py:70-166): degree-3 real SH,
    channel-major f_rest, sigmoid output.  Differentiable w.r.t. f_dc, f_rest, points and c2w (only its translation column
    moves the colour: dL/dc2w[:3,3] = -sum dL/dpoints)."""
    return _EvaluateShFn.apply(f_dc, f_rest, points, c2w)


# ---- the small helper functions the reference namespace also exports (host-side, not on the hot path) ----

HARMONICS = {   # reference gaussian_splatting/spherical_harmonics.py:50-67
    'SH_C0': 0.28209479177387814, 'SH_C1_x': 0.4886025119029199, 'SH_C1_y': 0.4886025119029199,
    'SH_C1_z': 0.4886025119029199, 'SH_C2_xy': 1.0925484305920792, 'SH_C2_xz': 1.0925484305920792,
    'SH_C2_yz': 1.0925484305920792, 'SH_C2_zz': 0.31539156525252005, 'SH_C2_xx_yy': 0.5462742152960396,
    'SH_C3_yxx_yyy': 0.5900435899266435, 'SH_C3_xyz': 2.890611442640554, 'SH_C3_yzz_yxx_yyy': 0.4570457994644658,
    'SH_C3_zzz_zxx_zyy': 0.3731763325901154, 'SH_C3_xzz_xxx_xyy': 0.4570457994644658,
    'SH_C3_zxx_zyy': 1.445305721320277, 'SH_C3_xxx_xyy': 0.5900435899266435,
}


def quat_to_rotmat(quat):
    """(x, y, z, w) quaternions [..., 4] -> rotation matrices [..., 3, 3], no normalisation (reference gaussian.py:24-68)."""
    x, y, z, w = quat.unbind(-1)
    m = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return m.reshape(quat.shape[:-1] + (3, 3))


def inv2x2(M, eps=1e-12):
    """Batched 2x2 inverse with the determinant clamped at eps (reference utils.py:152-191)."""
    det = (M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]).clamp(min=eps)
    adj = torch.stack([M[:, 1, 1], -M[:, 0, 1], -M[:, 1, 0], M[:, 0, 0]], -1).reshape(-1, 2, 2)
    return adj / det.reshape(-1, 1, 1)


def scale_intrinsics(H, W, H_src, W_src, fx, fy, cx, cy):
    """Rescale pinhole intrinsics to another resolution (reference utils.py:194-238)."""
    sx, sy = W / W_src, H / H_src
    return fx * sx, fy * sy, cx * sx, cy * sy


def project_points(pc, c2w, fx, fy, cx, cy):
    """World points -> (uv [N,2], x, y, z) in the camera frame (reference utils.py:99-149)."""
    rt = c2w[:3, :3].t()
    cam = pc @ rt.t() - rt @ c2w[:3, 3]
    x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
    return torch.stack([fx * x / z + cx, fy * y / z + cy], -1), x, y, z
