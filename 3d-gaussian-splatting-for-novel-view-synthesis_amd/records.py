"""The three per-Gaussian records a pass can fill beside its images and gradients -- DensifyStats, VisibleSet, ContributionStats -- on
one small base (the rows, reset(n), "does this record fit the frame"), the context slots of the two that frames add to during their
backward pass (densify_stats(), visible_set()), and the one dispatch of a frame to them (add_frame_records).  The slots are read
once, in the caller's thread, when a frame is rendered (frame_records); the backward pass, on autograd's thread, reads the frame's
own fields only.  This module reads the fields of the frame it is given and never imports ops.
"""
import contextlib
import contextvars
import ctypes as C

import torch
import torch.distributed as dist

from . import _abi
from ._dev import _launch, _p


class _Record:
    """`.data`: one row of `_ROW` elements of `_DTYPE` per Gaussian, zeros when made; `_ALIGN`: what the kernels need of its address."""
    _ROW, _DTYPE, _ALIGN = (), None, 1

    def __init__(self, n, device):
        self.data = torch.zeros((int(n),) + self._ROW, dtype=self._DTYPE, device=device)

    def reset(self, n=None):
        """Zero the record; with another n, a fresh record of n rows (after a densification or a pruning)."""
        if n is None or int(n) == self.data.shape[0]:
            self.data.zero_()
        else:
            self.data = torch.zeros((int(n),) + self._ROW, dtype=self._DTYPE, device=self.data.device)
        return self

    @classmethod
    def fits(cls, data, n, device):
        """Is the tensor `data` a record of this class for a frame of n Gaussians on `device`?"""
        return (data.dtype == cls._DTYPE and tuple(data.shape) == (n,) + cls._ROW and data.device == device and data.is_contiguous()
                and not data.data_ptr() % cls._ALIGN)


class DensifyStats(_Record):
    """Screen-space densification statistics of N Gaussians: `.data` [N, 4] float32 = (grad_sum, count, extent_max, 0).

        stats = ops.DensifyStats(n, device)
        with ops.densify_stats(stats):
            loss(render_gaussians(...)).backward()          # every backward pass of a frame rendered here adds that frame
        hot = stats.mean_grad() >= 0.0002

    Per frame, every Gaussian binned into at least one list adds the norm of the gradient of its projected centre (NDC units: the
    paper's 0.0002 carries over) to grad_sum and 1 to count, and raises extent_max to its screen half-extent (pixels, at most 250).
    The accumulation is a plain read-modify-write: backward passes that add into one record must be ordered on one stream."""
    _ROW, _DTYPE, _ALIGN = (4,), torch.float32, 16

    grad_sum = property(lambda self: self.data[:, 0])
    count = property(lambda self: self.data[:, 1])
    extent_max = property(lambda self: self.data[:, 2])

    def mean_grad(self):
        return self.grad_sum / self.count.clamp(min=1)

    def merge_(self, other):
        """self (+)= other -- (sum, sum, max) -- on the current stream; `other` is zero afterwards (the merge kernel clears the
        rows it consumed)."""
        a, b = self.data, other.data
        if not a.is_cuda:
            raise RuntimeError(f"the record is on {a.device}: the merge kernel needs GPU tensors (there is no CPU fallback)")
        if b.shape != a.shape or b.device != a.device or b.dtype != torch.float32 or not b.is_contiguous() or other is self:
            raise ValueError(f"merge_: the other record must be another float32 {tuple(a.shape)} record on {a.device}")
        _launch("gsplat_densify_stats_merge", a.device, a.shape[0], _p(b), _p(a))
        return self

    def all_reduce(self, group=None):
        """Sum grad_sum and count, take the maximum of extent_max over the ranks of `group` (plain torch.distributed on contiguous
        copies: CPU tensors over gloo work too).  Every rank ends with the same bits."""
        sums, ext = self.data[:, :2].contiguous(), self.data[:, 2].contiguous()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(ext, op=dist.ReduceOp.MAX, group=group)
        self.data[:, :2] = sums
        self.data[:, 2] = ext
        return self


class VisibleSet(_Record):
    """The Gaussians the frames of a pass binned: `.data` [N] uint8, non-zero = binned into at least one list of at
    least one frame -- the only rows that can have a non-zero gradient, and the rows optim.GaussianAdam.step(visible=...) steps.

        seen = ops.VisibleSet(n, device)
        with ops.visible_set(seen):
            loss(render_gaussians(...)).backward()          # every backward pass of a frame rendered here adds that frame's set
        optimizer.step(visible=seen)

    A frame only ever stores 1 and never reads the record, so frames on different streams add into one record with no ordering
    between them; reset() zeroes it.  Works on 'cpu' too (reset, all_reduce over gloo): only adding frames needs the GPU."""
    _ROW, _DTYPE = (), torch.uint8

    def all_reduce(self, group=None):
        """The union over the ranks of `group`: an element-wise MAX (plain torch.distributed: CPU tensors over gloo work too).  Every
        rank ends with the same bytes."""
        dist.all_reduce(self.data, op=dist.ReduceOp.MAX, group=group)
        return self


class ContributionStats(_Record):
    """Per-Gaussian contribution statistics of N Gaussians: how much each Gaussian takes part in the composite of the
    frames added so far.  `.data` [N, 4] int32 -- the 32-bit words of include/gsplat_mi355x.h, every one an order-independent integer:
    words 0-1 the little-endian uint64 sum_q (units of 2^-32), word 2 the float32 bits of weight_max, word 3 the uint32 pixel count
    (wraps after 2^32 pixel hits).

        stats = ops.contribution(pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw, c2ws, H, W, fx, fy, cx, cy)
        never_matters = stats.weight_max == 0

    Adding is integer add / max, so the record holds the same bits whatever order frames, streams or ranks arrive in.  Works on
    'cpu' too (accessors, merge_, all_reduce over gloo): only ops.contribution needs the GPU."""
    _ROW, _DTYPE, _ALIGN = (4,), torch.int32, 16

    def __init__(self, n, device):
        super().__init__(n, device)
        self.frames = 0                     # frames accumulated (a host count)

    n = property(lambda self: self.data.shape[0])
    sum_q = property(lambda self: self.data.view(torch.int64)[:, 0])                 # (read as unsigned: below 2^63 in practice)
    weight_sum = property(lambda self: self.sum_q.to(torch.float64) * 2.0 ** -32)
    weight_max = property(lambda self: self.data[:, 2].contiguous().view(torch.float32))
    pixels = property(lambda self: self.data[:, 3].to(torch.int64) & 0xFFFFFFFF)

    def reset(self, n=None):
        self.frames = 0
        return super().reset(n)

    def merge_(self, other):
        """self (+)= other -- (add, max, add) on the integer words, frames added; `other` is left as it is."""
        a, b = self.data, other.data
        if b.shape != a.shape or b.device != a.device or b.dtype != torch.int32 or not b.is_contiguous() or other is self:
            raise ValueError(f"merge_: the other record must be another int32 {tuple(a.shape)} record on {a.device}")
        a.view(torch.int64)[:, 0] += b.view(torch.int64)[:, 0]
        a[:, 2] = torch.maximum(a[:, 2], b[:, 2])        # (non-negative floats order like their bits)
        a[:, 3] += b[:, 3]                                # (int32 wraps like uint32)
        self.frames += other.frames
        return self

    def all_reduce(self, group=None):
        """SUM of sum_q and pixels, MAX of word 2 over the ranks of `group`, and the sum of .frames (plain torch.distributed on integer
        copies: CPU tensors over gloo work too).  Every rank ends with the same bits."""
        sums = torch.stack([self.sum_q, self.pixels, torch.full_like(self.sum_q, int(self.frames))], 1).contiguous()      # int64 [N, 3]
        if sums.shape[0] == 0:
            sums = torch.tensor([[0, 0, int(self.frames)]], dtype=torch.int64, device=self.data.device)
        mx = self.data[:, 2].contiguous()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        self.frames = int(sums[0, 2])
        if self.data.shape[0]:
            self.data.view(torch.int64)[:, 0] = sums[:, 0]
            self.data[:, 2] = mx
            self.data[:, 3] = sums[:, 1].contiguous().view(torch.int32).view(-1, 2)[:, 0]      # the low words: pixels mod 2^32
        return self


# The records the frames rendered inside a densify_stats() / visible_set() block add to.  Slots of their own (not a gradient route:
# they combine with any route and with each other), read once, in the caller's thread, when a frame is rendered (frame_records).
_stats = contextvars.ContextVar("gsplat_densify_stats", default=None)
_stats_absgrad = contextvars.ContextVar("gsplat_densify_stats_absgrad", default=False)
_visible = contextvars.ContextVar("gsplat_visible_set", default=None)
absgrad_calls = {"separate": 0, "arena": 0}      # statistics calls queued in absolute-gradient mode, by the kind of frame


@contextlib.contextmanager
def _block(rec, *settings):
    """The `with` of densify_stats() / visible_set(): every (slot, value) of `settings` holds inside and is restored on exit."""
    tokens = [(slot, slot.set(value)) for slot, value in settings]
    try:
        yield rec
    finally:
        for slot, token in reversed(tokens):
            slot.reset(token)


def densify_stats(rec, absgrad=False):
    """Every backward pass of a frame rendered inside the block adds that frame's statistics to `rec` (a DensifyStats, or its
    float32 [N, 4] tensor), once, on the backward's stream, behind its raster phase -- whatever route the gradients take.  Empty and
    all-culled frames, frames rendered under torch.no_grad() and frames that overflowed their pair capacity add nothing.  A record
    that does not fit the frame (float32 [n, 4], contiguous, on the frame's device) raises ValueError when the frame is rendered.

    absgrad=True (a bool, else TypeError): grad_sum gets the ABSOLUTE-gradient statistic (AbsGS) -- per pixel, the
    magnitudes of dL/du and dL/dv of the projected centre, added without their signs; the frame's raster backward is then the
    variant that forms them, and its gradients are unchanged.  count and extent_max are the same in both modes."""
    if type(absgrad) is not bool:
        raise TypeError(f"densify_stats(): absgrad must be a bool, not {absgrad!r}")
    data = rec.data if isinstance(rec, DensifyStats) else rec
    if not isinstance(data, torch.Tensor):
        raise TypeError("densify_stats() takes a DensifyStats or its [N, 4] tensor")
    return _block(rec, (_stats, data), (_stats_absgrad, absgrad))       # (the arguments are checked by the call, not by the `with`)


def visible_set(rec):
    """Every backward pass of a frame rendered inside the block adds that frame's visible set to `rec` (a VisibleSet, or its uint8 [N]
    tensor), once, on the backward's stream -- whatever route the gradients take, and beside densify_stats().  Empty and all-culled
    frames, frames rendered under torch.no_grad() and frames that overflowed their pair capacity add nothing.  A record that does
    not fit the frame (uint8 [n], contiguous, on the frame's device) raises ValueError when the frame is rendered."""
    data = rec.data if isinstance(rec, VisibleSet) else rec
    if not isinstance(data, torch.Tensor):
        raise TypeError("visible_set() takes a VisibleSet or its uint8 [N] tensor")
    return _block(rec, (_visible, data))       # (the argument is checked by the call, not by the `with`)


def _slot_record(slot, cls, who, pos):
    data = slot.get()
    if data is not None and not cls.fits(data, pos.shape[0], pos.device):
        raise ValueError(f"{who}: the record is {data.dtype} {tuple(data.shape)} on {data.device}; this frame needs a contiguous "
                         f"{str(cls._DTYPE)[6:]} {(pos.shape[0],) + cls._ROW} record on {pos.device}")
    return data


def frame_records(pos, need_grad):
    """(stats, absgrad, visible) of a frame of the Gaussians `pos`: the tensors of the active densify_stats() and visible_set() blocks
    and the mode of the former -- (None, False, None) for a frame without a backward pass.  A record that does not fit is refused
    whatever the frame (even where nothing is rendered), the densification record first."""
    stats, visible = _slot_record(_stats, DensifyStats, "densify_stats", pos), _slot_record(_visible, VisibleSet, "visible_set", pos)
    if not need_grad:
        return None, False, None
    return stats, stats is not None and _stats_absgrad.get(), visible


def add_frame_records(fr, st, grad2d=None):
    """Add a frame to its densification record (fr.stats, in the mode fr.absgrad) and its visible set (fr.visible), on the stream
    `st`, once its raster backward is queued.  A frame on an arena (fr.arena, queued by gsplat_forward_deferred) takes the
    gsplat_frame_* entries; any other takes the plain entries with fr.proj_state, and `grad2d` for the statistics."""
    if fr.stats is None and fr.visible is None:
        return
    lib, arena = _abi.lib(), fr.arena
    head = (fr.n, fr.n_pairs, C.byref(fr.spec.view)) + ((_p(fr.proj_state),) if arena is None else (_p(arena), arena.numel()))
    family, kind = ("gsplat_", "separate") if arena is None else ("gsplat_frame_", "arena")
    if fr.stats is not None:
        name = family + ("densify_stats_abs" if fr.absgrad else "densify_stats")
        _abi.check(getattr(lib, name)(*head, *((_p(grad2d),) if arena is None else ()), _p(fr.stats), st), name)
        if fr.absgrad:
            absgrad_calls[kind] += 1
    if fr.visible is not None:
        name = family + "visible_set"
        _abi.check(getattr(lib, name)(*head, _p(fr.visible), st), name)
