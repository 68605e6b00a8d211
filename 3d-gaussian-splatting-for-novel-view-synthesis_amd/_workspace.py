"""What outlives a frame on the host: the workspace (scratch, counter blocks, the pinned ring, events, pair capacities), the checks of
the frames that did not wait for their counters (DeferredChecks, run_deferred), the ONE reader of a counter block (read_counts) and
the counters of the most recent call (render_stats, binned_pairs).  `_last_counts` and `_last_binned` are rebound by _note_counts(),
so every reader of them lives here and other modules call the functions; what is mutated in place (forward_modes, _deferred_stack,
_ws) is never rebound anywhere.  Imports torch, ctypes and _abi only -- never ops.
"""
import collections
import ctypes as C
import weakref

import torch

from . import _abi

OFFSCREEN_MSG = "All projected points are off-screen"      # reference render.py:236


class PairCapacityExceeded(RuntimeError):
    """A frame rendered without waiting for its pair count (deferred_checks) had more (list, Gaussian) pairs than the buffers
    kept from earlier frames: its image and gradients are invalid.  The capacity has been raised; render it again."""


PINNED_SLOTS = 256      # counter blocks in flight per (device, stream) before one is reused


def capacity_key(device, view, n):
    """Pair capacities are kept per (device, image size, power-of-two bucket of the Gaussian count, filter mode): one large scene
    does not make every later frame of a small one allocate, launch over and (deterministic mode) clear its buffers, and a
    filtered frame -- the low-pass grows every footprint, and the pair count with it -- learns its own capacity."""
    return (device.type, device.index, view.H, view.W, max(int(n), 1).bit_length(), getattr(view, "filter", 0))


class _Workspace:
    """Grow-only scratch buffers, the persistent counter block of gsplat_project, a ring of pinned counter blocks and one
    event per (device, stream): calls on different streams never share them (scratch is dead after each call, in stream
    order).  `capacity`: per capacity_key(), the largest pair count seen x 1.25 (sizes the buffers of frames that do not wait).
    `key` = (device type, device index, stream handle) is the caller's, who looks the current stream up ONCE per pass: that lookup
    is the costliest thing these methods would do."""

    def __init__(self):
        self.scratch = {}
        self.pinned = {}
        self.events = {}
        self.counters = {}
        self.capacity = {}
        self.slot = {}
        self.owners = {}            # per (device, stream): slot -> weak reference to the DeferredChecks that still has to read it
        self.event_pool = {}        # per device: events of frames whose counters have been read, handed out again (get_event(fresh=True))
        self.sizes = {}             # (n, capacity, H, W, flags) -> (frame bytes, bin scratch bytes): host arithmetic, cached

    def get_counter_block(self, device, key):
        """Zeroed once; every gsplat_project call leaves it zeroed again (include/gsplat_mi355x.h)."""
        buf = self.counters.get(key)
        if buf is None:
            buf = self.counters[key] = torch.zeros(int(_abi.lib().gsplat_project_scratch_bytes(0)), dtype=torch.uint8, device=device)
        return buf

    def counter_set(self, device, key, owner=None, fresh_event=False):
        """(counters, pinned, slot, ready) of the next projection on the stream of `key`: the device's counter block, a pinned block of
        the ring with its index (owner: the DeferredChecks that will read it) and the event to record behind the counters."""
        return (self.get_counter_block(device, key), *self.next_pinned(device, key, owner), self.get_event(device, fresh_event, key))

    def next_pinned(self, device, key, owner=None):
        """A pinned, device-mapped counter block nobody else is using.  A slot whose last frame still waits to be looked at by
        its DeferredChecks (a block left without verify(), or a very long one) is read by that owner first -- the frame
        finished long ago -- so a ring that comes round never hands out a block somebody still has to read."""
        ring = self.pinned.get(key)
        if ring is None:
            ring = self.pinned[key] = torch.zeros((PINNED_SLOTS, C.sizeof(_abi.Counts)), dtype=torch.uint8).pin_memory()
            self.owners[key] = {}
        i = self.slot.get(key, 0)
        self.slot[key] = (i + 1) % PINNED_SLOTS
        owners = self.owners[key]
        ref = owners.pop(i, None)
        if ref is not None:
            prev = ref()
            if prev is not None:
                prev._release_slot(key, i)
        if owner is not None:
            owners[i] = weakref.ref(owner)
        return ring[i], i

    def note_pairs(self, ckey, n_binned):
        want = int(n_binned * 1.25) + 4096
        if want > self.capacity.get(ckey, 0):
            self.capacity[ckey] = want

    def pair_capacity(self, ckey):
        return self.capacity.get(ckey, 0)

    def get_event(self, device, fresh, key):
        """One reusable event per stream: gsplat_project records it right behind the counters (fresh: an event of its own,
        for a frame whose counters are read later)."""
        if fresh:
            pool = self.event_pool.get((device.type, device.index))
            if pool:
                return pool.pop()             # (its handle exists, and the frame it belonged to is long done)
        ev = None if fresh else self.events.get(key)
        if ev is None:
            ev = torch.cuda.Event(enable_timing=False, blocking=False)
            ev.record(torch.cuda.current_stream(device))          # events are created lazily: force the handle to exist
            if not fresh:
                self.events[key] = ev
        return ev

    def recycle_event(self, device, ev):
        pool = self.event_pool.setdefault((device.type, device.index), [])
        if len(pool) < 4 * PINNED_SLOTS:
            pool.append(ev)

    def get_scratch(self, device, nbytes, key):
        buf = self.scratch.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
            self.scratch[key] = buf
        return buf

    def frame_sizes(self, lib, n, capacity, view, flags):
        k = (n, capacity, view.H, view.W, flags)                  # (the filter bits change no size)
        got = self.sizes.get(k)
        if got is None:
            if len(self.sizes) > 4096:
                self.sizes.clear()
            got = self.sizes[k] = (lib.gsplat_frame_bytes(n, capacity, C.byref(view), flags),
                                   lib.gsplat_bin_scratch_bytes(capacity, C.byref(view)))
        return got


def reset_pair_capacity():
    """Forget the pair capacities kept from earlier frames (a new scene, a new Trainer): the next frame of every (device, image
    size, Gaussian-count bucket) waits for its own count again."""
    _ws.capacity.clear()


_ws = _Workspace()


def read_counts(pinned, ckey):
    """(counts, scene) of a frame whose event the caller has waited for: its pinned counter block as _abi.Counts and what the reference
    decides from it (a GSPLAT_SCENE_* code); raises the pair capacity kept for `ckey` to the frame's count.  What follows -- raising, an
    empty frame, a flag for verify() -- is the caller's."""
    counts = _abi.Counts.from_buffer_copy(pinned.numpy().tobytes())
    _ws.note_pairs(ckey, counts.n_binned)
    return counts, _abi.lib().gsplat_classify_counts(C.byref(counts))


class DeferredChecks:
    """Render without waiting for the per-frame counters (training loops, frame sequences):

        with ops.deferred_checks() as chk:
            for view in views: loss(render_gaussians(...)).backward()      # no host synchronisation per view
        chk.verify()                                                        # ONE wait, then every frame's checks

    Inside the block a render sizes its pair buffers from the capacity kept from earlier frames (x 1.25 of the largest
    count seen for that image size and Gaussian-count bucket) instead of waiting for its own count, and the SH colour is
    evaluated inside the projection kernel (one pass over the inputs).  What the reference decides from the counts is decided
    in verify(): survivors but none on screen -> the same Exception("All projected points are off-screen"), now raised there; no
    survivor -> the frame was a zero image with zero gradients anyway.  A frame with more pairs than the capacity raises
    PairCapacityExceeded (capacity raised; render the block again: its results are invalid).  The first render of a size on a
    device (no capacity known yet) waits like an ordinary one.

    A block that is left by an exception has its frames' counters read then and there (nothing is raised on top of the exception
    in flight); one that is simply never verified keeps its findings, and its pinned counter blocks are read before the ring
    hands them to another frame (_Workspace.next_pinned): no block is ever reused unread."""

    def __init__(self):
        self.pending = []          # _Unread, one per frame whose counters have not been looked at, in frame order
        self.counts = []
        self._overflow = self._offscreen = False

    def add(self, pinned, event, capacity, device, ckey, slot):
        self.pending.append(_Unread(pinned, event, capacity, device, ckey, slot))
        if len(self.pending) >= PINNED_SLOTS // 2:           # long sequences: look at the oldest frames before their pinned
            self._drain(len(self.pending) // 2)              # counter blocks come round again (they finished long ago)

    def _drain(self, count):
        for entry in self.pending[:count]:
            entry.event.synchronize()
            counts, scene = read_counts(entry.pinned, entry.ckey)
            self.counts.append(counts)
            self._overflow |= entry.capacity is not None and counts.n_binned > entry.capacity
            self._offscreen |= scene == _abi.GSPLAT_SCENE_ALL_OFFSCREEN
            _note_counts(counts)
            _ws.recycle_event(entry.device, entry.event)
            ring_key, index = entry.slot
            owners = _ws.owners.get(ring_key)
            if owners is not None:
                ref = owners.get(index)
                if ref is not None and ref() is self:
                    del owners[index]
        del self.pending[:count]

    def _release_slot(self, ring_key, index):
        """The ring is about to hand slot `index` to another frame: read everything up to the frame that holds it."""
        for k, entry in enumerate(self.pending):
            if entry.slot == (ring_key, index):
                self._drain(k + 1)
                return

    def __enter__(self):
        _deferred_stack.append(self)
        return self

    def __exit__(self, exc_type, exc, tb):
        _deferred_stack.remove(self)
        if exc_type is not None and self.pending:           # nobody will call verify(): read the counters now, raise nothing
            try:
                self._drain(len(self.pending))
            except Exception:                                # (a device error while draining must not mask the exception in flight)
                self.pending = []
        return False

    def verify(self):
        self._drain(len(self.pending))
        overflow, offscreen = self._overflow, self._offscreen
        self._overflow = self._offscreen = False
        if offscreen:
            raise Exception(OFFSCREEN_MSG)
        if overflow:
            raise PairCapacityExceeded("more (list, Gaussian) pairs than the buffers kept from earlier frames: render the block again")
        return self.counts


# a frame whose counters are still unread (between the halves of its forward pass, or in a DeferredChecks): its pinned counter block,
# the event recorded behind the counters, the pair capacity its buffers were sized with (None: it waits for its own count), its device
# and capacity_key(), and slot = (ring key, index) of the block in the ring, ring key = (device type, device index, stream)
_Unread = collections.namedtuple("_Unread", "pinned event capacity device ckey slot")
_deferred_stack = []
forward_modes = {"waited": 0, "deferred": 0}     # forward passes that waited for their counters / that did not (diagnostics, tests)


def deferred_checks():
    return DeferredChecks()


def run_deferred(fn, attempts=4):
    """fn() queues renders (and their backward passes) -- it runs inside deferred_checks() and is REPEATED while one of its frames
    outgrows the pair buffers kept from earlier frames (the capacity is raised each time; the first frame of a much larger scene
    does that once).  Returns fn()'s result of the pass that passed its checks; the off-screen exception propagates."""
    for _ in range(attempts):
        with deferred_checks() as chk:
            out = fn()
        try:
            chk.verify()
            return out
        except PairCapacityExceeded:
            continue
    raise RuntimeError(f"the pair buffers overflowed {attempts} times in a row")


_last_counts = None
_last_binned = None


def _note_counts(counts):
    """Keep the counters of the most recent call for render_stats() / binned_pairs(); returns the render_stats() triple."""
    global _last_counts, _last_binned
    _last_counts = (counts.n_survivors, counts.n_visible, int(counts.n_pairs))
    _last_binned = int(counts.n_binned)
    return _last_counts


def binned_pairs():
    """(list, Gaussian) pairs the most recent call really binned (after the exact ellipse / list test): P_b of DESIGN.md."""
    return _last_binned


def render_stats(image=None):
    """(n_survivors, n_visible V, n_pairs P) of the call that produced `image` (or of the most recent call)."""
    fn = image.grad_fn if image is not None else None
    got = getattr(fn, "counts", None) if fn is not None else None
    return got if got is not None else _last_counts
