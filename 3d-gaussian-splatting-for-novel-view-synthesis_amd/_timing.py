"""The optional per-stage timer of the kernels' launches: StageTimer, the `_stage` bracket round a launch, and the one installed timer.
`_timer` is rebound by set_stage_timer(), so every reader of it lives here; other modules call wants() and _stage.  Imports torch only.
"""
import torch


class StageTimer:
    """Optional per-stage timing with HIP events recorded on the stream the kernels are launched on (torch's current
    stream).  bench.py installs one with `set_stage_timer`; when none is installed the hooks cost nothing."""

    def __init__(self, only=None, every=1):
        self.events = []          # (stage, start_event, end_event)
        self.only = set(only) if only else None      # restrict to these stages (every event pair costs ~10 us of stream time)
        self.every = max(1, int(every))              # ... and to every n-th pass (the passes in between run exactly as without a timer)
        self.passes = 0

    def wants(self, stages):
        """Does this pass bracket any of `stages`?  (asked ONCE per pass and direction by the render op; counts the passes)"""
        if self.only is not None and not (self.only & stages):
            return False
        self.passes += 1
        return (self.passes - 1) % self.every == 0

    def totals_ms(self):
        """stage -> (launches, total milliseconds); call after a device synchronise."""
        out = {}
        for name, a, b in self.events:
            n, t = out.get(name, (0, 0.0))
            out[name] = (n + 1, t + a.elapsed_time(b))
        return out

    def reset(self):
        self.events = []


_timer = None


def set_stage_timer(timer):
    global _timer
    _timer = timer


def wants(stages):
    """Is a timer installed that brackets any of `stages` in this pass?  (once per pass and direction: StageTimer.wants counts)"""
    return _timer is not None and _timer.wants(stages)


class _stage:
    __slots__ = ("name", "a")

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.a = None
        if _timer is not None and (_timer.only is None or self.name in _timer.only):
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.a is not None and _timer is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _timer.events.append((self.name, self.a, b))
