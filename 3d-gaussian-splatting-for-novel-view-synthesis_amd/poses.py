"""Per-view camera-pose corrections (not in the reference): the poses a structure-from-motion run hands over are noisy,
and a model trained at them pays with blur.  As in gsplat (pose_opt) and nerfstudio's camera optimiser, every training camera gets a
small learned rigid correction that its given pose is composed with before the render:

    delta = (d[3], p[3], s[3]), zero at the start: a translation and the 6-D rotation of Zhou et al.
    a1 = p + (1,0,0), a2 = s + (0,1,0), Gram-Schmidt to the rows b1, b2, b3 = b1 x b2 of D;   out = [[R D, R d + e], [c2w[3]]]

    apply(c2w, delta)                        the composition, differentiable with respect to both
    PoseTable(n_views, device)               one delta per training camera, their gradient buffer and an Adam state of their own
    table.apply_view(c2w, idx)               the corrected pose of view idx; its backward adds into table.grad[idx]
    table.c2w(c2ws, idxs)                    the corrected poses of a batch, under no_grad (exports, viewers)

    img = gs.render_gaussians(..., poses.apply(c2w, delta), ...)      # the render's dL/dc2w flows into delta

TrainConfig.pose_opt switches it on in Trainer.step.  delta = 0 returns c2w as the same numbers, so the first iteration of a
pose-trained model renders the bits of a pose frame at the given pose.

ctypes calls into csrc/gsplat_pose_delta.hip on the current stream, in the style of exposure.py; nothing here reads the device.  One
lane per view and no atomics: the same bits on every call, every stream and every launch.  There is no CPU fallback.
"""
import torch

from . import _abi
from ._viewtable import ViewFn, ViewOp, ViewTable
from ._dev import _launch, _p


def _shapes(c2w, delta):
    shape = tuple(c2w.shape)
    if len(shape) not in (2, 3) or shape[-2:] != (4, 4):
        raise ValueError(f"c2w must be [4, 4] or [B, 4, 4], got {shape}")
    want = (shape[0], 9) if len(shape) == 3 else (9,)
    if tuple(delta.shape) != want:
        raise ValueError(f"delta must be {list(want)} for a c2w of {list(shape)}, got {list(delta.shape)}")
    if min(shape) < 1:
        raise ValueError(f"c2w has an empty dimension: {shape}")
    return shape, (shape[0] if len(shape) == 3 else 1,)


def _forward(c, d, dims, out, stream):
    _abi.check(_abi.lib().gsplat_pose_delta_forward(_p(c), _p(d), *dims, _p(out), stream), "gsplat_pose_delta_forward")


def _backward(c, d, g, dims, g_c2w, target, rows, flags, stream):
    _abi.check(_abi.lib().gsplat_pose_delta_backward(_p(c), _p(d), _p(g), *dims, _p(g_c2w), _p(target), _p(rows), flags, stream),
               "gsplat_pose_delta_backward")


# out = compose(c2w, delta) over gsplat_pose_delta_forward / gsplat_pose_delta_backward, in the skeleton of _viewtable.ViewFn
_OP = ViewOp("delta", _shapes, _forward, _backward, _abi.GSPLAT_POSE_DELTA_ACCUMULATE, "c2w")


def apply(c2w, delta):
    """The pose c2w composed with its correction: c2w [4, 4] with delta [9], or [B, 4, 4] with [B, 9] (one correction per pose).
    delta = 0 returns c2w as the same numbers.  Differentiable with respect to both; the half that is not needed is not computed.
    fp32 is computed directly, other dtypes are converted.  One launch forward, one backward."""
    return ViewFn.apply(_OP, c2w, delta, None, None)


class PoseTable(ViewTable):
    """One correction per training camera: `params` [V, 9] zeros, `grad` a buffer of the same shape, and an Adam state of its own -- a
    second optim.GaussianAdam over the one tensor (eps = 1e-8 and a dense step), apart from the model's optimiser: restarts of that
    one after a densification touch neither the table nor its moments.  As for the other tables the step is DENSE: a row no view of
    the iteration used still moves by the momentum earlier iterations left in its moments.

        table.zero_grad()
        img = render(..., table.apply_view(c2w, idx), ...); loss(img).backward()      # adds into table.grad[idx]
        table.regularise(cfg); table.step(lr)
    """

    name, op = 'pose', _OP

    def __init__(self, n_views, device, lr=1e-5, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(n_views, device, lr, betas, eps)

    def _identity(self, device):
        return torch.zeros(9, dtype=torch.float32, device=device)

    def regularise(self, cfg):
        """grad += cfg.pose_reg * params (the gradient of (pose_reg / 2) |params|^2; gsplat's pose_opt_reg, a weight decay inside its
        Adam): one launch over the whole table, after the all-reduce of `grad`.  Adds nothing to step()'s dict."""
        dev = self.params.device
        _launch("gsplat_pose_delta_decay", dev, _p(self.params), self.n_views, float(cfg.pose_reg), _p(self.grad))
        return {}

    @torch.no_grad()
    def c2w(self, c2ws, idxs):
        """The corrected poses of the given ones: c2ws [B, 4, 4] (or [4, 4] with one index) and idxs, B integers in [0, V) -- one
        gather of the rows and one launch, under no_grad; for exports and viewers."""
        single = isinstance(c2ws, torch.Tensor) and c2ws.dim() == 2
        idxs = [self.check_index(i) for i in ([idxs] if single else list(idxs))]
        dev = self.params.device
        if not isinstance(c2ws, torch.Tensor):
            c2ws = torch.stack([torch.as_tensor(c) for c in c2ws])
        c = c2ws[None] if single else c2ws
        if c.dim() != 3 or tuple(c.shape) != (len(idxs), 4, 4):
            raise ValueError(f"c2ws must be [{len(idxs)}, 4, 4] for {len(idxs)} indices, got {list(c2ws.shape)}")
        out = apply(c.to(dev), self.params[torch.tensor(idxs, dtype=torch.int64, device=dev)])
        return out[0] if single else out
