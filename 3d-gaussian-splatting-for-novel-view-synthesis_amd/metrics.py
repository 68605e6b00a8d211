"""Image quality metrics of held-out views (not in the reference): per-image PSNR, SSIM, L1 and MSE of a rendered
frame against its photograph, over an optional validity mask, and -- for a model trained with per-view exposure or bilateral grids,
which learns the scene up to a colour transform per image -- the same after a per-image affine colour correction (the `cc_psnr` of
gsplat and the Mip-NeRF 360 code base).

    image_metrics(pred, target, mask=None, colour_correct=False)   -> ImageMetrics(psnr, ssim, l1, mse, affine), device tensors
    psnr(pred, target, mask=None), ssim(pred, target, mask=None)   one value each
    fit_affine(pred, target, mask=None)                            the colour correction alone, [3, 4] = [M | t] per image
    evaluate(params, views, ...)                                   render the views forward-only and measure each: the report

Per image, over its n valid pixels (mask nonzero; no mask: all):
    l1 = sum |x - y| / (3 n),   mse = sum (x - y)^2 / (3 n),   psnr = -10 log10(mse)  (data range 1; +inf for mse == 0),
    ssim = the SSIM map of the training loss (11 x 11 Gaussian window, sigma 1.5, zero padding, per channel; computed from the whole
           images: the mask does not alter the window statistics) averaged over the valid pixels and the three channels.
    n == 0: NaN in all four and in the affine; no other image of the batch is affected.
The values are per image, never a batch mean, and a batch gives the same bits as its images one by one.
colour_correct=True: [M | t] minimising sum_valid |M x + t - y|^2 (float64 normal equations, a ridge of 1e-8 n toward the identity)
is fitted first, and the metrics are those of clamp(M x + t, 0, 1) against y.  Without it nothing is clamped.

ctypes calls into csrc/gsplat_metrics.hip on the current stream, in the style of exposure.py; nothing but evaluate()'s aggregation
reads the device.  Every sum is formed in a fixed order without float atomics: the same bits on every call, stream and rank.  There is no
gradient and no CPU fallback.
"""
import collections

import torch

from . import _abi, dp, harness, losses, ops
from ._dev import _f32, _p, _stream_ptr

ImageMetrics = collections.namedtuple("ImageMetrics", ("psnr", "ssim", "l1", "mse", "affine"))
MAX_BATCH = 65535          # images per call: the z extent of the kernels' grid (include/gsplat_mi355x.h)


def _scratch(lib, dims, flags, dev):
    """The scratch buffer of a call; ValueError where the library has no size for the shape (an image too large for its grid)."""
    nbytes = lib.gsplat_metrics_scratch_bytes(*dims, flags)
    if nbytes < 0:
        raise ValueError(f"the metrics kernels cannot take images of B, H, W = {dims} (B <= {MAX_BATCH}, H <= {16 * 65535}, H W < 2^38)")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _check_shapes(pred_shape, target_shape, mask):
    """(batched, (B, H, W)) of a call's arguments; ValueError / TypeError for what the kernels cannot take.  Looks at shapes and dtypes
    only: nothing here needs a GPU."""
    shape = tuple(pred_shape)
    if len(shape) not in (3, 4) or shape[-1] != 3 or tuple(target_shape) != shape:
        raise ValueError(f"pred/target must both be [H, W, 3] or [B, H, W, 3], got {shape} and {tuple(target_shape)}")
    if min(shape) < 1:
        raise ValueError(f"pred has an empty dimension: {shape}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise TypeError("mask must be a torch.Tensor")
        if tuple(mask.shape) != shape[:-1]:
            raise ValueError(f"mask must be {list(shape[:-1])} for images of {list(shape)}, got {list(mask.shape)}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be bool or uint8 (nonzero = valid), not {mask.dtype}")
    batched = len(shape) == 4
    if batched and shape[0] > MAX_BATCH:
        raise ValueError(f"a batch holds at most {MAX_BATCH} images (the kernels' grid), got {shape[0]}: split it")
    return batched, ((shape[0] if batched else 1), shape[-3], shape[-2])


def _mask_bytes(mask, dev):
    """The mask as contiguous bytes on the device (a bool tensor is one byte of 0 / 1 per element: viewed, not converted)."""
    if mask is None:
        return None
    if not mask.is_cuda:
        raise RuntimeError(f"mask is on {mask.device}: the metrics need GPU tensors (there is no CPU fallback)")
    m = mask.detach().to(dev).contiguous()
    return m.view(torch.uint8) if m.dtype is torch.bool else m


def _arguments(pred, target, mask):
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("pred and target must be torch.Tensors")
    batched, dims = _check_shapes(pred.shape, target.shape, mask)
    x, y = _f32(pred, tuple(pred.shape), "pred"), _f32(target, tuple(pred.shape), "target")
    return batched, dims, x, y, _mask_bytes(mask, x.device)


def _forward(x, y, m, dims, colour_correct, out, affine):
    """gsplat_metrics_forward into out [B, 4] (and affine [B, 12]) on the current stream of x's device."""
    lib = _abi.lib()
    flags = _abi.GSPLAT_METRICS_COLOUR_CORRECT if colour_correct else 0
    dev = x.device
    with torch.cuda.device(dev):
        scratch = _scratch(lib, dims, flags, dev)
        _abi.check(lib.gsplat_metrics_forward(_p(x), _p(y), _p(m), *dims, flags, _p(affine), _p(out), _p(scratch), _stream_ptr(dev)),
                   "gsplat_metrics_forward")


@torch.no_grad()
def image_metrics(pred, target, mask=None, colour_correct=False):
    """ImageMetrics(psnr, ssim, l1, mse, affine) of pred against target, [H, W, 3] or [B, H, W, 3], over the valid pixels of mask
    ([H, W] or [B, H, W], bool or uint8, nonzero = valid; None: every pixel): detached fp32 device tensors, [B] each or 0-d for an
    unbatched call; affine is [B, 3, 4] / [3, 4] with colour_correct=True (the fitted [M | t]; the metrics are then those of
    clamp(M pred + t, 0, 1)) and None without.  Per image, never a batch mean.  fp32 contiguous inputs are used as they stand, others
    are converted.  Runs on the caller's current stream and reads nothing back: two launches, four with the correction."""
    if type(colour_correct) is not bool:
        raise ValueError(f"colour_correct must be a bool, not {colour_correct!r}")
    batched, dims, x, y, m = _arguments(pred, target, mask)
    dev = x.device
    with torch.cuda.device(dev):
        out = torch.empty((dims[0], 4), dtype=torch.float32, device=dev)
        affine = torch.empty((dims[0], 3, 4), dtype=torch.float32, device=dev) if colour_correct else None
    _forward(x, y, m, dims, colour_correct, out, affine)
    if not batched:
        out, affine = out[0], (affine[0] if affine is not None else None)
    return ImageMetrics(out[..., 0], out[..., 1], out[..., 2], out[..., 3], affine)


def psnr(pred, target, mask=None):
    """-10 log10(mse) per image (data range 1; +inf for an image equal to its target)."""
    return image_metrics(pred, target, mask).psnr


def ssim(pred, target, mask=None):
    """The mean SSIM per image; with no mask and one image, 1 - the training loss's SSIM term."""
    return image_metrics(pred, target, mask).ssim


@torch.no_grad()
def fit_affine(pred, target, mask=None):
    """The colour correction alone: [3, 4] or [B, 3, 4] = [M | t] minimising sum_valid |M pred + t - target|^2 per image;
    exposure.apply(pred, affine) is the corrected image before the clamp.  Two launches on the current stream."""
    batched, dims, x, y, m = _arguments(pred, target, mask)
    lib = _abi.lib()
    dev = x.device
    with torch.cuda.device(dev):
        affine = torch.empty((dims[0], 3, 4), dtype=torch.float32, device=dev)
        scratch = _scratch(lib, dims, _abi.GSPLAT_METRICS_COLOUR_CORRECT, dev)
        _abi.check(lib.gsplat_metrics_fit_affine(_p(x), _p(y), _p(m), *dims, _p(affine), _p(scratch), _stream_ptr(dev)),
                   "gsplat_metrics_fit_affine")
    return affine if batched else affine[0]


# ---- evaluation of a model over views
_CAMERA = ('H', 'W', 'fx', 'fy', 'cx', 'cy')


def _check_views(views):
    """The views of evaluate() before anything is queued: each has an 'image' of [H, W, 3 or 4] and, if it has a 'mask', one of
    [H, W], bool or uint8 (ValueError otherwise).  Looks at shapes and dtypes only."""
    for k, v in enumerate(views):
        if 'image' not in v or v['image'] is None:
            raise ValueError(f"view {k} has no 'image': evaluate() needs the photograph of every view")
        shape = tuple(torch.as_tensor(v['image']).shape)
        h, w = int(v['H']), int(v['W'])
        if len(shape) != 3 or shape[:2] != (h, w) or shape[2] not in (3, 4):
            raise ValueError(f"view {k}: 'image' must be [{h}, {w}, 3] or [{h}, {w}, 4], got {list(shape)}")
        mask = v.get('mask')
        if mask is not None:
            mask = torch.as_tensor(mask)
            if tuple(mask.shape) != (h, w):
                raise ValueError(f"view {k}: 'mask' must be [{h}, {w}], got {list(mask.shape)}")
            if mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"view {k}: 'mask' must be bool or uint8 (nonzero = valid), not {mask.dtype}")


def aggregate(rows, idx, group=None):
    """The report of evaluate() from per-view rows.  `rows`: [n_local, 4] fp32 = (psnr, ssim, l1, mse) of THIS rank's views -- under a
    process group the views dp.shard_views(len(idx), rank, world) of the list, in that order; `idx`: the label of every view of the
    whole list, in view order.  The rows are all-gathered (uneven shards allowed), put back in view order and read in ONE copy to the
    host -- a single process reads the device that once; under a process group dp._all_gather_cat(equal=False) first reads the
    shard sizes it exchanges (one more small read).  The means are per-image means formed in float64 in view order, so every rank
    forms the same numbers from the same bits.  An image without a
    valid pixel (NaN) or equal to its target (psnr = +inf) enters the means as it is."""
    n = len(idx)
    world, rank = dp.world_and_rank(group)
    if world > 1:
        mine = dp.shard_views(n, rank, world)
        if rows.shape[0] != len(mine):
            raise ValueError(f"rank {rank} of {world} holds {len(mine)} of {n} views, got {rows.shape[0]} rows")
        rows = dp._all_gather_cat(rows.contiguous(), group, equal=False)
        order = [k for r in range(world) for k in dp.shard_views(n, r, world)]
    else:
        order = list(range(n))
    if tuple(rows.shape) != (n, 4):
        raise ValueError(f"{n} views need rows of [{n}, 4], got {list(rows.shape)}")
    got = rows.detach().cpu().double().tolist()                       # the one copy of the rows to the host
    table = [None] * n
    for row, k in zip(got, order):
        table[k] = row
    cols = list(zip(*table)) if n else [(), (), (), ()]

    def mean(col):
        total = 0.0
        for x in col:                                                  # float64, in view order
            total += x
        return total / n if n else float("nan")

    return {'n_views': n, 'psnr': mean(cols[0]), 'ssim': mean(cols[1]), 'l1': mean(cols[2]),
            'per_view': {'idx': list(idx), 'psnr': list(cols[0]), 'ssim': list(cols[1]), 'l1': list(cols[2]), 'mse': list(cols[3])}}


@torch.no_grad()
def evaluate(params, views, *, sh_degree=3, lowpass=0.0, antialias=False, background=None, colour_correct=False, group=None):
    """Render `views` forward-only and measure each against its photograph.  `params`: the six tensors as a dict, or a GaussianModel;
    `views`: the dicts Trainer.step takes (image, c2w, H, W, fx, fy, cx, cy).  An 'image' of [H, W, 4] is composited over the background
    (black without one) by its own alpha, exactly as the trainer's targets are; a 'mask' [H, W] (bool or uint8), if present, is the
    validity mask of the view.  sh_degree, lowpass, antialias, background: as for ops.render_frames, which renders each run of views
    with equal H, W, fx, fy, cx, cy through its two-stream pipeline -- no more than the pipeline's frames are alive at once, and each
    frame's metrics are computed on the device as it arrives.  colour_correct: as for image_metrics.

    Returns {'n_views', 'psnr', 'ssim', 'l1', 'per_view': {'idx', 'psnr', 'ssim', 'l1', 'mse'}}: Python floats, the means per-image
    means in float64 in view order; 'idx' is each view's 'idx', or its position in the list where it has none.  A single process
    reads the device once, at the end.  A view's photograph (and mask) that is not on the device yet is copied there when its frame
    arrives: from pageable host memory that copy blocks the host and holds back the queueing of the next frame, so keep the
    photographs on the device (or pinned) where the two-stream overlap of render_frames matters.  Under a process group there are two
    small reads more (the agreement that no rank failed, and the shard sizes of the all-gather).  Under a process group (`group`; None: the default group if initialised) every rank passes the SAME list, evaluates
    dp.shard_views of it and gets the same report, bit for bit: collective, every rank calls it."""
    views = list(views)
    _check_views(views)
    if type(colour_correct) is not bool:
        raise ValueError(f"colour_correct must be a bool, not {colour_correct!r}")
    p = harness._as_dict(params)
    dev = p['pos'].device
    world, rank = dp.world_and_rank(group)
    mine = dp.shard_views(len(views), rank, world)
    idx = [int(v['idx']) if v.get('idx') is not None else k for k, v in enumerate(views)]
    rows = torch.empty((len(mine), 4), dtype=torch.float32, device=dev)
    err = None
    try:
        start = 0
        while start < len(mine):                                        # one run of views with the same camera per render_frames call
            cam = tuple(views[mine[start]][k] for k in _CAMERA)
            stop = start + 1
            while stop < len(mine) and tuple(views[mine[stop]][k] for k in _CAMERA) == cam:
                stop += 1
            run = [views[k] for k in mine[start:stop]]

            def on_frame(j, image, run=run, first=start):
                v = run[j]
                target = torch.as_tensor(v['image']).to(dev)
                if target.shape[-1] == 4:
                    target = losses.composite_over(target[..., :3], target[..., 3], background if background is not None else (0.0, 0.0, 0.0))
                mask = v.get('mask')
                if mask is not None:
                    mask = torch.as_tensor(mask).to(dev)
                _, dims, x, y, m = _arguments(image, target, mask)
                with torch.cuda.device(dev):
                    affine = torch.empty((1, 12), dtype=torch.float32, device=dev) if colour_correct else None
                _forward(x, y, m, dims, colour_correct, rows[first + j:first + j + 1], affine)

            ops.render_frames(p['pos'], p['f_dc'], p['f_rest'], p['opacity_raw'], p['scale_raw'], p['q_raw'], [v['c2w'] for v in run],
                              int(cam[0]), int(cam[1]), float(cam[2]), float(cam[3]), float(cam[4]), float(cam[5]), on_frame=on_frame,
                              sh_degree=sh_degree, lowpass=lowpass, antialias=antialias, background=background)
            start = stop
    except Exception as e:                    # single process: the exception leaves as it is
        if world == 1:
            raise
        err = e
    if world > 1:
        # as in Trainer.step: what happened on this rank as ONE code and ONE agreement, so that a rank whose pose is off screen does
        # not leave its peers waiting in the all-gather -- every rank raises, or none does
        dp.raise_agreed(dp.agree_status(dp.status_of(err), group, device=dev), err, "evaluate")
    return aggregate(rows, idx, group)
