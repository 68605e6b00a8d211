"""One training iteration of the reference's loop on the MI355X ("next" row 2: optimiser / training step).

Follows scripts/train.py:446-569 statement by statement, on the fused pieces of this package:

    position learning rate (:446-457)          optim.position_lr
    zero_grad (:460)                           GaussianAdam.zero_grad
    per view of the batch (:471-527)           ops.render_gaussians (covariance build + SH folded in; the reference's
                                               build_sigma + evaluate_sh + render) -> losses.compute_loss_device,
                                               loss / batch size, accumulated
    backward (:530)                            per view, gradients accumulate in .grad (same sum, frees each view's buffers)
    [data parallel]                            dp.allreduce_gradients: sum over ranks (not in the reference)
    clip_grad_norm_(pos, 1.0) + step (:536-538) GaussianAdam.clip_grad_norm_ / .step (device-side coefficient, no host sync)
    densify / prune every `densification_interval` (:544-561)   model.GaussianModel.densify_and_prune + a fresh optimiser
                                               with the CURRENT position learning rate, as there
                                               (TrainConfig.densify_rule = "screen": densify_and_prune_screen on the screen-space
                                               statistics of the views since the last densification -- not in the reference)
    opacity reset every `opacity_reset_interval` (:564-569)     GaussianModel.reset_opacity
    [densify_rule = "mcmc", not in the reference; DESIGN.md §19]  a fixed budget cap_max instead of thresholds: the two regularisers join
                                               the complete gradients (mcmc.regularise), the position noise follows the step
                                               (mcmc.add_noise), and GaussianModel.refine_mcmc takes densification's place --
                                               rows are rewritten in place and the optimiser is KEPT; no opacity reset
    [filter3d > 0, not in the reference; DESIGN.md §23]       the 3D smoothing filter of Mip-Splatting: every view renders
                                               filter3d.apply(scale_raw, opacity_raw, filt) -- two leaves formed once per pass -- and ONE
                                               backward launch turns the leaves' complete gradients into scale_raw.grad / opacity_raw.grad
    [exposure, not in the reference; DESIGN.md §24]          per-view exposure compensation: each view's rendered colour goes through the
                                               affine transform of ITS training image (exposure.ExposureTable.apply_view) before the loss;
                                               the table has a gradient buffer, an Adam state and a learning-rate schedule of its own
    [bilagrid, not in the reference; DESIGN.md §25]          per-view bilateral grids: instead of one affine transform per image, a grid of
                                               them sliced at (x, y, luminance) (bilagrid.BilateralGridTable.apply_view), in the same
                                               place and with the same ordering; a total-variation term joins the table's gradient once

With data parallelism every rank holds the full model, renders its share of the batch's views and divides by the GLOBAL
number of views; the split noise of densification comes from a generator seeded identically on all ranks, so the
replicas stay bit-identical without a broadcast.
"""
import contextlib
import types
from dataclasses import dataclass

import torch

from . import _abi, bilagrid, dp, exposure, filter3d, losses, mcmc, metrics, ops, optim, poses


@dataclass
class TrainConfig:
    """Hyper-parameters of scripts/train.py:222-251 (same names, same defaults)."""
    iterations: int = 30000
    lr: float = 0.01
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30000
    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    lambda_l1: float = 0.8
    lambda_ssim: float = 0.2
    densify_until_iter: int = 15000
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    prune_opacity_threshold: float = 0.01
    max_grad: float = 0.01
    scale_threshold: float = 0.01
    checkpoint_interval: int = 1000
    densify_seed: int = 0
    # not a reference hyper-parameter: the views of one iteration alternate between this many HIP streams (1 or 2), so that the
    # latency-bound front of view k + 1 (projection, binning) runs beside the VALU-bound rasterisation of view k: ~10 % per view
    # at config 3.  Gradients accumulate in view order either way.
    view_streams: int = 2
    # not a reference hyper-parameter either: an iteration of ONE view on one process applies the Adam step of f_rest (81 % of the
    # parameters) inside the projection backward -- its gradient is neither written nor read back by the optimiser (0.07 ms of 1.0
    # at config 3); the same arithmetic as the optimiser's kernel, bit for bit.
    fold_rest_step: bool = True
    # an iteration of SEVERAL views on one process: the projection backward adds each view's gradients to one buffer itself
    # (ops.accumulate_grads) instead of autograd's accumulation pass per view -- the same sums in the same order.
    sum_views_in_kernel: bool = True
    # the densification criterion.  "reference": the reference's -- the world-space position gradient of the densification
    # iteration itself against max_grad.  "screen" (not in the reference; the paper's adaptive density control): the
    # gradient of the projected centre in NDC units, averaged over the views that saw the Gaussian since the last densification
    # (ops.DensifyStats), against densify_grad_threshold; Gaussians whose screen half-extent exceeded max_screen_size pixels are
    # pruned once iteration > opacity_reset_interval.
    densify_rule: str = "reference"
    densify_grad_threshold: float = 0.0002
    # densify_rule = "screen" only (ValueError under the other rules): the windows hold the ABSOLUTE-gradient statistic (AbsGS;
    # ops.densify_stats(absgrad=True)) -- per pixel, |dL/du| and |dL/dv| of the projected centre are added without their
    # signs, so a large blurry Gaussian whose pixels pull its centre in opposite directions is still seen.  The statistic is larger than
    # the signed one: densify_grad_threshold keeps its default but wants raising (the papers: 0.0004 - 0.0008).
    densify_absgrad: bool = False
    max_screen_size: float = 20.0
    # the paper's SH schedule (not in the reference, which always evaluates degree 3).  0: degree 3 always.  k > 0: iteration i renders
    # every view at SH degree min(3, i // k) (the paper: k = 1000) -- until a band is switched on its coefficients colour nothing and
    # get a zero gradient (ops.render_gaussians sh_degree).  A function of the iteration alone: checkpoints store
    # nothing for it and data-parallel ranks agree without a message.
    sh_degree_interval: int = 0
    # the screen-space low-pass of the paper's rasteriser and the opacity compensation of its antialiased variant (not in the reference;
    # ops.render_gaussians lowpass / antialias), given to every view.  The paper: lowpass = 0.3.  Without it a Gaussian
    # may shrink to a needle that one pixel centre sees.
    lowpass: float = 0.0
    antialias: bool = False
    # training with a background, an opacity target and depth maps (not in the reference).  All off by default, and
    # an iteration is then exactly the one above.  Any of them on makes the iteration an AUX PASS: the views are rendered with
    # ops.render_gaussians(aux=..., background=...) outside the folded step and the in-kernel view sum (those live on the composite
    # entries, which have no aux variant), and each view's loss is compute_loss_device + losses.aux_loss.
    #   background      None | (r, g, b) in [0, 1] | "random": the colour the render is composited over -- and a view's target too,
    #                   where the view has an alpha ('alpha', or a 4-channel 'image').  "random": one colour per iteration, a function
    #                   of (background_seed, iteration) alone, so its views and all ranks share it without a message.
    #   lambda_alpha    weight of mean |A - M| against the view's 'alpha'
    #   lambda_depth    weight of the composited depth residual |D - A Z| over the valid pixels of the view's 'depth'
    background: object = None
    background_seed: int = 0
    lambda_alpha: float = 0.0
    lambda_depth: float = 0.0
    # densify_rule = "mcmc" (not in the reference; Kheradmand et al. 2024): the model grows by mcmc_growth per refinement
    # up to cap_max Gaussians and stays there; every densification_interval iterations within [mcmc_start_iter, densify_until_iter)
    # the Gaussians with sigmoid(opacity_raw) <= mcmc_min_opacity are moved onto live ones.  Every iteration adds
    # mcmc_opacity_reg mean(opacity) + mcmc_scale_reg mean(scale) to the loss and, after the step, noise of size
    # lr_pos mcmc_noise_lr to the positions of the transparent Gaussians.  mcmc_seed keys that noise and the relocation draw (with the
    # iteration: the same on every rank).  All ignored by the other rules.
    cap_max: int = 1_000_000
    mcmc_start_iter: int = 500
    mcmc_min_opacity: float = 0.005
    mcmc_noise_lr: float = 5e5
    mcmc_opacity_reg: float = 0.01
    mcmc_scale_reg: float = 0.01
    mcmc_growth: float = 1.05
    mcmc_seed: int = 0
    # the sparse optimiser step (not in the reference, which steps every row with dense Adam; the INRIA trainer's sparse_adam, gsplat's
    # visible_adam / SelectiveAdam): only the Gaussians that at least one view of the iteration -- on any rank -- binned
    # are stepped; every other row keeps its parameter and both moments bit for bit instead of drifting on momentum left by other views.
    # A bool, else ValueError; not with densify_rule = "mcmc" (its regularisers give every row a gradient and its noise step assumes a
    # dense optimiser).  While it is on the folded f_rest step is not used (fold_rest_step is ignored): that kernel steps every row, and a
    # sparse variant of it is a follow-up.  Several views on one process take the data-parallel route of the SH gradients
    # (dp.FactoredExchange without a collective) instead of sum_views_in_kernel, so that ranks with one view each end with the bits of one
    # process given all of them.  Off by default: where nearly every Gaussian is in view it only costs the fold.
    sparse_adam: bool = False
    # the 3D smoothing filter of Mip-Splatting (not in the reference; filter3d.py), the companion of lowpass / antialias.
    # filter3d = s > 0 (the paper: 0.2; 0: off): Gaussian k is rendered convolved with an isotropic Gaussian of standard deviation
    # sqrt(s) t_k, t_k the smallest z / focal over the training cameras that see it -- the cameras of the WHOLE training set, given to
    # Trainer(cameras=...).  The limit is recomputed every filter3d_interval iterations and whenever the number of Gaussians changed; a
    # camera sees a Gaussian beyond filter3d_near whose projection lies inside the image widened by filter3d_margin of its size.
    # Densification, pruning, the opacity reset and the sparse optimiser keep acting on the RAW parameters and the raw gradients, as
    # Mip-Splatting's do.  Not with densify_rule = "mcmc" (its relocation and regularisers are written for unfiltered opacity and scale).
    filter3d: float = 0.0
    filter3d_interval: int = 100
    filter3d_near: float = 0.2
    filter3d_margin: float = 0.15
    # per-view exposure compensation (not in the reference; the INRIA trainer's exposure optimisation, gsplat's appearance transform;
    # exposure.py).  exposure = True (a bool, else ValueError): every training image has an affine colour transform
    # [M | t], the identity at the start, that its view's rendered colour -- after the background composite; the depth and opacity maps
    # are untouched -- goes through before the loss.  The table of transforms (Trainer.exposure) is trained beside the model by an Adam
    # of its own (eps 1e-8, dense) at the learning rate optim.position_lr gives for the four numbers below -- the INRIA trainer's
    # defaults, taken from there and not measured here.  A view names its image by its integer 'idx' (data.GaussianDataset supplies it);
    # the table has Trainer(exposure_views=V) rows, len(cameras) by default.  The op sits outside the render: every route of the
    # gradients, every densify rule, sparse_adam, filter3d and the aux passes work unchanged, and a fresh optimiser after a
    # densification touches neither the table nor its moments.  Novel views are rendered without it.  Off by default, and an iteration
    # is then exactly the one above.
    exposure: bool = False
    exposure_lr_init: float = 0.01
    exposure_lr_final: float = 0.001
    exposure_lr_delay_mult: float = 0.0
    exposure_lr_max_steps: int = 30000
    # per-view bilateral grids (not in the reference; gsplat's use_bilateral_grid; bilagrid.py).  bilagrid = True (a bool,
    # else ValueError): every training image has a grid of bilagrid_shape = (X, Y, L) affine colour transforms, the identity at the start,
    # sliced at (pixel x, pixel y, pixel luminance) -- what an in-camera ISP does locally (tone mapping, vignetting) -- in the place of
    # the exposure transform, which it contains: both at once is a ValueError (two tables on one colour are ill-conditioned).  The table
    # (Trainer.bilagrid; Trainer(bilagrid_views=V) rows, len(cameras) by default) is trained by an Adam of its own (eps 1e-15, dense) at
    # the learning rate optim.position_lr gives for the four numbers below, and bilagrid_tv times its total variation joins its gradient
    # once per iteration.  The defaults follow gsplat's trainer -- taken from there and not measured here.  Everything said of exposure
    # above about 'idx', the routes, the densify rules and novel views holds.  Off by default, and an iteration is then exactly the one
    # above.
    bilagrid: bool = False
    bilagrid_shape: tuple = (16, 16, 8)
    bilagrid_tv: float = 10.0
    bilagrid_lr_init: float = 0.002
    bilagrid_lr_final: float = 0.00002
    bilagrid_lr_delay_mult: float = 0.0
    bilagrid_lr_max_steps: int = 30000
    # per-view camera-pose corrections (not in the reference; gsplat's pose_opt, nerfstudio's camera optimiser; poses.py).
    # pose_opt = True (a bool, else ValueError): every training camera has a rigid correction of nine numbers, zero at the start, that
    # its given c2w is composed with before the render (poses.PoseTable.apply_view); the render's pose gradient trains
    # it.  The table (Trainer.poses; Trainer(pose_views=V) rows, len(cameras) by default) is trained by an Adam of its own (eps 1e-8,
    # dense) at the learning rate optim.position_lr gives for the four numbers below, and pose_reg times the table joins its gradient
    # once per iteration.  The defaults are gsplat's (pose_opt_lr, pose_opt_reg, a decay to 1 %) -- taken from there, not measured here
    # and NOT scaled by a scene extent.  A view names its camera by its integer 'idx'.  Allowed together with exposure or bilagrid.  A
    # view of such a pass is a pose frame: it takes the separate library calls, under the factored exchange where the pass has one
    # and under no route otherwise (fold_rest_step and sum_views_in_kernel do not apply).  filter3d's camera limits and
    # prune_by_contribution keep using the GIVEN poses.  Off by default, and an iteration is then exactly the one above.
    pose_opt: bool = False
    pose_lr_init: float = 1e-5
    pose_lr_final: float = 1e-7
    pose_lr_delay_mult: float = 0.0
    pose_lr_max_steps: int = 30000
    pose_reg: float = 1e-6

    def __post_init__(self):
        _validate(self)


def _need_finite(cfg, *names, at_least=0):
    """The numeric predicate of the checks below, for each of the fields `names`: an int or a float -- not a bool --, not NaN, finite
    and >= at_least."""
    for name in names:
        x = getattr(cfg, name)
        if not (isinstance(x, (int, float)) and not isinstance(x, bool) and at_least <= x < float("inf")):
            raise ValueError(f"{name} must be a finite number >= {at_least}, not {x!r}")


def _validate(cfg, cameras=False, exposure_views=None, bilagrid_views=None, pose_views=None):
    """Every check of a TrainConfig, in ONE order: ValueError for the first field that fails.  TrainConfig(...) itself -- the call
    without `cameras` -- refuses only the absgrad, sparse_adam, filter3d, exposure, bilagrid and pose_opt groups.  A Trainer checks
    every field (the six groups again: the fields of a config can be set after it is made) together with what its constructor was
    given -- `cameras` (None: it was given none), `exposure_views`, `bilagrid_views` and `pose_views` --, and gets back what it keeps
    of the checks: the filter keyword arguments of its renders and the background in the form background() returns."""
    trainer = cameras is not False
    if trainer:
        if cfg.densify_rule not in ("reference", "screen", "mcmc"):
            raise ValueError(f"densify_rule must be 'reference', 'screen' or 'mcmc', not {cfg.densify_rule!r}")
        # the MCMC fields: a value the rule cannot run with is refused whatever the rule is
        if type(cfg.cap_max) is not int or not 1 <= cfg.cap_max < 2 ** 31:
            raise ValueError(f"cap_max must be an integer in [1, 2^31), not {cfg.cap_max!r}")
        if type(cfg.mcmc_start_iter) is not int or cfg.mcmc_start_iter < 0:
            raise ValueError(f"mcmc_start_iter must be an integer >= 0, not {cfg.mcmc_start_iter!r}")
        if not (isinstance(cfg.mcmc_min_opacity, float) and 0.0 < cfg.mcmc_min_opacity < 1.0):
            raise ValueError(f"mcmc_min_opacity must be a float in (0, 1), not {cfg.mcmc_min_opacity!r}")
        _need_finite(cfg, "mcmc_noise_lr", "mcmc_opacity_reg", "mcmc_scale_reg")
        _need_finite(cfg, "mcmc_growth", at_least=1)
        if type(cfg.mcmc_seed) is not int or not 0 <= cfg.mcmc_seed < 2 ** 64:
            raise ValueError(f"mcmc_seed must be an integer in [0, 2^64), not {cfg.mcmc_seed!r}")
    # ---- the six groups TrainConfig(...) refuses too
    if type(cfg.densify_absgrad) is not bool:
        raise ValueError(f"densify_absgrad must be a bool, not {cfg.densify_absgrad!r}")
    if cfg.densify_absgrad and cfg.densify_rule != "screen":
        raise ValueError(f"densify_absgrad=True needs densify_rule='screen' (the other rules read no screen-space statistic), not {cfg.densify_rule!r}")
    if type(cfg.sparse_adam) is not bool:
        raise ValueError(f"sparse_adam must be a bool, not {cfg.sparse_adam!r}")
    if cfg.sparse_adam and cfg.densify_rule == "mcmc":
        raise ValueError("sparse_adam=True is not available with densify_rule='mcmc' (its regularisers give every row a gradient and its "
                         "noise step assumes a dense optimiser)")
    _need_finite(cfg, "filter3d", "filter3d_near", "filter3d_margin")
    if type(cfg.filter3d_interval) is not int or cfg.filter3d_interval < 1:
        raise ValueError(f"filter3d_interval must be an integer >= 1, not {cfg.filter3d_interval!r}")
    if cfg.filter3d > 0 and cfg.densify_rule == "mcmc":
        raise ValueError("filter3d > 0 is not available with densify_rule='mcmc' (its relocation and its regularisers are written for "
                         "unfiltered opacity and scale)")
    if cfg.filter3d > 0 and cameras is None:
        raise ValueError("filter3d > 0 needs the cameras of the whole training set: Trainer(model, config, group, cameras=views)")
    if type(cfg.exposure) is not bool:
        raise ValueError(f"exposure must be a bool, not {cfg.exposure!r}")
    if type(cfg.bilagrid) is not bool:
        raise ValueError(f"bilagrid must be a bool, not {cfg.bilagrid!r}")
    bilagrid.check_shape(cfg.bilagrid_shape)
    if cfg.bilagrid and cfg.exposure:
        raise ValueError("bilagrid=True is not available with exposure=True (the grid at the identity contains the global affine, and "
                         "two tables on one colour are ill-conditioned)")
    if type(cfg.pose_opt) is not bool:
        raise ValueError(f"pose_opt must be a bool, not {cfg.pose_opt!r}")
    if not trainer:
        return None
    # ---- the rest is the Trainer's alone
    for name, n_views, views_kw in (("exposure", exposure_views, "exposure_views"), ("bilagrid", bilagrid_views, "bilagrid_views"),
                                    ("pose_opt", pose_views, "pose_views")):
        if getattr(cfg, name) and n_views is None and cameras is None:
            raise ValueError(f"{name}=True needs the number of training images: Trainer(model, config, group, cameras=views) or "
                             f"Trainer(..., {views_kw}=V)")
    _need_finite(cfg, "bilagrid_tv", "bilagrid_lr_init", "bilagrid_lr_final", "bilagrid_lr_delay_mult")
    if type(cfg.bilagrid_lr_max_steps) is not int or cfg.bilagrid_lr_max_steps < 1:
        raise ValueError(f"bilagrid_lr_max_steps must be an integer >= 1, not {cfg.bilagrid_lr_max_steps!r}")
    _need_finite(cfg, "pose_reg", "pose_lr_init", "pose_lr_final", "pose_lr_delay_mult")
    if type(cfg.pose_lr_max_steps) is not int or cfg.pose_lr_max_steps < 1:
        raise ValueError(f"pose_lr_max_steps must be an integer >= 1, not {cfg.pose_lr_max_steps!r}")
    if type(cfg.sh_degree_interval) is not int or cfg.sh_degree_interval < 0:
        raise ValueError(f"sh_degree_interval must be an integer >= 0, not {cfg.sh_degree_interval!r}")
    filter_kw = _abi.filter_kwargs(cfg.lowpass, cfg.antialias)      # (ValueError for a mode the kernels cannot do)
    background = _check_background(cfg.background)
    if type(cfg.background_seed) is not int:
        raise ValueError(f"background_seed must be an integer, not {cfg.background_seed!r}")
    _need_finite(cfg, "lambda_alpha", "lambda_depth")
    return filter_kw, background


def _check_background(background):
    """TrainConfig.background as the trainer keeps it: None, "random" or a tuple of three floats in [0, 1] (ValueError otherwise)."""
    if background is None or (isinstance(background, str) and background == "random"):
        return background
    try:
        vals = tuple(float(x) for x in background) if not isinstance(background, str) else None
    except (TypeError, ValueError):
        vals = None
    if vals is None or len(vals) != 3 or not all(0.0 <= x <= 1.0 for x in vals):
        raise ValueError(f"background must be None, 'random' or three numbers (r, g, b) in [0, 1], not {background!r}")
    return vals


def _keyed_generator(seed, iteration):
    """A CPU generator keyed by (seed, iteration): the same stream of numbers on every rank and in a repeated pass, with no message."""
    g = torch.Generator()
    g.manual_seed(seed * 1000003 + int(iteration))
    return g


def _add_in_view_order(acc, per_view, main):
    """acc += the views' loss vectors, on the caller's stream `main` (None: the views ran on it), in view order."""
    for vals in per_view:
        if main is not None:
            vals.record_stream(main)              # (allocated on the view's stream)
        acc += vals


def _total(acc, acc_aux):
    """The loss of a pass from its two sum vectors (acc_aux None: no aux pass)."""
    return acc[2] if acc_aux is None else acc[2] + acc_aux[2]


_side_streams = {}           # per device: the two streams the views of an iteration alternate between (TrainConfig.view_streams)
_NO_CONTEXT = contextlib.nullcontext()      # (reusable: what a view enters where it has no stream or no statistics record of its own)
# the route of a pass that has none: autograd gets every gradient, and its consumer only says so
_NO_ROUTE = contextlib.nullcontext(types.SimpleNamespace(route_kind=ops.PLAIN))


class Trainer:
    """Owns the optimiser of a GaussianModel and runs iterations.  `group`: torch.distributed group for data parallelism
    by camera view (None = default group if initialised, else single process).  `cameras` (TrainConfig.filter3d > 0 only): the view
    dicts of the WHOLE training set -- only c2w, H, W, fx, fy, cx, cy are read; under data parallelism every rank passes the same
    list, so the filter is the same bits on every rank without a message.

    With filter3d > 0 the views are rendered from the filtered scale and opacity (filter3d.apply) and `self.filter3d` holds the
    per-Gaussian filter; densify_and_prune*, reset_opacity, prune_by_contribution's removal and the sparse optimiser keep acting on the
    RAW parameters and the raw gradients (the chain rule through the filter is applied before them), as Mip-Splatting's do.

    With exposure = True `self.exposure` is the exposure.ExposureTable of `exposure_views` rows (default: len(cameras)), one per training
    image, else None; under data parallelism every rank holds the whole table and the replicas stay bit-identical.  It is not part of
    harness.save_checkpoint's file set: it travels through its own state_dict() / load_state_dict().

    With bilagrid = True `self.bilagrid` is the bilagrid.BilateralGridTable of `bilagrid_views` rows (default: len(cameras)), else None;
    everything said of the exposure table holds for it.

    With pose_opt = True `self.poses` is the poses.PoseTable of `pose_views` rows (default: len(cameras)), one per training camera, else
    None; everything said of the exposure table holds for it, and it may stand beside either colour table."""

    def __init__(self, model, config=None, group=None, cameras=None, exposure_views=None, bilagrid_views=None, pose_views=None):
        self.model = model
        self.cfg = config or TrainConfig()
        self.group = group
        self._filter_kw, self._background = _validate(self.cfg, cameras, exposure_views, bilagrid_views, pose_views)
        # the per-image table a view's rendered colour goes through before the loss (the config check allows one at the most)
        self.exposure = self.bilagrid = self._table = None
        if self.cfg.exposure or self.cfg.bilagrid:
            n_views = exposure_views if self.cfg.exposure else bilagrid_views
            if n_views is None:
                n_views = len(cameras)
            if self.cfg.exposure:                                                    # (either: ValueError unless n_views is an integer >= 1)
                self._table = self.exposure = exposure.ExposureTable(n_views, model.pos.device)
            else:
                self._table = self.bilagrid = bilagrid.BilateralGridTable(n_views, model.pos.device, shape=self.cfg.bilagrid_shape)
        # the table of pose corrections a view's c2w is composed with before the render; the tables of a pass, in ONE fixed order --
        # the colour table, then the poses: the order of their all-reduces on every rank
        self.poses = None
        if self.cfg.pose_opt:
            self.poses = poses.PoseTable(len(cameras) if pose_views is None else pose_views, model.pos.device)
        self._tables = [t for t in (self._table, self.poses) if t is not None]
        # filter3d: the camera records (host copy; on the model's device from the first step on) and the per-Gaussian filter
        self._cameras = filter3d.pack_cameras(cameras, "cpu") if cameras is not None and self.cfg.filter3d > 0 else None
        self._cameras_dev = None
        self.filter3d = None
        self.optimizer = self._new_optimizer(self.cfg.position_lr_init)
        # densify_rule = "screen": the statistics since the last densification (None until the first such step; not stored in
        # checkpoints: a resumed run starts its window at zero), and one pass record per view of an iteration
        self.densify_stats = None
        self._pass_stats = []
        self._pass_dirty = False
        # sparse_adam: the Gaussians this iteration's views binned, one record per model size
        self.visible = None

    def _new_optimizer(self, pos_lr):
        c = self.cfg
        groups = optim.reference_param_groups(self.model, position_lr_init=pos_lr, feature_lr=c.feature_lr,
                                              opacity_lr=c.opacity_lr, scaling_lr=c.scaling_lr, rotation_lr=c.rotation_lr)
        return optim.GaussianAdam(groups, lr=c.lr, eps=1e-15)

    def _position_lr(self, iteration):
        c = self.cfg
        return optim.position_lr(iteration, c.position_lr_init, c.position_lr_final, c.position_lr_delay_mult, c.position_lr_max_steps)

    def _update_filter3d(self, iteration, dev):
        """self.filter3d for this iteration: recomputed (one library call, nothing read back) when it is missing or has another length
        than the model -- after a densification, a prune or a model swap -- and at every filter3d_interval-th iteration."""
        c, m = self.cfg, self.model
        if self._cameras_dev is None or self._cameras_dev.device != dev:
            self._cameras_dev = self._cameras.to(dev)
        f = self.filter3d
        if f is None or f.shape[0] != m.get_num_gaussians() or f.device != dev or iteration % c.filter3d_interval == 0:
            self.filter3d = filter3d.compute(m.pos, self._cameras_dev, s=c.filter3d, near=c.filter3d_near, margin=c.filter3d_margin)
        return self.filter3d

    def _view_streams(self, dev):
        key = (dev.type, dev.index)
        got = _side_streams.get(key)
        if got is None:
            got = _side_streams[key] = tuple(torch.cuda.Stream(dev) for _ in range(2))
            # the parameters' AccumulateGrad nodes live on the caller's stream and the views' backward passes on the side streams: that
            # is the point (the engine orders the two); torch would warn about it in every iteration
            quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
            if quiet is not None:
                quiet(False)
        return got

    def _prepare_stats(self, dev, n_views):
        """The pass records of this iteration's views: one per VIEW, merged into self.densify_stats in view order once the pass is
        agreed good -- so no two streams ever read-modify-write the same rows, a repeated pass counts nothing twice, and the sums
        are the same bits whatever streams the views ran on."""
        n = self.model.get_num_gaussians()
        if self.densify_stats is None or self.densify_stats.data.shape[0] != n:
            self.densify_stats = ops.DensifyStats(n, dev)
        if self._pass_stats and self._pass_stats[0].data.shape[0] != n:
            self._pass_stats, self._pass_dirty = [], False
        if self._pass_dirty:                      # an exception left the last pass half way
            self._clear_pass_stats(dev)
        while len(self._pass_stats) < n_views:
            self._pass_stats.append(ops.DensifyStats(n, dev))
        return self._pass_stats[:n_views]

    def _clear_pass_stats(self, dev):
        main = torch.cuda.current_stream(dev)
        for st in _side_streams.get((dev.type, dev.index), ()):
            main.wait_stream(st)
        for rec in self._pass_stats:
            rec.data.zero_()
        self._pass_dirty = False

    def _densify_generator(self, iteration):
        return _keyed_generator(self.cfg.densify_seed, iteration)      # the same stream of split noise on every rank

    def background(self, iteration):
        """The background colour of iteration `iteration` (TrainConfig.background): None, the configured colour, or -- "random" --
        three uniform numbers from a CPU generator keyed by (background_seed, iteration): the same on every rank and in a repeated
        pass, with no message."""
        if self._background != "random":
            return self._background
        return tuple(torch.rand(3, generator=_keyed_generator(self.cfg.background_seed, iteration)).tolist())

    def _view_targets(self, v, dev, bg, aux_pass):
        """(image, alpha, depth) targets of one view, on the device.  An aux pass: the image over the background where the view has an
        alpha ('alpha', or a 4-channel 'image'; over black without a background), alpha / depth None unless their weight is > 0 --
        and then a view without one is an error of that view (ValueError).  Any other pass reads neither 'alpha' nor 'depth' (both
        weights are 0 there): a 4-channel image goes over black by its own alpha, and that is all."""
        c = self.cfg
        image = torch.as_tensor(v['image']).to(dev)
        alpha = v.get('alpha') if aux_pass else None
        if alpha is not None:
            alpha = torch.as_tensor(alpha).to(dev)
        if image.shape[-1] == 4:
            if alpha is None:
                alpha = image[..., 3]
            image = image[..., :3]
        if c.lambda_alpha > 0 and alpha is None:
            raise ValueError("lambda_alpha > 0 needs an 'alpha' (or a 4-channel 'image') in every view")
        if c.lambda_depth > 0 and v.get('depth') is None:
            raise ValueError("lambda_depth > 0 needs a 'depth' in every view")
        if alpha is not None:
            image = losses.composite_over(image, alpha, bg if bg is not None else (0.0, 0.0, 0.0))
        depth = torch.as_tensor(v['depth']).to(dev) if c.lambda_depth > 0 else None
        return image, (alpha if c.lambda_alpha > 0 else None), depth

    def sh_degree(self, iteration):
        """The SH degree iteration `iteration` renders at (TrainConfig.sh_degree_interval)."""
        k = self.cfg.sh_degree_interval
        return 3 if k == 0 else max(0, min(3, int(iteration) // k))

    def prune_by_contribution(self, iteration, views, min_weight_max=None, keep_fraction=None):
        """Contribution-based pruning: accumulate ops.contribution over this rank's `views` (the dicts step() takes;
        the trainer's lowpass / antialias, the SH degree of `iteration`), all-reduce the integer record over the group when
        world > 1 -- every rank then decides from the same bits --, GaussianModel.prune_by_contribution(stats, min_weight_max,
        keep_fraction), and a fresh optimiser at the position learning rate of `iteration`, exactly as after a densification; the
        densification window restarts over the new set.  Returns {'removed', 'gaussians', 'frames'}.  Not part of step().  Data parallel:
        collective -- every rank calls it; a failure on one rank (an off-screen pose) raises on every rank before anything is pruned."""
        if min_weight_max is None and keep_fraction is None:
            raise ValueError("prune_by_contribution needs min_weight_max, keep_fraction or both")
        c, m = self.cfg, self.model
        dev = m.pos.device
        stats = ops.ContributionStats(m.get_num_gaussians(), dev)
        scale_in, opacity_in = m.scale_raw, m.opacity_raw
        if c.filter3d > 0:                                     # what the views of step() are rendered from
            baked = filter3d.bake(m, self._update_filter3d(iteration, dev))
            scale_in, opacity_in = baked["scale_raw"], baked["opacity_raw"]
        groups = {}
        for v in views:                                        # poses that share a camera go through one call
            cam = (int(v['H']), int(v['W']), float(v['fx']), float(v['fy']), float(v['cx']), float(v['cy']))
            groups.setdefault(cam, []).append(torch.as_tensor(v['c2w'], dtype=torch.float32).to(dev))
        world, err = dp.world_and_rank(self.group)[0], None
        try:
            for cam, poses in groups.items():
                ops.contribution(m.pos, m.f_dc, m.f_rest, opacity_in, scale_in, m.q_raw, poses, *cam, sh_degree=self.sh_degree(iteration),
                                 stats=stats, **self._filter_kw)
        except Exception as e:                # single process: the exception leaves as it is
            if world == 1:
                raise
            err = e
        if world > 1:
            # as in step(): what happened on this rank as ONE code and ONE agreement, so that a rank whose pose is off screen does not
            # leave its peers waiting in the all-reduce -- every rank raises, or none does, and nothing is pruned anywhere
            dp.raise_agreed(dp.agree_status(dp.status_of(err), self.group, device=dev), err, "prune_by_contribution")
            stats.all_reduce(self.group)
        removed = m.prune_by_contribution(stats, min_weight_max=min_weight_max, keep_fraction=keep_fraction)
        self.optimizer = self._new_optimizer(self._position_lr(iteration))
        if self.densify_stats is not None:
            self.densify_stats.reset(m.get_num_gaussians())
        self._pass_stats, self._pass_dirty = [], False
        return {'removed': removed, 'gaussians': m.get_num_gaussians(), 'frames': stats.frames}

    @torch.no_grad()
    def evaluate(self, views, iteration=None, colour_correct=None, refined_poses=False):
        """Per-image PSNR, SSIM and L1 of held-out `views` (the dicts step() takes, with their photographs):
        metrics.evaluate of the model as step() renders it -- the trainer's lowpass / antialias, the SH degree of `iteration` (None:
        degree 3), the filtered scale and opacity when filter3d > 0 (filter3d.apply, without gradient) -- over the trainer's group.
        The views are rendered over the trainer's background colour; background = "random" evaluates over BLACK (a report must not
        depend on a draw).  The exposure / bilateral-grid tables are NOT applied -- a held-out view has no row in them -- so with
        either on the model is only known up to a colour transform per image: colour_correct (None: cfg.exposure or cfg.bilagrid) fits
        that transform per view before measuring.  refined_poses = True (pose_opt only, else ValueError): a view that carries 'idx' --
        a TRAINING view -- is rendered at its corrected pose (poses.PoseTable.c2w); held-out views, which carry none, are always
        rendered at their given poses (there is no test-time pose alignment).  Returns metrics.evaluate's report.  Not part of step(); parameters, gradients, the
        optimiser, the statistics windows, the visible set and both tables are left bit for bit as they were.  Data parallel:
        collective -- every rank calls it with the same list."""
        c, m = self.cfg, self.model
        dev = m.pos.device
        params = m
        if c.filter3d > 0:
            filt = self.filter3d                   # (a local one where step() has not made it yet: nothing of the trainer changes here)
            if filt is None or filt.shape[0] != m.get_num_gaussians() or filt.device != dev:
                filt = filter3d.compute(m.pos, self._cameras.to(dev), s=c.filter3d, near=c.filter3d_near, margin=c.filter3d_margin)
            params = filter3d.bake(m, filt)
        if colour_correct is None:
            colour_correct = bool(c.exposure or c.bilagrid)
        if type(refined_poses) is not bool:
            raise ValueError(f"refined_poses must be a bool, not {refined_poses!r}")
        if refined_poses:
            if self.poses is None:
                raise ValueError("refined_poses=True needs a trainer with pose_opt=True")
            named = [k for k, v in enumerate(views) if v.get('idx') is not None]
            if named:                              # ONE launch for all of them; the callers' dicts are left as they are
                c2ws = torch.stack([torch.as_tensor(views[k]['c2w'], dtype=torch.float32) for k in named]).to(dev)
                refined = self.poses.c2w(c2ws, [views[k]['idx'] for k in named])
                views = list(views)
                for j, k in enumerate(named):
                    views[k] = {**views[k], 'c2w': refined[j]}
        return metrics.evaluate(params, views, sh_degree=3 if iteration is None else self.sh_degree(iteration),
                                background=None if self._background == "random" else self._background, colour_correct=colour_correct,
                                group=self.group, **self._filter_kw)

    def step(self, iteration, views, global_views=None, views_per_rank=None):
        """One iteration on this rank's `views` (list of dicts with image [H,W,3], c2w [4,4], H, W, fx, fy, cx, cy — the
        sample dict of data.GaussianDataset).  Data parallel: the ranks may hold different numbers of views; how many each
        holds is agreed COLLECTIVELY (it selects the exchange's sequence of collectives): pass `views_per_rank` (one count
        per rank, the same list on every rank) or leave it None and the counts are exchanged with one tiny all-gather.
        `global_views` (views of the whole batch over all ranks) is only checked against that.  Returns {'loss', 'l1',
        'ssim'} as device scalars (this rank's share, already divided by the global batch), 'gaussians', 'lr_pos',
        'densified', 'sh_degree' (the SH degree the views were rendered at).
        An aux pass (TrainConfig.background / lambda_alpha / lambda_depth): a view may also carry 'alpha' [H, W] in [0, 1] (an
        'image' of [H, W, 4] is shorthand for rgb + alpha) and 'depth' [H, W] (camera-space z; <= 0 or non-finite: no data); the
        dict also has 'l_alpha' and 'l_depth' (device scalars like 'l1', 0 for a term that is off) and 'loss' is the whole total.
        Otherwise those keys of a view are ignored, except that a 4-channel image is composited over black.
        exposure = True: every view carries 'idx', the integer in [0, V) of its training image (else ValueError, before anything is
        queued); the dict also has 'lr_exposure', the learning rate the table was stepped at.
        bilagrid = True: 'idx' likewise; the dict also has 'lr_bilagrid' and 'tv', the weighted total-variation term bilagrid_tv tv as a
        device scalar -- it joined the table's gradient and is NOT part of 'loss', whose meaning stays.
        pose_opt = True: 'idx' likewise (valid for every table of the trainer); the dict also has 'lr_pose'."""
        c, m = self.cfg, self.model
        # ---- the facts of this step
        rows = None
        for table in self._tables:                 # (one 'idx' per view names its row in every table: valid for each)
            rows = [table.check_index(v.get('idx')) for v in views]
        aux_maps = c.lambda_alpha > 0 or c.lambda_depth > 0
        aux = aux_maps if aux_maps or self._background is not None else None     # None: no aux pass; else: does it render the maps?
        bg = self.background(iteration)
        sh_degree = self.sh_degree(iteration)
        render_kw = dict(self._filter_kw)          # (without a schedule, a filter or an aux pass the render call is the reference's)
        if sh_degree != 3:
            render_kw['sh_degree'] = sh_degree
        if aux is not None:
            render_kw.update(aux=aux, background=bg)
        world, dev = dp.world_and_rank(self.group)[0], m.pos.device
        even, n_global = dp.agree_on_views(len(views), self.group, views_per_rank, device=dev)
        if global_views is not None and int(global_views) != n_global:
            raise ValueError(f"global_views={global_views}, but the ranks hold {n_global} views in all")
        pos_lr = self._position_lr(iteration)
        self.optimizer.param_groups[0]['lr'] = pos_lr
        screen = c.densify_rule == "screen" and iteration < c.densify_until_iter
        pass_stats = self._prepare_stats(dev, len(views)) if screen else None
        if c.sparse_adam and (self.visible is None or self.visible.data.shape[0] != m.get_num_gaussians() or self.visible.data.device != dev):
            self.visible = ops.VisibleSet(m.get_num_gaussians(), dev)
        if c.filter3d > 0:
            self._update_filter3d(iteration, dev)
        # ---- the pass: repeated, on every rank or on none, while a view outgrows the pair buffers
        for attempt in range(4):
            consumer, checks, error, leaves, acc, acc_aux = self._run_pass(views, rows, n_global, render_kw, aux, bg, pass_stats,
                                                                           world, even, sh_degree)
            if self._settle_pass(len(views), consumer, checks, error, pass_stats, world) == dp.STATUS_OK:
                break
        else:
            raise RuntimeError("the pair buffers overflowed four times in a row")
        # ---- the update, the refinement, the result
        table_out, reg = self._update(iteration, consumer, leaves, acc, acc_aux, world)
        densified = self._refine(iteration, pos_lr, screen, world)
        out = {'loss': reg[2] if reg is not None else _total(acc, acc_aux), 'l1': acc[0], 'ssim': acc[1],
               'gaussians': m.get_num_gaussians(), 'lr_pos': pos_lr, 'densified': densified, 'sh_degree': sh_degree}
        if reg is not None:
            out.update(reg_opacity=reg[0], reg_scale=reg[1])
        if aux is not None:
            out.update(l_alpha=acc_aux[0], l_depth=acc_aux[1])
        out.update(table_out)
        return out

    def _choose_route(self, world, n_views, aux_pass, params, even, sh_degree):
        """The route of a pass's gradients (ops.gradient_route), chosen ONCE per attempt: a context that yields the consumer.  Whatever
        depends on the choice afterwards reads the consumer's route_kind ("none" below: _NO_ROUTE, kind PLAIN).  First match:

            several ranks                                            FACTORED  the SH gradients in factored form (dp.FactoredExchange,
                                                                               2.6x fewer bytes over xGMI at 8 views)
            sparse_adam, several views                               FACTORED  the same exchange WITHOUT a collective: the SH gradients are
                                                                               rounded as a group of ranks rounds them, so a group steps the
                                                                               bits of one process given all its views
            an aux pass, a pose_opt pass                             none      its frames take the separate library calls (the routes below
                                                                               live on the composite entries, which have no aux and no
                                                                               pose variant)
            one view, fold_rest_step, not sparse_adam                FOLDED    the Adam step of f_rest inside the backward (that kernel steps
                                                                               every row: fold_rest_step is ignored under sparse_adam)
            several views, sum_views_in_kernel                       SUMMED    the views' sum formed by the backward (ops.accumulate_grads)
            anything else                                            none"""
        c = self.cfg
        if world > 1 or (c.sparse_adam and n_views > 1):
            return dp.FactoredExchange(params, world_views=1, group=self.group, equal_views=even, sh_degree=sh_degree)
        if aux_pass or self.poses is not None:
            return _NO_ROUTE
        if n_views == 1 and c.fold_rest_step and not c.sparse_adam:
            return self.optimizer.fused_rest_update(self.model.f_rest)
        if n_views > 1 and c.sum_views_in_kernel:
            return ops.accumulate_grads(params)
        return _NO_ROUTE

    def _run_pass(self, views, rows, n_global, render_kw, aux, bg, pass_stats, world, even, sh_degree):
        """One attempt at the pass: every view rendered and back-propagated, the losses summed.  Returns (the consumer of the gradient
        route, the deferred checks, the exception that stopped the pass on a rank of several or None, the (scale, opacity) the views
        were rendered from, the loss sums [l1, ssim, total], the aux sums [l_alpha, l_depth, total] or None).
        Everything a pass adds into is zeroed HERE, in every attempt, on the caller's stream and before the side streams wait on it: a
        repeated pass counts nothing from the failed one (whose streams the caller's stream has waited for)."""
        c, m = self.cfg, self.model
        dev = m.pos.device
        self.optimizer.zero_grad()
        for table in self._tables:
            table.zero_grad()
        params, scale_in, opacity_in = m.get_params(), m.scale_raw, m.opacity_raw
        if c.filter3d > 0:
            # the effective scale and opacity of this pass: ONE launch and two fresh leaves -- their gradients start empty in every
            # attempt.  The routes get the parameter dict with the two leaves in place: their addresses are the same for every view
            with torch.no_grad():
                scale_in, opacity_in = filter3d.apply(m.scale_raw.detach(), m.opacity_raw.detach(), self.filter3d)
            scale_in.requires_grad_(True)
            opacity_in.requires_grad_(True)
            params = {**params, 'scale_raw': scale_in, 'opacity_raw': opacity_in}
        acc = torch.zeros(3, dtype=torch.float32, device=dev)
        acc_aux = torch.zeros(3, dtype=torch.float32, device=dev) if aux is not None else None
        route = self._choose_route(world, len(views), aux is not None, params, even, sh_degree)
        consumer = route if world > 1 else None   # (the exchange is its own consumer: the settlement has it even if the pass stops before the `with`)
        checks = error = None
        try:
            # no host synchronisation per view: the renders size their buffers from earlier frames, the per-frame checks
            # (off-screen exception, buffer capacity) are made ONCE, after the last backward is queued
            with ops.deferred_checks() as checks, route as consumer, (ops.visible_set(self.visible) if c.sparse_adam else _NO_CONTEXT):
                if c.sparse_adam:
                    self.visible.reset()
                side = self._view_streams(dev) if (c.view_streams > 1 and len(views) > 1 and world == 1) else ()     # (one process: the
                # exchange's collectives of a data-parallel pass stay on the caller's stream)
                main = torch.cuda.current_stream(dev) if side else None
                for st in side:
                    st.wait_stream(main)                                           # parameters, zeroed gradients
                self._pass_dirty = pass_stats is not None
                per_view, per_view_aux, row_stream = [], [], {}
                for k, v in enumerate(views):
                    if rows is not None and side:
                        # two views of one training image add into ONE row of every table's gradient: the later one's stream waits
                        # for the earlier one's, so that the row is their sum in view order whichever streams they ran on
                        last = row_stream.get(rows[k])
                        if last is not None and last != k % len(side):
                            side[k % len(side)].wait_stream(side[last])
                        row_stream[rows[k]] = k % len(side)
                    with (torch.cuda.stream(side[k % len(side)]) if side else _NO_CONTEXT):
                        vals, aux_vals = self._view(v, rows[k] if rows is not None else None, scale_in, opacity_in, n_global, render_kw,
                                                    aux, bg, pass_stats[k] if pass_stats is not None else None)
                    per_view.append(vals)
                    if aux_vals is not None:
                        per_view_aux.append(aux_vals)
                for st in side:
                    main.wait_stream(st)
                if side and consumer.route_kind == ops.FACTORED:
                    for t in consumer.logits + consumer.eyes:                      # (allocated on a view's stream, read by finish() on the caller's)
                        t.record_stream(main)
                if consumer.route_kind == ops.SUMMED:
                    consumer.assign()
                _add_in_view_order(acc, per_view, main)
                _add_in_view_order(acc_aux, per_view_aux, main)
        except Exception as e:                # single process: nothing to agree on, the exception leaves as it is
            if world == 1:
                raise
            error = e
        return consumer, checks, error, (scale_in, opacity_in), acc, acc_aux

    def _view(self, v, row, scale_in, opacity_in, n_global, render_kw, aux, bg, stats):
        """One view of a pass, on the current stream: targets, render -- inside the view's statistics record `stats`, if any --, the
        transform (exposure or bilateral grid) of training image `row`, loss, backward; with pose_opt the render is at the corrected pose of
        camera `row`.  Returns its loss vector and its aux-loss vector (None: no maps)."""
        c, m = self.cfg, self.model
        dev = m.pos.device
        image_gt, alpha_gt, depth_gt = self._view_targets(v, dev, bg, aux is not None)
        c2w = torch.as_tensor(v['c2w'], dtype=torch.float32).to(dev)
        if self.poses is not None:
            c2w = self.poses.apply_view(c2w, row)      # (requires a gradient: the render below is a pose frame)
        with (ops.densify_stats(stats, absgrad=c.densify_absgrad) if stats is not None else _NO_CONTEXT):
            rendered = ops.render_gaussians(m.pos, m.f_dc, m.f_rest, opacity_in, scale_in, m.q_raw, c2w,
                                            int(v['H']), int(v['W']), float(v['fx']), float(v['fy']), float(v['cx']), float(v['cy']), **render_kw)
        if aux:
            rendered, depth, alpha = rendered
        if self._table is not None:
            rendered = self._table.apply_view(rendered, row)
        loss, vals = losses.compute_loss_device(rendered, image_gt, c.lambda_l1, c.lambda_ssim, scale=1.0 / n_global)
        if not aux:
            loss.backward()                        # (loss / batch size: the division is inside the loss kernels)
            return vals, None
        aux_total, aux_vals = losses.aux_loss(depth, alpha, depth_gt, alpha_gt, c.lambda_depth, c.lambda_alpha, scale=1.0 / n_global)
        torch.autograd.backward((loss, aux_total))      # loss + aux_total, one pass through the render's backward
        return vals, aux_vals

    def _settle_pass(self, n_views, consumer, checks, error, pass_stats, world):
        """What happened on this rank, as ONE code; then ONE agreement over the ranks: every rank repeats the pass, or none does; every
        rank raises, or none does.  Returns dp.STATUS_OK or dp.STATUS_REDO.  NOTHING may leave this function between the first
        collective of the pass and the agreement: a rank that raised here while its peers sat in the exchange would leave them waiting
        for ever."""
        dev = self.model.pos.device
        kind = consumer.route_kind
        status, err = dp.STATUS_OK, None
        try:
            if checks is not None:
                checks.verify()
            if kind == ops.FACTORED and consumer.n_added != n_views:
                raise RuntimeError(f"{consumer.n_added} of this rank's {n_views} views went through the factored exchange: a render "
                                   "of this model took the ordinary backward (are f_dc / f_rest the model's own tensors?)")
        except ops.PairCapacityExceeded:
            status = dp.STATUS_REDO           # a view outgrew the buffers: this pass's gradients are invalid (capacity now raised)
        except Exception as e:                # the reference's off-screen Exception (render.py:235-236), or anything else
            status, err = dp.status_of(e), e
        if status != dp.STATUS_OK and kind == ops.FOLDED:
            consumer.rollback()               # (the kernel stepped nothing for a frame that overflowed or is off screen: nothing counts)
        if error is not None:                 # an exception inside the render loop itself (a frame that waited for its counters, a device error)
            status, err = dp.status_of(error), error
        if world > 1:
            if kind == ops.FACTORED:
                consumer.pad_views(n_views)   # (a pass that stopped early: keep the sequence of collectives aligned)
            status = dp.agree_status(status, self.group, device=dev)
        if pass_stats is not None:
            # the caller's stream has waited for the views' streams: the pass records join the window in view order (and are zero
            # again); a pass that is repeated or fails counts nothing -- its valid views would otherwise count twice
            if status == dp.STATUS_OK:
                for rec in pass_stats:
                    self.densify_stats.merge_(rec)
                self._pass_dirty = False
            else:
                self._clear_pass_stats(dev)
        if kind == ops.FACTORED:
            if status != dp.STATUS_OK:
                consumer.abandon()
            else:
                consumer.finish()             # the loss was already divided by the global batch: world_views = 1
        dp.raise_agreed(status, err, "this training step")
        return status

    def _update(self, iteration, consumer, leaves, acc, acc_aux, world):
        """The optimiser steps of an iteration whose pass every rank agreed good -- so every rank is here, and none can be left in one
        of the collectives below.  Returns (what the per-image tables add to step()'s dict: 'lr_exposure', or 'lr_bilagrid' and 'tv'; 'lr_pose';
        mcmc.regularise's [reg_opacity, reg_scale, loss] or None)."""
        c, m = self.cfg, self.model
        table_out, reg = {}, None
        for table in self._tables:                 # (the fixed order of the constructor: one all-reduce per table, the same on every rank)
            # the table's gradient is complete on this rank -- the caller's stream has waited for the views' streams; summed over the
            # ranks, every replica steps the same bits.  The table's once-per-iteration term (the grid's TV) joins AFTER the all-reduce:
            # every rank computes the same one, and it counts once.  The table's own Adam, at this iteration's learning rate of its own
            if world > 1:
                dp.allreduce_table_grad(table.grad, self.group)
            table_out.update(table.regularise(c))
            sched = [getattr(c, f"{table.name}_lr_{k}") for k in ("init", "final", "delay_mult", "max_steps")]
            lr = optim.position_lr(iteration, *sched) if sched[0] > 0 else 0.0        # (a table frozen by a zero rate: no 0 / 0)
            table_out['lr_' + table.name] = lr
            table.step(lr)
        scale_in, opacity_in = leaves
        if c.filter3d > 0 and (scale_in.grad is not None or opacity_in.grad is not None):
            # the gradients of the two leaves are complete (every view; every rank: after the exchange's all-reduce): ONE launch takes them
            # through the filter to the raw parameters -- linear in the gradient and row-local, so exact after the sum and the same on
            # every rank.  Before the zero-fill, the clip and the optimiser step, which see the raw gradients only
            m.scale_raw.grad, m.opacity_raw.grad = torch.empty_like(m.scale_raw), torch.empty_like(m.opacity_raw)
            filter3d.backward_into(m.scale_raw.detach(), m.opacity_raw.detach(), self.filter3d,
                                   scale_in.grad if scale_in.grad is not None else torch.zeros_like(scale_in),
                                   opacity_in.grad if opacity_in.grad is not None else torch.zeros_like(opacity_in),
                                   m.scale_raw.grad, m.opacity_raw.grad)
        # f_rest was stepped inside the backward pass: no gradient, no second step
        folded = consumer.route_kind == ops.FOLDED and consumer.applied
        for k in dp.PARAM_NAMES:
            p = getattr(m, k)
            if p.grad is None and not (folded and p is m.f_rest):
                p.grad = torch.zeros_like(p)
        if c.densify_rule == "mcmc":
            # the gradients are complete (every view, every rank): the regularisers join them, and the loss, in ONE launch
            reg = mcmc.regularise(m, c.mcmc_opacity_reg, c.mcmc_scale_reg, base=_total(acc, acc_aux))
        self.optimizer.clip_grad_norm_(m.pos, max_norm=1.0)
        if c.sparse_adam:
            # the union over the ranks: every rank steps the same rows and the replicas stay bit-identical -- one collective of N bytes
            # per iteration
            if world > 1:
                self.visible.all_reduce(self.group)
            self.optimizer.step(visible=self.visible)
        else:
            self.optimizer.step()
        return table_out, reg

    def _refine(self, iteration, pos_lr, screen, world):
        """What follows the optimiser step: under MCMC the position noise and, at its interval, the relocation -- no densification, no
        opacity reset --; else densification at its interval (a fresh optimiser at the current position learning rate) and the opacity
        reset at its own.  Returns whether the set of Gaussians was refined."""
        c, m = self.cfg, self.model
        refine = bool(iteration < c.densify_until_iter and iteration % c.densification_interval == 0)
        if c.densify_rule == "mcmc":
            mcmc.add_noise(m, pos_lr * c.mcmc_noise_lr, c.mcmc_seed, int(iteration))
            refine = refine and bool(c.mcmc_start_iter <= iteration)
            if refine:
                # in place: the optimiser object and the moments of every row that did not change stay; nothing is read back
                m.refine_mcmc(self.optimizer, cap_max=c.cap_max, min_opacity=c.mcmc_min_opacity, growth=c.mcmc_growth,
                              seed=c.mcmc_seed, iteration=int(iteration))
            return refine
        if refine:
            if screen:
                if world > 1:                     # every rank decides from the statistics of all views: the replicas stay bit-identical
                    self.densify_stats.all_reduce(self.group)
                m.densify_and_prune_screen(self.densify_stats, opacity_threshold=c.prune_opacity_threshold,
                                           grad_threshold=c.densify_grad_threshold, scale_threshold=c.scale_threshold,
                                           max_screen_size=c.max_screen_size if iteration > c.opacity_reset_interval else None,
                                           generator=self._densify_generator(iteration))
                self.densify_stats.reset(m.get_num_gaussians())       # the next window, over the new set of Gaussians
            else:
                grads = {'pos': m.pos.grad, 'opacity_raw': m.opacity_raw.grad}
                m.densify_and_prune(grads, opacity_threshold=c.prune_opacity_threshold, max_grad=c.max_grad,
                                    scale_threshold=c.scale_threshold, generator=self._densify_generator(iteration))
            self.optimizer = self._new_optimizer(pos_lr)
        if iteration % c.opacity_reset_interval == 0:
            m.reset_opacity()
        return refine
