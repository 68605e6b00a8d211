"""Gaussian parameter container with the reference's adaptive density control ("next" row 2).

    GaussianModel(initial_params, device)                     scripts/train.py:48-86
      .densify_and_prune(grads, opacity_threshold=0.01, max_grad=0.01, scale_threshold=0.01, max_screen_size=20)
                                                              scripts/train.py:89-141
      .densify_and_prune_screen(stats, opacity_threshold=0.01, grad_threshold=0.0002, scale_threshold=0.01, max_screen_size=None)
                                                              the paper's criterion on ops.DensifyStats (not in the reference)
      .prune_by_contribution(stats, min_weight_max=None, keep_fraction=None)
                                                              contribution-based pruning on ops.ContributionStats (not in the reference)
      .refine_mcmc(optimizer, cap_max, min_opacity=0.005, growth=1.05, seed=0, iteration=0)
                                                              MCMC relocation at a fixed budget (not in the reference):
                                                              the one rule that KEEPS the optimiser and its moments
      ._prune_points / ._split_points / ._clone_points        scripts/train.py:143-195
      .reset_opacity(threshold=0.01, bump=0.01)               scripts/train.py:564-569 (inline in the loop there)
      .save_checkpoint / .load_checkpoint                     scripts/train.py:197-219 (-> harness.py)

Semantics kept (checked against the reference's own methods, tests/golden/densify.npz):
  * prune first (`sigmoid(opacity_raw) < opacity_threshold`), gradients are re-indexed with the same mask;
  * split keeps the parent and appends ONE child per selected Gaussian: position + randn * exp(scale_raw) * 0.1, scale_raw - 0.5,
    everything else copied; clone appends an exact copy; children go to the end, in mask order; split children before clones;
  * `max_screen_size` is accepted and unused by densify_and_prune, as in the reference (densify_and_prune_screen applies it);
  * the optimiser state is not carried over (the reference builds a fresh Adam after every densification, :554-561) -- by these
    rules; refine_mcmc rewrites rows in place and carries it.

One documented divergence: in the reference the clone mask is computed before the split and applied after it
(:136-141), so when a split and a clone are both due it indexes [N+S]-row tensors with an [N]-row mask and raises
IndexError.  Here the clone mask addresses the N pre-split rows it was computed for (what the reference evidently means,
and what it does whenever it does not raise); the fixture records the reference's exception for that case.

Host-side tensor bookkeeping (boolean masks + concatenation, run every `densification_interval` iterations): plain
torch ops on whatever device the parameters live on; no kernel of its own.  `generator` makes the split noise
reproducible and identical on every data-parallel rank.
"""
import math

import torch

from . import harness, mcmc

PARAM_KEYS = harness.PARAM_KEYS


class GaussianModel:
    def __init__(self, initial_params, device='cuda'):
        self.device = device
        for k in PARAM_KEYS:
            setattr(self, k, torch.nn.Parameter(initial_params[k].to(device)))

    def get_params(self):
        return {k: getattr(self, k) for k in PARAM_KEYS}

    def get_num_gaussians(self):
        return self.pos.shape[0]

    # ---- adaptive density control -------------------------------------------------------------------
    def densify_and_prune(self, grads, opacity_threshold=0.01, max_grad=0.01, scale_threshold=0.01, max_screen_size=20,
                          generator=None):
        opacity = torch.sigmoid(self.opacity_raw)
        prune_mask = opacity < opacity_threshold
        self._prune_points(prune_mask)
        if grads is not None:
            for key in grads:
                if grads[key] is not None:
                    grads[key] = grads[key][~prune_mask]
        if grads is not None and grads.get('pos') is not None:
            grad_norm = grads['pos'].norm(dim=-1)
            self._densify(grad_norm > max_grad, scale_threshold, generator)

    def densify_and_prune_screen(self, stats, opacity_threshold=0.01, grad_threshold=0.0002, scale_threshold=0.01, max_screen_size=None,
                                 generator=None):
        """The paper's criterion, from the screen-space statistics of ops.DensifyStats (`stats`: one, or its [N, 4] tensor =
        (grad_sum, count, extent_max, 0) on the parameters' device, a row per Gaussian): prune `sigmoid(opacity_raw) <
        opacity_threshold` and -- with max_screen_size -- `extent_max > max_screen_size` (pixels); then, of the surviving rows,
        `hot = grad_sum / max(count, 1) >= grad_threshold` (a Gaussian no view saw is never hot); split the hot ones whose largest
        scale exceeds scale_threshold, clone the others: the same split / clone and the same order as densify_and_prune."""
        data = getattr(stats, "data", stats)
        if tuple(data.shape) != (self.pos.shape[0], 4):
            raise ValueError(f"the statistics have shape {tuple(data.shape)}, the model has {self.pos.shape[0]} Gaussians")
        data = data.detach().to(self.pos.device)
        prune_mask = torch.sigmoid(self.opacity_raw) < opacity_threshold
        if max_screen_size is not None:
            prune_mask = prune_mask | (data[:, 2] > max_screen_size)
        self._prune_points(prune_mask)
        kept = data[~prune_mask]
        hot = kept[:, 0] / kept[:, 1].clamp(min=1) >= grad_threshold
        self._densify(hot, scale_threshold, generator)

    def prune_by_contribution(self, stats, min_weight_max=None, keep_fraction=None):
        """Remove the Gaussians that never matter in the composite of the views accumulated in `stats` (an ops.ContributionStats of
        this model's N rows; on any device).  Returns the number removed.
          min_weight_max   removes the rows with weight_max < min_weight_max -- every row is evaluated, never-seen ones included.
                           0.0 removes nothing; torch.finfo(torch.float32).tiny removes exactly the rows with weight_max == 0.
          keep_fraction    in (0, 1]: of the survivors of the first rule, keeps the ceil(keep_fraction * survivors) with the largest
                           weight_sum -- a stable sort on the integer sum_q, descending, ties broken by the lower index, so the choice
                           is the same on every rank and in every run.
        The two rules apply in that order; a call with neither raises ValueError, like a record of another size."""
        if min_weight_max is None and keep_fraction is None:
            raise ValueError("prune_by_contribution needs min_weight_max, keep_fraction or both")
        n = self.pos.shape[0]
        data = getattr(stats, "data", None)
        if not isinstance(data, torch.Tensor) or tuple(data.shape) != (n, 4) or data.dtype != torch.int32:
            raise ValueError(f"the statistics must be an ops.ContributionStats of {n} rows (the model's Gaussians), not "
                             f"{tuple(data.shape) if isinstance(data, torch.Tensor) else type(stats).__name__}")
        if keep_fraction is not None and not 0.0 < float(keep_fraction) <= 1.0:
            raise ValueError(f"keep_fraction must lie in (0, 1], not {keep_fraction!r}")
        if min_weight_max is not None and not float(min_weight_max) >= 0.0:
            raise ValueError(f"min_weight_max must be >= 0, not {min_weight_max!r}")
        remove = torch.zeros(n, dtype=torch.bool, device=data.device)
        if min_weight_max is not None:
            remove = stats.weight_max < float(min_weight_max)
        if keep_fraction is not None:
            alive = torch.nonzero(~remove).reshape(-1)              # ascending index
            keep = min(math.ceil(float(keep_fraction) * int(alive.numel())), int(alive.numel()))
            order = torch.sort(stats.sum_q[alive], descending=True, stable=True).indices       # ties: the lower index first
            remove[alive[order[keep:]]] = True
        removed = int(remove.sum())
        self._prune_points(remove.to(self.pos.device))
        return removed

    @torch.no_grad()
    def refine_mcmc(self, optimizer, cap_max, min_opacity=0.005, growth=1.05, seed=0, iteration=0):
        """One MCMC refinement.  Growth: n_target = min(cap_max, int(growth N)); if that is more than N, dead rows are
        appended (opacity_raw = -20, q_raw = (0, 0, 0, 1), everything else 0) and `optimizer` (a GaussianAdam over this model's
        parameters, or None) follows with GaussianAdam.grow_rows -- moments zero-padded, step counts kept; N never shrinks.  Then one
        library call (mcmc.relocate): every dead row, old or appended, becomes a copy of a live one drawn in proportion to the
        opacities.  No host read anywhere: the number of rows is a function of (N, cap_max, growth) alone.  Returns the rows appended."""
        n = self.get_num_gaussians()
        if type(cap_max) is not int or cap_max < 1:
            raise ValueError(f"cap_max must be an integer >= 1, not {cap_max!r}")
        if not (isinstance(growth, (int, float)) and not isinstance(growth, bool) and 1.0 <= growth < float("inf")):
            raise ValueError(f"growth must be a finite number >= 1, not {growth!r}")
        if not (isinstance(min_opacity, float) and 0.0 < min_opacity < 1.0):
            raise ValueError(f"min_opacity must be a float in (0, 1), not {min_opacity!r}")
        extra = max(0, min(cap_max, int(growth * n)) - n)
        if extra:
            for k in PARAM_KEYS:
                old = getattr(self, k)
                pad = old.new_zeros((extra,) + tuple(old.shape[1:]))
                if k == 'opacity_raw':
                    pad.fill_(-20.0)
                elif k == 'q_raw':
                    pad[:, 3] = 1.0
                new = torch.nn.Parameter(torch.cat([old.detach(), pad], dim=0))
                if optimizer is not None:
                    optimizer.grow_rows(old, new)
                setattr(self, k, new)
        mcmc.relocate(self, optimizer, min_opacity, seed, iteration)
        return extra

    def _densify(self, hot, scale_threshold, generator):
        """Split the `hot` Gaussians whose largest scale exceeds scale_threshold, clone the other hot ones (children at the end:
        split children first, then clones)."""
        max_scale = torch.exp(self.scale_raw).max(dim=-1)[0]
        split_mask = (max_scale > scale_threshold) & hot
        clone_mask = (max_scale <= scale_threshold) & hot
        n_before = self.pos.shape[0]
        self._split_points(split_mask, generator=generator)
        grown = self.pos.shape[0] - n_before
        if grown:       # the clone mask belongs to the pre-split rows (see the module docstring)
            clone_mask = torch.cat([clone_mask, clone_mask.new_zeros(grown)])
        self._clone_points(clone_mask)

    def _replace(self, new):
        for k in PARAM_KEYS:
            setattr(self, k, torch.nn.Parameter(new[k]))

    def _prune_points(self, mask):
        if not mask.any():
            return
        keep = ~mask
        self._replace({k: getattr(self, k)[keep] for k in PARAM_KEYS})

    def _split_points(self, mask, generator=None):
        if not mask.any():
            return
        sel = {k: getattr(self, k)[mask].clone() for k in PARAM_KEYS}
        if generator is None:
            noise = torch.randn_like(sel['pos'])
        else:
            noise = torch.randn(sel['pos'].shape, generator=generator, device=generator.device,
                                dtype=sel['pos'].dtype).to(sel['pos'].device)
        sel['pos'] = sel['pos'] + noise * torch.exp(self.scale_raw[mask]) * 0.1
        sel['scale_raw'] = sel['scale_raw'] - 0.5
        self._replace({k: torch.cat([getattr(self, k), sel[k]], dim=0) for k in PARAM_KEYS})

    def _clone_points(self, mask):
        if not mask.any():
            return
        self._replace({k: torch.cat([getattr(self, k), getattr(self, k)[mask]], dim=0) for k in PARAM_KEYS})

    @torch.no_grad()
    def reset_opacity(self, threshold=0.01, bump=0.01):
        """Opacity reset of the training loop (scripts/train.py:564-569): Gaussians below `threshold` get
        logit(clamp(opacity + bump, 0, 1)).  Returns the number of Gaussians touched (a host read, as `mask.any()` is there)."""
        opacity = torch.sigmoid(self.opacity_raw)
        mask = opacity < threshold
        n = int(mask.sum())
        if n:
            self.opacity_raw.data[mask] = torch.logit(torch.clamp(opacity[mask] + bump, 0, 1))
        return n

    # ---- checkpoints --------------------------------------------------------------------------------
    def save_checkpoint(self, path, iteration):
        harness.save_checkpoint(path, self, iteration)

    def load_checkpoint(self, path):
        params, iteration = harness.load_checkpoint(path, device=self.device)
        self._replace({k: params[k] for k in PARAM_KEYS})
        return iteration
