"""MI355X-native differentiable Gaussian-splat rasterizer: drop-in for the hot path of
ashu1069/3D-Gaussian-Splatting-for-Novel-View-Synthesis (its `gaussian_splatting` namespace,
reference gaussian_splatting/__init__.py:7-21).

The directory name is not a Python identifier; import it with

    import importlib
    gs = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd")

or through the alias module `gsplat_amd` at the repository root.  Same eight names as the reference namespace,
plus the fused entry `render_gaussians` and the data-parallel helpers in `.dp`.
"""
from .ops import (HARMONICS, build_sigma_from_params, evaluate_sh, inv2x2, project_points, quat_to_rotmat, render,
                  render_frames, render_gaussians, render_stats, scale_intrinsics, deferred_checks, run_deferred, set_deterministic,
                  PairCapacityExceeded, binned_pairs, reset_pair_capacity, DensifyStats, densify_stats,
                  ContributionStats, contribution, VisibleSet, visible_set)
from . import ops  # noqa: E402,F401

from . import losses  # noqa: E402,F401  (L1 + SSIM loss)
from .losses import compute_loss  # noqa: E402,F401
from . import optim  # noqa: E402,F401  (fused Adam + clip)
from . import harness  # noqa: E402,F401  (orbit, FPS meter, checkpoint formats: SURVEY §8f next row 3)
from . import data  # noqa: E402,F401  (on-disk layout + Gaussian initialisation: SURVEY §8f next row 4)
from . import dp  # noqa: E402,F401  (data-parallel-by-view helpers)
from . import mcmc  # noqa: E402,F401  (density control at a fixed budget: MCMC relocation, position noise)
from . import filter3d  # noqa: E402,F401  (the 3D smoothing filter of Mip-Splatting: per-Gaussian sampling limit from the cameras)
from . import exposure  # noqa: E402,F401  (per-view exposure compensation: an affine colour transform per training image)
from . import bilagrid  # noqa: E402,F401  (per-view bilateral grids: a sliced grid of affine colour transforms per training image)
from . import poses  # noqa: E402,F401  (per-view camera-pose corrections: a learned rigid correction per training camera)
from . import metrics  # noqa: E402,F401  (held-out views: per-image PSNR / SSIM / L1, colour-corrected on request)
from . import knn  # noqa: E402,F401  (scale initialisation from the 3 nearest neighbours: exact k-NN over a Morton sort)
from . import features  # noqa: E402,F401  (per-Gaussian feature vectors: N-channel maps and their adjoint, 2D maps lifted onto the Gaussians)
from . import model  # noqa: E402,F401  (GaussianModel: densify / prune / opacity reset)
from . import training  # noqa: E402,F401  (one training iteration of the reference's loop on the fused pieces)

__all__ = [
    'build_sigma_from_params', 'quat_to_rotmat', 'evaluate_sh', 'HARMONICS', 'render', 'project_points', 'inv2x2',
    'scale_intrinsics', 'render_gaussians', 'render_stats', 'render_frames', 'deferred_checks', 'run_deferred', 'set_deterministic',
    'PairCapacityExceeded', 'binned_pairs', 'reset_pair_capacity', 'DensifyStats', 'densify_stats', 'ContributionStats', 'contribution',
    'VisibleSet', 'visible_set',
]
