"""ctypes mirror of include/gsplat_mi355x.h and the loader of the HIP library.

The product path has NO CPU fallback: if libgsplat_mi355x.so is missing or does not export every
symbol the header declares, `lib()` raises and every op fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSPLAT_MI355X_LIB: explicit path of another build of the same library (tools/ use it for the diagnostics build)
LIB_PATH = os.environ.get("GSPLAT_MI355X_LIB") or os.path.join(_HERE, "csrc", "libgsplat_mi355x.so")

GSPLAT_OK = 0
GSPLAT_ERR_BAD_ARG = 1
GSPLAT_ERR_WORKSPACE = 3
GSPLAT_SCENE_OK = 0
GSPLAT_SCENE_ALL_CULLED = 10
GSPLAT_SCENE_ALL_OFFSCREEN = 11
ABI_VERSION = 12
GSPLAT_PROJECT_COLOUR_FUSED = 1
GSPLAT_PROJECT_COUNTS_MAPPED = 2
GSPLAT_PROJECT_SAVE_SH_JACOBIAN = 4
GSPLAT_PROJECT_COUNTS_LATE = 8
GSPLAT_BACKWARD_SH_JACOBIAN = 1
GSPLAT_FRAME_BACKWARD = 1
GSPLAT_FRAME_NO_SH_JACOBIAN = 2
GSPLAT_BACKWARD_PHASE_RASTER = 2
GSPLAT_BACKWARD_PHASE_PROJECT = 4
GSPLAT_BACKWARD_GRAD2D_DIRTY = 8
GSPLAT_BACKWARD_ACCUMULATE = 16
GSPLAT_BACKWARD_DEPTH = 64
GSPLAT_BACKWARD_ABSGRAD = 128
GSPLAT_FILTER3D_CAMERA_FLOATS = 24
GSPLAT_FILTER3D_CAMERA_CHUNK = 64
GSPLAT_EXPOSURE_ACCUMULATE = 1
GSPLAT_BILAGRID_ACCUMULATE = 1
GSPLAT_METRICS_COLOUR_CORRECT = 1
GSPLAT_KNN_BOX = 256
GSPLAT_POSE_DELTA_ACCUMULATE = 1
GSPLAT_FEATURES_MAX_CHANNELS = 512


def sh_bands_dropped(degree):
    """3 - degree for an SH degree that is one of the integers 0..3 (bool, float and anything else: ValueError)."""
    if type(degree) is not int or not 0 <= degree <= 3:
        raise ValueError(f"sh_degree must be one of the integers 0, 1, 2, 3, not {degree!r}")
    return 3 - degree


# the function-like macros of the header: the SH degree of a fused render in two flag bits, as "bands dropped" (0 = degree 3)
def GSPLAT_PROJECT_SH_DEGREE(d):
    return sh_bands_dropped(d) << 4


def GSPLAT_FRAME_SH_DEGREE(d):
    return sh_bands_dropped(d) << 4


def GSPLAT_BACKWARD_SH_DEGREE(d):
    return sh_bands_dropped(d) << 8


# the screen-space low-pass, in the same bits of the flags of the six entries that run the projection math
GSPLAT_FILTER_ANTIALIAS = 65536


def GSPLAT_FILTER_LOWPASS(c):
    return c << 17


def filter_bits(lowpass=0.0, antialias=False):
    """The GSPLAT_FILTER_* bits of a render's (lowpass, antialias), 0 for the default; ValueError for anything the kernels cannot do:
    lowpass off the 0.01 grid or outside [0, 2.55], an antialias that is not a bool, antialias without a low-pass."""
    if type(antialias) is not bool:
        raise ValueError(f"antialias must be a bool, not {antialias!r}")
    try:
        x = float(lowpass) * 100.0
        c = round(x)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"lowpass must be a multiple of 0.01 in [0, 2.55], not {lowpass!r}") from None
    if isinstance(lowpass, bool) or not abs(x - c) <= 1e-6 or not 0 <= c <= 255:
        raise ValueError(f"lowpass must be a multiple of 0.01 in [0, 2.55], not {lowpass!r}")
    if antialias and c == 0:
        raise ValueError("antialias=True needs lowpass > 0")
    return GSPLAT_FILTER_LOWPASS(c) | (GSPLAT_FILTER_ANTIALIAS if antialias else 0)


def filter_kwargs(lowpass=0.0, antialias=False):
    """The keyword arguments that carry a filter mode to the render entries: none for the default, so the default call stays the
    reference's (validated as filter_bits does)."""
    return dict(lowpass=lowpass, antialias=antialias) if filter_bits(lowpass, antialias) else {}


_F = C.POINTER(C.c_float)


class View(C.Structure):
    """gsplat_view: intrinsics + the 8 keyword arguments of render() (reference render.py:62-64)."""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("near_z", C.c_float), ("far_z", C.c_float), ("pix_guard", C.c_float),
                ("tile", C.c_int32), ("min_conis", C.c_float), ("chi_square_clip", C.c_float),
                ("alpha_max", C.c_float), ("alpha_cutoff", C.c_float)]


class Gaussians(C.Structure):
    _fields_ = [("n", C.c_int64), ("pos", C.c_void_p), ("opacity_raw", C.c_void_p), ("color", C.c_void_p),
                ("sigma", C.c_void_p), ("scale_raw", C.c_void_p), ("q_raw", C.c_void_p), ("f_dc", C.c_void_p),
                ("f_rest", C.c_void_p)]


class GaussianGrads(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("opacity_raw", C.c_void_p), ("color", C.c_void_p), ("sigma", C.c_void_p),
                ("scale_raw", C.c_void_p), ("q_raw", C.c_void_p), ("f_dc", C.c_void_p), ("f_rest", C.c_void_p)]


class AdamGroup(C.Structure):
    _fields_ = [("n", C.c_int64), ("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("lr", C.c_float), ("step", C.c_int32), ("grad_scale", C.c_void_p)]


class Counts(C.Structure):
    _fields_ = [("n_survivors", C.c_int32), ("n_visible", C.c_int32), ("n_pairs", C.c_int64),
                ("max_tiles_per_gaussian", C.c_int32), ("reserved", C.c_int32), ("n_binned", C.c_int64)]


class StateLayout(C.Structure):
    """gsplat_state_layout: byte offsets inside project_state (tests and tools only, no stable contract)."""
    _fields_ = [("bytes", C.c_int64), ("lists", C.c_int64), ("lists_x", C.c_int32), ("lists_y", C.c_int32)] + [
        (k, C.c_int64) for k in ("counts", "rec", "rect", "depth", "tiles", "mask", "ranges", "order", "class_bounds", "kj")]


class BinLayout(C.Structure):
    _fields_ = [("bytes", C.c_int64), ("sorted_ids", C.c_int64), ("pair_mask", C.c_int64)]


class McmcMoments(C.Structure):
    """gsplat_mcmc_moments: (exp_avg, exp_avg_sq) of each parameter, NULL pairs allowed."""
    _fields_ = [(k, C.c_void_p * 2) for k in ("pos", "f_dc", "f_rest", "opacity_raw", "scale_raw", "q_raw")]


class McmcLayout(C.Structure):
    """gsplat_mcmc_layout: byte offsets inside the MCMC scratch and the two constants of the scan (tests and tools only)."""
    _fields_ = [(k, C.c_int64) for k in ("bytes", "reg", "w", "prefix", "src", "count", "total", "block_sums")] + [
        ("scan_block", C.c_int32), ("scan_chunk", C.c_int32)]


_VP, _I64, _INT = C.c_void_p, C.c_int64, C.c_int
_PV, _PG, _PGG, _PC = C.POINTER(View), C.POINTER(Gaussians), C.POINTER(GaussianGrads), C.POINTER(Counts)

# name -> (restype, argtypes); must list every function include/gsplat_mi355x.h declares
SIGNATURES = {
    "gsplat_abi_version": (_INT, []),
    "gsplat_last_error": (C.c_char_p, []),
    "gsplat_classify_counts": (_INT, [_PC]),
    "gsplat_project_state_bytes": (_I64, [_I64, _PV]),
    "gsplat_project_scratch_bytes": (_I64, [_I64]),
    "gsplat_bin_state_bytes": (_I64, [_I64, _PV]),
    "gsplat_bin_scratch_bytes": (_I64, [_I64, _PV]),
    "gsplat_project_state_layout": (_INT, [_I64, _PV, C.POINTER(StateLayout)]),
    "gsplat_bin_state_layout": (_INT, [_I64, _PV, C.POINTER(BinLayout)]),
    "gsplat_project": (_INT, [_PG, _VP, _PV, _VP, _VP, _I64, _VP, _VP, C.c_int32, _VP]),
    "gsplat_bin": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _I64, _VP]),
    "gsplat_rasterize_forward": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gsplat_rasterize_forward_aux": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP]),
    "gsplat_rasterize_backward_scratch_bytes": (_I64, [_I64, _I64]),
    "gsplat_rasterize_backward_aux_scratch_bytes": (_I64, [_I64, _I64]),
    "gsplat_rasterize_backward_aux": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, C.c_int32, _VP, _I64, _VP]),
    "gsplat_rasterize_backward": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP, _I64, _VP]),
    "gsplat_rasterize_backward_abs_scratch_bytes": (_I64, [_I64, _I64]),
    "gsplat_rasterize_backward_aux_abs_scratch_bytes": (_I64, [_I64, _I64]),
    "gsplat_rasterize_backward_aux_abs": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, C.c_int32, _VP, _I64, _VP]),
    "gsplat_rasterize_backward_abs": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP, _I64, _VP]),
    "gsplat_project_backward": (_INT, [_PG, _VP, _PV, _VP, _VP, _PGG, C.c_int32, _VP]),
    "gsplat_pose_scratch_bytes": (_I64, [_I64]),
    "gsplat_project_backward_pose": (_INT, [_PG, _VP, _PV, _VP, _VP, _PGG, _VP, _VP, _I64, C.c_int32, _VP]),
    "gsplat_logit_grad": (_INT, [_I64, _PV, _VP, _VP, _VP, _VP]),
    "gsplat_densify_stats": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP]),
    "gsplat_frame_densify_stats": (_INT, [_I64, _I64, _PV, _VP, _I64, _VP, _VP]),
    "gsplat_densify_stats_abs": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP]),
    "gsplat_frame_densify_stats_abs": (_INT, [_I64, _I64, _PV, _VP, _I64, _VP, _VP]),
    "gsplat_densify_stats_merge": (_INT, [_I64, _VP, _VP, _VP]),
    "gsplat_visible_set": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP]),
    "gsplat_frame_visible_set": (_INT, [_I64, _I64, _PV, _VP, _I64, _VP, _VP]),
    "gsplat_contribution": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _VP]),
    "gsplat_frame_contribution": (_INT, [_I64, _I64, _PV, _VP, _I64, _VP, _VP]),
    "gsplat_features_forward": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _INT, _VP, _VP]),
    "gsplat_features_adjoint": (_INT, [_I64, _I64, _PV, _VP, _VP, _VP, _INT, _VP, _VP]),
    "gsplat_frame_bytes": (_I64, [_I64, _I64, _PV, C.c_int32]),
    "gsplat_forward_deferred": (_INT, [_PG, _VP, _PV, _VP, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, C.c_int32, _VP]),
    "gsplat_backward": (_INT, [_PG, _VP, _PV, _VP, _I64, _I64, _VP, _PGG, _VP, _VP, _I64, C.c_int32, _VP]),
    "gsplat_sh_accumulate": (_INT, [_I64, C.c_int32, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP]),
    "gsplat_sh_accumulate_degree": (_INT, [_I64, C.c_int32, _VP, _VP, _VP, C.c_float, _VP, _VP, C.c_int32, _VP]),
    "gsplat_build_sigma": (_INT, [_I64, _VP, _VP, _VP, _VP]),
    "gsplat_build_sigma_backward": (_INT, [_I64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gsplat_evaluate_sh": (_INT, [_I64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gsplat_evaluate_sh_backward": (_INT, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gsplat_loss_scratch_bytes": (_I64, [_I64, C.c_int32, C.c_int32, C.c_int32]),
    "gsplat_loss": (_INT, [_VP, _VP, _I64, C.c_int32, C.c_int32, C.c_float, C.c_float, _VP, _VP, _VP, _VP]),
    "gsplat_loss_forward": (_INT, [_VP, _VP, _I64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, _VP, _VP, _VP, C.c_int32, _VP]),
    "gsplat_loss_backward": (_INT, [_VP, _VP, _I64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, _VP, _VP, _VP, _VP]),
    "gsplat_aux_loss_scratch_bytes": (_I64, [_I64, C.c_int32, C.c_int32]),
    "gsplat_aux_loss_forward": (_INT, [_VP, _VP, _VP, _VP, _I64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, _VP, _VP, _VP, _VP]),
    "gsplat_aux_loss_backward": (_INT, [_VP, _VP, _VP, _VP, _I64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, _VP, _VP, _VP, _VP,
                                        _VP]),
    "gsplat_composite_target": (_INT, [_VP, _VP, _F, _I64, C.c_int32, C.c_int32, _VP, _VP]),
    "gsplat_clip_scratch_bytes": (_I64, []),
    "gsplat_clip_grad_norm": (_INT, [_I64, _VP, C.c_float, _VP, _VP, _VP]),
    "gsplat_adam_step": (_INT, [_I64, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, _VP, _VP]),
    "gsplat_adam_step_multi": (_INT, [C.c_int32, C.POINTER(AdamGroup), C.c_float, C.c_float, C.c_float, _VP]),
    "gsplat_adam_step_rows": (_INT, [C.c_int32, C.POINTER(AdamGroup), C.POINTER(C.c_int32), _I64, _VP, C.c_float, C.c_float, C.c_float, _VP]),
    "gsplat_backward_adam_rest": (_INT, [_PG, _VP, _PV, _VP, _I64, _I64, _VP, _PGG, _VP, _I64, C.c_int32, C.POINTER(AdamGroup), C.c_float, C.c_float,
                                         C.c_float, _VP]),
    "gsplat_mcmc_scratch_bytes": (_I64, [_I64]),
    "gsplat_mcmc_scratch_layout": (_INT, [_I64, C.POINTER(McmcLayout)]),
    "gsplat_mcmc_noise": (_INT, [_I64, _VP, _VP, _VP, _VP, C.c_float, C.c_uint64, C.c_uint32, _VP]),
    "gsplat_mcmc_regularise": (_INT, [_I64, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP, _VP]),
    "gsplat_mcmc_refine": (_INT, [_VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(McmcMoments), _I64, C.c_float, C.c_uint64, C.c_uint32, _VP, _VP]),
    "gsplat_filter3d_scratch_bytes": (_I64, [_I64]),
    "gsplat_filter3d_compute": (_INT, [_I64, _VP, C.c_int32, _VP, C.c_float, C.c_float, C.c_float, _VP, _VP, _VP]),
    "gsplat_filter3d_apply": (_INT, [_I64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "gsplat_filter3d_apply_backward": (_INT, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gsplat_exposure_scratch_bytes": (_I64, [_I64, C.c_int32, C.c_int32]),
    "gsplat_exposure_forward": (_INT, [_VP, _VP, _I64, C.c_int32, C.c_int32, _VP, _VP]),
    "gsplat_exposure_backward": (_INT, [_VP, _VP, _VP, _I64, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, _VP, _VP]),
    "gsplat_bilagrid_forward": (_INT, [_VP, _VP, _I64] + [C.c_int32] * 5 + [_VP, _VP]),
    "gsplat_bilagrid_backward": (_INT, [_VP, _VP, _VP, _I64] + [C.c_int32] * 5 + [_VP, _VP, _VP, C.c_int32, _VP]),
    "gsplat_bilagrid_tv_scratch_bytes": (_I64, [_I64, C.c_int32, C.c_int32, C.c_int32]),
    "gsplat_bilagrid_tv": (_INT, [_VP, _I64, C.c_int32, C.c_int32, C.c_int32, C.c_float, _VP, _VP, C.c_int32, _VP, _VP]),
    "gsplat_metrics_scratch_bytes": (_I64, [C.c_int32] * 4),
    "gsplat_metrics_fit_affine": (_INT, [_VP, _VP, _VP] + [C.c_int32] * 3 + [_VP, _VP, _VP]),
    "gsplat_metrics_forward": (_INT, [_VP, _VP, _VP] + [C.c_int32] * 4 + [_VP, _VP, _VP, _VP]),
    "gsplat_knn_scratch_bytes": (_I64, [_I64]),
    "gsplat_knn_mean_dist2": (_INT, [_I64, _VP, _VP, _VP, _VP]),
    "gsplat_pose_delta_forward": (_INT, [_VP, _VP, _I64, _VP, _VP]),
    "gsplat_pose_delta_backward": (_INT, [_VP, _VP, _VP, _I64, _VP, _VP, _VP, C.c_int32, _VP]),
    "gsplat_pose_delta_decay": (_INT, [_VP, _I64, C.c_float, _VP, _VP]),
}

_lib = None


class GsplatLibraryError(RuntimeError):
    pass


def lib():
    """Load libgsplat_mi355x.so (once).  Raises GsplatLibraryError if it is missing or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GsplatLibraryError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (or `make -C "
            f"{os.path.dirname(LIB_PATH)}`).  There is no CPU fallback for the render path.")
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise GsplatLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    ver = handle.gsplat_abi_version()
    if ver != ABI_VERSION:
        raise GsplatLibraryError(f"ABI version mismatch: library {ver}, Python host {ABI_VERSION}")
    _lib = handle
    return _lib


def check(status, what):
    if status != GSPLAT_OK:
        msg = lib().gsplat_last_error()
        raise RuntimeError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")


def make_view(H, W, fx, fy, cx, cy, near=0.01, far=100.0, pix_guard=32, T=16, min_conis=1e-6, chi_square_clip=6.25,
              alpha_max=0.99, alpha_cutoff=1 / 128.):
    return View(int(H), int(W), float(fx), float(fy), float(cx), float(cy), float(near), float(far), float(pix_guard),
                int(T), float(min_conis), float(chi_square_clip), float(alpha_max), float(alpha_cutoff))
