"""The refusals of the entries that walk a projected frame, without a GPU: every refusal comes before any launch, so
the entries are called with host addresses.  ONE table: per entry, each single bad argument -- and the pairs of faults that pin the
order of the checks -- with the exact text gsplat_last_error() then holds.  The texts were written down from the library as it stood
before the entries came to share one preamble; that library and this one pass with the same table."""
import ctypes as C
import importlib

import pytest

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
abi = importlib.import_module(PKG + "._abi")

_STATE = ("n", "pc", "view", "project_state")
_FRAME = ("n", "pc", "view", "frame", "frame_bytes")
_RASTER = _STATE + ("bin_state", "accum")
_TAIL = ("grad2d", "grad2d_zeroed", "det_scratch", "det_scratch_bytes", "stream")
ARGS = {
    "gsplat_densify_stats": _STATE + ("grad2d", "stats", "stream"),
    "gsplat_densify_stats_abs": _STATE + ("grad2d", "stats", "stream"),
    "gsplat_frame_densify_stats": _FRAME + ("stats", "stream"),
    "gsplat_frame_densify_stats_abs": _FRAME + ("stats", "stream"),
    "gsplat_visible_set": _STATE + ("visible", "stream"),
    "gsplat_frame_visible_set": _FRAME + ("visible", "stream"),
    "gsplat_contribution": _STATE + ("bin_state", "record", "stream"),
    "gsplat_frame_contribution": _FRAME + ("record", "stream"),
    "gsplat_features_forward": _STATE + ("bin_state", "features", "channels", "out", "stream"),
    "gsplat_features_adjoint": _STATE + ("bin_state", "grad_out", "channels", "grad_features", "stream"),
    "gsplat_rasterize_backward_abs": _RASTER + ("grad_image",) + _TAIL,
    "gsplat_rasterize_backward_aux_abs": _RASTER + ("accum_aux", "grad_image", "grad_depth", "grad_alpha", "background") + _TAIL,
}
_NOT_POINTERS = ("n", "pc", "view", "frame_bytes", "channels", "grad2d_zeroed", "det_scratch_bytes")
_NULL_BY_DEFAULT = ("stream", "det_scratch", "background")
N, PAIRS = 4, 16

# a bad value: NULL (a pointer or the view), H0 (the view with H = 0), a number (n or pc), ODD (the address + 4: aligned to 4 bytes
# only), SHORT (frame_bytes one byte below gsplat_frame_bytes(N, PAIRS): what every other call passes)
NULL, H0, ODD, SHORT = None, "H = 0", "address + 4", "one byte short"
BIG_N, BIG_PC = 1 << 40, 1 << 32
RANGE = "n / pair_capacity out of range"
VIEW = "bad view (image size, tile size)"
NULL_ARG, NULL_VIEW = "NULL argument", "view is NULL"
SMALL_B = "frame arena too small: was it made with GSPLAT_FRAME_BACKWARD?"
SMALL = "frame arena too small (gsplat_frame_bytes)"
ALIGN_F = "frame must be 256-byte aligned"

_OPENING = [(dict(view=NULL), NULL_VIEW), (dict(view=H0), VIEW), (dict(n=-1), RANGE), (dict(pc=-1), RANGE)]
_EVERYTHING_BAD = dict(n=-1, pc=-1)         # (+ every pointer NULL, below): with a NULL view


def _stats_rows(state, what):
    return _OPENING + [(dict(n=BIG_N), RANGE), ({state: NULL}, NULL_ARG), (dict(grad2d=NULL), NULL_ARG), (dict(stats=NULL), NULL_ARG),
                       (dict(stats=ODD), what), (dict(grad2d=ODD), what), ({"n": -1, state: NULL}, RANGE)]


def _frame_rows(out, small, after=()):
    """An entry on a frame arena: n = 2^40 and pc = 2^32 pass the arena's opening checks and are refused by its size."""
    return _OPENING + [(dict(n=BIG_N), small), (dict(pc=BIG_PC), small), (dict(frame=NULL), NULL_ARG), ({out: NULL}, NULL_ARG),
                       (dict(frame=ODD), ALIGN_F), (dict(frame_bytes=SHORT), small), (dict(n=-1, frame=NULL), RANGE),
                       (dict(n=BIG_N, frame_bytes=SHORT), small), (dict(frame=NULL, frame_bytes=SHORT), NULL_ARG),
                       (dict(frame=ODD, frame_bytes=SHORT), ALIGN_F)] + list(after)


_STATS_ALIGN = "stats / grad2d must be 16-byte aligned"
_RECORD_ALIGN = "record must be 16-byte aligned"
_FEATURES = _OPENING + [(dict(n=BIG_N), RANGE), (dict(pc=BIG_PC), RANGE), (dict(project_state=NULL), NULL_ARG), (dict(bin_state=NULL), NULL_ARG),
                        (dict(channels=0), "channels out of range (1 .. 512)"), (dict(channels=513), "channels out of range (1 .. 512)"),
                        (dict(n=-1, project_state=NULL), RANGE), (dict(project_state=NULL, channels=0), NULL_ARG)]
_BACKWARD = _OPENING + [(dict(n=BIG_N), RANGE), (dict(pc=BIG_PC), RANGE), (dict(project_state=NULL), NULL_ARG), (dict(bin_state=NULL), NULL_ARG),
                        (dict(accum=NULL), NULL_ARG), (dict(grad2d=NULL), NULL_ARG), (dict(n=-1, project_state=NULL), RANGE)]
_ALL_GRADS = "grad_image, grad_depth and grad_alpha are all NULL"
TABLE = {
    "gsplat_densify_stats": _stats_rows("project_state", _STATS_ALIGN),
    "gsplat_densify_stats_abs": _stats_rows("project_state", _STATS_ALIGN),
    # (behind the arena's checks the entry's own follow: a misaligned record is refused there; grad2d lies inside the arena)
    "gsplat_frame_densify_stats": _frame_rows("stats", SMALL_B, [(dict(stats=ODD), _STATS_ALIGN), (dict(stats=ODD, frame_bytes=SHORT), SMALL_B)]),
    "gsplat_frame_densify_stats_abs": _frame_rows("stats", SMALL_B, [(dict(stats=ODD), _STATS_ALIGN), (dict(stats=ODD, frame_bytes=SHORT), SMALL_B)]),
    "gsplat_visible_set": _OPENING + [(dict(n=BIG_N), RANGE), (dict(project_state=NULL), NULL_ARG), (dict(visible=NULL), NULL_ARG),
                                      (dict(n=-1, project_state=NULL), RANGE)],
    "gsplat_frame_visible_set": _frame_rows("visible", SMALL),
    "gsplat_contribution": _OPENING + [(dict(n=BIG_N), RANGE), (dict(pc=BIG_PC), RANGE), (dict(project_state=NULL), NULL_ARG),
                                       (dict(bin_state=NULL), NULL_ARG), (dict(record=NULL), NULL_ARG), (dict(record=ODD), _RECORD_ALIGN),
                                       (dict(n=-1, project_state=NULL), RANGE), (dict(bin_state=NULL, record=ODD), NULL_ARG)],
    "gsplat_frame_contribution": _frame_rows("record", SMALL, [(dict(record=ODD), _RECORD_ALIGN), (dict(record=ODD, frame_bytes=SHORT), SMALL)]),
    "gsplat_features_forward": _FEATURES + [(dict(features=NULL), NULL_ARG), (dict(out=NULL), NULL_ARG)],
    "gsplat_features_adjoint": _FEATURES + [(dict(grad_out=NULL), NULL_ARG), (dict(grad_features=NULL), NULL_ARG)],
    "gsplat_rasterize_backward_abs": _BACKWARD + [(dict(grad_image=NULL), NULL_ARG)],
    # (any one of the three upstream gradients may be left out, but not all; the all-NULL refusal comes before the NULL arguments)
    "gsplat_rasterize_backward_aux_abs": _BACKWARD + [(dict(accum_aux=NULL), NULL_ARG), (dict(grad_image=NULL, grad_depth=NULL, grad_alpha=NULL), _ALL_GRADS),
                                                      (dict(accum=NULL, grad_image=NULL, grad_depth=NULL, grad_alpha=NULL), _ALL_GRADS),
                                                      (dict(n=-1, grad_image=NULL, grad_depth=NULL, grad_alpha=NULL), RANGE)],
}
CASES = [(name, bad, text) for name, rows in TABLE.items() for bad, text in rows] + \
        [(name, dict(_EVERYTHING_BAD, view=NULL, **{a: NULL for a in ARGS[name] if a not in _NOT_POINTERS}), NULL_VIEW) for name in ARGS]


def _case_id(case):
    return case[0][len("gsplat_"):] + "-" + ",".join(f"{k}={'NULL' if v is None else v}" for k, v in case[1].items() if k in ("n", "pc") or len(case[1]) < 6)


@pytest.fixture(scope="module")
def host():
    """(lib, a 256-byte aligned host address with room behind it, the good view, the view with H = 0) -- nothing here is ever read."""
    buf = (C.c_char * 4096)()
    yield abi.lib(), (C.addressof(buf) + 255) // 256 * 256, abi.make_view(64, 64, 50.0, 50.0, 32.0, 32.0), abi.make_view(0, 64, 50.0, 50.0, 32.0, 32.0)
    del buf


def test_the_table_covers_every_entry_and_every_kind_of_bad_argument():
    assert set(TABLE) == set(ARGS) and len(ARGS) == 12
    for name, rows in TABLE.items():
        assert len(abi.SIGNATURES[name][1]) == len(ARGS[name]), name
        single = [next(iter(bad.items())) for bad, _ in rows if len(bad) == 1]
        assert {("view", NULL), ("view", H0), ("n", -1), ("n", BIG_N), ("pc", -1)} <= set(single), name
        required = [a for a in ARGS[name] if a not in _NOT_POINTERS + _NULL_BY_DEFAULT + ("grad_depth", "grad_alpha")
                    and not (name.endswith("aux_abs") and a == "grad_image")]
        assert {(a, NULL) for a in required} <= set(single), name
        assert any(len(bad) == 2 and bad.get("n") == -1 for bad, _ in rows), name
        if "frame" in ARGS[name]:
            assert ("frame_bytes", SHORT) in single and ("frame", ODD) in single and any(bad == dict(n=BIG_N, frame_bytes=SHORT) for bad, _ in rows), name


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_a_bad_argument_is_refused_with_the_exact_text(host, case):
    lib, p, view, view_h0 = host
    name, bad, text = case
    n, pc = bad.get("n", N), bad.get("pc", PAIRS)
    vals = []
    for a in ARGS[name]:
        v = bad.get(a, "good")
        if a == "n" or a == "pc":
            vals.append(n if a == "n" else pc)
        elif a == "view":
            vals.append(None if v is NULL else C.byref(view_h0 if v == H0 else view))
        elif a == "frame_bytes":
            flags = abi.GSPLAT_FRAME_BACKWARD if "densify" in name else 0
            vals.append(lib.gsplat_frame_bytes(N, PAIRS, C.byref(view), flags) - (1 if v == SHORT else 0))
        elif a == "channels":
            vals.append(8 if v == "good" else v)
        elif a in ("grad2d_zeroed", "det_scratch_bytes"):
            vals.append(0)
        elif v is NULL or (v == "good" and a in _NULL_BY_DEFAULT):
            vals.append(None)
        else:
            vals.append(C.c_void_p(p + 4 if v == ODD else p))
    status = getattr(lib, name)(*vals)
    assert status == abi.GSPLAT_ERR_BAD_ARG, (name, bad, status, lib.gsplat_last_error())
    assert lib.gsplat_last_error().decode() == f"{name}: {text}", (name, bad)
