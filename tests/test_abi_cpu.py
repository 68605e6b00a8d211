"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol include/*.h declares
(no compute calls without a GPU), the Python mirror agrees with the header, and the product fails loudly on CPU."""
import ctypes as C
import importlib
import os

import pytest
import torch

from tests.abi_checks import exported_functions, header_defines, header_functions, refused

abi = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd._abi")


def test_header_and_python_mirror_agree():
    names = header_functions()
    assert len(names) >= 16
    assert sorted(abi.SIGNATURES) == names


def test_header_constants_and_python_mirror_agree():
    """Every integer #define of the header that the Python host mirrors (flags, status / scene codes, ABI version) has the
    header's value there; the flag bits of one call are distinct."""
    defs = header_defines()
    assert defs["GSPLAT_ABI_VERSION"] == abi.ABI_VERSION
    mirrored = [k for k in defs if hasattr(abi, k)]
    assert {"GSPLAT_PROJECT_COLOUR_FUSED", "GSPLAT_PROJECT_COUNTS_MAPPED", "GSPLAT_PROJECT_SAVE_SH_JACOBIAN", "GSPLAT_PROJECT_COUNTS_LATE",
            "GSPLAT_BACKWARD_SH_JACOBIAN"} <= set(mirrored)
    for k in mirrored:
        assert getattr(abi, k) == defs[k], k
    project_flags = [defs[k] for k in defs if k.startswith("GSPLAT_PROJECT_")]
    assert len(set(project_flags)) == len(project_flags) and all(f & (f - 1) == 0 for f in project_flags)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(abi.LIB_PATH), "build the library first: python __graft_entry__.py"
    lib = C.CDLL(abi.LIB_PATH)
    for name in header_functions():
        assert hasattr(lib, name), f"{name} is declared in include/gsplat_mi355x.h but not exported"
    assert abi.lib().gsplat_abi_version() == abi.ABI_VERSION


def test_library_exports_nothing_but_the_declared_entry_points():
    """Every defined dynamic FUNCTION symbol of the product library is an entry point of include/gsplat_mi355x.h (a helper with C
    linkage inside the extern "C" block would be exported silently: round 2's carve_det)."""
    funcs = exported_functions()
    declared = set(header_functions())
    stray = [f for f in funcs if f not in declared and not f.startswith(("_init", "_fini", "__hip", "_ZN", "_ZT", "_ZS"))]
    assert not stray, f"non-ABI symbols exported by the product library: {stray}"
    assert not [f for f in funcs if f.startswith("gsplat_") and f not in declared], "exported gsplat_* symbol missing from the header"


def test_struct_layouts_match_header():
    # sizes the C side static_asserts / uses: gsplat_view 14 x 4 B, gsplat_counts 32 B, 9 and 8 pointer-sized fields
    assert C.sizeof(abi.View) == 56
    assert C.sizeof(abi.Counts) == 32
    assert C.sizeof(abi.Gaussians) == 9 * 8
    assert C.sizeof(abi.GaussianGrads) == 8 * 8


def test_size_queries_are_pure_host_functions():
    lib = abi.lib()
    v = abi.make_view(1080, 1920, 1100.0, 1100.0, 960.0, 540.0)
    n, p = 1_000_000, 2_720_508
    lists = 120 * 135                                    # 16 x 8-pixel half-tile lists of a 1920 x 1080 image
    assert lib.gsplat_project_state_bytes(n, C.byref(v)) >= n * (84 + 48) + lists * 12      # records + streams + the saved SH Jacobian
    assert lib.gsplat_project_state_bytes(n, None) == -1
    assert lib.gsplat_bin_state_bytes(p, C.byref(v)) >= p * 5                               # sorted ids + one mask byte per pair
    assert lib.gsplat_bin_scratch_bytes(p, C.byref(v)) >= p * 16
    assert lib.gsplat_project_scratch_bytes(n) >= 256 * 64 + 64          # the persistent counter block: 256 shards + the arrival counter
    # the layout queries (tests and tools only): the arrays lie inside the buffer, in 256-byte steps, without overlap, and the
    # sizes are the size queries' -- with no GPU in sight
    lay = abi.StateLayout()
    assert lib.gsplat_project_state_layout(n, C.byref(v), C.byref(lay)) == abi.GSPLAT_OK
    assert lay.bytes == lib.gsplat_project_state_bytes(n, C.byref(v)) and lay.lists == lists and (lay.lists_x, lay.lists_y) == (120, 135)
    need = dict(counts=32, rec=n * 64, rect=n * 8, depth=n * 4, tiles=n * 4, mask=n * 4, ranges=lists * 8, order=lists * 4,
                class_bounds=32, kj=n * 48)
    spans = sorted((getattr(lay, k), getattr(lay, k) + b, k) for k, b in need.items())
    assert spans[0][0] >= 0 and spans[-1][1] <= lay.bytes and all(o % 256 == 0 for o, _, _ in spans)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    bl = abi.BinLayout()
    assert lib.gsplat_bin_state_layout(p, C.byref(v), C.byref(bl)) == abi.GSPLAT_OK
    assert bl.bytes == lib.gsplat_bin_state_bytes(p, C.byref(v)) and bl.sorted_ids == 0
    assert bl.pair_mask >= p * 4 and bl.pair_mask % 256 == 0 and bl.pair_mask + p <= bl.bytes
    assert lib.gsplat_bin_state_layout(0, C.byref(v), C.byref(bl)) == abi.GSPLAT_OK and bl.bytes == lib.gsplat_bin_state_bytes(0, C.byref(v))


def test_scene_classification_mirrors_reference_conventions():
    lib = abi.lib()
    assert lib.gsplat_classify_counts(C.byref(abi.Counts(0, 0, 0, 0, 0))) == abi.GSPLAT_SCENE_ALL_CULLED
    assert lib.gsplat_classify_counts(C.byref(abi.Counts(5, 0, 0, 0, 0))) == abi.GSPLAT_SCENE_ALL_OFFSCREEN
    assert lib.gsplat_classify_counts(C.byref(abi.Counts(5, 3, 7, 4, 0))) == abi.GSPLAT_SCENE_OK


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    lib = abi.lib()
    v = abi.make_view(64, 64, 50.0, 50.0, 32.0, 32.0)
    assert lib.gsplat_project(None, None, C.byref(v), None, None, 0, None, None, 0, None) == 1
    assert b"NULL" in lib.gsplat_last_error()
    v0 = abi.make_view(64, 64, 50.0, 50.0, 32.0, 32.0, T=0)          # every T >= 1 is accepted (reference render.py:62-64)
    assert lib.gsplat_bin(0, 0, C.byref(v0), None, None, None, 0, None) == 1
    assert b"T must be" in lib.gsplat_last_error()
    v8 = abi.make_view(64, 64, 50.0, 50.0, 32.0, 32.0, T=8)
    assert lib.gsplat_bin(0, 0, C.byref(v8), None, None, None, 0, None) == 1
    assert b"state is NULL" in lib.gsplat_last_error()
    lay, bl = abi.StateLayout(), abi.BinLayout()
    bad = abi.make_view(0, 64, 50.0, 50.0, 32.0, 32.0)
    for status in (lib.gsplat_project_state_layout(4, None, C.byref(lay)), lib.gsplat_project_state_layout(4, C.byref(v), None),
                   lib.gsplat_project_state_layout(-1, C.byref(v), C.byref(lay)), lib.gsplat_project_state_layout(4, C.byref(bad), C.byref(lay))):
        refused(lib, status, "gsplat_project_state_layout")
    for status in (lib.gsplat_bin_state_layout(4, None, C.byref(bl)), lib.gsplat_bin_state_layout(4, C.byref(v), None),
                   lib.gsplat_bin_state_layout(-1, C.byref(v), C.byref(bl))):
        refused(lib, status, "gsplat_bin_state_layout")


def _host_words(n=16):
    """A non-NULL address for an argument check to look at; every call below is refused on the host before anything is launched."""
    buf = (C.c_float * n)()
    return buf, C.cast(buf, C.c_void_p)


def test_loss_entries_reject_bad_arguments_on_the_host():
    """gsplat_loss / gsplat_loss_forward / gsplat_loss_backward: a NULL required pointer, H, W or batch <= 0 and batch > 65535 (the
    grid's z extent) come back as GSPLAT_ERR_BAD_ARG with a message naming the entry."""
    lib = abi.lib()
    keep, p = _host_words()

    def loss(pred=p, target=p, batch=1, H=4, W=4, values=p, grad=p, scratch=p):
        return lib.gsplat_loss(pred, target, batch, H, W, 0.8, 0.2, values, grad, scratch, None)

    def fwd(pred=p, target=p, batch=1, H=4, W=4, values=p, total=p, scratch=p):
        return lib.gsplat_loss_forward(pred, target, batch, H, W, 0.8, 0.2, 1.0, values, total, scratch, 1, None)

    def bwd(pred=p, target=p, batch=1, H=4, W=4, upstream=p, grad=p, scratch=p):
        return lib.gsplat_loss_backward(pred, target, batch, H, W, 0.8, 0.2, 1.0, upstream, grad, scratch, None)

    for fn, name, required in ((loss, "gsplat_loss", ("pred", "target", "values", "scratch")),
                               (fwd, "gsplat_loss_forward", ("pred", "target", "values", "scratch")),
                               (bwd, "gsplat_loss_backward", ("pred", "target", "grad", "scratch"))):
        for arg in required:
            refused(lib, fn(**{arg: None}), name)
        for bad in (dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(batch=0), dict(batch=-2), dict(batch=65536), dict(batch=1 << 40)):
            refused(lib, fn(**bad), name)
    del keep


def test_optimiser_entries_reject_bad_arguments_on_the_host():
    lib = abi.lib()
    keep, p = _host_words()
    refused(lib, lib.gsplat_clip_grad_norm(-1, p, 1.0, p, p, None), "gsplat_clip_grad_norm")
    refused(lib, lib.gsplat_clip_grad_norm(4, None, 1.0, p, p, None), "gsplat_clip_grad_norm")
    refused(lib, lib.gsplat_clip_grad_norm(4, p, 1.0, None, p, None), "gsplat_clip_grad_norm")
    nine = (abi.AdamGroup * 9)(*[abi.AdamGroup(0, None, None, None, None, 0.01, 1, None) for _ in range(9)])
    refused(lib, lib.gsplat_adam_step_multi(9, nine, 0.9, 0.999, 1e-15, None), "gsplat_adam_step_multi")
    assert lib.gsplat_adam_step_multi(8, nine, 0.9, 0.999, 1e-15, None) == abi.GSPLAT_OK       # eight empty groups: nothing to launch
    refused(lib, lib.gsplat_adam_step_multi(-1, nine, 0.9, 0.999, 1e-15, None), "gsplat_adam_step_multi")
    refused(lib, lib.gsplat_adam_step_multi(1, None, 0.9, 0.999, 1e-15, None), "gsplat_adam_step_multi")
    for bad in (abi.AdamGroup(0, None, None, None, None, 0.01, 0, None),             # step < 1 (the bias correction divides by 1 - b^step)
                abi.AdamGroup(4, p, p, p, p, 0.01, -1, None),
                abi.AdamGroup(-1, p, p, p, p, 0.01, 1, None),                        # n < 0
                abi.AdamGroup(4, p, None, p, p, 0.01, 1, None)):                     # a NULL array of a non-empty group
        two = (abi.AdamGroup * 2)(abi.AdamGroup(0, None, None, None, None, 0.01, 1, None), bad)
        refused(lib, lib.gsplat_adam_step_multi(2, two, 0.9, 0.999, 1e-15, None), "gsplat_adam_step_multi")
        assert b"group 1" in lib.gsplat_last_error()
    refused(lib, lib.gsplat_adam_step(-1, p, p, p, p, 0.01, 0.9, 0.999, 1e-15, 1, None, None), "gsplat_adam_step")
    refused(lib, lib.gsplat_adam_step(4, p, p, p, p, 0.01, 0.9, 0.999, 1e-15, 0, None, None), "gsplat_adam_step")
    refused(lib, lib.gsplat_adam_step(4, p, p, None, p, 0.01, 0.9, 0.999, 1e-15, 1, None, None), "gsplat_adam_step")
    del keep


def test_loss_scratch_bytes_matches_the_layout_in_the_source():
    """gsplat_loss_scratch_bytes = [two partial sums per 32 x 16 tile and image, rounded up to 256 bytes | with_grad: the nine
    partial-derivative planes, batch x 9 x H x W floats] (csrc/gsplat_loss.hip); -1 for a size that is none."""
    lib = abi.lib()
    for batch, H, W in ((1, 1, 1), (3, 17, 33), (2, 1080, 1920), (1, 16, 32), (65535, 16, 32)):
        tiles = batch * ((W + 31) // 32) * ((H + 15) // 16)
        sums = 256 * ((tiles * 2 * 4 + 255) // 256)
        assert lib.gsplat_loss_scratch_bytes(batch, H, W, 0) == sums
        assert lib.gsplat_loss_scratch_bytes(batch, H, W, 1) == sums + batch * 9 * H * W * 4
    for batch, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4)):
        assert lib.gsplat_loss_scratch_bytes(batch, H, W, 1) == -1
    assert lib.gsplat_clip_scratch_bytes() == 1024 * 4


def test_unknown_backward_flags_are_refused_before_anything_else():
    """A flag bit a backward entry does not define is refused first (with host arguments only: nothing reaches the GPU), so that
    a library that does not know a flag cannot quietly do something else -- overwrite where the caller adds, say."""
    lib = abi.lib()
    v = abi.make_view(64, 64, 50.0, 50.0, 32.0, 32.0)
    unknown = 1 << 5
    assert lib.gsplat_backward(None, None, C.byref(v), None, 0, 0, None, None, None, None, 0, unknown, None) == abi.GSPLAT_ERR_BAD_ARG
    assert b"unknown flag" in lib.gsplat_last_error()
    group = abi.AdamGroup()
    assert lib.gsplat_backward_adam_rest(None, None, C.byref(v), None, 0, 0, None, None, None, 0, unknown, C.byref(group), 0.9, 0.999,
                                         1e-15, None) == abi.GSPLAT_ERR_BAD_ARG
    assert b"unknown flag" in lib.gsplat_last_error()
    for flags in (unknown, abi.GSPLAT_BACKWARD_PHASE_RASTER, abi.GSPLAT_BACKWARD_GRAD2D_DIRTY):     # (composite-only bits, too)
        assert lib.gsplat_project_backward(None, None, C.byref(v), None, None, None, flags, None) == abi.GSPLAT_ERR_BAD_ARG
        assert b"unknown flag" in lib.gsplat_last_error()
    # a defined bit with the same NULL arguments gets as far as the argument checks
    assert lib.gsplat_backward(None, None, C.byref(v), None, 0, 0, None, None, None, None, 0, abi.GSPLAT_BACKWARD_ACCUMULATE, None) == 1
    assert b"unknown flag" not in lib.gsplat_last_error()


def test_no_cpu_fallback(gs):
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.render(z(4, 3), z(4, 3), z(4), z(4, 3, 3), torch.eye(4), 16, 16, 10., 10., 8., 8.)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.build_sigma_from_params(z(4, 3), z(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs.evaluate_sh(z(4, 3), z(4, 45), z(4, 3), torch.eye(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # any tile size reaches the same check
        gs.render(z(4, 3), z(4, 3), z(4), z(4, 3, 3), torch.eye(4), 16, 16, 10., 10., 8., 8., T=8)
    with pytest.raises(ValueError, match="T must be"):
        gs.render(z(4, 3), z(4, 3), z(4), z(4, 3, 3), torch.eye(4), 16, 16, 10., 10., 8., 8., T=0)


def test_small_helpers_match_oracle():
    from oracle import torch_port as tp
    gs = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd")
    g = torch.Generator().manual_seed(3)
    q = torch.randn(7, 4, generator=g, dtype=torch.float64)
    assert torch.allclose(gs.quat_to_rotmat(q), tp.rotmat_from_quat(q))
    m = torch.randn(9, 2, 2, generator=g, dtype=torch.float64)
    assert torch.allclose(gs.inv2x2(m), tp.inv2x2(m))
    assert gs.scale_intrinsics(540, 960, 1080, 1920, 1100., 1090., 961.5, 538.25) == tp.scale_intrinsics(
        540, 960, 1080, 1920, 1100., 1090., 961.5, 538.25)
    pc = torch.randn(11, 3, generator=g, dtype=torch.float64) + torch.tensor([0, 0, 5.0])
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    a, b = gs.project_points(pc, c2w, 500., 510., 320., 240.), tp.project_points(pc, c2w, 500., 510., 320., 240.)
    for x, y in zip(a, b):
        assert torch.allclose(x, y)
    assert abs(gs.HARMONICS['SH_C3_xyz'] - tp.SH_K[10]) < 1e-15 and len(gs.HARMONICS) == 16
