"""The image metrics on the GPU (csrc/gsplat_metrics.hip) against the float64 oracle (tests/metrics_oracle.py): the
shapes where the kernels can go wrong, determinism, the padding of the corrected image, confined writes, and Trainer.evaluate.

Bounds (nothing here comes from what the kernels give):
  l1, ssim without correction   those tests/test_gpu_loss.py uses against float64 for the same quantities (calibrated there on the
                                reference's own fp32 run): |l1 - ref| <= 2e-6 |ref| + 1e-7,  |ssim - ref| <= 1e-5 |1 - ref| + 1e-6.
  mse, psnr without correction  4 x the largest fp32-vs-float64 error of a float32 torch restatement over the sweep's inputs, measured
                                on the CPU by `python -m tests.metrics_cases`: mse 1.05e-7 relative, psnr 1.80e-6 dB
                                -> MSE_REL = 4.2e-7, PSNR_ABS = 7.2e-6.  (The device's order of summation differs from torch's and
                                neither is the more accurate by construction.)  PSNR is compared where mse > 0 only.
  with the correction           8 x the oracle's own sensitivity -- the largest change of each output when every input of the case is
                                moved by a random +-1 fp32 ulp, 8 seeded draws on the CPU (tests/metrics_cases.py: per case; over
                                the sweep psnr 2e-7 .. 5e-6 dB, ssim 2e-9 .. 1.3e-8, l1 2e-9 .. 2.7e-8, mse 3e-10 .. 2.2e-9, affine
                                1.3e-8 .. 5.3e-7) -- plus the bound without correction; the affine, which has none, plus its own
                                rounding to fp32 (2^-24 of max(1, |value|)).  The sweep's colours are uniform random: cond(A) of the
                                normal equations is below COND_MAX = 200 wherever an image has at least 8 valid pixels (measured:
                                33 .. 100).
  the one-pixel image, corrected  four unknowns per row against one equation: the exact residual is 0 (t has no ridge), and what the
                                oracle's float64 gives for mse (0, or 1e-34) is its own rounding.  The device rounds the affine to
                                fp32 and applies it with three fp32 FMAs: |M x + t - y| <= 2^-24 (sum |M_k x_k| + |t|) from the
                                affine's rounding + 3 x 2^-24 x 2 from the FMAs (every partial sum is below 2) <= 8 x 2^-24 =
                                EXACT_FIT_ABS.  So there l1 gets EXACT_FIT_ABS and mse its square on top of the bounds above, and
                                psnr -- the logarithm of a number that is 0 up to rounding -- is not compared.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import metrics_cases as mc
from tests import metrics_oracle as mo
from tests import view_table_harness as vt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
MSE_REL = 4.2e-7          # 4 x 1.05e-7 (see above)
PSNR_ABS = 7.2e-6         # 4 x 1.80e-6 dB
COND_MAX = 200.0
K_SENS = 8.0
EXACT_FIT_ABS = 8 * 2.0 ** -24          # the fp32 residual of a fit that is exact (see above)
GUARD = 4096
PATTERN = 0xA5
KEYS = ("psnr", "ssim", "l1", "mse")


@pytest.fixture(scope="module")
def metrics():
    return importlib.import_module(PKG + ".metrics")


def _plain_bounds(ref):
    """{name: [B]} for float64 reference values {name: [B]} (NaN where the reference is NaN: compared separately)."""
    return dict(l1=2e-6 * np.abs(ref["l1"]) + 1e-7, ssim=1e-5 * np.abs(1 - ref["ssim"]) + 1e-6, mse=MSE_REL * ref["mse"],
                psnr=np.full_like(ref["psnr"], PSNR_ABS))


def _check(got, ref, bounds, what, psnr_above_mse=0.0):
    """got: ImageMetrics of [B] tensors; ref: oracle dict.  Prints every figure before it asserts.  PSNR is compared where the
    reference's mse is above `psnr_above_mse` only."""
    for k in KEYS:
        g, r, b = getattr(got, k).detach().cpu().double().numpy().reshape(-1), np.asarray(ref[k]).reshape(-1), np.asarray(bounds[k]).reshape(-1)
        print(f"{what} {k}: got {g} ref {r} |err| {np.abs(g - r)} allowed {b}")
        for i in range(len(r)):
            if np.isnan(r[i]):
                assert np.isnan(g[i]), f"{what}: {k}[{i}] must be NaN, got {g[i]!r}"
            elif k == "psnr" and not ref["mse"].reshape(-1)[i] > psnr_above_mse:
                assert g[i] > 0 and not np.isnan(g[i]), f"{what}: psnr[{i}] of a vanishing error must be large or +inf, got {g[i]!r}"
            elif np.isinf(r[i]):
                assert g[i] == r[i], f"{what}: {k}[{i}] must be {r[i]!r}, got {g[i]!r}"
            else:
                assert abs(g[i] - r[i]) <= b[i], f"{what}: {k}[{i}] {g[i]!r} vs {r[i]!r}: |err| {abs(g[i] - r[i]):.3e} > {b[i]:.3e}"


def _corrected_bounds(ref, sens):
    plain = _plain_bounds(ref)
    return {k: K_SENS * sens[k] + np.nan_to_num(plain[k], nan=0.0) for k in KEYS}


def _check_affine(got, ref, sens, what):
    g, r = got.detach().cpu().double().numpy().reshape(-1, 3, 4), np.asarray(ref).reshape(-1, 3, 4)
    for b in range(r.shape[0]):
        if np.isnan(r[b]).any():
            assert np.isnan(g[b]).all(), f"{what}: affine[{b}] must be NaN"
            continue
        bound = K_SENS * sens[b] + 2.0 ** -24 * np.maximum(1.0, np.abs(r[b]))
        print(f"{what} affine[{b}]: max |err| {np.abs(g[b] - r[b]).max():.3e} allowed {bound.min():.3e}")
        assert (np.abs(g[b] - r[b]) <= bound).all(), f"{what}: affine[{b}] max |err| {np.abs(g[b] - r[b]).max():.3e} > {bound.min():.3e}"


def _dev(a):
    return None if a is None else torch.tensor(a, device=DEV)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour_correct", [False, True], ids=["plain", "cc"])
@pytest.mark.parametrize("kind", mc.MASKS)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_sweep(metrics, shape, kind, colour_correct):
    pred, tgt = mc.inputs(shape)
    mask = mc.mask_of(kind, shape)
    ref = mc.reference(shape, kind, colour_correct)
    got = metrics.image_metrics(_dev(pred), _dev(tgt), _dev(mask), colour_correct=colour_correct)
    what = f"{shape} {kind} cc={colour_correct}"
    assert all(tuple(getattr(got, k).shape) == (shape[0],) and getattr(got, k).dtype == torch.float32 for k in KEYS)
    if not colour_correct:
        assert got.affine is None
        _check(got, ref, _plain_bounds(ref), what)
        return
    for n_valid, cond in mc.condition_numbers(shape, kind):
        assert n_valid < 8 or cond < COND_MAX, (what, n_valid, cond)
    sens = mc.ulp_sensitivity(shape, kind)
    assert tuple(got.affine.shape) == (shape[0], 3, 4)
    _check_affine(got.affine, ref["affine"], sens["affine"], what)
    bounds = _corrected_bounds(ref, sens)
    if shape[1] * shape[2] == 1:                   # the fit is exact: the device's residual is fp32 rounding, the oracle's float64 rounding
        bounds["l1"] = bounds["l1"] + EXACT_FIT_ABS
        bounds["mse"] = bounds["mse"] + EXACT_FIT_ABS ** 2
    _check(got, ref, bounds, what, psnr_above_mse=EXACT_FIT_ABS ** 2 if shape[1] * shape[2] == 1 else 0.0)


def test_unbatched_call_and_the_conveniences(metrics):
    pred, tgt = mc.inputs((1, 17, 33))
    mask = mc.mask_of("random", (1, 17, 33))
    x, y, m = _dev(pred[0]), _dev(tgt[0]), _dev(mask[0])
    one = metrics.image_metrics(x, y, m, colour_correct=True)
    batch = metrics.image_metrics(x[None], y[None], m[None], colour_correct=True)
    assert all(getattr(one, k).dim() == 0 for k in KEYS) and tuple(one.affine.shape) == (3, 4)
    assert all(vt._same(getattr(one, k), getattr(batch, k)[0]) for k in KEYS) and vt._same(one.affine, batch.affine[0])
    plain = metrics.image_metrics(x, y, m)
    assert vt._same(metrics.psnr(x, y, m), plain.psnr) and vt._same(metrics.ssim(x, y, m), plain.ssim)
    assert vt._same(metrics.fit_affine(x, y, m), one.affine) and vt._same(metrics.fit_affine(x[None], y[None], m[None]), batch.affine)
    assert vt._same(metrics.image_metrics(x, y, m.to(torch.uint8) * 3).l1, plain.l1)          # uint8, nonzero = valid


# ---- near convergence ---------------------------------------------------------------------------------------------------------------

def _smooth(shape, seed):
    """A smooth image in [0.2, 0.8] (low-order sinusoids per channel), the regime training ends in."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, shape[1]), np.linspace(0, 1, shape[2]), indexing="ij")
    img = np.stack([0.5 + 0.3 * np.sin(2 * np.pi * (rng.uniform(0.3, 1.5) * xx + rng.uniform(0.3, 1.5) * yy) + rng.uniform(0, 6))
                    for _ in range(3 * shape[0])], -1)
    return np.ascontiguousarray(img.reshape(shape[1], shape[2], shape[0], 3).transpose(2, 0, 1, 3)).astype(np.float32)


def test_near_convergence_and_an_image_against_itself(metrics):
    shape = (2, 40, 70)
    tgt = _smooth(shape, 3)
    pred = (tgt + 1e-4 * np.random.default_rng(4).standard_normal(tgt.shape)).astype(np.float32)
    ref = mo.image_metrics(pred, tgt)
    got = metrics.image_metrics(_dev(pred), _dev(tgt))
    _check(got, ref, _plain_bounds(ref), "near convergence")
    same = metrics.image_metrics(_dev(tgt), _dev(tgt.copy()))
    assert torch.isposinf(same.psnr).all() and (same.ssim == 1.0).all() and (same.l1 == 0.0).all() and (same.mse == 0.0).all()
    noise = mc.inputs((1, 17, 33))[0]
    same = metrics.image_metrics(_dev(noise), _dev(noise.copy()), _dev(mc.mask_of("random", (1, 17, 33))))
    assert torch.isposinf(same.psnr).all() and (same.ssim == 1.0).all() and (same.l1 == 0.0).all() and (same.mse == 0.0).all()


# ---- determinism --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour_correct", [False, True], ids=["plain", "cc"])
def test_same_bits_every_call_every_stream_and_image_by_image(metrics, colour_correct):
    shape = (3, 40, 70)
    pred, tgt = map(_dev, mc.inputs(shape))
    mask = _dev(mc.mask_of("random", shape))
    first = metrics.image_metrics(pred, tgt, mask, colour_correct=colour_correct)
    again = metrics.image_metrics(pred, tgt, mask, colour_correct=colour_correct)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = metrics.image_metrics(pred, tgt, mask, colour_correct=colour_correct)
    torch.cuda.current_stream().wait_stream(side)
    fields = KEYS + (("affine",) if colour_correct else ())
    for k in fields:
        assert vt._same(getattr(first, k), getattr(again, k)), k
        assert vt._same(getattr(first, k), getattr(other, k)), k
    for b in range(shape[0]):
        one = metrics.image_metrics(pred[b], tgt[b], mask[b], colour_correct=colour_correct)
        for k in fields:
            assert vt._same(getattr(first, k)[b], getattr(one, k)), (k, b)


# ---- the padding of the corrected image -----------------------------------------------------------------------------------------------

def test_the_window_pads_the_corrected_image_with_zero_not_with_t(metrics):
    """target = 2 pred + 0.1 inside [0, 1]: the fitted t is 0.1, and a kernel that corrected the padding too would see a border of 0.1
    around x -- the oracle of THAT image (built here) is further from the true one than 10 x the bound, so the check can tell."""
    shape = (1, 17, 33)
    pred = np.random.default_rng(12).uniform(0, 0.45, shape + (3,)).astype(np.float32)
    tgt = (2 * pred + np.float32(0.1)).astype(np.float32)
    ref = mo.image_metrics(pred, tgt, None, True)
    got = metrics.image_metrics(_dev(pred), _dev(tgt), colour_correct=True)
    plain = _plain_bounds(ref)
    assert abs(ref["affine"][0, 0, 3] - 0.1) < 1e-5
    # the wrong answer: x padded with clamp(t), y with 0 -- five pixels of border, then the map of the interior
    a = ref["affine"][0]
    xc = np.clip(pred[0].astype(np.float64) @ a[:, :3].T + a[:, 3], 0, 1)
    xp = np.broadcast_to(np.clip(a[:, 3], 0, 1), (27, 43, 3)).copy()
    xp[5:-5, 5:-5] = xc
    yp = np.zeros((27, 43, 3))
    yp[5:-5, 5:-5] = tgt[0]
    wrong = mo.ssim_map(xp, yp)[5:-5, 5:-5].mean()
    sens = mc.ulp_sensitivity_of(pred, tgt, None, ref)
    bound = K_SENS * sens["ssim"][0] + plain["ssim"][0]
    print(f"padding: ssim got {float(got.ssim[0])!r} ref {ref['ssim'][0]!r} padded-with-t {wrong!r} allowed {bound:.3e}")
    assert abs(wrong - ref["ssim"][0]) > 10 * bound
    assert abs(float(got.ssim[0]) - ref["ssim"][0]) <= bound


# ---- consistency ------------------------------------------------------------------------------------------------------------------------

def test_correction_equals_exposure_apply_then_plain_metrics(gs, metrics):
    shape = (2, 11, 45)
    pred, tgt = map(_dev, mc.inputs(shape))
    mask = _dev(mc.mask_of("random", shape))
    cc = metrics.image_metrics(pred, tgt, mask, colour_correct=True)
    assert vt._same(metrics.fit_affine(pred, tgt, mask), cc.affine)
    plain = metrics.image_metrics(gs.exposure.apply(pred, cc.affine).clamp(0, 1), tgt, mask)
    ref = {k: getattr(plain, k).cpu().double().numpy() for k in KEYS}
    _check(cc, ref, _plain_bounds(ref), "cc vs exposure.apply + clamp")


def test_ssim_agrees_with_the_training_loss(gs, metrics):
    for shape in ((1, 17, 33), (1, 40, 70)):
        pred, tgt = map(_dev, mc.inputs(shape))
        _, values = gs.losses.compute_loss_device(pred[0], tgt[0])
        got, loss_term = float(metrics.ssim(pred[0], tgt[0])), float(values[1])
        ref = mc.reference(shape, "none", False)["ssim"][0]
        allowed = 2 * (1e-5 * abs(1 - ref) + 1e-6)                        # the sum of the two bounds against float64
        print(f"ssim {shape}: metrics {got!r}, 1 - loss term {1 - loss_term!r}, float64 {ref!r}, allowed {allowed:.3e}")
        assert abs(got - (1 - loss_term)) <= allowed


# ---- confined writes ------------------------------------------------------------------------------------------------------------------

class _Guarded:
    """`nbytes` usable bytes in the middle of an allocation whose margins (GUARD bytes each side) hold a bit pattern."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0 and self.nbytes % 4 == 0

    def ptr(self):
        import ctypes as C
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def floats(self):
        return self.buf[GUARD:GUARD + self.nbytes].view(torch.float32)

    def margins_intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.nbytes:] == PATTERN).all())


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 33), (3, 40, 70)], ids=lambda s: "x".join(map(str, s)))
def test_nothing_is_written_outside_out_affine_and_scratch(metrics, shape):
    """gsplat_metrics_forward (with and without the correction) and gsplat_metrics_fit_affine on buffers of exactly the stated sizes
    between margins holding a bit pattern: the margins come back unchanged, the inputs too, every output element was written (the
    pattern 0xA5A5A5A5 is a float no metric equals) and equals the wrapper's.  Read-back only."""
    abi = importlib.import_module(PKG + "._abi")
    ops = importlib.import_module(PKG + ".ops")
    lib = abi.lib()
    B, H, W = shape
    pred, tgt = map(_dev, mc.inputs(shape))
    mask = _dev(mc.mask_of("random", shape)).view(torch.uint8)
    keep = (pred.clone(), tgt.clone(), mask.clone())
    stream = ops._stream_ptr(torch.device(DEV))
    CC = abi.GSPLAT_METRICS_COLOUR_CORRECT
    for flags in (0, CC):
        want = metrics.image_metrics(pred, tgt, mask, colour_correct=bool(flags))
        out, affine, scratch = _Guarded(16 * B), _Guarded(48 * B), _Guarded(lib.gsplat_metrics_scratch_bytes(B, H, W, flags))
        abi.check(lib.gsplat_metrics_forward(ops._p(pred), ops._p(tgt), ops._p(mask), B, H, W, flags, affine.ptr() if flags else None, out.ptr(),
                                             scratch.ptr(), stream), "gsplat_metrics_forward")
        torch.cuda.synchronize()
        for name, b in (("out", out), ("affine", affine), ("scratch", scratch)):
            assert b.margins_intact(), f"flags {flags} {shape}: bytes next to {name} were overwritten"
        got = out.floats().view(B, 4)
        for j, k in enumerate(KEYS):
            assert vt._same(got[:, j], getattr(want, k)), (flags, k)
        if flags:
            assert vt._same(affine.floats().view(B, 3, 4), want.affine)
        else:
            assert bool((affine.buf == PATTERN).all()), "the affine buffer was written without being asked for"
    affine, scratch = _Guarded(48 * B), _Guarded(lib.gsplat_metrics_scratch_bytes(B, H, W, CC))
    abi.check(lib.gsplat_metrics_fit_affine(ops._p(pred), ops._p(tgt), ops._p(mask), B, H, W, affine.ptr(), scratch.ptr(), stream),
              "gsplat_metrics_fit_affine")
    torch.cuda.synchronize()
    assert affine.margins_intact() and scratch.margins_intact()
    assert vt._same(affine.floats().view(B, 3, 4), want.affine)
    assert torch.equal(pred, keep[0]) and torch.equal(tgt, keep[1]) and torch.equal(mask, keep[2])


# ---- input forms ----------------------------------------------------------------------------------------------------------------------

def test_other_input_forms_give_the_result_of_their_contiguous_fp32_copy(metrics):
    shape = (2, 11, 45)
    pred, tgt = map(_dev, mc.inputs(shape))
    mask = _dev(mc.mask_of("random", shape))
    for cc in (False, True):
        want = metrics.image_metrics(pred, tgt, mask, colour_correct=cc)
        fields = KEYS + (("affine",) if cc else ())
        wide_p, wide_t = torch.zeros(2, 11, 90, 3, device=DEV), torch.zeros(2, 11, 45, 4, device=DEV)
        wide_p[:, :, ::2] = pred
        wide_t[..., :3] = tgt
        wide_m = torch.zeros(2, 45, 11, dtype=torch.bool, device=DEV)
        wide_m.copy_(mask.transpose(1, 2))
        forms = [(wide_p[:, :, ::2], wide_t[..., :3], wide_m.transpose(1, 2)),                 # strided views
                 (pred.double(), tgt.double(), mask.to(torch.uint8)),                            # float64 (exact fp32 values), uint8
                 (pred.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), tgt, mask)]         # a permuted layout
        for x, y, m in forms:
            got = metrics.image_metrics(x, y, m, colour_correct=cc)
            for k in fields:
                assert vt._same(getattr(got, k), getattr(want, k)), (k, cc)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------

def _eval_views():
    """The three views of the tiny scene: the first with a 4-channel image, the second with a 'mask'."""
    s, views = vt._scene()
    rng = np.random.default_rng(31)
    views = [dict(v) for v in views]
    alpha = rng.uniform(0, 1, views[0]["image"].shape[:2] + (1,)).astype(np.float32)
    views[0]["image"] = np.concatenate([views[0]["image"], alpha], -1)
    views[1]["mask"] = rng.uniform(size=views[1]["image"].shape[:2]) < 0.6
    return s, views


def _frames(gs, tr, views, bg):
    m = tr.model
    out = []
    with torch.no_grad():
        for v in views:
            kw = dict(background=bg) if bg is not None else {}
            out.append(gs.render_gaussians(m.pos, m.f_dc, m.f_rest, m.opacity_raw, m.scale_raw, m.q_raw, torch.tensor(v["c2w"], device=DEV),
                                           v["H"], v["W"], v["fx"], v["fy"], v["cx"], v["cy"], **kw))
    return out


def _trainer_state(tr):
    state = dict(vt._model_bits(tr))
    for k in vt.NAMES:
        p = getattr(tr.model, k)
        state["grad_" + k] = p.grad.clone() if p.grad is not None else torch.zeros(0, device=DEV)
        st = tr.optimizer._state(p)
        state["m_" + k], state["v_" + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        state["step_" + k] = torch.tensor([st["step"]], dtype=torch.int32)
    if tr.exposure is not None or tr.bilagrid is not None:
        state.update({"table_" + k: v for k, v in vt._table_bits(tr).items()})
    if tr.densify_stats is not None:
        state["densify_stats"] = tr.densify_stats.data.clone()
    if tr.visible is not None:
        state["visible"] = tr.visible.data.clone()
    return state


@pytest.mark.parametrize("mode", ["default", "background", "exposure"])
def test_trainer_evaluate(gs, metrics, mode):
    s, views = _eval_views()
    vt._warm(gs, s, views)
    bg = (0.2, 0.4, 0.6) if mode == "background" else None
    cfg = dict(background=bg) if bg else dict(exposure=True) if mode == "exposure" else dict(densify_rule="screen", densify_until_iter=100, sparse_adam=True)
    tr = vt._trainer(s, **cfg)
    train_views = vt._scene()[1]
    for it in (1, 2):
        tr.step(it, train_views)
    before = _trainer_state(tr)
    report = tr.evaluate(views)
    after = _trainer_state(tr)
    assert before.keys() == after.keys()
    for k in before:
        a, b = before[k], after[k]
        assert a.shape == b.shape and (vt._same(a, b) if a.dtype == torch.float32 else torch.equal(a, b)), k
    # the same numbers from image_metrics of the render_gaussians frames, bit for bit
    cc = mode == "exposure"
    rows = []
    for v, frame in zip(views, _frames(gs, tr, views, bg)):
        target = torch.tensor(v["image"], device=DEV)
        if target.shape[-1] == 4:
            target = gs.losses.composite_over(target[..., :3], target[..., 3], bg if bg is not None else (0.0, 0.0, 0.0))
        mask = torch.tensor(v["mask"], device=DEV) if "mask" in v else None
        got = metrics.image_metrics(frame, target, mask, colour_correct=cc)
        rows.append([float(getattr(got, k)) for k in KEYS])
    assert report["n_views"] == 3 and report["per_view"]["idx"] == [0, 2, 4]
    for j, k in enumerate(KEYS):
        assert report["per_view"][k] == [r[j] for r in rows], k
    for j, k in enumerate(("psnr", "ssim", "l1")):
        total = 0.0
        for r in rows:
            total += r[j]
        assert report[k] == total / 3
    assert all(np.isfinite(report[k]) for k in ("psnr", "ssim", "l1"))
    if cc:                                     # the default followed cfg.exposure; colour_correct=False overrides it
        plain = tr.evaluate(views, colour_correct=False)
        again = tr.evaluate(views, colour_correct=True)
        assert again == report and plain != report
        want = [float(metrics.image_metrics(f, torch.tensor(views[2]["image"], device=DEV)).psnr) for f in _frames(gs, tr, views[2:], bg)]
        assert plain["per_view"]["psnr"][2] == want[0]
        # (the identity is one of the transforms the fit chooses from, and clamping toward a target inside [0, 1] only helps)
        assert report["per_view"]["mse"][2] <= plain["per_view"]["mse"][2]
    with pytest.raises(ValueError, match="no 'image'"):
        tr.evaluate([{k: v for k, v in views[1].items() if k != "image"}])
