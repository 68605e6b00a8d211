"""The inputs of the image-metric tests (tests/test_gpu_metrics.py) and the CPU calibration of their bounds.

    python -m tests.metrics_cases        prints the calibration: the fp32-vs-float64 error of a float32 torch restatement of the
                                         uncorrected metrics over the sweep (the device gets 4 x the largest), and the range of the
                                         oracle's sensitivity to +-1 fp32 ulp of its inputs with the correction (the device gets 8 x
                                         each case's own, plus the uncorrected bound), with the condition numbers of the sweep.
Nothing here needs a GPU."""
import functools

import numpy as np
import torch

from tests import metrics_oracle as mo

SHAPES = [(1, 1, 1), (1, 4, 3), (1, 16, 32), (1, 17, 33), (2, 11, 45), (3, 40, 70)]
MASKS = ("none", "random", "one_invalid")
ULP_DRAWS = 8


def inputs(shape, seed=0):
    """(pred, target) fp32 [B, H, W, 3]: uniform random colours (the normal equations of the fit are well conditioned), the target a
    mild colour transform of them plus noise, clamped -- so that the corrected metrics differ from the plain ones."""
    rng = np.random.default_rng(1000 * seed + 97 * shape[0] + 13 * shape[1] + shape[2])
    pred = rng.uniform(0, 1, shape + (3,))
    M = np.array([[0.85, 0.05, 0.0], [0.02, 0.8, 0.04], [0.0, 0.06, 0.9]])
    tgt = np.clip(pred @ M.T + np.array([0.05, 0.03, 0.02]) + 0.08 * rng.standard_normal(shape + (3,)), 0, 1)
    return pred.astype(np.float32), tgt.astype(np.float32)


def mask_of(kind, shape, seed=0):
    """None | a seeded random mask (70 % valid; an image the draw left without a valid pixel gets its first one back, so that the
    one-pixel image is measured through a mask too) | the same with the LAST image of the batch fully invalid; bool [B, H, W]."""
    if kind == "none":
        return None
    m = np.random.default_rng(7000 + 1000 * seed + 31 * shape[1] + shape[2]).uniform(size=shape) < 0.7
    for b in range(shape[0]):
        if not m[b].any():
            m[b, 0, 0] = True
    if kind == "one_invalid":
        m[-1] = False
    return m


@functools.lru_cache(maxsize=None)
def reference(shape, kind, colour_correct, seed=0):
    """The float64 oracle of a case, computed once and shared (treat as read-only)."""
    pred, tgt = inputs(shape, seed)
    return mo.image_metrics(pred, tgt, mask_of(kind, shape, seed), colour_correct)


@functools.lru_cache(maxsize=None)
def ulp_sensitivity(shape, kind, seed=0):
    """ulp_sensitivity_of() of a case of the sweep, computed once and shared."""
    pred, tgt = inputs(shape, seed)
    return ulp_sensitivity_of(pred, tgt, mask_of(kind, shape, seed), reference(shape, kind, True, seed), seed)


def ulp_sensitivity_of(pred, tgt, mask, base, seed=0):
    """The oracle's own sensitivity with the correction, for inputs [B, H, W, 3] whose oracle is `base`: the largest change of each
    output (per image) when every input is moved by a random +-1 fp32 ulp -- seeded, ULP_DRAWS draws.
    {'psnr', 'ssim', 'l1', 'mse': [B], 'affine': [B]} (NaN images: 0)."""
    shape = pred.shape[:3]
    rng = np.random.default_rng(424242 + seed)
    worst = {k: np.zeros(shape[0]) for k in ("psnr", "ssim", "l1", "mse", "affine")}
    for _ in range(ULP_DRAWS):
        moved = []
        for a in (pred, tgt):
            up = rng.integers(0, 2, a.shape).astype(bool)
            moved.append(np.where(up, np.nextafter(a, np.float32(2)), np.nextafter(a, np.float32(-1))).astype(np.float32))
        got = mo.image_metrics(moved[0], moved[1], mask, True)
        for k in ("psnr", "ssim", "l1", "mse"):
            with np.errstate(invalid="ignore"):
                worst[k] = np.maximum(worst[k], np.nan_to_num(np.abs(got[k] - base[k]), nan=0.0, posinf=0.0))
        worst["affine"] = np.maximum(worst["affine"], np.nan_to_num(np.abs(got["affine"] - base["affine"]).reshape(shape[0], -1).max(1), nan=0.0))
    return worst


def condition_numbers(shape, kind, seed=0):
    """(number of valid pixels, cond(A + ridge)) of every image of a case that has a valid pixel."""
    pred, tgt = inputs(shape, seed)
    mask = mask_of(kind, shape, seed)
    out = []
    for b in range(shape[0]):
        valid = np.ones(shape[1:], dtype=bool) if mask is None else mask[b]
        if valid.any():
            out.append((int(valid.sum()), np.linalg.cond(mo.normal_equations(pred[b].astype(np.float64), tgt[b].astype(np.float64), valid)[0])))
    return out


def fp32_restatement(pred, tgt, mask):
    """The uncorrected metrics of one image in float32 torch ops on the CPU: (psnr, ssim, l1, mse) as float32 numbers."""
    x, y = torch.tensor(pred), torch.tensor(tgt)
    g = torch.exp(-((torch.arange(11, dtype=torch.float32) - 5) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    w = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()

    def f(a):
        return torch.nn.functional.conv2d(a.permute(2, 0, 1)[None], w, padding=5, groups=3)[0].permute(1, 2, 0)

    mu1, mu2 = f(x), f(y)
    s11, s22, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + mo.C1) * (2 * s12 + mo.C2)) / ((mu1 * mu1 + mu2 * mu2 + mo.C1) * (s11 + s22 + mo.C2))
    valid = torch.ones(x.shape[:2], dtype=torch.bool) if mask is None else torch.tensor(mask)
    n3 = torch.tensor(3.0 * float(valid.sum()), dtype=torch.float32)
    d = (x - y)[valid]
    mse = (d * d).sum() / n3
    return float(-10 * torch.log10(mse)), float(smap[valid].sum() / n3), float(d.abs().sum() / n3), float(mse)


def calibrate():
    worst = dict(psnr_abs=0.0, mse_rel=0.0, ssim_abs=0.0, l1_rel=0.0)
    for shape in SHAPES:
        for kind in ("none", "random"):
            pred, tgt = inputs(shape)
            mask = mask_of(kind, shape)
            ref = reference(shape, kind, False)
            for b in range(shape[0]):
                if mask is not None and not mask[b].any():
                    continue
                p, s, l, m = fp32_restatement(pred[b], tgt[b], None if mask is None else mask[b])
                worst["psnr_abs"] = max(worst["psnr_abs"], abs(p - ref["psnr"][b]))
                worst["mse_rel"] = max(worst["mse_rel"], abs(m - ref["mse"][b]) / ref["mse"][b])
                worst["ssim_abs"] = max(worst["ssim_abs"], abs(s - ref["ssim"][b]))
                worst["l1_rel"] = max(worst["l1_rel"], abs(l - ref["l1"][b]) / ref["l1"][b])
    print("fp32 torch restatement vs float64 over the sweep (largest):", {k: f"{v:.3e}" for k, v in worst.items()})
    for shape in SHAPES:
        for kind in MASKS:
            s = ulp_sensitivity(shape, kind)
            conds = condition_numbers(shape, kind)
            print(f"{shape} {kind:11s} +-1 ulp sensitivity:", " ".join(f"{k} {s[k].max():.2e}" for k in ("psnr", "ssim", "l1", "mse", "affine")),
                  " (valid pixels, cond)", " ".join(f"({n}, {c:.1e})" for n, c in conds))


if __name__ == "__main__":
    calibrate()
