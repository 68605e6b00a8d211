"""The float64 oracle of the image metrics (tests/metrics_oracle.py) against independent restatements: a torch conv2d SSIM map, the
reference's own loss values (tests/golden/loss.npz), and the properties the definitions promise."""
import numpy as np
import pytest
import torch

from tests import metrics_oracle as mo
from tests import util


def _images(shape, seed):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(0, 1, shape + (3,))
    return np.clip(tgt + 0.15 * rng.standard_normal(shape + (3,)), 0, 1), tgt


def _torch_ssim_map(x, y):
    """[H, W, 3] float64 -> [H, W, 3]: the SSIM map with a grouped 11 x 11 conv2d and zero padding."""
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    w = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()

    def f(a):
        return torch.nn.functional.conv2d(a.permute(2, 0, 1)[None], w, padding=5, groups=3)[0].permute(1, 2, 0)

    x, y = torch.tensor(x), torch.tensor(y)
    mu1, mu2 = f(x), f(y)
    s11, s22, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    return (((2 * mu1 * mu2 + mo.C1) * (2 * s12 + mo.C2)) / ((mu1 * mu1 + mu2 * mu2 + mo.C1) * (s11 + s22 + mo.C2))).numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (2, 17, 33)])
def test_ssim_map_matches_a_conv2d_restatement(shape):
    pred, tgt = _images(shape, 11)
    for b in range(shape[0]):
        got, want = mo.ssim_map(pred[b], tgt[b]), _torch_ssim_map(pred[b], tgt[b])
        assert got.shape == want.shape == shape[1:] + (3,)
        assert np.abs(got - want).max() < 1e-12          # two float64 evaluations of one formula, sums in different orders


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_l1_and_ssim_match_the_reference_loss_values(tag):
    """vals_* of tests/golden/loss.npz are the reference's own compute_loss outputs (l1, 1 - ssim, total) in fp32; the bounds are
    those of tests/test_gpu_loss.py::test_compute_loss_vs_reference_golden."""
    d = dict(np.load(util.GOLDEN + "/loss.npz"))
    pred, tgt, ref = d["pred_" + tag], d["target_" + tag], d["vals_" + tag]
    if pred.ndim == 3:
        got = mo.one_image(pred, tgt)
        l1, ssim = got["l1"], got["ssim"]
    else:                                                 # the loss is a batch mean: equal sizes, so the mean of the per-image values
        got = mo.image_metrics(pred, tgt)
        l1, ssim = got["l1"].mean(), got["ssim"].mean()
    assert abs(l1 - ref[0]) <= 2e-6 * abs(ref[0]) + 1e-7
    assert abs((1 - ssim) - ref[1]) <= 1e-5 * abs(ref[1]) + 1e-6


def test_an_image_against_itself_is_exact():
    pred, _ = _images((2, 9, 13), 3)
    got = mo.image_metrics(pred, pred.copy())             # (without correction: a fitted transform is the identity only up to rounding)
    assert np.all(np.isposinf(got["psnr"])) and np.all(got["l1"] == 0.0) and np.all(got["mse"] == 0.0)
    assert np.all(got["ssim"] == 1.0)


def test_a_planted_affine_is_recovered_within_the_ridge_bias():
    """target = M0 pred + t0 exactly (no clamp): P - P0 = (A + l n D)^-1 l n ([I3; 0] - D P0), so
    |P - P0|_F <= l n |(A + l n D)^-1|_2 |[I3; 0] - D P0|_F -- derived from lambda, plus float64 rounding of the solve."""
    rng = np.random.default_rng(5)
    pred = rng.uniform(0, 1, (24, 31, 3))
    M0 = np.array([[0.8, 0.1, -0.05], [0.02, 0.7, 0.1], [-0.04, 0.06, 0.9]])
    t0 = np.array([0.05, 0.08, 0.05])          # (the target stays inside [0, 1]: the clamp does nothing)
    tgt = pred @ M0.T + t0
    valid = rng.uniform(size=(24, 31)) < 0.7
    for v in (None, valid):
        vv = np.ones((24, 31), dtype=bool) if v is None else v
        A, _, n = mo.normal_equations(pred, tgt, vv)
        P0 = np.concatenate([M0.T, t0[None]], 0)
        D = np.diag([1.0, 1.0, 1.0, 0.0])
        bias = mo.RIDGE * n * np.linalg.norm(np.linalg.inv(A), 2) * np.linalg.norm(np.eye(4, 3) - D @ P0)
        cond = np.linalg.cond(A)
        assert cond < 1e3, cond                            # uniform random colours: well conditioned
        got = mo.fit_affine(pred, tgt, v)
        err = np.linalg.norm(got.T - P0)
        assert err <= bias + 1e-13 * cond, (err, bias)
        assert bias < 1e-6
        m = mo.one_image(pred, tgt, v, colour_correct=True)
        assert m["mse"] < 1e-12 and m["ssim"] > 1 - 1e-9


def test_an_all_invalid_mask_gives_nan_for_that_image_only():
    pred, tgt = _images((3, 8, 9), 7)
    mask = np.random.default_rng(1).uniform(size=(3, 8, 9)) < 0.6
    mask[1] = False
    for cc in (False, True):
        got = mo.image_metrics(pred, tgt, mask, cc)
        alone = [mo.one_image(pred[b], tgt[b], mask[b], cc) for b in range(3)]
        for k in ("psnr", "ssim", "l1", "mse"):
            assert np.isnan(got[k][1]) and np.isfinite(got[k][[0, 2]]).all()
            assert got[k][0] == alone[0][k] and got[k][2] == alone[2][k]
        if cc:
            assert np.isnan(got["affine"][1]).all() and np.isfinite(got["affine"][[0, 2]]).all()


def test_the_mask_changes_the_mean_not_the_map():
    pred, tgt = _images((1, 12, 14), 9)
    mask = np.random.default_rng(2).uniform(size=(12, 14)) < 0.5
    full, part = mo.one_image(pred[0], tgt[0]), mo.one_image(pred[0], tgt[0], mask)
    assert np.array_equal(full["map"], part["map"])
    assert part["ssim"] == full["map"][mask].sum() / (3 * mask.sum())
    assert part["ssim"] != full["ssim"]
    d = (pred[0] - tgt[0])[mask]
    assert part["l1"] == np.abs(d).sum() / (3 * mask.sum()) and part["mse"] == (d * d).sum() / (3 * mask.sum())
