"""Next-row parity: fused L1 + SSIM loss kernel against goldens from the reference's compute_loss."""
import importlib
import time

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"


@pytest.fixture(scope="module")
def losses():
    return importlib.import_module(PKG + ".losses")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_compute_loss_vs_reference_golden(losses, tag):
    d = dict(np.load(util.GOLDEN + "/loss.npz"))
    t = torch.tensor(d["target_" + tag], device=DEV)
    for lam, vals_key, grad_key in (((0.8, 0.2), "vals_", "grad_"), ((0.3, 1.7), None, "grad2_")):
        p = torch.tensor(d["pred_" + tag], device=DEV, requires_grad=True)
        total, parts = losses.compute_loss(p, t, *lam)
        total.backward()
        if vals_key:
            ref = d[vals_key + tag]
            assert abs(parts["l1"] - ref[0]) <= 2e-6 * abs(ref[0]) + 1e-7
            assert abs(parts["ssim"] - ref[1]) <= 1e-5 * abs(ref[1]) + 1e-6
            assert abs(float(total) - ref[2]) <= 1e-5 * abs(ref[2]) + 1e-6
        else:
            assert abs(float(total) - float(d["total2_" + tag])) <= 1e-5 * abs(float(d["total2_" + tag])) + 1e-6
        util.check_grad(p.grad.cpu().numpy(), d[grad_key + tag], "pred", l2=2e-5, mx=5e-5)


def test_l1_and_ssim_alone(losses):
    d = dict(np.load(util.GOLDEN + "/loss.npz"))
    p = torch.tensor(d["pred_a"], device=DEV)
    t = torch.tensor(d["target_a"], device=DEV)
    ref = d["vals_a"]
    assert abs(float(losses.l1_loss(p, t)) - ref[0]) < 1e-6
    assert abs(float(losses.ssim_loss(p, t)) - ref[1]) < 2e-6
    with pytest.raises(NotImplementedError):
        losses.ssim_loss(p, t, window_size=7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.compute_loss(p.cpu(), t.cpu())


def test_loss_1080p_vs_oracle_and_timing(losses):
    """Full 1080p frame: value and gradient against the float64 oracle on the CPU; prints the fused kernel's time next
    to the same loss written with PyTorch-ROCm ops (15 conv2d + autograd), for information."""
    g = torch.Generator().manual_seed(3)
    tgt = torch.rand(1080, 1920, 3, generator=g)
    pred = (tgt + 0.1 * torch.randn(1080, 1920, 3, generator=g)).clamp(0, 1)
    p64 = pred.double().requires_grad_(True)
    ref, _, _ = tp.compute_loss(p64, tgt.double())
    ref.backward()
    p = pred.to(DEV).requires_grad_(True)
    t = tgt.to(DEV)
    total, parts = losses.compute_loss(p, t)
    total.backward()
    assert abs(float(total) - float(ref)) < 1e-5 * float(ref)
    util.check_grad(p.grad.cpu().numpy(), p64.grad.numpy(), "pred", l2=5e-5, mx=2e-4)

    def bench(fn, n=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def fused():
        q = pred.to(DEV).requires_grad_(True) if False else p
        q.grad = None
        losses._LossFn.apply(q, t, 0.8, 0.2)[0].backward()

    def torch_ops():
        p.grad = None
        tp.compute_loss(p, t)[0].backward()

    print(f"loss fwd+bwd @1080p: fused HIP {bench(fused):.3f} ms, PyTorch-ROCm ops {bench(torch_ops):.3f} ms")


# ---------------------------------------------------------------------------------------------------------------------------------
# Edges of the two loss kernels: tile geometry (32 x 16 tiles, 5-pixel halo), the entry points, scale / upstream, and the
# regime training converges to (smooth, flat, nearly equal images: sigma^2 = E[x^2] - mu^2 cancels).
# Bounds: those of test_compute_loss_vs_reference_golden, against float64 -- the reference's own fp32 run stays below 5e-7 on the
# values and 1e-6 on the gradient at the sweep's shapes; where it does not (tests/golden/loss_edges.npz) its measured fp32-vs-fp64
# error is the calibration (tests/util.py: K_CAL).
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = [(1, 1), (1, 40), (33, 1), (5, 5), (10, 10), (11, 11), (12, 12), (15, 31), (16, 32), (17, 33), (32, 64), (48, 96),
                (6, 43), (27, 5), (16, 33), (17, 32), (3, 17, 33), (2, 16, 32)]
SWEEP_LAMBDAS = [(0.8, 0.2), (1.0, 0.0), (0.0, 1.0)]
GUARD = 4096            # bytes of margin on each side of a guarded buffer
PATTERN = 0xA5


def _inputs(shape, seed):
    """The recipe of tests/golden/loss.npz: uniform target, noisy clamped prediction, a few pixels bit-equal (sign(0) = 0);
    a different image in every slot of a batch."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand(*shape, 3, generator=g)
    pred = (tgt + 0.15 * torch.randn(*shape, 3, generator=g)).clamp(0, 1)
    flat_p, flat_t = pred.view(-1, 3), tgt.view(-1, 3)
    idx = torch.randperm(flat_p.shape[0], generator=g)[:flat_p.shape[0] // 7]
    flat_p[idx] = flat_t[idx]
    return pred, tgt


def _oracle(pred, tgt, lam):
    """float64 on the CPU: ((l1, 1 - ssim, total), gradient)."""
    p = pred.detach().cpu().double().requires_grad_(True)
    total, l1, sl = tp.compute_loss(p, tgt.detach().cpu().double(), *lam)
    total.backward()
    return np.array([float(l1), float(sl), float(total)]), p.grad.numpy()


def _value_bounds(ref):
    return np.array([2e-6 * abs(ref[0]) + 1e-7, 1e-5 * abs(ref[1]) + 1e-6, 1e-5 * abs(ref[2]) + 1e-6])


def _check_values(got, ref, what, cal=None):
    """(l1, 1 - ssim, total) against float64; cal = the reference's fp32 values: a bound may grow to K_CAL x their error."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, bound = np.abs(got - ref), _value_bounds(ref)
    cerr = np.abs(np.asarray(cal, dtype=np.float64) - ref) if cal is not None else np.full(3, np.nan)
    if cal is not None:
        bound = np.maximum(bound, util.K_CAL * cerr)
    print(f"values {what}: |err| l1 {err[0]:.2e} ssim {err[1]:.2e} total {err[2]:.2e} (allowed {bound[0]:.2e} {bound[1]:.2e} {bound[2]:.2e}; "
          f"fp32 reference {cerr[0]:.2e} {cerr[1]:.2e} {cerr[2]:.2e}; float64 values {ref[0]:.4e} {ref[1]:.4e} {ref[2]:.4e})")
    assert np.isfinite(got).all(), (what, got)
    for k, name in enumerate(("l1", "ssim", "total")):
        assert err[k] <= bound[k], f"{what}: {name} {got[k]!r} vs {ref[k]!r}: |err| {err[k]:.3e} > {bound[k]:.3e}"


def _hip(losses, pred, tgt, lam):
    p = pred.to(DEV).requires_grad_(True)
    total, parts = losses.compute_loss(p, tgt.to(DEV), *lam)
    total.backward()
    assert abs(float(total) - parts["total"]) == 0.0
    return np.array([parts["l1"], parts["ssim"], parts["total"]]), p.grad.cpu().numpy()


@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shape_sweep_vs_float64_oracle(losses, shape):
    """Dimensions of 1, around the 11-pixel window, exact tile multiples, tile multiples plus one (both ways round) and batches,
    three weightings each."""
    pred, tgt = _inputs(shape, seed=1000 + 7 * shape[-2] + shape[-1] + 31 * len(shape))
    for lam in SWEEP_LAMBDAS:
        ref_v, ref_g = _oracle(pred, tgt, lam)
        v, g = _hip(losses, pred, tgt, lam)
        _check_values(v, ref_v, f"{shape} {lam}")
        util.check_grad(g, ref_g, f"pred {shape} {lam}", l2=2e-5, mx=5e-5)
        if len(shape) == 3:          # every slot of a batch: 1 / B times the gradient of that image on its own
            B = shape[0]
            for b in range(B):
                ref_vb, ref_gb = _oracle(pred[b], tgt[b], lam)
                _, gb = _hip(losses, pred[b], tgt[b], lam)
                util.check_grad(B * g[b], ref_gb, f"pred {shape} {lam} slot {b} vs float64 alone", l2=2e-5, mx=5e-5)
                util.check_grad(B * g[b], gb, f"pred {shape} {lam} slot {b} vs HIP alone", l2=2e-5, mx=5e-5)


class _Guarded:
    """`nbytes` usable bytes in the middle of an allocation whose margins (GUARD bytes each side) hold a bit pattern."""

    def __init__(self, nbytes, fill=None):
        self.nbytes = int(nbytes)
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0 and self.nbytes % 4 == 0
        if fill is not None:
            self.floats().fill_(fill)

    def ptr(self):
        import ctypes as C
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def floats(self):
        return self.buf[GUARD:GUARD + self.nbytes].view(torch.float32)

    def margins_intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.nbytes:] == PATTERN).all())


@pytest.mark.parametrize("shape", [(1, 1), (17, 33), (33, 1), (3, 17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_nothing_is_written_outside_grad_values_and_scratch(shape):
    """gsplat_loss_forward + gsplat_loss_backward, gsplat_loss with and without a gradient, called on buffers of exactly the stated
    sizes (scratch: gsplat_loss_scratch_bytes) that sit between margins holding a bit pattern: the margins come back unchanged, every
    element of the gradient and of the values was written, the inputs are untouched.  Read-back only."""
    abi = importlib.import_module(PKG + "._abi")
    ops = importlib.import_module(PKG + ".ops")
    lib = abi.lib()
    B = shape[0] if len(shape) == 3 else 1
    H, W = shape[-2], shape[-1]
    pred, tgt = _inputs(shape, seed=77)
    n = pred.numel()
    stream = ops._stream_ptr(torch.device(DEV))
    ref_v, ref_g = _oracle(pred, tgt, (0.8, 0.2))

    def fresh(with_grad):
        x, y = _Guarded(4 * n), _Guarded(4 * n)
        x.floats().copy_(pred.reshape(-1))
        y.floats().copy_(tgt.reshape(-1))
        return (x, y, _Guarded(12, float("nan")), _Guarded(4, float("nan")), _Guarded(4 * n, float("nan")),
                _Guarded(lib.gsplat_loss_scratch_bytes(B, H, W, with_grad)))

    def verify(bufs, what, grad_written, total_written):
        torch.cuda.synchronize()
        x, y, values, total, grad, scratch = bufs
        for name, b in zip(("pred", "target", "values", "total", "grad_pred", "scratch"), bufs):
            assert b.margins_intact(), f"{what} {shape}: bytes next to {name} were overwritten"
        assert torch.equal(x.floats().cpu(), pred.reshape(-1)) and torch.equal(y.floats().cpu(), tgt.reshape(-1)), f"{what}: inputs changed"
        v = values.floats().cpu().numpy()
        _check_values(v, ref_v, f"{what} {shape}")
        if total_written:
            assert float(total.floats()[0]) == float(v[2])
        g = grad.floats().cpu().numpy()
        if grad_written:
            assert np.isfinite(g).all(), f"{what} {shape}: {int((~np.isfinite(g)).sum())} gradient elements never written"
            util.check_grad(g.reshape(ref_g.shape), ref_g, f"pred {what} {shape}", l2=2e-5, mx=5e-5)
        else:
            assert np.isnan(g).all(), f"{what} {shape}: the gradient buffer was written without being asked for"

    up = torch.ones(1, device=DEV)
    # the two halves the autograd node calls
    bufs = fresh(1)
    x, y, values, total, grad, scratch = bufs
    abi.check(lib.gsplat_loss_forward(x.ptr(), y.ptr(), B, H, W, 0.8, 0.2, 1.0, values.ptr(), total.ptr(), scratch.ptr(), 1, stream), "forward")
    verify(bufs, "gsplat_loss_forward", grad_written=False, total_written=True)
    abi.check(lib.gsplat_loss_backward(x.ptr(), y.ptr(), B, H, W, 0.8, 0.2, 1.0, ops._p(up), grad.ptr(), scratch.ptr(), stream), "backward")
    verify(bufs, "gsplat_loss_backward", grad_written=True, total_written=True)
    # value only: a scratch without room for the maps
    bufs = fresh(0)
    x, y, values, total, grad, scratch = bufs
    abi.check(lib.gsplat_loss_forward(x.ptr(), y.ptr(), B, H, W, 0.8, 0.2, 1.0, values.ptr(), total.ptr(), scratch.ptr(), 0, stream), "forward")
    verify(bufs, "gsplat_loss_forward (no maps)", grad_written=False, total_written=True)
    # the one-call form
    bufs = fresh(1)
    x, y, values, total, grad, scratch = bufs
    abi.check(lib.gsplat_loss(x.ptr(), y.ptr(), B, H, W, 0.8, 0.2, values.ptr(), grad.ptr(), scratch.ptr(), stream), "gsplat_loss")
    verify(bufs, "gsplat_loss", grad_written=True, total_written=False)
    bufs = fresh(0)
    x, y, values, total, grad, scratch = bufs
    abi.check(lib.gsplat_loss(x.ptr(), y.ptr(), B, H, W, 0.8, 0.2, values.ptr(), None, scratch.ptr(), stream), "gsplat_loss")
    verify(bufs, "gsplat_loss (value only)", grad_written=False, total_written=False)


@pytest.mark.parametrize("shape", [(17, 33), (3, 17, 33), (45, 70), (1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_one_call_entry_equals_the_two_call_path_bitwise(losses, shape):
    """gsplat_loss (the form INTEGRATION.md names; the only path on which loss_grad_kernel adds up the sums itself) against
    gsplat_loss_forward + gsplat_loss_backward as the autograd node calls them: the same kernels on the same partial sums in the same
    fixed order, scale = upstream = 1 multiplied in exactly -- values and gradient bit for bit.  With grad_pred = NULL and a scratch
    without maps: the same values."""
    abi = importlib.import_module(PKG + "._abi")
    ops = importlib.import_module(PKG + ".ops")
    lib = abi.lib()
    B = shape[0] if len(shape) == 3 else 1
    H, W = shape[-2], shape[-1]
    pred, tgt = _inputs(shape, seed=5)
    stream = ops._stream_ptr(torch.device(DEV))
    for lam in SWEEP_LAMBDAS:
        p = pred.to(DEV).requires_grad_(True)
        t = tgt.to(DEV)
        total, v2 = losses.compute_loss_device(p, t, *lam)
        total.backward()
        values = torch.full((3,), float("nan"), device=DEV)
        grad = torch.full_like(p, float("nan"))
        scratch = torch.empty(lib.gsplat_loss_scratch_bytes(B, H, W, 1), dtype=torch.uint8, device=DEV)
        abi.check(lib.gsplat_loss(ops._p(p.detach()), ops._p(t), B, H, W, lam[0], lam[1], ops._p(values), ops._p(grad), ops._p(scratch), stream),
                  "gsplat_loss")
        assert torch.equal(values, v2), (shape, lam, values.tolist(), v2.tolist())
        assert float(total) == float(values[2])
        assert torch.equal(grad, p.grad), (shape, lam, float((grad - p.grad).abs().max()))
        values0 = torch.full((3,), float("nan"), device=DEV)
        scratch0 = torch.empty(lib.gsplat_loss_scratch_bytes(B, H, W, 0), dtype=torch.uint8, device=DEV)
        abi.check(lib.gsplat_loss(ops._p(p.detach()), ops._p(t), B, H, W, lam[0], lam[1], ops._p(values0), None, ops._p(scratch0), stream),
                  "gsplat_loss")
        assert torch.equal(values0, v2), (shape, lam, values0.tolist(), v2.tolist())


def test_scale_and_upstream_reach_values_and_gradient(losses):
    """compute_loss_device(scale = 0.25) and an upstream gradient of 3: values = 0.25 x, gradient = 0.75 x the float64 oracle's
    (the kernels multiply both in; only whole-trainer tests came this way before)."""
    shape = (3, 17, 33)
    pred, tgt = _inputs(shape, seed=11)
    ref_v, ref_g = _oracle(pred, tgt, (0.8, 0.2))
    p = pred.to(DEV).requires_grad_(True)
    total, v = losses.compute_loss_device(p, tgt.to(DEV), 0.8, 0.2, scale=0.25)
    (total * 3.0).backward()
    assert float(total) == float(v[2])
    _check_values(v.cpu().numpy().astype(np.float64) / 0.25, ref_v, "scale 0.25 (divided out)")
    util.check_grad(p.grad.cpu().numpy(), 0.75 * ref_g, "pred, scale 0.25 x upstream 3", l2=2e-5, mx=5e-5)
    # and the bound is about the factor, not only about the shape of the gradient
    assert abs(np.linalg.norm(p.grad.cpu().numpy().astype(np.float64)) / np.linalg.norm(ref_g) - 0.75) <= 0.75 * 2e-5


def _edge_cases():
    d = dict(np.load(util.GOLDEN + "/loss_edges.npz"))
    return [(str(tag), sfx) for tag in d["cases"] for sfx in ("", "__ssim") if not sfx or tag in d["ssim_only_cases"]]


@pytest.mark.parametrize("tag,sfx", _edge_cases(), ids=lambda v: v or "l1_ssim")
def test_hard_numerics_vs_reference_float64_calibrated(losses, tag, sfx):
    """tests/golden/loss_edges.npz: images as they are near convergence.  There B2 = sigma1^2 + sigma2^2 + C2 approaches C2 = 9e-4 with
    sigma^2 = E[x^2] - mu^2 the difference of two numbers near 1, and the reference's OWN fp32 run errs up to 4 orders of magnitude
    more than on noise images.  Bounds: those of test_compute_loss_vs_reference_golden, exceeded only next to that measured error, by
    at most K_CAL times.  Measured on the MI355X, |error| of 1 - ssim HIP | reference fp32: smooth 1.0e-7 | 2.3e-7, flat_bright
    6.8e-8 | 2.2e-4, flat_dark 1.9e-8 | 1.1e-7, saturated 5.0e-8 | 1.9e-6, batch3 8.5e-8 | 6.5e-5; gradient rel-L2 3.2e-5 | 7.3e-5,
    2.8e-5 | 2.2e-4, 9.0e-8 | 1.5e-6, 7.6e-6 | 2.0e-5, 1.7e-5 | 1.2e-4; equal images: gradient exactly 0 (DESIGN.md section 9, row 1,
    has the whole table, and what the kernel computed before it formed the variance of x - y directly: saturated 6.0e-6, beyond K_CAL)."""
    d = dict(np.load(util.GOLDEN + "/loss_edges.npz"))
    lam = (0.0, 1.0) if sfx else (0.8, 0.2)
    pred, tgt = torch.tensor(d["pred_" + tag]), torch.tensor(d["target_" + tag])
    ref_v, ref_g = d[f"vals_{tag}{sfx}"], d[f"grad_{tag}{sfx}"]
    cal_v, cal_g = d[f"vals32_{tag}{sfx}"], d[f"grad32_{tag}{sfx}"]
    v, g = _hip(losses, pred, tgt, lam)
    _check_values(v, ref_v, f"{tag}{sfx}", cal=cal_v)
    if tag.startswith("equal_"):
        # the float64 gradient is zero to 1e-17 (every term cancels): an absolute bound on the scale 1 / n of an unequal image's gradient
        n = pred.numel()
        bound = max(5e-5 / n, util.K_CAL * float(np.abs(cal_g).max()))
        print(f"grad {tag}: max|g| {np.abs(g).max():.2e} (allowed {bound:.2e}, fp32 reference {np.abs(cal_g).max():.2e}, float64 {np.abs(ref_g).max():.2e})")
        assert np.isfinite(g).all()
        assert np.abs(g).max() <= bound, f"{tag}: max|g| {np.abs(g).max():.3e} > {bound:.3e}"
        assert abs(v[2]) <= 1e-6, v
    else:
        util.check_grad(g, ref_g, f"pred {tag}{sfx}", cal=cal_g, l2=2e-5, mx=5e-5)


def test_same_inputs_give_the_same_bits_and_other_input_forms_their_contiguous_copy(losses):
    """The sums are added in a fixed order (no atomics): two calls agree bit for bit.  A float64 prediction gets a float64 total and
    gradient; a prediction that is a strided view, or whose storage starts 4 bytes off a 16-byte boundary, gives the bits of its
    contiguous, aligned copy."""
    shape = (2, 37, 70)
    pred, tgt = _inputs(shape, seed=21)
    t = tgt.to(DEV)

    def run(p):
        total, v = losses.compute_loss_device(p, t, 0.8, 0.2)
        total.backward()
        return total.detach().clone(), v.clone(), p.grad.clone()

    base = run(pred.to(DEV).requires_grad_(True))
    again = run(pred.to(DEV).requires_grad_(True))
    for a, b in zip(base, again):
        assert torch.equal(a, b)
    # float64 in, float64 out
    p64 = pred.double().to(DEV).requires_grad_(True)
    total64, parts = losses.compute_loss(p64, t.double(), 0.8, 0.2)
    total64.backward()
    assert total64.dtype == torch.float64 and p64.grad.dtype == torch.float64
    ref_v, ref_g = _oracle(pred, tgt, (0.8, 0.2))
    _check_values([parts["l1"], parts["ssim"], float(total64)], ref_v, "float64 prediction")
    util.check_grad(p64.grad.cpu().numpy(), ref_g, "pred (float64)", l2=2e-5, mx=5e-5)
    # a strided view of a larger tensor
    wide = torch.rand(2, 37, 70 + 9, 3, device=DEV)
    wide[:, :, 4:74] = pred.to(DEV)
    view = wide[:, :, 4:74].detach().requires_grad_(True)
    assert not view.is_contiguous()
    for a, b in zip(base, run(view)):
        assert torch.equal(a, b)
    # storage that starts one float off a 16-byte boundary
    buf = torch.empty(pred.numel() + 1, device=DEV)
    off = buf[1:].view(pred.shape)
    off.copy_(pred.to(DEV))
    off = off.detach().requires_grad_(True)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    for a, b in zip(base, run(off)):
        assert torch.equal(a, b)
