"""float64 oracle of the auxiliary loss on the depth / opacity maps and of a target over a background (helper, not a test).

    v = [Z finite and > 0],  n = number of pixels,  n_v = max(1, sum v)
    L_alpha = sum |A - M| / n,   L_depth = sum v |D - A Z| / n_v
    values = scale (L_alpha, L_depth, l_a L_alpha + l_d L_depth)
    g_D = scale up l_d v sign(D - A Z) / n_v,   g_A = scale up (l_a sign(A - M) / n - l_d v Z sign(D - A Z) / n_v),   sign(0) = 0

`aux_loss` is the closed form, `aux_loss_plain` the formula written plainly for autograd; `make_inputs` draws the inputs the CPU and
the GPU tests share: no residual is ambiguous in fp32.
"""
import numpy as np
import torch

# three workgroups of the kernels (1024 pixels each: 256 threads x 4 pixels) plus 5 pixels: several partial sums and a ragged tail
THREE_WORKGROUPS_PLUS_5 = (17, 181)
assert THREE_WORKGROUPS_PLUS_5[0] * THREE_WORKGROUPS_PLUS_5[1] == 3 * 1024 + 5
SHAPES = [(1, 1), (1, 63), (1, 65), (7, 37), (33, 64), (3, 7, 37), (2, 1, 65), THREE_WORKGROUPS_PLUS_5]


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def valid_depth(Z):
    return torch.isfinite(Z) & (Z > 0)


def aux_loss(D, A, Z=None, M=None, lambda_depth=1.0, lambda_alpha=1.0, scale=1.0, upstream=1.0):
    """-> dict(values [3], grad_depth, grad_alpha, res_alpha, res_depth, valid) in float64.  A term whose target is None is off
    (value 0, grad_depth None without Z)."""
    D, A, Z, M = _f64(D), _f64(A), _f64(Z), _f64(M)
    n = A.numel()
    la = ld = 0.0
    gA = torch.zeros_like(A)
    gD = res_a = res_d = v = None
    if M is not None:
        res_a = A - M
        la = float(res_a.abs().sum()) / n
        gA = gA + scale * upstream * lambda_alpha * torch.sign(res_a) / n
    if Z is not None:
        v = valid_depth(Z)
        Zc = torch.where(v, Z, torch.zeros_like(Z))
        n_v = max(1, int(v.sum()))
        res_d = torch.where(v, D - A * Zc, torch.zeros_like(A))
        ld = float(res_d.abs().sum()) / n_v
        gD = scale * upstream * lambda_depth * torch.sign(res_d) / n_v
        gA = gA - gD * Zc
    values = np.array([scale * la, scale * ld, scale * (lambda_alpha * la + lambda_depth * ld)])
    return dict(values=values, grad_depth=gD, grad_alpha=gA, res_alpha=res_a, res_depth=res_d, valid=v)


def aux_loss_plain(D, A, Z=None, M=None, lambda_depth=1.0, lambda_alpha=1.0, scale=1.0):
    """The total, written as the definition reads, differentiable by autograd (|x| has derivative 0 at 0 there too)."""
    total = A.sum() * 0.0
    if M is not None:
        total = total + lambda_alpha * (A - M).abs().mean()
    if Z is not None:
        v = valid_depth(Z)
        Zc = torch.where(v, Z, torch.zeros_like(Z))                 # (masked before it meets the graph: 0 * NaN is NaN)
        total = total + lambda_depth * ((D - A * Zc).abs() * v.to(A.dtype)).sum() / max(1, int(v.sum()))
    return scale * total


def composite_over(rgb, alpha, background):
    rgb, a = _f64(rgb), _f64(alpha).unsqueeze(-1)
    return rgb * a + (1 - a) * torch.tensor([float(x) for x in background], dtype=torch.float64)


def make_inputs(shape, seed):
    """fp32 (D, A, Z, M) of `shape`.  Residuals r with |r| in [1e-3, 1] and a random sign; A = M + r', D = A Z + r formed in float64
    and rounded to fp32.  About a seventh of the pixels are exact zeros of the kinds that exist in practice -- an empty pixel
    (A = D = 0) and A a bit-copy of M --, about a fifth of Z is invalid: 0, negative, NaN, Inf."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))

    def residual():
        mag = 10.0 ** (-3.0 * torch.rand(n, generator=g, dtype=torch.float64))
        return mag * (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1)

    M = (0.05 + 0.9 * torch.rand(n, generator=g, dtype=torch.float64)).float()
    Z = (0.5 + 9.5 * torch.rand(n, generator=g, dtype=torch.float64)).float()
    A = (M.double() + residual()).float()
    kind = torch.randint(0, 14, (n,), generator=g)               # 0: empty pixel, 1: A == M (a seventh between them)
    A = torch.where(kind == 1, M, A)
    A = torch.where(kind == 0, torch.zeros_like(A), A)
    D = (A.double() * Z.double() + residual()).float()
    D = torch.where(kind == 0, torch.zeros_like(D), D)
    bad = torch.randint(0, 20, (n,), generator=g)                # 0..3: the four kinds of "no data" (a fifth between them)
    for k, val in enumerate((0.0, -1.5, float("nan"), float("inf"))):
        Z = torch.where(bad == k, torch.full_like(Z, val), Z)
    return tuple(t.reshape(shape).clone() for t in (D, A, Z, M))


def assert_unambiguous(ref):
    """Every residual of the oracle is exactly 0 or outside +-1e-4: no sign depends on fp32 rounding, so NO pixel is left out of a
    gradient comparison."""
    for key in ("res_alpha", "res_depth"):
        r = ref[key]
        if r is not None:
            assert bool(((r == 0) | (r.abs() > 1e-4)).all()), key
