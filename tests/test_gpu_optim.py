"""Next-row parity: fused Adam + clip_grad_norm_ + position-LR schedule against fixtures produced by
torch.optim.Adam / torch.nn.utils.clip_grad_norm_ at the reference's call-site settings (scripts/train.py:394-401,
446-457, 536-538), float64."""
import importlib

import numpy as np
import pytest
import torch

from tests import util

PKG = "3d-gaussian-splatting-for-novel-view-synthesis_amd"
NAMES = ("pos", "opacity_raw", "f_dc", "f_rest", "scale_raw", "q_raw")


def test_position_lr_schedule_cpu():
    optim = importlib.import_module(PKG + ".optim")
    d = dict(np.load(util.GOLDEN + "/optim.npz"))
    for it, lr in zip(d["iters"], d["pos_lr"]):
        assert abs(optim.position_lr(int(it)) - lr) <= 1e-15 + 1e-12 * lr


@pytest.mark.gpu
def test_fused_adam_matches_torch_adam_at_the_reference_settings():
    optim = importlib.import_module(PKG + ".optim")
    d = dict(np.load(util.GOLDEN + "/optim.npz"))
    dev = "cuda:0"

    class M:
        pass
    m = M()
    for k in NAMES:
        setattr(m, k, torch.tensor(d["init_" + k], device=dev).requires_grad_(True))
    opt = optim.GaussianAdam(optim.reference_param_groups(m), lr=0.01, eps=1e-15)
    for j, it in enumerate(d["iters"]):
        opt.param_groups[0]['lr'] = optim.position_lr(int(it))
        for k in NAMES:
            getattr(m, k).grad = torch.tensor(d["grads_" + k][j], device=dev)
        cn = opt.clip_grad_norm_(m.pos, max_norm=1.0)
        opt.step()
        assert abs(float(cn[1]) - d["pos_grad_norm"][j]) <= 1e-5 * d["pos_grad_norm"][j]
        assert np.abs(m.pos.grad.cpu().numpy() - d[f"clipped{j}_pos"]).max() <= 1e-5 * np.abs(d[f"clipped{j}_pos"]).max()
        for k in NAMES:
            ref = d[f"after{j}_{k}"]
            got = getattr(m, k).detach().cpu().numpy()
            # parameters are O(1), one step moves them by ~lr: compare the accumulated movement
            moved = np.abs(ref - d["init_" + k]).max()
            # + a few fp32 ulps of the parameter itself (the position LR is 1.6e-6: steps are close to the fp32 resolution)
            assert np.abs(got - ref).max() <= 2e-4 * moved + 4 * 1.2e-7 * max(1.0, np.abs(ref).max()), (k, j, np.abs(got - ref).max(), moved)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu = M()
        for k in NAMES:
            setattr(cpu, k, torch.zeros(2, 3).requires_grad_(True))
            getattr(cpu, k).grad = torch.zeros(2, 3)
        optim.GaussianAdam(optim.reference_param_groups(cpu)).step()


@pytest.mark.gpu
def test_full_training_step_runs():
    """render -> loss -> backward -> clip -> Adam on a golden scene: finite, and the loss goes down over a few steps."""
    gs = importlib.import_module(PKG)
    optim = importlib.import_module(PKG + ".optim")
    d = util.load("g1_generic")
    dev = "cuda:0"

    class M:
        pass
    m = M()
    for k in NAMES:
        setattr(m, k, torch.tensor(d[k], device=dev).requires_grad_(True))
    target = torch.tensor(d["image"], dtype=torch.float32, device=dev)
    # perturb the colours: the optimiser has something to fix
    with torch.no_grad():
        m.f_dc += 0.5 * torch.randn_like(m.f_dc)
    opt = optim.GaussianAdam(optim.reference_param_groups(m), lr=0.01, eps=1e-15)
    c2w = torch.tensor(d["c2w"], device=dev)
    hist = []
    for it in range(25):
        opt.zero_grad()
        img = gs.render_gaussians(m.pos, m.f_dc, m.f_rest, m.opacity_raw, m.scale_raw, m.q_raw, c2w, *util.cam_args(d))
        total, parts = gs.compute_loss(img, target)
        total.backward()
        opt.param_groups[0]['lr'] = optim.position_lr(it)
        opt.clip_grad_norm_(m.pos, 1.0)
        opt.step()
        hist.append(parts['total'])
    assert all(np.isfinite(hist)) and hist[-1] < 0.8 * hist[0], hist


@pytest.mark.gpu
def test_adam_launch_for_many_tensors_handles_tails_unaligned_views_and_more_than_eight_groups():
    """gsplat_adam_step_multi: one launch for up to eight tensors with 16-byte accesses where the four arrays of a tensor allow it.
    Sizes that are no multiple of four (the tail), views that start 4 bytes into an allocation (the scalar path), an empty tensor, and
    eleven tensors (two launches) against torch.optim.Adam in float64; the second step runs with a clip coefficient on one tensor."""
    optim = importlib.import_module(PKG + ".optim")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(3)
    sizes = [1, 2, 3, 5, 4097, 70001, 0, 1024, 333, 12, 7]
    base, params, ref, first = [], [], [], {}
    for k, n in enumerate(sizes):
        off = 1 if k % 3 == 1 else 0                                       # every third tensor: misaligned by one float
        buf = torch.randn(n + off, generator=g).to(dev)
        base.append(buf)
        first[k] = float(buf[0]) if n + off else None
        p = buf[off:].detach().requires_grad_(True)
        assert (p.data_ptr() % 16 != 0) == (off == 1 and n > 0) or n == 0
        params.append(p)
        ref.append(torch.nn.Parameter(p.detach().cpu().double()))
    groups = [{'params': [p], 'lr': 0.01 * (k + 1)} for k, p in enumerate(params)]
    opt = optim.GaussianAdam(groups, lr=0.01, eps=1e-15)
    topt = torch.optim.Adam([{'params': [r], 'lr': 0.01 * (k + 1)} for k, r in enumerate(ref)], lr=0.01, eps=1e-15)
    for step in range(3):
        for p, r in zip(params, ref):
            gr = torch.randn(p.shape, generator=g) * (5.0 if step == 1 else 1.0)
            p.grad = gr.to(dev) if p.numel() else torch.zeros_like(p)
            r.grad = gr.double()
        if step == 1:
            opt.clip_grad_norm_(params[5], max_norm=1.0)
            torch.nn.utils.clip_grad_norm_(ref[5], max_norm=1.0)
        opt.step()
        topt.step()
        for k, (p, r) in enumerate(zip(params, ref)):
            if p.numel():
                err = (p.detach().cpu().double() - r.detach()).abs().max()
                assert err <= 2e-6 * max(1.0, float(r.detach().abs().max())), (step, k, sizes[k], float(err))
    for k, n in enumerate(sizes):                                          # the float in front of a misaligned view was never written
        if k % 3 == 1:
            assert float(base[k][0]) == first[k]


# ---------------------------------------------------------------------------------------------------------------------------------
# Edges of the optimiser kernels: more than one pass of the grid-stride loops, gradients down to where g^2 is a denormal
# (eps = 1e-15 makes the step scale-free), exact zeros, coef == 1, the single-tensor entry.
# ---------------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
NORM_BLOCK = 1024 * 256        # values the norm kernel's 1024 workgroups cover in one pass
# Relative bounds on the moments against torch.optim.Adam in float64.  The entry points take the betas as fp32: the kernel's 1 - b is
# exact for the fp32 beta and differs from the float64 run's by up to half an ulp of beta, 2^-25 for 0.9 and 0.999 -- 3e-7 of
# 1 - b1 = 0.1 and 3e-5 of 1 - b2 = 0.001 (the step is consistent with it: the bias corrections use the same fp32 betas).  On top of
# that a few fp32 roundings per step: 1e-6.
M_REL, V_REL = 2.0 ** -25 / 0.1 + 1e-6, 2.0 ** -25 / 0.001 + 1e-6


def _adam_pair(p0, lr=0.01, eps=1e-15):
    """(parameter on the GPU, GaussianAdam, float64 parameter on the CPU, torch.optim.Adam) from one initial fp32 tensor."""
    optim = importlib.import_module(PKG + ".optim")
    p = p0.to(DEV).requires_grad_(True)
    r = torch.nn.Parameter(p0.double())
    return p, optim.GaussianAdam([{'params': [p]}], lr=lr, eps=eps), r, torch.optim.Adam([r], lr=lr, eps=eps)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, NORM_BLOCK, NORM_BLOCK + 1, 3 * NORM_BLOCK + 5])
def test_clip_grad_norm_over_tails_and_more_than_one_stride(n):
    """gsplat_clip_grad_norm + the step that applies it against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64: one value,
    a tail of a workgroup, exactly one pass of the 1024 workgroups, one value more, three passes and a tail.  A norm above max_norm
    clips; below it coef == 1.0 exactly and the stored gradient keeps its bits; an all-zero gradient has norm 0, coef 1 and moves
    nothing."""
    gen = torch.Generator().manual_seed(100 + n % 1000)
    p, opt, r, topt = _adam_pair(torch.randn(n, generator=gen))
    for step, target_norm in enumerate((5.0, 0.5)):
        g = torch.randn(n, generator=gen)
        g = g * (target_norm / float(g.double().norm()))
        p.grad = g.to(DEV)
        r.grad = g.double()
        cn = opt.clip_grad_norm_(p, max_norm=1.0)
        opt.step()
        ref_norm = float(torch.nn.utils.clip_grad_norm_(r, max_norm=1.0))
        topt.step()
        coef, norm = float(cn[0]), float(cn[1])
        print(f"n = {n}, norm {ref_norm:.6g}: HIP norm {norm:.6g} coef {coef:.6g}")
        assert abs(norm - ref_norm) <= 1e-5 * ref_norm
        clipped = r.grad.numpy()
        assert np.abs(p.grad.cpu().numpy() - clipped).max() <= 1e-5 * np.abs(clipped).max()
        if target_norm > 1.0:
            assert coef < 1.0 and abs(coef - 1.0 / (ref_norm + 1e-6)) <= 1e-5 * coef
        else:
            assert coef == 1.0
            assert torch.equal(p.grad.cpu(), g), "coef == 1: the gradient written back must be the one given, bit for bit"
        err = (p.detach().cpu().double() - r.detach()).abs().max()
        assert err <= 2e-6 * max(1.0, float(r.detach().abs().max())), (n, step, float(err))
    # an all-zero gradient on a fresh optimiser (a Gaussian no view has seen yet)
    p0 = torch.randn(n, generator=gen)
    p, opt, _, _ = _adam_pair(p0)
    p.grad = torch.zeros(n, device=DEV)
    cn = opt.clip_grad_norm_(p, max_norm=1.0)
    opt.step()
    assert float(cn[1]) == 0.0 and float(cn[0]) == 1.0
    assert torch.isfinite(p).all() and torch.equal(p.detach().cpu(), p0), "an all-zero gradient moved a parameter"
    assert float(p.grad.abs().max()) == 0.0
    assert float(opt.state[p]['exp_avg'].abs().max()) == 0.0 and float(opt.state[p]['exp_avg_sq'].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned_16_byte_path", "offset_by_one_float_scalar_path"])
def test_adam_over_more_than_one_stride(offset):
    """adam_kernel gives a tensor at most 4096 workgroups: 4 * 4096 * 256 + 4 * 256 + 3 values make the 16-byte path run a second
    pass (one workgroup's worth) and leave a tail of three; the same length as a view one float into its allocation takes the scalar
    path over five passes.  Three steps against torch.optim.Adam in float64; the float in front of the view is never written."""
    optim = importlib.import_module(PKG + ".optim")
    n = 4 * 4096 * 256 + 4 * 256 + 3
    gen = torch.Generator().manual_seed(7 + offset)
    buf = torch.randn(n + offset, generator=gen).to(DEV)
    first = float(buf[0])
    p = buf[offset:].detach().requires_grad_(True)
    assert (p.data_ptr() % 16 != 0) == (offset == 1)
    r = torch.nn.Parameter(p.detach().cpu().double())
    opt = optim.GaussianAdam([{'params': [p]}], lr=0.01, eps=1e-15)
    topt = torch.optim.Adam([r], lr=0.01, eps=1e-15)
    for step in range(3):
        g = torch.randn(n, generator=gen)
        p.grad = g.to(DEV)
        r.grad = g.double()
        opt.step()
        topt.step()
        d = (p.detach().cpu().double() - r.detach()).abs()
        err, where = float(d.max()), int(d.argmax())
        print(f"offset {offset} step {step}: max |err| {err:.2e} at {where} of {n}")
        assert err <= 2e-6 * max(1.0, float(r.detach().abs().max())), (step, err, where)
    st = opt.state[p]
    ref_st = topt.state[r]
    assert (st['exp_avg'].cpu().double() - ref_st['exp_avg']).abs().max() <= M_REL * float(ref_st['exp_avg'].abs().max())
    assert (st['exp_avg_sq'].cpu().double() - ref_st['exp_avg_sq']).abs().max() <= V_REL * float(ref_st['exp_avg_sq'].abs().max())
    if offset:
        assert float(buf[0]) == first
    del buf, p, opt, st
    torch.cuda.empty_cache()


GRAD_SCALES = (1e3, 1.0, 1e-8, 1e-18, 1e-20, 1e-22)


@pytest.mark.gpu
def test_adam_gradient_magnitudes_down_to_denormal_squares():
    """With eps = 1e-15 the step is scale-free down to |g| ~ 1e-13; below, g / (|g| + eps) shrinks it (1e-18: lr / 1000), and from
    |g| ~ 1e-19 down g^2, (1 - b2) g^2 and its square root are denormals that have to survive: flushed, the denominator loses its
    sqrt(v) part.  Per element N(0, 1) x a scale from 1e3 to 1e-22, a tenth of the elements exactly zero in every step; three steps from
    N(0, 1e-3) parameters (a step of lr is far above their fp32 resolution) against torch.optim.Adam in float64.  Bound per scale
    class: 2e-4 x the movement + 4 ulp (the form of the golden test above), widened only to K_CAL x the error torch.optim.Adam in
    FLOAT32 on the CPU makes on the same inputs; the share of elements beyond the plain bound may likewise reach K_CAL x that of fp32
    torch.  The moments: M_REL / V_REL wherever the float64 value is a normal fp32 number (exp_avg against the sum of the magnitudes it
    is made of: its terms cancel)."""
    optim = importlib.import_module(PKG + ".optim")
    n_class, lr, b1, b2 = 8192, 0.01, 0.9, 0.999
    n = n_class * len(GRAD_SCALES) + 3                                     # (+ 3: the 16-byte path's tail takes part)
    gen = torch.Generator().manual_seed(31)
    cls = torch.arange(n) % len(GRAD_SCALES)
    scale = torch.tensor(GRAD_SCALES, dtype=torch.float64)[cls]
    zero = torch.rand(n, generator=gen) < 0.1
    p0 = (1e-3 * torch.randn(n, generator=gen)).float()
    grads = []
    for _ in range(3):
        g = (torch.randn(n, generator=gen, dtype=torch.float64) * scale).float()          # (rounded to fp32 once: all three runs see the same numbers)
        g[zero] = 0.0
        grads.append(g)
    p = p0.to(DEV).requires_grad_(True)
    opt = optim.GaussianAdam([{'params': [p]}], lr=lr, eps=1e-15)
    r64, r32 = torch.nn.Parameter(p0.double()), torch.nn.Parameter(p0.clone())
    t64, t32 = torch.optim.Adam([r64], lr=lr, eps=1e-15), torch.optim.Adam([r32], lr=lr, eps=1e-15)
    for g in grads:
        p.grad, r64.grad, r32.grad = g.to(DEV), g.double(), g.clone()
        opt.step()
        t64.step()
        t32.step()
    got, ref, cal = p.detach().cpu().double(), r64.detach(), r32.detach().double()
    m, v = opt.state[p]['exp_avg'].cpu().double(), opt.state[p]['exp_avg_sq'].cpu().double()
    m64, v64 = t64.state[r64]['exp_avg'], t64.state[r64]['exp_avg_sq']
    # exact zeros: never visible Gaussians do not move, and their moments stay zero
    assert torch.equal(p.detach().cpu()[zero], p0[zero]), "a parameter with an exactly zero gradient moved"
    assert float(m[zero].abs().max()) == 0.0 and float(v[zero].abs().max()) == 0.0
    FLT_MIN = 1.17549435e-38
    absg = torch.stack([g.double().abs() for g in grads])
    m_scale = b1 * b1 * (1 - b1) * absg[0] + b1 * (1 - b1) * absg[1] + (1 - b1) * absg[2]   # the sum of the magnitudes m is made of
    failures = []
    for k, s in enumerate(GRAD_SCALES):
        sel = (cls == k) & ~zero
        moved = (ref[sel] - p0.double()[sel]).abs()
        plain = 2e-4 * float(moved.max()) + 4 * 1.2e-7 * float(ref[sel].abs().max())
        e, c = (got[sel] - ref[sel]).abs(), (cal[sel] - ref[sel]).abs()
        bound = max(plain, util.K_CAL * float(c.max()))
        frac, cfrac = float((e > plain).double().mean()), float((c > plain).double().mean())
        frac_allowed = util.K_CAL * cfrac + 1.0 / int(sel.sum())
        ok_m = m64[sel].abs() >= FLT_MIN
        em = float(((m[sel] - m64[sel]).abs() / m_scale[sel])[ok_m].max()) if ok_m.any() else float("nan")
        ok_v = v64[sel] >= FLT_MIN
        ev = float(((v[sel] - v64[sel]).abs() / v64[sel])[ok_v].max()) if ok_v.any() else float("nan")
        print(f"gradient scale {s:g}: moved {float(moved.max()):.3e} (median {float(moved.median()):.3e}); max |err| HIP {float(e.max()):.2e}, "
              f"fp32 torch {float(c.max()):.2e} (plain bound {plain:.2e}, allowed {bound:.2e}); beyond the plain bound: HIP {frac:.2e}, fp32 torch "
              f"{cfrac:.2e} (allowed {frac_allowed:.2e}); exp_avg rel {em:.2e} on {int(ok_m.sum())}, exp_avg_sq rel {ev:.2e} on {int(ok_v.sum())} normal values")
        if float(e.max()) > bound:
            failures.append(f"scale {s:g}: max |err| {float(e.max()):.3e} > {bound:.3e}")
        if frac > frac_allowed:
            failures.append(f"scale {s:g}: {frac:.3e} of the elements beyond {plain:.3e} (allowed {frac_allowed:.3e})")
        if ok_m.any() and not em <= M_REL:
            failures.append(f"scale {s:g}: exp_avg off by {em:.3e} of its terms")
        if ok_v.any() and not ev <= V_REL:
            failures.append(f"scale {s:g}: exp_avg_sq off by {ev:.3e} relative")
    assert torch.isfinite(p).all()
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("with_scale", [False, True], ids=["no_grad_scale", "grad_scale"])
def test_single_tensor_adam_entry_equals_the_multi_entry_with_one_group(with_scale):
    """gsplat_adam_step (the single-tensor form of the header; no Python code calls it) and gsplat_adam_step_multi with one group: the
    same bits in parameter, gradient and both moments, over two steps, with and without a device-side gradient scale, on an
    aligned tensor with a tail and on a view one float into its allocation."""
    import ctypes as C
    abi = importlib.import_module(PKG + "._abi")
    ops = importlib.import_module(PKG + ".ops")
    lib = abi.lib()
    stream = ops._stream_ptr(torch.device(DEV))
    gen = torch.Generator().manual_seed(41)
    gs = torch.tensor([0.37], device=DEV) if with_scale else None
    for n, off in ((70001, 0), (4099, 1), (1, 0)):
        init = [torch.randn(n + off, generator=gen) for _ in range(2)] + [torch.rand(n + off, generator=gen) for _ in range(2)]
        init[1] = init[1] * 1e-3                                             # p, m, v, and below a gradient per step
        grads = [torch.randn(n + off, generator=gen) for _ in range(2)]
        runs = []
        for entry in ("single", "multi"):
            bufs = [t.to(DEV) for t in (init[0], grads[0], init[1], init[2])]                  # p, g, m, v
            pp, gg, mm, vv = [b[off:] for b in bufs]
            assert (pp.data_ptr() % 16 != 0) == (off == 1)
            for step in (1, 2):
                gg.copy_(grads[step - 1][off:].to(DEV))
                if entry == "single":
                    abi.check(lib.gsplat_adam_step(n, ops._p(pp), ops._p(gg), ops._p(mm), ops._p(vv), 0.01, 0.9, 0.999, 1e-15, step, ops._p(gs),
                                                   stream), "gsplat_adam_step")
                else:
                    one = (abi.AdamGroup * 1)(abi.AdamGroup(n, ops._p(pp).value, ops._p(gg).value, ops._p(mm).value, ops._p(vv).value, 0.01, step,
                                                            ops._p(gs).value if gs is not None else None))
                    abi.check(lib.gsplat_adam_step_multi(1, one, 0.9, 0.999, 1e-15, stream), "gsplat_adam_step_multi")
            torch.cuda.synchronize()
            runs.append([b.cpu() for b in bufs])
        for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), *runs):
            assert torch.equal(a, b), (n, off, name, float((a - b).abs().max()))
        assert not torch.equal(runs[0][0], init[0]), "the step moved nothing"
        if with_scale:
            assert torch.equal(runs[0][1][off:], grads[1][off:] * torch.tensor(0.37)), "the scaled gradient is written back"
        if off:
            for t, orig in zip(runs[0], (init[0], grads[0], init[1], init[2])):
                assert float(t[0]) == float(orig[0]), "the float in front of a view was written"
