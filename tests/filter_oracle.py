"""Oracle of the screen-space low-pass and the antialiased opacity (helper, not a test).

Built on oracle/torch_port.py without changing it.  Sigma + s I has Sigma's eigenvectors and its eigenvalues plus s, and the oracle
clamps AFTER torch.linalg.eigh: inside `lowpass_eigh(s)` that function returns (lambda + s, V), which turns
tp.render(..., stages=st, stop_after_binning=True) into the filtered projection and binning -- radii, tile rectangles, the pair count
P and the conics included.  The opacity compensation

    rho = sqrt(max(det Sigma, 0) / det(Sigma + s I)),   det Sigma = l1 l2,  det(Sigma + s I) = (l1 + s)(l2 + s)

follows from the UNFILTERED eigenvalues the wrapper saw (before the clamp); they belong to the frustum survivors (F4-F6), whose
indices are recomputed here and mapped to the final survivors through st["ids"].  The F14 loop of torch_port.render is then repeated
over the oracle's tiles with st["opacity"] * rho, as tests/aux_oracle.py repeats it, carrying the channels (r, g, b, z, 1) and a
background.  Everything is differentiable, in the dtype of the inputs; s is the float32-rounded value in both dtypes, as the kernels'.
"""
import contextlib

import numpy as np
import torch

from oracle import torch_port as tp


def lowpass_value(lowpass):
    """The s the kernels use: hundredths of a px^2, rounded once to float32."""
    return float(np.float32(round(float(lowpass) * 100.0) * 0.01))


@contextlib.contextmanager
def lowpass_eigh(s):
    """Inside the block torch.linalg.eigh(A) returns (eigenvalues + s, eigenvectors); yields the list of the unfiltered eigenvalue
    tensors it saw, one per call."""
    seen = []
    real = torch.linalg.eigh

    def eigh(A, *args, **kw):
        lam, vec = real(A, *args, **kw)
        seen.append(lam)
        return lam + s, vec

    torch.linalg.eigh = eigh
    try:
        yield seen
    finally:
        torch.linalg.eigh = real


def _zero_maps(color, H, W):
    z = color.sum() * 0.0
    return z.expand(H * W * 3).reshape(H, W, 3), z.expand(H * W).reshape(H, W), z.expand(H * W).reshape(H, W)


def _compose(C, D, A, background):
    if background is not None:
        C = C + (1 - A).unsqueeze(-1) * torch.as_tensor(background, dtype=C.dtype)
    return C.clamp(0, 1), D, A


def render_unfused(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, lowpass=0.0, antialias=False, background=None,
                   stages=None, stop_after_binning=False, **kw):
    """(image, depth, alpha) of torch_port.render's scene under the filter; `stages` (a dict) receives the oracle's stages of the
    filtered projection plus rho [survivors] and opacity_record = opacity * rho.  stop_after_binning (with `stages`): return None
    once the stages are there (no compositing)."""
    H, W = int(H), int(W)
    s = lowpass_value(lowpass)
    st = stages if stages is not None else {}
    with lowpass_eigh(s) as seen:
        early = tp.render(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, stages=st, stop_after_binning=True, **kw)
    if early is not None:                                # no survivor: the zero image (the off-screen case has raised)
        return _compose(*_zero_maps(color, H, W), background)
    T = int(kw.get("T", 16))
    chi = kw.get("chi_square_clip", 6.25)
    alpha_max, alpha_cutoff = kw.get("alpha_max", 0.99), kw.get("alpha_cutoff", 1 / 128.)
    u, v, opacity, col, conic = st["u"], st["v"], st["opacity"], st["color"], st["conic"]
    if antialias:
        # the Gaussians the eigh call saw: the survivors of F4 (opacity) and F6 (frustum), in input order
        keep = torch.sigmoid(opacity_raw).clamp(0, 0.999) >= alpha_cutoff * 0.5
        x_, y_, z_ = tp.to_camera(pos, c2w)
        keep = keep & tp.in_frustum(x_, y_, z_, fx, fy, cx, cy, H, W, kw.get("near", 0.01), kw.get("far", 100.0), kw.get("pix_guard", 32))
        lam = seen[0]
        assert lam.shape[0] == int(keep.sum())
        slot = torch.full((pos.shape[0],), -1, dtype=torch.int64)
        slot[keep] = torch.arange(lam.shape[0])
        lam = lam[slot[st["ids"]]]
        rho = torch.sqrt((lam[:, 0] * lam[:, 1]).clamp(min=0) / ((lam[:, 0] + s) * (lam[:, 1] + s)))
        opacity = opacity * rho
    else:
        rho = torch.ones_like(opacity)
    st["rho"], st["opacity_record"] = rho, opacity
    if stop_after_binning:
        return None
    z = tp.to_camera(pos, c2w)[2][st["ids"]]
    c5 = torch.cat([col, z.unsqueeze(1), torch.ones_like(z).unsqueeze(1)], 1)            # (r, g, b, z, 1)
    k11, k12, k22 = conic[:, 0], conic[:, 1], conic[:, 2]
    tiles_x = (W + T - 1) // T
    chunks, where = [], []
    for t, s0, s1 in zip(st["tile_ids"].tolist(), st["tile_start"].tolist(), st["tile_end"].tolist()):
        gx, gy = (t % tiles_x) * T, (t // tiles_x) * T
        w_t, h_t = min(gx + T, W) - gx, min(gy + T, H) - gy
        if w_t <= 0 or h_t <= 0:
            continue
        px = torch.arange(gx, gx + w_t, dtype=pos.dtype).repeat(h_t)
        py = torch.arange(gy, gy + h_t, dtype=pos.dtype).repeat_interleave(w_t)
        g = st["pair_gauss"][s0:s1]
        du = px.unsqueeze(0) - u[g].unsqueeze(1)
        dv = py.unsqueeze(0) - v[g].unsqueeze(1)
        q = k11[g].unsqueeze(1) * du * du + 2 * k12[g].unsqueeze(1) * du * dv + k22[g].unsqueeze(1) * dv * dv
        fall = torch.exp(-0.5 * q.clamp(max=chi))
        fall = torch.where(q <= chi, fall, torch.zeros_like(fall))
        alpha = (opacity[g].unsqueeze(1) * fall).clamp_max(alpha_max)
        alpha = torch.where(alpha >= alpha_cutoff, alpha, torch.zeros_like(alpha))
        trans = torch.cumprod(1 - alpha, 0)
        trans = torch.cat([torch.ones_like(trans[:1]), trans[:-1]], 0)      # exclusive product
        w = alpha * trans * (trans > 5e-5).to(pos.dtype)
        chunks.append((w.unsqueeze(-1) * c5[g].unsqueeze(1)).sum(0))
        where.append((py * W + px).to(torch.int64))
    out = pos.new_zeros(H * W, 5)
    if chunks:
        out = out.scatter_add(0, torch.cat(where).unsqueeze(-1).expand(-1, 5), torch.cat(chunks))
    out = out.reshape(H, W, 5)
    return _compose(out[..., :3], out[..., 3], out[..., 4], background)


def render(pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw, c2w, H, W, fx, fy, cx, cy, lowpass=0.0, antialias=False, background=None,
           stages=None, stop_after_binning=False, **kw):
    """(image, depth, alpha) of torch_port.render_fused's scene under the filter."""
    sigma = tp.covariance_from_params(scale_raw, q_raw)
    color = tp.sh_colour(f_dc, f_rest, pos, c2w)
    return render_unfused(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, lowpass=lowpass, antialias=antialias,
                          background=background, stages=stages, stop_after_binning=stop_after_binning, **kw)


def pair_count(stages):
    """The reference's (tile, Gaussian) pairs P of the filtered projection."""
    return int(stages["pair_gauss"].shape[0])
