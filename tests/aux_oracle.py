"""Oracle of the depth / opacity maps and the background (helper, not a test).

Built on oracle/torch_port.py without changing it: the oracle projects and bins (F4-F13, stop_after_binning), and the F14 loop of
torch_port.render is repeated here over its tiles with five channels (r, g, b, z, 1) -- the same alpha, T and alive rule:

    w_i = alpha_i T_i [T_i > 5e-5],  C = sum w_i c_i,  A = sum w_i,  D = sum w_i z_i,  image = clamp(C + (1 - A) bg, 0, 1)

Everything is differentiable (the camera depth z included), in the dtype of the inputs.
"""
import torch

from oracle import torch_port as tp


def _zero_maps(color, H, W):
    z = color.sum() * 0.0                                # (keeps the graph: zero gradients, like torch_port._zero_image)
    return z.expand(H * W * 3).reshape(H, W, 3), z.expand(H * W).reshape(H, W), z.expand(H * W).reshape(H, W)


def _compose(C, D, A, background):
    if background is not None:
        C = C + (1 - A).unsqueeze(-1) * torch.as_tensor(background, dtype=C.dtype)
    return C.clamp(0, 1), D, A


def render_aux_unfused(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, background=None, **kw):
    """(image, depth, alpha) of torch_port.render's scene."""
    H, W = int(H), int(W)
    st = {}
    early = tp.render(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, stages=st, stop_after_binning=True, **kw)
    if early is not None:                                # no survivor: the zero image (the off-screen case has raised)
        return _compose(*_zero_maps(color, H, W), background)
    T = int(kw.get("T", 16))
    chi = kw.get("chi_square_clip", 6.25)
    alpha_max, alpha_cutoff = kw.get("alpha_max", 0.99), kw.get("alpha_cutoff", 1 / 128.)
    u, v, opacity, col, conic = st["u"], st["v"], st["opacity"], st["color"], st["conic"]
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


def render_aux(pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw, c2w, H, W, fx, fy, cx, cy, background=None, **kw):
    """(image, depth, alpha) of torch_port.render_fused's scene, in the dtype of its inputs."""
    sigma = tp.covariance_from_params(scale_raw, q_raw)
    color = tp.sh_colour(f_dc, f_rest, pos, c2w)
    return render_aux_unfused(pos, color, opacity_raw, sigma, c2w, H, W, fx, fy, cx, cy, background=background, **kw)
