// host_math_check.cpp -- host build of the per-Gaussian bodies in gs_body.h, for CPU unit tests only.
//
// NOT part of the product path: the product library (libgsplat_mi355x.so) contains only HIP kernels and fails
// loudly without a GPU.  This file lets `pytest -m "not gpu"` check the projection math (forward and analytic
// backward) against the oracle on a machine with no GPU, before any GPU time is spent.
#include <type_traits>

#include "gs_body.h"

using namespace gsm;

extern "C" {

// rect / tiles: the reference's own tile rectangle and pair count (F10/F11); brect / btiles: what the kernels bin
// (tight box, 16 x 8 half-tile lists)
void hm_project(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, float* rec64, uint32_t* rect, float* depth,
                uint32_t* tiles, int32_t* vis, uint32_t* brect, uint32_t* btiles, uint32_t* bmask) {
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v);
    const bool fused = g->scale_raw != nullptr;
    Records out{(Rec64*)rec64, (u2*)brect, depth, btiles, bmask, (u2*)rect, tiles};
    for (int64_t i = 0; i < g->n; ++i) {
        ShCoefGlobal coef{fused ? g->f_dc + i * 3 : nullptr, fused ? g->f_rest + i * 45 : nullptr};
        vis[i] = project_one(i, *g, fused, coef, cam, vk, out);
    }
}

void hm_project_backward(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, const uint32_t* tiles,
                         const float* grad2d, const gsplat_gaussian_grads* out) {
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v);
    const bool fused = g->scale_raw != nullptr;
    for (int64_t i = 0; i < g->n; ++i) {
        ShCoefGlobal coef{fused ? g->f_dc + i * 3 : nullptr, fused ? g->f_rest + i * 45 : nullptr};
        ShEmitGlobal emit{fused ? out->f_dc + i * 3 : nullptr, fused ? out->f_rest + i * 45 : nullptr};
        project_backward_one(i, *g, fused, coef, emit, cam, vk, tiles, grad2d, out);
    }
}

// The same two with the GSPLAT_FILTER_* bits of `flags` (the screen-space low-pass and the opacity compensation): the FILTER
// variants of the bodies, as the kernels select them.  flags without those bits: exactly hm_project / hm_project_backward.
void hm_project_flags(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, int32_t flags, float* rec64, uint32_t* rect,
                      float* depth, uint32_t* tiles, int32_t* vis, uint32_t* brect, uint32_t* btiles, uint32_t* bmask) {
    if (!(flags & GSPLAT_FILTER_LOWPASS(255))) return hm_project(g, c2w, v, rec64, rect, depth, tiles, vis, brect, btiles, bmask);
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v, flags);
    const bool fused = g->scale_raw != nullptr;
    Records out{(Rec64*)rec64, (u2*)brect, depth, btiles, bmask, (u2*)rect, tiles};
    for (int64_t i = 0; i < g->n; ++i) {
        ShCoefGlobal coef{fused ? g->f_dc + i * 3 : nullptr, fused ? g->f_rest + i * 45 : nullptr};
        vis[i] = project_one<true>(i, *g, fused, coef, cam, vk, out);
    }
}

void hm_project_backward_flags(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, int32_t flags, const uint32_t* tiles,
                               const float* grad2d, const gsplat_gaussian_grads* out) {
    if (!(flags & GSPLAT_FILTER_LOWPASS(255))) return hm_project_backward(g, c2w, v, tiles, grad2d, out);
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v, flags);
    const bool fused = g->scale_raw != nullptr;
    for (int64_t i = 0; i < g->n; ++i) {
        ShCoefGlobal coef{fused ? g->f_dc + i * 3 : nullptr, fused ? g->f_rest + i * 45 : nullptr};
        ShEmitGlobal emit{fused ? out->f_dc + i * 3 : nullptr, fused ? out->f_rest + i * 45 : nullptr};
        project_backward_one<true>(i, *g, fused, coef, emit, cam, vk, tiles, grad2d, out);
    }
}

// rho[n] of the FILTER projection (1 without GSPLAT_FILTER_ANTIALIAS; 0 for a Gaussian that is not projected): for the needle test
void hm_filter_rho(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, int32_t flags, float* rho) {
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v, flags);
    const bool fused = g->scale_raw != nullptr;
    for (int64_t i = 0; i < g->n; ++i) {
        const GaussIn in = load_gauss_global(i, *g, fused);
        float S[6]; CovMid cm;
        if (fused) cov_from_params(in.sr, in.qr, S, cm);
        else load_cov6(in.S9, S);
        Proj o; ProjMid m;
        m.rho = 0.f;
        project_gaussian<true>(in.p, S, in.o_raw, cam, vk, o, m, fused ? &cm : nullptr);
        rho[i] = o.vis == VIS_CULLED ? 0.f : m.rho;
    }
}

namespace {
struct ShEmitNullable {     // ShEmitGlobal that drops the values when there is no gradient row (pose only)
    float* dc;
    float* rest;
    void operator()(int k, int ch, float v) const {
        if (dc) ShEmitGlobal{dc, rest}(k, ch, v);
    }
};
}  // namespace

// hm_project_backward plus the camera-pose gradient: grad_c2w[16] = dL/dc2w (4 x 4 row-major) of the rows' cotangents, the
// per-Gaussian terms of gs_math.h pose_grad_w summed in double.  out may be NULL (pose only).
void hm_project_backward_pose(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, const uint32_t* tiles,
                              const float* grad2d, const gsplat_gaussian_grads* out, float* grad_c2w) {
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v);
    const bool fused = g->scale_raw != nullptr;
    double sw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sp[3] = {0, 0, 0};
    for (int64_t i = 0; i < g->n; ++i) {
        ShCoefGlobal coef{fused ? g->f_dc + i * 3 : nullptr, fused ? g->f_rest + i * 45 : nullptr};
        ShEmitNullable emit{fused && out ? out->f_dc + i * 3 : nullptr, fused && out ? out->f_rest + i * 45 : nullptr};
        float gw[9];
        const GradOut o = project_backward_one(i, *g, fused, coef, emit, cam, vk, tiles, grad2d, out, gw);
        for (int k = 0; k < 9; ++k) sw[k] += gw[k];
        for (int k = 0; k < 3; ++k) sp[k] += o.p[k];
    }
    // W = c2w[:3,:3]^T: dL/dc2w[:3,:3] = (dL/dW)^T; dL/dc2w[:3,3] = -sum dL/dp; the last row is constant
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) grad_c2w[r * 4 + c] = (float)sw[c * 3 + r];
        grad_c2w[r * 4 + 3] = (float)-sp[r];
    }
    for (int c = 0; c < 4; ++c) grad_c2w[12 + c] = 0.f;
}

void hm_project_backward_pose_flags(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, int32_t flags, const uint32_t* tiles,
                                    const float* grad2d, const gsplat_gaussian_grads* out, float* grad_c2w) {
    if (!(flags & GSPLAT_FILTER_LOWPASS(255))) return hm_project_backward_pose(g, c2w, v, tiles, grad2d, out, grad_c2w);
    Camera cam; build_camera(c2w, cam);
    const ViewK vk = make_viewk(*v, flags);
    const bool fused = g->scale_raw != nullptr;
    double sw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sp[3] = {0, 0, 0};
    for (int64_t i = 0; i < g->n; ++i) {
        ShCoefGlobal coef{fused ? g->f_dc + i * 3 : nullptr, fused ? g->f_rest + i * 45 : nullptr};
        ShEmitNullable emit{fused && out ? out->f_dc + i * 3 : nullptr, fused && out ? out->f_rest + i * 45 : nullptr};
        float gw[9];
        const GradOut o = project_backward_one<true>(i, *g, fused, coef, emit, cam, vk, tiles, grad2d, out, gw);
        for (int k = 0; k < 9; ++k) sw[k] += gw[k];
        for (int k = 0; k < 3; ++k) sp[k] += o.p[k];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) grad_c2w[r * 4 + c] = (float)sw[c * 3 + r];
        grad_c2w[r * 4 + 3] = (float)-sp[r];
    }
    for (int c = 0; c < 4; ++c) grad_c2w[12 + c] = 0.f;
}

extern "C++" {      // (a template cannot have C linkage)
namespace {
// one instantiation of the K8 body, over every Gaussian, the way project_backward_kernel calls it: `moments` rows, the Jacobian
// sh_colour_jac<NB> leaves (from_jac) instead of the coefficients, dL/dz from column 9 of grad2d (DEPTH)
template <bool POSE, bool DEPTH, int NB, bool FILTER>
void backward_variant(const gsplat_gaussians& g, const Camera& cam, const ViewK& vk, bool moments, bool from_jac, const uint32_t* tiles,
                      const float* grad2d, const gsplat_gaussian_grads* out, float* grad_c2w) {
    const bool fused = g.scale_raw != nullptr;
    double sw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sp[3] = {0, 0, 0};
    for (int64_t i = 0; i < g.n; ++i) {
        const GaussIn in = load_gauss_global(i, g, fused);
        const bool vis = tiles[i] != 0;
        ShCoefGlobal coef{fused ? g.f_dc + i * 3 : nullptr, fused ? g.f_rest + i * 45 : nullptr};
        ShEmitNullable emit{fused && out ? out->f_dc + i * 3 : nullptr, fused && out ? out->f_rest + i * 45 : nullptr};
        float kj[12], rgb[3], gw[9];
        const bool jac = fused && from_jac;
        if (jac && vis) {
            ShMid sm;
            sh_basis(in.p, cam.eye, sm);
            sh_colour_jac<NB>(sm, coef, rgb, kj);
        }
        const GradOut o = project_backward_core<POSE, DEPTH, NB, FILTER>(in, fused, coef, emit, cam, vk, vis, grad2d + i * 16, moments,
                                                                         jac ? kj : nullptr, POSE ? gw : nullptr, DEPTH ? grad2d[i * 16 + 9] : 0.f);
        if (POSE) {
            for (int k = 0; k < 9; ++k) sw[k] += gw[k];
            for (int k = 0; k < 3; ++k) sp[k] += o.p[k];
        }
        if (!out) continue;
        for (int k = 0; k < 3; ++k) out->pos[i * 3 + k] = o.p[k];
        out->opacity_raw[i] = o.o_raw;
        if (fused) {
            for (int k = 0; k < 3; ++k) out->scale_raw[i * 3 + k] = o.sr[k];
            for (int k = 0; k < 4; ++k) out->q_raw[i * 4 + k] = o.qr[k];
        } else {
            for (int k = 0; k < 9; ++k) out->sigma[i * 9 + k] = o.S9[k];
            for (int k = 0; k < 3; ++k) out->color[i * 3 + k] = o.col[k];
        }
    }
    if (POSE) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) grad_c2w[r * 4 + c] = (float)sw[c * 3 + r];
            grad_c2w[r * 4 + 3] = (float)-sp[r];
        }
        for (int c = 0; c < 4; ++c) grad_c2w[12 + c] = 0.f;
    }
}
}  // namespace
}  // extern "C++"

// The K8 body in any of its <POSE, DEPTH, NB, FILTER> instantiations: flags = the GSPLAT_FILTER_* bits (FILTER = a low-pass is set),
// degree 0..3 (NB = (degree + 1)^2; un-fused inputs: 3), depth: column 9 of grad2d is dL/dz, moments: columns 0..5 are the raster
// backward's moment sums (else the 2-D gradients themselves), from_jac: the colour backward from sh_colour_jac's 12 values.
// grad_c2w == NULL: no pose; out == NULL with a pose: pose only.  Returns 0, or 1 for arguments outside that.
int hm_project_backward_variant(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, int32_t flags, int32_t degree, int32_t depth,
                                int32_t moments, int32_t from_jac, const uint32_t* tiles, const float* grad2d,
                                const gsplat_gaussian_grads* out, float* grad_c2w) {
    if (degree < 0 || degree > 3 || (!out && !grad_c2w) || (!g->scale_raw && degree != 3)) return 1;
    Camera cam; build_camera(c2w, cam);
    const bool filter = (flags & GSPLAT_FILTER_LOWPASS(255)) != 0;
    const ViewK vk = make_viewk(*v, filter ? flags : 0);
    const bool m = moments != 0, j = from_jac != 0;
    return with_sh_bases(degree, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        auto run = [&](auto pose, auto dep, auto filt) {
            backward_variant<decltype(pose)::value, decltype(dep)::value, NB, decltype(filt)::value>(*g, cam, vk, m, j, tiles, grad2d, out, grad_c2w);
        };
        auto with_bool = [](bool b, auto f) { if (b) f(std::true_type{}); else f(std::false_type{}); };
        with_bool(grad_c2w != nullptr, [&](auto pose) {
            with_bool(depth != 0, [&](auto dep) { with_bool(filter, [&](auto filt) { run(pose, dep, filt); }); });
        });
        return 0;
    });
}

// the row spans of a large Gaussian's rectangle (gs_math.h big_row_span), as the binning kernels enumerate them: xa[r], xb[r] for the
// rows by0 .. by1 of the rectangle (rect_lo = bx0 | by0 << 16, rect_hi = bx1 | by1 << 16); empty rows have xa > xb
void hm_row_spans(const float* rec16, uint32_t rect_lo, uint32_t rect_hi, const gsplat_view* v, int32_t* xa, int32_t* xb) {
    const ViewK vk = make_viewk(*v);
    const int bx0 = rect_lo & 0xFFFF, by0 = rect_lo >> 16, bx1 = rect_hi & 0xFFFF, by1 = rect_hi >> 16;
    float k4[4];
    big_span_constants(rec16[2], rec16[3], rec16[4], rec16[6], vk.chi_pad, k4);
    const BigSpanK bk = big_span_setup(rec16[0], rec16[1], rec16[6], rec16[7], k4, bx0, bx1);
    for (int y = by0; y <= by1; ++y) {
        const RowSpan sp = big_row_span(bk, y);
        xa[y - by0] = sp.xa; xb[y - by0] = sp.xb;
    }
}

void hm_build_sigma(int64_t n, const float* scale_raw, const float* q_raw, float* sigma) {
    for (int64_t i = 0; i < n; ++i) build_sigma_one(i, scale_raw, q_raw, sigma);
}
void hm_build_sigma_backward(int64_t n, const float* scale_raw, const float* q_raw, const float* grad_sigma, float* gs, float* gq) {
    for (int64_t i = 0; i < n; ++i) build_sigma_backward_one(i, scale_raw, q_raw, grad_sigma, gs, gq);
}
void hm_evaluate_sh(int64_t n, const float* f_dc, const float* f_rest, const float* pts, const float* c2w, float* color) {
    Camera cam; build_camera(c2w, cam);
    for (int64_t i = 0; i < n; ++i) evaluate_sh_one(i, f_dc, f_rest, pts, cam, color);
}
void hm_evaluate_sh_backward(int64_t n, const float* f_dc, const float* f_rest, const float* pts, const float* c2w,
                             const float* grad_color, float* g_dc, float* g_rest, float* g_pts) {
    Camera cam; build_camera(c2w, cam);
    for (int64_t i = 0; i < n; ++i) evaluate_sh_backward_one(i, f_dc, f_rest, pts, cam, grad_color, g_dc, g_rest, g_pts);
}

// ---- the SH colour at a degree (0..3): the code the projection kernels run with NB = (degree + 1)^2 active bases --------------
// Both return 0, or 1 for a degree outside 0..3 (nothing is written then).
// color[n,3]; kj[n,12] = the saved Jacobian of sh_colour_jac (d rgb / d logit [3], d logit / d point [3][3]).
int hm_sh_colour_degree(int64_t n, const float* f_dc, const float* f_rest, const float* pts, const float* c2w, int32_t degree,
                        float* color, float* kj) {
    if (degree < 0 || degree > 3) return 1;
    Camera cam; build_camera(c2w, cam);
    return with_sh_bases(degree, [&](auto nb) {
        for (int64_t i = 0; i < n; ++i) {
            ShMid sm;
            sh_basis(pts + i * 3, cam.eye, sm);
            sh_colour_jac<decltype(nb)::value>(sm, ShCoefGlobal{f_dc + i * 3, f_rest + i * 45}, color + i * 3, kj + i * 12);
        }
        return 0;
    });
}
// The backward of that colour: from_jac = 0 from the coefficients (sh_colour_backward), 1 from the saved Jacobian
// (sh_colour_backward_jac, which does not read f_dc / f_rest again).  Every slot of g_dc[n,3], g_rest[n,45], g_pts[n,3] is written.
int hm_sh_backward_degree(int64_t n, const float* f_dc, const float* f_rest, const float* pts, const float* c2w,
                          const float* grad_color, int32_t degree, int32_t from_jac, float* g_dc, float* g_rest, float* g_pts) {
    if (degree < 0 || degree > 3) return 1;
    Camera cam; build_camera(c2w, cam);
    return with_sh_bases(degree, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        for (int64_t i = 0; i < n; ++i) {
            ShMid sm;
            sh_basis(pts + i * 3, cam.eye, sm);
            const ShCoefGlobal coef{f_dc + i * 3, f_rest + i * 45};
            const ShEmitGlobal emit{g_dc + i * 3, g_rest + i * 45};
            float rgb[3], kj[12];
            if (from_jac) {
                sh_colour_jac<NB>(sm, coef, rgb, kj);
                sh_colour_backward_jac<NB>(sm, kj, grad_color + i * 3, emit, g_pts + i * 3);
            } else {
                sh_colour<NB>(sm, coef, rgb);
                sh_colour_backward<NB>(sm, coef, rgb, grad_color + i * 3, emit, g_pts + i * 3);
            }
        }
        return 0;
    });
}
}
