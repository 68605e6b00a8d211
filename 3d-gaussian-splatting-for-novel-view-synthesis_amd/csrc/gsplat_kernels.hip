// gsplat_kernels.hip -- MI355X (gfx950, wave64) kernels and the C ABI of include/gsplat_mi355x.h.
//
// Pipeline (stage ids of SURVEY.md §8a in brackets):
//   K1  project_kernel         per Gaussian: camera block, culls, EWA, eigen clamp, conic, rectangles; optionally the SH colour;
//                              counters totalled by its last wave                              [F1-F8, F10, F13 (+F3)]
//   K1b colour_kernel          SH colour of the binned Gaussians as a pass of its own (host waits for the counters)   [F3]
//   K3  bin_count / bin_scatter / split_count / split_scatter_kernel   two-level counting sort of the pairs by list  [F11, F12]
//   K4  list_sort_kernel       per-list depth sort in LDS (lists of 8192+: in global memory)    [F9, F12]
//   K5  plan_kernel            longest-first launch order of the lists, sort size classes
//   K6  raster_forward_kernel  one wave64 per 16 x 8-pixel list = eight 8-lane groups, one 4 x 4 sub-tile each   [F14, F15]
//   K7  raster_backward_kernel same traversal, analytic gradients, sums per group -> LDS slots -> one atomic per pair   [B1]
//       (K6, K7 <AUX>: depth and opacity maps beside the colour, a background under it -- not in the reference)
//       (+ tile_block_sum / pair_base / pair_reduce_kernel: deterministic mode)
//   K8  project_backward_kernel chain rule to the reference's input tensors                     [B2, B3]
//   K9  densify_stats_kernel / densify_stats_merge_kernel   screen-space densification statistics behind K7 (not in the reference)
//       (K7, K9 <ABS>: the absolute-gradient statistic -- two sums more per pair, columns 10-11 of grad2d)
//   K9b visible_set_kernel                                  the rows a frame binned, one byte each (gs_visible.h; not in the reference)
//   K10 raster_contrib_kernel  K6's traversal without colours: per-Gaussian blending-weight statistics (not in the reference)
//   K11 raster_features_kernel / K12 raster_features_adjoint_kernel   K6's traversal over an [n, C] feature table, 8 channels per wave,
//                              and its adjoint (gs_features.h; not in the reference)
//
// Everything is hand-written HIP for gfx950; no library kernels.  No MFMA: there is no dense contraction on this path.
// No CPU fallback: without a GPU every entry point returns GSPLAT_ERR_HIP.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include <hip/hip_runtime.h>

#include "gs_layout.h"
#include "gs_wave.h"
#include "gs_project.h"
#include "gs_bin.h"
#include "gs_sort.h"
#include "gs_raster.h"
#include "gs_project_backward.h"
#include "gs_densify.h"
#include "gs_visible.h"
#include "gs_contrib.h"
#include "gs_features.h"
#include "gs_ops.h"

thread_local char gsplat_err_buf[512] = "";      // shared with gsplat_loss.hip; read through gsplat_last_error()

namespace {

char (&g_err)[512] = gsplat_err_buf;

int fail(int code, const char* fmt, const char* a = "", const char* b = "") {
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) return fail(GSPLAT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// hipLaunchKernelGGL(kernel, grid, block, LDS bytes, stream, arguments...) and the check of the launch
#define LAUNCH(name, ...)                                                               \
    do {                                                                                \
        hipLaunchKernelGGL(__VA_ARGS__);                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) return fail(GSPLAT_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e_)); \
    } while (0)

// the 13 traversal arguments that K10, K11 and K12 begin with (counts ... id_max), from the entry's Ctx `c` and its own arguments
#define WALK_ARGS(c, pair_capacity, bin_state, n)                                                                      \
    (c).ps.counts, (long long)(pair_capacity), (c).ps.ranges, (const uint32_t*)(bin_state), (c).ps.rec, (c).ps.order, \
    (c).vk.lists_x, (c).vk.H, (c).vk.W, (c).vk.chi_clip, (c).vk.alpha_max, (c).vk.alpha_cutoff, (uint32_t)((n) - 1)

int check_view(const gsplat_view* v) {
    if (!v) return fail(GSPLAT_ERR_BAD_ARG, "view is NULL");
    if (v->H <= 0 || v->W <= 0) return fail(GSPLAT_ERR_BAD_ARG, "image size must be positive");
    if (v->tile < 1) return fail(GSPLAT_ERR_BAD_ARG, "tile size T must be >= 1");
    if ((v->W + 15) / 16 > 65535 || (v->H + 7) / 8 > 65535 || n_bins(n_lists(v)) > MAX_BINS) return fail(GSPLAT_ERR_BAD_ARG, "image too large");
    return GSPLAT_OK;
}

int check_gaussians(const gsplat_gaussians* g, bool* fused) {
    if (!g) return fail(GSPLAT_ERR_BAD_ARG, "gaussians is NULL");
    if (g->n < 0 || g->n > (int64_t)ID_MASK + 1) return fail(GSPLAT_ERR_BAD_ARG, "n out of range (at most 2^26 Gaussians per call)");
    const bool f = g->scale_raw || g->q_raw || g->f_dc || g->f_rest;
    const bool u = g->color || g->sigma;
    if (f == u) return fail(GSPLAT_ERR_BAD_ARG, "give either (color, sigma) or (scale_raw, q_raw, f_dc, f_rest)");
    if (g->n > 0) {
        if (!g->pos || !g->opacity_raw) return fail(GSPLAT_ERR_BAD_ARG, "pos / opacity_raw is NULL");
        if (f && !(g->scale_raw && g->q_raw && g->f_dc && g->f_rest)) return fail(GSPLAT_ERR_BAD_ARG, "fused inputs incomplete");
        if (u && !(g->color && g->sigma)) return fail(GSPLAT_ERR_BAD_ARG, "color / sigma is NULL");
    }
    const void* ptrs[] = {g->pos, g->opacity_raw, g->color, g->sigma, g->scale_raw, g->q_raw, g->f_dc, g->f_rest};
    for (const void* q : ptrs)
        if (q && (reinterpret_cast<uintptr_t>(q) & 15u)) return fail(GSPLAT_ERR_BAD_ARG, "Gaussian arrays must be 16-byte aligned");
    *fused = f;
    return GSPLAT_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What an entry that works on a frame needs, built once (host arithmetic only; after the entry's argument checks).
struct Ctx { hipStream_t st; ViewK vk; int64_t nl, nb; ProjectState ps; };
Ctx open_ctx(int64_t n, const gsplat_view* v, const void* project_state, void* stream_, int32_t filter = 0) {
    const int64_t nl = n_lists(v);
    return Ctx{(hipStream_t)stream_, make_viewk(*v, filter), nl, n_bins(nl), carve_project((void*)project_state, n > 0 ? n : 1, nl)};
}

// TOTALS = !late (GSPLAT_PROJECT_COUNTS_LATE)
template <bool FUSED, bool COLOUR, bool JAC, int NB = 16, bool FILTER = false>
auto project_kernel_for(bool late) { return late ? project_kernel<FUSED, COLOUR, JAC, false, NB, FILTER> : project_kernel<FUSED, COLOUR, JAC, true, NB, FILTER>; }

// The screen-space low-pass travels in the same bits of the flags of the six entries that run the projection math
// (include/gsplat_mi355x.h: GSPLAT_FILTER_ANTIALIAS, GSPLAT_FILTER_LOWPASS).  Host dispatch from the bits to the FILTER variants:
// f(std::true_type / std::false_type), like with_sh_bases.
constexpr int32_t FILTER_BITS = GSPLAT_FILTER_ANTIALIAS | GSPLAT_FILTER_LOWPASS(255);
template <class F>
inline auto with_filter(int32_t filter, F f) { return filter ? f(std::true_type{}) : f(std::false_type{}); }
int check_filter(const char* entry, int32_t flags) {
    if ((flags & GSPLAT_FILTER_ANTIALIAS) && !(flags & GSPLAT_FILTER_LOWPASS(255)))
        return fail(GSPLAT_ERR_BAD_ARG, "%s: GSPLAT_FILTER_ANTIALIAS needs a low-pass (GSPLAT_FILTER_LOWPASS(c) with c > 0)", entry);
    return GSPLAT_OK;
}
// Which filter bits was a project_state last projected with?  Kept on the HOST (the state itself is device memory, and a backward call
// is refused before anything is launched): only filtered states have an entry, so the default path erases from an empty map.  An
// entry outlives its state until the address is projected again; the table is cleared should it ever hold 65 536 of them.
std::mutex g_filter_mutex;
std::unordered_map<const void*, int32_t> g_filter_of;
void note_filter(const void* project_state, int32_t filter) {
    std::lock_guard<std::mutex> lock(g_filter_mutex);
    if (!filter) { if (!g_filter_of.empty()) g_filter_of.erase(project_state); return; }
    if (g_filter_of.size() >= 65536) g_filter_of.clear();
    g_filter_of[project_state] = filter;
}
int check_filter_of(const char* entry, const void* project_state, int32_t filter) {
    int32_t was = 0;
    {
        std::lock_guard<std::mutex> lock(g_filter_mutex);
        if (!g_filter_of.empty()) {
            const auto it = g_filter_of.find(project_state);
            if (it != g_filter_of.end()) was = it->second;
        }
    }
    if (was != filter) return fail(GSPLAT_ERR_BAD_ARG, "%s: the GSPLAT_FILTER_* bits differ from those the state was projected with", entry);
    return GSPLAT_OK;
}

// The SH degree of a fused render travels in two flag bits as "bands dropped" = 3 - degree, so that flags of 0 stay degree 3:
// bits 4-5 of gsplat_project / gsplat_forward_deferred, bits 8-9 of the backward entries (include/gsplat_mi355x.h).
constexpr int32_t PROJECT_SH_BITS = GSPLAT_PROJECT_SH_DEGREE(0), BACKWARD_SH_BITS = GSPLAT_BACKWARD_SH_DEGREE(0);
static_assert(GSPLAT_FRAME_SH_DEGREE(0) == PROJECT_SH_BITS, "gsplat_forward_deferred hands its degree bits to gsplat_project as they are");
inline int project_sh_degree(int32_t flags) { return 3 - ((flags & PROJECT_SH_BITS) >> 4); }
inline int backward_sh_degree(int32_t flags) { return 3 - ((flags & BACKWARD_SH_BITS) >> 8); }
int check_sh_degree(const char* entry, int degree, bool fused) {
    if (degree != 3 && !fused) return fail(GSPLAT_ERR_BAD_ARG, "%s: an SH degree below 3 needs fused inputs (scale_raw, q_raw, f_dc, f_rest): color + sigma carry no SH", entry);
    return GSPLAT_OK;
}

// the flag bits the backward entries define; a call with any other bit is refused before it does anything (a library that ignored
// a flag it does not know would, for GSPLAT_BACKWARD_ACCUMULATE, overwrite where the caller adds)
// (GSPLAT_BACKWARD_DEPTH: the two projection entries only -- the composite entries have no depth / opacity frame)
constexpr int32_t PROJECT_BACKWARD_FLAGS = GSPLAT_BACKWARD_SH_JACOBIAN | GSPLAT_BACKWARD_ACCUMULATE | GSPLAT_BACKWARD_DEPTH;
constexpr int32_t BACKWARD_FLAGS = GSPLAT_BACKWARD_SH_JACOBIAN | GSPLAT_BACKWARD_ACCUMULATE | GSPLAT_BACKWARD_PHASE_RASTER |
                                   GSPLAT_BACKWARD_PHASE_PROJECT | GSPLAT_BACKWARD_GRAD2D_DIRTY | GSPLAT_BACKWARD_ABSGRAD;

// K8 for gsplat_project_backward, the composite entries (ar: the in-place f_rest step) and gsplat_project_backward_pose (pose: where
// the camera-pose gradient goes; `out` may then be NULL = pose only).
struct PoseOut { float* grad_c2w; void* scratch; int64_t scratch_bytes; };
// K8 of fused inputs at NB active SH bases -- <FUSED, JAC, ADAM, ACC, POSE, DEPTH, NB, FILTER>: every fused instantiation there is
template <int NB, bool FILTER = false>
auto fused_backward_kernel_for(bool adam, bool acc, bool depth, bool pose, bool jac) {
    return adam    ? project_backward_kernel<true, true, true, false, false, false, NB, FILTER>
           : acc   ? project_backward_kernel<true, true, false, true, false, false, NB, FILTER>
           : depth ? (pose ? (jac ? project_backward_kernel<true, true, false, false, true, true, NB, FILTER>
                                  : project_backward_kernel<true, false, false, false, true, true, NB, FILTER>)
                           : (jac ? project_backward_kernel<true, true, false, false, false, true, NB, FILTER>
                                  : project_backward_kernel<true, false, false, false, false, true, NB, FILTER>))
           : pose  ? (jac ? project_backward_kernel<true, true, false, false, true, false, NB, FILTER>
                          : project_backward_kernel<true, false, false, false, true, false, NB, FILTER>)
                   : (jac ? project_backward_kernel<true, true, false, false, false, false, NB, FILTER>
                          : project_backward_kernel<true, false, false, false, false, false, NB, FILTER>);
}
// ... and of un-fused inputs
template <bool FILTER = false>
auto unfused_backward_kernel_for(bool depth, bool pose) {
    return depth ? (pose ? project_backward_kernel<false, false, false, false, true, true, 16, FILTER> : project_backward_kernel<false, false, false, false, false, true, 16, FILTER>)
                 : (pose ? project_backward_kernel<false, false, false, false, true, false, 16, FILTER> : project_backward_kernel<false, false, false, false, false, false, 16, FILTER>);
}

// entry: the name of the C ABI entry, for the messages that must carry it
int project_backward_impl(const char* entry, const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, const void* project_state, const float* grad2d,
                          const gsplat_gaussian_grads* out, int32_t flags, void* stream_, const AdamRest* ar, const PoseOut* pose = nullptr) {
    bool fused = false;
    const int32_t filter = flags & FILTER_BITS;
    int rc = check_filter(entry, flags);
    if (rc) return rc;
    if ((rc = check_gaussians(g, &fused))) return rc;
    const int degree = backward_sh_degree(flags);
    if ((rc = check_sh_degree(entry, degree, fused))) return rc;
    if ((rc = check_view(v))) return rc;
    if (pose && !pose->grad_c2w) return fail(GSPLAT_ERR_BAD_ARG, "grad_c2w is NULL");
    if (!c2w || !project_state || !grad2d || (!pose && !out)) return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    PoseScratch prs = {nullptr, nullptr, 0, 0};
    if ((rc = check_filter_of(entry, project_state, filter))) return rc;
    if (pose) {
        prs = carve_pose(pose->scratch, g->n);
        if (!pose->scratch || pose->scratch_bytes < prs.bytes) return fail(GSPLAT_ERR_WORKSPACE, "pose scratch too small (gsplat_pose_scratch_bytes)");
        if (reinterpret_cast<uintptr_t>(pose->scratch) & 63u) return fail(GSPLAT_ERR_BAD_ARG, "pose scratch must be 64-byte aligned");
    } else if (g->n == 0) {
        return GSPLAT_OK;
    }
    // fused inputs, f_dc and f_rest NULL, color given: hand out the colour-logit gradients instead of the SH gradients (a pose call
    // too: the kernel's `factored` branches do not depend on POSE; a pose call without `out` writes no gradient rows at all)
    const bool factored = out && fused && !out->f_dc && !out->f_rest;
    const bool jac = fused && (flags & GSPLAT_BACKWARD_SH_JACOBIAN) != 0;
    const bool acc = (flags & GSPLAT_BACKWARD_ACCUMULATE) != 0;
    const bool depth = (flags & GSPLAT_BACKWARD_DEPTH) != 0;
    if (depth && (acc || ar)) return fail(GSPLAT_ERR_BAD_ARG, "GSPLAT_BACKWARD_DEPTH goes with the plain backward (no accumulation, no in-place step)");
    if (out) {
        if (!out->pos || !out->opacity_raw) return fail(GSPLAT_ERR_BAD_ARG, "grad pos / opacity_raw is NULL");
        if (acc && (ar || !(jac && !factored)))
            return fail(GSPLAT_ERR_BAD_ARG, "GSPLAT_BACKWARD_ACCUMULATE needs fused inputs, the saved SH Jacobian and SH gradients (no factored exchange, no in-place step)");
        if (ar && !(jac && !factored))
            return fail(GSPLAT_ERR_BAD_ARG, "the in-place f_rest step needs fused inputs, the saved SH Jacobian and SH gradients (no factored exchange)");
        if (fused && !factored && !(out->scale_raw && out->q_raw && out->f_dc && (out->f_rest || ar))) return fail(GSPLAT_ERR_BAD_ARG, "fused grads incomplete");
        if (factored && !(out->scale_raw && out->q_raw)) return fail(GSPLAT_ERR_BAD_ARG, "fused grads incomplete");
        if (!fused && !(out->color && out->sigma)) return fail(GSPLAT_ERR_BAD_ARG, "grad color / sigma is NULL");
    }
    const Ctx c = open_ctx(g->n, v, project_state, stream_, filter);
    if (g->n == 0) {                // (pose only: the other entries have left)
        HIP_TRY(hipMemsetAsync(pose->grad_c2w, 0, 16 * sizeof(float), c.st));
        return GSPLAT_OK;
    }
    AdamRest a = {nullptr, nullptr, nullptr, {0.f, 0.f, 0.f, 0.f, 0.f}, nullptr, 0};
    if (ar) { a = *ar; a.counts = c.ps.counts; }
    const gsplat_gaussian_grads o = out ? *out : gsplat_gaussian_grads{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // (ar and acc have been checked to come with fused inputs)
    const auto kernel = with_filter(filter, [&](auto filt) {
        constexpr bool FILTER = decltype(filt)::value;
        return fused ? with_sh_bases(degree, [&](auto nb) { return fused_backward_kernel_for<decltype(nb)::value, FILTER>(ar != nullptr, acc, depth, pose != nullptr, jac); })
                     : unfused_backward_kernel_for<FILTER>(depth, pose != nullptr);
    });
    LAUNCH(pose ? "project_backward_kernel<pose>" : "project_backward_kernel", kernel, dim3(blocks64(g->n)), dim3(64), 0, c.st, *g, c.ps.cam, c.vk, c.ps.tiles, grad2d, o, factored,
           jac ? c.ps.kj : nullptr, a, prs.rows);
    if (!pose) return GSPLAT_OK;
    const float* rows = reinterpret_cast<const float*>(prs.rows);
    if (prs.nrows > POSE_PARTS) {
        LAUNCH("pose_reduce_kernel", pose_reduce_kernel<false>, dim3(POSE_PARTS), dim3(256), 0, c.st, rows, prs.nrows, POSE_PARTS, prs.part);
        LAUNCH("pose_reduce_kernel<final>", pose_reduce_kernel<true>, dim3(1), dim3(256), 0, c.st, prs.part, (int64_t)POSE_PARTS, 1, pose->grad_c2w);
    } else {
        LAUNCH("pose_reduce_kernel<final>", pose_reduce_kernel<true>, dim3(1), dim3(256), 0, c.st, rows, prs.nrows, 1, pose->grad_c2w);
    }
    return GSPLAT_OK;
}

// the background of the depth / opacity entries: 3 host floats, NULL = none (the kernels then add nothing)
template <class Aux>
void set_background(Aux& a, const float* background) {
    a.has_bg = background != nullptr;
    for (int k = 0; k < 3; ++k) a.bg[k] = background ? background[k] : 0.f;
}

// K7 and (deterministic mode) the kernels around it, for gsplat_rasterize_backward and gsplat_rasterize_backward_aux (aux: the
// depth / opacity variant, rows of 10) and their _abs twins (abs: the absolute-gradient sums in columns 10-11, rows of 11 and 12).
constexpr int raster_row(bool aux, bool abs) { return (aux ? 10 : 9) + (abs ? 2 : 0); }
auto raster_backward_kernel_for(bool det, bool aux, bool abs) {
    return abs ? (aux ? (det ? raster_backward_kernel<true, true, true> : raster_backward_kernel<false, true, true>)
                      : (det ? raster_backward_kernel<true, false, true> : raster_backward_kernel<false, false, true>))
               : (aux ? (det ? raster_backward_kernel<true, true> : raster_backward_kernel<false, true>)
                      : (det ? raster_backward_kernel<true> : raster_backward_kernel<false>));
}
const char* raster_backward_name(bool det, bool aux, bool abs) {       // (the _abs launches never named their deterministic twin)
    return abs ? (aux ? "raster_backward_kernel<aux, abs>" : "raster_backward_kernel<abs>")
               : (aux ? (det ? "raster_backward_kernel<deterministic, aux>" : "raster_backward_kernel<aux>")
                      : (det ? "raster_backward_kernel<deterministic>" : "raster_backward_kernel"));
}
int raster_backward_impl(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, const void* bin_state,
                         const float* accum, const float* grad_image, float* grad2d, int32_t grad2d_zeroed, void* det_scratch,
                         int64_t det_scratch_bytes, void* stream_, const AuxBwd* aux, bool abs = false) {
    const auto [st, vk, nl, nb, ps] = open_ctx(n, v, project_state, stream_);
    const bool det = det_scratch != nullptr;
    const int row = raster_row(aux != nullptr, abs);
    if (!grad2d_zeroed && !det) HIP_TRY(hipMemsetAsync(grad2d, 0, (size_t)(n > 0 ? n : 0) * 16 * sizeof(float), st));
    if (n == 0) return GSPLAT_OK;
    if (n_binned == 0) {
        if (det) HIP_TRY(hipMemsetAsync(grad2d, 0, (size_t)n * 16 * sizeof(float), st));
        return GSPLAT_OK;
    }
    // deterministic: rows stored per (list, Gaussian) pair, then added per Gaussian in a fixed order
    const DetScratch ds = carve_det(det_scratch, n, n_binned, row);
    if (det) {
        if (ds.bytes > det_scratch_bytes) return fail(GSPLAT_ERR_WORKSPACE, "deterministic-backward scratch too small");
        const unsigned pb_blocks = (unsigned)((n + PB_BLOCK - 1) / PB_BLOCK);
        HIP_TRY(hipMemsetAsync(ds.part, 0, (size_t)n_binned * 4 * row, st));          // rows of entries a saturated list never reaches
        LAUNCH("tile_block_sum_kernel", tile_block_sum_kernel, dim3(pb_blocks), dim3(256), 0, st, n, ps.tiles, ds.block_sum);
        LAUNCH("pair_base_kernel", pair_base_kernel, dim3(pb_blocks), dim3(256), 0, st, n, ps.tiles, ds.block_sum, ds.pair_base);
    }
    const DetArgs da = det ? DetArgs{ps.rect, ps.mask, ps.tiles, ds.pair_base, ds.part, (uint32_t)n_binned} : DetArgs{};
    const bool a = aux != nullptr;
    LAUNCH(raster_backward_name(det, a, abs), raster_backward_kernel_for(det, a, abs), dim3((unsigned)nl), dim3(64), 0, st, ps.ranges,
           (const uint32_t*)bin_state, ps.rec, ps.order, vk.lists_x, vk.H, vk.W, vk.chi_clip, vk.alpha_max, vk.alpha_cutoff,
           accum, grad_image, grad2d, STATS_BWD, (uint32_t)(n - 1), da, pair_mask_of(bin_state, n_binned), a ? *aux : AuxBwd{});
    if (det) {
        const auto reduce = abs ? (a ? pair_reduce_kernel<12> : pair_reduce_kernel<11, true>) : (a ? pair_reduce_kernel<10> : pair_reduce_kernel<9>);
        LAUNCH(abs ? "pair_reduce_kernel<abs>" : "pair_reduce_kernel", reduce, dim3(blocks256(n)), dim3(256), 0, st, n, ps.tiles, ds.pair_base, ds.part,
               (uint32_t)n_binned, grad2d);
    }
    return GSPLAT_OK;
}

// a refusal of an entry whose messages name it (name given), or of one of the older entries, whose messages do not (name == NULL)
int refuse(const char* name, const char* msg) { return name ? fail(GSPLAT_ERR_BAD_ARG, "%s: %s", name, msg) : fail(GSPLAT_ERR_BAD_ARG, "%s", msg); }

// The opening refusals of an entry that walks a projected frame and names itself in its messages: the view, n, pair_capacity
// (pairs32: the entry's kernels index the pairs with 32 bits).
int check_walk(const char* name, int64_t n, int64_t pair_capacity, const gsplat_view* v, bool pairs32) {
    if (!v) return refuse(name, "view is NULL");
    if (check_view(v)) return refuse(name, "bad view (image size, tile size)");
    if (n < 0 || n > (int64_t)ID_MASK + 1 || pair_capacity < 0 || (pairs32 && pair_capacity > 0xFFFFFFFFLL)) return refuse(name, "n / pair_capacity out of range");
    return GSPLAT_OK;
}

// The four gsplat_rasterize_backward* entries behind their checks.  name: the entries whose refusals name them (they check n / n_binned,
// too); aux: the two depth / opacity entries, which read accum_aux ... background and may leave grad_image out; abs: the ABS kernels.
int raster_backward_entry(const char* name, bool aux, bool abs, int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, const void* bin_state,
                          const float* accum, const float* accum_aux, const float* grad_image, const float* grad_depth, const float* grad_alpha,
                          const float* background, float* grad2d, int32_t grad2d_zeroed, void* det_scratch, int64_t det_scratch_bytes, void* stream_) {
    if (int rc = name ? check_walk(name, n, n_binned, v, true) : check_view(v)) return rc;
    if (aux && !grad_image && !grad_depth && !grad_alpha) return refuse(name, "grad_image, grad_depth and grad_alpha are all NULL");
    if (!project_state || !bin_state || !accum || (aux ? !accum_aux : !grad_image) || !grad2d) return refuse(name, "NULL argument");
    AuxBwd ab = {accum_aux, grad_depth, grad_alpha, {0.f, 0.f, 0.f}, 0};
    if (aux) set_background(ab, background);
    return raster_backward_impl(n, n_binned, v, project_state, bin_state, accum, grad_image, grad2d, grad2d_zeroed, det_scratch, det_scratch_bytes,
                                stream_, aux ? &ab : nullptr, abs);
}

// K6 for gsplat_rasterize_forward and gsplat_rasterize_forward_aux (aux: depth, alpha and accum_aux are read, and the background)
int raster_forward_impl(bool aux, int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, void* bin_state, float* image, float* depth,
                        float* alpha, float* accum, float* accum_aux, float* grad2d, const float* background, void* stream_) {
    int rc = check_view(v);
    if (rc) return rc;
    if (!project_state || !bin_state || !image) return fail(GSPLAT_ERR_BAD_ARG, "state / image is NULL");
    if (aux && !accum != !accum_aux) return fail(GSPLAT_ERR_BAD_ARG, "accum and accum_aux go together");
    const Ctx c = open_ctx(n, v, project_state, stream_);
    AuxFwd af = {depth, alpha, accum_aux, {0.f, 0.f, 0.f}, 0};
    if (aux) set_background(af, background);
    // accum given = a backward pass will follow: exact sub-tile masks, saved per pair
    const auto kernel = aux ? (accum ? raster_forward_kernel<true, true> : raster_forward_kernel<false, true>)
                            : (accum ? raster_forward_kernel<true> : raster_forward_kernel<false>);
    LAUNCH(aux ? "raster_forward_kernel<aux>" : "raster_forward_kernel", kernel, dim3((unsigned)c.nl), dim3(64), 0, c.st, c.ps.ranges,
           (const uint32_t*)bin_state, c.ps.rec, c.ps.order, c.vk.lists_x, c.vk.H, c.vk.W, c.vk.chi_clip, c.vk.alpha_max, c.vk.alpha_cutoff,
           image, accum, STATS_FWD, (uint32_t)(n > 0 ? n - 1 : 0), grad2d, grad2d ? n : 0,
           accum ? pair_mask_of(bin_state, n_binned) : nullptr, af);
    return GSPLAT_OK;
}

// The preamble of an entry that reads a finished frame arena (every message names the entry): the view, n / pair_capacity, the
// arguments, the arena's alignment, and its size by frame_parts(flags) -- hint: how "frame arena too small" ends.
// (gsplat_forward_deferred and the backward entries check other things in another order, with messages of their own: not through here.)
int open_frame(const char* name, int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes, const void* out,
               int32_t flags, const char* hint, FrameParts* f) {
    if (!v) return refuse(name, "view is NULL");
    if (check_view(v)) return refuse(name, "bad view (image size, tile size)");
    if (n < 0 || pair_capacity < 0) return refuse(name, "n / pair_capacity out of range");
    if (!frame || !out) return refuse(name, "NULL argument");
    if (reinterpret_cast<uintptr_t>(frame) & 255u) return refuse(name, "frame must be 256-byte aligned");
    *f = frame_parts(n, pair_capacity, v, flags);
    if (f->total > frame_bytes) return fail(GSPLAT_ERR_BAD_ARG, "%s: frame arena too small%s", name, hint);
    return GSPLAT_OK;
}

// gsplat_densify_stats / gsplat_frame_densify_stats behind their argument checks (every message names the entry)
int densify_stats_impl(const char* name, int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const float* grad2d,
                       float* stats, void* stream_, bool abs = false) {
    if (int rc = check_walk(name, n, pair_capacity, v, false)) return rc;
    if (!project_state || !grad2d || !stats) return fail(GSPLAT_ERR_BAD_ARG, "%s: NULL argument", name);
    if (!aligned16(stats) || !aligned16(grad2d)) return fail(GSPLAT_ERR_BAD_ARG, "%s: stats / grad2d must be 16-byte aligned", name);
    if (n == 0) return GSPLAT_OK;
    const Ctx c = open_ctx(n, v, project_state, stream_);
    LAUNCH("densify_stats_kernel", abs ? densify_stats_kernel<true> : densify_stats_kernel<false>, dim3(blocks256(n)), dim3(256), 0, c.st, n, c.ps.counts, (long long)pair_capacity, c.ps.tiles,
           c.ps.rec, grad2d, 0.5f * (float)v->W, 0.5f * (float)v->H, reinterpret_cast<f4*>(stats));
    return GSPLAT_OK;
}

// gsplat_visible_set / gsplat_frame_visible_set behind their argument checks (every message names the entry)
int visible_set_impl(const char* name, int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, uint8_t* visible,
                     void* stream_) {
    if (int rc = check_walk(name, n, pair_capacity, v, false)) return rc;
    if (!project_state || !visible) return fail(GSPLAT_ERR_BAD_ARG, "%s: NULL argument", name);
    if (n == 0) return GSPLAT_OK;
    const Ctx c = open_ctx(n, v, project_state, stream_);
    LAUNCH("visible_set_kernel", visible_set_kernel, dim3(blocks256(n)), dim3(256), 0, c.st, n, c.ps.counts, (long long)pair_capacity, c.ps.tiles, visible);
    return GSPLAT_OK;
}

// gsplat_contribution / gsplat_frame_contribution behind their argument checks (every message names the entry)
int contribution_impl(const char* name, int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const void* bin_state,
                      uint32_t* record, void* stream_) {
    if (int rc = check_walk(name, n, pair_capacity, v, true)) return rc;
    if (!project_state || !bin_state || !record) return fail(GSPLAT_ERR_BAD_ARG, "%s: NULL argument", name);
    if (!aligned16(record)) return fail(GSPLAT_ERR_BAD_ARG, "%s: record must be 16-byte aligned", name);
    if (n == 0) return GSPLAT_OK;
    const Ctx c = open_ctx(n, v, project_state, stream_);
    LAUNCH("raster_contrib_kernel", raster_contrib_kernel, dim3((unsigned)c.nl), dim3(64), 0, c.st, WALK_ARGS(c, pair_capacity, bin_state, n), record);
    return GSPLAT_OK;
}

// gsplat_features_forward / gsplat_features_adjoint behind their argument checks (every message names the entry): `in` -> `out` is
// features -> the map, or grad_out -> grad_features
int features_impl(const char* name, bool adjoint, int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                  const void* bin_state, const float* in, int channels, float* out, void* stream_) {
    if (int rc = check_walk(name, n, pair_capacity, v, true)) return rc;
    if (!project_state || !bin_state || !in || !out) return fail(GSPLAT_ERR_BAD_ARG, "%s: NULL argument", name);
    if (channels < 1 || channels > GSPLAT_FEATURES_MAX_CHANNELS) return fail(GSPLAT_ERR_BAD_ARG, "%s: channels out of range (1 .. 512)", name);
    if (n == 0) return GSPLAT_OK;
    const Ctx c = open_ctx(n, v, project_state, stream_);
    const dim3 grid((unsigned)c.nl, (unsigned)((channels + FGROUP - 1) / FGROUP));
    // rows as two 16-byte accesses where every row of a full group is 16-byte aligned; the arrays the kernel moves float by float need no alignment
    const int vec = channels % 4 == 0 && aligned16(in) && (adjoint || aligned16(out));
    LAUNCH(adjoint ? "raster_features_adjoint_kernel" : "raster_features_kernel", adjoint ? raster_features_adjoint_kernel : raster_features_kernel,
           grid, dim3(64), 0, c.st, WALK_ARGS(c, pair_capacity, bin_state, n), in, channels, vec, out);
    return GSPLAT_OK;
}

}  // namespace

// ======================================================================================================
// C ABI
// ======================================================================================================
extern "C" {

int gsplat_abi_version(void) { return GSPLAT_ABI_VERSION; }

#ifdef GSPLAT_DIAGNOSTICS
// Diagnostics build only (libgsplat_mi355x_diag.so, loaded by tools/ alone; not declared in include/gsplat_mi355x.h and not
// in the product library): register device buffers of lists * 16 bytes each that the raster kernels fill with per-wave
// statistics; pass NULL to switch the statistics off again.
void gsplat_debug_set_stats(void* fwd, void* bwd) { g_stats_fwd = (WaveStats*)fwd; g_stats_bwd = (WaveStats*)bwd; }
// device buffers of n x 8 and n x 4 bytes that the projection kernel fills with the reference's tile rectangle / tile count
void gsplat_debug_set_ref_rect(void* rect, void* tiles) { g_ref_rect = (u2*)rect; g_ref_tiles = (uint32_t*)tiles; }
#endif

const char* gsplat_last_error(void) { return g_err; }

int gsplat_classify_counts(const gsplat_counts* c) {
    if (!c) return GSPLAT_SCENE_ALL_CULLED;
    if (c->n_survivors == 0) return GSPLAT_SCENE_ALL_CULLED;       // render.py:109-112,139-142,190-193
    if (c->n_visible == 0) return GSPLAT_SCENE_ALL_OFFSCREEN;      // render.py:235-236
    return GSPLAT_SCENE_OK;
}

// (the layouts themselves: gs_layout.h)
int64_t gsplat_project_state_bytes(int64_t n, const gsplat_view* v) {
    if (!v || v->H <= 0 || v->W <= 0) return -1;
    return carve_project(nullptr, n > 0 ? n : 1, n_lists(v)).bytes;
}

int64_t gsplat_project_scratch_bytes(int64_t n) { (void)n; return up(sizeof(CounterBlock)); }   // the persistent counter block

int64_t gsplat_bin_state_bytes(int64_t pair_capacity, const gsplat_view* v) { return v ? bin_state_bytes(pair_capacity) : -1; }

int64_t gsplat_bin_scratch_bytes(int64_t pair_capacity, const gsplat_view* v) {
    if (!v) return -1;
    return carve_bin_scratch(nullptr, pair_capacity, n_bins(n_lists(v))).bytes;
}

int64_t gsplat_rasterize_backward_scratch_bytes(int64_t n, int64_t pair_capacity) { return carve_det(nullptr, n, pair_capacity).bytes; }

int64_t gsplat_rasterize_backward_aux_scratch_bytes(int64_t n, int64_t pair_capacity) { return carve_det(nullptr, n, pair_capacity, 10).bytes; }

int64_t gsplat_rasterize_backward_abs_scratch_bytes(int64_t n, int64_t pair_capacity) { return carve_det(nullptr, n, pair_capacity, raster_row(false, true)).bytes; }

int64_t gsplat_rasterize_backward_aux_abs_scratch_bytes(int64_t n, int64_t pair_capacity) { return carve_det(nullptr, n, pair_capacity, raster_row(true, true)).bytes; }

int64_t gsplat_pose_scratch_bytes(int64_t n) { return n < 0 ? -1 : carve_pose(nullptr, n).bytes; }

int64_t gsplat_frame_bytes(int64_t n, int64_t pair_capacity, const gsplat_view* v, int32_t flags) {
    if (!v || v->H <= 0 || v->W <= 0 || n < 0 || pair_capacity < 0) return -1;
    return frame_parts(n, pair_capacity, v, flags).total;
}

// For tests and tools (see the header): the offsets carve_project / pair_mask_of give, so that nobody mirrors them.
int gsplat_project_state_layout(int64_t n, const gsplat_view* v, gsplat_state_layout* out) {
    if (!v || !out) return fail(GSPLAT_ERR_BAD_ARG, "gsplat_project_state_layout: view / out is NULL");
    if (v->H <= 0 || v->W <= 0 || n < 0) return fail(GSPLAT_ERR_BAD_ARG, "gsplat_project_state_layout: image size must be positive, n >= 0");
    const int64_t nl = n_lists(v);
    const ProjectState s = carve_project(nullptr, n > 0 ? n : 1, nl);
    const auto off = [](const void* p) { return (int64_t)reinterpret_cast<intptr_t>(p); };
    out->bytes = s.bytes; out->lists = nl;
    out->lists_x = (v->W + LIST_W - 1) / LIST_W; out->lists_y = (v->H + LIST_H - 1) / LIST_H;
    out->counts = off(s.counts); out->rec = off(s.rec); out->rect = off(s.rect); out->depth = off(s.depth); out->tiles = off(s.tiles);
    out->mask = off(s.mask); out->ranges = off(s.ranges); out->order = off(s.order); out->class_bounds = off(s.class_bounds);
    out->kj = off(s.kj);
    return GSPLAT_OK;
}

int gsplat_bin_state_layout(int64_t pair_capacity, const gsplat_view* v, gsplat_bin_layout* out) {
    if (!v || !out) return fail(GSPLAT_ERR_BAD_ARG, "gsplat_bin_state_layout: view / out is NULL");
    if (pair_capacity < 0) return fail(GSPLAT_ERR_BAD_ARG, "gsplat_bin_state_layout: pair_capacity must be >= 0");
    out->bytes = bin_state_bytes(pair_capacity);
    out->sorted_ids = 0;
    out->pair_mask = (int64_t)reinterpret_cast<intptr_t>(pair_mask_of(nullptr, pair_capacity));
    return GSPLAT_OK;
}

int gsplat_project(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* project_state, void* scratch,
                   int64_t scratch_bytes, gsplat_counts* counts_host, void* counts_event, int32_t flags, void* stream_) {
    bool fused = false;
    int rc = check_filter("gsplat_project", flags);
    if (rc) return rc;
    if ((rc = check_gaussians(g, &fused))) return rc;
    if ((rc = check_sh_degree("gsplat_project", project_sh_degree(flags), fused))) return rc;
    const int32_t filter = flags & FILTER_BITS;
    if ((rc = check_view(v))) return rc;
    if (!c2w || !project_state) return fail(GSPLAT_ERR_BAD_ARG, "c2w / project_state is NULL");
    if (!scratch || scratch_bytes < (int64_t)sizeof(CounterBlock)) return fail(GSPLAT_ERR_WORKSPACE, "project scratch (counter block) too small");
    if (reinterpret_cast<uintptr_t>(scratch) & 63u) return fail(GSPLAT_ERR_BAD_ARG, "project scratch must be 64-byte aligned");
    const int64_t n = g->n;
    const auto [st, vk, nl, nb, ps] = open_ctx(n, v, project_state, stream_, filter);
    note_filter(project_state, filter);
    const bool mapped = (flags & GSPLAT_PROJECT_COUNTS_MAPPED) != 0;
    const bool colour_inside = !fused || (flags & GSPLAT_PROJECT_COLOUR_FUSED) != 0;
    const bool jac = fused && (flags & GSPLAT_PROJECT_SAVE_SH_JACOBIAN) != 0;
    const bool late = (flags & GSPLAT_PROJECT_COUNTS_LATE) != 0 && n > 0;      // counters totalled by bin_count_kernel
    const int degree = project_sh_degree(flags);
    if (n > 0) {
        const Records out{ps.rec, ps.rect, ps.depth, ps.tiles, ps.mask, REF_RECT, REF_TILES};
        DevCounts* cm = mapped ? (DevCounts*)counts_host : nullptr;
        const auto kernel = with_filter(filter, [&](auto filt) {
            constexpr bool FILTER = decltype(filt)::value;
            return !fused          ? project_kernel_for<false, true, false, 16, FILTER>(late)
                   : colour_inside ? with_sh_bases(degree, [&](auto nb) {
                         constexpr int NB = decltype(nb)::value;
                         return jac ? project_kernel_for<true, true, true, NB, FILTER>(late) : project_kernel_for<true, true, false, NB, FILTER>(late);
                     })
                                   : project_kernel_for<true, false, false, 16, FILTER>(late);
        });
        LAUNCH("project_kernel", kernel, dim3(blocks64(n)), dim3(64), 0, st, *g, c2w, ps.cam, vk, out, (CounterBlock*)scratch, ps.counts, cm,
               ps.bin_total, (int)nb, colour_inside && jac ? ps.kj : nullptr, ps.big_flag);
        if (counts_host && !mapped && !late) HIP_TRY(hipMemcpyAsync(counts_host, ps.counts, sizeof(gsplat_counts), hipMemcpyDeviceToHost, st));
    } else {                        // no kernel runs: the counters are zero by definition
        HIP_TRY(hipMemsetAsync(ps.counts, 0, sizeof(DevCounts), st));
        HIP_TRY(hipMemsetAsync(ps.bin_total, 0, BIN_TOTAL_ROWS * nb * sizeof(uint32_t), st));
        if (counts_host) HIP_TRY(hipMemsetAsync(counts_host, 0, sizeof(gsplat_counts), st));
    }
    if (counts_event && !late) HIP_TRY(hipEventRecord((hipEvent_t)counts_event, st));
    if (n > 0) {                    // these need no pair buffer: queued behind the event, they run while a waiting host sizes the buffers
        LAUNCH("bin_count_kernel", bin_count_kernel, dim3((unsigned)(n_bin_blocks(n) + big_count_blocks(n))), dim3(256), bin_lds_bytes(nb, 256, 4), st, n, ps.rect, ps.tiles, ps.mask, vk.lists_x, (int)nb,
               ps.bin_total, ps.block_off, ps.list_count, ps.ranges, (int)nl, late ? (CounterBlock*)scratch : nullptr, ps.counts,
               late && mapped ? (DevCounts*)counts_host : nullptr, ps.rec, ps.big_flag, (uint32_t)n_bin_blocks(n), bin_batches(n));
        if (late) {                 // the counters exist only now
            if (counts_host && !mapped) HIP_TRY(hipMemcpyAsync(counts_host, ps.counts, sizeof(gsplat_counts), hipMemcpyDeviceToHost, st));
            if (counts_event) HIP_TRY(hipEventRecord((hipEvent_t)counts_event, st));
        }
        if (!colour_inside) {
            const auto colour = with_sh_bases(degree, [&](auto nb) {
                constexpr int NB = decltype(nb)::value;
                return jac ? colour_kernel<true, NB> : colour_kernel<false, NB>;
            });
            LAUNCH("colour_kernel", colour, dim3(blocks64(n)), dim3(64), 0, st, *g, ps.cam, ps.tiles, ps.rec, jac ? ps.kj : nullptr);
        }
    }
    return GSPLAT_OK;
}

int gsplat_bin(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, void* bin_state, void* scratch,
               int64_t scratch_bytes, void* stream_) {
    int rc = check_view(v);
    if (rc) return rc;
    const int64_t n_binned = pair_capacity;       // what the buffers hold; the actual count is read on the device (counts->n_binned)
    if (n < 0 || n_binned < 0 || n_binned > 0xFFFFFFFFLL) return fail(GSPLAT_ERR_BAD_ARG, "n / pair_capacity out of range");
    if (!project_state || !bin_state) return fail(GSPLAT_ERR_BAD_ARG, "state is NULL");
    const auto [st, vk, nl, nb, ps] = open_ctx(n, v, project_state, stream_);
    if (n_binned == 0 || n == 0) {
        HIP_TRY(hipMemsetAsync(ps.ranges, 0, nl * sizeof(uint2), st));
        LAUNCH("plan_kernel", plan_kernel, dim3(1), dim3(1024), 0, st, (int)nl, ps.ranges, ps.order, ps.class_bounds);
        return GSPLAT_OK;
    }
    BinScratch sc = carve_bin_scratch(scratch, n_binned, nb);
    if (!scratch || sc.bytes > scratch_bytes) return fail(GSPLAT_ERR_WORKSPACE, "bin scratch too small");
    uint32_t* sorted_ids = (uint32_t*)bin_state;
    LAUNCH("bin_scatter_kernel", bin_scatter_kernel, dim3((unsigned)(n_bin_blocks(n) + big_bin_blocks(n))), dim3(256), bin_lds_bytes(nb, 9 * 1024), st, n, ps.rect, ps.tiles, ps.mask, ps.depth, vk.lists_x,
           (int)nb, ps.bin_total, ps.block_off, ps.bin_start, (uint32_t)n_binned, sc.bvals, ps.rec, ps.big_flag,
           (uint32_t)n_bin_blocks(n), bin_batches(n));
    LAUNCH("split_count_kernel", split_count_kernel, dim3((unsigned)n_chunks(n_binned)), dim3(256), 0, st, (int)nb, ps.bin_start, sc.bvals,
           (uint32_t)n_binned, ps.counts, ps.list_count, sc.seg_off);
    LAUNCH("split_scatter_kernel", split_scatter_kernel, dim3((unsigned)n_chunks(n_binned) + 1u), dim3(SPLIT_THREADS), 0, st, (int)nl, (int)nb, ps.bin_start, sc.bvals,
           (uint32_t)n_binned, ps.counts, ps.list_count, sc.seg_off, ps.ranges, sc.vals, ps.order, ps.class_bounds);
    // F9 + F12: per-list sort by (depth, index); one launch per size class, grids bounded by what the class can hold
    uint64_t* vals = sc.vals;
    const auto cap = [nl = nl, n_binned](int64_t min_len) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(nl, n_binned / min_len)); };
    // lists of 4096+ entries: 100 KB of LDS per workgroup (8192+ fall back to global memory inside).  An empty launch of that kernel
    // still costs ~4 us, so it is made only where the AVERAGE list has 256 entries (lists 16x the average are the far tail: the longest
    // list of config 3 is 12x its average of 200); elsewhere the launch below takes such a list too.
    const bool class0 = n_binned >= 4096 && n_binned >= 256 * nl;
    if (class0) {
        LAUNCH("list_sort_kernel<8192>", (list_sort_kernel<1024, 8, 13, 0>), dim3(std::min(cap(4096), 256u)), dim3(1024), 0, st, ps.order, ps.class_bounds, ps.ranges,
               vals, sorted_ids, 0);
    }
    if (n_binned >= 1024) {       // lists of 1024 .. 4095 entries: 50 KB per workgroup
        LAUNCH("list_sort_kernel<4096>", (list_sort_kernel<512, 8, 12, 1>), dim3(std::min(cap(1024), 768u)), dim3(512), 0, st, ps.order, ps.class_bounds, ps.ranges,
               vals, sorted_ids, class0 ? 0 : 1);
    }
    {
        const unsigned mid_blocks = n_binned >= 256 ? std::min(cap(256), 4096u) : 0u;
        const unsigned small_blocks = std::min((cap(1) + 3u) / 4u, 16384u);
        LAUNCH("list_sort_small_kernel", list_sort_small_kernel, dim3(mid_blocks + small_blocks), dim3(256), 0, st, ps.order, ps.class_bounds, mid_blocks,
               ps.ranges, vals, sorted_ids);
    }
    return GSPLAT_OK;
}

int gsplat_rasterize_forward(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, void* bin_state,
                             float* image, float* accum, float* grad2d, void* stream_) {
    return raster_forward_impl(false, n, n_binned, v, project_state, bin_state, image, nullptr, nullptr, accum, nullptr, grad2d, nullptr, stream_);
}

int gsplat_rasterize_forward_aux(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, void* bin_state,
                                 float* image, float* depth, float* alpha, float* accum, float* accum_aux, float* grad2d,
                                 const float* background, void* stream_) {
    return raster_forward_impl(true, n, n_binned, v, project_state, bin_state, image, depth, alpha, accum, accum_aux, grad2d, background, stream_);
}

int gsplat_rasterize_backward(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, const void* bin_state,
                              const float* accum, const float* grad_image, float* grad2d, int32_t grad2d_zeroed,
                              void* det_scratch, int64_t det_scratch_bytes, void* stream_) {
    return raster_backward_entry(nullptr, false, false, n, n_binned, v, project_state, bin_state, accum, nullptr, grad_image, nullptr, nullptr, nullptr, grad2d,
                                 grad2d_zeroed, det_scratch, det_scratch_bytes, stream_);
}

int gsplat_rasterize_backward_aux(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, const void* bin_state,
                                  const float* accum, const float* accum_aux, const float* grad_image, const float* grad_depth,
                                  const float* grad_alpha, const float* background, float* grad2d, int32_t grad2d_zeroed,
                                  void* det_scratch, int64_t det_scratch_bytes, void* stream_) {
    return raster_backward_entry(nullptr, true, false, n, n_binned, v, project_state, bin_state, accum, accum_aux, grad_image, grad_depth, grad_alpha, background,
                                 grad2d, grad2d_zeroed, det_scratch, det_scratch_bytes, stream_);
}

// the _abs twins: the same arguments, the absolute-gradient sums beside the gradients; every refusal names the entry
int gsplat_rasterize_backward_abs(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, const void* bin_state,
                                  const float* accum, const float* grad_image, float* grad2d, int32_t grad2d_zeroed,
                                  void* det_scratch, int64_t det_scratch_bytes, void* stream_) {
    return raster_backward_entry("gsplat_rasterize_backward_abs", false, true, n, n_binned, v, project_state, bin_state, accum, nullptr, grad_image, nullptr, nullptr,
                                 nullptr, grad2d, grad2d_zeroed, det_scratch, det_scratch_bytes, stream_);
}

int gsplat_rasterize_backward_aux_abs(int64_t n, int64_t n_binned, const gsplat_view* v, const void* project_state, const void* bin_state,
                                      const float* accum, const float* accum_aux, const float* grad_image, const float* grad_depth,
                                      const float* grad_alpha, const float* background, float* grad2d, int32_t grad2d_zeroed,
                                      void* det_scratch, int64_t det_scratch_bytes, void* stream_) {
    return raster_backward_entry("gsplat_rasterize_backward_aux_abs", true, true, n, n_binned, v, project_state, bin_state, accum, accum_aux, grad_image, grad_depth,
                                 grad_alpha, background, grad2d, grad2d_zeroed, det_scratch, det_scratch_bytes, stream_);
}

int gsplat_project_backward(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, const void* project_state,
                            const float* grad2d, const gsplat_gaussian_grads* out, int32_t flags, void* stream_) {
    if (flags & ~(PROJECT_BACKWARD_FLAGS | BACKWARD_SH_BITS | FILTER_BITS)) return fail(GSPLAT_ERR_BAD_ARG, "unknown flag bits");
    return project_backward_impl("gsplat_project_backward", g, c2w, v, project_state, grad2d, out, flags, stream_, nullptr);
}

int gsplat_project_backward_pose(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, const void* project_state,
                                 const float* grad2d, const gsplat_gaussian_grads* out, float* grad_c2w, void* pose_scratch,
                                 int64_t pose_scratch_bytes, int32_t flags, void* stream_) {
    if (flags & ~(GSPLAT_BACKWARD_SH_JACOBIAN | GSPLAT_BACKWARD_DEPTH | BACKWARD_SH_BITS | FILTER_BITS)) return fail(GSPLAT_ERR_BAD_ARG, "unknown flag bits");
    const PoseOut pose = {grad_c2w, pose_scratch, pose_scratch_bytes};
    return project_backward_impl("gsplat_project_backward_pose", g, c2w, v, project_state, grad2d, out, flags, stream_, nullptr, &pose);
}

// ---- one call per direction (include/gsplat_mi355x.h: "composite entries"; the frame arena: gs_layout.h frame_parts) ---------
int gsplat_forward_deferred(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame, int64_t frame_bytes,
                            int64_t pair_capacity, void* counters, int64_t counters_bytes, void* bin_scratch, int64_t bin_scratch_bytes,
                            gsplat_counts* counts_host, void* counts_event, float* image, int32_t flags, void* stream_) {
    int rc = check_filter("gsplat_forward_deferred", flags);
    if (rc) return rc;
    if (!g || !v) return fail(GSPLAT_ERR_BAD_ARG, "gaussians / view is NULL");
    if ((rc = check_sh_degree("gsplat_forward_deferred", project_sh_degree(flags), g->scale_raw != nullptr))) return rc;
    if ((rc = check_view(v))) return rc;
    if (!frame || !image) return fail(GSPLAT_ERR_BAD_ARG, "frame / image is NULL");
    if (reinterpret_cast<uintptr_t>(frame) & 255u) return fail(GSPLAT_ERR_BAD_ARG, "frame must be 256-byte aligned");
    if (pair_capacity < 1) return fail(GSPLAT_ERR_BAD_ARG, "pair_capacity must be positive (a capacity kept from earlier frames)");
    const FrameParts f = frame_parts(g->n, pair_capacity, v, flags);
    if (f.total > frame_bytes) return fail(GSPLAT_ERR_WORKSPACE, "frame arena too small (gsplat_frame_bytes)");
    char* base = (char*)frame;
    const bool bwd = (flags & GSPLAT_FRAME_BACKWARD) != 0;
    const bool fused = g->scale_raw != nullptr;
    int32_t pf = GSPLAT_PROJECT_COLOUR_FUSED | GSPLAT_PROJECT_COUNTS_LATE | (counts_host ? GSPLAT_PROJECT_COUNTS_MAPPED : 0) | (flags & (PROJECT_SH_BITS | FILTER_BITS));
    if (bwd && fused && !(flags & GSPLAT_FRAME_NO_SH_JACOBIAN)) pf |= GSPLAT_PROJECT_SAVE_SH_JACOBIAN;
    if ((rc = gsplat_project(g, c2w, v, base + f.project_state, counters, counters_bytes, counts_host, counts_event, pf, stream_))) return rc;
    if ((rc = gsplat_bin(g->n, pair_capacity, v, base + f.project_state, base + f.bin_state, bin_scratch, bin_scratch_bytes, stream_))) return rc;
    float* accum = bwd ? (float*)(base + f.accum) : nullptr;
    float* grad2d = bwd && forward_clears_grad2d(g->n, v) ? (float*)(base + f.grad2d) : nullptr;
    return gsplat_rasterize_forward(g->n, pair_capacity, v, base + f.project_state, base + f.bin_state, image, accum, grad2d, stream_);
}

// (a helper inside the extern "C" block must be `static`: an anonymous namespace does not stop a function with C linkage from
//  being exported, and the product library exports nothing but the gsplat_* entry points -- tests/test_abi_cpu.py)
static int backward_impl(const char* entry, const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame, int64_t frame_bytes,
                         int64_t pair_capacity, const float* grad_image, const gsplat_gaussian_grads* out, float* grad_logit,
                         void* det_scratch, int64_t det_scratch_bytes, int32_t flags, void* stream_, const AdamRest* ar) {
    int rc = check_filter(entry, flags);
    if (rc) return rc;
    if (!g || !v) return fail(GSPLAT_ERR_BAD_ARG, "gaussians / view is NULL");
    if ((rc = check_sh_degree(entry, backward_sh_degree(flags), g->scale_raw != nullptr))) return rc;
    if ((rc = check_view(v))) return rc;
    if (!frame) return fail(GSPLAT_ERR_BAD_ARG, "frame is NULL");
    const FrameParts f = frame_parts(g->n, pair_capacity, v, GSPLAT_FRAME_BACKWARD);
    if (f.total > frame_bytes) return fail(GSPLAT_ERR_WORKSPACE, "frame arena too small: was it made with GSPLAT_FRAME_BACKWARD?");
    char* base = (char*)frame;
    if ((rc = check_filter_of(entry, base + f.project_state, flags & FILTER_BITS))) return rc;      // (before the raster phase, too)
    float* grad2d = (float*)(base + f.grad2d);
    const bool both = !(flags & (GSPLAT_BACKWARD_PHASE_RASTER | GSPLAT_BACKWARD_PHASE_PROJECT));
    if (both || (flags & GSPLAT_BACKWARD_PHASE_RASTER)) {
        if (!grad_image) return fail(GSPLAT_ERR_BAD_ARG, "grad_image is NULL");
        const int32_t zeroed = forward_clears_grad2d(g->n, v) && !(flags & GSPLAT_BACKWARD_GRAD2D_DIRTY);
        const auto raster = (flags & GSPLAT_BACKWARD_ABSGRAD) ? gsplat_rasterize_backward_abs : gsplat_rasterize_backward;
        if ((rc = raster(g->n, pair_capacity, v, base + f.project_state, base + f.bin_state, (const float*)(base + f.accum),
                         grad_image, grad2d, zeroed, det_scratch, det_scratch_bytes, stream_))) return rc;
        if (grad_logit && (rc = gsplat_logit_grad(g->n, v, base + f.project_state, grad2d, grad_logit, stream_))) return rc;
    }
    if (both || (flags & GSPLAT_BACKWARD_PHASE_PROJECT)) {
        if (!out) return fail(GSPLAT_ERR_BAD_ARG, "grads is NULL");
        if ((rc = project_backward_impl(entry, g, c2w, v, base + f.project_state, grad2d, out,
                                        flags & (GSPLAT_BACKWARD_SH_JACOBIAN | GSPLAT_BACKWARD_ACCUMULATE | BACKWARD_SH_BITS | FILTER_BITS), stream_, ar))) return rc;
    }
    return GSPLAT_OK;
}

int gsplat_backward(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame, int64_t frame_bytes,
                    int64_t pair_capacity, const float* grad_image, const gsplat_gaussian_grads* out, float* grad_logit,
                    void* det_scratch, int64_t det_scratch_bytes, int32_t flags, void* stream_) {
    if (flags & ~(BACKWARD_FLAGS | BACKWARD_SH_BITS | FILTER_BITS)) return fail(GSPLAT_ERR_BAD_ARG, "unknown flag bits");
    return backward_impl("gsplat_backward", g, c2w, v, frame, frame_bytes, pair_capacity, grad_image, out, grad_logit, det_scratch, det_scratch_bytes, flags,
                         stream_, nullptr);
}

int gsplat_backward_adam_rest(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame, int64_t frame_bytes,
                              int64_t pair_capacity, const float* grad_image, const gsplat_gaussian_grads* out, void* det_scratch,
                              int64_t det_scratch_bytes, int32_t flags, const gsplat_adam_group* f_rest, float beta1, float beta2, float eps,
                              void* stream_) {
    if (flags & ~(BACKWARD_FLAGS | BACKWARD_SH_BITS | FILTER_BITS)) return fail(GSPLAT_ERR_BAD_ARG, "unknown flag bits");
    if (int rc = check_filter("gsplat_backward_adam_rest", flags)) return rc;
    if (!g || !f_rest) return fail(GSPLAT_ERR_BAD_ARG, "gaussians / f_rest update is NULL");
    if (int rc = check_sh_degree("gsplat_backward_adam_rest", backward_sh_degree(flags), g->scale_raw != nullptr)) return rc;
    if (flags & (GSPLAT_BACKWARD_PHASE_RASTER | GSPLAT_BACKWARD_PHASE_PROJECT)) return fail(GSPLAT_ERR_BAD_ARG, "the in-place step runs the whole backward pass");
    if (f_rest->n != g->n * 45 || f_rest->step < 1 || !f_rest->param || !f_rest->exp_avg || !f_rest->exp_avg_sq || f_rest->grad_scale ||
        f_rest->param != g->f_rest)
        return fail(GSPLAT_ERR_BAD_ARG, "f_rest update: param must be the f_rest the frame was rendered from (45 n values), moments given, no grad_scale");
    if ((reinterpret_cast<uintptr_t>(f_rest->param) | reinterpret_cast<uintptr_t>(f_rest->exp_avg) | reinterpret_cast<uintptr_t>(f_rest->exp_avg_sq)) & 15u)
        return fail(GSPLAT_ERR_BAD_ARG, "f_rest update: 16-byte aligned arrays");
    const double bc1 = 1.0 - pow((double)beta1, (double)f_rest->step), bc2 = 1.0 - pow((double)beta2, (double)f_rest->step);
    const AdamRest ar = {f_rest->param, f_rest->exp_avg, f_rest->exp_avg_sq,
                         {(float)((double)f_rest->lr / bc1), (float)(1.0 / sqrt(bc2)), beta1, beta2, eps}, nullptr, (long long)pair_capacity};
    return backward_impl("gsplat_backward_adam_rest", g, c2w, v, frame, frame_bytes, pair_capacity, grad_image, out, nullptr, det_scratch, det_scratch_bytes, flags, stream_, &ar);
}

int gsplat_build_sigma(int64_t n, const float* scale_raw, const float* q_raw, float* sigma, void* stream_) {
    if (n < 0) return fail(GSPLAT_ERR_BAD_ARG, "n < 0");
    if (n == 0) return GSPLAT_OK;
    if (!scale_raw || !q_raw || !sigma) return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    LAUNCH("build_sigma_kernel", build_sigma_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream_, n, scale_raw, q_raw, sigma);
    return GSPLAT_OK;
}

int gsplat_build_sigma_backward(int64_t n, const float* scale_raw, const float* q_raw, const float* grad_sigma, float* grad_scale_raw,
                                float* grad_q_raw, void* stream_) {
    if (n < 0) return fail(GSPLAT_ERR_BAD_ARG, "n < 0");
    if (n == 0) return GSPLAT_OK;
    if (!scale_raw || !q_raw || !grad_sigma || !grad_scale_raw || !grad_q_raw) return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    LAUNCH("build_sigma_backward_kernel", build_sigma_backward_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream_, n, scale_raw, q_raw,
           grad_sigma, grad_scale_raw, grad_q_raw);
    return GSPLAT_OK;
}

int gsplat_evaluate_sh(int64_t n, const float* f_dc, const float* f_rest, const float* points, const float* c2w, float* color,
                       void* stream_) {
    if (n < 0) return fail(GSPLAT_ERR_BAD_ARG, "n < 0");
    if (n == 0) return GSPLAT_OK;
    if (!f_dc || !f_rest || !points || !c2w || !color) return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    LAUNCH("evaluate_sh_kernel", evaluate_sh_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream_, n, f_dc, f_rest, points, c2w, color);
    return GSPLAT_OK;
}

int gsplat_evaluate_sh_backward(int64_t n, const float* f_dc, const float* f_rest, const float* points, const float* c2w,
                                const float* grad_color, float* grad_f_dc, float* grad_f_rest, float* grad_points, void* stream_) {
    if (n < 0) return fail(GSPLAT_ERR_BAD_ARG, "n < 0");
    if (n == 0) return GSPLAT_OK;
    if (!f_dc || !f_rest || !points || !c2w || !grad_color || !grad_f_dc || !grad_f_rest || !grad_points)
        return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    if (!aligned16(f_dc) || !aligned16(f_rest) || !aligned16(points) || !aligned16(grad_color) || !aligned16(grad_f_dc) ||
        !aligned16(grad_f_rest) || !aligned16(grad_points))
        return fail(GSPLAT_ERR_BAD_ARG, "arrays must be 16-byte aligned");
    LAUNCH("evaluate_sh_backward_kernel", evaluate_sh_backward_kernel, dim3(blocks64(n)), dim3(64), 0, (hipStream_t)stream_, n, f_dc, f_rest, points, c2w,
           grad_color, grad_f_dc, grad_f_rest, grad_points);
    return GSPLAT_OK;
}

int gsplat_logit_grad(int64_t n, const gsplat_view* v, const void* project_state, const float* grad2d, float* grad_logit, void* stream_) {
    int rc = check_view(v);
    if (rc) return rc;
    if (n < 0) return fail(GSPLAT_ERR_BAD_ARG, "n < 0");
    if (n == 0) return GSPLAT_OK;
    if (!project_state || !grad2d || !grad_logit) return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    const Ctx c = open_ctx(n, v, project_state, stream_);
    LAUNCH("logit_grad_kernel", logit_grad_kernel, dim3(blocks256(n)), dim3(256), 0, c.st, n, c.ps.tiles, c.ps.rec, grad2d, grad_logit);
    return GSPLAT_OK;
}

int gsplat_sh_accumulate(int64_t n, int32_t n_views, const float* pos, const float* eyes, const float* grad_logit, float scale,
                         float* grad_f_dc, float* grad_f_rest, void* stream_) {
    return gsplat_sh_accumulate_degree(n, n_views, pos, eyes, grad_logit, scale, grad_f_dc, grad_f_rest, 3, stream_);
}

int gsplat_sh_accumulate_degree(int64_t n, int32_t n_views, const float* pos, const float* eyes, const float* grad_logit, float scale,
                                float* grad_f_dc, float* grad_f_rest, int32_t sh_degree, void* stream_) {
    if (sh_degree < 0 || sh_degree > 3) return fail(GSPLAT_ERR_BAD_ARG, "gsplat_sh_accumulate_degree: sh_degree must be 0, 1, 2 or 3");
    if (n < 0 || n_views < 0) return fail(GSPLAT_ERR_BAD_ARG, "n / n_views < 0");
    if (n == 0) return GSPLAT_OK;
    if (!pos || !grad_f_dc || !grad_f_rest || (n_views > 0 && (!eyes || !grad_logit))) return fail(GSPLAT_ERR_BAD_ARG, "NULL argument");
    if (!aligned16(pos) || !aligned16(grad_f_dc) || !aligned16(grad_f_rest)) return fail(GSPLAT_ERR_BAD_ARG, "arrays must be 16-byte aligned");
    const auto kernel = with_sh_bases(sh_degree, [](auto nb) { return sh_accumulate_kernel<decltype(nb)::value>; });
    LAUNCH("sh_accumulate_kernel", kernel, dim3(blocks64(n)), dim3(64), 0, (hipStream_t)stream_, n, (int)n_views, pos, eyes, grad_logit,
           scale, grad_f_dc, grad_f_rest);
    return GSPLAT_OK;
}

// ---- screen-space densification statistics (include/gsplat_mi355x.h; the kernels: gs_densify.h) ------------------------------
int gsplat_densify_stats(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const float* grad2d,
                         float* stats, void* stream_) {
    return densify_stats_impl("gsplat_densify_stats", n, pair_capacity, v, project_state, grad2d, stats, stream_);
}

int gsplat_densify_stats_abs(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const float* grad2d,
                             float* stats, void* stream_) {
    return densify_stats_impl("gsplat_densify_stats_abs", n, pair_capacity, v, project_state, grad2d, stats, stream_, true);
}

static int frame_densify_stats_impl(const char* name, int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes,
                                    float* stats, void* stream_, bool abs) {
    FrameParts f;
    if (int rc = open_frame(name, n, pair_capacity, v, frame, frame_bytes, stats, GSPLAT_FRAME_BACKWARD, ": was it made with GSPLAT_FRAME_BACKWARD?", &f)) return rc;
    const char* base = (const char*)frame;
    return densify_stats_impl(name, n, pair_capacity, v, base + f.project_state, (const float*)(base + f.grad2d), stats, stream_, abs);
}

int gsplat_frame_densify_stats(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes,
                               float* stats, void* stream_) {
    return frame_densify_stats_impl("gsplat_frame_densify_stats", n, pair_capacity, v, frame, frame_bytes, stats, stream_, false);
}

int gsplat_frame_densify_stats_abs(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes,
                                   float* stats, void* stream_) {
    return frame_densify_stats_impl("gsplat_frame_densify_stats_abs", n, pair_capacity, v, frame, frame_bytes, stats, stream_, true);
}

int gsplat_densify_stats_merge(int64_t n, float* pass, float* total, void* stream_) {
    const char* name = "gsplat_densify_stats_merge";
    if (n < 0) return fail(GSPLAT_ERR_BAD_ARG, "%s: n < 0", name);
    if (!pass || !total) return fail(GSPLAT_ERR_BAD_ARG, "%s: NULL argument", name);
    if (pass == total) return fail(GSPLAT_ERR_BAD_ARG, "%s: pass and total are the same record", name);
    if (!aligned16(pass) || !aligned16(total)) return fail(GSPLAT_ERR_BAD_ARG, "%s: records must be 16-byte aligned", name);
    if (n == 0) return GSPLAT_OK;
    LAUNCH("densify_stats_merge_kernel", densify_stats_merge_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream_, n, reinterpret_cast<f4*>(pass),
           reinterpret_cast<f4*>(total));
    return GSPLAT_OK;
}

// ---- the visible set of a frame (include/gsplat_mi355x.h; the kernel: gs_visible.h) -----------------------------------------------
int gsplat_visible_set(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, uint8_t* visible, void* stream_) {
    return visible_set_impl("gsplat_visible_set", n, pair_capacity, v, project_state, visible, stream_);
}

int gsplat_frame_visible_set(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes,
                             uint8_t* visible, void* stream_) {
    const char* name = "gsplat_frame_visible_set";
    FrameParts f;         // (flags 0: project_state lies at the same offset with and without GSPLAT_FRAME_BACKWARD)
    if (int rc = open_frame(name, n, pair_capacity, v, frame, frame_bytes, visible, 0, " (gsplat_frame_bytes)", &f)) return rc;
    return visible_set_impl(name, n, pair_capacity, v, (const char*)frame + f.project_state, visible, stream_);
}

// ---- per-Gaussian contribution statistics (include/gsplat_mi355x.h; the kernel: gs_contrib.h) ----------------------------------
int gsplat_contribution(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const void* bin_state,
                        uint32_t* record, void* stream_) {
    return contribution_impl("gsplat_contribution", n, pair_capacity, v, project_state, bin_state, record, stream_);
}

int gsplat_frame_contribution(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes,
                              uint32_t* record, void* stream_) {
    const char* name = "gsplat_frame_contribution";
    FrameParts f;         // (flags 0: project_state | bin_state lie at the same offsets with and without GSPLAT_FRAME_BACKWARD)
    if (int rc = open_frame(name, n, pair_capacity, v, frame, frame_bytes, record, 0, " (gsplat_frame_bytes)", &f)) return rc;
    const char* base = (const char*)frame;
    return contribution_impl(name, n, pair_capacity, v, base + f.project_state, base + f.bin_state, record, stream_);
}

// ---- per-Gaussian feature vectors (include/gsplat_mi355x.h; the kernels: gs_features.h) -----------------------------------------
int gsplat_features_forward(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const void* bin_state,
                            const float* features, int channels, float* out, void* stream_) {
    return features_impl("gsplat_features_forward", false, n, pair_capacity, v, project_state, bin_state, features, channels, out, stream_);
}

int gsplat_features_adjoint(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, const void* bin_state,
                            const float* grad_out, int channels, float* grad_features, void* stream_) {
    return features_impl("gsplat_features_adjoint", true, n, pair_capacity, v, project_state, bin_state, grad_out, channels, grad_features, stream_);
}

}  // extern "C"
