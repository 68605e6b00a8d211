/*
 * gsplat_mi355x.h -- C ABI of the MI355X-native differentiable Gaussian-splat rasterizer.
 *
 * Drop-in boundary for the hot path of ashu1069/3D-Gaussian-Splatting-for-Novel-View-Synthesis.
 * The reference has no FFI of its own: its boundary is three Python functions in the
 * `gaussian_splatting` namespace (reference gaussian_splatting/__init__.py:7-21).  This header is
 * what a binding for those three functions links against; INTEGRATION.md shows the ctypes stub.
 *
 *   reference function (file:line)                               replaced by
 *   ------------------------------------------------------------ --------------------------------------
 *   render()                  gaussian_splatting/render.py:62    gsplat_project + gsplat_bin +
 *                                                                gsplat_rasterize_forward (+ the two
 *                                                                *_backward calls for autograd)
 *   build_sigma_from_params() gaussian_splatting/gaussian.py:71  gsplat_build_sigma[_backward], or folded
 *                                                                into gsplat_project (fused inputs)
 *   evaluate_sh()   gaussian_splatting/spherical_harmonics.py:70 gsplat_evaluate_sh[_backward], or folded
 *                                                                into gsplat_project (fused inputs)
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; `stream` is a hipStream_t passed as void*.
 *   - every pointer is a DEVICE pointer to fp32 data in the reference's own tensor layout
 *     (pos[N,3], f_rest[N,45] channel-major, sigma[N,3,3], image[H,W,3] ...), except where a
 *     parameter name ends in `_host`.
 *   - the library never allocates or frees memory the caller can see: inputs, outputs, state kept
 *     for the backward pass and scratch are caller-owned (PyTorch tensors in the Python host).
 *     `*_bytes()` functions give the sizes; the internal carving is private to the library.
 *   - every call is stream-ordered and returns immediately (no host synchronisation inside).
 *   - return value: GSPLAT_OK or a GSPLAT_ERR_* code; gsplat_last_error() gives the text
 *     (thread-local).
 */
#ifndef GSPLAT_MI355X_H
#define GSPLAT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSPLAT_ABI_VERSION 12

/* call status */
#define GSPLAT_OK 0
#define GSPLAT_ERR_BAD_ARG 1     /* null pointer, negative size, unsupported tile size ...          */
#define GSPLAT_ERR_HIP 2         /* a HIP runtime call or kernel launch failed                      */
#define GSPLAT_ERR_WORKSPACE 3   /* caller-provided state / scratch buffer too small                */

/* scene status, from gsplat_classify_counts(): mirrors the reference's empty / error conventions   */
#define GSPLAT_SCENE_OK 0
#define GSPLAT_SCENE_ALL_CULLED 10     /* render.py:109-112,139-142,182-193,206-209 -> zero image   */
#define GSPLAT_SCENE_ALL_OFFSCREEN 11  /* render.py:235-236 -> Exception("All projected points ...") */

/* Per-view scalars: the intrinsics and the 8 keyword arguments of render() (render.py:62-64).      */
typedef struct gsplat_view {
    int32_t H, W;                 /* image size                                                      */
    float fx, fy, cx, cy;         /* pinhole intrinsics (pixels)                                     */
    float near_z, far_z;          /* near=0.01, far=100.0                                            */
    float pix_guard;              /* 32                                                              */
    int32_t tile;                 /* T=16; any T >= 1 (it sets the reference's tile rectangles = the
                                     reported pair count; the image does not depend on it)            */
    float min_conis;              /* 1e-6                                                            */
    float chi_square_clip;        /* 6.25                                                            */
    float alpha_max;              /* 0.99                                                            */
    float alpha_cutoff;           /* 1/128                                                           */
} gsplat_view;

/* Gaussian parameters of one scene.  Exactly one of the two input sets is given:
 *   un-fused (the reference render() signature): color + sigma, the four fused pointers NULL;
 *   fused (build_sigma_from_params + evaluate_sh folded in): scale_raw, q_raw, f_dc, f_rest,
 *          color and sigma NULL.                                                                    */
typedef struct gsplat_gaussians {
    int64_t n;
    const float* pos;           /* [n,3]                                                             */
    const float* opacity_raw;   /* [n]                                                               */
    const float* color;         /* [n,3]   or NULL                                                   */
    const float* sigma;         /* [n,3,3] or NULL                                                   */
    const float* scale_raw;     /* [n,3]   or NULL   (log scale)                                     */
    const float* q_raw;         /* [n,4]   or NULL   (x,y,z,w), un-normalised                        */
    const float* f_dc;          /* [n,3]   or NULL                                                   */
    const float* f_rest;        /* [n,45]  or NULL   channel-major R1..R15,G1..G15,B1..B15           */
} gsplat_gaussians;

/* Gradient outputs, same shapes as the inputs of gsplat_gaussians; unused ones NULL.
 * Every row is written (rows of culled Gaussians get zeros, as in the reference).                    */
typedef struct gsplat_gaussian_grads {
    float* pos;
    float* opacity_raw;
    float* color;
    float* sigma;
    float* scale_raw;
    float* q_raw;
    float* f_dc;
    float* f_rest;
} gsplat_gaussian_grads;

/* Counters produced by gsplat_project (copied to pinned host memory when asked).                    */
typedef struct gsplat_counts {
    int32_t n_survivors;   /* pass the opacity prefilter, frustum cull and finite check              */
    int32_t n_visible;     /* ... and have an on-screen AABB  (V of SURVEY.md)                       */
    int64_t n_pairs;       /* the reference's (tile, Gaussian) pairs, F11  (P of SURVEY.md)          */
    int32_t max_tiles_per_gaussian;   /* of the binned rectangles                                    */
    int32_t reserved;
    int64_t n_binned;      /* (list, Gaussian) pairs actually binned: the ellipse of each Gaussian over
                              16 x 8-pixel lists; sizes the gsplat_bin buffers                        */
} gsplat_counts;

int gsplat_abi_version(void);
const char* gsplat_last_error(void);
int gsplat_classify_counts(const gsplat_counts* counts_host);

/* ---- buffer sizes (bytes) ---------------------------------------------------------------------- */
int64_t gsplat_project_state_bytes(int64_t n, const gsplat_view* v);    /* kept until the backward pass */
int64_t gsplat_project_scratch_bytes(int64_t n);     /* persistent counter block of gsplat_project: see there         */
int64_t gsplat_bin_state_bytes(int64_t pair_capacity, const gsplat_view* v);   /* kept until the backward pass   */
int64_t gsplat_bin_scratch_bytes(int64_t pair_capacity, const gsplat_view* v); /* free after gsplat_bin          */

/* ---- layout queries: FOR TESTS AND TOOLS ONLY ---------------------------------------------------
 * Where the arrays a test wants to look at lie inside project_state / bin_state (byte offsets from the start of the buffer).
 * Pure host functions, nothing is launched.  NOT a stable contract: the carving stays private to the library, the offsets
 * and the set of arrays may change with any version; a product host never needs them.
 *   rec           [n][16] floats: u, v, A11, A12 | A22, opacity, ex, ey | r, g, b, depth | the row-span constants
 *   rect          [n][2] uint32: x0 | y0 << 16, x1 | y1 << 16 -- inclusive rectangle of 16 x 8-pixel lists
 *   depth [n] float, tiles [n] uint32 (lists the Gaussian is binned to; 0 = culled), mask [n] uint32 (bit k = list k of the
 *                 rectangle, row-major; all ones for rectangles of more than 32 lists)
 *   ranges        [lists][2] uint32 start, end in sorted_ids; order [lists] uint32; class_bounds [8] uint32; kj [n][12] floats
 *   counts        the device copy of gsplat_counts
 *   sorted_ids    [pair_capacity] uint32; pair_mask [pair_capacity] bytes (written by gsplat_rasterize_forward with `accum`)
 * Return GSPLAT_OK, or GSPLAT_ERR_BAD_ARG (NULL view / out, non-positive image size, negative n or pair_capacity).          */
typedef struct gsplat_state_layout {
    int64_t bytes;                /* = gsplat_project_state_bytes(n, v)                                  */
    int64_t lists;                /* lists_x * lists_y                                                   */
    int32_t lists_x, lists_y;
    int64_t counts, rec, rect, depth, tiles, mask, ranges, order, class_bounds, kj;
} gsplat_state_layout;
typedef struct gsplat_bin_layout {
    int64_t bytes;                /* = gsplat_bin_state_bytes(pair_capacity, v)                          */
    int64_t sorted_ids, pair_mask;
} gsplat_bin_layout;
int gsplat_project_state_layout(int64_t n, const gsplat_view* v, gsplat_state_layout* out);
int gsplat_bin_state_layout(int64_t pair_capacity, const gsplat_view* v, gsplat_bin_layout* out);

/* ---- forward ----------------------------------------------------------------------------------- */
/* F1-F8, F10, F13 (+F2, F3 when fused): per-Gaussian projection, culls, EWA covariance, eigen clamp,
 * conic, rectangle and mask of 16 x 8-pixel lists, colour; counts the (list, Gaussian) pairs in total and
 * per coarse bin.  At most 2^26 Gaussians per call.  c2w is the DEVICE [4,4] row-major camera-to-world matrix (no
 * host read -> no synchronisation).
 *   scratch        gsplat_project_scratch_bytes() bytes, 64-byte aligned: a block of counters that must be ZERO when
 *                  the call starts.  Zero it once after allocating it; every call leaves it zeroed again (the last wave
 *                  of the projection kernel adds the counters up and clears them: no clearing or totals kernel).  One
 *                  block per stream; calls sharing a block must be stream-ordered.
 *   counts_host    (nullable) receives the counters: by hipMemcpyAsync on `stream`, or -- flag
 *                  GSPLAT_PROJECT_COUNTS_MAPPED: it is device-accessible pinned host memory (hipHostMalloc) -- stored by
 *                  the kernel itself (one stream operation less).
 *   counts_event   (hipEvent_t, nullable) recorded right behind the counters: a caller that wants exact buffer sizes
 *                  waits for it (not for the stream: the first binning kernel and, without COLOUR_FUSED, the SH colour
 *                  pass are queued BEHIND the event and run during the host's round trip) and reads n_binned.
 *   flags          GSPLAT_PROJECT_COLOUR_FUSED: evaluate the SH colour inside the projection kernel (one pass over the
 *                  inputs: best when the host does NOT wait for the counters -- see gsplat_bin's pair_capacity).
 *                  GSPLAT_PROJECT_SAVE_SH_JACOBIAN (fused inputs; set it when a backward pass will follow): the colour pass
 *                  also leaves, per visible Gaussian, d colour / d logit and d logit / d position (48 bytes) in
 *                  project_state, so that gsplat_project_backward (flag GSPLAT_BACKWARD_SH_JACOBIAN) does not read the
 *                  192 bytes of SH coefficients again.  Ignored for un-fused inputs.
 *                  GSPLAT_PROJECT_COUNTS_LATE (for callers that do NOT wait for the counters in the middle of the forward
 *                  pass): the counters -- device copy, counts_host, counts_event -- are produced by the first binning kernel
 *                  instead of by the projection kernel's last wave; the projection's waves then retire without waiting
 *                  for their stores.  Everything queued after this call sees them as before.                           */
#define GSPLAT_PROJECT_COLOUR_FUSED 1
#define GSPLAT_PROJECT_COUNTS_MAPPED 2
#define GSPLAT_PROJECT_SAVE_SH_JACOBIAN 4
#define GSPLAT_PROJECT_COUNTS_LATE 8
/* The SH degree of a fused render, 0..3 (bits 4-5 hold the bands dropped, 3 - degree, so flags without them mean degree 3, as
 * before there was a degree): the colour is sigmoid(sum_{k < (d+1)^2} f_k Y_k).  f_rest stays [n,45] channel-major; the ACTIVE
 * entries of a row are the columns ch * 15 + j with j < (d+1)^2 - 1 (0, 3, 8 or 15 per channel).  Inactive entries are ignored:
 * their values, NaN included, change no output bit, and the image equals the degree-3 image of the same scene with zeros there.
 * Degree 0 does not read f_rest at all.  A degree below 3 with un-fused inputs (color + sigma) is GSPLAT_ERR_BAD_ARG.  Every
 * backward call on the state must be given the SAME degree (GSPLAT_BACKWARD_SH_DEGREE): the saved SH Jacobian holds the active
 * bands only.  gsplat_forward_deferred takes the degree in the same bits of ITS flags (GSPLAT_FRAME_SH_DEGREE).              */
#define GSPLAT_PROJECT_SH_DEGREE(d) ((3 - (d)) << 4)
/* The screen-space low-pass of the paper's rasteriser, in the SAME bits of the flags of the six entries that run the
 * projection math: gsplat_project, gsplat_forward_deferred, gsplat_project_backward[_pose], gsplat_backward,
 * gsplat_backward_adam_rest.  The eigen clamp is applied to Sigma + s I instead of the projected covariance Sigma; radius,
 * rectangles, pair counts, conic and masks follow.  GSPLAT_FILTER_LOWPASS(c): s = c / 100 px^2, c = 0..255 (bits 17-24; 0 = no
 * filter, today's render bit for bit).  GSPLAT_FILTER_ANTIALIAS (needs c > 0, else GSPLAT_ERR_BAD_ARG): the opacity in the record is
 * clamp(sigmoid(o), 0, 0.999) * sqrt(max(det Sigma, 0) / det(Sigma + s I)), both determinants before the clamp; the opacity pre-filter
 * stays on the unscaled value.  Every backward call must carry the bits of the forward call that filled project_state / the frame:
 * other bits are refused with GSPLAT_ERR_BAD_ARG before anything is launched (the library remembers, on the host, the bits each
 * state was last projected with).  Any other entry refuses the bits as unknown flags; the size queries ignore them.              */
#define GSPLAT_FILTER_ANTIALIAS 65536
#define GSPLAT_FILTER_LOWPASS(c) ((c) << 17)
int gsplat_project(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* project_state,
                   void* scratch, int64_t scratch_bytes, gsplat_counts* counts_host, void* counts_event, int32_t flags,
                   void* stream);

/* F9, F11, F12: every Gaussian is appended to the lists of its rectangle (two-level counting sort),
 * the lists get their [start, end) and a longest-first launch order, and every list is sorted; the
 * order inside a list is (camera depth, Gaussian index) ascending.  The rendered image does not
 * depend on the binning granularity, only on that order.
 *   pair_capacity  pairs the bin_state / scratch buffers were sized for (gsplat_bin_*_bytes).  The number of pairs
 *                  really binned is read on the DEVICE (the counters gsplat_project left in project_state), so the
 *                  host may pass the exact n_binned it waited for, or -- without ever synchronising -- a capacity kept
 *                  from earlier frames.  If the frame has more pairs than that, nothing is written out of bounds, the
 *                  frame's image and gradients are garbage, and the caller finds n_binned > pair_capacity in the
 *                  counters whenever it reads them: it then renders the frame again with larger buffers.
 *                  At most 2^32 - 1 pairs; images up to 8192 coarse bins (64 lists each: 8192 x 8192 pixels).
 *                  ONE gsplat_bin per gsplat_project: it adds to per-list counters in project_state that only gsplat_project
 *                  clears (a frame rendered again with larger buffers is projected again).                             */
int gsplat_bin(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, void* bin_state,
               void* scratch, int64_t scratch_bytes, void* stream);

/* F14, F15: per-tile front-to-back compositing.  image[H,W,3] receives clamp(C,0,1); accum[H,W,3]
 * (nullable; required for the backward pass) receives the unclamped C.  grad2d (nullable, [n,16]
 * floats): cleared here for the coming gsplat_rasterize_backward (pass grad2d_zeroed = 1 there), which
 * saves that call a 64-byte-per-Gaussian fill; only worth it when n / lists is small (<= 256).
 * pair_capacity must be the value gsplat_bin was given.  With `accum` (a backward pass will follow) the call
 * also leaves one byte per pair in bin_state -- which 4 x 4-pixel sub-tiles of its list the Gaussian's ellipse
 * reaches, by the exact test -- and gsplat_rasterize_backward composites from those.                    */
int gsplat_rasterize_forward(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                             void* bin_state, float* image, float* accum, float* grad2d, void* stream);

/* The same compositing with a depth map, an opacity map and a background (no counterpart in the reference).  With
 * w_i = alpha_i T_i [T_i > 5e-5] (the reference's alpha, T and alive rule) a pixel gets
 *     C = sum w_i c_i,   A = sum w_i,   D = sum w_i z_i      (z_i = camera-space depth of Gaussian i)
 *     image = clamp(C + (1 - A) bg, 0, 1),   depth = D,   alpha = A     (D and A neither clamped nor normalised: the expected
 *                                                                        depth is D / A, formed by the caller)
 *   depth, alpha   [H,W] each, nullable (a background alone).
 *   accum, accum_aux  both or neither; for gsplat_rasterize_backward_aux: accum[H,W,3] = C as above, accum_aux[H,W,2] = (D, A).
 *   background     3 floats in HOST memory, read during the call; NULL = none (the image is gsplat_rasterize_forward's).
 * Everything else as for gsplat_rasterize_forward.                                                                        */
int gsplat_rasterize_forward_aux(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                                 void* bin_state, float* image, float* depth, float* alpha, float* accum, float* accum_aux,
                                 float* grad2d, const float* background, void* stream);

/* ---- backward ---------------------------------------------------------------------------------- */
/* B1: gradient of the compositing w.r.t. the per-Gaussian 2D quantities.  grad2d is [n,16] floats, private to the
 * library (moments of dL/dq over the pixels for the centre and the conic, then opacity, r, g, b, padding); it is zeroed
 * by this call before accumulation (unless grad2d_zeroed: gsplat_rasterize_forward already cleared it) and consumed
 * by gsplat_project_backward.
 *   det_scratch    NULL: the per-(list, Gaussian) sums are added into grad2d with float atomics (fastest; the order of the
 *                  additions, hence the last bits of the gradients, varies from run to run).  Not NULL
 *                  (gsplat_rasterize_backward_scratch_bytes(n, pair_capacity) bytes): DETERMINISTIC mode -- the sums are
 *                  stored per pair and added per Gaussian in a fixed order: gradients are bitwise reproducible.            */
int64_t gsplat_rasterize_backward_scratch_bytes(int64_t n, int64_t pair_capacity);
int gsplat_rasterize_backward(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                              const void* bin_state, const float* accum, const float* grad_image,
                              float* grad2d, int32_t grad2d_zeroed, void* det_scratch, int64_t det_scratch_bytes,
                              void* stream);

/* B1 behind gsplat_rasterize_forward_aux: upstream gradients of the image, the depth map and the opacity map ([H,W,3], [H,W],
 * [H,W]; a NULL one means zeros, all three NULL is GSPLAT_ERR_BAD_ARG).  (z, 1) are two more colour channels: with
 * c+ = (r, g, b, z, 1) and G+ = (G_r, G_g, G_b, G_D, G_A - sum_c G_c bg_c), G_c masked by the clamp of C + (1 - A) bg,
 *     d alpha_i = alive_i T_i (c+_i . G+) - (sum_{k>i} w_k c+_k . G+) / (1 - alpha_i).
 * grad2d gets one column more: column 9 = dL/dz_i = sum over the pixels of w_i G_D, which gsplat_project_backward[_pose] adds to
 * the camera-space depth gradient when given GSPLAT_BACKWARD_DEPTH.  `background` as in the forward call (the same values).
 * Deterministic mode as for gsplat_rasterize_backward, with a scratch of gsplat_rasterize_backward_aux_scratch_bytes (rows of 10). */
int64_t gsplat_rasterize_backward_aux_scratch_bytes(int64_t n, int64_t pair_capacity);
int gsplat_rasterize_backward_aux(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                                  const void* bin_state, const float* accum, const float* accum_aux, const float* grad_image,
                                  const float* grad_depth, const float* grad_alpha, const float* background, float* grad2d,
                                  int32_t grad2d_zeroed, void* det_scratch, int64_t det_scratch_bytes, void* stream);

/* The absolute-gradient twins (AbsGS, gsplat's absgrad): the arguments, the gradients and the deterministic mode of
 * gsplat_rasterize_backward / gsplat_rasterize_backward_aux -- columns 0-8 (0-9) of grad2d are theirs, bit for bit in deterministic
 * mode -- and, per Gaussian, two sums more over all pixels p of all its lists.  With a_p = dL/dalpha exp(-q/2) (zero unless the pixel
 * is alive, alpha passed its tests and o g <= alpha_max: the quantity whose moments columns 0-5 hold), du = px - u, dv = py - v:
 *     column 10 = Sx = sum_p |a_p (A11 du + A12 dv)|        column 11 = Sy = sum_p |a_p (A12 du + A22 dv)|
 * in BOTH variants: o Sx, o Sy are the per-pixel |dL/du|, |dL/dv| of the projected centre added without their signs, where columns
 * 0-1 let them cancel.  Column 9 stays dL/dz behind the aux entry and is otherwise left as gsplat_rasterize_backward leaves it.
 * gsplat_densify_stats_abs reads the two columns.  The scratch of the deterministic mode has rows of 11 and 12 floats: its own size
 * queries.  GSPLAT_ERR_BAD_ARG (the text names the entry): a NULL view or required pointer, a bad view, n or pair_capacity out of
 * range.  n == 0: GSPLAT_OK, no kernel is launched.                                                                             */
int64_t gsplat_rasterize_backward_abs_scratch_bytes(int64_t n, int64_t pair_capacity);
int64_t gsplat_rasterize_backward_aux_abs_scratch_bytes(int64_t n, int64_t pair_capacity);
int gsplat_rasterize_backward_abs(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                                  const void* bin_state, const float* accum, const float* grad_image, float* grad2d,
                                  int32_t grad2d_zeroed, void* det_scratch, int64_t det_scratch_bytes, void* stream);
int gsplat_rasterize_backward_aux_abs(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                                      const void* bin_state, const float* accum, const float* accum_aux, const float* grad_image,
                                      const float* grad_depth, const float* grad_alpha, const float* background, float* grad2d,
                                      int32_t grad2d_zeroed, void* det_scratch, int64_t det_scratch_bytes, void* stream);

/* B2 (+B3 when fused): chain the 2D gradients back to the inputs of gsplat_project.
 * Factored form (fused inputs; out->f_dc and out->f_rest NULL): instead of the 48 SH-coefficient
 * gradients per Gaussian, out->color[n,3] (if given) receives the gradient w.r.t. the colour LOGIT (the sigmoid's argument,
 * spherical_harmonics.py:166); gsplat_sh_accumulate turns logit gradients of any number of views into SH gradients.
 *   flags          GSPLAT_BACKWARD_SH_JACOBIAN: project_state was filled by gsplat_project with
 *                  GSPLAT_PROJECT_SAVE_SH_JACOBIAN for the SAME g and c2w (same results up to fp32 rounding, 144 bytes
 *                  less HBM traffic per visible Gaussian).  Without the flag the SH coefficients are read again.
 *                  GSPLAT_BACKWARD_DEPTH: grad2d comes from gsplat_rasterize_backward_aux -- its column 9 holds dL/dz of the
 *                  Gaussian's camera-space depth, which joins the position (and pose) gradient.  Not with ACCUMULATE.
 *                  Also GSPLAT_BACKWARD_ACCUMULATE (below); any other bit is refused with GSPLAT_ERR_BAD_ARG.             */
#define GSPLAT_BACKWARD_SH_JACOBIAN 1
#define GSPLAT_BACKWARD_DEPTH 64
/* The SH degree of the forward call that filled project_state / the frame (bits 8-9 hold 3 - degree; without them: degree 3).
 * It MUST be that call's degree, in every backward entry: gsplat_project_backward[_pose], gsplat_backward,
 * gsplat_backward_adam_rest.  The gradient of every inactive f_rest entry is then an exact zero (every row is still written;
 * with GSPLAT_BACKWARD_ACCUMULATE at degree 0 the f_rest gradient is not touched), d colour / d pos carries the active bands only,
 * and the in-place step of gsplat_backward_adam_rest steps the inactive entries with a zero gradient, as gsplat_adam_step would.
 * A degree below 3 with un-fused inputs is GSPLAT_ERR_BAD_ARG (the text names the entry).                                     */
#define GSPLAT_BACKWARD_SH_DEGREE(d) ((3 - (d)) << 8)
int gsplat_project_backward(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v,
                            const void* project_state, const float* grad2d, const gsplat_gaussian_grads* out,
                            int32_t flags, void* stream);

/* gsplat_project_backward plus the gradient w.r.t. the camera pose: grad_c2w[16] (device, row-major 4 x 4) receives dL/dc2w of
 * the same grad2d (render.py:122,156-159 and spherical_harmonics.py:132 differentiated w.r.t. c2w; its last row is 0).
 *   out            as for gsplat_project_backward: all gradients of the inputs, or -- fused inputs, f_dc and f_rest NULL -- the
 *                  factored form (the colour-logit gradients into out->color if given, no SH gradients: a pose frame inside a
 *                  factored exchange); or NULL: the pose gradient only.
 *   pose_scratch   gsplat_pose_scratch_bytes(n) bytes, 64-byte aligned, caller-owned; nothing needs clearing.
 *   flags          GSPLAT_BACKWARD_SH_JACOBIAN and GSPLAT_BACKWARD_DEPTH; any other bit is refused with GSPLAT_ERR_BAD_ARG.
 * The per-Gaussian terms are added in a fixed order, without atomics: the same inputs give the same bits.  NULL grad_c2w is
 * GSPLAT_ERR_BAD_ARG, a scratch below the size GSPLAT_ERR_WORKSPACE.                                                       */
int64_t gsplat_pose_scratch_bytes(int64_t n);
int gsplat_project_backward_pose(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v,
                                 const void* project_state, const float* grad2d, const gsplat_gaussian_grads* out,
                                 float* grad_c2w, void* pose_scratch, int64_t pose_scratch_bytes, int32_t flags,
                                 void* stream);

/* ---- composite entries: one call per direction ----------------------------------------------------------------------
 * For a host that does not wait for the counters in the middle of the forward pass (a training loop, a frame sequence:
 * the pair buffers are sized from a capacity kept from earlier frames, see gsplat_bin) the forward pass is three library
 * calls and five caller-owned buffers, the backward pass two or three calls; on a Python host every call and every
 * allocation is several microseconds, and the whole step is ~0.5 ms of GPU time.  These two entries queue exactly the same
 * kernels from ONE call each, on ONE caller-owned arena:
 *
 *   frame arena   gsplat_frame_bytes(n, pair_capacity, v, flags) bytes, 256-byte aligned: project_state | bin_state, and with
 *                 GSPLAT_FRAME_BACKWARD also accum [H,W,3] | grad2d [n,16]; kept until the backward pass, private to the library.
 *   gsplat_forward_deferred = gsplat_project(COLOUR_FUSED | COUNTS_LATE | COUNTS_MAPPED if counts_host | SAVE_SH_JACOBIAN if
 *                 GSPLAT_FRAME_BACKWARD and fused inputs) + gsplat_bin + gsplat_rasterize_forward.  `counters` is
 *                 gsplat_project's persistent counter block, `bin_scratch` gsplat_bin's scratch (gsplat_bin_scratch_bytes);
 *                 counts_host (nullable) must be device-mapped pinned memory; counts_event (nullable) is recorded behind the
 *                 counters.  The caller reads counts_host when it likes (n_binned > pair_capacity: the frame is garbage, render
 *                 it again with larger buffers; survivors but nothing visible: the reference's off-screen exception).
 *   gsplat_backward = gsplat_rasterize_backward [+ gsplat_logit_grad if grad_logit] + gsplat_project_backward on the same
 *                 arena.  flags: GSPLAT_BACKWARD_SH_JACOBIAN as for gsplat_project_backward (set it iff the frame was made
 *                 with GSPLAT_FRAME_BACKWARD from fused inputs without GSPLAT_FRAME_NO_SH_JACOBIAN);
 *                 GSPLAT_BACKWARD_PHASE_RASTER / _PROJECT: only that half (a data-parallel host starts exchanging grad_logit
 *                 between the two); GSPLAT_BACKWARD_GRAD2D_DIRTY: a second backward pass through the same frame;
 *                 GSPLAT_BACKWARD_ACCUMULATE (below).  Any other bit is refused with GSPLAT_ERR_BAD_ARG, GSPLAT_BACKWARD_DEPTH
 *                 included: a depth / opacity frame takes the separate calls.                                               */
#define GSPLAT_FRAME_BACKWARD 1
#define GSPLAT_FRAME_NO_SH_JACOBIAN 2
#define GSPLAT_FRAME_SH_DEGREE(d) ((3 - (d)) << 4)    /* gsplat_forward_deferred: as GSPLAT_PROJECT_SH_DEGREE; not a gsplat_frame_bytes flag */
#define GSPLAT_BACKWARD_PHASE_RASTER 2
#define GSPLAT_BACKWARD_PHASE_PROJECT 4
#define GSPLAT_BACKWARD_GRAD2D_DIRTY 8
/* the gradients are ADDED to what `out` holds (the views of one iteration summed by the projection backward itself; the caller
 * clears or writes the arrays with the first view).  Fused inputs with GSPLAT_BACKWARD_SH_JACOBIAN, all six gradients given.  */
#define GSPLAT_BACKWARD_ACCUMULATE 16
/* gsplat_backward / gsplat_backward_adam_rest: the raster phase is gsplat_rasterize_backward_abs (its deterministic scratch then
 * has gsplat_rasterize_backward_abs_scratch_bytes), so that gsplat_frame_densify_stats_abs may follow.  Accepted and ignored where
 * only GSPLAT_BACKWARD_PHASE_PROJECT runs; an unknown bit to gsplat_project_backward[_pose].                                   */
#define GSPLAT_BACKWARD_ABSGRAD 128
int64_t gsplat_frame_bytes(int64_t n, int64_t pair_capacity, const gsplat_view* v, int32_t flags);
int gsplat_forward_deferred(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame,
                            int64_t frame_bytes, int64_t pair_capacity, void* counters, int64_t counters_bytes,
                            void* bin_scratch, int64_t bin_scratch_bytes, gsplat_counts* counts_host, void* counts_event,
                            float* image, int32_t flags, void* stream);
int gsplat_backward(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame, int64_t frame_bytes,
                    int64_t pair_capacity, const float* grad_image, const gsplat_gaussian_grads* out, float* grad_logit,
                    void* det_scratch, int64_t det_scratch_bytes, int32_t flags, void* stream);

/* Data-parallel exchange helper: per view the SH-coefficient gradient is the outer product of the 3
 * colour-logit gradients with the 16 SH basis values of the view direction, so ranks exchange 12 B per Gaussian and view
 * instead of 192 B per Gaussian and rebuild the sum here:
 *   grad_f_dc[i,ch] = scale * sum_v grad_logit[v,i,ch] * Y_0,  grad_f_rest[i, ch*15 + k-1] = scale * sum_v grad_logit[v,i,ch] * Y_k(d_v(i))
 * pos[n,3]; eyes[n_views,3] = camera positions (c2w[:3,3]) on the DEVICE; grad_logit[n_views,n,3].                        */
int gsplat_sh_accumulate(int64_t n, int32_t n_views, const float* pos, const float* eyes, const float* grad_logit,
                         float scale, float* grad_f_dc, float* grad_f_rest, void* stream);
/* The same for views rendered at SH degree sh_degree (0..3, else GSPLAT_ERR_BAD_ARG): the inactive columns of grad_f_rest are
 * written as zeros.  gsplat_sh_accumulate is this with sh_degree = 3.                                                          */
int gsplat_sh_accumulate_degree(int64_t n, int32_t n_views, const float* pos, const float* eyes, const float* grad_logit,
                                float scale, float* grad_f_dc, float* grad_f_rest, int32_t sh_degree, void* stream);
/* The same colour-logit gradients [n,3] straight from gsplat_rasterize_backward's grad2d (and the colours kept in
 * project_state), without waiting for gsplat_project_backward: the exchange of the logit gradients can overlap it.
 * (In the factored form of gsplat_project_backward out->color may then be NULL.)                                      */
int gsplat_logit_grad(int64_t n, const gsplat_view* v, const void* project_state, const float* grad2d,
                      float* grad_logit, void* stream);

/* ---- screen-space densification statistics (no counterpart in the reference) -----------------------------
 * A record is [n,4] floats, 16-byte aligned, one row per Gaussian: (grad_sum, count, extent_max, 0).  Behind the raster backward of
 * ONE frame, every Gaussian binned into at least one list of that frame ("visible") adds, with the frame's own record
 * (u, v, A11, A12, A22, opacity o, ex, ey) and the moments (Mx, My) in columns 0-1 of grad2d,
 *     g_u = o (A11 Mx + A12 My),  g_v = o (A12 Mx + A22 My)        (the gradient of the projected centre, pixels)
 *     grad_sum += sqrt((g_u W/2)^2 + (g_v H/2)^2)                  (NDC units)
 *     count    += 1
 *     extent_max = max(extent_max, min(max(ex, ey), 250))          (half-extents of {q <= chi_square_clip}, pixels)
 * Rows of Gaussians that are not visible are not touched.  A frame with nothing on screen, or one whose pairs outgrew
 * pair_capacity (n_binned > pair_capacity in its device counters: its grad2d is garbage), adds nothing -- decided on the device,
 * as in gsplat_backward_adam_rest.
 *   gsplat_densify_stats        after gsplat_rasterize_backward[_aux] on the same project_state and grad2d.
 *   gsplat_frame_densify_stats  the same on the arena of gsplat_forward_deferred built with GSPLAT_FRAME_BACKWARD, after the raster
 *                               phase of gsplat_backward / gsplat_backward_adam_rest (before or after the projection phase).
 *   gsplat_densify_stats_merge  total (+)= pass -- (sum, sum, max) -- for the rows with pass.count > 0, which are then written back
 *                               as zeros: a pass record is zero again after a merge.  pass != total.
 * ORDERING: the accumulation is a plain read-modify-write without atomics.  Calls that add into (or merge) the same record must
 * be ordered on one stream, or by events between streams.
 * GSPLAT_ERR_BAD_ARG (the text names the entry): a NULL pointer, n < 0, pair_capacity < 0, a record that is not 16-byte aligned,
 * frame_bytes below gsplat_frame_bytes(n, pair_capacity, v, GSPLAT_FRAME_BACKWARD).  n == 0: GSPLAT_OK, nothing is launched.        */
int gsplat_densify_stats(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                         const float* grad2d, float* stats, void* stream);
int gsplat_frame_densify_stats(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame,
                               int64_t frame_bytes, float* stats, void* stream);
int gsplat_densify_stats_merge(int64_t n, float* pass, float* total, void* stream);
/* The absolute-gradient statistic: the same record, rules, guards and errors, but
 *     grad_sum += sqrt((o Sx W/2)^2 + (o Sy H/2)^2)        (Sx, Sy) = columns 10-11 of grad2d
 * so grad2d / the frame must come from gsplat_rasterize_backward[_aux]_abs, or from gsplat_backward / gsplat_backward_adam_rest
 * with GSPLAT_BACKWARD_ABSGRAD (behind the plain entries the two columns hold zeros or stale values).  count and extent_max are
 * what the plain entries add; records of the two kinds merge with gsplat_densify_stats_merge alike.                               */
int gsplat_densify_stats_abs(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                             const float* grad2d, float* stats, void* stream);
int gsplat_frame_densify_stats_abs(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame,
                                   int64_t frame_bytes, float* stats, void* stream);

/* ---- the visible set of a frame (not in the reference) -----------------------------------------------------
 * One byte per Gaussian: behind ONE frame, visible[i] = 1 for every Gaussian binned into at least one list of that frame -- the
 * rows gsplat_densify_stats counts, and the only rows of the frame that can have a non-zero gradient.  The record is never read
 * and 0 is never stored, so frames on different streams may add into one record with NO ordering between them (every store
 * writes the same value); the caller zeroes it.  A frame with nothing on screen, or one whose pairs outgrew pair_capacity, adds
 * nothing -- decided on the device, as in gsplat_densify_stats.
 *   gsplat_visible_set        on the project_state of gsplat_project + gsplat_bin.
 *   gsplat_frame_visible_set  the same on the arena of gsplat_forward_deferred (with or without GSPLAT_FRAME_BACKWARD).
 * GSPLAT_ERR_BAD_ARG (the text names the entry): a NULL pointer, n < 0, pair_capacity < 0, frame_bytes below
 * gsplat_frame_bytes(n, pair_capacity, v, 0).  n == 0: GSPLAT_OK, nothing is launched.                                            */
int gsplat_visible_set(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state, uint8_t* visible,
                       void* stream);
int gsplat_frame_visible_set(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame, int64_t frame_bytes,
                             uint8_t* visible, void* stream);

/* ---- per-Gaussian contribution statistics (not in the reference) ------------------------------------------------------------
 * How much does each Gaussian take part in the composite?  With the blending weight w_i(p) = alpha_i T_i [T_i > 5e-5] of Gaussian i
 * at pixel p, exactly as the forward rasteriser forms it, one frame adds to row i of `record`, over all pixels of all lists the
 * Gaussian is binned into,
 *     weight_sum += sum_p w_i(p)      weight_max = max(weight_max, max_p w_i(p))      pixels += #{p : w_i(p) > 0}.
 * A record is [n,4] 32-bit words, 16-byte aligned, one row per Gaussian, every word an order-independent integer:
 *     words 0-1  uint64 sum_q (little endian) in units of 2^-32: every (list, Gaussian) pair adds round_to_nearest(pair_sum * 2^32),
 *                pair_sum = the float32 sum of w over the pair's <= 128 pixels (< 2^7: 2^25 such terms fit)
 *     word 2     the float32 bits of weight_max (non-negative: an unsigned integer maximum)
 *     word 3     uint32 pixels; wraps after 2^32 pixel hits (not guarded)
 * The kernel adds with integer atomics, so the record is bitwise the same whatever the order of waves, streams, frames or ranks:
 * calls on different streams may add into one record at the same time.  The caller zeroes a new record.  Rows of Gaussians in no
 * list are not touched, and a pair without a pixel of w > 0 (everything behind an opaque surface) issues no memory operation.  A frame
 * with nothing on screen, or one whose pairs outgrew pair_capacity (n_binned > pair_capacity in its device counters: its lists are
 * garbage), adds nothing -- decided on the device, as in gsplat_densify_stats.  No image is written and no colour is read.
 *   gsplat_contribution        after gsplat_bin on the same project_state / bin_state and pair_capacity; no raster call is needed.
 *   gsplat_frame_contribution  the same on the arena of gsplat_forward_deferred (with or without GSPLAT_FRAME_BACKWARD).
 * GSPLAT_ERR_BAD_ARG (the text names the entry): a NULL pointer, n < 0, pair_capacity < 0, a record that is not 16-byte aligned,
 * frame_bytes below gsplat_frame_bytes(n, pair_capacity, v, 0).  n == 0: GSPLAT_OK, nothing is launched.                            */
int gsplat_contribution(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                        const void* bin_state, uint32_t* record, void* stream);
int gsplat_frame_contribution(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* frame,
                              int64_t frame_bytes, uint32_t* record, void* stream);

/* ---- per-Gaussian feature vectors: N-channel maps and their adjoint (not in the reference) ----------------------------------
 * With the blending weight w_i(p) = alpha_i T_i [T_i > 5e-5] of Gaussian i at pixel p, exactly as the forward rasteriser forms it,
 * and a table features [n, channels] (float32, row i = Gaussian i, rows contiguous):
 *   gsplat_features_forward   out[p, c] = sum_i w_i(p) features[i, c].  out is [H, W, channels] float32, channel last; every pixel
 *                             and channel is written, zeros where nothing reaches the pixel: the caller clears nothing.  Neither
 *                             clamped nor normalised; a channel of ones renders the opacity map.
 *   gsplat_features_adjoint   grad_features[i, c] += sum_p w_i(p) grad_out[p, c]: the gradient with respect to the table, and the
 *                             closed-form lift of a 2D map [H, W, channels] onto the Gaussians.  It ADDS, with float atomics (the sums
 *                             differ in their last bits from run to run; there is no deterministic variant): the caller zeroes the
 *                             table, or accumulates over views.  A zero is never added: the row of a Gaussian in no list, or whose
 *                             weights are all zero (everything behind an opaque surface), is not touched.
 * Both run after gsplat_bin on the same project_state / bin_state and pair_capacity; no raster call is needed.  The records' colours
 * are not read.  A table of C channels costs ceil(C / 8) traversals of the lists.  A frame with nothing on screen, or one whose pairs
 * outgrew pair_capacity (n_binned > pair_capacity in its device counters: its lists are garbage), writes and adds nothing -- decided
 * on the device, as in gsplat_contribution.  No array needs more than float alignment; 16-byte aligned arrays of a channel count
 * divisible by 4 move in 16-byte pieces.
 * GSPLAT_ERR_BAD_ARG (the text begins with the entry's name and a colon): a NULL pointer, n < 0, pair_capacity < 0, channels outside
 * 1 .. GSPLAT_FEATURES_MAX_CHANNELS, a bad view.  n == 0: GSPLAT_OK, nothing is launched.                                         */
#define GSPLAT_FEATURES_MAX_CHANNELS 512
int gsplat_features_forward(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                            const void* bin_state, const float* features, int channels, float* out, void* stream);
int gsplat_features_adjoint(int64_t n, int64_t pair_capacity, const gsplat_view* v, const void* project_state,
                            const void* bin_state, const float* grad_out, int channels, float* grad_features, void* stream);

/* ---- the two small exported functions as stand-alone ops --------------------------------------- */
int gsplat_build_sigma(int64_t n, const float* scale_raw, const float* q_raw, float* sigma, void* stream);
int gsplat_build_sigma_backward(int64_t n, const float* scale_raw, const float* q_raw, const float* grad_sigma,
                                float* grad_scale_raw, float* grad_q_raw, void* stream);
int gsplat_evaluate_sh(int64_t n, const float* f_dc, const float* f_rest, const float* points, const float* c2w,
                       float* color, void* stream);
int gsplat_evaluate_sh_backward(int64_t n, const float* f_dc, const float* f_rest, const float* points,
                                const float* c2w, const float* grad_color, float* grad_f_dc, float* grad_f_rest,
                                float* grad_points, void* stream);

/* ---- next row of the path: the training loss ------------------------------------
 * compute_loss() of the reference (gaussian_splatting/losses.py:158-185; l1_loss :27, ssim_loss :44,
 * 11 x 11 Gaussian window, sigma 1.5, zero padding): lambda_l1 * mean|pred - target| + lambda_ssim * (1 - SSIM).
 * pred/target/grad_pred are [batch, H, W, 3] fp32 device arrays.  values[3] (device) receives (l1, 1 - ssim, total);
 * grad_pred (nullable) receives d total / d pred.  scratch: gsplat_loss_scratch_bytes(batch, H, W, grad_pred != NULL) device
 * bytes (the partial sums, and -- with a gradient -- the three partial-derivative maps of the SSIM term, 36 B per value).   */
int64_t gsplat_loss_scratch_bytes(int64_t batch, int32_t H, int32_t W, int32_t with_grad);
int gsplat_loss(const float* pred, const float* target, int64_t batch, int32_t H, int32_t W, float lambda_l1,
                float lambda_ssim, float* values, float* grad_pred, void* scratch, void* stream);
/* The same loss as two calls, for a caller whose graph supplies d L / d total later (an autograd node).  gsplat_loss_forward:
 * values[3] = scale * (l1, 1 - ssim, total), *total (nullable, device) = values[2]; with keep_maps the partial-derivative maps stay in
 * scratch (sized with_grad = 1) for gsplat_loss_backward, which writes grad_pred = scale * (*upstream) * d total / d pred
 * (upstream: device scalar, NULL = 1) -- the upstream factor is multiplied in by the kernel, not by a pass over the gradient.  */
int gsplat_loss_forward(const float* pred, const float* target, int64_t batch, int32_t H, int32_t W, float lambda_l1,
                        float lambda_ssim, float scale, float* values, float* total, void* scratch, int32_t keep_maps, void* stream);
int gsplat_loss_backward(const float* pred, const float* target, int64_t batch, int32_t H, int32_t W, float lambda_l1,
                         float lambda_ssim, float scale, const float* upstream, float* grad_pred, void* scratch, void* stream);

/* ---- training with a background, an opacity target and depth maps ----------------------------------------
 * The auxiliary loss on the maps of an aux render.  depth = D, alpha = A of the render, target_depth = Z (camera-space z, the unit
 * of D; a pixel counts iff Z is finite and > 0), target_alpha = M: [batch, H, W] fp32 device arrays.  With n = batch H W,
 * v = [Z valid], n_v = max(1, sum v):
 *   L_alpha = sum |A - M| / n,   L_depth = sum v |D - A Z| / n_v,   values[3] = scale * (L_alpha, L_depth, lambda_alpha L_alpha +
 *   lambda_depth L_depth),   *total (nullable) = values[2].
 * A NULL target switches its term off (value 0); depth may be NULL when target_depth is.  The sums (the count of valid pixels
 * included) are one partial per workgroup added in a fixed order in double: no atomics, the same bits every call.  The forward
 * leaves n_v in scratch for the backward, which writes
 *   grad_depth = scale up lambda_depth v sign(D - A Z) / n_v                                  (nullable when target_depth is NULL)
 *   grad_alpha = scale up (lambda_alpha sign(A - M) / n - lambda_depth v Z sign(D - A Z) / n_v),        sign(0) = 0,
 * up = *upstream (device scalar, NULL = 1), multiplied in by the kernel.  scratch: the bytes the size query returns (256 + 12
 * per 1024 pixels, rounded up to 256).  batch <= 65535, as for the image loss.                                                */
int64_t gsplat_aux_loss_scratch_bytes(int64_t batch, int32_t H, int32_t W);
int gsplat_aux_loss_forward(const float* depth, const float* alpha, const float* target_depth, const float* target_alpha, int64_t batch,
                            int32_t H, int32_t W, float lambda_depth, float lambda_alpha, float scale, float* values, float* total,
                            void* scratch, void* stream);
int gsplat_aux_loss_backward(const float* depth, const float* alpha, const float* target_depth, const float* target_alpha, int64_t batch,
                             int32_t H, int32_t W, float lambda_depth, float lambda_alpha, float scale, const float* upstream,
                             float* grad_depth, float* grad_alpha, void* scratch, void* stream);
/* A target image over a background: out = rgb * alpha + (1 - alpha) * background.  rgb [batch, H, W, 3] is straight colour (not
 * pre-multiplied), alpha [batch, H, W], background: 3 HOST floats read during the call; inputs in [0, 1], nothing is clamped.   */
int gsplat_composite_target(const float* rgb, const float* alpha, const float* background, int64_t batch, int32_t H, int32_t W,
                            float* out, void* stream);

/* ---- next row 2: the optimiser step of scripts/train.py:394-401, 536-538 ---------------------
 * gsplat_clip_grad_norm = torch.nn.utils.clip_grad_norm_ on one tensor: coef_and_norm[2] (device) receives
 * (min(1, max_norm / (||grad|| + 1e-6)), ||grad||); nothing is scaled yet and nothing is read back to the host.
 * gsplat_adam_step = one torch.optim.Adam update (amsgrad off, no weight decay) of one flat fp32 tensor at 1-based
 * `step`; if grad_scale (device scalar, e.g. the clip coefficient) is given the gradient is multiplied by it in place
 * first, exactly like clip_grad_norm_ followed by optimizer.step().                                                  */
int64_t gsplat_clip_scratch_bytes(void);
int gsplat_clip_grad_norm(int64_t n, const float* grad, float max_norm, float* coef_and_norm, void* scratch, void* stream);
int gsplat_adam_step(int64_t n, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, int32_t step, const float* grad_scale, void* stream);
/* The same update for up to 8 tensors in ONE launch (the six parameter groups of scripts/train.py:394-401): group k is
 * gsplat_adam_step(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale) with its own lr / step.          */
typedef struct gsplat_adam_group {
    int64_t n;
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float lr;
    int32_t step;
    const float* grad_scale;      /* nullable device scalar */
} gsplat_adam_group;
int gsplat_adam_step_multi(int32_t n_groups, const gsplat_adam_group* groups, float beta1, float beta2, float eps, void* stream);
/* The sparse step: group k is n_rows rows of row_width[k] >= 1 values (groups[k].n == n_rows * row_width[k]),
 * and only the rows whose byte of `visible` (device, n_rows bytes) is non-zero are stepped -- exactly as gsplat_adam_step_multi
 * steps them, with the tensor's own `step` in the bias corrections and the clip coefficient where the group has one.  A row whose
 * byte is zero keeps param, grad, exp_avg and exp_avg_sq bit for bit, whatever they hold (NaN included).  With every byte non-zero
 * the result is bit-identical to gsplat_adam_step_multi.  Up to 8 groups in one launch.  GSPLAT_ERR_BAD_ARG, before any launch:
 * more than 8 groups, a NULL `visible` or `row_width`, a width < 1, n != n_rows * width, and what gsplat_adam_step_multi refuses.  */
int gsplat_adam_step_rows(int32_t n_groups, const gsplat_adam_group* groups, const int32_t* row_width, int64_t n_rows,
                          const uint8_t* visible, float beta1, float beta2, float eps, void* stream);

/* gsplat_backward with the Adam step of f_rest folded into the projection backward: the 45 SH gradients of a Gaussian (192 of the 236
 * gradient bytes) are applied to f_rest as they are formed -- they are neither written nor read again by the optimiser.  For an
 * iteration of ONE view (gradients of several views must be added up before a step): f_rest->param must be the f_rest the frame
 * was rendered from, f_rest->n = 45 n, no grad_scale; out->f_rest is not written (may be NULL); every other gradient as in
 * gsplat_backward.  Needs fused inputs and GSPLAT_BACKWARD_SH_JACOBIAN (a frame queued without GSPLAT_FRAME_NO_SH_JACOBIAN); both
 * phases run.  The same arithmetic, instruction for instruction, as gsplat_adam_step on the gradient gsplat_backward would write.
 * A frame whose pairs outgrew pair_capacity (n_binned > pair_capacity: its gradients are garbage, the caller renders it again) or
 * that has nothing on screen steps NOTHING: the kernel reads the frame's device counters itself; the caller, once it has read them
 * too, knows which of the two happened (and must not count the step).                                                          */
int gsplat_backward_adam_rest(const gsplat_gaussians* g, const float* c2w, const gsplat_view* v, void* frame, int64_t frame_bytes,
                              int64_t pair_capacity, const float* grad_image, const gsplat_gaussian_grads* out, void* det_scratch,
                              int64_t det_scratch_bytes, int32_t flags, const gsplat_adam_group* f_rest, float beta1, float beta2,
                              float eps, void* stream);

/* ---- density control at a fixed budget: MCMC relocation, position noise, regularisers (not in the reference) ----
 * Random numbers are Philox4x32-10 with key = the two halves of `seed` and counter = (row low, row high, iteration, stream), stream 0
 * for the noise and 1 for the relocation: a function of its arguments alone, the same bits on every rank.  n < 2^31 everywhere.
 *
 * Noise: pos_i += Sigma_i (z_i scale g_i), Sigma the covariance the projection builds from (scale_raw, q_raw), z three
 *   Box-Muller normals of the row, g = 1 / (1 + exp(100 sigmoid(opacity_raw) - 0.5)); a row whose g is 0 is not written.
 * Regularise: values[3] (device) = (L_o, L_s, *base + L_o + L_s) with L_o = lambda_opacity mean sigmoid(opacity_raw), L_s =
 *   lambda_scale mean exp(scale_raw), base a nullable device scalar; d L_o / d opacity_raw and d L_s / d scale_raw are ADDED to the
 *   two gradient arrays (each nullable: values only).  One partial sum per workgroup, added in index order in double: the same
 *   bits every call.  ONE launch.
 * Refine: row i is dead iff sigmoid(opacity_raw_i) <= min_opacity; a live row weighs max(1, floor(sigmoid 2^24)).  Every dead row draws
 *   a source in proportion to the weights (an exclusive uint64 prefix sum and a binary search: exact, order-free), becomes a bit copy
 *   of its pos, f_dc, f_rest, q_raw, and source and copies get the opacity and the scale that leave the rendered image unchanged
 *   (n = min(draws + 1, 51) Gaussians in place of one).  moments (nullable, and each parameter's pair nullable): the two Adam moments
 *   of every parameter, zeroed on the rows that changed.  Six launches, nothing waits on the host or on another workgroup.
 * scratch: gsplat_mcmc_scratch_bytes(n) device bytes, 256-byte aligned, shared by the regulariser and the refinement (they use
 *   different parts).  The first 256 bytes (the regulariser's arrival counter) must be ZERO before the first call; every call leaves
 *   them zero.  The layout query (tests and tools only, no stable contract) gives the byte offsets of the refinement's arrays:
 *   w uint32[n], prefix uint64[n], src int32[n] (-1: drew nothing), count int32[n], total uint64, and the two constants of the scan.  */
typedef struct gsplat_mcmc_moments {       /* [0] = exp_avg, [1] = exp_avg_sq */
    float* pos[2];
    float* f_dc[2];
    float* f_rest[2];
    float* opacity_raw[2];
    float* scale_raw[2];
    float* q_raw[2];
} gsplat_mcmc_moments;
typedef struct gsplat_mcmc_layout {
    int64_t bytes, reg, w, prefix, src, count, total, block_sums;
    int32_t scan_block;       /* rows per workgroup of the scan */
    int32_t scan_chunk;       /* block sums one pass of the middle kernel holds */
} gsplat_mcmc_layout;
int64_t gsplat_mcmc_scratch_bytes(int64_t n);
int gsplat_mcmc_scratch_layout(int64_t n, gsplat_mcmc_layout* out);
int gsplat_mcmc_noise(int64_t n, float* pos, const float* opacity_raw, const float* scale_raw, const float* q_raw, float scale,
                      uint64_t seed, uint32_t iteration, void* stream);
int gsplat_mcmc_regularise(int64_t n, const float* opacity_raw, const float* scale_raw, float* grad_opacity_raw, float* grad_scale_raw,
                           float lambda_opacity, float lambda_scale, const float* base, float* values, void* scratch, void* stream);
int gsplat_mcmc_refine(float* pos, float* f_dc, float* f_rest, float* opacity_raw, float* scale_raw, float* q_raw,
                       const gsplat_mcmc_moments* moments, int64_t n, float min_opacity, uint64_t seed, uint32_t iteration, void* scratch,
                       void* stream);

/* ---- the Mip-Splatting 3D smoothing filter (not in the reference) -------------------------------------------------
 * Every entry runs on the caller's stream, reads nothing back and allocates nothing.  n < 2^31.
 *
 * Compute: filt[k] = sqrt(s) t_k, the standard deviation in world units of the low-pass that Gaussian k is convolved with.
 *   t_k = min over the cameras that SEE k of z / max(fx, fy), with (x, y, z) = R^T (p_k - t) of the camera's c2w = [R | t]; a camera
 *   sees k iff z > near, -margin W <= fx x / z + cx <= (1 + margin) W and -margin H <= fy y / z + cy <= (1 + margin) H.  A NaN or
 *   infinite position is seen by nobody.  A Gaussian nobody sees gets the largest t of the seen ones; with n_cams == 0 (filt is
 *   zeroed; pos, cams and scratch may be NULL) or nobody seen at all, every filt[k] = 0.  Minimum and maximum are taken on the
 *   integer bits of the floats: the same bits every call, on any stream.
 *   cams: n_cams records of GSPLAT_FILTER3D_CAMERA_FLOATS floats on the device:
 *     [0..11] c2w[:3, :4] row-major   [12] fx  [13] fy  [14] cx  [15] cy  [16] W  [17] H  [18..23] padding, not read
 *   (they are staged through LDS GSPLAT_FILTER3D_CAMERA_CHUNK at a time).  A camera whose fx or fy is not a positive finite number
 *   sees nothing.  scratch: gsplat_filter3d_scratch_bytes(n) device bytes, 256-byte aligned, any contents; one call at a time per
 *   scratch buffer.  Two launches behind a 4-byte memset node.
 * Apply, in raw-parameter space, with s_j = max(exp(scale_raw_j), 1e-6) (the render's activation), sigma = sigmoid(opacity_raw), f = filt[k]:
 *     scale_out_j = log sqrt(s_j^2 + f^2),   c = sqrt(prod s_j^2 / prod (s_j^2 + f^2)),   opacity_out = logit(c sigma)
 *   -- rendering (scale_out, opacity_out) renders the Gaussian convolved with an isotropic Gaussian of variance f^2, its peak rescaled
 *   so that its integral is kept.  (The render's own clamp of the opacity at 0.999 then acts on c sigma.)  A row with f == 0 is
 *   copied bit for bit.  scale arrays are [n, 3], the others [n]; no output may alias an input.
 * Apply backward: g_scale_raw, g_opacity_raw = the vector-Jacobian product of (g_scale_out, g_opacity_out), c and sigma recomputed
 *   from the inputs; zero through an active 1e-6 clamp; filt gets no gradient.  accumulate != 0: ADDED to the destinations.
 * Arrays 4-byte aligned.  One launch each.                                                                                       */
#define GSPLAT_FILTER3D_CAMERA_FLOATS 24
#define GSPLAT_FILTER3D_CAMERA_CHUNK 64
int64_t gsplat_filter3d_scratch_bytes(int64_t n);
int gsplat_filter3d_compute(int64_t n, const float* pos, int32_t n_cams, const float* cams, float near, float margin, float s, float* filt,
                            void* scratch, void* stream);
int gsplat_filter3d_apply(int64_t n, const float* scale_raw, const float* opacity_raw, const float* filt, float* scale_out, float* opacity_out,
                          void* stream);
int gsplat_filter3d_apply_backward(int64_t n, const float* scale_raw, const float* opacity_raw, const float* filt, const float* g_scale_out,
                                   const float* g_opacity_out, float* g_scale_raw, float* g_opacity_raw, int32_t accumulate, void* stream);

/* ---- per-view exposure compensation (not in the reference) ---------------------------------------------------------
 * An affine colour transform per image, E = [M | t], twelve floats row-major 3 x 4, applied to a frame before the loss:
 *     o_r = fma(M_r0, c_0, fma(M_r1, c_1, fma(M_r2, c_2, t_r)))      (no clamp; the identity returns every finite c bit for bit)
 * image, out, grad_out, grad_image: [batch, H, W, 3] floats; params: [batch, 12].  Every entry runs on the caller's stream, reads
 * nothing back and allocates nothing.  H, W, batch > 0 and batch <= 65535, else GSPLAT_ERR_BAD_ARG (gsplat_exposure_scratch_bytes: -1),
 * as for a NULL required pointer -- before anything is launched.  Arrays 4-byte aligned; 16-byte aligned ones are read 16 bytes at a
 * time, with the same bits.  No output may alias an input.
 * Forward: one launch.
 * Backward: grad_image[k] = sum_r M_rk grad_out[r] per pixel (grad_image == NULL: not computed), and
 *     grad_params[r, k] = sum over the pixels of grad_out[r] c_k (k < 3),  grad_params[r, 3] = sum over the pixels of grad_out[r]
 *   (grad_params == NULL: not computed; scratch may then be NULL).  The sums are formed in a fixed order without float atomics -- per
 *   thread, per wave, per workgroup in fp32, over the workgroups in double -- so they are the same bits on every call, stream and launch.
 *   The twelve floats of image b go to row b of grad_params, or to row row_index[b] when row_index (batch int32 on the device; a
 *   negative entry drops the row) is given; the rows named must be distinct.  flags: GSPLAT_EXPOSURE_ACCUMULATE adds to the
 *   destination rows instead of overwriting them; any other bit is refused first ("unknown flag").
 *   scratch: gsplat_exposure_scratch_bytes(batch, H, W) device bytes, any contents; one call at a time per scratch buffer.
 *   One launch, two with grad_params.                                                                                             */
#define GSPLAT_EXPOSURE_ACCUMULATE 1
int64_t gsplat_exposure_scratch_bytes(int64_t batch, int32_t H, int32_t W);
int gsplat_exposure_forward(const float* image, const float* params, int64_t batch, int32_t H, int32_t W, float* out, void* stream);
int gsplat_exposure_backward(const float* image, const float* params, const float* grad_out, int64_t batch, int32_t H, int32_t W,
                             float* grad_image, float* grad_params, const int32_t* row_index, int32_t flags, void* scratch, void* stream);

/* ---- per-view bilateral grids (not in the reference) ----------------------------------------------------------------
 * A grid of affine colour transforms per image, G[12, L, Y, X] floats (channel 4 r + k = entry (r, k) of [M | t]), sliced at
 * (pixel x, pixel y, pixel luminance) with trilinear weights and applied to a frame before the loss (csrc/gs_bilagrid.h has the
 * formulas; the identity grid returns every finite colour bit for bit).  image, out, grad_out, grad_image: [batch, H, W, 3] floats;
 * grids: [batch, 12, L, Y, X].  2 <= X, Y <= 64 and 2 <= L <= 16; 0 < H, W <= 2^20, H W < 2^31, 0 < batch <= 65535; else GSPLAT_ERR_BAD_ARG (the
 * scratch size: -1), as for a NULL required pointer -- before anything is launched.  Every entry runs on the caller's stream, reads
 * nothing back and allocates nothing.  Arrays 4-byte aligned.  No output may alias an input.  No float atomics: every result is the
 * same bits on every call, stream and launch.
 * Forward: one launch.
 * Backward: grad_image (NULL: not computed) is one launch over the pixels; grad_grids (NULL: not computed) is one launch of one
 *   workgroup per spatial vertex and image, which gathers the pixels of the vertex's support and owns its 12 L outputs -- no scratch.
 *   The grid of image b goes to row b of grad_grids ([V, 12, L, Y, X]), or to row row_index[b] when row_index (batch int32 on the
 *   device; a negative entry drops the image) is given; the rows named must be distinct.  flags: GSPLAT_BILAGRID_ACCUMULATE adds to
 *   the destination rows instead of overwriting them; any other bit is refused first ("unknown flag").
 * Total variation of a table grids[V, 12, L, Y, X]:  tv = (1 / V) sum_v sum_axis mean((G shifted by one along the axis - G)^2), the
 *   axes L, Y, X, the mean over the 12 channels and all pairs along the axis.  loss_out (one float, NULL: not computed) = scale tv;
 *   grad (NULL: not computed) = scale dtv/dG, or += with GSPLAT_BILAGRID_ACCUMULATE: every element gathers from its at most six
 *   neighbours.  scratch: gsplat_bilagrid_tv_scratch_bytes(V, X, Y, L) device bytes, 8-byte aligned, any contents, needed for loss_out
 *   only (one double per workgroup -- V 12 planes of ceil(L Y X / 256) -- added in a fixed order by a second launch); one call at a time per
 *   scratch buffer.                                                                                                              */
#define GSPLAT_BILAGRID_ACCUMULATE 1
int gsplat_bilagrid_forward(const float* image, const float* grids, int64_t batch, int32_t H, int32_t W, int32_t X, int32_t Y, int32_t L,
                            float* out, void* stream);
int gsplat_bilagrid_backward(const float* image, const float* grids, const float* grad_out, int64_t batch, int32_t H, int32_t W, int32_t X,
                             int32_t Y, int32_t L, float* grad_image, float* grad_grids, const int32_t* row_index, int32_t flags, void* stream);
int64_t gsplat_bilagrid_tv_scratch_bytes(int64_t V, int32_t X, int32_t Y, int32_t L);
int gsplat_bilagrid_tv(const float* grids, int64_t V, int32_t X, int32_t Y, int32_t L, float scale, float* loss_out, float* grad, int32_t flags,
                       void* scratch, void* stream);

/* ---- image quality metrics of held-out views (not in the reference) -------------------------------------------------
 * Per image b of pred, target [B, H, W, 3] floats over the valid pixels of mask [B, H, W] bytes (nonzero = valid; NULL: every pixel):
 *     l1 = sum |x - y| / (3 n),  mse = sum (x - y)^2 / (3 n),  psnr = -10 log10(mse) (+inf for mse == 0),
 *     ssim = the SSIM map of gsplat_loss (computed from the whole images: the mask does not alter the window statistics) averaged over
 *     the valid pixels and the three channels;  n == 0: NaN in all four (and in the affine), no other image is affected.
 * out: [B, 4] = psnr, ssim, l1, mse.  GSPLAT_METRICS_COLOUR_CORRECT: first the affine [M | t] (twelve floats row-major 3 x 4, the layout of
 * gsplat_exposure_forward's params) minimising sum_valid |M x + t - y|^2 with a ridge of 1e-8 n toward the identity is fitted per image
 * and written to affine [B, 12]; the metrics are then those of clamp(M x + t, 0, 1) against y (the SSIM window's zero padding is of
 * the corrected image).  Without the flag nothing is clamped and affine may be NULL.  gsplat_metrics_fit_affine runs the fit alone.
 * B, H, W >= 1, B <= 65535, H <= 16 x 65535, H W < 2^38, else GSPLAT_ERR_BAD_ARG (the scratch size: -1), as for a NULL required pointer, an unknown flag
 * bit or the flag with a NULL affine -- before anything is launched.  Every entry runs on the caller's stream, reads nothing back and
 * allocates nothing.  No float atomics: every sum is formed in a fixed order (per thread, wave, workgroup and over the workgroups of
 * an image, in double from the first term on -- the SSIM values themselves are fp32 --; pixel counts in integers), so the values are the same
 * bits on every call, stream and launch, and an image gets in a batch the bits it gets alone.
 * scratch: gsplat_metrics_scratch_bytes(B, H, W, flags) device bytes, 8-byte aligned, any contents (the fit alone: the size with the
 * flag); one call at a time per scratch buffer.  Two launches, four with the flag (the fit alone: two).                             */
#define GSPLAT_METRICS_COLOUR_CORRECT 1
int64_t gsplat_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t flags);
int gsplat_metrics_fit_affine(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, float* affine,
                              void* scratch, void* stream);
int gsplat_metrics_forward(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                           float* affine, float* out, void* scratch, void* stream);

/* ---- scale initialisation: exact 3-nearest-neighbour mean squared distance (not in the reference) --------------------
 * dist2[i] = the mean of the m = min(3, F - 1) smallest d2(i, j) over the FINITE rows j != i of points [n, 3] (F = their number):
 * what the paper, simple_knn's distCUDA2 and gsplat's knn(points, 4) start the scales from.
 *   d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) of the three fp32 differences (csrc/gs_knn.h: one function for the device and the host
 *   test build); the m values are summed in ascending order and scaled by a float constant (1, 1/2, 1/3): no division.
 *   j != i is by index: a duplicate of a point is its neighbour at distance 0.  A row with a NaN or an infinity is nobody's
 *   neighbour and gets 0; F <= 1 gives 0 everywhere.
 * The search is exact: the result depends on the multiset of the other points only -- the same bits every call, on any stream, and
 * under any permutation of the rows.  Points are sorted by a 63-bit Morton key (a stable radix sort written here), cut into boxes of
 * GSPLAT_KNN_BOX sorted points with the AABB of their actual points, and a wave skips a box only when the box is strictly farther than
 * the third-best of every one of its lanes.  O(n * n / GSPLAT_KNN_BOX) box tests.
 * scratch: gsplat_knn_scratch_bytes(n) device bytes (about 40 n; -1 for n outside [0, 2^31)), 256-byte aligned, any contents; one
 * call at a time per scratch buffer.  points and dist2 4-byte aligned.  n == 0 launches nothing.  No float atomic; nothing is read
 * back to the host.                                                                                                               */
#define GSPLAT_KNN_BOX 256
int64_t gsplat_knn_scratch_bytes(int64_t n);
int gsplat_knn_mean_dist2(int64_t n, const float* points, float* dist2, void* scratch, void* stream);

/* ---- per-view camera-pose corrections (not in the reference) --------------------------------------------------------
 * A rigid correction per training camera, delta = (d[3], p[3], s[3]), nine floats with zero as the identity -- a translation and the
 * 6-D rotation of Zhou et al., gsplat's pose_opt parametrisation --, composed with the given pose before the render.  With
 * c2w = [[R, e], [r3]] (row-major 4 x 4):
 *     a1 = p + (1,0,0)   a2 = s + (0,1,0)   b1 = a1 / max(|a1|, 1e-12)   u2 = a2 - (b1.a2) b1   b2 = u2 / max(|u2|, 1e-12)   b3 = b1 x b2
 *     out[:3,:3] = R D, D the 3 x 3 with ROWS b1, b2, b3;      out[:3,3] = R d + e;      out[3,:] = c2w[3,:]
 * (csrc/gs_pose_delta.h has the fma chains: delta = 0 returns every finite c2w as the same numbers -- a -0 may come back as +0.)  An
 * active clamp treats its denominator as a constant in the backward.  c2w, out, grad_out, grad_c2w: [batch, 16] floats; delta:
 * [batch, 9].  These are NOT the render's own pose gradient (gsplat_pose_scratch_bytes / gsplat_project_backward_pose, dL/dc2w of a
 * frame): they take that gradient as grad_out.  Every entry is one launch of one lane per view on the caller's stream, reads
 * nothing back, allocates nothing and needs no scratch.  batch (n_views) > 0 and <= 2^30, else GSPLAT_ERR_BAD_ARG, as for a NULL
 * required pointer -- before anything is launched.  Arrays 4-byte aligned.  No output may alias an input.
 * Backward: grad_c2w (NULL: not computed) = dL/dc2w, and the nine floats dL/ddelta of view b (grad_delta == NULL: not computed) go to
 *   row b of grad_delta, or to row row_index[b] when row_index (batch int32 on the device; a negative entry drops the view) is given;
 *   the rows named must be distinct; a row no view names keeps its bits.  flags: GSPLAT_POSE_DELTA_ACCUMULATE adds to the
 *   destination rows instead of overwriting them; any other bit is refused first ("unknown flag").  Either half alone has the bits
 *   it has in a call for both.  No atomics: the same bits on every call, stream and launch.
 * Decay: grad[v, k] = fma(reg, delta[v, k], grad[v, k]) over a table of n_views rows -- the gradient of (reg / 2) |delta|^2.      */
#define GSPLAT_POSE_DELTA_ACCUMULATE 1
int gsplat_pose_delta_forward(const float* c2w, const float* delta, int64_t batch, float* out, void* stream);
int gsplat_pose_delta_backward(const float* c2w, const float* delta, const float* grad_out, int64_t batch, float* grad_c2w, float* grad_delta,
                               const int32_t* row_index, int32_t flags, void* stream);
int gsplat_pose_delta_decay(const float* delta, int64_t n_views, float reg, float* grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_MI355X_H */
