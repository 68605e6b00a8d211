// gs_project_backward.h -- K8 project_backward_kernel, pose reduce, logit gradients, SH accumulate.
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"
#include "gs_project.h"

using namespace gsm;
namespace {

// ---- K8 ------------------------------------------------------------------------------------------
// Same per-wave LDS staging as K1 for the inputs; the gradients go the other way: every lane writes its rows into LDS
// (f_rest gradient over the staged f_rest: each coefficient is read before its gradient is written) and the wave
// stores the 64 rows with coalesced 16-byte accesses.  Direct per-lane stores of a [N,45] gradient wrote 3.8x the
// algorithmic bytes (partial lines evicted before they filled).

// JAC (fused inputs): the forward left d rgb / d logit and d logit / d position in project_state (GSPLAT_PROJECT_SAVE_SH_JACOBIAN),
// so the 192 bytes of SH coefficients are not read again: 48 instead of 192 bytes per visible Gaussian, and no dY accumulators.
// ADAM (fused inputs, saved Jacobian, not factored): the 45 f_rest gradients of a Gaussian are not written: the rows are stepped in
// place (adam_rows) -- the 192 of the 236 gradient bytes per Gaussian neither leave this kernel nor come back into the optimiser's.
// ACC (fused inputs, saved Jacobian, not factored): every gradient is ADDED to what `out` holds -- the gradients of the views of one
// iteration summed by the kernel that forms them, instead of a pass of the host's autograd per view (read two, write one).
// POSE (plain or factored): also the camera-pose gradient.  Every lane forms its Gaussian's 12 terms -- dL/dW (gs_math.h pose_grad_w)
// and dL/dp -- the wave adds them up in a fixed order (wave_sum_f) and stores ONE 64-byte row per block into pose_rows[blockIdx.x]
// (every block writes its row: nothing to clear); pose_reduce_kernel adds the rows.  out.pos == NULL: no gradient row is stored
// (pose only).
// DEPTH (not with ADAM / ACC): column 9 of grad2d holds dL/dz of the Gaussian's camera depth (gsplat_rasterize_backward_aux); it joins
// the camera-space z gradient, from where position and pose get it.
// NB (fused inputs): the active SH bases of the forward that filled the frame (gs_math.h).  The inactive columns of the f_rest
// gradient are exact zeros (NB = 4, 9: written into the LDS rows by the emitter, so the rows leave as before).  NB = 1 (degree 0): f_rest
// is not read, its gradient is not formed and has no LDS -- the rows are stored as zeros (zero_rows), stepped with a zero gradient
// (ADAM) or left alone (ACC).
// FILTER: the state was projected with the low-pass (gs_math.h project_gaussian<true>): the recomputed projection adds the same s, and
// with vk.antialias the opacity compensation rho joins the covariance gradient and scales the opacity's own.
template <bool FUSED, bool JAC = false, bool ADAM = false, bool ACC = false, bool POSE = false, bool DEPTH = false, int NB = 16, bool FILTER = false>
__global__ __launch_bounds__(64) void project_backward_kernel(gsplat_gaussians g, const Camera* __restrict__ camp, ViewK vk,
                                                              const uint32_t* __restrict__ tiles, const float* __restrict__ grad2d,
                                                              gsplat_gaussian_grads out, bool factored, const float* __restrict__ kj_in,
                                                              AdamRest ar, f4* __restrict__ pose_rows = nullptr) {
    static_assert(!ADAM || (FUSED && JAC), "the in-place step needs the direct path");
    static_assert(!ACC || (FUSED && JAC && !ADAM), "accumulation is built for the direct path");
    static_assert(!POSE || (!ADAM && !ACC), "the pose gradient is built for the plain backward");
    static_assert(!DEPTH || (!ADAM && !ACC), "the depth gradient is built for the plain backward");
    // DIRECT (fused inputs, saved Jacobian): nothing is staged IN (the 44 bytes of geometry are loaded by the lanes), and of the
    // gradients only the 45 f_rest rows go OUT through LDS (the rows of 1 / 3 / 4 floats are stored by the lanes): 11 520 B per
    // wave instead of 15 104 -> 14 waves per CU instead of 10.
    static_assert(NB == 16 || FUSED, "the SH degree belongs to fused inputs");
    constexpr bool DIRECT = FUSED && JAC;
    constexpr bool REST = FUSED && NB > 1;                // are there f_rest gradients to form?
    __shared__ float s_geo[DIRECT ? 4 : sizeof(ProjectLds<FUSED>) / 4];
    ProjectLds<FUSED>& s = *reinterpret_cast<ProjectLds<FUSED>*>(s_geo);
    __shared__ float s_dc[FUSED && !DIRECT ? 64 * 3 : 4];
    __shared__ float s_rest[REST ? 64 * 45 : 4];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + lane;
    const Camera cam = *camp;
    const bool vis = (i < g.n) && tiles[i] != 0;
    const bool any_vis = __any(vis);
    float r9[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float g_z = 0.f;                                      // (DEPTH)
    float kj[12];
    GaussIn in;
    if (any_vis) {
        if (DIRECT) {
            if (vis) {
#pragma unroll
                for (int k = 0; k < 3; ++k) in.p[k] = g.pos[i * 3 + k];
                in.o_raw = g.opacity_raw[i];
                const f4 q = *reinterpret_cast<const f4*>(g.q_raw + i * 4);
                in.qr[0] = q.x; in.qr[1] = q.y; in.qr[2] = q.z; in.qr[3] = q.w;
#pragma unroll
                for (int k = 0; k < 3; ++k) in.sr[k] = g.scale_raw[i * 3 + k];
            }
        } else {
            stage_geometry<FUSED>(s, g, row0, lane);
        }
        if (FUSED && !JAC) {
            stage_rows<3>(s_dc, g.f_dc, row0, g.n, lane);
            if (REST) stage_rows<45>(s_rest, g.f_rest, row0, g.n, lane);
        }
        if (JAC && vis) {
            const f4* src = reinterpret_cast<const f4*>(kj_in + i * 12);
            const f4 k0 = src[0], k1 = src[1], k2 = src[2];
            kj[0] = k0.x; kj[1] = k0.y; kj[2] = k0.z; kj[3] = k0.w; kj[4] = k1.x; kj[5] = k1.y; kj[6] = k1.z; kj[7] = k1.w;
            kj[8] = k2.x; kj[9] = k2.y; kj[10] = k2.z; kj[11] = k2.w;
        }
        if (vis) {
            const f4 g0 = *reinterpret_cast<const f4*>(grad2d + i * 16), g1 = *reinterpret_cast<const f4*>(grad2d + i * 16 + 4);
            r9[0] = g0.x; r9[1] = g0.y; r9[2] = g0.z; r9[3] = g0.w; r9[4] = g1.x; r9[5] = g1.y; r9[6] = g1.z; r9[7] = g1.w;
            r9[8] = grad2d[i * 16 + 8];
            if (DEPTH) g_z = grad2d[i * 16 + 9];
        }
    }
    if (!DIRECT) __syncthreads();
    GradOut go;
    float gdc[3] = {0.f, 0.f, 0.f};                       // (DIRECT) d L / d f_dc of this lane's Gaussian
    float* const dc_rows = DIRECT ? gdc : s_dc + lane * 3;
    float gw[9];                                          // (POSE) d L / d W of this lane's Gaussian
    if (vis) {
        if (!DIRECT) in = gauss_from_lds<FUSED>(s, lane);
        go = project_backward_core<POSE, DEPTH, NB, FILTER>(in, FUSED, ShCoefLds{dc_rows, s_rest + lane * 45},
                                   ShEmitFor<NB>{dc_rows, s_rest + lane * 45}, cam, vk, true, r9, true, JAC ? kj : nullptr,
                                   POSE ? gw : nullptr, g_z);
    } else {
        go = GradOut{};
        if (FUSED) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dc_rows[k] = 0.f;
            if (REST)
                for (int k = 0; k < 45; ++k) s_rest[lane * 45 + k] = 0.f;
        }
        if (POSE) {
#pragma unroll
            for (int k = 0; k < 9; ++k) gw[k] = 0.f;
        }
    }
    if (POSE) {
        float t[12];
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = wave_sum_f(gw[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) t[9 + k] = wave_sum_f(go.p[k]);
        if (lane == 0) {
            f4* row = pose_rows + (int64_t)blockIdx.x * 4;
            row[0] = f4{t[0], t[1], t[2], t[3]};
            row[1] = f4{t[4], t[5], t[6], t[7]};
            row[2] = f4{t[8], t[9], t[10], t[11]};
            row[3] = f4{0.f, 0.f, 0.f, 0.f};
        }
        if (!out.pos) return;                               // pose only (uniform)
    }
    if (DIRECT) {
        if (ACC) {
            if (vis) {                                      // (a Gaussian that is not visible adds nothing)
#pragma unroll
                for (int k = 0; k < 3; ++k) out.pos[i * 3 + k] += go.p[k];
                out.opacity_raw[i] += go.o_raw;
                const f4 q0 = *reinterpret_cast<const f4*>(out.q_raw + i * 4);
                *reinterpret_cast<f4*>(out.q_raw + i * 4) = f4{q0.x + go.qr[0], q0.y + go.qr[1], q0.z + go.qr[2], q0.w + go.qr[3]};
#pragma unroll
                for (int k = 0; k < 3; ++k) out.scale_raw[i * 3 + k] += go.sr[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) out.f_dc[i * 3 + k] += gdc[k];
            }
            if (REST && any_vis) {                          // (degree 0 adds nothing to f_rest)
                __syncthreads();
                unstage_rows<45, true>(out.f_rest, s_rest, row0, g.n, lane);
            }
            return;
        }
        if (i < g.n) {                                      // every row is written (zeros for a Gaussian that is not visible)
#pragma unroll
            for (int k = 0; k < 3; ++k) out.pos[i * 3 + k] = go.p[k];
            out.opacity_raw[i] = go.o_raw;
            *reinterpret_cast<f4*>(out.q_raw + i * 4) = f4{go.qr[0], go.qr[1], go.qr[2], go.qr[3]};
#pragma unroll
            for (int k = 0; k < 3; ++k) out.scale_raw[i * 3 + k] = go.sr[k];
            if (factored) {
                // d L / d f_dc = (d L / d colour logit) * Y0: hand out the 3 logit gradients instead of the 48 SH gradients
                if (out.color) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) out.color[i * 3 + k] = gdc[k] * (1.0f / GS_K0);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) out.f_dc[i * 3 + k] = gdc[k];
            }
        }
        if (!factored) {
            if (REST) __syncthreads();
            if (ADAM) {
                const DevCounts* cnt = reinterpret_cast<const DevCounts*>(ar.counts);
                // skipped only for the frames the host rolls back: an overflow, or survivors that are all off screen.  A frame with
                // no survivor at all is a valid zero image: every gradient row is zero and the rows take the zero-gradient step
                if (cnt->n_binned <= ar.capacity && !(cnt->n_survivors > 0 && cnt->n_visible == 0)) adam_rows<45, !REST>(ar, s_rest, row0, g.n, lane);      // (uniform)
            } else if (REST) {
                unstage_rows<45>(out.f_rest, s_rest, row0, g.n, lane);
            } else {
                zero_rows<45>(out.f_rest, row0, g.n, lane);
            }
        }
        return;
    }
    __syncthreads();      // every lane has read its inputs: the geometry buffers can take the gradients
#pragma unroll
    for (int k = 0; k < 3; ++k) s.pos[lane * 3 + k] = go.p[k];
    s.opa[lane] = go.o_raw;
    if (FUSED) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s.a[lane * 4 + k] = go.qr[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) s.b[lane * 3 + k] = go.sr[k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) s.a[lane * 9 + k] = go.S9[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) s.b[lane * 3 + k] = go.col[k];
    }
    __syncthreads();
    unstage_rows<3>(out.pos, s.pos, row0, g.n, lane);
    unstage_rows<1>(out.opacity_raw, s.opa, row0, g.n, lane);
    if (FUSED) {
        unstage_rows<4>(out.q_raw, s.a, row0, g.n, lane);
        unstage_rows<3>(out.scale_raw, s.b, row0, g.n, lane);
        if (factored) {
            // d L / d f_dc = (d L / d colour logit) * Y0: hand out the 3 logit gradients instead of the 48 SH gradients
            // (gsplat_sh_accumulate rebuilds those, for any number of views, from logit gradients and view directions)
#pragma unroll
            for (int k = 0; k < 3; ++k) s_dc[lane * 3 + k] *= 1.0f / GS_K0;      // each lane its own slots: no barrier needed
            __syncthreads();
            if (out.color) unstage_rows<3>(out.color, s_dc, row0, g.n, lane);
        } else {
            unstage_rows<3>(out.f_dc, s_dc, row0, g.n, lane);
            if (REST) unstage_rows<45>(out.f_rest, s_rest, row0, g.n, lane);
            else zero_rows<45>(out.f_rest, row0, g.n, lane);
        }
    } else {
        unstage_rows<9>(out.sigma, s.a, row0, g.n, lane);
        unstage_rows<3>(out.color, s.b, row0, g.n, lane);
    }
}

// ---- the camera-pose gradient: the rows of project_backward_kernel<..., POSE> added up ------------------------------------------
// A row (16 floats) = (dL/dW row-major [9], dL/dp [3], 0 [4]) of one block of 64 Gaussians.  Block b of a launch adds rows
// [b nrows / parts, (b + 1) nrows / parts) -- 16 threads per row, 16 rows at a time, then the 16 partial rows in LDS in a fixed order
// -- and stores one row into out[b]; with FINAL (one block) it stores dL/dc2w instead: W = c2w[:3,:3]^T -> the transpose,
// dL/dc2w[:3,3] = -sum dL/dp, the last row of c2w is a constant.  No atomics, no block waits for another: the same rows give the
// same bits.  Two launches at most: POSE_PARTS blocks, then one.

template <bool FINAL>
__global__ __launch_bounds__(256) void pose_reduce_kernel(const float* __restrict__ rows, int64_t nrows, int parts, float* __restrict__ out) {
    __shared__ float s_part[16][17];
    __shared__ float s_sum[16];
    const int term = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * nrows / parts, r1 = (int64_t)(blockIdx.x + 1) * nrows / parts;
    float acc = 0.f;
    for (int64_t r = r0 + grp; r < r1; r += 16) acc += rows[r * 16 + term];
    s_part[grp][term] = acc;
    __syncthreads();
    if (threadIdx.x < 16) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s_part[k][term];
        if (FINAL) s_sum[term] = t;
        else out[(int64_t)blockIdx.x * 16 + term] = t;
    }
    if (!FINAL) return;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int r = term >> 2, c = term & 3;          // this thread's entry of dL/dc2w
        out[term] = r == 3 ? 0.f : (c == 3 ? -s_sum[9 + r] : s_sum[c * 3 + r]);
    }
}

// ---- colour-logit gradients straight from the raster backward's sums (data-parallel exchange) -----------
// d L / d logit[ch] = (d L / d colour[ch]) * c (1 - c): only needs the raster backward's colour sums and the colour in the
// record, so the all-gather of the logit gradients can start BEFORE gsplat_project_backward and overlap it.
__global__ __launch_bounds__(256) void logit_grad_kernel(int64_t n, const uint32_t* __restrict__ tiles, const Rec64* __restrict__ rec,
                                                         const float* __restrict__ grad2d, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float g[3] = {0.f, 0.f, 0.f};
    if (tiles[i] != 0u) {
        const f4 c = rec[i].r2;
        const float* r = grad2d + i * 16;
        g[0] = r[6] * c.x * (1.f - c.x); g[1] = r[7] * c.y * (1.f - c.y); g[2] = r[8] * c.z * (1.f - c.z);
    }
    out[i * 3] = g[0]; out[i * 3 + 1] = g[1]; out[i * 3 + 2] = g[2];
}

// ---- SH gradients from logit gradients (data-parallel exchange) ---------------------------------------
// grad f_dc[i, ch] = scale * sum_v glogit[v, i, ch] * Y0,  grad f_rest[i, ch * 15 + k - 1] = scale * sum_v glogit[v, i, ch] * Y_k(d_v(i)),
// d_v(i) = unit vector from camera v's position to Gaussian i (spherical_harmonics.py:132-133).
// NB: the active SH bases of the views' renders; the columns of the inactive ones are written as zeros.
template <int NB = 16>
__global__ __launch_bounds__(64) void sh_accumulate_kernel(int64_t n, int n_views, const float* __restrict__ pos, const float* __restrict__ eyes,
                                                           const float* __restrict__ glogit, float scale, float* __restrict__ grad_f_dc,
                                                           float* __restrict__ grad_f_rest) {
    __shared__ float s_pos[64 * 3], s_dc[64 * 3], s_rest[64 * 45];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + lane;
    stage_rows<3>(s_pos, pos, row0, n, lane);
    __syncthreads();
    float acc[48];
#pragma unroll
    for (int k = 0; k < 48; ++k) acc[k] = 0.f;
    if (i < n) {
        const float p[3] = {s_pos[lane * 3], s_pos[lane * 3 + 1], s_pos[lane * 3 + 2]};
        for (int v = 0; v < n_views; ++v) {
            const float* gl = glogit + ((int64_t)v * n + i) * 3;
            const float g0 = gl[0], g1 = gl[1], g2 = gl[2];
            if (g0 == 0.f && g1 == 0.f && g2 == 0.f) continue;       // not binned in this view
            const float eye[3] = {eyes[v * 3], eyes[v * 3 + 1], eyes[v * 3 + 2]};
            ShMid sm;
            sh_basis(p, eye, sm);
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                acc[k] += g0 * sm.Y[k]; acc[16 + k] += g1 * sm.Y[k]; acc[32 + k] += g2 * sm.Y[k];
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        s_dc[lane * 3 + ch] = scale * acc[ch * 16];
#pragma unroll
        for (int k = 1; k < 16; ++k) s_rest[lane * 45 + ch * 15 + (k - 1)] = k < NB ? scale * acc[ch * 16 + k] : 0.f;
    }
    __syncthreads();
    unstage_rows<3>(grad_f_dc, s_dc, row0, n, lane);
    unstage_rows<45>(grad_f_rest, s_rest, row0, n, lane);
}

}  // namespace
