// One iteration of the object-pose fit for B starts, enqueued as one launch sequence on the caller's stream: no host read, no
// allocation (interactvlm_amd.fit.DevicePoseFit calls it once per iteration).  It chains the entry points of pose.hip,
// silhouette.hip and contact_pair.hip with the small kernels of this file:
//
//    1 pose_forward                            moved = (s v) R + t
//    2 fit_offset                              moved_off = moved + hum_centroid_offset (a separate fp32 add, as torch has it)
//    3 soft_silhouette_forward                 alpha
//    4 silhouette_terms                        mask loss, centroid, sums
//    5 fit_combine                             the total, its terms (history rows) and the seeds g_loss, g_centroid
//    6 silhouette_terms (backward form)        grad_alpha
//    7 soft_silhouette_backward                g_sil = dL/d moved_off = dL/d moved
//    8 contact_pair                            contact value and g_pair = d contact / d moved
//    9 fit_vertex_grad                         g = g_sil + w_k g_pair (the product rounded first, then the sum)
//   10 pose_transform_backward                 the parameter gradients
//   11 fit_adam                                parameters and moments
//   12 fit_advance                             the step counter, one thread
//
// 8 runs before 5 (5 reads its value); 2-4, 6, 7 are not launched when neither image term counts, 8 and 9 not when the contact
// term does not.  Which terms count is the caller's (host) fact: a run has one launch sequence per phase.
//
// Numerics.  This file is built with -ffp-contract=off (build.py): every operation below is its own IEEE operation.  fit_combine
// and fit_vertex_grad repeat the fp32 operations of ObjectPoseFit.forward and of its autograd backward one by one, so that an
// iteration computes the bits of the torch step.  fit_adam evaluates torch's Adam (amsgrad off, no weight decay) per element in
// fp64 and rounds each stored value (p, m, v) to fp32 once.  Everything is per start or per element: a start's bits do not depend
// on B or on its place in the batch.  The step counter is read by 5 and 11 and written by 12 alone, in a launch of its own.
#include <cmath>
#include <cstdint>

#include "fit_common.h"

namespace ivlm {
namespace {

constexpr int kThreads = 256;
constexpr int kParams = 10;  // elements per start: rot6d 6, translation 3, scale 1

__global__ __launch_bounds__(kThreads) void fit_offset_kernel(const float* __restrict__ moved, const float* __restrict__ off, int64_t total,
                                                              float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < total) out[e] = moved[e] + off[e % 3];
}

// one thread per start.  on: IVLM_FIT_MASK | IVLM_FIT_CENTROID | IVLM_FIT_CONTACT; loss / centroid are read only when an image term
// is on, contact only when the contact term is.  The history rows are written while *step < max_iter.
__global__ __launch_bounds__(kThreads) void fit_combine_kernel(const float* __restrict__ loss, const float* __restrict__ centroid,
                                                               const float* __restrict__ contact, const float* __restrict__ target_c,
                                                               float w_m, float w_c, float w_k, int on, int B, int max_iter,
                                                               const int32_t* __restrict__ step, float* __restrict__ history,
                                                               float* __restrict__ term_history, float* __restrict__ g_loss,
                                                               float* __restrict__ g_centroid) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    float terms[3] = {0.0f, 0.0f, 0.0f};
    float total = 0.0f;
    if (on & IVLM_FIT_MASK) {
        terms[0] = loss[b];
        total = total + terms[0] * w_m;
    }
    float d0 = 0.0f, d1 = 0.0f;
    if (on & IVLM_FIT_CENTROID) {
        d0 = centroid[b * 2] - target_c[0];
        d1 = centroid[b * 2 + 1] - target_c[1];
        terms[1] = d0 * d0 + d1 * d1;
        total = total + terms[1] * w_c;
    }
    if (on & IVLM_FIT_CONTACT) {
        terms[2] = contact[b];
        total = total + terms[2] * w_k;
    }
    const int t = *step;
    if (t >= 0 && t < max_iter) {
        history[(int64_t)t * B + b] = total;
#pragma unroll
        for (int k = 0; k < 3; ++k) term_history[((int64_t)t * 3 + k) * B + b] = terms[k];
    }
    if (on & (IVLM_FIT_MASK | IVLM_FIT_CENTROID)) {  // what autograd hands to the backward of silhouette_terms
        g_loss[b] = (on & IVLM_FIT_MASK) ? w_m : 0.0f;
        g_centroid[b * 2] = (on & IVLM_FIT_CENTROID) ? 2.0f * (w_c * d0) : 0.0f;  // w_c d + w_c d: exact
        g_centroid[b * 2 + 1] = (on & IVLM_FIT_CENTROID) ? 2.0f * (w_c * d1) : 0.0f;
    }
}

// g = g_sil + w_k g_pair, or w_k g_pair alone (g_sil NULL).  out may be g_pair: an element is read and written by its own thread.
__global__ __launch_bounds__(kThreads) void fit_vertex_grad_kernel(const float* __restrict__ g_sil, const float* g_pair, float w_k,
                                                                   int64_t total, float* out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const float c = w_k * g_pair[e];
    out[e] = g_sil ? g_sil[e] + c : c;
}

struct AdamGroups {
    float* p[3];
    const float* g[3];
    float* m[3];
    float* v[3];
    double lr[3];
    double beta1, beta2, eps;
};

// one thread per parameter element: element e of start b is rot6d[e] (e < 6), translation[e - 6] (e < 9) or the scale
__global__ __launch_bounds__(kThreads) void fit_adam_kernel(AdamGroups a, int B, const int32_t* __restrict__ step) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= B * kParams) return;
    const int b = idx / kParams, e = idx - b * kParams;
    const int grp = e < 6 ? 0 : (e < 9 ? 1 : 2);
    if (!a.g[grp]) return;  // not optimised: not touched
    const int64_t at = grp == 0 ? (int64_t)b * 6 + e : (grp == 1 ? (int64_t)b * 3 + (e - 6) : (int64_t)b);
    const double t = (double)(*step + 1);
    const double g = (double)a.g[grp][at];
    const double m = a.beta1 * (double)a.m[grp][at] + (1.0 - a.beta1) * g;
    const double v = a.beta2 * (double)a.v[grp][at] + (1.0 - a.beta2) * (g * g);
    const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
    const double p = (double)a.p[grp][at] - (a.lr[grp] / bc1) * m / (sqrt(v) / sqrt(bc2) + a.eps);
    a.m[grp][at] = (float)m;
    a.v[grp][at] = (float)v;
    a.p[grp][at] = (float)p;
}

__global__ void fit_advance_kernel(int32_t* step) { *step = *step + 1; }

int launch_adam(const AdamGroups& a, int B, const int32_t* step, hipStream_t st) {
    fit_adam_kernel<<<(B * kParams + kThreads - 1) / kThreads, kThreads, 0, st>>>(a, B, step);
    return ivlm_launch_status();
}

bool adam_ok(double lr, double beta1, double beta2, double eps) {
    // eps > 0: with eps == 0 a zero gradient on zero moments would be 0 / 0
    return std::isfinite(lr) && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && std::isfinite(eps) && eps > 0.0;
}

struct FitLayout {
    size_t pose, sil, terms, pair, moved, moved_off, alpha, galpha, g_sil, g_pair, sums, small, total;
    size_t pose_bytes, sil_bytes, terms_bytes, pair_bytes;
};

// 0 in .total: a member refuses the sizes
FitLayout fit_layout(int B, int N, int F, int H, int W, int N_h) {
    FitLayout l = {};
    if (B <= 0 || N <= 0 || F <= 0 || H <= 0 || W <= 0 || N_h <= 0 || B > 65535) return l;
    l.pose_bytes = pose_transform_workspace_bytes(B, N);
    l.sil_bytes = soft_silhouette_workspace_bytes(B, N, F, H, W);
    l.pair_bytes = contact_pair_workspace_bytes(B, N, N_h);
    if (!l.pose_bytes || !l.sil_bytes || !l.pair_bytes) return l;
    l.terms_bytes = IVLM_SILHOUETTE_TERMS_WORKSPACE(B, H);
    const size_t verts = (size_t)B * N * 3 * sizeof(float), image = (size_t)B * H * W * sizeof(float);
    Carve c;
    l.pose = c.take(l.pose_bytes);
    l.sil = c.take(l.sil_bytes);
    l.terms = c.take(l.terms_bytes);
    l.pair = c.take(l.pair_bytes);
    l.moved = c.take(verts);
    l.moved_off = c.take(verts);
    l.alpha = c.take(image);
    l.galpha = c.take(image);
    l.g_sil = c.take(verts);
    l.g_pair = c.take(verts);
    l.sums = c.take((size_t)B * 5 * sizeof(double));
    l.small = c.take((size_t)B * 7 * sizeof(float));  // loss 1, centroid 2, contact 1, g_loss 1, g_centroid 2
    l.total = c.off;
    return l;
}

}  // namespace

size_t fit_step_workspace_bytes(int B, int N, int F, int H, int W, int N_h) { return fit_layout(B, N, F, H, W, N_h).total; }

int fit_adam(const AdamGroups& a, int B, const int32_t* step, hipStream_t st) {
    if (!step || B <= 0 || (!a.g[0] && !a.g[1] && !a.g[2])) return IVLM_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) {
        if (a.g[k] && (!a.p[k] || !a.m[k] || !a.v[k])) return IVLM_ERR_INVALID_ARG;
        if (a.g[k] && !adam_ok(a.lr[k], a.beta1, a.beta2, a.eps)) return IVLM_ERR_INVALID_ARG;
    }
    if (B > 65535) return IVLM_ERR_UNSUPPORTED;
    return launch_adam(a, B, step, st);
}

int fit_step(const IvlmFitStepArgs& x, hipStream_t st) {
    const int B = x.B, N = x.N, F = x.F, H = x.H, W = x.W, N_h = x.N_h;
    const int on = x.terms_on;
    const bool image = on & (IVLM_FIT_MASK | IVLM_FIT_CENTROID), contact = on & IVLM_FIT_CONTACT;
    const bool pose = x.optimise & IVLM_FIT_POSE, scale = x.optimise & IVLM_FIT_SCALE;
    if (!x.obj_verts || !x.faces || !x.vert_face_offsets || !x.vert_face_list || !x.human_verts || !x.obj_probs || !x.human_probs ||
        !x.target || !x.target_centroid || !x.centroid_offset || !x.rotation || !x.translation || !x.scale || !x.step || !x.history ||
        !x.term_history || !x.workspace)
        return IVLM_ERR_INVALID_ARG;
    if (B <= 0 || N <= 0 || F <= 0 || H <= 0 || W <= 0 || N_h <= 0 || x.max_iter <= 0) return IVLM_ERR_INVALID_ARG;
    if (!(image || contact) || (on & ~7) || !(pose || scale) || (x.optimise & ~3)) return IVLM_ERR_INVALID_ARG;
    if (pose && (!x.grad_rotation || !x.grad_translation || !x.m_rotation || !x.m_translation || !x.v_rotation || !x.v_translation))
        return IVLM_ERR_INVALID_ARG;
    if (scale && (!x.grad_scale || !x.m_scale || !x.v_scale)) return IVLM_ERR_INVALID_ARG;
    AdamGroups a = {};
    a.beta1 = x.beta1, a.beta2 = x.beta2, a.eps = x.eps;
    a.lr[0] = x.lr_rotation, a.lr[1] = x.lr_translation, a.lr[2] = x.lr_scale;
    for (int k = 0; k < 3; ++k)
        if (!adam_ok(a.lr[k], a.beta1, a.beta2, a.eps)) return IVLM_ERR_INVALID_ARG;
    if (x.p_dtype != IVLM_F32 && x.p_dtype != IVLM_BF16) return IVLM_ERR_UNSUPPORTED;
    if (!(std::isfinite(x.fx) && std::isfinite(x.fy) && std::isfinite(x.px) && std::isfinite(x.py) && std::isfinite(x.sigma) &&
          x.sigma > 0.0f && std::isfinite(x.blur_radius) && x.blur_radius >= 0.0f))
        return IVLM_ERR_UNSUPPORTED;
    const FitLayout l = fit_layout(B, N, F, H, W, N_h);
    if (!l.total) return IVLM_ERR_UNSUPPORTED;
    void* ws = x.workspace;
    if (!workspace_ok(ws, x.workspace_bytes, l.total, 256)) return IVLM_ERR_WORKSPACE;

    float* moved = ws_at<float>(ws, l.moved);
    float* moved_off = ws_at<float>(ws, l.moved_off);
    float* alpha = ws_at<float>(ws, l.alpha);
    float* galpha = ws_at<float>(ws, l.galpha);
    float* g_sil = ws_at<float>(ws, l.g_sil);
    float* g_pair = ws_at<float>(ws, l.g_pair);
    double* sums = ws_at<double>(ws, l.sums);
    float* loss = ws_at<float>(ws, l.small);
    float* centroid = loss + B;
    float* value = loss + 3 * (size_t)B;
    float* g_loss = loss + 4 * (size_t)B;
    float* g_centroid = loss + 5 * (size_t)B;
    const int64_t nv = (int64_t)B * N * 3;
    const unsigned vblocks = (unsigned)((nv + kThreads - 1) / kThreads);
    int rc;

#define FIT_TRY(call)                 \
    do {                              \
        rc = (call);                  \
        if (rc != IVLM_OK) return rc; \
    } while (0)

    FIT_TRY(pose_transform_forward(x.obj_verts, x.rotation, x.translation, x.scale, B, N, moved, st));
    if (image) {
        fit_offset_kernel<<<vblocks, kThreads, 0, st>>>(moved, x.centroid_offset, nv, moved_off);
        FIT_TRY(ivlm_launch_status());
        FIT_TRY(soft_silhouette_forward(moved_off, x.faces, B, N, F, H, W, x.fx, x.fy, x.px, x.py, x.sigma, x.blur_radius, alpha,
                                        ws_at<char>(ws, l.sil), l.sil_bytes, st));
        FIT_TRY(silhouette_terms(alpha, x.target, 0, B, H, W, loss, centroid, sums, nullptr, nullptr, nullptr, ws_at<char>(ws, l.terms),
                                 l.terms_bytes, st));
    }
    if (contact)
        FIT_TRY(contact_pair(moved, x.human_verts, x.obj_probs, x.human_probs, x.p_dtype, B, N, N_h, (int64_t)N * 3, 0, value, g_pair,
                             nullptr, ws_at<char>(ws, l.pair), l.pair_bytes, st));
    fit_combine_kernel<<<(B + kThreads - 1) / kThreads, kThreads, 0, st>>>(loss, centroid, value, x.target_centroid, x.w_mask,
                                                                           x.w_centroid, x.w_contact, on, B, x.max_iter, x.step,
                                                                           x.history, x.term_history, g_loss, g_centroid);
    FIT_TRY(ivlm_launch_status());
    if (image) {
        FIT_TRY(silhouette_terms(nullptr, x.target, 0, B, H, W, nullptr, nullptr, sums, g_loss, g_centroid, galpha, nullptr, 0, st));
        FIT_TRY(soft_silhouette_backward(moved_off, x.vert_face_offsets, x.vert_face_list, galpha, B, N, F, H, W, x.fx, x.fy, x.px,
                                         x.py, x.sigma, x.blur_radius, g_sil, ws_at<char>(ws, l.sil), l.sil_bytes, st));
    }
    const float* g = g_sil;
    if (contact) {
        fit_vertex_grad_kernel<<<vblocks, kThreads, 0, st>>>(image ? g_sil : nullptr, g_pair, x.w_contact, nv, g_pair);
        FIT_TRY(ivlm_launch_status());
        g = g_pair;
    }
    FIT_TRY(pose_transform_backward(x.obj_verts, x.rotation, x.scale, g, B, N, pose ? x.grad_rotation : nullptr,
                                    pose ? x.grad_translation : nullptr, scale ? x.grad_scale : nullptr, ws_at<char>(ws, l.pose), l.pose_bytes,
                                    st));
    a.p[0] = x.rotation, a.p[1] = x.translation, a.p[2] = x.scale;
    a.m[0] = x.m_rotation, a.m[1] = x.m_translation, a.m[2] = x.m_scale;
    a.v[0] = x.v_rotation, a.v[1] = x.v_translation, a.v[2] = x.v_scale;
    a.g[0] = pose ? x.grad_rotation : nullptr;
    a.g[1] = pose ? x.grad_translation : nullptr;
    a.g[2] = scale ? x.grad_scale : nullptr;
    FIT_TRY(launch_adam(a, B, x.step, st));
#undef FIT_TRY
    fit_advance_kernel<<<1, 1, 0, st>>>(x.step);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_fit_step_workspace_bytes(int B, int N, int F, int H, int W, int N_h) {
    return ivlm::fit_step_workspace_bytes(B, N, F, H, W, N_h);
}
int ivlm_fit_step(const IvlmFitStepArgs* args, ivlm_stream_t s) {
    ivlm_enter();
    if (!args) return IVLM_ERR_INVALID_ARG;
    return ivlm::fit_step(*args, ivlm_stream(s));
}
int ivlm_fit_adam(float* rotation, float* translation, float* scale, const float* grad_rotation, const float* grad_translation,
                  const float* grad_scale, float* m_rotation, float* m_translation, float* m_scale, float* v_rotation,
                  float* v_translation, float* v_scale, int B, const int32_t* step, double lr_rotation, double lr_translation,
                  double lr_scale, double beta1, double beta2, double eps, ivlm_stream_t s) {
    ivlm_enter();
    ivlm::AdamGroups a = {};
    a.p[0] = rotation, a.p[1] = translation, a.p[2] = scale;
    a.g[0] = grad_rotation, a.g[1] = grad_translation, a.g[2] = grad_scale;
    a.m[0] = m_rotation, a.m[1] = m_translation, a.m[2] = m_scale;
    a.v[0] = v_rotation, a.v[1] = v_translation, a.v[2] = v_scale;
    a.lr[0] = lr_rotation, a.lr[1] = lr_translation, a.lr[2] = lr_scale;
    a.beta1 = beta1, a.beta2 = beta2, a.eps = eps;
    return ivlm::fit_adam(a, B, step, ivlm_stream(s));
}
}
