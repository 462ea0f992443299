// Differentiable soft silhouette of a posed triangle mesh and the two image losses built on it: the mask and centroid terms of
// the reference's joint fitting stage (optim/optimizer.py `ObjPose_Opt.forward`, rendered there by pytorch3d's
// SoftSilhouetteShader), without a [H W, F] array.
//
//   projection   u = fx X / Z + px, v = fy Y / Z + py (OpenCV pinhole); pixel (row i, col j) has its centre at (j + 0.5, i + 0.5)
//   per face k   d_k = the smallest squared distance (pixels^2) from the pixel centre to the three edge SEGMENTS,
//                  t = clamp(dot(b - a, p - a) / |b - a|^2, 0, 1); an edge with |b - a|^2 <= 1e-8 uses |p - b|^2
//                kappa = (2 / min(H, W))^2 (pytorch3d's NDC scaling); the face counts at the pixel if the pixel is strictly inside
//                it or kappa d_k < blur_radius;  s_k = -kappa d_k inside, +kappa d_k outside;  p_k = sigmoid(-s_k / sigma)
//   alpha = 1 - prod_k (1 - p_k) over every counted face (no cap at the K nearest: the product does not depend on depth order)
//   a face is skipped whole when its screen area is zero or any of its vertices has Z <= 1e-6
//   d alpha / d s_k = -(1 - alpha) p_k / sigma, then through the segment distance (d d / d a = -2 (1 - t) r, d d / d b = -2 t r
//   with r = p - a - t (b - a) of the nearest edge: nothing flows through t, whose derivative is zero where the clamp is inactive)
//   and through the projection.
//
// Launches (all on the caller's stream, no atomics on floats, every sum in a fixed order - the same bits every call, for a pose
// whatever the batch around it).  The walk over the faces is screen_common.h's, shared with depth_order.hip; this file holds what
// is done per (pixel, face):
//   screen_project    per vertex (u, v); resets the pose's union box
//   sil_faces         screen_face with the box grown by r_px = sqrt(blur_radius / kappa); per face its three screen vertices (two
//                     float4) and its box; union_fold
//   sil_forward       tile_chunk: the records of the faces that meet the tile go to LDS, then every lane reads the same record (a
//                     broadcast ds_read_b128) and multiplies 1 + e^(-s_k / sigma) into a running fp32 product D - one rounding per
//                     face; 1 - alpha = 1 / D.  Writes alpha and keeps 1 - alpha.
//   sil_backward      box_walk<6>: at every pixel of the face's grown box it reads g_alpha (1 - alpha), recomputes p_k and the
//                     distance's derivative and adds to the six screen-space vertex gradients, IVLM_SILHOUETTE_CHAIN fp32 additions
//                     per lane; one [3, 2] fp32 record per face
//   screen_gather<2>  per vertex: the records of its incident faces, chained through the projection to dL/d(X, Y, Z)
//   terms_rows / terms_final / terms_grad   one fp64 reduction of (sum alpha, sum alpha t, sum t, sum i alpha, sum j alpha) per pose
//                 (per row block4_sum, then the rows by wave_fold: fit_common.h), mask_loss = 1 - sum(alpha t) / (sum alpha + sum t),
//                 centroid = (sum i alpha, sum j alpha) / sum alpha, and their analytic d / d alpha image.
#include <algorithm>
#include <cmath>

#include "screen_common.h"

namespace ivlm {
namespace {

constexpr int kChain = IVLM_SILHOUETTE_CHAIN;   // fp32 additions per lane before the fp64 accumulators take over
constexpr float kMinEdge2 = 1e-8f;
constexpr float kMaxExp2 = 100.0f;              // e^(-s / sigma) is clamped at 2^100 and the product at 1e30: 1 - alpha >= 1e-30
constexpr float kMaxProd = 1e30f;

struct SilParams {
    ScreenParams s;
    float c;      // kappa / sigma
    float c2;     // kappa / sigma * log2(e)
    float d_cut;  // blur_radius / kappa: the cut-off in pixels^2
    float r_px;   // sqrt(d_cut), rounded up
};

SilParams sil_params(int N, int F, int H, int W, float fx, float fy, float px, float py, float sigma, float blur) {
    SilParams p;
    const double side = (double)std::min(H, W);
    const double kappa = (2.0 / side) * (2.0 / side);
    p.s = ScreenParams{fx, fy, px, py, N, F, H, W};
    p.c = (float)(kappa / (double)sigma);
    p.c2 = (float)(kappa / (double)sigma * 1.4426950408889634);
    p.d_cut = (float)((double)blur / kappa);
    p.r_px = std::nextafter((float)std::sqrt((double)blur / kappa), INFINITY);
    return p;
}

// workspace carve, shared by the size query and both launchers
struct SilLayout {
    ScreenLayout s;
    size_t oma, frec, total;
};

SilLayout sil_layout(int B, int N, int F, int H, int W) {
    SilLayout l;
    Carve c;
    l.s = screen_layout(c, B, N, F, 32);
    l.oma = c.take((size_t)B * H * W * 4);
    l.frec = c.take((size_t)B * F * 24);
    l.total = c.off;
    return l;
}

__global__ __launch_bounds__(256) void sil_faces_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                        const float2* __restrict__ uv, float4* __restrict__ tri,
                                                        int4* __restrict__ box, int4* __restrict__ uni, SilParams p) {
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    int4 bx = make_int4(p.s.W, p.s.H, -1, -1);  // empty
    if (f < p.s.F) {
        const ScreenFace t = screen_face(verts, faces, uv, b, f, p.r_px, p.s);
        const int64_t at = (int64_t)b * p.s.F + f;
        tri[at * 2] = make_float4(t.a.x, t.a.y, t.b.x, t.b.y);
        tri[at * 2 + 1] = make_float4(t.c.x, t.c.y, 0.f, 0.f);
        box[at] = bx = t.box;
    }
    union_fold(bx, uni + b);
}

// squared distance from q to the segment a-b: d, the residual r = q - a - t (b - a), t, and the edge function cross(b - a, q - a)
__device__ __forceinline__ void seg_dist(float ax, float ay, float bx, float by, float qx, float qy, float& d, float& rx, float& ry,
                                         float& t, float& cr) {
    const float ex = bx - ax, ey = by - ay, wx = qx - ax, wy = qy - ay;
    const float ee = fmaf(ey, ey, ex * ex), ew = fmaf(ey, wy, ex * wx);
    t = ee > kMinEdge2 ? fminf(fmaxf(__fdividef(ew, ee), 0.0f), 1.0f) : 1.0f;
    rx = fmaf(-t, ex, wx);
    ry = fmaf(-t, ey, wy);
    d = fmaf(ry, ry, rx * rx);
    cr = ex * wy - ey * wx;
}

// One face at one pixel centre (qx, qy).  -> counted; e = e^(-s / sigma) (clamped), and for the backward the nearest edge m (0: a-b,
// 1: b-c, 2: c-a), its residual and t, and whether the pixel is inside.
struct FaceEval {
    float e, rx, ry, t;
    int m;
    bool inside;
};

__device__ __forceinline__ bool face_eval(const float4 r0, const float4 r1, float qx, float qy, const SilParams& p, FaceEval& o) {
    float d0, d1, d2, x0, y0, x1, y1, x2, y2, t0, t1, t2, c0, c1, c2;
    seg_dist(r0.x, r0.y, r0.z, r0.w, qx, qy, d0, x0, y0, t0, c0);
    seg_dist(r0.z, r0.w, r1.x, r1.y, qx, qy, d1, x1, y1, t1, c1);
    seg_dist(r1.x, r1.y, r0.x, r0.y, qx, qy, d2, x2, y2, t2, c2);
    o.inside = (c0 > 0.f && c1 > 0.f && c2 > 0.f) || (c0 < 0.f && c1 < 0.f && c2 < 0.f);
    float d = d0;
    o.m = 0, o.rx = x0, o.ry = y0, o.t = t0;
    if (d1 < d) d = d1, o.m = 1, o.rx = x1, o.ry = y1, o.t = t1;
    if (d2 < d) d = d2, o.m = 2, o.rx = x2, o.ry = y2, o.t = t2;
    const float x = o.inside ? d * p.c2 : -d * p.c2;  // -s / sigma in log2 units
    o.e = __builtin_amdgcn_exp2f(fminf(x, kMaxExp2));
    return o.inside || d < p.d_cut;
}

__global__ __launch_bounds__(kChunk) void sil_forward_kernel(const float4* __restrict__ tri, const int4* __restrict__ box,
                                                             const int4* __restrict__ uni, float* __restrict__ alpha,
                                                             float* __restrict__ oma, SilParams p) {
    __shared__ float4 rec[kChunk * 2];
    const int b = blockIdx.z;
    const TilePixel t = tile_pixel(p.s);
    float D = 1.0f;
    if (tile_meets(uni[b], t)) {
        const int4* bb = box + (int64_t)b * p.s.F;
        const float4* tb = tri + (int64_t)b * p.s.F * 2;
        for (int c0 = 0; c0 < p.s.F; c0 += kChunk) {
            const int total = tile_chunk(bb, p.s.F, c0, t, [&](int pos, int f, const int4&) {
                rec[pos * 2] = tb[(int64_t)f * 2];
                rec[pos * 2 + 1] = tb[(int64_t)f * 2 + 1];
            });
            if (t.live) {
                for (int k = 0; k < total; ++k) {
                    FaceEval o;
                    if (face_eval(rec[k * 2], rec[k * 2 + 1], t.qx, t.qy, p, o)) D = fminf(fmaf(D, o.e, D), kMaxProd);
                }
            }
        }
    }
    if (t.live) {
        const float om = 1.0f / D;
        const int64_t at = ((int64_t)b * p.s.H + t.i) * p.s.W + t.j;
        oma[at] = om;
        alpha[at] = 1.0f - om;
    }
}

__global__ __launch_bounds__(256) void sil_backward_kernel(const float4* __restrict__ tri, const int4* __restrict__ box,
                                                           const float* __restrict__ oma, const float* __restrict__ galpha,
                                                           float* __restrict__ frec, SilParams p) {
    const int b = blockIdx.y;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= p.s.F) return;  // wave-uniform
    const int64_t at = (int64_t)b * p.s.F + f;
    const float4 r0 = tri[at * 2], r1 = tri[at * 2 + 1];
    const float* gp = galpha + (int64_t)b * p.s.H * p.s.W;
    const float* op = oma + (int64_t)b * p.s.H * p.s.W;
    box_walk<6, kChain>(box[at], p.s.W, [&](int i, int j, int64_t px, float (&a)[6]) {
        const float G = gp[px] * op[px];
        if (G == 0.0f) return;
        FaceEval o;
        if (!face_eval(r0, r1, (float)j + 0.5f, (float)i + 0.5f, p, o)) return;
        const float pk = __fdividef(o.e, 1.0f + o.e);
        // dL/dd = -/+ G p_k kappa / sigma (outside / inside); d d / d(edge start) = -2 (1 - t) r, d d / d(edge end) = -2 t r
        const float h = (o.inside ? -2.0f : 2.0f) * G * pk * p.c;
        const float hb = h * o.t, ha = h - hb;
        const float wa = o.m == 0 ? ha : (o.m == 2 ? hb : 0.f);
        const float wb = o.m == 1 ? ha : (o.m == 0 ? hb : 0.f);
        const float wc = o.m == 2 ? ha : (o.m == 1 ? hb : 0.f);
        a[0] = fmaf(wa, o.rx, a[0]);
        a[1] = fmaf(wa, o.ry, a[1]);
        a[2] = fmaf(wb, o.rx, a[2]);
        a[3] = fmaf(wb, o.ry, a[3]);
        a[4] = fmaf(wc, o.rx, a[4]);
        a[5] = fmaf(wc, o.ry, a[5]);
    }, frec + at * 6);
}

// ---- image losses --------------------------------------------------------------------------------------------------------------
// rowsum[b][i][5] = (sum alpha, sum alpha t, sum t, i sum alpha, sum j alpha) of row i, every element converted to fp64 first
__global__ __launch_bounds__(256) void terms_rows_kernel(const float* __restrict__ alpha, const float* __restrict__ target,
                                                         int64_t t_bstride, double* __restrict__ rowsum, int H, int W) {
    __shared__ double red[4][4];
    const int b = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
    const float* a = alpha + ((int64_t)b * H + i) * W;
    const float* m = target + (int64_t)b * t_bstride + (int64_t)i * W;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = t; j < W; j += 256) {
        const double av = (double)a[j], tv = (double)m[j];
        s[0] += av;
        s[1] += av * tv;
        s[2] += tv;
        s[3] += av * (double)j;
    }
    block4_sum(s, red);
    if (t == 0) {
        double* out = rowsum + ((int64_t)b * H + i) * 5;
        out[0] = s[0];
        out[1] = s[1];
        out[2] = s[2];
        out[3] = s[0] * (double)i;
        out[4] = s[3];
    }
}

// one wave per pose: the rows by wave_fold -> sums f64 [5], mask_loss, centroid (row, col)
__global__ __launch_bounds__(64) void terms_final_kernel(const double* __restrict__ rowsum, double* __restrict__ sums,
                                                         float* __restrict__ loss, float* __restrict__ centroid, int H, int W) {
    const int b = blockIdx.x;
    double s[5];
    wave_fold(rowsum + (int64_t)b * H * 5, H, s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) sums[(int64_t)b * 5 + k] = s[k];
        const double u = s[0] + s[2];
        loss[b] = u > 0.0 ? (float)(1.0 - s[1] / u) : 1.0f;
        centroid[b * 2] = s[0] > 0.0 ? (float)(s[3] / s[0]) : 0.5f * (float)H;
        centroid[b * 2 + 1] = s[0] > 0.0 ? (float)(s[4] / s[0]) : 0.5f * (float)W;
    }
}

__global__ __launch_bounds__(256) void terms_grad_kernel(const float* __restrict__ target, int64_t t_bstride,
                                                         const double* __restrict__ sums,
                                                         const float* __restrict__ g_loss, const float* __restrict__ g_centroid,
                                                         float* __restrict__ galpha, int H, int W) {
    const int b = blockIdx.y;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)H * W) return;
    const int i = (int)(idx / W), j = (int)(idx - (int64_t)i * W);
    const double* s = sums + (int64_t)b * 5;
    const double A = s[0], I = s[1], u = s[0] + s[2];
    double g = 0.0;
    if (u > 0.0) g += (double)g_loss[b] * -((double)target[(int64_t)b * t_bstride + idx] * u - I) / (u * u);
    if (A > 0.0)
        g += ((double)g_centroid[b * 2] * ((double)i - s[3] / A) + (double)g_centroid[b * 2 + 1] * ((double)j - s[4] / A)) / A;
    galpha[(int64_t)b * H * W + idx] = (float)g;
}

}  // namespace

size_t soft_silhouette_workspace_bytes(int B, int N, int F, int H, int W) {
    if (!screen_sizes_ok(B, N, F, H, W)) return 0;
    return sil_layout(B, N, F, H, W).total;
}

static bool sil_camera_ok(float fx, float fy, float px, float py, float sigma, float blur) {
    return screen_camera_ok(fx, fy, px, py) && std::isfinite(sigma) && sigma > 0.0f && std::isfinite(blur) && blur >= 0.0f;
}

int soft_silhouette_forward(const float* verts, const int32_t* faces, int B, int N, int F, int H, int W, float fx, float fy, float px,
                            float py, float sigma, float blur, float* alpha, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!verts || !faces || !alpha || !ws) return IVLM_ERR_INVALID_ARG;
    if (!screen_sizes_ok(B, N, F, H, W) || !sil_camera_ok(fx, fy, px, py, sigma, blur)) return IVLM_ERR_UNSUPPORTED;
    const SilLayout l = sil_layout(B, N, F, H, W);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    const SilParams p = sil_params(N, F, H, W, fx, fy, px, py, sigma, blur);
    screen_forward(sil_faces_kernel, sil_forward_kernel, verts, faces, B, p.s, p, l.s, ws, alpha, ws_at<float>(ws, l.oma), st);
    return ivlm_launch_status();
}

int soft_silhouette_backward(const float* verts, const int32_t* vf_off, const int32_t* vf_list, const float* galpha, int B, int N, int F,
                             int H, int W, float fx, float fy, float px, float py, float sigma, float blur, float* gverts, void* ws,
                             size_t ws_bytes, hipStream_t st) {
    if (!verts || !vf_off || !vf_list || !galpha || !gverts || !ws) return IVLM_ERR_INVALID_ARG;
    if (!screen_sizes_ok(B, N, F, H, W) || !sil_camera_ok(fx, fy, px, py, sigma, blur)) return IVLM_ERR_UNSUPPORTED;
    const SilLayout l = sil_layout(B, N, F, H, W);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    const SilParams p = sil_params(N, F, H, W, fx, fy, px, py, sigma, blur);
    const float4* tri = ws_at<float4>(ws, l.s.tri);
    const int4* box = ws_at<int4>(ws, l.s.box);
    const float* oma = ws_at<float>(ws, l.oma);
    float* frec = ws_at<float>(ws, l.frec);
    sil_backward_kernel<<<dim3((F + 3) / 4, B), 256, 0, st>>>(tri, box, oma, galpha, frec, p);
    screen_gather_kernel<2><<<dim3((N + 255) / 256, B), 256, 0, st>>>(verts, frec, vf_off, vf_list, gverts, p.s);
    return ivlm_launch_status();
}

int silhouette_terms(const float* alpha, const float* target, int64_t t_bstride, int B, int H, int W, float* loss, float* centroid, double* sums,
                     const float* g_loss, const float* g_centroid, float* galpha, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!target || !sums || B <= 0 || H <= 0 || W <= 0 || t_bstride < 0) return IVLM_ERR_INVALID_ARG;
    if (B > 65535 || H > kMaxSide || W > kMaxSide) return IVLM_ERR_UNSUPPORTED;
    if (galpha) {  // the d / d alpha image from the sums of an earlier call
        if (!g_loss || !g_centroid) return IVLM_ERR_INVALID_ARG;
        const int64_t npx = (int64_t)H * W;
        terms_grad_kernel<<<dim3((unsigned)((npx + 255) / 256), B), 256, 0, st>>>(target, t_bstride, sums, g_loss, g_centroid, galpha, H, W);
        return ivlm_launch_status();
    }
    if (!alpha || !loss || !centroid || !ws) return IVLM_ERR_INVALID_ARG;
    if (!workspace_ok(ws, ws_bytes, IVLM_SILHOUETTE_TERMS_WORKSPACE(B, H), 8)) return IVLM_ERR_WORKSPACE;
    double* rowsum = static_cast<double*>(ws);
    terms_rows_kernel<<<dim3(H, B), 256, 0, st>>>(alpha, target, t_bstride, rowsum, H, W);
    terms_final_kernel<<<B, 64, 0, st>>>(rowsum, sums, loss, centroid, H, W);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_soft_silhouette_workspace_bytes(int B, int N, int F, int H, int W) {
    return ivlm::soft_silhouette_workspace_bytes(B, N, F, H, W);
}
int ivlm_soft_silhouette_forward(const float* verts, const int32_t* faces, int B, int N, int F, int H, int W, float fx, float fy,
                                 float px, float py, float sigma, float blur_radius, float* alpha_out, void* workspace,
                                 size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::soft_silhouette_forward(verts, faces, B, N, F, H, W, fx, fy, px, py, sigma, blur_radius, alpha_out, workspace,
                                         workspace_bytes, ivlm_stream(s));
}
int ivlm_soft_silhouette_backward(const float* verts, const int32_t* vert_face_offsets, const int32_t* vert_face_list,
                                  const float* grad_alpha, int B, int N, int F, int H, int W, float fx, float fy, float px, float py,
                                  float sigma, float blur_radius, float* grad_verts_out, void* workspace, size_t workspace_bytes,
                                  ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::soft_silhouette_backward(verts, vert_face_offsets, vert_face_list, grad_alpha, B, N, F, H, W, fx, fy, px, py, sigma,
                                          blur_radius, grad_verts_out, workspace, workspace_bytes, ivlm_stream(s));
}
int ivlm_silhouette_terms(const float* alpha, const float* target, int64_t target_batch_stride, int B, int H, int W, float* loss_out, float* centroid_out,
                          double* sums, const float* g_loss, const float* g_centroid, float* grad_alpha_out, void* workspace,
                          size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::silhouette_terms(alpha, target, target_batch_stride, B, H, W, loss_out, centroid_out, sums, g_loss, g_centroid, grad_alpha_out, workspace,
                                  workspace_bytes, ivlm_stream(s));
}
}
