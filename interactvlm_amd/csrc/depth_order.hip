// The z-buffer of a posed triangle mesh in the camera of silhouette.hip, and the depth-order term built on it (NOT the reference's:
// PHOSA's ordinal-depth loss on the object's own z-buffer against a constant occluder depth image).
//
//   projection   u = fx X / Z + px, v = fy Y / Z + py (OpenCV pinhole); pixel (row i, col j) has its centre q at (j + 0.5, i + 0.5)
//   per face k   with screen vertices a, b, c:  e_a = cross(c - b, q - b), e_b = cross(a - c, q - c), e_c = cross(b - a, q - a); the face
//                covers the pixel when the three are all > 0 or all < 0 (strict; both windings count, nothing is culled)
//                z_k = s / (e_a / Z_a + e_b / Z_b + e_c / Z_c), s = e_a + e_b + e_c: the perspective-correct depth 1 / sum_i (w_i / Z_i)
//                with the screen-space barycentrics w_i = e_i / s
//   a face is skipped whole when its screen area is zero or any of its vertices has Z <= 1e-6 (or an index outside [0, N))
//   depth = min_k z_k over the covering faces (+inf: none), face_id = the face that attains it, the lowest index among equals (-1: none)
//
//   depth order  x = sign(c) (D_o - D_h) / tau at pixels with c != 0 and D_o, D_h both finite;  L = (tau / n) sum |c| softplus(x),
//                n = sum |c| over the whole image; softplus(x) = max(x, 0) + log1p(exp(-|x|)); L = 0 exactly when n == 0
//   backward     the winner held fixed: dL/dD_o = c sigmoid(x) / n, then d z / d e_i = n_i / t^2 with t = sum_j e_j / Z_j and
//                n_i = sum_j e_j (Z_i - Z_j) / (Z_i Z_j) (the difference of the depths is taken first: it is what is left of t - s / Z_i
//                after the cancellation), d z / d Z_i = z e_i / (t Z_i^2), the e_i to the six screen coordinates, the projection.
//                Nothing flows through the coverage edge or through D_h.
//
// Launches (the caller's stream, no atomics on floats, every sum in a fixed order: the same bits every call, for a pose whatever the
// batch around it; built with -ffp-contract=off, so every fp32 operation below - and of screen_common.h's walk, shared with
// silhouette.hip, as it is compiled into this file - is the one that is written):
//   screen_project    per vertex (u, v); resets the pose's union box
//   dep_faces         screen_face without growth; per face three float4 (a, b | c, 1 / Z_a, 1 / Z_b | 1 / Z_c, Z_a, Z_b, Z_c) and its
//                     box; union_fold
//   dep_forward       tile_chunk: the records of the faces that meet the tile go to LDS with their index and box, then every lane
//                     reads the same record and, at the pixels of the face's own box (the pixels the backward walks), keeps (z, k)
//                     under a strict <, so equal depths stay with the lowest index
//   dord_rows / dord_final   per image row the fp64 sums (sum |c| softplus, sum |c|), every pixel converted to fp64 before it is added
//                     (block4_sum), then the rows by wave_fold; the value and (S, n) per pose
//   dord_backward     box_walk<9>: at the pixels the face won it recomputes the e_i and adds to the [3, 3] record (du, dv, dZ direct
//                     per corner), IVLM_DEPTH_ORDER_CHAIN fp32 additions per lane
//   screen_gather<3>  per vertex: the records of its incident faces (the CSR lists of the silhouette), chained through the
//                     projection to dL/d(X, Y, Z)
#include <algorithm>
#include <cmath>

#include "screen_common.h"

namespace ivlm {
namespace {

constexpr int kChain = IVLM_DEPTH_ORDER_CHAIN;   // fp32 additions per lane before the fp64 accumulators take over

// workspace carves, shared by the size queries and the launchers
struct DepLayout {
    ScreenLayout s;
    size_t depth, fid, frec, rows, sums, total;
};

DepLayout dep_layout(int B, int N, int F, int H, int W, bool order) {
    DepLayout l = {};
    Carve c;
    l.s = screen_layout(c, B, N, F, 48);
    if (order) {
        l.depth = c.take((size_t)B * H * W * 4);
        l.fid = c.take((size_t)B * H * W * 4);
        l.frec = c.take((size_t)B * F * 36);
        l.rows = c.take((size_t)B * H * 16);
        l.sums = c.take((size_t)B * 16);
    }
    l.total = c.off;
    return l;
}

__global__ __launch_bounds__(256) void dep_faces_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                        const float2* __restrict__ uv, float4* __restrict__ tri,
                                                        int4* __restrict__ box, int4* __restrict__ uni, ScreenParams p) {
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    int4 bx = make_int4(p.W, p.H, -1, -1);  // empty
    if (f < p.F) {
        const ScreenFace t = screen_face(verts, faces, uv, b, f, 0.0f, p);
        const int64_t at = (int64_t)b * p.F + f;
        tri[at * 3] = make_float4(t.a.x, t.a.y, t.b.x, t.b.y);
        tri[at * 3 + 1] = make_float4(t.c.x, t.c.y, 1.0f / t.za, 1.0f / t.zb);
        tri[at * 3 + 2] = make_float4(1.0f / t.zc, t.za, t.zb, t.zc);
        box[at] = bx = t.box;
    }
    union_fold(bx, uni + b);
}

// the three edge functions of a face (r0 = a, b; c = (cx, cy)) at the pixel centre (qx, qy) -> covered
__device__ __forceinline__ bool edge_functions(const float4 r0, float cx, float cy, float qx, float qy, float& ea, float& eb, float& ec) {
    ea = (cx - r0.z) * (qy - r0.w) - (cy - r0.w) * (qx - r0.z);
    eb = (r0.x - cx) * (qy - cy) - (r0.y - cy) * (qx - cx);
    ec = (r0.z - r0.x) * (qy - r0.y) - (r0.w - r0.y) * (qx - r0.x);
    return (ea > 0.f && eb > 0.f && ec > 0.f) || (ea < 0.f && eb < 0.f && ec < 0.f);
}

__global__ __launch_bounds__(kChunk) void dep_forward_kernel(const float4* __restrict__ tri, const int4* __restrict__ box,
                                                             const int4* __restrict__ uni, float* __restrict__ depth,
                                                             int32_t* __restrict__ face_id, ScreenParams p) {
    __shared__ float4 rec[kChunk * 2];
    __shared__ float rec_izc[kChunk];
    __shared__ int rec_f[kChunk];
    __shared__ int4 rec_box[kChunk];
    const int b = blockIdx.z;
    const TilePixel t = tile_pixel(p);
    float best = INFINITY;
    int who = -1;
    if (tile_meets(uni[b], t)) {
        const int4* bb = box + (int64_t)b * p.F;
        const float4* tb = tri + (int64_t)b * p.F * 3;
        for (int c0 = 0; c0 < p.F; c0 += kChunk) {
            const int total = tile_chunk(bb, p.F, c0, t, [&](int pos, int f, const int4& bx) {
                rec[pos * 2] = tb[(int64_t)f * 3];
                rec[pos * 2 + 1] = tb[(int64_t)f * 3 + 1];
                rec_izc[pos] = tb[(int64_t)f * 3 + 2].x;
                rec_f[pos] = f;
                rec_box[pos] = bx;
            });
            if (t.live) {
                for (int k = 0; k < total; ++k) {
                    // only inside the face's own box, which is all that dord_backward walks: the two kernels see the same pixels
                    // (| and not ||: one 16-byte LDS read and one branch instead of a dependent read per comparison)
                    const int4 kb = rec_box[k];
                    if ((t.j < kb.x) | (t.j > kb.z) | (t.i < kb.y) | (t.i > kb.w)) continue;
                    const float4 r0 = rec[k * 2], r1 = rec[k * 2 + 1];
                    float ea, eb, ec;
                    if (!edge_functions(r0, r1.x, r1.y, t.qx, t.qy, ea, eb, ec)) continue;
                    const float s = (ea + eb) + ec;
                    const float tt = (ea * r1.z + eb * r1.w) + ec * rec_izc[k];
                    const float z = s / tt;
                    if (z < best) best = z, who = rec_f[k];  // ascending face order and a strict <: equal depths stay with the lowest index
                }
            }
        }
    }
    if (t.live) {
        const int64_t at = ((int64_t)b * p.H + t.i) * p.W + t.j;
        depth[at] = best;
        face_id[at] = who;
    }
}

// x = sign(c) (D_o - D_h) / tau where the pixel counts -> true
__device__ __forceinline__ bool order_argument(float c, float d_o, float d_h, float tau, float& x) {
    if (c == 0.0f || !(fabsf(d_o) < INFINITY) || !(fabsf(d_h) < INFINITY)) return false;
    const float d = d_o - d_h;
    x = (c > 0.0f ? d : -d) / tau;
    return true;
}

// rowsum[b][i][2] = (sum |c| softplus(x), sum |c|) of row i, every element converted to fp64 first
__global__ __launch_bounds__(256) void dord_rows_kernel(const float* __restrict__ depth, const float* __restrict__ occ,
                                                        const float* __restrict__ cw, float tau, double* __restrict__ rowsum, int H,
                                                        int W) {
    __shared__ double red[4][2];
    const int b = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
    const float* d = depth + ((int64_t)b * H + i) * W;
    const float* o = occ + (int64_t)i * W;
    const float* c = cw + (int64_t)i * W;
    double s[2] = {0.0, 0.0};
    for (int j = t; j < W; j += 256) {
        const float cv = c[j];
        s[1] += (double)fabsf(cv);
        float x;
        if (order_argument(cv, d[j], o[j], tau, x)) {
            const float sp = fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
            s[0] += (double)(fabsf(cv) * sp);
        }
    }
    block4_sum(s, red);
    if (t == 0) {
        rowsum[((int64_t)b * H + i) * 2] = s[0];
        rowsum[((int64_t)b * H + i) * 2 + 1] = s[1];
    }
}

// one wave per pose: the rows by wave_fold -> sums f64 [2] = (S, n), value = (tau / n) S (an exact 0 when n == 0)
__global__ __launch_bounds__(64) void dord_final_kernel(const double* __restrict__ rowsum, double* __restrict__ sums,
                                                        float* __restrict__ value, float tau, int H) {
    const int b = blockIdx.x;
    double s[2];
    wave_fold(rowsum + (int64_t)b * H * 2, H, s);
    if (threadIdx.x == 0) {
        sums[(int64_t)b * 2] = s[0];
        sums[(int64_t)b * 2 + 1] = s[1];
        value[b] = s[1] > 0.0 ? (float)((double)tau / s[1] * s[0]) : 0.0f;
    }
}

__global__ __launch_bounds__(256) void dord_backward_kernel(const float4* __restrict__ tri, const int4* __restrict__ box,
                                                            const float* __restrict__ depth, const int32_t* __restrict__ face_id,
                                                            const float* __restrict__ occ, const float* __restrict__ cw,
                                                            const double* __restrict__ sums, const float* __restrict__ gvalue,
                                                            float tau, float* __restrict__ frec, ScreenParams p) {
    const int b = blockIdx.y;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= p.F) return;  // wave-uniform
    const int64_t at = (int64_t)b * p.F + f;
    const float4 r0 = tri[at * 3], r1 = tri[at * 3 + 1], r2 = tri[at * 3 + 2];
    const float* dp = depth + (int64_t)b * p.H * p.W;
    const int32_t* fp = face_id + (int64_t)b * p.H * p.W;
    const double n = sums[(int64_t)b * 2 + 1];
    const float gn = n > 0.0 ? (float)((double)gvalue[b] / n) : 0.0f;  // dL/dD_o = gn c sigmoid(x)
    // 1 / Z_j - 1 / Z_i = (Z_i - Z_j) / (Z_i Z_j), the difference of the depths taken first
    const float dab = (r2.y - r2.z) * (r1.z * r1.w), dac = (r2.y - r2.w) * (r1.z * r2.x), dbc = (r2.z - r2.w) * (r1.w * r2.x);
    box_walk<9, kChain>(box[at], p.W, [&](int i, int j, int64_t px, float (&a)[9]) {
        if (fp[px] != f) return;
        const float cv = cw[px];
        float x;
        if (!order_argument(cv, dp[px], occ[px], tau, x)) return;
        const float ex = expf(-fabsf(x));
        const float sg = (x >= 0.0f ? 1.0f : ex) / (1.0f + ex);
        const float G = (gn * cv) * sg;
        if (G == 0.0f) return;
        const float qx = (float)j + 0.5f, qy = (float)i + 0.5f;
        float ea, eb, ec;
        edge_functions(r0, r1.x, r1.y, qx, qy, ea, eb, ec);  // (covered: the forward kernel evaluated these very operations)
        const float s = (ea + eb) + ec;
        const float tt = (ea * r1.z + eb * r1.w) + ec * r2.x;
        const float z = s / tt;
        const float h = G / (tt * tt);
        const float ga = h * (eb * dab + ec * dac);    // G dz/de_a, n_a = e_b (1/Z_b - 1/Z_a) + e_c (1/Z_c - 1/Z_a)
        const float gb = h * (ec * dbc - ea * dab);
        const float gc = h * (-(ea * dac) - eb * dbc);
        const float k = (G * z) / tt;                  // G dz/dZ_i = k e_i / Z_i^2
        a[0] += gb * (qy - r1.y) + gc * (r0.w - qy);   // a: the end of edge c -> a (e_b), the start of a -> b (e_c)
        a[1] += gb * (r1.x - qx) + gc * (qx - r0.z);
        a[2] += k * (ea * (r1.z * r1.z));
        a[3] += gc * (qy - r0.y) + ga * (r1.y - qy);   // b: the end of a -> b (e_c), the start of b -> c (e_a)
        a[4] += gc * (r0.x - qx) + ga * (qx - r1.x);
        a[5] += k * (eb * (r1.w * r1.w));
        a[6] += ga * (qy - r0.w) + gb * (r0.y - qy);   // c: the end of b -> c (e_a), the start of c -> a (e_b)
        a[7] += ga * (r0.z - qx) + gb * (qx - r0.x);
        a[8] += k * (ec * (r2.x * r2.x));
    }, frec + at * 9);
}

}  // namespace

size_t depth_image_workspace_bytes(int B, int N, int F, int H, int W) {
    if (!screen_sizes_ok(B, N, F, H, W)) return 0;
    return dep_layout(B, N, F, H, W, false).total;
}

size_t depth_order_workspace_bytes(int B, int N, int F, int H, int W) {
    if (!screen_sizes_ok(B, N, F, H, W)) return 0;
    return dep_layout(B, N, F, H, W, true).total;
}

int depth_image(const float* verts, const int32_t* faces, int B, int N, int F, int H, int W, float fx, float fy, float px, float py,
                float* depth, int32_t* face_id, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!verts || !faces || !depth || !face_id || !ws) return IVLM_ERR_INVALID_ARG;
    if (!screen_sizes_ok(B, N, F, H, W) || !screen_camera_ok(fx, fy, px, py)) return IVLM_ERR_UNSUPPORTED;
    const DepLayout l = dep_layout(B, N, F, H, W, false);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    const ScreenParams p = {fx, fy, px, py, N, F, H, W};
    screen_forward(dep_faces_kernel, dep_forward_kernel, verts, faces, B, p, p, l.s, ws, depth, face_id, st);
    return ivlm_launch_status();
}

static bool tau_ok(float tau) { return std::isfinite(tau) && tau > 0.0f; }

int depth_order_forward(const float* verts, const int32_t* faces, const float* occ, const float* cw, int B, int N, int F, int H, int W,
                        float fx, float fy, float px, float py, float tau, float* value, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!verts || !faces || !occ || !cw || !value || !ws) return IVLM_ERR_INVALID_ARG;
    if (!screen_sizes_ok(B, N, F, H, W) || !screen_camera_ok(fx, fy, px, py) || !tau_ok(tau)) return IVLM_ERR_UNSUPPORTED;
    const DepLayout l = dep_layout(B, N, F, H, W, true);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    float* depth = ws_at<float>(ws, l.depth);
    double* rows = ws_at<double>(ws, l.rows);
    const ScreenParams p = {fx, fy, px, py, N, F, H, W};
    screen_forward(dep_faces_kernel, dep_forward_kernel, verts, faces, B, p, p, l.s, ws, depth, ws_at<int32_t>(ws, l.fid), st);
    dord_rows_kernel<<<dim3(H, B), 256, 0, st>>>(depth, occ, cw, tau, rows, H, W);
    dord_final_kernel<<<B, 64, 0, st>>>(rows, ws_at<double>(ws, l.sums), value, tau, H);
    return ivlm_launch_status();
}

int depth_order_backward(const float* verts, const int32_t* vf_off, const int32_t* vf_list, const float* occ, const float* cw,
                         const float* gvalue, int B, int N, int F, int H, int W, float fx, float fy, float px, float py, float tau,
                         float* gverts, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!verts || !vf_off || !vf_list || !occ || !cw || !gvalue || !gverts || !ws) return IVLM_ERR_INVALID_ARG;
    if (!screen_sizes_ok(B, N, F, H, W) || !screen_camera_ok(fx, fy, px, py) || !tau_ok(tau)) return IVLM_ERR_UNSUPPORTED;
    const DepLayout l = dep_layout(B, N, F, H, W, true);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    const ScreenParams p = {fx, fy, px, py, N, F, H, W};
    float* frec = ws_at<float>(ws, l.frec);
    dord_backward_kernel<<<dim3((F + 3) / 4, B), 256, 0, st>>>(ws_at<float4>(ws, l.s.tri), ws_at<int4>(ws, l.s.box), ws_at<float>(ws, l.depth),
                                                               ws_at<int32_t>(ws, l.fid), occ, cw, ws_at<double>(ws, l.sums), gvalue, tau,
                                                               frec, p);
    screen_gather_kernel<3><<<dim3((N + 255) / 256, B), 256, 0, st>>>(verts, frec, vf_off, vf_list, gverts, p);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_depth_image_workspace_bytes(int B, int N, int F, int H, int W) { return ivlm::depth_image_workspace_bytes(B, N, F, H, W); }
int ivlm_depth_image(const float* verts, const int32_t* faces, int B, int N, int F, int H, int W, float fx, float fy, float px, float py,
                     float* depth_out, int32_t* face_id_out, void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::depth_image(verts, faces, B, N, F, H, W, fx, fy, px, py, depth_out, face_id_out, workspace, workspace_bytes,
                             ivlm_stream(s));
}
size_t ivlm_depth_order_workspace_bytes(int B, int N, int F, int H, int W) { return ivlm::depth_order_workspace_bytes(B, N, F, H, W); }
int ivlm_depth_order_forward(const float* verts, const int32_t* faces, const float* occluder_depth, const float* signed_weight, int B,
                             int N, int F, int H, int W, float fx, float fy, float px, float py, float tau, float* value_out,
                             void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::depth_order_forward(verts, faces, occluder_depth, signed_weight, B, N, F, H, W, fx, fy, px, py, tau, value_out,
                                     workspace, workspace_bytes, ivlm_stream(s));
}
int ivlm_depth_order_backward(const float* verts, const int32_t* vert_face_offsets, const int32_t* vert_face_list,
                              const float* occluder_depth, const float* signed_weight, const float* grad_value, int B, int N, int F, int H,
                              int W, float fx, float fy, float px, float py, float tau, float* grad_verts_out, void* workspace,
                              size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::depth_order_backward(verts, vert_face_offsets, vert_face_list, occluder_depth, signed_weight, grad_value, B, N, F, H, W,
                                      fx, fy, px, py, tau, grad_verts_out, workspace, workspace_bytes, ivlm_stream(s));
}
}
