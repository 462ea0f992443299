// Signed distance to a closed triangle mesh and the penetration term of the object-pose fit (NOT the reference's: its
// ObjPose_Opt.forward has three terms and none of them knows inside from outside).
//
//   c(x)  closest point of the surface, per face by Ericson's region classification;  d(x) = |x - c(x)|
//   k(x)  a face that attains d(x): among faces whose fp32 squared distance compares equal, the lowest index
//   w(x)  = (1 / 4 pi) sum_f Omega_f(x), Omega_f = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|),
//           a, b, c = v0 - x, v1 - x, v2 - x (Van Oosterom - Strackee);  inside(x) <=> w(x) > 0.5;  sdf = -d inside, +d outside
//   L     = (1 / N) sum_i inside(x_i) d(x_i)^2,  dL/dx_i = inside(x_i) 2 (x_i - c(x_i)) / N;  no gradient to the mesh
//   a face of zero area (fp32 cross product of its edges exactly 0) contributes to neither sum
//
// The plan (ivlm_mesh_sdf_prepare): a 256-byte header {face and chunk counts, the bounding box of the vertices} and one 48-byte
// record per face, {v0, v1, v2, mark, 0, 0} as three float4; mark = 0 for a zero-area face (or one that names a vertex out of range).
//
// Kernels (no atomics, every sum in a fixed order, nothing depends on B or on a pose's place in the batch):
//   sdf_sweep<WIND, CLOSE>  the hot kernel.  One wave per block, one point per lane in registers, against one CHUNK of faces,
//                  staged TILE records at a time in LDS and read by all lanes at one address (three broadcast ds_read_b128 per
//                  face).  One pass over a face serves the solid angle and the closest-point test: both start from a, b, c.  Per
//                  (point, chunk) it writes {q = c - x, |q|^2} , the face and the fp32 sum of atan2 over the chunk.
//   sdf_query_fold per point: the chunk partials in chunk order - strict '<' keeps the lower face on equal d^2, the winding sum
//                  in fp64 - and the four outputs.
//   penetration    sdf_compact<0>: the points inside the bounding box, in index order, per pose (block_compact of fit_common.h);
//                  sdf_sweep<1,0> over them;  sdf_compact<1>: folds their winding sums and keeps the inside ones;  sdf_sweep<0,1>
//                  over those;  sdf_pen_fold: the gradient rows and the fp64 sum of d^2 per block of 256 (block4_sum);
//                  sdf_pen_value: the block sums by wave_fold, / N, rounded once.  The gradient is zeroed first, so every other
//                  row is an exact 0; a pose with no point in the box runs no sweep (all its blocks leave at once).
//
//   intrusion      the other direction: the plan is the OBJECT, the points are the human's vertices h [N,3], shared by B poses
//                  (rot6d, t, s), y = (s v) R + t.  sdf_unpose: R by rot6d.h's Gram-Schmidt in fp64, rounded to fp32 once, then per
//                  point in fp32 u = h - t, x_i = ((u_0 R_i0 + u_1 R_i1) + u_2 R_i2) / s -> x [B,N,3] in the workspace;  the four
//                  kernels of the penetration, unchanged, with x as the points;  sdf_intrusion_fold: per inside point, in fp64,
//                  c = x + q, e = -s (q R) (from q: h - (s c R + t) cancels) and the 14 sums {s^2 dd, e, e.(c R), c_i e_k} per block
//                  of 256 (block4_sum);  sdf_intrusion_finish: one wave per pose, wave_fold over the blocks, the factors
//                  dL/dt = -(2/N) sum e, dL/ds = -(2/N) sum e.(cR), dL/dR_ik = -(2 s/N) sum c_i e_k and rot6d.h's chain, each
//                  output rounded once.  The value's sum has the order of sdf_pen_fold / sdf_pen_value: at the identity pose x == h
//                  and the value is the penetration's bit for bit.  A pose with s not > 0 gets NaN (its x is NaN: no sweep).
//
// The query, penetration and intrusion calls are not told F: it lives in the plan, on the device.  The host derives from
// workspace_bytes how many chunks the workspace holds (Cw), sizes the grid by it and lays the partials out by it; the kernels read
// the plan's chunk count C and sweep only when C <= Cw; otherwise the folds write NaN (face -1) and nothing is read or written past
// the workspace.  A workspace of ivlm_mesh_sdf_workspace_bytes(B, N, F) gives Cw == C.
//
// Built with -ffp-contract=off: each fp32 operation is the one tests/_mesh_sdf_ref.py states, so the tolerance constants measured
// with its fp32 mode describe this arithmetic, apart from the device's sqrt / atan2 and the order of the winding sum.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "fit_common.h"
#include "rot6d.h"

namespace ivlm {
namespace {

constexpr int kTile = IVLM_MESH_SDF_TILE;    // faces per LDS tile
constexpr int kChunk = IVLM_MESH_SDF_CHUNK;  // faces per grid chunk
constexpr int kWave = 64;                    // threads (= points) of a sweep block
constexpr int kFold = 256;                   // threads (= points) of a fold block
constexpr int kMaxN = 1 << 20;
constexpr int kMaxF = 1 << 22;
constexpr int kMagic = 0x53444631;           // "SDF1"
static_assert(kChunk % kTile == 0, "a chunk is a whole number of tiles");

struct SdfHeader {  // 256 bytes at the head of the plan
    int32_t magic, n_verts, n_faces, n_chunks;
    float lo[3], hi[3];
    int32_t pad[54];
};
static_assert(sizeof(SdfHeader) == 256, "plan header");

// workspace carve for a capacity of C chunks
struct SdfLayout {
    size_t cnt, list[2], blockval, p4, pf, pw, total;
    int nb;  // fold blocks per pose
};

SdfLayout sdf_layout(int B, int N, int C) {
    SdfLayout l;
    Carve c;
    l.nb = (N + kFold - 1) / kFold;
    l.cnt = c.take((size_t)2 * B * 4);
    l.list[0] = c.take((size_t)B * N * 4);
    l.list[1] = c.take((size_t)B * N * 4);
    l.blockval = c.take((size_t)B * l.nb * 8);
    l.p4 = c.take((size_t)C * B * N * 16);
    l.pf = c.take((size_t)C * B * N * 4);
    l.pw = c.take((size_t)C * B * N * 4);
    l.total = c.off;
    return l;
}

// the largest chunk capacity a workspace of ws_bytes holds (0: not even one)
int sdf_capacity(int B, int N, size_t ws_bytes) {
    const size_t fixed = sdf_layout(B, N, 0).total;
    if (ws_bytes <= fixed) return 0;
    size_t c = (ws_bytes - fixed) / ((size_t)24 * B * N);
    c = std::min(c, (size_t)(kMaxF / kChunk));
    while (c > 0 && sdf_layout(B, N, (int)c).total > ws_bytes) --c;
    return (int)c;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sdf_records_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int n_verts,
                                                          int n_faces, float4* __restrict__ rec) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    float v[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float mark = 0.0f;
    if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {
        const int id[3] = {i0, i1, i2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[3 * c] = verts[3 * (int64_t)id[c]];
            v[3 * c + 1] = verts[3 * (int64_t)id[c] + 1];
            v[3 * c + 2] = verts[3 * (int64_t)id[c] + 2];
        }
        const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
        const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        mark = (nx != 0.0f || ny != 0.0f || nz != 0.0f) ? 1.0f : 0.0f;  // (a NaN corner also leaves a mark: it then shows in the results)
    }
    rec[3 * (int64_t)f] = make_float4(v[0], v[1], v[2], v[3]);
    rec[3 * (int64_t)f + 1] = make_float4(v[4], v[5], v[6], v[7]);
    rec[3 * (int64_t)f + 2] = make_float4(v[8], mark, 0.0f, 0.0f);
}

// one block: the header, with the bounding box of all vertices (min and max do not depend on the order)
__global__ __launch_bounds__(1024) void sdf_header_kernel(const float* __restrict__ verts, int n_verts, int n_faces, SdfHeader* __restrict__ hdr) {
    __shared__ float red[16][6];
    const int t = threadIdx.x;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = t; i < n_verts; i += 1024) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = verts[3 * (int64_t)i + c];
            lo[c] = fminf(lo[c], x);
            hi[c] = fmaxf(hi[c], x);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
        }
        if ((t & 63) == 0) {
            red[t >> 6][c] = lo[c];
            red[t >> 6][3 + c] = hi[c];
        }
    }
    __syncthreads();
    if (t == 0) {
        hdr->magic = kMagic;
        hdr->n_verts = n_verts;
        hdr->n_faces = n_faces;
        hdr->n_chunks = (n_faces + kChunk - 1) / kChunk;
        for (int c = 0; c < 3; ++c) {
            float a = red[0][c], b = red[0][3 + c];
            for (int v = 1; v < 16; ++v) {
                a = fminf(a, red[v][c]);
                b = fmaxf(b, red[v][3 + c]);
            }
            hdr->lo[c] = a;
            hdr->hi[c] = b;
        }
        for (int i = 0; i < 54; ++i) hdr->pad[i] = 0;
    }
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------
struct SweepArgs {
    const SdfHeader* hdr;
    const float4* rec;
    const float* points;   // [B,N,3]
    const int32_t* list;   // [B,N] indices of the points to serve, or null: every point
    const int32_t* count;  // [B] entries of list, or null: N
    float4* p4;            // [B,Cw,N] {q, |q|^2}
    int32_t* pf;           // [B,Cw,N] face
    float* pw;             // [B,Cw,N] sum of atan2 over the chunk
    int N, Cw;
};

template <bool WIND, bool CLOSE>
__global__ __launch_bounds__(kWave) void sdf_sweep_kernel(SweepArgs s) {
    __shared__ float4 tile[3 * kTile];
    const int lane = threadIdx.x, chunk = blockIdx.y, b = blockIdx.z;
    const int C = s.hdr->n_chunks, F = s.hdr->n_faces;
    const int m = s.count ? s.count[b] : s.N;
    const int k = blockIdx.x * kWave + lane;
    if (C > s.Cw || chunk >= C || (int)blockIdx.x * kWave >= m) return;  // block-uniform
    const bool live = k < m;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
        const int i = s.list ? s.list[(int64_t)b * s.N + k] : k;
        const float* p = s.points + ((int64_t)b * s.N + i) * 3;
        px = p[0];
        py = p[1];
        pz = p[2];
    }
    float wsum = 0.0f, best = FLT_MAX, qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int bface = -1;
    const int f_end = min(F, (chunk + 1) * kChunk);
    for (int f0 = chunk * kChunk; f0 < f_end; f0 += kTile) {
        const int nf = min(kTile, f_end - f0);
        __syncthreads();  // the tile of the round before has been read
        for (int j = lane; j < 3 * nf; j += kWave) tile[j] = s.rec[3 * (int64_t)f0 + j];
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < nf; ++j) {
            const float4 r0 = tile[3 * j], r1 = tile[3 * j + 1], r2 = tile[3 * j + 2];
            if (r2.y == 0.0f) continue;  // a zero-area face: the same for all lanes
            const float ax = r0.x - px, ay = r0.y - py, az = r0.z - pz;
            const float bx = r0.w - px, by = r1.x - py, bz = r1.y - pz;
            const float cx = r1.z - px, cy = r1.w - py, cz = r2.x - pz;
            if constexpr (WIND) {
                const float ux = by * cz - bz * cy, uy = bz * cx - bx * cz, uz = bx * cy - by * cx;
                const float num = (ax * ux + ay * uy) + az * uz;
                const float la = sqrtf((ax * ax + ay * ay) + az * az);
                const float lb = sqrtf((bx * bx + by * by) + bz * bz);
                const float lc = sqrtf((cx * cx + cy * cy) + cz * cz);
                const float ab = (ax * bx + ay * by) + az * bz;
                const float ac = (ax * cx + ay * cy) + az * cz;
                const float bc = (bx * cx + by * cy) + bz * cz;
                const float den = (((la * lb) * lc + ab * lc) + ac * lb) + bc * la;
                wsum += atan2f(num, den);
            }
            if constexpr (CLOSE) {
                const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
                const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
                const float d1 = -((e1x * ax + e1y * ay) + e1z * az), d2 = -((e2x * ax + e2y * ay) + e2z * az);
                const float d3 = -((e1x * bx + e1y * by) + e1z * bz), d4 = -((e2x * bx + e2y * by) + e2z * bz);
                const float d5 = -((e1x * cx + e1y * cy) + e1z * cz), d6 = -((e2x * cx + e2y * cy) + e2z * cz);
                const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
                const float d43 = d4 - d3, d56 = d5 - d6;
                // barycentric (v, w) of the closest point as (nv, nw) / dn; Ericson's early returns, the last override wins
                float nv = vb, nw = vc, dn = (va + vb) + vc;                          // the face's interior
                if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) nv = d56, nw = d43, dn = d43 + d56;  // edge bc
                if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) nv = 0.0f, nw = d2, dn = d2 - d6;      // edge ac
                if (d6 >= 0.0f && d5 <= d6) nv = 0.0f, nw = 1.0f, dn = 1.0f;                       // corner c
                if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) nv = d1, nw = 0.0f, dn = d1 - d3;      // edge ab
                if (d3 >= 0.0f && d4 <= d3) nv = 1.0f, nw = 0.0f, dn = 1.0f;                       // corner b
                if (d1 <= 0.0f && d2 <= 0.0f) nv = 0.0f, nw = 0.0f, dn = 1.0f;                     // corner a
                const float inv = 1.0f / dn;
                const float v = nv * inv, w = nw * inv;
                const float tx = (ax + e1x * v) + e2x * w, ty = (ay + e1y * v) + e2y * w, tz = (az + e1z * v) + e2z * w;
                const float dd = (tx * tx + ty * ty) + tz * tz;
                if (dd < best) {  // strict: the lower face index stays on equal d^2
                    best = dd;
                    bface = f0 + j;
                    qx = tx;
                    qy = ty;
                    qz = tz;
                }
            }
        }
    }
    if (live) {
        const int64_t at = ((int64_t)b * s.Cw + chunk) * s.N + k;
        if constexpr (WIND) s.pw[at] = wsum;
        if constexpr (CLOSE) {
            s.p4[at] = make_float4(qx, qy, qz, best);
            s.pf[at] = bface;
        }
    }
}

__device__ __forceinline__ float fold_winding(const SweepArgs& s, int C, int b, int k) {
    double w = 0.0;
    for (int c = 0; c < C; ++c) w += (double)s.pw[((int64_t)b * s.Cw + c) * s.N + k];
    return (float)(w * 0.15915494309189535);  // sum of atan2 = sum Omega / 2;  / (2 pi)
}

__device__ __forceinline__ void fold_closest(const SweepArgs& s, int C, int b, int k, float4& q, int& face) {
    q = make_float4(0.0f, 0.0f, 0.0f, FLT_MAX);
    face = -1;
    for (int c = 0; c < C; ++c) {
        const int64_t at = ((int64_t)b * s.Cw + c) * s.N + k;
        const float4 v = s.p4[at];
        if (v.w < q.w) {  // chunk order and strict: the lower face index stays on equal d^2
            q = v;
            face = s.pf[at];
        }
    }
}

__global__ __launch_bounds__(kFold) void sdf_query_fold_kernel(SweepArgs s, float* __restrict__ sdf, float* __restrict__ closest,
                                                               int32_t* __restrict__ face, float* __restrict__ winding) {
    const int b = blockIdx.y, k = blockIdx.x * kFold + threadIdx.x;
    if (k >= s.N) return;
    const int C = s.hdr->n_chunks;
    const int64_t o = (int64_t)b * s.N + k;
    float w = NAN, d = NAN;
    float4 q = make_float4(NAN, NAN, NAN, NAN);
    int fc = -1;
    if (C <= s.Cw) {
        w = fold_winding(s, C, b, k);
        fold_closest(s, C, b, k, q, fc);
        d = fc >= 0 ? sqrtf(q.w) : INFINITY;
    }
    if (sdf) sdf[o] = w > 0.5f ? -d : d;
    if (closest) {
        closest[3 * o] = s.points[3 * o] + q.x;
        closest[3 * o + 1] = s.points[3 * o + 1] + q.y;
        closest[3 * o + 2] = s.points[3 * o + 2] + q.z;
    }
    if (face) face[o] = fc;
    if (winding) winding[o] = w;
}

// ---- penetration ----------------------------------------------------------------------------------------------------------------
// One block per pose.  MODE 0: keep the points inside the bounding box (out = list 0);  MODE 1: of the entries of list 0, keep
// those whose folded winding number says inside (out = list 1).  Index order is kept.
template <int MODE>
__global__ __launch_bounds__(1024) void sdf_compact_kernel(SweepArgs s, const int32_t* __restrict__ in_list, const int32_t* __restrict__ in_count,
                                                           int32_t* __restrict__ out_list, int32_t* __restrict__ out_count) {
    __shared__ int32_t cnt[1024];
    const int b = blockIdx.x, t = threadIdx.x;
    const int C = s.hdr->n_chunks;
    const int n = C > s.Cw ? 0 : (MODE == 0 ? s.N : in_count[b]);
    const float lx = s.hdr->lo[0], ly = s.hdr->lo[1], lz = s.hdr->lo[2], hx = s.hdr->hi[0], hy = s.hdr->hi[1], hz = s.hdr->hi[2];
    auto keep = [&](int k) {
        if constexpr (MODE == 0) {
            const float* p = s.points + ((int64_t)b * s.N + k) * 3;
            return p[0] >= lx && p[0] <= hx && p[1] >= ly && p[1] <= hy && p[2] >= lz && p[2] <= hz;  // (a NaN is outside)
        } else {
            return fold_winding(s, C, b, k) > 0.5f;
        }
    };
    const int m = block_compact(n, cnt, keep, [&](int at, int k) {
        out_list[(int64_t)b * s.N + at] = MODE == 0 ? k : in_list[(int64_t)b * s.N + k];
    });
    if (t == 1023) out_count[b] = m;
}

// per inside point (list 1): the gradient row, and per block the fp64 sum of d^2
__global__ __launch_bounds__(kFold) void sdf_pen_fold_kernel(SweepArgs s, float* __restrict__ grad, double* __restrict__ blockval, int nb) {
    __shared__ double red[4][1];
    static_assert(kFold == 256, "block4_sum: four waves");
    const int b = blockIdx.y, t = threadIdx.x, k = blockIdx.x * kFold + t;
    const int C = s.hdr->n_chunks;
    if (C > s.Cw) return;
    const int m = s.count[b];
    if ((int)blockIdx.x * kFold >= m) return;  // block-uniform
    double d2[1] = {0.0};
    if (k < m) {
        float4 q;
        int fc;
        fold_closest(s, C, b, k, q, fc);
        if (fc >= 0) {
            d2[0] = (double)q.w;
            if (grad) {
                const float sc = 2.0f / (float)s.N;
                float* g = grad + ((int64_t)b * s.N + s.list[(int64_t)b * s.N + k]) * 3;
                g[0] = -q.x * sc;  // x - c = -q
                g[1] = -q.y * sc;
                g[2] = -q.z * sc;
            }
        }
    }
    block4_sum(d2, red);
    if (t == 0) blockval[(int64_t)b * nb + blockIdx.x] = d2[0];
}

// one wave per pose: the block sums, / N, rounded once
__global__ __launch_bounds__(64) void sdf_pen_value_kernel(SweepArgs s, const double* __restrict__ blockval, int nb, float* __restrict__ value) {
    const int b = blockIdx.x;
    if (s.hdr->n_chunks > s.Cw) {
        if (threadIdx.x == 0) value[b] = NAN;
        return;
    }
    const int used = (s.count[b] + kFold - 1) / kFold;
    double v[1];
    wave_fold(blockval + (int64_t)b * nb, used, v);
    if (threadIdx.x == 0) value[b] = (float)(v[0] / (double)s.N);
}

// ---- intrusion ------------------------------------------------------------------------------------------------------------------
constexpr int kIntr = 14;  // sums per pose: s^2 dd, e[3], e.(c R), c_i e_k [9]

// x = ((h - t) R^T) / s per pose and point; a pose whose s is not > 0 gets NaN (outside every bounding box: no sweep)
__global__ __launch_bounds__(kFold) void sdf_unpose_kernel(const float* __restrict__ h, const float* __restrict__ rot6d,
                                                           const float* __restrict__ trans, const float* __restrict__ scale, int N,
                                                           float* __restrict__ x) {
    __shared__ float pose[13];  // R row-major, t, s
    const int b = blockIdx.y, t = threadIdx.x;
    if (t == 0) {
        const Frame f = gram_schmidt(rot6d + (int64_t)b * 6);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            pose[i * 3 + 0] = (float)f.b1[i];
            pose[i * 3 + 1] = (float)f.b2[i];
            pose[i * 3 + 2] = (float)f.b3[i];
            pose[9 + i] = trans[(int64_t)b * 3 + i];
        }
        pose[12] = scale[b];
    }
    __syncthreads();
    const int n = blockIdx.x * kFold + t;
    if (n >= N) return;
    const float s = pose[12];
    const float u0 = h[(int64_t)n * 3] - pose[9], u1 = h[(int64_t)n * 3 + 1] - pose[10], u2 = h[(int64_t)n * 3 + 2] - pose[11];
    float* o = x + ((int64_t)b * N + n) * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = s > 0.0f ? ((u0 * pose[3 * i] + u1 * pose[3 * i + 1]) + u2 * pose[3 * i + 2]) / s : NAN;
}

// per inside point (list 1), all in fp64: the 14 sums of its block into part[(b nb + block) 14 + k]
__global__ __launch_bounds__(kFold) void sdf_intrusion_fold_kernel(SweepArgs s, const float* __restrict__ rot6d, const float* __restrict__ scale,
                                                                   double* __restrict__ part, int nb) {
    __shared__ double red[4][kIntr];
    __shared__ double pose[10];  // R row-major, s
    static_assert(kFold == 256, "block4_sum: four waves");
    const int b = blockIdx.y, t = threadIdx.x, k = blockIdx.x * kFold + t;
    const int C = s.hdr->n_chunks;
    if (C > s.Cw) return;
    const int m = s.count[b];
    if ((int)blockIdx.x * kFold >= m) return;  // block-uniform
    if (t == 0) {
        const Frame f = gram_schmidt(rot6d + (int64_t)b * 6);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            pose[i * 3 + 0] = f.b1[i];
            pose[i * 3 + 1] = f.b2[i];
            pose[i * 3 + 2] = f.b3[i];
        }
        pose[9] = (double)scale[b];
    }
    __syncthreads();
    double acc[kIntr];
#pragma unroll
    for (int j = 0; j < kIntr; ++j) acc[j] = 0.0;
    if (k < m) {
        float4 q;
        int fc;
        fold_closest(s, C, b, k, q, fc);
        if (fc >= 0) {
            const double sc = pose[9];
            const float* xp = s.points + ((int64_t)b * s.N + s.list[(int64_t)b * s.N + k]) * 3;
            const double qd[3] = {(double)q.x, (double)q.y, (double)q.z};
            const double c[3] = {(double)xp[0] + qd[0], (double)xp[1] + qd[1], (double)xp[2] + qd[2]};
            double e[3], cr[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                e[j] = -sc * ((qd[0] * pose[j] + qd[1] * pose[3 + j]) + qd[2] * pose[6 + j]);
                cr[j] = (c[0] * pose[j] + c[1] * pose[3 + j]) + c[2] * pose[6 + j];
            }
            acc[0] = (sc * sc) * (double)q.w;
            acc[4] = (e[0] * cr[0] + e[1] * cr[1]) + e[2] * cr[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                acc[1 + i] = e[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[5 + 3 * i + j] = c[i] * e[j];
            }
        }
    }
    block4_sum(acc, red);
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < kIntr; ++j) part[((int64_t)b * nb + blockIdx.x) * kIntr + j] = acc[j];
    }
}

// one wave per pose: the block sums, the factors, the chain to rot6d; each output rounded once
__global__ __launch_bounds__(64) void sdf_intrusion_finish_kernel(SweepArgs s, const float* __restrict__ rot6d, const float* __restrict__ scale,
                                                                  const double* __restrict__ part, int nb, float* __restrict__ value,
                                                                  float* __restrict__ grad_r6, float* __restrict__ grad_t,
                                                                  float* __restrict__ grad_s) {
    const int b = blockIdx.x;
    const double sc = (double)scale[b];
    const bool bad = s.hdr->n_chunks > s.Cw || !(sc > 0.0);  // block-uniform
    double v[kIntr];
    if (!bad) wave_fold(part + (int64_t)b * nb * kIntr, (s.count[b] + kFold - 1) / kFold, v);
    if (threadIdx.x != 0) return;
    if (bad) {
        value[b] = NAN;
        if (grad_t) grad_t[(int64_t)b * 3] = grad_t[(int64_t)b * 3 + 1] = grad_t[(int64_t)b * 3 + 2] = NAN;
        if (grad_s) grad_s[b] = NAN;
        if (grad_r6) {
            for (int i = 0; i < 6; ++i) grad_r6[(int64_t)b * 6 + i] = NAN;
        }
        return;
    }
    const double n = (double)s.N;
    value[b] = (float)(v[0] / n);
    const double w = -2.0 / n;
    if (grad_t) {
#pragma unroll
        for (int j = 0; j < 3; ++j) grad_t[(int64_t)b * 3 + j] = (float)(w * v[1 + j]);
    }
    if (grad_s) grad_s[b] = (float)(w * v[4]);
    if (!grad_r6) return;
    const Frame f = gram_schmidt(rot6d + (int64_t)b * 6);
    const double ws = w * sc;
    double gb1[3], gb2[3], gb3[3], ga1[3], ga2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // dL/dR_ik = -(2 s / N) sum c_i e_k, by columns
        gb1[i] = ws * v[5 + 3 * i];
        gb2[i] = ws * v[5 + 3 * i + 1];
        gb3[i] = ws * v[5 + 3 * i + 2];
    }
    gram_schmidt_backward(f, gb1, gb2, gb3, ga1, ga2);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        grad_r6[(int64_t)b * 6 + 2 * i] = (float)ga1[i];
        grad_r6[(int64_t)b * 6 + 2 * i + 1] = (float)ga2[i];
    }
}

bool sizes_ok(int B, int N) { return B > 0 && N > 0 && B <= 65535 && N <= kMaxN; }

}  // namespace

size_t mesh_sdf_plan_bytes(int n_verts, int n_faces) {
    if (n_verts <= 0 || n_faces <= 0 || n_verts > kMaxF || n_faces > kMaxF) return 0;
    return sizeof(SdfHeader) + (size_t)n_faces * 48;
}

int mesh_sdf_prepare(const float* verts, const int32_t* faces, int n_verts, int n_faces, void* plan, size_t plan_bytes, hipStream_t st) {
    if (!verts || !faces || !plan || n_verts <= 0 || n_faces <= 0 || (reinterpret_cast<uintptr_t>(plan) & 15)) return IVLM_ERR_INVALID_ARG;
    if (n_verts > kMaxF || n_faces > kMaxF) return IVLM_ERR_UNSUPPORTED;
    if (plan_bytes < mesh_sdf_plan_bytes(n_verts, n_faces)) return IVLM_ERR_WORKSPACE;
    SdfHeader* hdr = static_cast<SdfHeader*>(plan);
    sdf_records_kernel<<<(n_faces + 255) / 256, 256, 0, st>>>(verts, faces, n_verts, n_faces, reinterpret_cast<float4*>(hdr + 1));
    sdf_header_kernel<<<1, 1024, 0, st>>>(verts, n_verts, n_faces, hdr);
    return ivlm_launch_status();
}

size_t mesh_sdf_workspace_bytes(int B, int N, int n_faces) {
    if (!sizes_ok(B, N) || n_faces <= 0 || n_faces > kMaxF) return 0;
    return sdf_layout(B, N, (n_faces + kChunk - 1) / kChunk).total;
}

namespace {
// what the intrusion call keeps behind the penetration's layout: x [B,N,3] and the block partials [B,nb,14]
struct IntrusionExtra {
    size_t x, part, total;
};

IntrusionExtra intrusion_extra(int B, int N) {
    IntrusionExtra e;
    Carve c;
    e.x = c.take((size_t)B * N * 12);
    e.part = c.take((size_t)B * ((N + kFold - 1) / kFold) * kIntr * 8);
    e.total = c.off;
    return e;
}

// -> the sweep arguments over a checked workspace, or an error code in *rc
// extra: bytes the caller keeps for itself behind the layout (the chunk capacity is derived from what is left)
SweepArgs sweep_args(const void* plan, const float* points, int B, int N, void* ws, size_t ws_bytes, SdfLayout* l, int* rc,
                     size_t extra = 0) {
    SweepArgs s = {};
    *rc = IVLM_OK;
    if (!plan || !points || !ws || B <= 0 || N <= 0 || (reinterpret_cast<uintptr_t>(plan) & 15)) {
        *rc = IVLM_ERR_INVALID_ARG;
        return s;
    }
    if (!sizes_ok(B, N)) {
        *rc = IVLM_ERR_UNSUPPORTED;
        return s;
    }
    if (!workspace_ok(ws, ws_bytes, sdf_layout(B, N, 1).total + extra, 16)) {  // not even one chunk
        *rc = IVLM_ERR_WORKSPACE;
        return s;
    }
    const int Cw = sdf_capacity(B, N, ws_bytes - extra);
    *l = sdf_layout(B, N, Cw);
    s.hdr = static_cast<const SdfHeader*>(plan);
    s.rec = reinterpret_cast<const float4*>(s.hdr + 1);
    s.points = points;
    s.p4 = ws_at<float4>(ws, l->p4);
    s.pf = ws_at<int32_t>(ws, l->pf);
    s.pw = ws_at<float>(ws, l->pw);
    s.N = N;
    s.Cw = Cw;
    return s;
}

// What penetration and intrusion share: the points of s.points inside the bounding box (list 0), their winding sums, the inside ones
// among them (list 1), their closest points.  Leaves s on list 1 for the caller's fold.
void sweep_inside(SweepArgs& s, const SdfLayout& l, void* ws, int B, hipStream_t st) {
    int32_t* cnt = ws_at<int32_t>(ws, l.cnt);
    int32_t* list0 = ws_at<int32_t>(ws, l.list[0]);
    int32_t* list1 = ws_at<int32_t>(ws, l.list[1]);
    const dim3 grid((s.N + kWave - 1) / kWave, s.Cw, B);
    sdf_compact_kernel<0><<<B, 1024, 0, st>>>(s, nullptr, nullptr, list0, cnt);
    s.list = list0;
    s.count = cnt;
    sdf_sweep_kernel<true, false><<<grid, kWave, 0, st>>>(s);
    sdf_compact_kernel<1><<<B, 1024, 0, st>>>(s, list0, cnt, list1, cnt + B);
    s.list = list1;
    s.count = cnt + B;
    sdf_sweep_kernel<false, true><<<grid, kWave, 0, st>>>(s);
}
}  // namespace

int mesh_sdf_query(const void* plan, const float* points, int B, int N, float* sdf, float* closest, int32_t* face, float* winding,
                   void* ws, size_t ws_bytes, hipStream_t st) {
    if (!sdf && !closest && !face && !winding) return IVLM_ERR_INVALID_ARG;
    SdfLayout l;
    int rc;
    SweepArgs s = sweep_args(plan, points, B, N, ws, ws_bytes, &l, &rc);
    if (rc != IVLM_OK) return rc;
    sdf_sweep_kernel<true, true><<<dim3((N + kWave - 1) / kWave, s.Cw, B), kWave, 0, st>>>(s);
    sdf_query_fold_kernel<<<dim3((N + kFold - 1) / kFold, B), kFold, 0, st>>>(s, sdf, closest, face, winding);
    return ivlm_launch_status();
}

int mesh_sdf_penetration(const void* plan, const float* points, int B, int N, float* value, float* grad, void* ws, size_t ws_bytes,
                         hipStream_t st) {
    if (!value) return IVLM_ERR_INVALID_ARG;
    SdfLayout l;
    int rc;
    SweepArgs s = sweep_args(plan, points, B, N, ws, ws_bytes, &l, &rc);
    if (rc != IVLM_OK) return rc;
    double* blockval = ws_at<double>(ws, l.blockval);
    if (grad) IVLM_HIP_TRY(hipMemsetAsync(grad, 0, (size_t)B * N * 12, st));
    sweep_inside(s, l, ws, B, st);
    sdf_pen_fold_kernel<<<dim3(l.nb, B), kFold, 0, st>>>(s, grad, blockval, l.nb);
    sdf_pen_value_kernel<<<B, 64, 0, st>>>(s, blockval, l.nb, value);
    return ivlm_launch_status();
}

size_t mesh_sdf_intrusion_workspace_bytes(int B, int N, int n_faces) {
    const size_t base = mesh_sdf_workspace_bytes(B, N, n_faces);
    return base ? base + intrusion_extra(B, N).total : 0;
}

int mesh_sdf_intrusion(const void* plan, const float* points, const float* rot6d, const float* trans, const float* scale, int B, int N,
                       float* value, float* grad_r6, float* grad_t, float* grad_s, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!value || !rot6d || !trans || !scale) return IVLM_ERR_INVALID_ARG;
    SdfLayout l;
    int rc;
    const IntrusionExtra ex = sizes_ok(B, N) ? intrusion_extra(B, N) : IntrusionExtra{};
    SweepArgs s = sweep_args(plan, points, B, N, ws, ws_bytes, &l, &rc, ex.total);
    if (rc != IVLM_OK) return rc;
    float* x = ws_at<float>(ws, l.total + ex.x);
    double* part = ws_at<double>(ws, l.total + ex.part);
    sdf_unpose_kernel<<<dim3(l.nb, B), kFold, 0, st>>>(points, rot6d, trans, scale, N, x);
    s.points = x;
    sweep_inside(s, l, ws, B, st);
    sdf_intrusion_fold_kernel<<<dim3(l.nb, B), kFold, 0, st>>>(s, rot6d, scale, part, l.nb);
    sdf_intrusion_finish_kernel<<<B, 64, 0, st>>>(s, rot6d, scale, part, l.nb, value, grad_r6, grad_t, grad_s);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_mesh_sdf_plan_bytes(int N_h, int F) { return ivlm::mesh_sdf_plan_bytes(N_h, F); }
int ivlm_mesh_sdf_prepare(const float* vertices, const int32_t* faces, int N_h, int F, void* plan, size_t plan_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mesh_sdf_prepare(vertices, faces, N_h, F, plan, plan_bytes, ivlm_stream(s));
}
size_t ivlm_mesh_sdf_workspace_bytes(int B, int N, int F) { return ivlm::mesh_sdf_workspace_bytes(B, N, F); }
int ivlm_mesh_sdf_query(const void* plan, const float* points, int B, int N, float* sdf, float* closest, int32_t* face, float* winding,
                        void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mesh_sdf_query(plan, points, B, N, sdf, closest, face, winding, workspace, workspace_bytes, ivlm_stream(s));
}
int ivlm_mesh_sdf_penetration(const void* plan, const float* points, int B, int N, float* value, float* grad, void* workspace,
                              size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mesh_sdf_penetration(plan, points, B, N, value, grad, workspace, workspace_bytes, ivlm_stream(s));
}
size_t ivlm_mesh_sdf_intrusion_workspace_bytes(int B, int N, int F) { return ivlm::mesh_sdf_intrusion_workspace_bytes(B, N, F); }
int ivlm_mesh_sdf_intrusion(const void* plan, const float* points, const float* rot6d, const float* translation, const float* scale, int B,
                            int N, float* value, float* grad_rot6d, float* grad_translation, float* grad_scale, void* workspace,
                            size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mesh_sdf_intrusion(plan, points, rot6d, translation, scale, B, N, value, grad_rot6d, grad_translation, grad_scale,
                                    workspace, workspace_bytes, ivlm_stream(s));
}
}
