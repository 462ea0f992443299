// What silhouette.hip and depth_order.hip share: the walk over the faces of a posed mesh in screen space, in the camera both use
// (u = fx X / Z + px, v = fy Y / Z + py; pixel (row i, col j) has its centre at (j + 0.5, i + 0.5)).  Everything the image terms'
// "same bits every call, for a pose whatever the batch" rests on is here once (DESIGN 4.50 lists it): the order in which a tile's
// faces are compacted, the length of the backward's fp32 chains and its fp64 fold, the order of a vertex's incident faces.
//
// fit_common.h's rule (only integer and fp64 additions) does NOT hold here: this header has fp32 and fp64 products next to sums -
// area2, ax X + ay Y - and the two files are built with different -ffp-contract (depth_order.hip off, silhouette.hip the default),
// so the same text is different arithmetic in each, which is what keeps each file's bits.  The rule here: the including file's
// flag decides; nothing here may be called from a third file without deciding that.  So that one file can never launch the
// other's code, every kernel and function below has internal linkage (the anonymous namespace): two external instantiations of one
// name in two objects would be merged by the linker into one host stub.
#pragma once
#include <cmath>

#include "fit_common.h"

namespace ivlm {
namespace {

constexpr int kTile = 16;         // pixels per tile side
constexpr int kChunk = 256;       // faces tested per block step = threads per block of a tile kernel
constexpr int kMaxN = 1 << 22;    // vertices, faces
constexpr int kMaxSide = 16384;   // H, W
constexpr float kMinZ = 1e-6f;

struct ScreenParams {
    float fx, fy, px, py;
    int N, F, H, W;
};

bool screen_sizes_ok(int B, int N, int F, int H, int W) {
    return B > 0 && N > 0 && F > 0 && H > 0 && W > 0 && B <= 65535 && N <= kMaxN && F <= kMaxN && H <= kMaxSide && W <= kMaxSide;
}

bool screen_camera_ok(float fx, float fy, float px, float py) {
    return std::isfinite(fx) && std::isfinite(fy) && std::isfinite(px) && std::isfinite(py);
}

// ---- per vertex, per face -----------------------------------------------------------------------------------------------------------
// per vertex (u, v); resets the pose's union box
__global__ __launch_bounds__(256) void screen_project_kernel(const float* __restrict__ verts, float2* __restrict__ uv,
                                                             int4* __restrict__ uni, ScreenParams p) {
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0) uni[b] = make_int4(p.W, p.H, -1, -1);  // empty; the faces kernel (next on the stream) folds the boxes into it
    if (n >= p.N) return;
    const float* v = verts + ((int64_t)b * p.N + n) * 3;
    const float z = v[2];
    uv[(int64_t)b * p.N + n] = make_float2(fmaf(p.fx, v[0] / z, p.px), fmaf(p.fy, v[1] / z, p.py));
}

// first / last pixel whose centre can lie within [lo, hi], one pixel of slack on each side, clamped to [0, n - 1]
__device__ __forceinline__ void pixel_range(float lo, float hi, int n, int& first, int& last) {
    first = max((int)floorf(fminf(fmaxf(lo - 0.5f, -1.0f), (float)n)), 0);
    last = min((int)ceilf(fminf(fmaxf(hi - 0.5f, -1.0f), (float)n)), n - 1);
}

// Face f of pose b.  ok: its indices lie in [0, N), its three Z are > 1e-6 and its screen area is not zero - else the face is skipped
// whole.  a, b, c: the screen vertices (zeros when an index or a Z fails); za, zb, zc (1 unless ok); box: its pixel bounding box
// grown by `grow` pixels, empty (it meets no tile, holds no pixel) for a skipped face or one that misses the image.
struct ScreenFace {
    float2 a, b, c;
    float za, zb, zc;
    int4 box;
    bool ok;
};

__device__ __forceinline__ ScreenFace screen_face(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                  const float2* __restrict__ uv, int b, int f, float grow, const ScreenParams& p) {
    ScreenFace t;
    t.a = t.b = t.c = make_float2(0.f, 0.f);
    t.za = t.zb = t.zc = 1.0f;
    t.box = make_int4(p.W, p.H, -1, -1);
    const int i0 = faces[(int64_t)f * 3], i1 = faces[(int64_t)f * 3 + 1], i2 = faces[(int64_t)f * 3 + 2];
    t.ok = (unsigned)i0 < (unsigned)p.N && (unsigned)i1 < (unsigned)p.N && (unsigned)i2 < (unsigned)p.N;
    if (t.ok) {
        const float* v = verts + (int64_t)b * p.N * 3;
        t.za = v[(int64_t)i0 * 3 + 2];
        t.zb = v[(int64_t)i1 * 3 + 2];
        t.zc = v[(int64_t)i2 * 3 + 2];
        t.ok = t.za > kMinZ && t.zb > kMinZ && t.zc > kMinZ;
    }
    if (t.ok) {
        const float2* q = uv + (int64_t)b * p.N;
        t.a = q[i0];
        t.b = q[i1];
        t.c = q[i2];
        const float area2 = (t.b.x - t.a.x) * (t.c.y - t.a.y) - (t.b.y - t.a.y) * (t.c.x - t.a.x);
        t.ok = area2 != 0.0f;
    }
    if (t.ok) {
        int x0, x1, y0, y1;
        pixel_range(fminf(t.a.x, fminf(t.b.x, t.c.x)) - grow, fmaxf(t.a.x, fmaxf(t.b.x, t.c.x)) + grow, p.W, x0, x1);
        pixel_range(fminf(t.a.y, fminf(t.b.y, t.c.y)) - grow, fmaxf(t.a.y, fmaxf(t.b.y, t.c.y)) + grow, p.H, y0, y1);
        if (x0 <= x1 && y0 <= y1) t.box = make_int4(x0, y0, x1, y1);
    } else {
        t.za = t.zb = t.zc = 1.0f;
    }
    return t;
}

// folds a thread's box (empty for a thread without a face) into the pose's union: min / max across the wave, then four integer
// atomics per wave - the result does not depend on the order.  Every thread of the block calls it.
__device__ __forceinline__ void union_fold(const int4 bx, int4* __restrict__ uni) {
    int mnx = bx.x, mny = bx.y, mxx = bx.z, mxy = bx.w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, o, 64));
        mny = min(mny, __shfl_xor(mny, o, 64));
        mxx = max(mxx, __shfl_xor(mxx, o, 64));
        mxy = max(mxy, __shfl_xor(mxy, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && mxx >= 0) {
        atomicMin(&uni->x, mnx);
        atomicMin(&uni->y, mny);
        atomicMax(&uni->z, mxx);
        atomicMax(&uni->w, mxy);
    }
}

// ---- pixel-stationary: one 256-thread block per 16 x 16 tile, one pixel per thread ---------------------------------------------------
struct TilePixel {
    int tx0, ty0, tx1, ty1;  // the tile, clipped to the image
    int i, j;                // this thread's pixel; live: inside the image
    float qx, qy;            // its centre
    bool live;
};

__device__ __forceinline__ TilePixel tile_pixel(const ScreenParams& p) {
    TilePixel t;
    const int tid = threadIdx.x;
    t.tx0 = blockIdx.x * kTile, t.ty0 = blockIdx.y * kTile;
    t.tx1 = min(t.tx0 + kTile - 1, p.W - 1), t.ty1 = min(t.ty0 + kTile - 1, p.H - 1);
    t.j = t.tx0 + (tid & (kTile - 1)), t.i = t.ty0 + tid / kTile;
    t.live = t.i < p.H && t.j < p.W;
    t.qx = (float)t.j + 0.5f, t.qy = (float)t.i + 0.5f;
    return t;
}

// does the pose's union box meet the tile?  (block-uniform: a tile outside it leaves at once)
__device__ __forceinline__ bool tile_meets(const int4 U, const TilePixel& t) {
    return U.x <= t.tx1 && U.z >= t.tx0 && U.y <= t.ty1 && U.w >= t.ty0;
}

// One step of the walk over a pose's F boxes bb in chunks of 256, one box per thread: the faces c0 .. c0 + 255 whose box meets the
// tile are compacted in ascending face order (ballot + prefix: the list is a function of the geometry alone) - stage(pos, f, box)
// writes the caller's LDS records of face f at slot pos -> the number of faces staged, which every live pixel then visits as
// k = 0 .. total - 1.  Two barriers, so EVERY thread of the block calls this (a dead pixel is not an early return), and the caller's
// visits of one chunk are safe from the next chunk's records: those are written behind its first barrier, which every wave reaches
// after its visits.
template <typename Stage>
__device__ __forceinline__ int tile_chunk(const int4* __restrict__ bb, int F, int c0, const TilePixel& t, Stage stage) {
    __shared__ int wcnt[kChunk / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = c0 + tid;
    bool hit = false;
    int4 bx = make_int4(0, 0, -1, -1);
    if (f < F) {
        bx = bb[f];
        hit = bx.x <= t.tx1 && bx.z >= t.tx0 && bx.y <= t.ty1 && bx.w >= t.ty0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kChunk / 64; ++w) {
        const int n = wcnt[w];
        base += w < wv ? n : 0;
        total += n;
    }
    if (hit) stage(base + __popcll(m & ((1ull << lane) - 1ull)), f, bx);
    __syncthreads();
    return total;
}

// ---- face-stationary: one wave per face ----------------------------------------------------------------------------------------------
// The wave walks the pixels of the box 64 at a time (the two-roles-instead-of-atomics choice of contact_pair.hip): term(i, j, px, a)
// adds pixel (i, j) (px = i W + j) to the lane's K fp32 accumulators, Chain pixels per lane; then they go to fp64, wave_sum's fp64
// butterfly across the lanes, and lane 0 stores K floats.  All 64 lanes call it, with wave-uniform arguments.  A box of very many
// pixels (one huge triangle) is walked by that one wave: correct, and its latency is accepted.
template <int K, int Chain, typename Term>
__device__ __forceinline__ void box_walk(const int4 bx, int W, Term term, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int bw = bx.z - bx.x + 1, bh = bx.w - bx.y + 1;
    const int npx = bw > 0 && bh > 0 ? bw * bh : 0;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int s0 = 0; s0 < npx; s0 += 64 * Chain) {  // wave-uniform bounds
        float a[K];
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = 0.f;
        const int s1 = min(s0 + 64 * Chain, npx);
        for (int idx = s0 + lane; idx < s1; idx += 64) {
            const int dy = idx / bw, dx = idx - dy * bw;
            const int i = bx.y + dy, j = bx.x + dx;
            term(i, j, (int64_t)i * W + j, a);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += (double)a[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = (float)acc[k];
    }
}

// per vertex: the records of its incident faces (C values per corner: du, dv and, with C == 3, a direct dZ) in ascending face order -
// the incidence lists are inputs, built once per topology by the caller -, summed in fp64, chained through the projection to
// dL/d(X, Y, Z)
template <int C>
__global__ __launch_bounds__(256) void screen_gather_kernel(const float* __restrict__ verts, const float* __restrict__ frec,
                                                            const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_list,
                                                            float* __restrict__ gverts, ScreenParams p) {
    static_assert(C == 2 || C == 3, "du, dv and perhaps dZ");
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.N) return;
    const float* fr = frec + (int64_t)b * p.F * (3 * C);
    const int e0 = vf_off[n], e1 = vf_off[n + 1];
    double s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.0;
    for (int e = e0; e < e1; ++e) {  // ascending face order: the list is sorted
        const int slot = vf_list[e];  // face * 3 + corner
        if ((unsigned)slot < (unsigned)p.F * 3u) {
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] += (double)fr[(int64_t)slot * C + c];
        }
    }
    const float* v = verts + ((int64_t)b * p.N + n) * 3;
    float* g = gverts + ((int64_t)b * p.N + n) * 3;
    const double z = (double)v[2];
    const double iz = v[2] > kMinZ ? 1.0 / z : 0.0;  // every face of a vertex with Z <= 1e-6 is skipped: the sums are 0
    const double ax = s[0] * (double)p.fx * iz, ay = s[1] * (double)p.fy * iz;
    g[0] = (float)ax;
    g[1] = (float)ay;
    // two expressions on purpose: with a dZ of 0.0 the second gives +0 where the first gives -0
    if constexpr (C == 2) g[2] = (float)(-(ax * (double)v[0] + ay * (double)v[1]) * iz);
    else g[2] = (float)(s[2] - (ax * (double)v[0] + ay * (double)v[1]) * iz);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the first four regions of either file's workspace; tri holds `record_bytes` per face
struct ScreenLayout {
    size_t uv, tri, box, uni;
};

ScreenLayout screen_layout(Carve& c, int B, int N, int F, size_t record_bytes) {
    ScreenLayout l;
    l.uv = c.take((size_t)B * N * 8);
    l.tri = c.take((size_t)B * F * record_bytes);
    l.box = c.take((size_t)B * F * 16);
    l.uni = c.take((size_t)B * 16);
    return l;
}

// the three forward launches: the projection, the file's faces kernel, the file's tile kernel with its two outputs
template <typename P, typename O1, typename O2>
void screen_forward(void (*faces_kernel)(const float*, const int32_t*, const float2*, float4*, int4*, int4*, P),
                    void (*tile_kernel)(const float4*, const int4*, const int4*, O1*, O2*, P), const float* verts, const int32_t* faces,
                    int B, const ScreenParams& s, const P& p, const ScreenLayout& l, void* ws, O1* out1, O2* out2, hipStream_t st) {
    float2* uv = ws_at<float2>(ws, l.uv);
    float4* tri = ws_at<float4>(ws, l.tri);
    int4* box = ws_at<int4>(ws, l.box);
    int4* uni = ws_at<int4>(ws, l.uni);
    screen_project_kernel<<<dim3((s.N + 255) / 256, B), 256, 0, st>>>(verts, uv, uni, s);
    faces_kernel<<<dim3((s.F + 255) / 256, B), 256, 0, st>>>(verts, faces, uv, tri, box, uni, p);
    tile_kernel<<<dim3((s.W + kTile - 1) / kTile, (s.H + kTile - 1) / kTile, B), kChunk, 0, st>>>(tri, box, uni, out1, out2, p);
}

}  // namespace
}  // namespace ivlm
