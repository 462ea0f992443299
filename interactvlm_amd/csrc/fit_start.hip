// The start of the object-pose fit: what the reference computes between "two meshes, two contact vectors, one mask" and the
// (rotation_init, translation_init, scaling_init) its optimiser starts from (optim/data_io.py:40-42, 69-71, 175, 192-194 and
// optim/fit.py:119-135), without pytorch3d or trimesh.  DESIGN 4.49.
//
//   mesh_vertex_normals    n_v = sum over the incident faces of cross(b - a, c - a) (twice the area times the face normal: pytorch3d's
//                          area weighting), divided by its length; a zero sum gives (0, 0, 0), never a NaN.  One thread per vertex
//                          walks the vertex's slots (face * 3 + corner, ascending: silhouette.topology_of) and adds in that order from
//                          0.0, so the order is a function of the slot list alone.
//   mesh_surface_centroid  sum_f A_f (a + b + c) / 3 / sum_f A_f, A_f = |cross(b - a, c - a)| / 2 (trimesh's Trimesh.centroid).  One
//                          face per thread, block4_sum<4> per block of 256 faces, then one wave: wave_fold<4> and one division per axis.
//   mask_stats             count, bounding box, row and column sums and the first two non-zero pixels in row-major order of a [H,W]
//                          byte mask.  Integer arithmetic only: exact, and the same whatever the order.
//   contact_depth          count and sum of z over the vertices whose probability is strictly above a threshold: block4_sum<2>, then
//                          wave_fold<2>; the mean is rounded once.
//   start_translation      one thread: T[3] from the two records, the camera and the mode.
//
// Every sum is fp64 from the fp32 coordinates in a stated order (fit_common.h), no floating-point atomics, results rounded to fp32
// once, plain vector stores, wave64, everything on the caller's stream with no host read.  A kernel that can meet an empty or
// degenerate input writes a status word (0 = fine) and zeros in place of the result, never a NaN.
//
// This file is built with -ffp-contract=off (the EXTRA table of build.py): the fp32 steps of start_translation's mirror mode,
// ((r + c) / 2 - p) * z / f, are the reference's torch operations one by one and the tests compare their bits; the fp64 cross products
// are then also the unfused ones of tests/_fit_start_ref.py.
#include <cstdint>

#include "fit_common.h"

namespace ivlm {
namespace {

constexpr int kBlock = 256;             // threads of every block kernel here = four waves (block4_sum)
constexpr int kMaskPerThread = 16;      // pixels per thread of mask_stats_kernel
constexpr int kMaskTile = kBlock * kMaskPerThread;
constexpr int kMaskVals = 9;            // count, row min, row max, col min, col max, row sum, col sum, first, second (linear indices)
constexpr int kMaxMesh = 1 << 22;       // N, F
constexpr int kMaxSide = 16384;         // H, W
constexpr int64_t kNone = INT64_MAX;    // "no such pixel" while indices are folded by min

struct Vec3d {
    double x, y, z;
};

__device__ __forceinline__ Vec3d load3(const float* __restrict__ verts, int i) {
    return {(double)verts[3 * (int64_t)i], (double)verts[3 * (int64_t)i + 1], (double)verts[3 * (int64_t)i + 2]};
}

// cross(b - a, c - a) in fp64
__device__ __forceinline__ Vec3d face_cross(const Vec3d& a, const Vec3d& b, const Vec3d& c) {
    const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const double wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
    return {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
}

// the three vertex indices of face f, false when one lies outside [0, N) (such a face is skipped whole)
__device__ __forceinline__ bool face_indices(const int32_t* __restrict__ faces, int f, int N, int& ia, int& ib, int& ic) {
    ia = faces[3 * (int64_t)f];
    ib = faces[3 * (int64_t)f + 1];
    ic = faces[3 * (int64_t)f + 2];
    return (unsigned)ia < (unsigned)N && (unsigned)ib < (unsigned)N && (unsigned)ic < (unsigned)N;
}

// ---- vertex normals ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void vertex_normals_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ offsets, const int32_t* __restrict__ slots,
                                                                int N, int F, float* __restrict__ out) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= N) return;
    const int k0 = max(offsets[v], 0), k1 = min(offsets[v + 1], 3 * F);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = k0; k < k1; ++k) {  // ascending slot order from 0.0
        const int slot = slots[k];
        if ((unsigned)slot >= (unsigned)(3 * F)) continue;
        int ia, ib, ic;
        if (!face_indices(faces, slot / 3, N, ia, ib, ic)) continue;
        const Vec3d n = face_cross(load3(verts, ia), load3(verts, ib), load3(verts, ic));
        sx += n.x;
        sy += n.y;
        sz += n.z;
    }
    const double ss = (sx * sx + sy * sy) + sz * sz;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (ss > 0.0 && ss < INFINITY) {  // an unreferenced vertex, or only zero-area faces: (0, 0, 0)
        const double len = sqrt(ss);
        ox = (float)(sx / len);
        oy = (float)(sy / len);
        oz = (float)(sz / len);
    }
    out[3 * (int64_t)v] = ox;
    out[3 * (int64_t)v + 1] = oy;
    out[3 * (int64_t)v + 2] = oz;
}

// ---- surface centroid ----------------------------------------------------------------------------------------------------------------
// part[block * 4 + k]: sum A x, sum A y, sum A z, sum A of the block's faces
__global__ __launch_bounds__(kBlock) void centroid_partial_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int N,
                                                                  int F, double* __restrict__ part) {
    __shared__ double red[4][4];
    const int f = blockIdx.x * kBlock + threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    int ia, ib, ic;
    if (f < F && face_indices(faces, f, N, ia, ib, ic)) {
        const Vec3d a = load3(verts, ia), b = load3(verts, ib), c = load3(verts, ic);
        const Vec3d n = face_cross(a, b, c);
        const double area = 0.5 * sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
        if (area > 0.0 && area < INFINITY) {
            v[0] = area * (((a.x + b.x) + c.x) / 3.0);
            v[1] = area * (((a.y + b.y) + c.y) / 3.0);
            v[2] = area * (((a.z + b.z) + c.z) / 3.0);
            v[3] = area;
        }
    }
    block4_sum<4>(v, red);
    if (threadIdx.x < 4) part[(int64_t)blockIdx.x * 4 + threadIdx.x] = v[threadIdx.x];
}

__global__ __launch_bounds__(64) void centroid_finish_kernel(const double* __restrict__ part, int n_part, float* __restrict__ centroid,
                                                             int64_t* __restrict__ status) {
    double s[4];
    wave_fold<4>(part, n_part, s);
    if (threadIdx.x == 0) {
        const bool ok = s[3] > 0.0 && s[3] < INFINITY;
        centroid[0] = ok ? (float)(s[0] / s[3]) : 0.0f;
        centroid[1] = ok ? (float)(s[1] / s[3]) : 0.0f;
        centroid[2] = ok ? (float)(s[2] / s[3]) : 0.0f;
        status[0] = ok ? 0 : IVLM_START_NO_AREA;
    }
}

// ---- mask statistics -----------------------------------------------------------------------------------------------------------------
struct MaskVals {
    int64_t v[kMaskVals];
};

__device__ __forceinline__ MaskVals mask_none() {
    return {{0, kNone, -1, kNone, -1, 0, 0, kNone, kNone}};
}

// of two records whose (first, second) are ascending: counts and sums added, extremes by min / max, the two smallest indices of the four
__device__ __forceinline__ MaskVals mask_join(const MaskVals& a, const MaskVals& b) {
    MaskVals r;
    r.v[0] = a.v[0] + b.v[0];
    r.v[1] = min(a.v[1], b.v[1]);
    r.v[2] = max(a.v[2], b.v[2]);
    r.v[3] = min(a.v[3], b.v[3]);
    r.v[4] = max(a.v[4], b.v[4]);
    r.v[5] = a.v[5] + b.v[5];
    r.v[6] = a.v[6] + b.v[6];
    r.v[7] = min(a.v[7], b.v[7]);
    r.v[8] = min(max(a.v[7], b.v[7]), min(a.v[8], b.v[8]));
    return r;
}

__device__ __forceinline__ MaskVals mask_wave_join(MaskVals m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MaskVals o;
#pragma unroll
        for (int k = 0; k < kMaskVals; ++k) o.v[k] = __shfl_xor((long long)m.v[k], off, 64);
        m = mask_join(m, o);
    }
    return m;
}

__global__ __launch_bounds__(kBlock) void mask_partial_kernel(const uint8_t* __restrict__ mask, int W, int HW, int64_t* __restrict__ part) {
    __shared__ int64_t red[4][kMaskVals];
    MaskVals m = mask_none();
    const int base = blockIdx.x * kMaskTile + threadIdx.x;
    for (int k = 0; k < kMaskPerThread; ++k) {  // ascending pixel index within the thread
        const int i = base + k * kBlock;
        if (i < HW && mask[i] != 0) {
            const int r = i / W, c = i - r * W;
            m.v[0] += 1;
            m.v[1] = min(m.v[1], (int64_t)r);
            m.v[2] = max(m.v[2], (int64_t)r);
            m.v[3] = min(m.v[3], (int64_t)c);
            m.v[4] = max(m.v[4], (int64_t)c);
            m.v[5] += r;
            m.v[6] += c;
            if (m.v[7] == kNone) m.v[7] = i;
            else if (m.v[8] == kNone) m.v[8] = i;
        }
    }
    m = mask_wave_join(m);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kMaskVals; ++k) red[threadIdx.x >> 6][k] = m.v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MaskVals w[4];
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < kMaskVals; ++k) w[j].v[k] = red[j][k];
        const MaskVals s = mask_join(mask_join(w[0], w[1]), mask_join(w[2], w[3]));
        for (int k = 0; k < kMaskVals; ++k) part[(int64_t)blockIdx.x * kMaskVals + k] = s.v[k];
    }
}

// record: the IVLM_MASK_* fields of include/ivlm_hip.h
__global__ __launch_bounds__(64) void mask_finish_kernel(const int64_t* __restrict__ part, int n_part, int W, int64_t* __restrict__ record) {
    MaskVals m = mask_none();
    for (int j = threadIdx.x; j < n_part; j += 64) {
        MaskVals o;
        for (int k = 0; k < kMaskVals; ++k) o.v[k] = part[(int64_t)j * kMaskVals + k];
        m = mask_join(m, o);
    }
    m = mask_wave_join(m);
    if (threadIdx.x == 0) {
        const bool any = m.v[0] > 0;
        record[IVLM_MASK_COUNT] = m.v[0];
        record[IVLM_MASK_ROW_MIN] = any ? m.v[1] : -1;
        record[IVLM_MASK_ROW_MAX] = m.v[2];
        record[IVLM_MASK_COL_MIN] = any ? m.v[3] : -1;
        record[IVLM_MASK_COL_MAX] = m.v[4];
        record[IVLM_MASK_ROW_SUM] = m.v[5];
        record[IVLM_MASK_COL_SUM] = m.v[6];
        const bool one = m.v[7] != kNone, two = m.v[8] != kNone;
        record[IVLM_MASK_FIRST_ROW] = one ? m.v[7] / W : -1;
        record[IVLM_MASK_FIRST_COL] = one ? m.v[7] % W : -1;
        record[IVLM_MASK_SECOND_ROW] = two ? m.v[8] / W : -1;
        record[IVLM_MASK_SECOND_COL] = two ? m.v[8] % W : -1;
        record[IVLM_MASK_STATUS] = any ? 0 : IVLM_START_EMPTY_MASK;
    }
}

// ---- contact depth -------------------------------------------------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(kBlock) void depth_partial_kernel(const float* __restrict__ verts, const void* __restrict__ probs, int N,
                                                               float threshold, double* __restrict__ part) {
    __shared__ double red[4][2];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (i < N) {
        float p;
        if constexpr (BF16) p = bf16_to_f32(static_cast<const bf16_t*>(probs)[i]);
        else p = static_cast<const float*>(probs)[i];
        if (p > threshold) {  // strictly above, compared in fp32
            v[0] = 1.0;
            v[1] = (double)verts[3 * (int64_t)i + 2];
        }
    }
    block4_sum<2>(v, red);
    if (threadIdx.x < 2) part[(int64_t)blockIdx.x * 2 + threadIdx.x] = v[threadIdx.x];
}

// record: [0] count, [1] status; z_sum: the fp64 sum; z: its mean rounded once (0 for no vertex)
__global__ __launch_bounds__(64) void depth_finish_kernel(const double* __restrict__ part, int n_part, int64_t* __restrict__ record,
                                                          double* __restrict__ z_sum, float* __restrict__ z) {
    double s[2];
    wave_fold<2>(part, n_part, s);
    if (threadIdx.x == 0) {
        const bool any = s[0] > 0.0;
        record[IVLM_DEPTH_COUNT] = (int64_t)s[0];
        record[IVLM_DEPTH_STATUS] = any ? 0 : IVLM_START_NO_CONTACT;
        z_sum[0] = s[1];
        z[0] = any ? (float)(s[1] / s[0]) : 0.0f;
    }
}

// ---- the stage-1 translation ------------------------------------------------------------------------------------------------------------
// cam = (fx, fy, px, py); offset = hum_centroid_offset or NULL for (0, 0, 0).
// mirror: optim/fit.py:119-135 as written, fp32, one operation at a time: nonzero(mask)[1] is the SECOND non-zero pixel's (row, col) and
// its mean goes with px; nonzero(mask)[0] is the FIRST pixel's and its mean goes with py.
// intent (NOT the reference's): the object's origin on the camera ray through the mask's mean pixel centre (mean col + 0.5, mean row +
// 0.5: silhouette.py's convention) at depth Z = z + offset.z, expressed in the fit's frame (minus the offset); fp64, rounded once.
__global__ void start_translation_kernel(const int64_t* __restrict__ mask_record, const int64_t* __restrict__ depth_record,
                                         const float* __restrict__ z_mean, const float* __restrict__ cam, const float* __restrict__ offset,
                                         int mirror, float* __restrict__ T, int64_t* __restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t count = mask_record[IVLM_MASK_COUNT];
    int64_t bad = 0;
    if (count < (mirror ? 2 : 1)) bad |= mirror ? IVLM_START_FEW_PIXELS : IVLM_START_EMPTY_MASK;
    if (depth_record[IVLM_DEPTH_COUNT] < 1) bad |= IVLM_START_NO_CONTACT;
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
    if (!bad) {
        const float fx = cam[0], fy = cam[1], px = cam[2], py = cam[3];
        const float z = z_mean[0];
        if (mirror) {
            const float mx = ((float)mask_record[IVLM_MASK_SECOND_ROW] + (float)mask_record[IVLM_MASK_SECOND_COL]) / 2.0f;
            const float my = ((float)mask_record[IVLM_MASK_FIRST_ROW] + (float)mask_record[IVLM_MASK_FIRST_COL]) / 2.0f;
            const float cx = mx - px;
            const float cy = my - py;
            const float ax = cx * z;
            const float ay = cy * z;
            t0 = ax / fx;
            t1 = ay / fy;
            t2 = z;
        } else {
            const double ox = offset ? (double)offset[0] : 0.0, oy = offset ? (double)offset[1] : 0.0, oz = offset ? (double)offset[2] : 0.0;
            const double u = (double)mask_record[IVLM_MASK_COL_SUM] / (double)count + 0.5;
            const double v = (double)mask_record[IVLM_MASK_ROW_SUM] / (double)count + 0.5;
            const double Z = (double)z + oz;
            t0 = (float)((u - (double)px) * Z / (double)fx - ox);
            t1 = (float)((v - (double)py) * Z / (double)fy - oy);
            t2 = z;  // (z + oz) - oz
        }
    }
    T[0] = t0;
    T[1] = t1;
    T[2] = t2;
    status[0] = bad;
}

int blocks_of(int n, int per) { return (n + per - 1) / per; }

}  // namespace

// ---- host ------------------------------------------------------------------------------------------------------------------------------
size_t mesh_surface_centroid_workspace_bytes(int F) {
    if (F <= 0 || F > kMaxMesh) return 0;
    Carve c;
    c.take((size_t)blocks_of(F, kBlock) * 4 * sizeof(double));
    return c.off;
}

size_t mask_stats_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide) return 0;
    Carve c;
    c.take((size_t)blocks_of(H * W, kMaskTile) * kMaskVals * sizeof(int64_t));
    return c.off;
}

size_t contact_depth_workspace_bytes(int N) {
    if (N <= 0 || N > kMaxMesh) return 0;
    Carve c;
    c.take((size_t)blocks_of(N, kBlock) * 2 * sizeof(double));
    return c.off;
}

int mesh_vertex_normals(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* slots, int N, int F, float* out,
                        hipStream_t st) {
    if (!verts || !faces || !offsets || !slots || !out || N <= 0 || F <= 0) return IVLM_ERR_INVALID_ARG;
    if (N > kMaxMesh || F > kMaxMesh) return IVLM_ERR_UNSUPPORTED;
    vertex_normals_kernel<<<blocks_of(N, kBlock), kBlock, 0, st>>>(verts, faces, offsets, slots, N, F, out);
    return ivlm_launch_status();
}

int mesh_surface_centroid(const float* verts, const int32_t* faces, int N, int F, float* centroid, int64_t* status, void* ws,
                          size_t ws_bytes, hipStream_t st) {
    if (!verts || !faces || !centroid || !status || !ws || N <= 0 || F <= 0) return IVLM_ERR_INVALID_ARG;
    if (N > kMaxMesh || F > kMaxMesh) return IVLM_ERR_UNSUPPORTED;
    if (!workspace_ok(ws, ws_bytes, mesh_surface_centroid_workspace_bytes(F), 16)) return IVLM_ERR_WORKSPACE;
    double* part = ws_at<double>(ws, 0);
    const int nb = blocks_of(F, kBlock);
    centroid_partial_kernel<<<nb, kBlock, 0, st>>>(verts, faces, N, F, part);
    centroid_finish_kernel<<<1, 64, 0, st>>>(part, nb, centroid, status);
    return ivlm_launch_status();
}

int mask_stats(const uint8_t* mask, int H, int W, int64_t* record, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!mask || !record || !ws || H <= 0 || W <= 0) return IVLM_ERR_INVALID_ARG;
    if (H > kMaxSide || W > kMaxSide) return IVLM_ERR_UNSUPPORTED;
    if (!workspace_ok(ws, ws_bytes, mask_stats_workspace_bytes(H, W), 16)) return IVLM_ERR_WORKSPACE;
    int64_t* part = ws_at<int64_t>(ws, 0);
    const int nb = blocks_of(H * W, kMaskTile);
    mask_partial_kernel<<<nb, kBlock, 0, st>>>(mask, W, H * W, part);
    mask_finish_kernel<<<1, 64, 0, st>>>(part, nb, W, record);
    return ivlm_launch_status();
}

int contact_depth(const float* verts, const void* probs, int p_dtype, int N, float threshold, int64_t* record, double* z_sum, float* z,
                  void* ws, size_t ws_bytes, hipStream_t st) {
    if (!verts || !probs || !record || !z_sum || !z || !ws || N <= 0 || !(threshold == threshold)) return IVLM_ERR_INVALID_ARG;
    if ((p_dtype != IVLM_F32 && p_dtype != IVLM_BF16) || N > kMaxMesh) return IVLM_ERR_UNSUPPORTED;
    if (!workspace_ok(ws, ws_bytes, contact_depth_workspace_bytes(N), 16)) return IVLM_ERR_WORKSPACE;
    double* part = ws_at<double>(ws, 0);
    const int nb = blocks_of(N, kBlock);
    if (p_dtype == IVLM_BF16) depth_partial_kernel<true><<<nb, kBlock, 0, st>>>(verts, probs, N, threshold, part);
    else depth_partial_kernel<false><<<nb, kBlock, 0, st>>>(verts, probs, N, threshold, part);
    depth_finish_kernel<<<1, 64, 0, st>>>(part, nb, record, z_sum, z);
    return ivlm_launch_status();
}

int start_translation(const int64_t* mask_record, const int64_t* depth_record, const float* z, const float* cam, const float* offset,
                      int mirror, float* T, int64_t* status, hipStream_t st) {
    if (!mask_record || !depth_record || !z || !cam || !T || !status || (mirror != 0 && mirror != 1)) return IVLM_ERR_INVALID_ARG;
    start_translation_kernel<<<1, 64, 0, st>>>(mask_record, depth_record, z, cam, offset, mirror, T, status);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
int ivlm_mesh_vertex_normals(const float* verts, const int32_t* faces, const int32_t* vert_face_offsets, const int32_t* vert_face_list,
                             int N, int F, float* normals_out, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mesh_vertex_normals(verts, faces, vert_face_offsets, vert_face_list, N, F, normals_out, ivlm_stream(s));
}
size_t ivlm_mesh_surface_centroid_workspace_bytes(int F) { return ivlm::mesh_surface_centroid_workspace_bytes(F); }
int ivlm_mesh_surface_centroid(const float* verts, const int32_t* faces, int N, int F, float* centroid_out, int64_t* status_out,
                               void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mesh_surface_centroid(verts, faces, N, F, centroid_out, status_out, workspace, workspace_bytes, ivlm_stream(s));
}
size_t ivlm_mask_stats_workspace_bytes(int H, int W) { return ivlm::mask_stats_workspace_bytes(H, W); }
int ivlm_mask_stats(const uint8_t* mask, int H, int W, int64_t* record_out, void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mask_stats(mask, H, W, record_out, workspace, workspace_bytes, ivlm_stream(s));
}
size_t ivlm_contact_depth_workspace_bytes(int N) { return ivlm::contact_depth_workspace_bytes(N); }
int ivlm_contact_depth(const float* verts, const void* probs, int p_dtype, int N, float threshold, int64_t* record_out, double* z_sum_out,
                       float* z_out, void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::contact_depth(verts, probs, p_dtype, N, threshold, record_out, z_sum_out, z_out, workspace, workspace_bytes,
                               ivlm_stream(s));
}
int ivlm_start_translation(const int64_t* mask_record, const int64_t* depth_record, const float* z, const float* camera,
                           const float* centroid_offset, int mirror, float* translation_out, int64_t* status_out, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::start_translation(mask_record, depth_record, z, camera, centroid_offset, mirror, translation_out, status_out,
                                   ivlm_stream(s));
}
}
