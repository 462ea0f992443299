// The rigid transform of the object-pose fit for B poses at once, forward and backward (the reference's optim/utils.py
// `apply_transformation`; interactvlm_amd.fit.apply_transformation keeps its conventions):
//
//   a1, a2 = the two interleaved columns of rot6d;  b1 = a1 / max(|a1|, 1e-12);  u2 = a2 - (b1.a2) b1;  b2 = u2 / max(|u2|, 1e-12)
//   b3 = b1 x b2;  R = [b1 b2 b3] (columns);  y_n = (s v_n) R + t  (row vectors)
//
// Three launches, no atomics, every sum in a fixed order that depends on N only (the same bits every call, for a pose whatever
// the batch around it, and under graph replay):
//   pose_forward   grid (vertex chunk, pose).  Thread 0 of a block rebuilds its pose's R in fp64 from the six numbers, rounds it
//                  once to fp32 and hands R, t, s to the block through LDS (13 floats, read by all lanes at one address).
//   pose_partial   grid (vertex chunk, pose), IVLM_POSE_CHUNK vertices per block.  The backward's reduction does not depend on the
//                  pose: per (chunk, pose) the twelve sums G = sum_n v_n^T g_n (3 x 3) and sum_n g_n.  Every product v_i g_j of two
//                  floats is exact in fp64 and is added in fp64 from the first term (the fp32 chain is IVLM_POSE_CHAIN = 1): per
//                  lane its kPerThread vertices in ascending order, then the 64 lanes by wave_sum, then the waves in order.  A
//                  vertex past N adds exact zeros.
//   pose_finish    one wave per pose: lanes 0..11 add the partials of one sum each in ascending chunk order; lane 0 chains
//                  dL/dR = s G through the Gram-Schmidt analytically, all in fp64, and rounds each result to fp32 once.
//                  dL/dt = sum g;  dL/ds = sum_ij R_ij G_ij.
// The Gram-Schmidt and its chain are rot6d.h's (shared with mesh_sdf.hip).
#include <cstdint>

#include "fit_common.h"
#include "rot6d.h"

namespace ivlm {
namespace {

constexpr int kChunk = IVLM_POSE_CHUNK;  // vertices per block
constexpr int kThreads = 256;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxN = 1 << 22;
static_assert(kChunk % kThreads == 0, "a chunk is a whole number of vertices per thread");

__global__ __launch_bounds__(kThreads) void pose_forward_kernel(const float* __restrict__ verts, const float* __restrict__ rot6d,
                                                                const float* __restrict__ trans, const float* __restrict__ scale, int N,
                                                                float* __restrict__ out) {
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
    float R[9], T[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = pose[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) T[i] = pose[9 + i];
    const float s = pose[12];
    float* o = out + (int64_t)b * N * 3;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int n = blockIdx.x * kChunk + k * kThreads + t;
        if (n < N) {
            const float x = verts[(int64_t)n * 3] * s, y = verts[(int64_t)n * 3 + 1] * s, z = verts[(int64_t)n * 3 + 2] * s;
#pragma unroll
            for (int j = 0; j < 3; ++j) o[(int64_t)n * 3 + j] = fmaf(z, R[6 + j], fmaf(y, R[3 + j], fmaf(x, R[j], T[j])));
        }
    }
}

// part[(b * chunks + chunk) * 12 + k]: k = 3 i + j is G_ij = sum v_i g_j, k = 9 + j is sum g_j
__global__ __launch_bounds__(kThreads) void pose_partial_kernel(const float* __restrict__ verts, const float* __restrict__ g, int N,
                                                                double* __restrict__ part) {
    __shared__ double red[kWaves][12];
    const int b = blockIdx.y, t = threadIdx.x;
    const float* gb = g + (int64_t)b * N * 3;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int n = blockIdx.x * kChunk + k * kThreads + t;
        double v[3] = {0.0, 0.0, 0.0}, gn[3] = {0.0, 0.0, 0.0};
        if (n < N) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v[i] = (double)verts[(int64_t)n * 3 + i];
                gn[i] = (double)gb[(int64_t)n * 3 + i];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 * i + j] += v[i] * gn[j];
            acc[9 + i] += gn[i];
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) red[t >> 6][k] = acc[k];
    }
    __syncthreads();
    // NOT block4_sum's order: the waves are added one after the other, ((w0 + w1) + w2) + w3 - only the butterfly is the shared one
    if (t < 12) {
        double s = red[0][t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += red[w][t];
        part[((int64_t)b * gridDim.x + blockIdx.x) * 12 + t] = s;
    }
}

__global__ __launch_bounds__(64) void pose_finish_kernel(const float* __restrict__ rot6d, const float* __restrict__ scale,
                                                         const double* __restrict__ part, int chunks, float* __restrict__ grad_r6,
                                                         float* __restrict__ grad_t, float* __restrict__ grad_s) {
    __shared__ double sums[12];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 12) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += part[((int64_t)b * chunks + c) * 12 + t];
        sums[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    if (grad_t) {
#pragma unroll
        for (int j = 0; j < 3; ++j) grad_t[(int64_t)b * 3 + j] = (float)sums[9 + j];
    }
    if (!grad_r6 && !grad_s) return;
    const Frame f = gram_schmidt(rot6d + (int64_t)b * 6);
    if (grad_s) {
        double gs = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) gs += f.b1[i] * sums[3 * i] + f.b2[i] * sums[3 * i + 1] + f.b3[i] * sums[3 * i + 2];
        grad_s[b] = (float)gs;
    }
    if (!grad_r6) return;
    const double s = (double)scale[b];
    double gb1[3], gb2[3], gb3[3], ga1[3], ga2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // dL/dR = s G, by columns
        gb1[i] = s * sums[3 * i];
        gb2[i] = s * sums[3 * i + 1];
        gb3[i] = s * sums[3 * i + 2];
    }
    gram_schmidt_backward(f, gb1, gb2, gb3, ga1, ga2);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        grad_r6[(int64_t)b * 6 + 2 * i] = (float)ga1[i];
        grad_r6[(int64_t)b * 6 + 2 * i + 1] = (float)ga2[i];
    }
}

inline bool pose_sizes_ok(int B, int N) { return B > 0 && N > 0 && B <= 65535 && N <= kMaxN; }

}  // namespace

size_t pose_transform_workspace_bytes(int B, int N) {
    if (!pose_sizes_ok(B, N)) return 0;
    const size_t chunks = (size_t)(N + kChunk - 1) / kChunk;
    Carve c;
    c.take((size_t)B * chunks * 12 * sizeof(double));
    return c.off;
}

int pose_transform_forward(const float* verts, const float* rot6d, const float* trans, const float* scale, int B, int N, float* out,
                           hipStream_t st) {
    if (!verts || !rot6d || !trans || !scale || !out || B <= 0 || N <= 0) return IVLM_ERR_INVALID_ARG;
    if (!pose_sizes_ok(B, N)) return IVLM_ERR_UNSUPPORTED;
    const int chunks = (N + kChunk - 1) / kChunk;
    pose_forward_kernel<<<dim3(chunks, B), kThreads, 0, st>>>(verts, rot6d, trans, scale, N, out);
    return ivlm_launch_status();
}

int pose_transform_backward(const float* verts, const float* rot6d, const float* scale, const float* grad_out, int B, int N,
                            float* grad_r6, float* grad_t, float* grad_s, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!verts || !rot6d || !scale || !grad_out || !ws || B <= 0 || N <= 0 || (!grad_r6 && !grad_t && !grad_s))
        return IVLM_ERR_INVALID_ARG;
    if (!pose_sizes_ok(B, N)) return IVLM_ERR_UNSUPPORTED;
    if (!workspace_ok(ws, ws_bytes, pose_transform_workspace_bytes(B, N), 16)) return IVLM_ERR_WORKSPACE;
    const int chunks = (N + kChunk - 1) / kChunk;
    double* part = static_cast<double*>(ws);
    pose_partial_kernel<<<dim3(chunks, B), kThreads, 0, st>>>(verts, grad_out, N, part);
    pose_finish_kernel<<<B, 64, 0, st>>>(rot6d, scale, part, chunks, grad_r6, grad_t, grad_s);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_pose_transform_workspace_bytes(int B, int N) { return ivlm::pose_transform_workspace_bytes(B, N); }
int ivlm_pose_transform_forward(const float* verts, const float* rot6d, const float* translation, const float* scale, int B, int N,
                                float* out, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::pose_transform_forward(verts, rot6d, translation, scale, B, N, out, ivlm_stream(s));
}
int ivlm_pose_transform_backward(const float* verts, const float* rot6d, const float* scale, const float* grad_out, int B, int N,
                                 float* grad_rot6d, float* grad_translation, float* grad_scale, void* workspace, size_t workspace_bytes,
                                 ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::pose_transform_backward(verts, rot6d, scale, grad_out, B, N, grad_rot6d, grad_translation, grad_scale, workspace,
                                         workspace_bytes, ivlm_stream(s));
}
}
