// The metrics of the reference's validate() loop (evaluate.py:37-260) that are not in metrics.hip, kept on the device:
//   seg_iou_counts   get_segmentation_metrics / intersectionAndUnionGPU with K = 2 (utils/eval_utils.py:27-61): per view the
//                    (intersection, output area, target area) pixel counts of classes 0 and 1 of (pred > 0) against gt.int(),
//                    one streaming pass over the V x H x W masks (HBM-bound), integer counts => exact and bit-reproducible
//   afford_metrics   get_o_affordance_metrics (utils/eval_utils.py:153-213): SIM, MAE, ROC-AUC and the mean IoU over T
//                    thresholds per sample; the reference copies every sample to the host for sklearn's roc_auc_score and
//                    loops over the thresholds in Python.  One block per sample with the row in LDS; AUC as an integer pair count.
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ivlm {
namespace {

// ---- seg_iou_counts ----------------------------------------------------------------------------------------------------
// Stage 1: blockIdx.y = view, the view's pixels dealt to kSegBlocks blocks; a lane reads 16 B of pred and the 4 gt values
// beside them per load (a wave: 1 KiB of pred in full lines), four loads in flight per lane; six integer counters per lane,
// reduced over the wave by shuffles and over the block's 4 waves through LDS; the block stores its six sums.
// Stage 2: one wave per view adds the block sums in a fixed order.  No atomics, no floating point.
constexpr int kSegBlocks = 256;
constexpr int kSegThreads = 256;
constexpr int kSegUnroll = 4;

__device__ __forceinline__ void seg_count(float p, int g, int ignore, bool in_range, int (&c)[6]) {
    const int keep = in_range && g != ignore;  // a pixel whose gt is the ignore label counts nowhere
    const int o = p > 0.0f;                    // (pred > 0).int(); NaN is class 0
    c[0] += keep & (o == 0) & (g == 0);        // intersection = output[output == target], histc bins 0 / 1
    c[1] += keep & (o == 1) & (g == 1);
    c[2] += keep & (o == 0);                   // output area
    c[3] += keep & (o == 1);
    c[4] += keep & (g == 0);                   // target area: a gt value outside {0, 1} is in no bin
    c[5] += keep & (g == 1);
}

template <typename G, typename G4, bool VEC>
__global__ __launch_bounds__(kSegThreads) void seg_iou_partial_kernel(const float* __restrict__ pred, const G* __restrict__ gt,
                                                                      int64_t hw, int ignore,
                                                                      int32_t* __restrict__ partial /*[V][gridDim.x][6]*/) {
    __shared__ int s[6][kSegThreads / 64];
    const int v = blockIdx.y;
    const float* p = pred + (int64_t)v * hw;
    const G* g = gt + (int64_t)v * hw;
    const int64_t stride = (int64_t)gridDim.x * kSegThreads;
    int c[6] = {0, 0, 0, 0, 0, 0};
    if (VEC) {
        const int64_t nvec = hw >> 2;  // hw % 4 == 0 and 16-byte aligned bases (checked by the launcher)
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const G4* g4 = reinterpret_cast<const G4*>(g);
        for (int64_t i0 = (int64_t)blockIdx.x * kSegThreads + threadIdx.x; i0 < nvec; i0 += stride * kSegUnroll) {
            float4 a[kSegUnroll];
            G4 b[kSegUnroll];
            bool in[kSegUnroll];
#pragma unroll
            for (int u = 0; u < kSegUnroll; ++u) {
                const int64_t i = i0 + u * stride;
                in[u] = i < nvec;
                const int64_t j = in[u] ? i : i0;  // a clamped index keeps the load in bounds; its values are not counted
                a[u] = p4[j];
                b[u] = g4[j];
            }
#pragma unroll
            for (int u = 0; u < kSegUnroll; ++u) {
                seg_count(a[u].x, (int)b[u].x, ignore, in[u], c);
                seg_count(a[u].y, (int)b[u].y, ignore, in[u], c);
                seg_count(a[u].z, (int)b[u].z, ignore, in[u], c);
                seg_count(a[u].w, (int)b[u].w, ignore, in[u], c);
            }
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kSegThreads + threadIdx.x; i < hw; i += stride)
            seg_count(p[i], (int)g[i], ignore, true, c);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_xor(c[k], off, 64);
        if ((threadIdx.x & 63) == 0) s[k][threadIdx.x >> 6] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        int t = 0;
        for (int w = 0; w < kSegThreads / 64; ++w) t += s[threadIdx.x][w];
        partial[((int64_t)v * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void seg_iou_finish_kernel(const int32_t* __restrict__ partial, int blocks,
                                                            int32_t* __restrict__ out /*[V][3][2]*/) {
    const int v = blockIdx.x, lane = threadIdx.x;
    for (int k = 0; k < 6; ++k) {
        int t = 0;
        for (int b = lane; b < blocks; b += 64) t += partial[((int64_t)v * blocks + b) * 6 + k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) out[v * 6 + k] = t;
    }
}

template <typename G, typename G4>
void seg_iou_launch(const float* pred, const void* gt, int V, int64_t hw, int ignore, int32_t* partial, int blocks, bool vec,
                    hipStream_t st) {
    const G* g = static_cast<const G*>(gt);
    if (vec)
        seg_iou_partial_kernel<G, G4, true><<<dim3(blocks, V), kSegThreads, 0, st>>>(pred, g, hw, ignore, partial);
    else
        seg_iou_partial_kernel<G, G4, false><<<dim3(blocks, V), kSegThreads, 0, st>>>(pred, g, hw, ignore, partial);
}

// ---- afford_metrics ----------------------------------------------------------------------------------------------------
constexpr int kAffordMaxN = IVLM_AFFORD_MAX_N;  // row length held in LDS: 9 bytes per element
constexpr int kAffordMaxT = IVLM_AFFORD_MAX_T;
constexpr int kAffordThreads = 512;
constexpr int kAffordWaves = kAffordThreads / 64;

// sum over the block in a fixed order (lanes by shuffle, then the waves in index order); every thread gets the total
__device__ __forceinline__ double afford_block_sum(double v, double* sh /*[kAffordWaves]*/) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // (sh may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < kAffordWaves; ++w) t += sh[w];
    return t;
}

__device__ __forceinline__ unsigned afford_block_sum_u(unsigned v, unsigned* sh /*[kAffordWaves]*/) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned t = 0;
    for (int w = 0; w < kAffordWaves; ++w) t += sh[w];
    return t;
}

__global__ __launch_bounds__(kAffordThreads) void afford_metrics_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                                        int n, const float* __restrict__ thresholds, int T,
                                                                        float mae_div, float* __restrict__ out /*[B,4]*/,
                                                                        int32_t* __restrict__ valid /*[B]*/) {
    __shared__ __attribute__((aligned(16))) float s_pred[kAffordMaxN];
    __shared__ __attribute__((aligned(16))) float s_neg[kAffordMaxN];  // pred of the gt < 0.5 entries, NaN elsewhere
    __shared__ uint8_t s_lab[kAffordMaxN];                             // gt >= 0.5
    __shared__ double s_d[kAffordWaves];
    __shared__ unsigned s_u[kAffordWaves];
    __shared__ double s_iou[kAffordMaxT];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* g = gt + (int64_t)b * n;
    const float* p = pred + (int64_t)b * n;
    const float nan = __builtin_nanf("");
    const int n4 = (n + 3) & ~3;  // <= kAffordMaxN (a multiple of 4)

    // pass 1: the row into LDS; sum(gt), sum(pred), sum|gt - pred| in fp64, positives, finiteness of pred
    double sg = 0.0, sp = 0.0, sa = 0.0;
    unsigned npos = 0, nbad = 0;
#pragma unroll 1
    for (int i = tid; i < n4; i += kAffordThreads) {
        if (i < n) {
            const float gi = g[i], pi = p[i];
            const bool lab = gi >= 0.5f;
            s_pred[i] = pi;
            s_neg[i] = lab ? nan : pi;
            s_lab[i] = lab;
            sg += (double)gi;
            sp += (double)pi;
            sa += fabs((double)gi - (double)pi);
            npos += lab;
            nbad += !(fabsf(pi) <= 3.402823466e38f);  // NaN or +-inf
        } else {
            s_neg[i] = nan;  // padding of the last float4: compares false
        }
    }
    sg = afford_block_sum(sg, s_d);
    sp = afford_block_sum(sp, s_d);
    sa = afford_block_sum(sa, s_d);
    npos = afford_block_sum_u(npos, s_u);
    nbad = afford_block_sum_u(nbad, s_u);  // (the barriers inside also publish the LDS row)

    // SIM = sum min(gt / (sum gt + eps), pred / (sum pred + eps)), eps = 1e-12; torch.min propagates NaN
    const double ig = 1.0 / (sg + 1e-12), ip = 1.0 / (sp + 1e-12);
    double sim = 0.0;
#pragma unroll 1
    for (int i = tid; i < n; i += kAffordThreads) {
        const double a = (double)g[i] * ig, c = (double)s_pred[i] * ip;
        sim += (a != a || c != c) ? (double)nan : (a < c ? a : c);
    }
    sim = afford_block_sum(sim, s_d);

    // AUC = (#{pos > neg} + 0.5 #{pos == neg}) / (P N): a thread owns positives, every negative is read from LDS as a broadcast
    unsigned c2 = 0;  // 2 #{>} + #{==} <= 2 P N <= n^2 / 2 < 2^32
#pragma unroll 1
    for (int i = tid; i < n; i += kAffordThreads) {
        if (!s_lab[i]) continue;
        const float pi = s_pred[i];
#pragma unroll 2
        for (int j = 0; j < n4; j += 4) {
            const float4 q = *reinterpret_cast<const float4*>(&s_neg[j]);
            c2 += 2u * (pi > q.x) + (pi == q.x);
            c2 += 2u * (pi > q.y) + (pi == q.y);
            c2 += 2u * (pi > q.z) + (pi == q.z);
            c2 += 2u * (pi > q.w) + (pi == q.w);
        }
    }
    c2 = afford_block_sum_u(c2, s_u);

    // aIoU: a wave owns thresholds wave, wave + 8, ...; |pred >= t & gt| / |pred >= t | gt| from integer counts
    for (int t = wave; t < T; t += kAffordWaves) {
        const float thr = thresholds[t];  // fp32 compare, as torch compares an fp32 tensor with a scalar
        int ci = 0, cu = 0;
#pragma unroll 2
        for (int j = lane; j < n; j += 64) {
            const int pb = s_pred[j] >= thr, lb = s_lab[j];
            ci += pb & lb;
            cu += pb | lb;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            ci += __shfl_xor(ci, off, 64);
            cu += __shfl_xor(cu, off, 64);
        }
        if (lane == 0) s_iou[t] = (double)ci / (double)cu;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned nneg = (unsigned)n - npos;
        const bool ok = npos > 0 && nneg > 0 && nbad == 0;  // single-class gt / non-finite pred: no AUC, no aIoU
        double iou = 0.0;
        for (int t = 0; t < T; ++t) iou += s_iou[t];
        out[4 * b + 0] = (float)sim;
        out[4 * b + 1] = (float)(sa / (double)mae_div);
        out[4 * b + 2] = ok ? (float)((double)c2 / (2.0 * (double)npos * (double)nneg)) : nan;
        out[4 * b + 3] = ok ? (float)(iou / (double)T) : nan;
        valid[b] = ok;
    }
}

}  // namespace

size_t seg_iou_workspace_bytes(int V) { return V > 0 ? (size_t)V * kSegBlocks * 6 * sizeof(int32_t) : 0; }

int seg_iou_counts(const float* pred, const void* gt, int gt_dtype, int V, int H, int W, int ignore_label, int32_t* out, void* ws,
                   size_t ws_bytes, hipStream_t st) {
    if (!pred || !gt || !out || !ws || V <= 0 || H <= 0 || W <= 0) return IVLM_ERR_INVALID_ARG;
    if (gt_dtype != IVLM_SEG_GT_U8 && gt_dtype != IVLM_SEG_GT_I32 && gt_dtype != IVLM_SEG_GT_F32) return IVLM_ERR_UNSUPPORTED;
    const int64_t hw = (int64_t)H * W;
    if (hw >= ((int64_t)1 << 31) || V > 65535) return IVLM_ERR_UNSUPPORTED;  // int32 counts per view; grid y
    if (ws_bytes < seg_iou_workspace_bytes(V)) return IVLM_ERR_WORKSPACE;
    const size_t gsz = gt_dtype == IVLM_SEG_GT_U8 ? 1 : 4;
    const bool vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(pred) % 16 == 0 && reinterpret_cast<uintptr_t>(gt) % (4 * gsz) == 0;
    const int64_t units = vec ? hw / 4 : hw;
    const int blocks = (int)std::min<int64_t>(kSegBlocks, (units + kSegThreads - 1) / kSegThreads);
    int32_t* partial = static_cast<int32_t*>(ws);
    if (gt_dtype == IVLM_SEG_GT_U8)
        seg_iou_launch<uint8_t, uchar4>(pred, gt, V, hw, ignore_label, partial, blocks, vec, st);
    else if (gt_dtype == IVLM_SEG_GT_I32)
        seg_iou_launch<int32_t, int4>(pred, gt, V, hw, ignore_label, partial, blocks, vec, st);
    else
        seg_iou_launch<float, float4>(pred, gt, V, hw, ignore_label, partial, blocks, vec, st);
    seg_iou_finish_kernel<<<V, 64, 0, st>>>(partial, blocks, out);
    return ivlm_launch_status();
}

int afford_metrics(const float* gt, const float* pred, int B, int n, const float* thresholds, int T, float mae_div, float* out,
                   int32_t* valid, hipStream_t st) {
    if (!gt || !pred || !thresholds || !out || !valid || B <= 0 || n <= 0 || T <= 0 || !(mae_div > 0.0f)) return IVLM_ERR_INVALID_ARG;
    if (n > kAffordMaxN || T > kAffordMaxT) return IVLM_ERR_UNSUPPORTED;  // before any launch
    afford_metrics_kernel<<<B, kAffordThreads, 0, st>>>(gt, pred, n, thresholds, T, mae_div, out, valid);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_seg_iou_workspace_bytes(int V) { return ivlm::seg_iou_workspace_bytes(V); }
int ivlm_seg_iou_counts(const float* pred, const void* gt, int gt_dtype, int V, int H, int W, int ignore_label, int32_t* out,
                        void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::seg_iou_counts(pred, gt, gt_dtype, V, H, W, ignore_label, out, workspace, workspace_bytes, ivlm_stream(s));
}
int ivlm_afford_metrics(const float* gt, const float* pred, int B, int n, const float* thresholds, int T, float mae_div, float* out,
                        int32_t* valid, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::afford_metrics(gt, pred, B, n, thresholds, T, mae_div, out, valid, ivlm_stream(s));
}
}
