// The filter stage behind the promptable mask decoder (segment_anything/automatic_mask_generator.py:_process_batch / _process_crop)
// for gfx950, without the full-resolution logits:
//   ivlm_mask_census  per candidate, the three threshold counts and the box of {v > t_mid}, v = Sam.postprocess_masks(low)[y, x]
//                     evaluated on the fly from the low-res source (bilinear.h: the operations of postprocess_kernel, one by one)
//   ivlm_box_nms      torchvision's box NMS on boxes already in score order: a bit matrix of suppressions, then one wave that
//                     walks the rows in order
// Integer results only: the order in which blocks combine does not change them.
#include <limits.h>

#include "bilinear.h"

namespace {
using namespace ivlm_bilinear;

constexpr int CENSUS_COLS = 8;
constexpr int CENSUS_BLOCKS = 8192;  // blocks per launch aimed at: a candidate gets ceil(CENSUS_BLOCKS / n) of them, at most one per row

// counts 0, an empty box as (INT_MAX, INT_MAX, -1, -1): what the atomics of census_kernel fold into
__global__ __launch_bounds__(256) void census_init_kernel(int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * CENSUS_COLS) return;
    const int c = i & (CENSUS_COLS - 1);
    out[i] = (c == 3 || c == 4) ? INT_MAX : ((c == 5 || c == 6) ? -1 : 0);
}

// an empty {v > t_mid} has the box 0, 0, 0, 0 (batched_mask_to_box)
__global__ __launch_bounds__(256) void census_finish_kernel(int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t* o = out + (size_t)i * CENSUS_COLS;
    if (o[1] == 0) o[3] = o[4] = o[5] = o[6] = 0;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// stage1 with the row axis `ay` taken by the caller (the same axis_src call, once per output row instead of once per tap)
__device__ __forceinline__ float stage1_row(const float* __restrict__ r0, const float* __restrict__ r1, const Axis ay, const Axis ax) {
    const float t = r0[ax.i0] * ax.l0 + r0[ax.i1] * ax.l1;
    const float b = r1[ax.i0] * ax.l0 + r1[ax.i1] * ax.l1;
    return t * ay.l0 + b * ay.l1;
}

// grid (blocks per candidate, n): block bx of candidate i walks the rows bx, bx + gridDim.x, ...; a thread the pixels tid, tid + 256, ...
template <bool IDENT2>
__global__ __launch_bounds__(256) void census_kernel(const float* __restrict__ low, int h, int w, int img, int in_h, int in_w, int oh,
                                                     int ow, float t_hi, float t_mid, float t_lo, const int32_t* __restrict__ active,
                                                     int32_t* __restrict__ out) {
    const int i = blockIdx.y;
    if (active && active[i] == 0) return;  // (the whole block: no sampling; census_init / census_finish leave the row zero)
    const float* lowp = low + (size_t)i * h * w;
    const float s1y = (float)h / (float)img, s1x = (float)w / (float)img;
    const float s2y = (float)in_h / (float)oh, s2x = (float)in_w / (float)ow;
    int c_hi = 0, c_mid = 0, c_lo = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int y = blockIdx.x; y < oh; y += gridDim.x) {
        const Axis by = IDENT2 ? Axis{y, y, 1.0f, 0.0f} : axis_src(y, s2y, in_h);
        const Axis ay0 = axis_src(by.i0, s1y, h), ay1 = axis_src(by.i1, s1y, h);
        const float* r00 = lowp + (size_t)ay0.i0 * w;
        const float* r01 = lowp + (size_t)ay0.i1 * w;
        const float* r10 = lowp + (size_t)ay1.i0 * w;
        const float* r11 = lowp + (size_t)ay1.i1 * w;
        int row_mid = 0;
        for (int x = threadIdx.x; x < ow; x += 256) {
            float v;
            if (IDENT2) {
                v = stage1_row(r00, r01, ay0, axis_src(x, s1x, w));
            } else {
                const Axis bx = axis_src(x, s2x, in_w);
                const Axis ax0 = axis_src(bx.i0, s1x, w), ax1 = axis_src(bx.i1, s1x, w);
                const float a = stage1_row(r00, r01, ay0, ax0);
                const float b = stage1_row(r00, r01, ay0, ax1);
                const float c = stage1_row(r10, r11, ay1, ax0);
                const float d = stage1_row(r10, r11, ay1, ax1);
                v = (a * bx.l0 + b * bx.l1) * by.l0 + (c * bx.l0 + d * bx.l1) * by.l1;
            }
            c_hi += v > t_hi;
            c_lo += v > t_lo;
            if (v > t_mid) {
                ++row_mid;
                x0 = min(x0, x);
                x1 = max(x1, x);
            }
        }
        if (row_mid) {
            c_mid += row_mid;
            y0 = min(y0, y);
            y1 = max(y1, y);
        }
    }
    // thread -> wave -> block -> out
    c_hi = wave_sum_i(c_hi), c_mid = wave_sum_i(c_mid), c_lo = wave_sum_i(c_lo);
    x0 = wave_min_i(x0), y0 = wave_min_i(y0), x1 = wave_max_i(x1), y1 = wave_max_i(y1);
    __shared__ int part[4][7];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = c_hi, part[wave][1] = c_mid, part[wave][2] = c_lo;
        part[wave][3] = x0, part[wave][4] = y0, part[wave][5] = x1, part[wave][6] = y1;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; ++k) {
        c_hi += part[k][0], c_mid += part[k][1], c_lo += part[k][2];
        x0 = min(x0, part[k][3]), y0 = min(y0, part[k][4]), x1 = max(x1, part[k][5]), y1 = max(y1, part[k][6]);
    }
    int32_t* o = out + (size_t)i * CENSUS_COLS;
    if (c_hi) atomicAdd(o + 0, c_hi);
    if (c_lo) atomicAdd(o + 2, c_lo);
    if (c_mid) {
        atomicAdd(o + 1, c_mid);
        atomicMin(o + 3, x0), atomicMin(o + 4, y0), atomicMax(o + 5, x1), atomicMax(o + 6, y1);
    }
}

// ---- box NMS ----------------------------------------------------------------------------------------------------------------------
constexpr int NMS_MAX = 16384;
constexpr int NMS_WORDS_MAX = NMS_MAX / 64;

// grid (ceil(W / 4), n), one wave per 64-bit word: bit l of word (i, wj) is set when j = 64 wj + l > i, both rows are valid and
// IoU(i, j) > thr in torchvision's fp32 arithmetic
__global__ __launch_bounds__(256) void nms_pair_kernel(const float4* __restrict__ boxes, const int32_t* __restrict__ valid, int n, int W,
                                                       float thr, unsigned long long* __restrict__ mat) {
    const int i = blockIdx.y;
    const int wj = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wj >= W) return;
    const int lane = threadIdx.x & 63;
    const int j = wj * 64 + lane;
    bool hit = false;
    if (j > i && j < n && (!valid || (valid[i] != 0 && valid[j] != 0))) {
        const float4 a = boxes[i], b = boxes[j];
        const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
        const float dx = fminf(a.z, b.z) - fmaxf(a.x, b.x), dy = fminf(a.w, b.w) - fmaxf(a.y, b.y);
        const float inter = (dx > 0.0f ? dx : 0.0f) * (dy > 0.0f ? dy : 0.0f);
        hit = inter / (area_a + area_b - inter) > thr;  // 0 / 0 is NaN: not above
    }
    const unsigned long long word = __ballot(hit);
    if (lane == 0) mat[(size_t)i * W + wj] = word;
}

// one wave: rows in order, 64 at a time; a row is kept when it is valid and no kept row before it has its bit set, and only a kept
// row's suppressions are ORed into `removed`
__global__ __launch_bounds__(64) void nms_scan_kernel(const unsigned long long* __restrict__ mat, const int32_t* __restrict__ valid, int n,
                                                      int W, int32_t* __restrict__ keep) {
    __shared__ unsigned long long removed[NMS_WORDS_MAX];
    __shared__ unsigned long long ok[NMS_WORDS_MAX];
    const int lane = threadIdx.x;
    for (int wd = 0; wd < W; ++wd) {
        const int j = wd * 64 + lane;
        const unsigned long long v = __ballot(j < n && (!valid || valid[j] != 0));
        if (lane == 0) ok[wd] = v, removed[wd] = 0ull;
    }
    __syncthreads();
    for (int wc = 0; wc < W; ++wc) {
        unsigned long long cand = ok[wc] & ~removed[wc];  // the same value in every lane
        unsigned long long kept = 0ull;
        while (cand) {
            const int b = __ffsll((long long)cand) - 1;
            const unsigned long long* row = mat + (size_t)(wc * 64 + b) * W;
            kept |= 1ull << b;
            for (int wd = wc + 1 + lane; wd < W; wd += 64) removed[wd] |= row[wd];
            cand &= ~(row[wc] | (1ull << b));
        }
        const int j = wc * 64 + lane;
        if (j < n) keep[j] = (int32_t)((kept >> lane) & 1ull);
        __syncthreads();  // (the word a lane ORs into changes with wc)
    }
}

}  // namespace

// low f32 [n,h,w] -> out i32 [n,8]; see include/ivlm_hip.h
extern "C" int ivlm_mask_census(const float* low, int n, int h, int w, int img, int in_h, int in_w, int oh, int ow, float t_hi,
                                float t_mid, float t_lo, const int32_t* active, int32_t* out, ivlm_stream_t stream) {
    IVLM_CHECK_ARG(low && out);
    IVLM_CHECK_ARG(n > 0 && h > 0 && w > 0 && img > 0 && oh > 0 && ow > 0);
    IVLM_CHECK_ARG(in_h > 0 && in_w > 0 && in_h <= img && in_w <= img);
    if (n > 65535 || (int64_t)oh * ow >= (1ll << 31)) return IVLM_ERR_UNSUPPORTED;  // grid.y; the counts are int32
    hipStream_t st = ivlm_stream(stream);
    ivlm_enter();
    int per = (CENSUS_BLOCKS + n - 1) / n;
    per = per > oh ? oh : per;
    const dim3 grid(per, n);
    census_init_kernel<<<(n * CENSUS_COLS + 255) / 256, 256, 0, st>>>(out, n);
    if (in_h == oh && in_w == ow)
        census_kernel<true><<<grid, 256, 0, st>>>(low, h, w, img, in_h, in_w, oh, ow, t_hi, t_mid, t_lo, active, out);
    else
        census_kernel<false><<<grid, 256, 0, st>>>(low, h, w, img, in_h, in_w, oh, ow, t_hi, t_mid, t_lo, active, out);
    census_finish_kernel<<<(n + 255) / 256, 256, 0, st>>>(out, n);
    return ivlm_launch_status();
}

extern "C" size_t ivlm_box_nms_workspace_bytes(int n) {
    if (n < 1 || n > NMS_MAX) return 0;
    return (size_t)n * ((n + 63) / 64) * sizeof(unsigned long long);
}

// boxes f32 [n,4] XYXY in score order -> keep i32 [n]; see include/ivlm_hip.h
extern "C" int ivlm_box_nms(const float* boxes, const int32_t* valid, int n, float iou_threshold, int32_t* keep, void* workspace,
                            size_t workspace_bytes, ivlm_stream_t stream) {
    IVLM_CHECK_ARG(boxes && keep && workspace && n > 0);
    IVLM_CHECK_ARG((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
    if (n > NMS_MAX) return IVLM_ERR_UNSUPPORTED;
    if (workspace_bytes < ivlm_box_nms_workspace_bytes(n)) return IVLM_ERR_WORKSPACE;
    hipStream_t st = ivlm_stream(stream);
    ivlm_enter();
    const int W = (n + 63) / 64;
    unsigned long long* mat = static_cast<unsigned long long*>(workspace);
    nms_pair_kernel<<<dim3((W + 3) / 4, n), 256, 0, st>>>(reinterpret_cast<const float4*>(boxes), valid, n, W, iou_threshold, mat);
    nms_scan_kernel<<<1, 64, 0, st>>>(mat, valid, n, W, keep);
    return ivlm_launch_status();
}
