// Band census: how many results of a call sit within a margin of a decision threshold.
//
// The vertex-id sets {p >= 0.5} and {p > 0.3} of a contact map computed in a reduced-precision mode can differ from the fp32
// oracle's only at vertices whose probability lies within that mode's error of the threshold; the thresholded object-mesh lift
// (lift.hip MODE 1, components.py:445-489) adds the pixels whose sigmoid(logit) lies within the mask error of its own 0.3.  These
// kernels count both populations on the device; the policy that reads the counts is InteractVLMForCausalLM.evaluate(exact_sets=).
//
//   contact_band_census   p f32 [B, Nv] (row stride ld) -> per row and threshold the number of finite p with |p - thr| <= margin,
//                         the number of non-finite p and the smallest |p - thr| over the finite ones.  One block per row.
//   mask_band_census      the pixel ENTRIES of a resident lift plan (the CSR of ivlm_lift_plan_build) whose logit sits in the band
//                         of the lift's threshold, walked like lift_plan_kernel: one wave per CSR row, lanes stride its entries.
//
// Both are streaming reads (HBM / L2 bound), integer counts and fminf only: any summation order gives the same bits; the orders
// are fixed all the same (wave butterfly, waves in index order, blocks in index order by a second launch).  No atomics, plain
// vector stores.
#include "kernels.h"

namespace ivlm {
namespace {

constexpr int kCensusBlock = 256;
constexpr int kCensusWaves = kCensusBlock / 64;
constexpr int kMaxThr = 4;
constexpr int kMaskBlocks = 1024;  // partial slots of the mask census (4 blocks per CU)

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) < __builtin_inff(); }  // false for NaN and +-inf

struct BandAcc {
    int cnt[kMaxThr];
    float mind[kMaxThr];
    int nonfinite;
};

template <int J>
__device__ __forceinline__ void band_visit(BandAcc& a, float x, const float (&t)[kMaxThr], float margin) {
    if (!finite_f32(x)) {
        ++a.nonfinite;
        return;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const float d = fabsf(x - t[j]);
        a.cnt[j] += d <= margin;
        a.mind[j] = fminf(a.mind[j], d);
    }
}

template <int J>
__global__ __launch_bounds__(kCensusBlock) void contact_band_census_kernel(const float* __restrict__ p, int64_t ld, int nv,
                                                                           const float* __restrict__ thr, float margin, int vec4,
                                                                           int32_t* __restrict__ counts /*[B,J+1]*/,
                                                                           float* __restrict__ mindist /*[B,J]*/) {
    __shared__ int s_cnt[kCensusWaves][kMaxThr + 1];
    __shared__ float s_min[kCensusWaves][kMaxThr];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ row = p + (int64_t)b * ld;
    float t[kMaxThr];
    BandAcc a;
    a.nonfinite = 0;
#pragma unroll
    for (int j = 0; j < kMaxThr; ++j) {
        t[j] = j < J ? thr[j] : 0.0f;
        a.cnt[j] = 0;
        a.mind[j] = __builtin_inff();
    }
    int done = 0;
    if (vec4) {  // every row starts on a 16-byte boundary: 16-byte loads over the multiple-of-4 body, scalar tail
        const int n4 = nv >> 2;
        const float4* __restrict__ row4 = reinterpret_cast<const float4*>(row);
        for (int i = threadIdx.x; i < n4; i += kCensusBlock) {
            const float4 x = row4[i];
            band_visit<J>(a, x.x, t, margin);
            band_visit<J>(a, x.y, t, margin);
            band_visit<J>(a, x.z, t, margin);
            band_visit<J>(a, x.w, t, margin);
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < nv; i += kCensusBlock) band_visit<J>(a, row[i], t, margin);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.nonfinite += __shfl_xor(a.nonfinite, off, 64);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            a.cnt[j] += __shfl_xor(a.cnt[j], off, 64);
            a.mind[j] = fminf(a.mind[j], __shfl_xor(a.mind[j], off, 64));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            s_cnt[wave][j] = a.cnt[j];
            s_min[wave][j] = a.mind[j];
        }
        s_cnt[wave][J] = a.nonfinite;
    }
    __syncthreads();
    if (threadIdx.x <= J) {  // thread j finishes threshold j, thread J the non-finite count: waves in index order
        const int j = threadIdx.x;
        int c = 0;
        for (int w = 0; w < kCensusWaves; ++w) c += s_cnt[w][j];
        counts[(int64_t)b * (J + 1) + j] = c;
        if (j < J) {
            float m = s_min[0][j];
            for (int w = 1; w < kCensusWaves; ++w) m = fminf(m, s_min[w][j]);
            mindist[(int64_t)b * J + j] = m;
        }
    }
}

// One wave per CSR row (row = view * Nv + vertex, as lift_plan_body indexes it), lanes stride the row's entries: 256-byte
// contiguous loads of ent_pix, one gathered logit each.  Block `blockIdx.x` owns the contiguous rows [r0, r1) - neighbouring
// vertices of one view, whose pixels are neighbours in the mask.  An entry is a (pixel, vertex) pair: a pixel inside a triangle
// has three entries, so the count says "none / some", not how many distinct pixels.
__global__ __launch_bounds__(kCensusBlock) void mask_band_partial_kernel(const float* __restrict__ logits, int64_t HW,
                                                                         const int32_t* __restrict__ ent_pix,
                                                                         const int32_t* __restrict__ row_ptr, int n_rows,
                                                                         int rows_per_view, int rows_per_block, float thr,
                                                                         float margin, int32_t* __restrict__ partial /*[grid,2]*/) {
    __shared__ int s_cnt[kCensusWaves][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(r0 + rows_per_block, n_rows);
    int band = 0, bad = 0;
    for (int row = r0 + wave; row < r1; row += kCensusWaves) {
        const float* __restrict__ lg = logits + (int64_t)(row / rows_per_view) * HW;
        const int s = row_ptr[row], e = row_ptr[row + 1];
        // 4-deep predicated unroll, as lift_plan_body: the entry loads of a typical row are all in flight before the first gather
        for (int i = s + lane; i < e; i += 256) {
            int pix[4];
            float x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) pix[k] = ent_pix[min(i + 64 * k, e - 1)];  // clamped: the load is always legal
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = (uint32_t)pix[k] < (uint32_t)HW;  // (always, for a plan of ivlm_lift_plan_build: keeps the gather in bounds)
                x[k] = lg[in ? pix[k] : 0];
                if (!in) x[k] = 0.0f, pix[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + 64 * k >= e || pix[k] < 0) continue;
                if (!finite_f32(x[k])) {
                    ++bad;
                } else {
                    band += fabsf(sigmoid_f32(x[k]) - thr) <= margin;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        band += __shfl_xor(band, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
        s_cnt[wave][0] = band;
        s_cnt[wave][1] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int c = 0;
        for (int w = 0; w < kCensusWaves; ++w) c += s_cnt[w][threadIdx.x];
        partial[2 * blockIdx.x + threadIdx.x] = c;
    }
}

// counts[k] = sum of the blocks' partials in block order (one block; thread t owns the blocks t, t + 256, ...)
__global__ __launch_bounds__(kCensusBlock) void mask_band_finish_kernel(const int32_t* __restrict__ partial, int blocks,
                                                                        int32_t* __restrict__ counts) {
    __shared__ int s_cnt[kCensusWaves][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int band = 0, bad = 0;
    for (int i = threadIdx.x; i < blocks; i += kCensusBlock) {
        band += partial[2 * i];
        bad += partial[2 * i + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        band += __shfl_xor(band, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
        s_cnt[wave][0] = band;
        s_cnt[wave][1] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int c = 0;
        for (int w = 0; w < kCensusWaves; ++w) c += s_cnt[w][threadIdx.x];
        counts[threadIdx.x] = c;
    }
}

}  // namespace

int contact_band_census(const float* p, int64_t ld, int B, int nv, const float* thr, int J, float margin, int32_t* counts,
                        float* mindist, hipStream_t st) {
    if (!p || !thr || !counts || !mindist || B <= 0 || nv <= 0 || ld < nv || J < 1 || J > kMaxThr || !(margin >= 0.0f))
        return IVLM_ERR_INVALID_ARG;
    // 16-byte loads need every row to start on a 16-byte boundary: an aligned base and (for B > 1) a stride that keeps it
    const int vec4 = (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (B == 1 || (ld & 3) == 0);
    switch (J) {
        case 1: contact_band_census_kernel<1><<<B, kCensusBlock, 0, st>>>(p, ld, nv, thr, margin, vec4, counts, mindist); break;
        case 2: contact_band_census_kernel<2><<<B, kCensusBlock, 0, st>>>(p, ld, nv, thr, margin, vec4, counts, mindist); break;
        case 3: contact_band_census_kernel<3><<<B, kCensusBlock, 0, st>>>(p, ld, nv, thr, margin, vec4, counts, mindist); break;
        default: contact_band_census_kernel<4><<<B, kCensusBlock, 0, st>>>(p, ld, nv, thr, margin, vec4, counts, mindist); break;
    }
    return ivlm_launch_status();
}

size_t mask_band_census_workspace_bytes() { return sizeof(int32_t) * 2 * kMaskBlocks; }

int mask_band_census(const float* logits, int V, int64_t HW, const int32_t* ent_pix, const int32_t* row_ptr, int n_rows,
                     float thr_p, float margin_p, int32_t* counts, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!logits || !ent_pix || !row_ptr || !counts || !ws || V <= 0 || HW <= 0 || HW >= (1ll << 30) || n_rows <= 0 ||
        n_rows % V != 0 || !(margin_p >= 0.0f))
        return IVLM_ERR_INVALID_ARG;
    if (ws_bytes < mask_band_census_workspace_bytes()) return IVLM_ERR_WORKSPACE;
    // a whole number of waves' rows per block, at most kMaskBlocks blocks
    int rpb = (n_rows + kMaskBlocks - 1) / kMaskBlocks;
    rpb = (rpb + kCensusWaves - 1) / kCensusWaves * kCensusWaves;
    const int blocks = (n_rows + rpb - 1) / rpb;
    int32_t* partial = static_cast<int32_t*>(ws);
    mask_band_partial_kernel<<<blocks, kCensusBlock, 0, st>>>(logits, HW, ent_pix, row_ptr, n_rows, n_rows / V, rpb, thr_p, margin_p,
                                                             partial);
    mask_band_finish_kernel<<<1, kCensusBlock, 0, st>>>(partial, blocks, counts);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
int ivlm_contact_band_census(const float* p, int64_t ld, int B, int Nv, const float* thr, int J, float margin, int32_t* counts,
                             float* mindist, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::contact_band_census(p, ld, B, Nv, thr, J, margin, counts, mindist, ivlm_stream(s));
}
size_t ivlm_mask_band_census_workspace_bytes(void) { return ivlm::mask_band_census_workspace_bytes(); }
int ivlm_mask_band_census(const float* logits, int V, int64_t HW, const int32_t* ent_pix, const int32_t* row_ptr, int n_rows,
                          float thr_p, float margin_p, int32_t* counts, void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::mask_band_census(logits, V, HW, ent_pix, row_ptr, n_rows, thr_p, margin_p, counts, workspace, workspace_bytes,
                                  ivlm_stream(s));
}
}
