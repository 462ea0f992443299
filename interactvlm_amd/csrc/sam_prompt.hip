// The point / box / mask prompts of SAM's prompt encoder (gfx950, wave64; built with -ffp-contract=off: every fp32 operation is
// the one written here).
//   prompt_embed     PromptEncoder._embed_points / _embed_boxes (prompt_encoder.py:78-109) for R rows at once
//   mask_downscale   PromptEncoder._embed_masks (prompt_encoder.py:56-64, 111-114): conv k2s2 -> LayerNorm2d -> GELU -> conv k2s2 ->
//                    LayerNorm2d -> GELU -> conv 1x1 as ONE kernel, channels-last output
#include "kernels.h"

namespace ivlm {
namespace {

constexpr int kT = 256;
constexpr int kTable = 5;  // rows of the label table: negative point, positive point, box corner 0, box corner 1, not-a-point

// out[r, f] = sin(a), out[r, F + f] = cos(a), a = 2 pi (cx g[0, f] + cy g[1, f]), (cx, cy) = 2 (coord + 0.5) / (W, H) - 1: the
// reference's operations one by one (shift, divide, 2c - 1, the two-term product, the 2 pi scale: all fp32), then + table[label].
// label -1: the not-a-point row alone (the reference zeroes the encoding, then adds); a label outside -1..3: NaN, no table access.
__global__ __launch_bounds__(kT) void prompt_embed_kernel(const float* __restrict__ coords, const int32_t* __restrict__ labels,
                                                          const float* __restrict__ gauss, const float* __restrict__ table,
                                                          float* __restrict__ out, int64_t R, int F, float H, float W) {
    const int64_t total = R * F;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int f = (int)(i % F);
        const int64_t r = i / F;
        const int label = labels[r];
        float* o = out + r * 2 * F;
        if (label == -1) {
            o[f] = table[(kTable - 1) * 2 * F + f];
            o[F + f] = table[(kTable - 1) * 2 * F + F + f];
            continue;
        }
        if (label < 0 || label > 3) {
            o[f] = o[F + f] = __uint_as_float(0x7fc00000u);
            continue;
        }
        float cx = (coords[2 * r] + 0.5f) / W, cy = (coords[2 * r + 1] + 0.5f) / H;
        cx = 2.0f * cx - 1.0f;
        cy = 2.0f * cy - 1.0f;
        float a = cx * gauss[f] + cy * gauss[F + f];
        a = 6.283185307179586f * a;
        const float* t = table + (int64_t)label * 2 * F;
        o[f] = sinf(a) + t[f];
        o[F + f] = cosf(a) + t[F + f];
    }
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f)); }

// LayerNorm2d over N channels of one pixel (common.py: u = mean, s = mean (x - u)^2, (x - u) / sqrt(s + eps) * w + b), then GELU
template <int N>
__device__ __forceinline__ void ln_gelu(float* x, const float* w, const float* b, float eps) {
    float u = 0.0f;
#pragma unroll
    for (int c = 0; c < N; ++c) u += x[c];
    u = u / (float)N;
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < N; ++c) s += (x[c] - u) * (x[c] - u);
    const float d = sqrtf(s / (float)N + eps);
#pragma unroll
    for (int c = 0; c < N; ++c) x[c] = gelu_erf(w[c] * ((x[c] - u) / d) + b[c]);
}

// offsets of the small tensors in the block's LDS copy (floats); the 1x1 conv follows them transposed, [16][C], then its bias
constexpr int kW0 = 0, kB0 = 16, kG1 = 20, kE1 = 24, kW3 = 28, kB3 = kW3 + 256, kG2 = kB3 + 16, kE2 = kG2 + 16, kSmall = kE2 + 16;
constexpr int kMid = 16, kHLd = kMid + 1;  // mask_in_chans, and the row stride of the per-cell hidden vectors in LDS
constexpr int kCMax = 256;

struct MaskDownW {
    const float *w0, *b0, *g1, *e1, *w3, *b3, *g2, *e2, *w6, *b6;
};

// One block = kT consecutive output cells (b, y, x).  Phase 1: thread t runs cell t's 4x4 patch through the two strided convolutions
// (its 16 hidden channels stay in registers, the weights are LDS broadcasts) and leaves the 16 channels in LDS.  Phase 2: the block's
// kT * C outputs are one contiguous span of `dense`; consecutive lanes take consecutive float4s of it (C = 256: one wave instruction
// writes one whole cell, 1 KB), each 4 output channels a 16-term product with the transposed 1x1 weight (consecutive lanes read
// consecutive float4s of one LDS row; the cell's hidden vector is a broadcast).
__global__ __launch_bounds__(kT) void mask_downscale_kernel(const float* __restrict__ mask, MaskDownW w, float* __restrict__ dense,
                                                            int64_t cells, int gh, int gw, int C, float eps) {
    __shared__ __attribute__((aligned(16))) float sm[kSmall];
    __shared__ __attribute__((aligned(16))) float w6t[kMid * kCMax];
    __shared__ __attribute__((aligned(16))) float b6[kCMax];
    __shared__ float hid[kT * kHLd];
    const int t = threadIdx.x;
    if (t < 16) sm[kW0 + t] = w.w0[t];
    if (t < 4) sm[kB0 + t] = w.b0[t], sm[kG1 + t] = w.g1[t], sm[kE1 + t] = w.e1[t];
    sm[kW3 + t] = w.w3[t];  // (kT == 256 == 16 * 4 * 2 * 2)
    if (t < 16) sm[kB3 + t] = w.b3[t], sm[kG2 + t] = w.g2[t], sm[kE2 + t] = w.e2[t];
    for (int j = t; j < kMid * C; j += kT) w6t[(j % kMid) * C + j / kMid] = w.w6[j];  // [C][16] -> [16][C]
    for (int j = t; j < C; j += kT) b6[j] = w.b6[j];
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * kT;
    const int n = (int)(cells - base < kT ? cells - base : kT);
    if (t < n) {
        const int64_t cell = base + t;
        const int x = (int)(cell % gw), y = (int)((cell / gw) % gh);
        const int64_t b = cell / ((int64_t)gw * gh);
        const float* mp = mask + ((b * 4 * gh + 4 * y) * 4 * gw + 4 * x);
        float m[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(mp + (int64_t)r * 4 * gw);
            m[r][0] = v.x, m[r][1] = v.y, m[r][2] = v.z, m[r][3] = v.w;
        }
        float h2[kMid];
#pragma unroll
        for (int o = 0; o < kMid; ++o) h2[o] = 0.0f;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                float h1[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float a = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) a += sm[kW0 + c * 4 + k] * m[2 * py + (k >> 1)][2 * px + (k & 1)];
                    h1[c] = a + sm[kB0 + c];
                }
                ln_gelu<4>(h1, sm + kG1, sm + kE1, eps);
#pragma unroll
                for (int o = 0; o < kMid; ++o) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) h2[o] += sm[kW3 + ((o * 4 + c) * 2 + py) * 2 + px] * h1[c];
                }
            }
        }
#pragma unroll
        for (int o = 0; o < kMid; ++o) h2[o] += sm[kB3 + o];
        ln_gelu<kMid>(h2, sm + kG2, sm + kE2, eps);
#pragma unroll
        for (int o = 0; o < kMid; ++o) hid[t * kHLd + o] = h2[o];
    }
    __syncthreads();

    const int c4n = C >> 2;
    float4* out = reinterpret_cast<float4*>(dense + base * C);
    for (int j = t; j < n * c4n; j += kT) {
        const int cell = j / c4n, c4 = j - cell * c4n;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < kMid; ++k) {
            const float h = hid[cell * kHLd + k];
            const float4 wv = *reinterpret_cast<const float4*>(w6t + k * C + 4 * c4);
            acc.x += wv.x * h, acc.y += wv.y * h, acc.z += wv.z * h, acc.w += wv.w * h;
        }
        const float4 bv = *reinterpret_cast<const float4*>(b6 + 4 * c4);
        out[j] = make_float4(acc.x + bv.x, acc.y + bv.y, acc.z + bv.z, acc.w + bv.w);
    }
}

}  // namespace

int prompt_embed(const float* coords, const int32_t* labels, const float* gauss, const float* table, float* out, int64_t R, int F,
                 int H, int W, hipStream_t st) {
    if (!coords || !labels || !gauss || !table || !out || R <= 0 || H <= 0 || W <= 0) return IVLM_ERR_INVALID_ARG;
    if (F < 32 || F > 128 || (F & 31)) return IVLM_ERR_UNSUPPORTED;
    if (R > (1LL << 24)) return IVLM_ERR_UNSUPPORTED;
    const int64_t blocks = (R * F + kT - 1) / kT;
    prompt_embed_kernel<<<(int)(blocks < 4096 ? blocks : 4096), kT, 0, st>>>(coords, labels, gauss, table, out, R, F, (float)H, (float)W);
    return ivlm_launch_status();
}

int mask_downscale(const float* mask, const float* const* weights, float* dense, int B, int gh, int gw, int C, int mid, float eps,
                   hipStream_t st) {
    if (!mask || !weights || !dense || B <= 0 || gh <= 0 || gw <= 0 || C <= 0) return IVLM_ERR_INVALID_ARG;
    for (int i = 0; i < 10; ++i)
        if (!weights[i]) return IVLM_ERR_INVALID_ARG;
    if (mid != kMid || C > kCMax || (C & 63)) return IVLM_ERR_UNSUPPORTED;
    const int64_t cells = (int64_t)B * gh * gw;
    if (cells > (1LL << 30) || gh > (1 << 20) || gw > (1 << 20)) return IVLM_ERR_UNSUPPORTED;
    if (((uintptr_t)mask & 15) || ((uintptr_t)dense & 15)) return IVLM_ERR_INVALID_ARG;  // float4 reads of the patch rows / stores
    const MaskDownW w = {weights[0], weights[1], weights[2], weights[3], weights[4], weights[5], weights[6], weights[7], weights[8], weights[9]};
    mask_downscale_kernel<<<(int)((cells + kT - 1) / kT), kT, 0, st>>>(mask, w, dense, cells, gh, gw, C, eps);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
int ivlm_prompt_embed(const float* coords, const int32_t* labels, const float* gauss, const float* table, float* out, int64_t R,
                      int F, int H, int W, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::prompt_embed(coords, labels, gauss, table, out, R, F, H, W, ivlm_stream(s));
}
int ivlm_mask_downscale(const float* mask, const float* w0, const float* b0, const float* ln1_w, const float* ln1_b, const float* w3,
                        const float* b3, const float* ln2_w, const float* ln2_b, const float* w6, const float* b6, float* dense, int B,
                        int gh, int gw, int C, int mask_in_chans, float eps, ivlm_stream_t s) {
    ivlm_enter();
    const float* const weights[10] = {w0, b0, ln1_w, ln1_b, w3, b3, ln2_w, ln2_b, w6, b6};
    return ivlm::mask_downscale(mask, weights, dense, B, gh, gw, C, mask_in_chans, eps, ivlm_stream(s));
}
}  // extern "C"
