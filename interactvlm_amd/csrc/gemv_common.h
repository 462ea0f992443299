// What the weight-streaming linears (gemv.hip, gemv_p12.hip, gemv_mfma.hip) share: the activation switch, the output store, the block
// prologue that stages one fp32 activation row in LDS, the one-row-per-wave finish and the tile finish of the skinny MFMA kernels, and on
// the host side the argument filler of one fp32 row and the tiles-per-block rule.
// Every function is inlined into its kernel: the arithmetic, its order and the barriers are those of the kernel that calls it.
// (Not here: the fp32 fragment -> hi / lo operand block in the K loops of the two skinny kernels.  As one function the same text
//  compiled to another loop schedule in skinny_p12m_kernel<true, T> - 12 more register moves per trip - and the batched decode step
//  (tools/bench_decode.py, 7B, three alternating runs, twice) moved BOTH ways: batch 8 slower, 3.51 - 3.54 against 3.47 - 3.50 ms per
//  token, outside the inline form's run-to-run range both times; batch 16 equal or faster, 4.36 - 4.46 against 4.40 - 4.48.  Neither is a
//  change this header is for: the block stays in the two loops, where it compiles as before.)
#pragma once
#include "gemm_common.h"

namespace ivlm {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;  // native vector: nontemporal-loadable
typedef __attribute__((ext_vector_type(4))) float f32x4v_t;

constexpr int kRowWaves = 16;  // waves (= weight rows) per block of the one-row-per-wave kernels

// The 12-bit weight kernels stage x as x * 2^64: an exact power-of-two scaling, chosen in the MIDDLE of fp32's exponent range (ADVICE
// r4: 2^100 turned any |x| >= 2^28 ~ 2.7e8 into inf and the row into NaN, a range gemv1_kernel's plain fp32 x does not have).  A
// rebuilt weight is 1.m x 2^(code - 127) with code 1 .. 15, i.e. 2^-126 .. 2^-111, so the products x * 2^64 * w are normal fp32 numbers
// for 2^-64 <~ |x| < 2^64 (5e-20 .. 1.8e19) and every result inside that range is independent of the scale (the hi / lo / lo2 split and
// the fp32 accumulation are scale-invariant): bit-identical to the 2^100 staging on every activation the model produces.
constexpr int kXScaleExp = 64;

// (GELU in its erff form: gemm_act of the tile GEMMs uses a polynomial erf and gives other bits)
__device__ __forceinline__ float gemv_act(float x, int act) {
    switch (act) {
        case ACT_GELU: return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
        case ACT_QUICK_GELU: return x / (1.0f + __expf(-1.702f * x));
        case ACT_RELU: return x < 0.0f ? 0.0f : x;  // (torch.relu semantics: a NaN stays a NaN; fmaxf would turn it into 0)
        case ACT_SILU: return x / (1.0f + __expf(-x));
        case ACT_SIGMOID: return 1.0f / (1.0f + __expf(-x));
        default: return x;
    }
}

__device__ __forceinline__ void gemv_store(const GemmArgs& g, int64_t idx, float v) {
    if (g.out_f32) static_cast<float*>(g.C)[idx] = v;
    else static_cast<bf16_t*>(g.C)[idx] = f32_to_bf16(v);
}

// one 8-element chunk of an fp32 row (two 16-byte halves) under the fused RMSNorm: sum of squares of the raw values, then times gamma
__device__ __forceinline__ void sum_squares8(float& ssq, const f32x4v_t& xa, const f32x4v_t& xb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ssq += xa[j] * xa[j] + xb[j] * xb[j];
}
__device__ __forceinline__ void scale_by_gamma8(f32x4v_t& xa, f32x4v_t& xb, const u32x4_t& gv) {
    xa[0] *= __uint_as_float(gv[0] << 16); xa[1] *= __uint_as_float(gv[0] & 0xffff0000u);
    xa[2] *= __uint_as_float(gv[1] << 16); xa[3] *= __uint_as_float(gv[1] & 0xffff0000u);
    xb[0] *= __uint_as_float(gv[2] << 16); xb[1] *= __uint_as_float(gv[2] & 0xffff0000u);
    xb[2] *= __uint_as_float(gv[3] << 16); xb[3] *= __uint_as_float(gv[3] & 0xffff0000u);
}

// Block prologue of the one-row-per-wave kernels: the fp32 row g.A (times gamma under RMS; times 2^kXScaleExp when SCALED) into LDS
// as two planes xf[2][nchunk] of 16 bytes - consecutive lanes read consecutive 16 bytes - and, under RMS, every wave's part of sum(x^2)
// into s_red[wave].  The caller's barrier publishes both.
template <bool RMS, bool SCALED>
__device__ __forceinline__ void stage_row_f32(const GemmArgs& g, f32x4v_t* xf, int nchunk, int nthreads, float* s_red, int lane, int wave) {
    float ssq = 0.0f;
    for (int c = threadIdx.x; c < nchunk; c += nthreads) {
        const f32x4v_t* xp = reinterpret_cast<const f32x4v_t*>(g.A) + 2 * c;
        f32x4v_t xa = xp[0], xb = xp[1];
        if (RMS) {
            const u32x4_t gv = *(reinterpret_cast<const u32x4_t*>(g.rms_w) + c);
            sum_squares8(ssq, xa, xb);
            scale_by_gamma8(xa, xb, gv);
        }
        if (SCALED) {
            const float xs = __builtin_ldexpf(1.0f, kXScaleExp);
            xa = xa * xs;
            xb = xb * xs;
        }
        xf[c] = xa;
        xf[nchunk + c] = xb;
    }
    if (RMS) {
        ssq = wave_sum(ssq);
        if (lane == 0) s_red[wave] = ssq;
    }
}

// Finish of the one-row-per-wave kernels: acc = the wave's reduced dot product of weight row `row` (every lane holds it).  Row scale
// from the kRowWaves partials in s_red, bias, then either the SwiGLU pair - rows (gate_j, up_j) interleaved, the even wave finishes the
// pair through s_val behind a block barrier that EVERY wave of the block must reach, dead ones (live == false) included - or
// activation, residual and the store by lane 0.  PAIRS = false: a kernel whose waves do not all arrive here (never launched with SwiGLU).
template <bool RMS, bool PAIRS = true>
__device__ __forceinline__ void finish_row(const GemmArgs& g, float acc, int row, bool live, int lane, int wave, const float* s_red,
                                           float* s_val) {
    if (RMS) {
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < kRowWaves; ++i) q += s_red[i];
        acc *= rsqrtf(q / (float)g.K + g.rms_eps);
    }
    float v = acc + ((g.bias && live) ? bf16_to_f32(g.bias[row]) : 0.0f);
    if (PAIRS && g.act == ACT_SWIGLU) {
        if (lane == 0) s_val[wave] = v;
        __syncthreads();
        if (lane != 0 || (wave & 1) || !live) return;
        gemv_store(g, row >> 1, (v / (1.0f + __expf(-v))) * s_val[wave + 1]);
        return;
    }
    if (lane != 0 || !live) return;
    v = gemv_act(v, g.act);
    if (g.residual) v += gemm_residual_at(g, g.residual, row);
    gemv_store(g, row, v);
}

// Finish of one 16 x 16 tile of the skinny MFMA kernels (blocks of kW waves; EVERY thread of the block calls it: three block barriers).
// acc = this wave's K slice of the tile at weight rows nt .. nt + 15, lane (r = lane & 15, kg = lane >> 4) holding C[m = r][n = 4 kg + i].
// The kW partials are summed through s_part in wave order; fix(v, m, nn) corrects the sum of activation row m and weight row nn before
// the row scale (s_ssq) and the bias; SwiGLU pairs, activation and residual go through s_fin.  `first` = false: the block's previous
// tile may still be read from s_fin.  Tiles behind N are skipped and a row behind N reads the bias of row N - 1 (never stored).
template <bool RMS, int kW, typename Fix>
__device__ __forceinline__ void skinny_finish_tile(const GemmArgs& g, const f32x4v_t& acc, int nt, bool first, float (*s_part)[16][17],
                                                   const float (*s_ssq)[16], float (*s_fin)[17], Fix fix) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const int m = threadIdx.x >> 4, n = threadIdx.x & 15;
    if (!first) __syncthreads();  // the previous tile's s_fin readers are done
#pragma unroll
    for (int i = 0; i < 4; ++i) s_part[wave][r][kg * 4 + i] = acc[i];
    __syncthreads();
    if (threadIdx.x < 256 && nt < g.N) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < kW; ++w) v += s_part[w][m][n];
        const int nn = min(nt + n, g.N - 1);
        v = fix(v, m, nn);
        if (RMS) {
            float q = 0.0f;
#pragma unroll
            for (int w = 0; w < kW; ++w) q += s_ssq[w][m];
            v *= rsqrtf(q / (float)g.K + g.rms_eps);
        }
        s_fin[m][n] = v + (g.bias ? bf16_to_f32(g.bias[nn]) : 0.0f);
    }
    __syncthreads();
    if (threadIdx.x >= 256 || m >= g.M || nt + n >= g.N) return;
    float v = s_fin[m][n];
    int64_t col = nt + n;
    if (g.act == ACT_SWIGLU) {  // rows (gate_j, up_j) interleaved: even n pairs with n + 1
        if (n & 1) return;
        const float up = s_fin[m][n + 1];
        v = (v / (1.0f + __expf(-v))) * up;
        col >>= 1;
    } else {
        v = gemv_act(v, g.act);
        if (g.residual) {
            const int64_t rrow = g.res_mod > 0 ? (m % g.res_mod) : m;
            v += gemm_residual_at(g, g.residual, rrow * g.ldr + col);
        }
    }
    gemv_store(g, (int64_t)m * g.ldc + col, v);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// the arguments of one fp32 activation row x[K] against N weight rows (the weight operand is the caller's)
static inline GemmArgs gemv_row_args(const float* x, void* C, const void* bias, const void* residual, int N, int K, int act, int out_f32,
                                     const void* rms_w, float rms_eps, int flags) {
    GemmArgs g;
    g.A = reinterpret_cast<const bf16_t*>(x);
    g.a_f32 = 1;
    g.C = C;
    g.bias = static_cast<const bf16_t*>(bias);
    g.residual = static_cast<const bf16_t*>(residual);
    g.res_f32 = (flags & IVLM_GEMM_RES_F32) ? 1 : 0;
    g.M = 1; g.N = N; g.K = K;
    g.lda = K;
    g.act = act;
    g.out_f32 = out_f32;
    g.rms_w = static_cast<const bf16_t*>(rms_w);
    g.rms_eps = rms_eps;
    return g;
}

// 16-row tiles per block of the skinny MFMA kernels (override > 0: that many): fewest (blocks per CU) x (tiles per block), then the most
// tiles (least activation re-reading)
static inline int skinny_tiles(int N, int override) {
    if (override > 0) return override;
    const int tiles = (N + 15) / 16, cus = 256;
    int best = 1, best_cost = 1 << 30;
    for (int t : {1, 2, 3}) {  // (4 and 6 tiles per block measured slower: gate|up 230 blocks of 6 tiles 4.56 ms per step, 459 of 3: 4.44)
        const int blocks = (tiles + t - 1) / t;
        const int cost = ((blocks + cus - 1) / cus) * t;
        if (cost <= best_cost) { best = t; best_cost = cost; }
    }
    return best;
}

}  // namespace ivlm
