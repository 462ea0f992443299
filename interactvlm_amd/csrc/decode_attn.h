// Single-query LLaMA attention: the one home of its arithmetic.  Every decode mode but the many-query ones (speculative verify, the
// shared phase of the prefix kernel) is "one query of head h against a range of cached keys": decode_attn_range below, called by
// the one-block and batched kernel, the split-KV / parts kernel (decode.hip), the own phase of the shared-prefix kernel
// (decode_prefix.hip) and the producer blocks of the fused attention + o_proj launch (decode_fused.hip); merge_ranges combines the
// (o, max, sum) partials of several ranges.  verify.hip and the prefix kernel's shared phase take only rope_cos_sin.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace ivlm {
namespace decattn {

constexpr int kMaxD = 128;
constexpr int kMaxT = 4096;  // scores live in LDS (16 KB)
constexpr int kMaxSplits = 16;  // key ranges per head that merge_ranges takes

constexpr int kDecThreads = 1024;  // the one-block kernels: 64 groups of 16 lanes, 64 key rows per sweep

// cos / sin of RoPE pair d (of half = D / 2) at position pos: from the table when there is one
struct CosSin { float c, s; };
__device__ __forceinline__ CosSin rope_cos_sin(const float* __restrict__ ct, const float* __restrict__ stab, int pos, int d, int half,
                                               int D, float theta) {
    if (ct) return {ct[pos * half + d], stab[pos * half + d]};
    const float ang = (float)pos * powf(theta, -(float)(2 * d) / (float)D);
    return {cosf(ang), sinf(ang)};
}

// What a block knows about its key range when decode_attn_range returns: o = element t of sum_j p_j v_j (threads t < D; 0 elsewhere),
// m = the largest score of the range (-1e30 when it is empty), l = sum_j e^(s_j - m) (0 when empty).
struct RangeOut { float o, m, l; };

// One query (head h of the qkv row [3, H, D]) against the keys [k0, k1) of one cache slab [Tmax, H, D]; pos = the position of the new
// token, whose K / V row is not in the cache yet: a range that holds pos takes that row from qkv, and the block with `append`
// (at most one per head) writes it to row pos of the slab.  An empty range (k1 <= k0) is allowed.  THREADS / 16 groups of 16
// lanes share a key row each (16-byte loads, 256 B coalesced per row); group g owns keys k0 + g, k0 + g + THREADS / 16, ...
// F32IO: qkv is fp32 (the decode path keeps fp32 activations between its weight-streaming kernels: q and the softmax weights are
// then NOT rounded to bf16 - only the K / V rows appended to the 16-bit cache are); otherwise bf16, with the roundings of the MFMA
// prefill path (q, k after RoPE and P rounded to bf16).
// LO ("parity" precision, with F32IO): the cache holds K / V as hi + lo bf16 planes (kcache_lo / vcache_lo, same layout): the
// appended rows are not rounded to bf16 and the cached ones are read back as hi + lo.
// CF16 (with F32IO): the cache holds IEEE halves (the fp16-operand prefill appends them): appended rows are rounded to fp16, the
// cached ones are read as fp16.
// NORM: the one-block arithmetic - the weights are divided by l before P.V (and rounded to bf16 when !F32IO: HF does softmax in
// fp32, casts to the model dtype, then @ V), so o is the attention output itself; without it o is unnormalised, for merge_ranges.
// Summation orders are part of the contract (callers are compared bit for bit): the xor ladder 8, 4, 2, 1 per key, tiles in order,
// groups in index order.  Loads of cached rows are clamped to rows [0, max(pos - 1, 0)] of the slab and masked where used.
template <int THREADS, bool F32IO, bool LO, bool CF16, bool NORM>
__device__ __forceinline__ RangeOut decode_attn_range(const int h, const void* __restrict__ qkv_v, bf16_t* __restrict__ kcache,
                                                      bf16_t* __restrict__ vcache, bf16_t* __restrict__ kcache_lo,
                                                      bf16_t* __restrict__ vcache_lo, int H, int D, const int pos, const int k0,
                                                      const int k1, const bool append, float theta, float scale,
                                                      const float* __restrict__ ct, const float* __restrict__ stab) {
    static_assert(!CF16 || (F32IO && !LO), "fp16 cache: fp32 qkv / o, no lo planes");
    static_assert(!LO || F32IO, "lo planes: fp32 qkv / o");
    constexpr int kG = THREADS / 16, kU = 6, kTile = kG * kU;  // 6 rows per group and tile: 384 keys per tile at 1024 threads, 96 at 256
    constexpr int NW = THREADS / 64;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    __shared__ float q_s[kMaxD];
    __shared__ float knew_s[kMaxD];
    __shared__ float vnew_s[kMaxD];
    __shared__ float sc[kMaxT];
    __shared__ float red[2 * NW];
    __shared__ float part[kG][kMaxD];
    const int t = threadIdx.x;
    const int len = k1 > k0 ? k1 - k0 : 0;
    const int half = D >> 1;
    const int sub = t & 15, grp = t >> 4;
    const int nch = D >> 3;  // 16-byte chunks per row (<= 16)
    const int csub = sub < nch ? sub : nch - 1;
    const int64_t rstride = (int64_t)H * D;
    const bf16_t* kb = kcache + (int64_t)h * D + csub * 8;
    const bf16_t* vb = vcache + (int64_t)h * D + csub * 8;
    const bf16_t* kbl = LO ? kcache_lo + (int64_t)h * D + csub * 8 : nullptr;
    const bf16_t* vbl = LO ? vcache_lo + (int64_t)h * D + csub * 8 : nullptr;
    // K and V rows of the first tile go in flight before anything else (they do not depend on q): the kernel is a chain of
    // dependent memory round trips otherwise (one per sweep of kG keys)
    u32x4_t kr[kU], vr[kU];
    const int jmax = pos > 0 ? pos - 1 : 0;  // loads are clamped and unconditional, masked where used (pos == 0: row 0 is unused)
    if (len > 0) {
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            int j = k0 + grp + kG * i;
            j = j < jmax ? j : jmax;
            kr[i] = *reinterpret_cast<const u32x4_t*>(kb + j * rstride);
            vr[i] = *reinterpret_cast<const u32x4_t*>(vb + j * rstride);
        }
    }
    const bf16_t* qkv = static_cast<const bf16_t*>(qkv_v);
    const float* qkvf = static_cast<const float*>(qkv_v);
    auto ld = [&](int64_t e) -> float { return F32IO ? qkvf[e] : bf16_to_f32(qkv[e]); };
    // ---- RoPE on q (every block) and on the new k (the block that appends); append k, v --------------------------------------------
    if (t < half) {
        const int64_t q = (int64_t)h * D, k = (int64_t)H * D + h * D;
        const CosSin r = rope_cos_sin(ct, stab, pos, t, half, D, theta);
        const float c = r.c, s = r.s;
        const float q0 = ld(q + t), q1 = ld(q + t + half);
        const float qaf = q0 * c - q1 * s, qbf = q1 * c + q0 * s;
        // bf16 I/O: round q, k to bf16 exactly like the prefill path (rope_kv_kernel) so both paths see the same values
        q_s[t] = F32IO ? qaf : bf16_to_f32(f32_to_bf16(qaf));
        q_s[t + half] = F32IO ? qbf : bf16_to_f32(f32_to_bf16(qbf));
        if (append) {
            const float k0f = ld(k + t), k1f = ld(k + t + half);
            const float kaf = k0f * c - k1f * s, kbf = k1f * c + k0f * s;
            const bf16_t ka = f32_to_h16<CF16>(kaf), kb16 = f32_to_h16<CF16>(kbf);
            knew_s[t] = F32IO ? kaf : bf16_to_f32(ka);
            knew_s[t + half] = F32IO ? kbf : bf16_to_f32(kb16);
            bf16_t* kc = kcache + ((int64_t)pos * H + h) * D;
            kc[t] = ka;
            kc[t + half] = kb16;
            if (LO) {
                bf16_t* kcl = kcache_lo + ((int64_t)pos * H + h) * D;
                kcl[t] = f32_to_bf16(kaf - bf16_to_f32(ka));
                kcl[t + half] = f32_to_bf16(kbf - bf16_to_f32(kb16));
            }
        }
    } else if (append && t >= 128 && t < 128 + D) {
        const int d = t - 128;
        const float v = ld(2 * (int64_t)H * D + h * D + d);
        vnew_s[d] = v;
        const bf16_t vh = f32_to_h16<CF16>(v);
        vcache[((int64_t)pos * H + h) * D + d] = vh;
        if (LO) vcache_lo[((int64_t)pos * H + h) * D + d] = f32_to_bf16(v - bf16_to_f32(vh));
    }
    __syncthreads();
    // ---- scores of the range -----------------------------------------------------------------------------------------------------
    float qr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qr[e] = sub < nch ? q_s[sub * 8 + e] : 0.0f;
    auto score = [&](const u32x4_t& kv, int j) {
        float d = 0.0f;
        if (sub < nch) {
            if (j < pos) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d += pair_lo_f32<CF16>(kv[e]) * qr[2 * e];
                    d += pair_hi_f32<CF16>(kv[e]) * qr[2 * e + 1];
                }
                if (LO) {
                    const u32x4_t kl = *reinterpret_cast<const u32x4_t*>(kbl + j * rstride);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        d += __uint_as_float(kl[e] << 16) * qr[2 * e];
                        d += __uint_as_float(kl[e] & 0xffff0000u) * qr[2 * e + 1];
                    }
                }
            } else if (j == pos) {
#pragma unroll
                for (int e = 0; e < 8; ++e) d += knew_s[sub * 8 + e] * qr[e];
            }
        }
        d += __shfl_xor(d, 8, 64);
        d += __shfl_xor(d, 4, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 1, 64);
        if (sub == 0 && j < k1) sc[j - k0] = d * scale;
    };
    if (len > 0) {
#pragma unroll
        for (int i = 0; i < kU; ++i) score(kr[i], k0 + grp + kG * i);
        for (int j0 = k0 + kTile; j0 < k1; j0 += kTile) {  // longer ranges: further tiles
#pragma unroll
            for (int i = 0; i < kU; ++i) {
                int j = j0 + grp + kG * i;
                j = j < jmax ? j : jmax;
                kr[i] = *reinterpret_cast<const u32x4_t*>(kb + j * rstride);
            }
#pragma unroll
            for (int i = 0; i < kU; ++i) score(kr[i], j0 + grp + kG * i);
        }
    }
    __syncthreads();
    // ---- softmax of the range (fp32): max m, p = e^(s - m), sum l --------------------------------------------------------------------
    float mx = -1.0e30f;
    for (int j = t; j < len; j += THREADS) mx = fmaxf(mx, sc[j]);
    mx = wave_max(mx);
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red[w]);
    float sum = 0.0f;
    for (int j = t; j < len; j += THREADS) {
        const float p = __expf(sc[j] - mx);
        sc[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    if ((t & 63) == 0) red[NW + (t >> 6)] = sum;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += red[NW + w];
    const float inv_sum = NORM ? 1.0f / tot : 1.0f;
    // ---- o = sum p v over the range: lane sub owns 8 dims (V rows of the first tile already loaded) ----------------------------------
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    auto pv = [&](const u32x4_t& vv, int j) {
        if (j < k1 && sub < nch) {
            float p = sc[j - k0];
            if (NORM) p = F32IO ? p * inv_sum : bf16_to_f32(f32_to_bf16(p * inv_sum));
            if (j < pos) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[2 * e] += p * pair_lo_f32<CF16>(vv[e]);
                    acc[2 * e + 1] += p * pair_hi_f32<CF16>(vv[e]);
                }
                if (LO) {
                    const u32x4_t vl = *reinterpret_cast<const u32x4_t*>(vbl + j * rstride);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[2 * e] += p * __uint_as_float(vl[e] << 16);
                        acc[2 * e + 1] += p * __uint_as_float(vl[e] & 0xffff0000u);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += p * vnew_s[sub * 8 + e];
            }
        }
    };
    if (len > 0) {
#pragma unroll
        for (int i = 0; i < kU; ++i) pv(vr[i], k0 + grp + kG * i);
        for (int j0 = k0 + kTile; j0 < k1; j0 += kTile) {
#pragma unroll
            for (int i = 0; i < kU; ++i) {
                int j = j0 + grp + kG * i;
                j = j < jmax ? j : jmax;
                vr[i] = *reinterpret_cast<const u32x4_t*>(vb + j * rstride);
            }
#pragma unroll
            for (int i = 0; i < kU; ++i) pv(vr[i], j0 + grp + kG * i);
        }
    }
    if (sub < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) part[grp][sub * 8 + e] = acc[e];
    }
    __syncthreads();
    float r = 0.0f;
    if (t < D) {
#pragma unroll
        for (int g2 = 0; g2 < kG; ++g2) r += part[g2][t];
    }
    return {r, mx, tot};
}

// Merge of S <= kMaxSplits range partials (pm = max, pl = sum, po = this thread's element of the unnormalised o; entries >= S are
// ignored) and, with have_own, of one more range that the calling block has just computed itself, by the online-softmax rule:
// o = sum_s e^(m_s - M) o_s / sum_s e^(m_s - M) l_s, ranges in index order, the own range last.  A range that published l = 0 is
// empty and takes no part (not in M either); nothing at all: 0.  How the partials were loaded is the caller's business.
__device__ __forceinline__ float merge_ranges(const float (&pm)[kMaxSplits], const float (&pl)[kMaxSplits], const float (&po)[kMaxSplits],
                                              int S, bool have_own, const RangeOut& own) {
    float M = have_own ? own.m : -1.0e30f;
#pragma unroll
    for (int s2 = 0; s2 < kMaxSplits; ++s2)
        if (s2 < S && pl[s2] > 0.0f) M = fmaxf(M, pm[s2]);
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int s2 = 0; s2 < kMaxSplits; ++s2) {
        if (s2 < S && pl[s2] > 0.0f) {
            const float w = __expf(pm[s2] - M);
            num += w * po[s2];
            den += w * pl[s2];
        }
    }
    if (have_own) {
        const float w = __expf(own.m - M);
        num += w * own.o;
        den += w * own.l;
    }
    return den > 0.0f ? num / den : 0.0f;
}

// ---- host side: what the four files of the family share under decode_attn (decode.hip) -------------------------------------------
// kernel ids and template-flag bits of a launch record (ivlm_llama_decode_attn_query)
enum Kernel : int { K_ONE_BLOCK = 0, K_SPLIT_KV, K_PREFIX_SHARED, K_PREFIX_OWN, K_VERIFY, K_FUSED };
constexpr int kFlagF32IO = 1, kFlagLO = 2, kFlagCF16 = 4, kFlagParts = 8;  // (the fused kernel: NB << 8)

// the fp32-only forms: f(record flags, CF16 as a std::bool_constant) for the call's cache kind
template <class F>
inline void with_cache_f16(const DecodeAttnArgs& a, F&& f) {
    if (a.cache_f16) f(kFlagF32IO | kFlagCF16, std::true_type{});
    else f(kFlagF32IO, std::false_type{});
}

// a dry run (ivlm_llama_decode_attn_query) points this at its record: launches are then noted instead of made
struct LaunchLog {
    int32_t* rec;  // 6 int32 per launch: kernel, flags, grid.x, grid.y, block, byte offset of the partials in the scratch (-1: none)
    int cap, n;
};
extern thread_local LaunchLog* t_launch_log;

// the one launcher of the family (ivlm_launch: a plain launch unless the caller armed ivlm_profile_launches - then the timing events
// ride on the kernel).  args must have the kernel's parameter types.
template <class K, class... A>
inline void launch(Kernel id, int flags, int64_t part_off, K kfn, dim3 grid, dim3 block, hipStream_t st, A... args) {
    if (LaunchLog* log = t_launch_log) {
        if (log->n < log->cap) {
            const int32_t v[6] = {id, flags, (int32_t)grid.x, (int32_t)grid.y, (int32_t)block.x, (int32_t)part_off};
            for (int i = 0; i < 6; ++i) log->rec[6 * log->n + i] = v[i];
        }
        ++log->n;
        return;
    }
    ivlm_launch(kfn, grid, block, 0, st, args...);
}

// the launches of a CHECKED call of the forms that live outside decode.hip
void launch_prefix(const DecodeAttnArgs& a, hipStream_t st);  // decode_prefix.hip
void launch_verify(const DecodeAttnArgs& a, hipStream_t st);  // verify.hip
int launch_fused(const DecodeAttnArgs& a, hipStream_t st);    // decode_fused.hip (asks the runtime for the CUs when a.cus == 0)
constexpr int kPrefixMaxB = 16, kVerifyMaxK = 16;

}  // namespace decattn
}  // namespace ivlm
