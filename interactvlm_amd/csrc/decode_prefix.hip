// One decode step of B <= 16 sequences whose first P cached positions are the SAME rows (several questions about one picture: the
// system text and the 256 image features).  The plain batched kernel (decode.hip, grid H x B) streams those P rows once per sequence
// from each sequence's own slab; here they are read from slab 0 ONCE for all B queries.
//
//   shared phase (llama_prefix_shared_kernel, grid H x S): the keys [0, P) of slab 0 are cut into S ranges.  A block stages 64 K / V
//       rows of its range in LDS (coalesced 16-byte loads, K and V of a chunk in flight together), computes the 64 x B scores (one key
//       per lane, four queries per wave, q broadcast from LDS), an online softmax per query and o += p.V for all B queries, and
//       publishes unnormalised (o, max, sum) per query: parts[h][s][b][decode_parts_stride(D)], plain stores.
//   own phase + merge (llama_prefix_own_kernel, grid H x B, the next launch on the same stream - the kernel boundary is the
//       synchronisation, no counter, no block waits for another): sequence b does RoPE of q and k, appends its new row at pos_dev[b]
//       of ITS slab, attends over its own rows [P, pos_dev[b]] (decode_attn_range on that range) and merges the S shared partials
//       (range order) and its own by the online-softmax rule (merge_ranges).  The order is fixed, so a launch is reproducible.
//
// Arithmetic: the single-token kernel's with fp32 I/O (decode_attn.h): fp32 q, fp32 softmax, the cached rows as stored (bf16 or
// IEEE fp16), the sequence's own new row unrounded; the appended rows are bit-identical to the plain batched kernel's.  The result
// differs from it by the fp32 summation order only.  P and the positions live in device memory: one captured graph per B.
#include "decode_attn.h"

namespace ivlm {
namespace {

using namespace decattn;

namespace prefix {
constexpr int kT = 256, kChunk = 64, kMaxB = kPrefixMaxB, kMinPer = 16;
constexpr int kG = kT / 16;  // staging rows per sweep (16 lanes share a row)
__host__ __device__ inline int clampP(int P, int tmax) {
    const int cap = tmax < kMaxT ? tmax : kMaxT;
    return P < 0 ? 0 : (P > cap ? cap : P);
}
inline int splits(int H) {
    const int s = 256 / H;
    return s < 1 ? 1 : (s > kMaxSplits ? kMaxSplits : s);
}
}  // namespace prefix

template <bool CF16>
__global__ __launch_bounds__(prefix::kT) void llama_prefix_shared_kernel(
    const float* __restrict__ qkv, int64_t ldq, const bf16_t* __restrict__ kcache /* slab 0 */, const bf16_t* __restrict__ vcache, int B,
    int H, int D, float theta, float scale, const float* __restrict__ ct, const float* __restrict__ stab,
    const int32_t* __restrict__ pos_dev, const int32_t* __restrict__ prefix_len_dev, int tmax, float* __restrict__ part) {
    using namespace prefix;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    __shared__ __attribute__((aligned(16))) float q_t[kMaxD][kMaxB];           // RoPE'd queries, [dim][query]
    __shared__ __attribute__((aligned(16))) uint32_t k_s[kChunk][kMaxD / 2 + 1];  // 16-bit pairs; padded: a lane per key row, no bank conflict
    __shared__ __attribute__((aligned(16))) uint32_t v_s[kChunk][kMaxD / 2];
    __shared__ __attribute__((aligned(16))) float sc[kChunk][kMaxB];           // scores, then softmax weights, [key][query]
    __shared__ float m_s[kMaxB], l_s[kMaxB], a_s[kMaxB];
    const int h = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int P = clampP(__builtin_amdgcn_readfirstlane(*prefix_len_dev), tmax);
    int per = (P + S - 1) / S;
    per = per < kMinPer ? kMinPer : per;
    const int k0 = min(sp * per, P), k1 = min(P, k0 + per);  // this block's keys [k0, k1): empty for the last ranges of a short prefix
    const int half = D >> 1, nch = D >> 3;
    const int64_t rstride = (int64_t)H * D;
    if (t < kMaxB) {
        m_s[t] = -INFINITY;
        l_s[t] = 0.0f;
        a_s[t] = 1.0f;
    }
    // ---- RoPE of the B queries (a sequence past its slab, or a row >= B: zeros, never used) -------------------------------------
    for (int e = t; e < kMaxB * half; e += kT) {
        const int i = e / half, d = e - i * half;
        float qa = 0.0f, qb = 0.0f;
        if (i < B) {
            const int pos = pos_dev[i];
            if (pos >= 0 && pos < tmax && pos < kMaxT) {
                const CosSin r = rope_cos_sin(ct, stab, pos, d, half, D, theta);
                const float* row = qkv + i * ldq + (int64_t)h * D;
                const float q0 = row[d], q1 = row[d + half];
                qa = q0 * r.c - q1 * r.s;
                qb = q1 * r.c + q0 * r.s;
            }
        }
        q_t[d][i] = qa;
        q_t[d + half][i] = qb;
    }
    const int pd = t & 127, pks = t >> 7;  // P.V: thread = (dim, key slice of 2), all 16 queries
    float acc[kMaxB];
#pragma unroll
    for (int i = 0; i < kMaxB; ++i) acc[i] = 0.0f;
    const int srow = t >> 4, sch = t & 15;  // staging: 16 lanes share a row, 16 rows per sweep
    const bf16_t* kb = kcache + (int64_t)h * D + sch * 8;
    const bf16_t* vb = vcache + (int64_t)h * D + sch * 8;
    for (int j0 = k0; j0 < k1; j0 += kChunk) {
        const int clen = min(kChunk, k1 - j0);
        // ---- stage the chunk's K / V rows (all loads in flight before the first store) ------------------------------------------
        {
            u32x4_t kr[kChunk / kG], vr[kChunk / kG];
#pragma unroll
            for (int it = 0; it < kChunk / kG; ++it) {
                int jj = srow + kG * it;
                jj = jj < clen ? jj : clen - 1;  // clamped (inside [k0, k1)), masked below
                const int c = sch < nch ? sch : 0;
                kr[it] = *reinterpret_cast<const u32x4_t*>(kb + (int64_t)(j0 + jj) * rstride + (c - sch) * 8);
                vr[it] = *reinterpret_cast<const u32x4_t*>(vb + (int64_t)(j0 + jj) * rstride + (c - sch) * 8);
            }
#pragma unroll
            for (int it = 0; it < kChunk / kG; ++it) {
                const int jj = srow + kG * it;
                if (jj < clen && sch < nch) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) k_s[jj][sch * 4 + e] = kr[it][e];
                    *reinterpret_cast<u32x4_t*>(&v_s[jj][sch * 4]) = vr[it];
                }
            }
        }
        __syncthreads();
        // ---- scores: lane = key, wave = four queries ----------------------------------------------------------------------------
        {
            const int i0 = w * 4;
            float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (i0 < B && lane < clen) {
#pragma unroll 8
                for (int d2 = 0; d2 < half; ++d2) {
                    const uint32_t kk = k_s[lane][d2];
                    const float klo = pair_lo_f32<CF16>(kk), khi = pair_hi_f32<CF16>(kk);
                    const float4 qa = *reinterpret_cast<const float4*>(&q_t[2 * d2][i0]);
                    const float4 qb = *reinterpret_cast<const float4*>(&q_t[2 * d2 + 1][i0]);
                    a4[0] += klo * qa.x;
                    a4[1] += klo * qa.y;
                    a4[2] += klo * qa.z;
                    a4[3] += klo * qa.w;
                    a4[0] += khi * qb.x;
                    a4[1] += khi * qb.y;
                    a4[2] += khi * qb.z;
                    a4[3] += khi * qb.w;
                }
            }
            float4 s4;
            s4.x = a4[0] * scale;
            s4.y = a4[1] * scale;
            s4.z = a4[2] * scale;
            s4.w = a4[3] * scale;
            *reinterpret_cast<float4*>(&sc[lane][i0]) = s4;
        }
        __syncthreads();
        // ---- online softmax: wave w owns queries w, w + 4, w + 8, w + 12 ----------------------------------------------------------
#pragma unroll
        for (int r = 0; r < kMaxB / 4; ++r) {
            const int i = w + 4 * r;
            if (i < B) {
                const float s = lane < clen ? sc[lane][i] : -INFINITY;
                const float mx = wave_max(s);
                const float m_old = m_s[i], m_new = fmaxf(m_old, mx);
                const float p = lane < clen ? __expf(s - m_new) : 0.0f;
                sc[lane][i] = p;
                const float sum = wave_sum(p);
                const float alpha = m_old > -INFINITY ? __expf(m_old - m_new) : 0.0f;
                if (lane == 0) {
                    m_s[i] = m_new;
                    l_s[i] = l_s[i] * alpha + sum;
                    a_s[i] = alpha;
                }
            } else {
                sc[lane][i] = 0.0f;
            }
        }
        __syncthreads();
        // ---- o += p.V: every staged V element is read by one thread, for all queries --------------------------------------------
        if (pd < D) {
#pragma unroll
            for (int i = 0; i < kMaxB; ++i) acc[i] *= a_s[i];
            for (int jj = pks; jj < clen; jj += 2) {
                const uint32_t vv = v_s[jj][pd >> 1];
                const float v = (pd & 1) ? pair_hi_f32<CF16>(vv) : pair_lo_f32<CF16>(vv);
                const float4* pr = reinterpret_cast<const float4*>(&sc[jj][0]);
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const float4 p4 = pr[c4];
                    acc[4 * c4] += p4.x * v;
                    acc[4 * c4 + 1] += p4.y * v;
                    acc[4 * c4 + 2] += p4.z * v;
                    acc[4 * c4 + 3] += p4.w * v;
                }
            }
        }
        __syncthreads();
    }
    // ---- sum the two key slices and publish (o, m, l) per query (an empty range: o = 0, m = -inf, l = 0) ---------------------------
    float* red = reinterpret_cast<float*>(&k_s[0][0]);  // [16][128] fp32 <= the K stage
    if (pks == 1 && pd < D) {
#pragma unroll
        for (int i = 0; i < kMaxB; ++i) red[i * kMaxD + pd] = acc[i];
    }
    __syncthreads();
    const int pstride = decode_parts_stride(D);
    float* mine = part + ((int64_t)h * S + sp) * B * pstride;
    if (pks == 0 && pd < D) {
#pragma unroll
        for (int i = 0; i < kMaxB; ++i)
            if (i < B) mine[i * pstride + pd] = acc[i] + red[i * kMaxD + pd];
    } else if (pks == 1 && pd < B) {
        mine[pd * pstride + D] = m_s[pd];
        mine[pd * pstride + D + 1] = l_s[pd];
    }
}

template <bool CF16>
__global__ __launch_bounds__(prefix::kT) void llama_prefix_own_kernel(
    const float* __restrict__ qkv_all, int64_t ldq, bf16_t* __restrict__ kcache_all, bf16_t* __restrict__ vcache_all,
    int64_t cache_stride, float* __restrict__ o_all, int64_t ldo, int H, int D, float theta, float scale,
    const float* __restrict__ ct, const float* __restrict__ stab, const int32_t* __restrict__ pos_dev,
    const int32_t* __restrict__ prefix_len_dev, int tmax, const float* __restrict__ part, int S) {
    using namespace prefix;
    const int h = blockIdx.x, b = blockIdx.y, B = gridDim.y;
    const int t = threadIdx.x;
    const int pos = __builtin_amdgcn_readfirstlane(pos_dev[b]);
    float* o = o_all + b * ldo;
    if (pos < 0 || pos >= tmax || pos >= kMaxT) {  // past the slab: nothing appended, a zero row (as the plain batched kernel)
        if (t < D) o[(int64_t)h * D + t] = 0.0f;
        return;
    }
    const int P = clampP(__builtin_amdgcn_readfirstlane(*prefix_len_dev), tmax);
    // the sequence's own keys [P, pos]; a position inside the prefix (excluded by the caller): own range empty, nothing appended.
    // The arithmetic of the plain batched kernel on that range: the appended rows are the same bit for bit.
    const bool owner = pos >= P;
    const RangeOut own = decode_attn_range<kT, true, false, CF16, false>(h, qkv_all + b * ldq, kcache_all + b * cache_stride,
                                                                          vcache_all + b * cache_stride, nullptr, nullptr, H, D, pos, P,
                                                                          owner ? pos + 1 : P, owner, theta, scale, ct, stab);
    if (t >= D) return;
    // ---- merge: the S shared partials in range order, then the own range (written by the previous launch: plain loads) -----------
    const int pstride = decode_parts_stride(D);
    const float* base = part + ((int64_t)h * S * B + b) * pstride;
    const int64_t sstride = (int64_t)B * pstride;
    float pm[kMaxSplits], pl[kMaxSplits], po[kMaxSplits];
#pragma unroll
    for (int s2 = 0; s2 < kMaxSplits; ++s2) {
        const float* ps = base + (s2 < S ? s2 : 0) * sstride;
        pm[s2] = ps[D];
        pl[s2] = ps[D + 1];
        po[s2] = ps[t];
    }
    o[(int64_t)h * D + t] = merge_ranges(pm, pl, po, S, own.l > 0.0f, own);
}

}  // namespace

size_t llama_decode_attn_batch_prefix_scratch_bytes(int B, int H, int D) {
    if (B <= 0 || H <= 0 || D <= 0) return 0;
    return (size_t)H * prefix::splits(H) * B * decode_parts_stride(D) * sizeof(float);
}

// the two launches of a checked call (with ivlm_profile_launches armed the start event rides on the first kernel, the stop event on
// the last); the partials fill the scratch from its start
void decattn::launch_prefix(const DecodeAttnArgs& a, hipStream_t st) {
    const int S = prefix::splits(a.H);
    float* part = static_cast<float*>(a.scratch);
    const float* q = static_cast<const float*>(a.qkv);
    with_cache_f16(a, [&](int flags, auto cf) {
        launch(K_PREFIX_SHARED, flags, 0, llama_prefix_shared_kernel<cf.value>, dim3(a.H, S), dim3(prefix::kT), st, q, a.ldq,
               (const bf16_t*)a.kcache, (const bf16_t*)a.vcache, a.B, a.H, a.D, a.theta, a.scale, a.cos_tab, a.sin_tab, a.pos_dev,
               a.prefix_len_dev, a.tmax, part);
        launch(K_PREFIX_OWN, flags, 0, llama_prefix_own_kernel<cf.value>, dim3(a.H, a.B), dim3(prefix::kT), st, q, a.ldq, a.kcache, a.vcache,
               a.cache_stride, static_cast<float*>(a.o), a.ldo, a.H, a.D, a.theta, a.scale, a.cos_tab, a.sin_tab, a.pos_dev, a.prefix_len_dev,
               a.tmax, (const float*)part, S);
    });
}

}  // namespace ivlm

extern "C" size_t ivlm_llama_decode_attn_batch_prefix_scratch_bytes(int B, int H, int D) {
    return ivlm::llama_decode_attn_batch_prefix_scratch_bytes(B, H, D);
}

static int prefix_entry(const void* qkv, int io_f32, int64_t ldq, void* kcache, void* vcache, int cache_f16, int64_t cache_stride, int tmax,
                        void* o, int64_t ldo, int B, int H, int D, const int32_t* pos_dev, const int32_t* prefix_len_dev, float theta,
                        float scale, const float* cos_tab, const float* sin_tab, void* scratch, size_t scratch_bytes, ivlm_stream_t stream) {
    ivlm_enter();
    ivlm::DecodeAttnArgs a = ivlm::decode_attn_args(qkv, io_f32, kcache, vcache, cache_f16, tmax, o, H, D, 0, pos_dev, theta, scale,
        cos_tab, sin_tab).rows(ldq, cache_stride, ldo, B);
    a.prefix_len_dev = prefix_len_dev; a.scratch = scratch; a.scratch_bytes = scratch_bytes;
    return ivlm::decode_attn(ivlm::DA_PREFIX, a, ivlm_stream(stream));
}

extern "C" int ivlm_llama_decode_attn_batch_prefix(const void* qkv, int io_dtype, int64_t ldq, void* kcache, void* vcache,
                                                   int64_t cache_stride, int tmax, void* o, int64_t ldo, int B, int H, int D,
                                                   const int32_t* pos_dev, const int32_t* prefix_len_dev, float theta, float scale,
                                                   const float* cos_tab, const float* sin_tab, void* scratch, size_t scratch_bytes,
                                                   ivlm_stream_t stream) {
    return prefix_entry(qkv, io_dtype == IVLM_F32, ldq, kcache, vcache, 0, cache_stride, tmax, o, ldo, B, H, D, pos_dev, prefix_len_dev, theta,
                        scale, cos_tab, sin_tab, scratch, scratch_bytes, stream);
}

extern "C" int ivlm_llama_decode_attn_batch_prefix_f16(const void* qkv, int64_t ldq, void* kcache, void* vcache, int64_t cache_stride,
                                                       int tmax, void* o, int64_t ldo, int B, int H, int D, const int32_t* pos_dev,
                                                       const int32_t* prefix_len_dev, float theta, float scale, const float* cos_tab,
                                                       const float* sin_tab, void* scratch, size_t scratch_bytes,
                                                       ivlm_stream_t stream) {
    return prefix_entry(qkv, 1, ldq, kcache, vcache, 1, cache_stride, tmax, o, ldo, B, H, D, pos_dev, prefix_len_dev, theta, scale, cos_tab,
                        sin_tab, scratch, scratch_bytes, stream);
}
