// Speculative greedy decoding of ONE sequence: the attention of a verify pass (k <= 16 new tokens against the KV cache in one
// launch) and the accept step that turns the pass's argmax ids into the number of accepted draft tokens.
//
//   llama_verify_attn : rows i = 0 .. k-1 of qkv sit at positions pos .. pos+k-1 (pos read from device memory).  RoPE of q and k,
//                       append of the k key / value rows, causal attention (query i sees keys 0 .. pos+i), fp32 out.  One block per
//                       head: it appends its rows, keeps them in LDS, and streams the cached K / V rows 0 .. pos-1 ONCE for all k
//                       queries (online softmax over chunks of 256 keys).  The arithmetic is the single-token kernel's
//                       (decode_attn.h, fp32 I/O): fp32 q, the cached rows as stored, fp32 softmax and accumulation; query i sees
//                       the new rows 0 .. i-1 as they were cached (rounded) and its own row unrounded - exactly what i sequential
//                       decode steps see.  No block reads a row another block writes (the new rows come from LDS): the batched
//                       kernel with all rows on one slab would race.
//   spec_accept       : n_acc = leading draft tokens equal to the previous row's argmax, next token = argmax of row n_acc,
//                       pos += n_acc + 1 (one thread; graph-capturable).
#include "decode_attn.h"

namespace ivlm {
namespace {

constexpr int kVMaxK = decattn::kVerifyMaxK, kVMaxD = decattn::kMaxD, kVThreads = 1024, kVChunk = 256;

template <bool CF16>
__global__ __launch_bounds__(kVThreads) void llama_verify_attn_kernel(const float* __restrict__ qkv, int k, bf16_t* __restrict__ kcache,
                                                                      bf16_t* __restrict__ vcache, float* __restrict__ o, int H, int D,
                                                                      float theta, float scale, const float* __restrict__ ct,
                                                                      const float* __restrict__ stab,
                                                                      const int32_t* __restrict__ pos_dev, int tmax) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    __shared__ float q_s[kVMaxK][kVMaxD];
    __shared__ float kn_s[2][kVMaxK][kVMaxD];  // new key rows: [0] unrounded, [1] as cached; reused by the final reduction
    __shared__ float vn_s[2][kVMaxK][kVMaxD];
    __shared__ float sc[kVChunk][kVMaxK];      // scores, then softmax weights, of one chunk: [key][query]
    __shared__ float m_s[kVMaxK], l_s[kVMaxK], a_s[kVMaxK];
    const int h = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int pos = __builtin_amdgcn_readfirstlane(*pos_dev);
    const int half = D >> 1;
    const int64_t ldq = 3LL * H * D, rstride = (int64_t)H * D;
    // rows at or past the end of the slab are neither appended nor attended: their output rows are zeros
    const int kv = pos < 0 ? 0 : max(0, min(k, tmax - pos));
    const int nk = kv > 0 ? pos + kv : 0;  // keys seen by the last valid query (pos < tmax when kv > 0)
    if (t < kVMaxK) {
        m_s[t] = -INFINITY;
        l_s[t] = 0.0f;
        a_s[t] = 1.0f;
    }
    // ---- RoPE on q and k, append k / v (rounding as the single-token kernel) -------------------------------------------------
    for (int e = t; e < kv * half; e += kVThreads) {
        const int i = e / half, d = e - i * half, p = pos + i;
        const decattn::CosSin r = decattn::rope_cos_sin(ct, stab, p, d, half, D, theta);
        const float c = r.c, s = r.s;
        const float* row = qkv + i * ldq;
        const int64_t q = (int64_t)h * D, kk = rstride + h * D;
        const float q0 = row[q + d], q1 = row[q + d + half];
        const float k0 = row[kk + d], k1 = row[kk + d + half];
        const float qaf = q0 * c - q1 * s, qbf = q1 * c + q0 * s, kaf = k0 * c - k1 * s, kbf = k1 * c + k0 * s;
        const bf16_t ka = f32_to_h16<CF16>(kaf), kb = f32_to_h16<CF16>(kbf);
        q_s[i][d] = qaf;
        q_s[i][d + half] = qbf;
        kn_s[0][i][d] = kaf;
        kn_s[0][i][d + half] = kbf;
        kn_s[1][i][d] = h16_to_f32<CF16>(ka);
        kn_s[1][i][d + half] = h16_to_f32<CF16>(kb);
        bf16_t* kc = kcache + (int64_t)p * rstride + h * D;
        kc[d] = ka;
        kc[d + half] = kb;
    }
    for (int e = t; e < kv * D; e += kVThreads) {
        const int i = e / D, d = e - i * D;
        const float v = qkv[i * ldq + 2 * rstride + h * D + d];
        const bf16_t vh = f32_to_h16<CF16>(v);
        vn_s[0][i][d] = v;
        vn_s[1][i][d] = h16_to_f32<CF16>(vh);
        vcache[(int64_t)(pos + i) * rstride + h * D + d] = vh;
    }
    __syncthreads();
    // P.V accumulators: thread = (dim d, key slice ks of 8), all 16 queries; slices are summed at the end
    const int d = t & 127, ks = t >> 7;
    float acc[kVMaxK];
#pragma unroll
    for (int i = 0; i < kVMaxK; ++i) acc[i] = 0.0f;
    const int nch = D >> 3;
    for (int j0 = 0; j0 < nk; j0 += kVChunk) {
        const int clen = min(kVChunk, nk - j0);
        // ---- scores: wave w = (key block w & 3 of 64 keys, query group w >> 2 of 4 queries), one key per lane ------------------
        {
            const int jj = (w & 3) * 64 + lane, j = j0 + jj, i0 = (w >> 2) * 4;
            float s4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (i0 < kv && j < nk) {
                if (j < pos) {  // a cached row: every valid query sees it
                    float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    const bf16_t* kr = kcache + (int64_t)j * rstride + h * D;
#pragma unroll 4
                    for (int c8 = 0; c8 < nch; ++c8) {
                        const u32x4_t kv4 = *reinterpret_cast<const u32x4_t*>(kr + c8 * 8);
                        float kf[8];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            kf[2 * e] = pair_lo_f32<CF16>(kv4[e]);
                            kf[2 * e + 1] = pair_hi_f32<CF16>(kv4[e]);
                        }
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const float* qr = &q_s[min(i0 + qq, kVMaxK - 1)][c8 * 8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) a4[qq] += kf[e] * qr[e];
                        }
                    }
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
                        if (i0 + qq < kv) s4[qq] = a4[qq] * scale;
                } else {  // new row jn: rounded for the later queries, unrounded for its own, unseen by the earlier ones
                    const int jn = j - pos;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int i = i0 + qq;
                        if (i < kv && jn <= i) {
                            const float* kr = kn_s[jn == i ? 0 : 1][jn];
                            float a = 0.0f;
                            for (int e = 0; e < D; ++e) a += kr[e] * q_s[i][e];
                            s4[qq] = a * scale;
                        }
                    }
                }
            }
            if (i0 < kVMaxK) {
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) sc[jj][i0 + qq] = s4[qq];
            }
        }
        __syncthreads();
        // ---- online softmax: wave w = query w --------------------------------------------------------------------------------
        if (w < kVMaxK) {
            const int i = w;
            if (i < kv) {
                float mx = -INFINITY;
                for (int jj = lane; jj < clen; jj += 64) mx = fmaxf(mx, sc[jj][i]);
                mx = wave_max(mx);
                const float m_old = m_s[i], m_new = fmaxf(m_old, mx);
                float sum = 0.0f;
                for (int jj = lane; jj < kVChunk; jj += 64) {
                    const float p = (jj < clen && m_new > -INFINITY) ? __expf(sc[jj][i] - m_new) : 0.0f;
                    sc[jj][i] = p;
                    sum += p;
                }
                sum = wave_sum(sum);
                const float alpha = m_old > -INFINITY ? __expf(m_old - m_new) : 0.0f;
                if (lane == 0) {
                    m_s[i] = m_new;
                    l_s[i] = l_s[i] * alpha + sum;
                    a_s[i] = alpha;
                }
            } else {
                for (int jj = lane; jj < kVChunk; jj += 64) sc[jj][i] = 0.0f;
            }
        }
        __syncthreads();
        // ---- O += P.V: each V element is read once by the block ----------------------------------------------------------------
        if (d < D) {
            float al[kVMaxK];
#pragma unroll
            for (int i = 0; i < kVMaxK; ++i) {
                al[i] = a_s[i];
                acc[i] *= al[i];
            }
            const bf16_t* vb = vcache + h * D + d;
#pragma unroll 4
            for (int jj = ks; jj < clen; jj += 8) {
                const int j = j0 + jj;
                const float4* pr = reinterpret_cast<const float4*>(&sc[jj][0]);
                float p[kVMaxK];
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const float4 v4 = pr[c4];
                    p[4 * c4] = v4.x;
                    p[4 * c4 + 1] = v4.y;
                    p[4 * c4 + 2] = v4.z;
                    p[4 * c4 + 3] = v4.w;
                }
                if (j < pos) {
                    const float v = h16_to_f32<CF16>(vb[(int64_t)j * rstride]);
#pragma unroll
                    for (int i = 0; i < kVMaxK; ++i) acc[i] += p[i] * v;
                } else {
                    const int jn = j - pos;
                    const float vx = vn_s[0][jn][d], vq = vn_s[1][jn][d];
#pragma unroll
                    for (int i = 0; i < kVMaxK; ++i) acc[i] += p[i] * (i == jn ? vx : vq);
                }
            }
        }
        __syncthreads();
    }
    // ---- sum the 8 key slices (4 queries per round through LDS) and normalise ------------------------------------------------
    float* red = &kn_s[0][0][0];  // [8][4][128]
#pragma unroll
    for (int r = 0; r < kVMaxK / 4; ++r) {
        if (r * 4 >= k) break;
        if (d < D) {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) red[(ks * 4 + qq) * kVMaxD + d] = acc[r * 4 + qq];
        }
        __syncthreads();
        if (t < 4 * kVMaxD) {
            const int qq = t >> 7, dd = t & 127, i = r * 4 + qq;
            if (dd < D && i < k) {
                float s = 0.0f;
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) s += red[(s8 * 4 + qq) * kVMaxD + dd];
                o[(int64_t)i * rstride + h * D + dd] = i < kv ? s / l_s[i] : 0.0f;
            }
        }
        __syncthreads();
    }
}

__global__ void spec_accept_kernel(const int32_t* __restrict__ amax, const int32_t* __restrict__ fed, const int32_t* __restrict__ nd_dev,
                                   int k, int32_t* __restrict__ n_acc, int32_t* __restrict__ tok, int32_t* __restrict__ pos) {
    if (threadIdx.x != 0) return;
    const int nd = min(*nd_dev, k - 1);
    int n = 0;
    while (n < nd && fed[n + 1] == amax[n]) ++n;
    *n_acc = n;
    *tok = amax[n];
    *pos += n + 1;
}

}  // namespace

void decattn::launch_verify(const DecodeAttnArgs& a, hipStream_t st) {  // (a checked call: B = k rows)
    with_cache_f16(a, [&](int flags, auto cf) {
        launch(K_VERIFY, flags, -1, llama_verify_attn_kernel<cf.value>, dim3(a.H), dim3(kVThreads), st,
               static_cast<const float*>(a.qkv), a.B, a.kcache, a.vcache, static_cast<float*>(a.o), a.H, a.D, a.theta, a.scale, a.cos_tab, a.sin_tab,
               a.pos_dev, a.tmax);
    });
}

int spec_accept(const int32_t* amax, const int32_t* fed, const int32_t* nd_dev, int k, int32_t* n_acc, int32_t* tok, int32_t* pos,
                hipStream_t st) {
    if (!amax || !fed || !nd_dev || !n_acc || !tok || !pos || k <= 0 || k > kVMaxK) return IVLM_ERR_INVALID_ARG;
    spec_accept_kernel<<<1, 64, 0, st>>>(amax, fed, nd_dev, k, n_acc, tok, pos);
    return ivlm_launch_status();
}

}  // namespace ivlm

static int verify_entry(const float* qkv, int k, void* kcache, void* vcache, int cache_f16, int tmax, float* o, int H, int D,
                        const int32_t* pos_dev, float theta, float scale, const float* cos_tab, const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return ivlm::decode_attn(ivlm::DA_VERIFY, ivlm::decode_attn_args(qkv, 1, kcache, vcache, cache_f16, tmax, o, H, D, 0, pos_dev, theta,
        scale, cos_tab, sin_tab).rows(0, 0, 0, k), ivlm_stream(stream));
}

extern "C" int ivlm_llama_verify_attn(const float* qkv, int k, void* kcache, void* vcache, int tmax, float* o, int H, int D,
                                      const int32_t* pos_dev, float theta, float scale, const float* cos_tab, const float* sin_tab,
                                      ivlm_stream_t stream) {
    return verify_entry(qkv, k, kcache, vcache, 0, tmax, o, H, D, pos_dev, theta, scale, cos_tab, sin_tab, stream);
}

extern "C" int ivlm_llama_verify_attn_f16(const float* qkv, int k, void* kcache, void* vcache, int tmax, float* o, int H, int D,
                                          const int32_t* pos_dev, float theta, float scale, const float* cos_tab, const float* sin_tab,
                                          ivlm_stream_t stream) {
    return verify_entry(qkv, k, kcache, vcache, 1, tmax, o, H, D, pos_dev, theta, scale, cos_tab, sin_tab, stream);
}

extern "C" int ivlm_spec_accept(const int32_t* amax, const int32_t* fed, const int32_t* n_draft, int k, int32_t* n_acc, int32_t* tok,
                                int32_t* pos, ivlm_stream_t stream) {
    ivlm_enter();
    return ivlm::spec_accept(amax, fed, n_draft, k, n_acc, tok, pos, ivlm_stream(stream));
}
