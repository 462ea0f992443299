// Single-token decode kernels of the LLaMA path (batch-1 greedy search driven by InteractVLM.evaluate,
// model/InteractVLM.py:524-531; arithmetic = HF LlamaAttention with a KV cache).
//
//   llama_decode_attn : RoPE(q,k at position pos) + KV-cache append + softmax(q.K^T/sqrt(d)).V for ONE new token,
//                       one workgroup per head.  Latency-bound (a few hundred KB of cache per layer): the three
//                       launches of the generic path (rope, cache write, attention) collapse into one.
//                       16 lanes share one key row (16-byte loads, 256-B coalesced per row), fp32 softmax.
//
// The arithmetic itself - one query against a key range of a slab - lives in decode_attn.h (decode_attn_range, merge_ranges) and is
// shared with decode_prefix.hip and decode_fused.hip; the kernels here are a prologue (position, past-the-slab zero row, the block's
// range), the range call, and an epilogue (store, or publish + merge).
#include "decode_attn.h"

namespace ivlm {
namespace {

using namespace decattn;

// B sequences of one decode step on grid (H, B): blockIdx.y picks the sequence; each has its own cache slab, qkv row, output row and
// position (the sequences of a batch sit at different lengths: prompts differ, model/InteractVLM.py:524-531 pads them).  The
// single-sequence entry point is B = 1, its position from the host (pos_dev null) or from device memory (one captured HIP graph
// then serves every decode step).
template <bool F32IO, bool LO, bool CF16>
__global__ __launch_bounds__(kDecThreads) void llama_decode_attn_kernel(
    const void* __restrict__ qkv, int64_t ldq, bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, int64_t cache_stride,
    void* __restrict__ o, int64_t ldo, int H, int D, int pos_arg, float theta, float scale, const float* __restrict__ ct,
    const float* __restrict__ stab, const int32_t* __restrict__ pos_dev, int tmax, bf16_t* __restrict__ kcache_lo,
    bf16_t* __restrict__ vcache_lo) {
    const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    constexpr int esz = F32IO ? 4 : 2;
    const int pos = pos_dev ? __builtin_amdgcn_readfirstlane(pos_dev[b]) : pos_arg;
    const int64_t e = b * ldo + (int64_t)h * D + t;
    // a sequence that has filled its cache slab (batched generation keeps stepping finished sequences; a C caller may step past
    // tmax) is skipped: nothing is appended and its output row is ZEROS, written here, so that nobody reads stale memory and the
    // caller does not have to clear the buffer with a launch of its own before every layer of every step
    if (pos >= tmax || pos >= kMaxT) {
        if (t < D) {
            if (F32IO) static_cast<float*>(o)[e] = 0.0f;
            else static_cast<bf16_t*>(o)[e] = 0;
        }
        return;
    }
    const RangeOut r = decode_attn_range<kDecThreads, F32IO, LO, CF16, true>(
        h, static_cast<const char*>(qkv) + b * ldq * esz, kcache + b * cache_stride, vcache + b * cache_stride,
        LO ? kcache_lo + b * cache_stride : nullptr, LO ? vcache_lo + b * cache_stride : nullptr, H, D, pos, 0, pos + 1, true, theta,
        scale, ct, stab);
    if (t < D) {
        if (F32IO) static_cast<float*>(o)[e] = r.o;
        else static_cast<bf16_t*>(o)[e] = f32_to_bf16(r.o);
    }
}

// ---- split-KV single-token attention (fp32 qkv / o; bf16 or fp16 cache) ------------------------------------------------------
// One 1024-thread block per head leaves 224 of the 256 CUs idle and walks its ~650 keys as a chain of dependent round trips
// (K tile, K tile, softmax, V tile): 6-8 us per layer.  Here the keys of a head are cut into S ranges (grid H x S, 256-thread
// blocks: 16 groups of 16 lanes, one key row per group and sweep, 96 keys per tile with K AND V of the tile in flight before
// anything else), every block runs decode_attn_range on its range (local max m, local sum l, unnormalised o = sum p v) and
// publishes (o, m, l); the block that arrives LAST for a head (one agent-scope counter per head, reset by that block: no spin,
// no residency assumption) merges the S partials in range order (merge_ranges).  The result does not depend on which block arrives
// last.  RoPE of q is recomputed by every block (64 lanes); the new K / V row is appended by the block whose range holds the position.
namespace splitkv {
constexpr int kT = 256, kG = kT / 16;  // ranges are whole sweeps of kG keys
}  // namespace splitkv

// PARTS: the block only writes its (o, m, l) - rows of decode_parts_stride(D) floats, plain stores - and the CONSUMER merges them (the
// o_proj GEMV reads the S partials of a head while it stages its activation row: ivlm_gemv1_bf12m_parts; the kernel boundary is the
// synchronisation, no counter, no merge round trips).
template <bool CF16, bool PARTS = false>
__global__ __launch_bounds__(splitkv::kT) void llama_decode_attn_splitkv_kernel(
    const float* __restrict__ qkv, bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, float* __restrict__ o, int H, int D,
    int pos_arg, float theta, float scale, const float* __restrict__ ct, const float* __restrict__ stab,
    const int32_t* __restrict__ pos_dev, int tmax, float* __restrict__ part, int32_t* __restrict__ counters) {
    using namespace splitkv;
    const int h = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const int t = threadIdx.x;
    const int pos = pos_dev ? __builtin_amdgcn_readfirstlane(*pos_dev) : pos_arg;
    const int pstride = PARTS ? decode_parts_stride(D) : D + 2;  // (the merged form keeps its partials in its own scratch)
    float* mine = part + ((int64_t)h * S + sp) * pstride;
    if (pos >= tmax || pos >= kMaxT) {  // past the slab: nothing appended, zeros out (as the one-block kernel)
        if (PARTS) {  // (o = 0, m = 0, l = 1 for range 0 and l = 0 for the others: the merge gives exactly 0)
            if (t < D) mine[t] = 0.0f;
            else if (t == 128) { mine[D] = 0.0f; mine[D + 1] = sp == 0 ? 1.0f : 0.0f; }
        } else if (sp == 0 && t < D) {
            o[(int64_t)h * D + t] = 0.0f;
        }
        return;
    }
    const int nkeys = pos + 1;
    int per = (nkeys + S - 1) / S;
    per = ((per + kG - 1) / kG) * kG;
    const int k0 = sp * per, k1 = min(nkeys, k0 + per);  // this block's keys [k0, k1): empty for the last ranges of a short context
    const RangeOut r = decode_attn_range<kT, true, false, CF16, false>(h, qkv, kcache, vcache, nullptr, nullptr, H, D, pos, k0, k1,
                                                                        pos >= k0 && pos < k1, theta, scale, ct, stab);
    // ---- publish (o, m, l); the last block of the head merges --------------------------------------------------------------------
    if (PARTS) {
        if (t < D) mine[t] = r.o;
        else if (t == 128) { mine[D] = r.m; mine[D + 1] = r.l; }
        return;
    }
    if (t < D) {
        __hip_atomic_store(mine + t, r.o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (t == 128) {
        __hip_atomic_store(mine + D, r.m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + D + 1, r.l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's agent-scope stores are performed
    __syncthreads();
    __shared__ int s_last;
    if (t == 0) {
        const int old = __hip_atomic_fetch_add(counters + h, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == S - 1;
        if (last) __hip_atomic_store(counters + h, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
        s_last = last;
    }
    __syncthreads();
    if (!s_last || t >= D) return;
    // all 3 S agent-scope loads in flight at once (a load per partial and round trip was most of the kernel's time)
    const float* base = part + (int64_t)h * S * pstride;
    float pm[kMaxSplits], pl[kMaxSplits], po[kMaxSplits];
#pragma unroll
    for (int s2 = 0; s2 < kMaxSplits; ++s2) {
        const float* ps = base + (int64_t)(s2 < S ? s2 : 0) * pstride;
        pm[s2] = __hip_atomic_load(ps + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pl[s2] = __hip_atomic_load(ps + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        po[s2] = __hip_atomic_load(ps + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    o[(int64_t)h * D + t] = merge_ranges(pm, pl, po, S, false, RangeOut{});
}

}  // namespace

// the one dispatch of the one-block kernel over (io_f32, lo planes, cache_f16), on grid (H, B); arguments checked by the callers
// (ivlm_launch: a plain launch unless the caller armed ivlm_profile_launches - then the timing events ride on the kernel)
static int launch_decode_attn(const void* qkv, int io_f32, int64_t ldq, bf16_t* kcache, bf16_t* vcache, int64_t cache_stride, int tmax,
                              void* o, int64_t ldo, int B, int H, int D, int pos, const int32_t* pos_dev, float theta, float scale,
                              const float* cos_tab, const float* sin_tab, hipStream_t st, bf16_t* kcache_lo, bf16_t* vcache_lo,
                              int cache_f16) {
    if ((kcache_lo != nullptr) != (vcache_lo != nullptr) || (kcache_lo && !io_f32)) return IVLM_ERR_INVALID_ARG;
    if (cache_f16 && (!io_f32 || kcache_lo)) return IVLM_ERR_INVALID_ARG;
    auto go = [&](auto kfn) {
        ivlm_launch(kfn, dim3(H, B), dim3(kDecThreads), 0, st, qkv, ldq, kcache, vcache, cache_stride, o, ldo, H, D, pos, theta, scale,
                    cos_tab, sin_tab, pos_dev, tmax, kcache_lo, vcache_lo);
    };
    if (cache_f16) go(llama_decode_attn_kernel<true, false, true>);
    else if (kcache_lo) go(llama_decode_attn_kernel<true, true, false>);
    else if (io_f32) go(llama_decode_attn_kernel<true, false, false>);
    else go(llama_decode_attn_kernel<false, false, false>);
    return ivlm_launch_status();
}

int llama_decode_attn_batch(const void* qkv, int io_f32, int64_t ldq, bf16_t* kcache, bf16_t* vcache, int64_t cache_stride,
                            int tmax, void* o, int64_t ldo, int B, int H, int D, const int32_t* pos_dev, float theta, float scale,
                            const float* cos_tab, const float* sin_tab, hipStream_t st, bf16_t* kcache_lo, bf16_t* vcache_lo,
                            int cache_f16) {
    if (!qkv || !kcache || !vcache || !o || !pos_dev) return IVLM_ERR_INVALID_ARG;
    if (B <= 0 || B > 65535 || H <= 0 || D <= 0 || D > kMaxD || (D & 15)) return IVLM_ERR_INVALID_ARG;
    if (ldq < 3LL * H * D || ldo < (int64_t)H * D || cache_stride < (int64_t)H * D || ((ldq | ldo | cache_stride) & 7))
        return IVLM_ERR_INVALID_ARG;  // 16-byte rows
    if (tmax <= 0 || (int64_t)tmax * H * D > cache_stride) return IVLM_ERR_INVALID_ARG;
    return launch_decode_attn(qkv, io_f32, ldq, kcache, vcache, cache_stride, tmax, o, ldo, B, H, D, 0, pos_dev, theta, scale, cos_tab,
                              sin_tab, st, kcache_lo, vcache_lo, cache_f16);
}

size_t llama_decode_attn_splitkv_scratch_bytes(int H, int D) {
    if (H <= 0 || D <= 0) return 0;
    return 256 + (((size_t)H * 4 + 255) / 256) * 256 + (size_t)H * kMaxSplits * (D + 2) * 4;
}

int g_splitkv_splits = 8;  // A/B hook: ivlm_llama_decode_attn_splits

// the PARTS form: S = g_decode_parts_S ranges, partials [H][S][decode_parts_stride(D)] fp32 for ivlm_gemv1_bf12m_parts
int llama_decode_attn_parts(const float* qkv, bf16_t* kcache, bf16_t* vcache, int tmax, float* parts, int H, int D, int pos, float theta,
                            float scale, hipStream_t st, const float* cos_tab, const float* sin_tab, const int32_t* pos_dev,
                            int cache_f16) {
    if (!qkv || !kcache || !vcache || !parts || H <= 0 || D <= 0 || D > kMaxD || (D & 15) || tmax <= 0) return IVLM_ERR_INVALID_ARG;
    if (!pos_dev && (pos < 0 || pos >= kMaxT || pos >= tmax)) return IVLM_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(parts) & 15) return IVLM_ERR_INVALID_ARG;
    const int S = g_decode_parts_S;
    if (cache_f16)
        llama_decode_attn_splitkv_kernel<true, true><<<dim3(H, S), splitkv::kT, 0, st>>>(qkv, kcache, vcache, nullptr, H, D, pos, theta, scale,
                                                                                         cos_tab, sin_tab, pos_dev, tmax, parts, nullptr);
    else
        llama_decode_attn_splitkv_kernel<false, true><<<dim3(H, S), splitkv::kT, 0, st>>>(qkv, kcache, vcache, nullptr, H, D, pos, theta, scale,
                                                                                          cos_tab, sin_tab, pos_dev, tmax, parts, nullptr);
    return ivlm_launch_status();
}

int llama_decode_attn_splitkv(const float* qkv, bf16_t* kcache, bf16_t* vcache, int tmax, float* o, int H, int D, int pos, float theta,
                              float scale, hipStream_t st, const float* cos_tab, const float* sin_tab, const int32_t* pos_dev,
                              int cache_f16, void* scratch, size_t scratch_bytes) {
    if (!qkv || !kcache || !vcache || !o || !scratch || H <= 0 || D <= 0 || D > kMaxD || (D & 15) || tmax <= 0) return IVLM_ERR_INVALID_ARG;
    if (!pos_dev && (pos < 0 || pos >= kMaxT || pos >= tmax)) return IVLM_ERR_INVALID_ARG;
    if (scratch_bytes < llama_decode_attn_splitkv_scratch_bytes(H, D) || (reinterpret_cast<uintptr_t>(scratch) & 15)) return IVLM_ERR_WORKSPACE;
    int32_t* counters = static_cast<int32_t*>(scratch);
    float* part = reinterpret_cast<float*>(static_cast<char*>(scratch) + (((size_t)H * 4 + 255) / 256) * 256);
    const int S = g_splitkv_splits;
    if (cache_f16)
        llama_decode_attn_splitkv_kernel<true><<<dim3(H, S), splitkv::kT, 0, st>>>(qkv, kcache, vcache, o, H, D, pos, theta, scale, cos_tab,
                                                                                   sin_tab, pos_dev, tmax, part, counters);
    else
        llama_decode_attn_splitkv_kernel<false><<<dim3(H, S), splitkv::kT, 0, st>>>(qkv, kcache, vcache, o, H, D, pos, theta, scale, cos_tab,
                                                                                    sin_tab, pos_dev, tmax, part, counters);
    return ivlm_launch_status();
}

int llama_decode_attn(const void* qkv, int io_f32, bf16_t* kcache, bf16_t* vcache, int tmax, void* o, int H, int D, int pos,
                      float theta, float scale, hipStream_t st, const float* cos_tab, const float* sin_tab,
                      const int32_t* pos_dev, bf16_t* kcache_lo, bf16_t* vcache_lo, int cache_f16) {
    if (!qkv || !kcache || !vcache || !o || H <= 0 || D <= 0 || D > kMaxD || (D & 15) || tmax <= 0) return IVLM_ERR_INVALID_ARG;
    if (!pos_dev && (pos < 0 || pos >= kMaxT || pos >= tmax)) return IVLM_ERR_INVALID_ARG;
    return launch_decode_attn(qkv, io_f32, 0, kcache, vcache, 0, tmax, o, 0, 1, H, D, pos, pos_dev, theta, scale, cos_tab, sin_tab, st,
                              kcache_lo, vcache_lo, cache_f16);
}

}  // namespace ivlm

extern "C" int ivlm_llama_decode_attn(const void* qkv, int io_dtype, void* kcache, void* vcache, int tmax, void* o, int H, int D,
                                      int pos, const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                      const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return ivlm::llama_decode_attn(qkv, io_dtype == IVLM_F32, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), tmax, o,
                                   H, D, pos, theta, scale, ivlm_stream(stream), cos_tab, sin_tab, pos_dev);
}

// "parity" precision: K / V cached as hi + lo bf16 planes (fp32 qkv / o); kcache_lo / vcache_lo as the hi caches
extern "C" int ivlm_llama_decode_attn_split(const void* qkv, void* kcache, void* kcache_lo, void* vcache, void* vcache_lo, int tmax,
                                            void* o, int H, int D, int pos, const int32_t* pos_dev, float theta, float scale,
                                            const float* cos_tab, const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    if (!kcache_lo || !vcache_lo) return IVLM_ERR_INVALID_ARG;
    return ivlm::llama_decode_attn(qkv, 1, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), tmax, o, H, D, pos, theta,
                                   scale, ivlm_stream(stream), cos_tab, sin_tab, pos_dev, static_cast<bf16_t*>(kcache_lo),
                                   static_cast<bf16_t*>(vcache_lo));
}

extern "C" int ivlm_llama_decode_attn_batch_split(const void* qkv, int64_t ldq, void* kcache, void* kcache_lo, void* vcache,
                                                  void* vcache_lo, int64_t cache_stride, int tmax, void* o, int64_t ldo, int B, int H,
                                                  int D, const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                                  const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    if (!kcache_lo || !vcache_lo) return IVLM_ERR_INVALID_ARG;
    return ivlm::llama_decode_attn_batch(qkv, 1, ldq, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), cache_stride, tmax,
                                         o, ldo, B, H, D, pos_dev, theta, scale, cos_tab, sin_tab, ivlm_stream(stream),
                                         static_cast<bf16_t*>(kcache_lo), static_cast<bf16_t*>(vcache_lo));
}

extern "C" int ivlm_llama_decode_attn_batch(const void* qkv, int io_dtype, int64_t ldq, void* kcache, void* vcache,
                                            int64_t cache_stride, int tmax, void* o, int64_t ldo, int B, int H, int D,
                                            const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                            const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return ivlm::llama_decode_attn_batch(qkv, io_dtype == IVLM_F32, ldq, static_cast<bf16_t*>(kcache),
                                         static_cast<bf16_t*>(vcache), cache_stride, tmax, o, ldo, B, H, D, pos_dev, theta, scale,
                                         cos_tab, sin_tab, ivlm_stream(stream));
}

// fp16 KV cache (the fp16-operand prefill appends IEEE halves): fp32 qkv / o, K / V rows appended as fp16 and read back as fp16
extern "C" int ivlm_llama_decode_attn_f16(const void* qkv, void* kcache, void* vcache, int tmax, void* o, int H, int D, int pos,
                                          const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                          const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return ivlm::llama_decode_attn(qkv, 1, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), tmax, o, H, D, pos, theta,
                                   scale, ivlm_stream(stream), cos_tab, sin_tab, pos_dev, nullptr, nullptr, 1);
}

extern "C" int ivlm_llama_decode_attn_batch_f16(const void* qkv, int64_t ldq, void* kcache, void* vcache, int64_t cache_stride,
                                                int tmax, void* o, int64_t ldo, int B, int H, int D, const int32_t* pos_dev,
                                                float theta, float scale, const float* cos_tab, const float* sin_tab,
                                                ivlm_stream_t stream) {
    ivlm_enter();
    return ivlm::llama_decode_attn_batch(qkv, 1, ldq, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), cache_stride, tmax,
                                         o, ldo, B, H, D, pos_dev, theta, scale, cos_tab, sin_tab, ivlm_stream(stream), nullptr,
                                         nullptr, 1);
}

// split-KV variant of ivlm_llama_decode_attn (fp32 qkv / o; cache_dtype IVLM_BF16 or IVLM_F16): H x S blocks, partials merged by the
// last block of each head.  scratch: ivlm_llama_decode_attn_splitkv_scratch_bytes(H, D) bytes, ZEROED once by the caller (it holds
// the per-head arrival counters, which the kernel leaves at zero), not shared by launches that may run concurrently.
extern "C" size_t ivlm_llama_decode_attn_splitkv_scratch_bytes(int H, int D) { return ivlm::llama_decode_attn_splitkv_scratch_bytes(H, D); }

extern "C" int ivlm_llama_decode_attn_splitkv(const float* qkv, int cache_dtype, void* kcache, void* vcache, int tmax, float* o, int H,
                                              int D, int pos, const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                              const float* sin_tab, void* scratch, size_t scratch_bytes, ivlm_stream_t stream) {
    ivlm_enter();
    if (cache_dtype != IVLM_BF16 && cache_dtype != IVLM_F16) return IVLM_ERR_INVALID_ARG;
    return ivlm::llama_decode_attn_splitkv(qkv, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), tmax, o, H, D, pos, theta,
                                           scale, ivlm_stream(stream), cos_tab, sin_tab, pos_dev, cache_dtype == IVLM_F16, scratch,
                                           scratch_bytes);
}

extern "C" int ivlm_llama_decode_attn_splits(int splits) {
    if (splits < 1 || splits > ivlm::decattn::kMaxSplits) return IVLM_ERR_INVALID_ARG;
    ivlm::g_splitkv_splits = splits;
    return IVLM_OK;
}

// Split-KV attention WITHOUT the merge: four key ranges per head, partials parts[H][4][D + 4] fp32 (o unnormalised | max | sum | pad) for
// the o_proj GEMV that merges them while it stages its activation row (ivlm_gemv1_bf12m_parts).  parts: 16-byte aligned,
// H * 4 * (D + 4) floats; no other state.
extern "C" int ivlm_llama_decode_attn_parts(const float* qkv, int cache_dtype, void* kcache, void* vcache, int tmax, float* parts, int H,
                                            int D, int pos, const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                            const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    if (cache_dtype != IVLM_BF16 && cache_dtype != IVLM_F16) return IVLM_ERR_INVALID_ARG;
    return ivlm::llama_decode_attn_parts(qkv, static_cast<bf16_t*>(kcache), static_cast<bf16_t*>(vcache), tmax, parts, H, D, pos, theta,
                                         scale, ivlm_stream(stream), cos_tab, sin_tab, pos_dev, cache_dtype == IVLM_F16);
}
