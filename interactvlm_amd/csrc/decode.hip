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
//
// Host side of the whole family (this file, decode_prefix.hip, verify.hip, decode_fused.hip): a call is a DecodeAttnArgs and a form
// (kernels.h); decode_attn_check holds every argument rule, decode_attn routes a checked call to its kernel instantiation(s) through
// the one cache-kind dispatch and the one launcher of decode_attn.h.  The C entry points only fill the struct.
#include <climits>

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

// split-KV scratch: the per-head arrival counters, then (at this offset, a 256-byte boundary) the partials [H][kMaxSplits][D + 2] fp32
static size_t splitkv_partials(int H) { return (((size_t)H * 4 + 255) / 256) * 256; }
size_t llama_decode_attn_splitkv_scratch_bytes(int H, int D) {
    return H <= 0 || D <= 0 ? 0 : 256 + splitkv_partials(H) + (size_t)H * kMaxSplits * (D + 2) * 4;
}

int g_splitkv_splits = 8;  // A/B hook: ivlm_llama_decode_attn_splits

thread_local decattn::LaunchLog* decattn::t_launch_log = nullptr;

DecodeAttnArgs decode_attn_args(const void* qkv, int io_f32, void* kcache, void* vcache, int cache_f16, int tmax, void* o, int H, int D, int pos,
                                const int32_t* pos_dev, float theta, float scale, const float* cos_tab, const float* sin_tab) {
    DecodeAttnArgs a;
    a.qkv = qkv; a.io_f32 = io_f32; a.o = o; a.tmax = tmax; a.H = H; a.D = D; a.pos = pos; a.pos_dev = pos_dev;
    a.kcache = static_cast<bf16_t*>(kcache); a.vcache = static_cast<bf16_t*>(vcache); a.cache_f16 = cache_f16;
    a.theta = theta; a.scale = scale; a.cos_tab = cos_tab; a.sin_tab = sin_tab;
    return a;
}

// What each form requires, in the order the codes are reported when two rules are violated: INVALID_ARG for pointers and shapes,
// UNSUPPORTED for what the prefix and fused forms have no kernel for, INVALID_ARG for strides / positions / tables / cache kind (the
// prefix form has always reported these after its UNSUPPORTED rules; so does the fused form's lone table), WORKSPACE last.
int decode_attn_check(DecodeAttnForm form, const DecodeAttnArgs& a) {
    const bool prefix = form == DA_PREFIX, fused = form == DA_FUSED, strided = form == DA_BATCHED || prefix;
    const bool host_pos = form == DA_ONE_BLOCK || form == DA_SPLIT_KV || form == DA_PARTS;  // pos_dev may be null
    const bool any_io = form == DA_ONE_BLOCK || form == DA_BATCHED;                         // bf16 I/O and lo planes exist
    const bool own_scratch = form == DA_SPLIT_KV || form == DA_PARTS || fused;              // (a null one is reported at once)
    const int max_b = form == DA_BATCHED ? 65535 : form == DA_VERIFY ? kVerifyMaxK : prefix ? INT_MAX : 1;  // (grid.y; k of verify)
    const bool bad_d = a.D > kMaxD || (a.D & 15), misaligned = reinterpret_cast<uintptr_t>(a.scratch) & 15;
    const int64_t hd = (int64_t)a.H * a.D;
    if (!a.qkv || !a.kcache || !a.vcache || (!a.o && form != DA_PARTS && !fused) || (!a.pos_dev && !host_pos) ||
        (prefix && !a.prefix_len_dev) || (own_scratch && !a.scratch) ||
        (fused && (!a.wo || !a.x || !a.x_out || !a.step_dev || !a.counter || !a.status)))
        return IVLM_ERR_INVALID_ARG;
    if (a.B <= 0 || a.B > max_b || a.H <= 0 || (prefix && a.H > 65535) || a.D <= 0 || (!prefix && bad_d) || (!fused && a.tmax <= 0))
        return IVLM_ERR_INVALID_ARG;
    if (prefix && (!a.io_f32 || bad_d || a.B > kPrefixMaxB)) return IVLM_ERR_UNSUPPORTED;
    if (fused && (a.tmax <= 0 || !attn_oproj_fits(a.H, a.D, a.cus ? a.cus : INT_MAX))) return IVLM_ERR_UNSUPPORTED;
    if (!a.scratch && prefix) return IVLM_ERR_INVALID_ARG;
    if (strided && (a.ldq < 3 * hd || a.ldo < hd || a.cache_stride < hd || ((a.ldq | a.ldo | a.cache_stride) & 7) ||  // 16-byte rows
                    a.tmax * hd > a.cache_stride))                                                                      // tmax rows a slab
        return IVLM_ERR_INVALID_ARG;
    if (host_pos && !a.pos_dev && (a.pos < 0 || a.pos >= kMaxT || a.pos >= a.tmax)) return IVLM_ERR_INVALID_ARG;
    if ((a.cos_tab != nullptr) != (a.sin_tab != nullptr) || (a.kcache_lo != nullptr) != (a.vcache_lo != nullptr)) return IVLM_ERR_INVALID_ARG;
    if ((!a.io_f32 && (a.kcache_lo || a.cache_f16 || !any_io)) || (a.kcache_lo && (a.cache_f16 || !any_io)) || (a.cache_f16 && fused))
        return IVLM_ERR_INVALID_ARG;
    if (form == DA_PARTS && misaligned) return IVLM_ERR_INVALID_ARG;
    if (form == DA_SPLIT_KV && (a.scratch_bytes < llama_decode_attn_splitkv_scratch_bytes(a.H, a.D) || misaligned)) return IVLM_ERR_WORKSPACE;
    if (prefix && (a.scratch_bytes < llama_decode_attn_batch_prefix_scratch_bytes(a.B, a.H, a.D) || misaligned)) return IVLM_ERR_WORKSPACE;
    return IVLM_OK;
}

// the one-block kernel on grid (H, B) - the one-sequence form is B = 1 on strides 0 - over (io_f32, lo planes, cache_f16)
static void launch_one_block(const DecodeAttnArgs& a, hipStream_t st) {
    auto go = [&](int flags, auto kfn) {
        launch(K_ONE_BLOCK, flags, -1, kfn, dim3(a.H, a.B), dim3(kDecThreads), st, a.qkv, a.ldq, a.kcache, a.vcache, a.cache_stride, a.o, a.ldo,
               a.H, a.D, a.pos, a.theta, a.scale, a.cos_tab, a.sin_tab, a.pos_dev, a.tmax, a.kcache_lo, a.vcache_lo);
    };
    if (a.cache_f16) go(kFlagF32IO | kFlagCF16, llama_decode_attn_kernel<true, false, true>);
    else if (a.kcache_lo) go(kFlagF32IO | kFlagLO, llama_decode_attn_kernel<true, true, false>);
    else if (a.io_f32) go(kFlagF32IO, llama_decode_attn_kernel<true, false, false>);
    else go(0, llama_decode_attn_kernel<false, false, false>);
}
// the split-KV kernel on grid (H, S); PARTS: S = g_decode_parts_S ranges, the scratch is the parts buffer of ivlm_gemv1_bf12m_parts
template <bool PARTS>
static void launch_splitkv(const DecodeAttnArgs& a, hipStream_t st) {
    const size_t part_off = PARTS ? 0 : splitkv_partials(a.H);
    float* part = reinterpret_cast<float*>(static_cast<char*>(a.scratch) + part_off);
    with_cache_f16(a, [&](int flags, auto cf) {
        launch(K_SPLIT_KV, flags | (PARTS ? kFlagParts : 0), part_off, llama_decode_attn_splitkv_kernel<cf.value, PARTS>,
               dim3(a.H, PARTS ? g_decode_parts_S : g_splitkv_splits), dim3(splitkv::kT), st, static_cast<const float*>(a.qkv), a.kcache, a.vcache,
               PARTS ? nullptr : static_cast<float*>(a.o), a.H, a.D, a.pos, a.theta, a.scale, a.cos_tab, a.sin_tab, a.pos_dev, a.tmax, part,
               PARTS ? nullptr : static_cast<int32_t*>(a.scratch));
    });
}

int decode_attn(DecodeAttnForm form, const DecodeAttnArgs& a, hipStream_t st) {
    if (const int rc = decode_attn_check(form, a)) return rc;
    switch (form) {
        case DA_ONE_BLOCK:
        case DA_BATCHED: launch_one_block(a, st); break;
        case DA_SPLIT_KV: launch_splitkv<false>(a, st); break;
        case DA_PARTS: launch_splitkv<true>(a, st); break;
        case DA_PREFIX: launch_prefix(a, st); break;
        case DA_VERIFY: launch_verify(a, st); break;
        default:
            if (const int rc = launch_fused(a, st)) return rc;
    }
    return t_launch_log ? IVLM_OK : ivlm_launch_status();  // (a dry run made no launch and asks no runtime)
}

}  // namespace ivlm

// ---- C ABI: each entry point fills DecodeAttnArgs (one sequence: B = 1 on strides 0) and names its form ---------------------------
using ivlm::decode_attn;
using ivlm::decode_attn_args;

extern "C" int ivlm_llama_decode_attn(const void* qkv, int io_dtype, void* kcache, void* vcache, int tmax, void* o, int H, int D,
                                      int pos, const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                      const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return decode_attn(ivlm::DA_ONE_BLOCK, decode_attn_args(qkv, io_dtype == IVLM_F32, kcache, vcache, 0, tmax, o, H, D, pos, pos_dev,
        theta, scale, cos_tab, sin_tab), ivlm_stream(stream));
}

// "parity" precision: K / V cached as hi + lo bf16 planes (fp32 qkv / o); kcache_lo / vcache_lo as the hi caches
extern "C" int ivlm_llama_decode_attn_split(const void* qkv, void* kcache, void* kcache_lo, void* vcache, void* vcache_lo, int tmax,
                                            void* o, int H, int D, int pos, const int32_t* pos_dev, float theta, float scale,
                                            const float* cos_tab, const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    if (!kcache_lo || !vcache_lo) return IVLM_ERR_INVALID_ARG;
    return decode_attn(ivlm::DA_ONE_BLOCK, decode_attn_args(qkv, 1, kcache, vcache, 0, tmax, o, H, D, pos, pos_dev, theta, scale, cos_tab,
        sin_tab).lo(kcache_lo, vcache_lo), ivlm_stream(stream));
}

extern "C" int ivlm_llama_decode_attn_batch_split(const void* qkv, int64_t ldq, void* kcache, void* kcache_lo, void* vcache,
                                                  void* vcache_lo, int64_t cache_stride, int tmax, void* o, int64_t ldo, int B, int H,
                                                  int D, const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                                  const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    if (!kcache_lo || !vcache_lo) return IVLM_ERR_INVALID_ARG;
    return decode_attn(ivlm::DA_BATCHED, decode_attn_args(qkv, 1, kcache, vcache, 0, tmax, o, H, D, 0, pos_dev, theta, scale, cos_tab,
        sin_tab).rows(ldq, cache_stride, ldo, B).lo(kcache_lo, vcache_lo), ivlm_stream(stream));
}

extern "C" int ivlm_llama_decode_attn_batch(const void* qkv, int io_dtype, int64_t ldq, void* kcache, void* vcache,
                                            int64_t cache_stride, int tmax, void* o, int64_t ldo, int B, int H, int D,
                                            const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                            const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return decode_attn(ivlm::DA_BATCHED, decode_attn_args(qkv, io_dtype == IVLM_F32, kcache, vcache, 0, tmax, o, H, D, 0, pos_dev, theta,
        scale, cos_tab, sin_tab).rows(ldq, cache_stride, ldo, B), ivlm_stream(stream));
}

// fp16 KV cache (the fp16-operand prefill appends IEEE halves): fp32 qkv / o, K / V rows appended as fp16 and read back as fp16
extern "C" int ivlm_llama_decode_attn_f16(const void* qkv, void* kcache, void* vcache, int tmax, void* o, int H, int D, int pos,
                                          const int32_t* pos_dev, float theta, float scale, const float* cos_tab,
                                          const float* sin_tab, ivlm_stream_t stream) {
    ivlm_enter();
    return decode_attn(ivlm::DA_ONE_BLOCK, decode_attn_args(qkv, 1, kcache, vcache, 1, tmax, o, H, D, pos, pos_dev, theta, scale, cos_tab,
        sin_tab), ivlm_stream(stream));
}

extern "C" int ivlm_llama_decode_attn_batch_f16(const void* qkv, int64_t ldq, void* kcache, void* vcache, int64_t cache_stride,
                                                int tmax, void* o, int64_t ldo, int B, int H, int D, const int32_t* pos_dev,
                                                float theta, float scale, const float* cos_tab, const float* sin_tab,
                                                ivlm_stream_t stream) {
    ivlm_enter();
    return decode_attn(ivlm::DA_BATCHED, decode_attn_args(qkv, 1, kcache, vcache, 1, tmax, o, H, D, 0, pos_dev, theta, scale, cos_tab,
        sin_tab).rows(ldq, cache_stride, ldo, B), ivlm_stream(stream));
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
    ivlm::DecodeAttnArgs a = decode_attn_args(qkv, 1, kcache, vcache, cache_dtype == IVLM_F16, tmax, o, H, D, pos, pos_dev, theta, scale,
        cos_tab, sin_tab);
    a.scratch = scratch, a.scratch_bytes = scratch_bytes;
    return decode_attn(ivlm::DA_SPLIT_KV, a, ivlm_stream(stream));
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
    ivlm::DecodeAttnArgs a = decode_attn_args(qkv, 1, kcache, vcache, cache_dtype == IVLM_F16, tmax, nullptr, H, D, pos, pos_dev, theta,
        scale, cos_tab, sin_tab);
    a.scratch = parts;
    return decode_attn(ivlm::DA_PARTS, a, ivlm_stream(stream));
}

// Test hook: the check and the routing of ONE described call of the family, recorded instead of launched (see ivlm_hip.h).  The
// pointers are dummies of the alignment a caller's would have; nothing dereferences them on the host.
extern "C" int ivlm_llama_decode_attn_query(int form, int io_dtype, int cache_f16, int64_t ldq, int64_t ldo, int64_t cache_stride, int tmax,
                                            int B, int H, int D, int pos, int present, int scratch_skew, int64_t scratch_bytes, int cus,
                                            int32_t* record) {
    if (!record || form < 0 || form >= ivlm::DA_FORMS || (form == ivlm::DA_FUSED && cus <= 0)) return IVLM_ERR_INVALID_ARG;
    int bit = 0;
    const auto next = [&]() -> char* {  // the next pointer in the documented order of `present`: null when its bit is clear
        ++bit;
        return (present >> (bit - 1)) & 1 ? reinterpret_cast<char*>((uintptr_t)bit << 20) : nullptr;
    };
    char *qkv = next(), *kc = next(), *vc = next(), *o = next(), *pos_dev = next(), *plen = next(), *klo = next(), *vlo = next(), *ct = next(),
         *st = next(), *scratch = next();
    ivlm::DecodeAttnArgs a = decode_attn_args(qkv, io_dtype == IVLM_F32, kc, vc, cache_f16, tmax, o, H, D, pos,
        reinterpret_cast<int32_t*>(pos_dev), 10000.0f, 1.0f, reinterpret_cast<float*>(ct), reinterpret_cast<float*>(st)).rows(ldq,
        cache_stride, ldo, B).lo(klo, vlo);
    a.prefix_len_dev = reinterpret_cast<int32_t*>(plen);
    a.scratch = scratch ? scratch + scratch_skew : nullptr, a.scratch_bytes = (size_t)scratch_bytes, a.cus = cus;
    a.wo = reinterpret_cast<bf16_t*>(next()), a.x = reinterpret_cast<float*>(next()), a.x_out = reinterpret_cast<float*>(next());
    a.step_dev = reinterpret_cast<int32_t*>(next()), a.counter = reinterpret_cast<int32_t*>(next()), a.status = reinterpret_cast<int32_t*>(next());
    for (int i = 0; i < 14; ++i) record[i] = 0;
    ivlm::decattn::LaunchLog log{record + 2, 2, 0};
    ivlm::decattn::t_launch_log = &log;
    record[0] = decode_attn(static_cast<ivlm::DecodeAttnForm>(form), a, nullptr);
    ivlm::decattn::t_launch_log = nullptr;
    record[1] = log.n;
    return IVLM_OK;
}

