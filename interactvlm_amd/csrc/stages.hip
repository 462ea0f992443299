// Stage-level entry points of the language path (ivlm_llama_prefill / ivlm_llama_decode): thin C++ sequencers
// over the op launchers of this library, so that a non-Python caller can run a stage without re-implementing llava.py.
//
//   ivlm_llama_prefill      HF LlamaModel.forward over T new positions with a KV cache (model/llava/model/language_model/
//                           llava_llama.py:93-102 -> transformers LlamaModel): RMSNorm -> q|k|v GEMM -> RoPE + cache append ->
//                           causal flash attention -> o_proj (+ fp32 residual) -> RMSNorm -> gate|up GEMM with the SwiGLU
//                           epilogue -> down_proj (+ residual), final RMSNorm.
//   ivlm_llama_decode_step  the same for ONE new position on the weight-streaming kernels (fp32 activations, exact products):
//                           RMSNorm fused into the q|k|v and gate|up GEMVs, attention + o_proj in one launch when the grid fits
//                           the CUs, SwiGLU / residual adds in the GEMV epilogues.
//
// Weights arrive as a table of DEVICE pointers (one ivlm_llama_layer per decoder layer, bf16, the layouts of
// interactvlm_amd/llava.py: q|k|v rows concatenated, gate/up rows interleaved); all scratch lives in a caller workspace; nothing
// is allocated, nothing synchronises.  Same kernels and the same launch order as interactvlm_amd/llava.py: the results are
// bit-identical to the Python-sequenced path (tests/test_stages_gpu.py).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "kernels.h"

namespace ivlm {

namespace {

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// Hands out 256-byte aligned regions of a caller workspace.  Every stage names its buffers ONCE, in a carve_*() function: its body
// runs that on the real workspace, its *_workspace_bytes on a measuring carver (Carver{}: no base, no limit) and returns `used`,
// so a size cannot disagree with the takes.
struct Carver {
    char* base = nullptr;
    size_t room = SIZE_MAX, used = 0;
    bool ok = true;
    void* take(size_t bytes) {
        bytes = al(bytes);
        if (bytes > room - used) {
            ok = false;
            return nullptr;
        }
        used += bytes;
        return base ? base + (used - bytes) : nullptr;
    }
    template <class T>
    T* get(size_t count) {
        return static_cast<T*>(take(count * sizeof(T)));
    }
};
template <class Carve, class... Args>
size_t carved_bytes(Carve carve, Args... args) {
    Carver measure;
    carve(args..., measure);
    return measure.used;
}

// The fused split-K reduction (SplitKFused, kernels.h) is OPT-IN for the stage sequencers, as it is for the host model
// (ops.SPLITK_FUSED): on MI355X it measured 2 - 3 x SLOWER than the two-launch form (down_proj 64 -> 192 us, prefill 12.0 -> 26.3 ms;
// tools/experiments/README.md) - each block's agent-scope release / acquire around its arrival costs more than the launch it saves.
// Switch: ivlm_stages_splitk_fused(1), or IVLM_SPLITK_FUSED=1 in the environment at first use.  Off (default): no counters, no
// memset, the two-launch form everywhere.
// When it is on, the arrival counters live in the LAST 16 KB of a sequencer's split-K region: every stage call zeroes them once
// (sk_counters_zero, right after the region is carved) and the GEMMs leave them at zero; a product whose partials would reach into
// them takes the two-launch form on the region BELOW the counters (sk_partial_bytes), so the partials can never overwrite them.
// Every sequencer reads the switch ONCE, into the SkRegion it hands to its GEMMs: the counters it zeroed (or did not) are the ones its
// GEMMs count on (or do not), whatever the switch does meanwhile.
std::atomic<int> g_sk_fused{-1};  // -1: not read yet
bool sk_fused_on() {
    int v = g_sk_fused.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv("IVLM_SPLITK_FUSED");
        const int env = (e && e[0] == '1' && e[1] == 0) ? 1 : 0;
        if (g_sk_fused.compare_exchange_strong(v, env)) v = env;  // (else: another thread or the hook set it first - v holds that)
    }
    return v == 1;
}
struct SkRegion {  // a stage call's split-K workspace (none: no split-K) and its snapshot of the switch
    float* ws = nullptr;
    size_t bytes = 0;
    bool fused = false;
};
constexpr size_t kSkCounterBytes = (size_t)kSplitKCounters * 4;
int32_t* sk_counters(const SkRegion& sk, size_t partial_bytes) {
    if (!sk.fused || !sk.ws || sk.bytes < partial_bytes + kSkCounterBytes + 16) return nullptr;
    return reinterpret_cast<int32_t*>(reinterpret_cast<char*>(sk.ws) + ((sk.bytes - kSkCounterBytes) & ~(size_t)15));
}
// bytes of the region the PARTIALS may use: everything when the fused form is off, the part below the counters when it is on
size_t sk_partial_bytes(const SkRegion& sk) {
    if (!sk.fused || sk.bytes < kSkCounterBytes + 16) return sk.bytes;
    return (sk.bytes - kSkCounterBytes) & ~(size_t)15;
}
int sk_counters_zero(const SkRegion& sk, hipStream_t st) {
    int32_t* c = sk_counters(sk, 0);
    if (c) IVLM_HIP_TRY(hipMemsetAsync(c, 0, kSkCounterBytes, st));
    return IVLM_OK;
}
// one split-K product of a sequencer: fused when the switch is on and the partials stay below the counters, else the two-launch
// form - on the region below the counters, or (partials larger than that) on the whole region with the counters re-zeroed after
int sk_gemm(const GemmArgs& g, int sp, const SkRegion& sk, hipStream_t st) {
    const size_t pb = (size_t)sp * g.M * g.N * 4;
    int32_t* c = sk_counters(sk, pb);
    if (c) return gemm_bf16_splitk(g, sp, sk.ws, sk.bytes, st, c);
    if (pb <= sk_partial_bytes(sk)) return gemm_bf16_splitk(g, sp, sk.ws, sk_partial_bytes(sk), st, nullptr);
    if (int rc = gemm_bf16_splitk(g, sp, sk.ws, sk.bytes, st, nullptr)) return rc;
    return sk_counters_zero(sk, st);  // (only reachable with the switch on: the partials ran over the counter words)
}

// the linears of the LLaMA stages; flags: IVLM_GEMM_A_F32 / RES_F32 / F16 (A and W are IEEE halves: the fp16-operand prefill) /
// OUT_F16 (a 16-bit output is written as IEEE halves)
int lin(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int out_f32, int64_t ldc, const void* res, int M, int N, int K,
        int act, const void* rms_w, float eps, const SkRegion& sk, hipStream_t st, int flags) {
    GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, nullptr, res, N, 0, M, N, K, act, out_f32, flags);
    g.rms_w = static_cast<const bf16_t*>(rms_w);
    g.rms_eps = eps;
    const int sp = g.a_f32 ? 1 : gemm_splitk_choice(M, N, K, act, rms_w != nullptr);
    if (sp > 1 && (ldc & 3) == 0)
        return sk_gemm(g, sp, sk, st);
    return linear_bf16(g, st);
}

__global__ void bump_kernel(int32_t* a, int32_t* b) {
    if (a) *a += 1;
    if (b) *b += 1;
}

}  // namespace
}  // namespace ivlm

using namespace ivlm;

extern "C" int ivlm_stages_splitk_fused(int on) {
    const int prev = sk_fused_on() ? 1 : 0;
    if (on == 0 || on == 1) g_sk_fused.store(on, std::memory_order_relaxed);
    return prev;
}

static bool cfg_ok(const ivlm_llama_cfg* c) {
    // (max_len: the decode attention keeps one score per cached position in LDS - decattn::kMaxT = 4096 positions)
    return c && c->layers > 0 && c->hidden > 0 && c->heads > 0 && c->inter > 0 && c->hidden % c->heads == 0 && c->max_len > 0 &&
           c->max_len <= 4096 && (c->hidden & 7) == 0 && (c->inter & 7) == 0;
}

namespace {

// (xa / xb: the two fp32 residual streams; sk: split-K partials, <= 8 slices of [T, N <= max(hidden, inter)])
struct PrefillBufs { bf16_t *y, *qkv, *att, *hh; float *xa, *xb, *sk; size_t skb; };
PrefillBufs carve_prefill(const ivlm_llama_cfg* c, int T, Carver& cv) {
    const size_t t = T, h = c->hidden, in = c->inter, skb = 8 * t * std::max(h, in) * 4;
    return {cv.get<bf16_t>(t * h), cv.get<bf16_t>(t * 3 * h), cv.get<bf16_t>(t * h), cv.get<bf16_t>(t * in),
            cv.get<float>(t * h),  cv.get<float>(t * h),      cv.get<float>(skb / 4), skb};
}

}  // namespace

extern "C" size_t ivlm_llama_prefill_workspace_bytes(const ivlm_llama_cfg* c, int T) {
    return cfg_ok(c) && T > 0 ? carved_bytes(carve_prefill, c, T) : 0;
}

static int llama_prefill(const ivlm_llama_cfg* c, const ivlm_llama_layer* layers_host, const void* final_norm, void* kcache,
                         void* vcache, const float* cos_tab, const float* sin_tab, const float* x_in, int T, int pos0, float* hidden_out,
                         void* workspace, size_t workspace_bytes, ivlm_stream_t stream, const int f16) {
    ivlm_enter();
    if (!cfg_ok(c) || !layers_host || !final_norm || !kcache || !vcache || !x_in || !hidden_out || !workspace || T <= 0 || pos0 < 0 ||
        pos0 + T > c->max_len)
        return IVLM_ERR_INVALID_ARG;
    Carver cv{static_cast<char*>(workspace), workspace_bytes};
    auto [y, qkv, att, hh, xa, xb, skw, skb] = carve_prefill(c, T, cv);
    if (!cv.ok) return IVLM_ERR_WORKSPACE;
    const SkRegion sk{skw, skb, sk_fused_on()};
    hipStream_t st = ivlm_stream(stream);
    const int Hd = c->hidden, H = c->heads, D = Hd / H, I = c->inter;
    if (int rc0 = sk_counters_zero(sk, st)) return rc0;
    const int in16 = f16 ? IVLM_GEMM_F16 : 0, io16 = f16 ? IVLM_GEMM_F16 | IVLM_GEMM_OUT_F16 : 0;  // fp16 operands (and 16-bit outputs)
    const int64_t cache_layer = (int64_t)c->max_len * Hd;
    const float* x = x_in;
    int rc;
    for (int l = 0; l < c->layers; ++l) {
        const ivlm_llama_layer& L = layers_host[l];
        bf16_t* kc = static_cast<bf16_t*>(kcache) + l * cache_layer;
        bf16_t* vc = static_cast<bf16_t*>(vcache) + l * cache_layer;
        if ((rc = rmsnorm(x, 1, static_cast<const bf16_t*>(L.ln1), y, f16 ? 4 : 0, T, Hd, c->eps, st))) return rc;
        if ((rc = lin(y, Hd, L.qkv, Hd, qkv, 0, 3 * Hd, nullptr, T, 3 * Hd, Hd, ACT_NONE, nullptr, 0.f, sk, st, io16))) return rc;
        if ((rc = rope_kv(qkv, 3 * Hd, T, H, D, pos0, c->theta, kc, vc, st, cos_tab, sin_tab, f16))) return rc;
        AttnArgs a{};
        a.f16 = f16;
        a.q = qkv; a.k = kc; a.v = vc; a.o = att;
        a.q_bs = 0; a.q_hs = D; a.q_rs = 3 * Hd;
        a.k_bs = 0; a.k_hs = D; a.k_rs = Hd;
        a.v_bs = 0; a.v_hs = D; a.v_rs = Hd;
        a.o_bs = 0; a.o_hs = D; a.o_rs = Hd;
        a.B = 1; a.H = H; a.Sq = T; a.Sk = pos0 + T; a.D = D;
        a.scale = 1.0f / sqrtf((float)D);
        a.causal = 1; a.q_pos0 = pos0;
        a.kv_batch_div = 1; a.prescale_q = 0;
        if ((rc = attention_bf16(a, st))) return rc;
        float* x1 = (x == xa) ? xb : xa;
        if ((rc = lin(att, Hd, L.o, Hd, x1, 1, Hd, x, T, Hd, Hd, ACT_NONE, nullptr, 0.f, sk, st, in16 | IVLM_GEMM_RES_F32))) return rc;
        if ((rc = rmsnorm(x1, 1, static_cast<const bf16_t*>(L.ln2), y, f16 ? 4 : 0, T, Hd, c->eps, st))) return rc;
        if ((rc = lin(y, Hd, L.gu, Hd, hh, 0, I, nullptr, T, 2 * I, Hd, ACT_SWIGLU, nullptr, 0.f, sk, st, io16))) return rc;
        float* x2 = (x1 == xa) ? xb : xa;
        if ((rc = lin(hh, I, L.down, I, x2, 1, Hd, x1, T, Hd, I, ACT_NONE, nullptr, 0.f, sk, st, in16 | IVLM_GEMM_RES_F32))) return rc;
        x = x2;
    }
    return rmsnorm(x, 1, static_cast<const bf16_t*>(final_norm), hidden_out, 1, T, Hd, c->eps, st);
}

extern "C" int ivlm_llama_prefill(const ivlm_llama_cfg* c, const ivlm_llama_layer* layers_host, const void* final_norm,
                                  void* kcache, void* vcache, const float* cos_tab, const float* sin_tab, const float* x_in, int T,
                                  int pos0, float* hidden_out, void* workspace, size_t workspace_bytes, ivlm_stream_t stream) {
    return llama_prefill(c, layers_host, final_norm, kcache, vcache, cos_tab, sin_tab, x_in, T, pos0, hidden_out, workspace,
                         workspace_bytes, stream, 0);
}

// The default precision of the host model (interactvlm_amd/llava.py Llama._prefill_layer, "f16"): IEEE fp16 MFMA operands in one
// pass - the qkv / o / gu / down pointers of layers16_host are fp16 copies of the bf16 weights (ivlm_bf16_to_f16: exact inside the
// fp16 range; ln1 / ln2 stay the bf16 norm weights), RMSNorm / q|k|v / SwiGLU outputs and the KV cache are fp16.  Needs T > 16.
extern "C" int ivlm_llama_prefill_f16(const ivlm_llama_cfg* c, const ivlm_llama_layer* layers16_host, const void* final_norm,
                                      void* kcache16, void* vcache16, const float* cos_tab, const float* sin_tab, const float* x_in,
                                      int T, int pos0, float* hidden_out, void* workspace, size_t workspace_bytes,
                                      ivlm_stream_t stream) {
    if (T <= 16) return IVLM_ERR_UNSUPPORTED;  // (the fp16 tile GEMMs; short chunks go through ivlm_llama_decode_step_f16kv)
    return llama_prefill(c, layers16_host, final_norm, kcache16, vcache16, cos_tab, sin_tab, x_in, T, pos0, hidden_out, workspace,
                         workspace_bytes, stream, 1);
}

namespace {

// One carve for every form of the decode step (the caller zeroes it at the start of a generation, whichever form it then calls):
// activations | the fused launch's state: per-layer arrival counters (128 B apart), words [0] status, [1] tokens decoded so far,
// per-layer attention rows | the split-KV attention partials of the packed step (the parts layout of kernels.h, at its largest)
struct DecodeBufs { float *qkv, *hh, *xa, *xb, *att; int32_t *counters, *words; float *scratch, *parts; };
DecodeBufs carve_decode(const ivlm_llama_cfg* c, Carver& cv) {
    const size_t h = c->hidden, L = c->layers, H = c->heads;
    return {cv.get<float>(3 * h), cv.get<float>(c->inter), cv.get<float>(h), cv.get<float>(h), cv.get<float>(h),
            cv.get<int32_t>(L * 32), cv.get<int32_t>(64), cv.get<float>(L * h), cv.get<float>(H * kDecodePartsMaxS * decode_parts_stride(h / H))};
}

// The "linear" of a decode step, out = act(W . rmsnorm(x)) + res on fp32 activations with exact products (rms: the norm weight of the
// RMSNorm prologue or null; SwiGLU: N = 2 * inter interleaved gate / up rows -> inter outputs): on a bf16 matrix ...
int dec_linear(const ivlm_llama_cfg* c, const float* x, const void* W, float* out, const float* res, int N, int K, int act,
               const void* rms, ivlm_stream_t stream) {
    return lin(x, K, W, K, out, 1, act == ACT_SWIGLU ? N / 2 : N, res, 1, N, K, act, rms, rms ? c->eps : 0.f, SkRegion{}, ivlm_stream(stream),
               IVLM_GEMM_A_F32 | (res ? IVLM_GEMM_RES_F32 : 0));
}
// ... or on a losslessly packed one
int dec_linear(const ivlm_llama_cfg* c, const float* x, const ivlm_bf12m& m, float* out, const float* res, int N, int K, int act,
               const void* rms, ivlm_stream_t stream) {
    return ivlm_gemv1_bf12m(x, m.Pf, m.Ef, m.ebase, m.patch_ptr, m.patch_col, m.patch_val, out, nullptr, res, N, K, act, 1, rms,
                            rms ? c->eps : 0.0f, res ? IVLM_GEMM_RES_F32 : 0, stream);
}

// The decode step, written once for Layer = ivlm_llama_layer (bf16 weights) and ivlm_llama_layer_bf12 (packed weights).  Attention
// and o_proj take one of three forms:
//   fused      one launch, the o_proj blocks wait on device counters (bf16 weights and cache, fuse_attn_oproj, a grid that fits the CUs)
//   one block  one attention block per head, then o_proj as a linear (bf16 weights otherwise; packed weights with fuse_attn_oproj)
//   split KV   four key ranges per head, merged by the prologue of the packed o_proj (packed weights: the host model's default)
template <class Layer>
int decode_step(const ivlm_llama_cfg* c, const Layer* layers_host, const void* final_norm, void* kcache, void* vcache, int cache_f16,
                const float* cos_tab, const float* sin_tab, const float* x_in, int32_t* pos_dev, int advance, float* hidden_out,
                void* workspace, size_t workspace_bytes, ivlm_stream_t stream) {
    constexpr bool packed = std::is_same<Layer, ivlm_llama_layer_bf12>::value;
    ivlm_enter();
    if (!cfg_ok(c) || !layers_host || !final_norm || !kcache || !vcache || !cos_tab || !sin_tab || !x_in || !pos_dev || !hidden_out ||
        !workspace)
        return IVLM_ERR_INVALID_ARG;
    Carver cv{static_cast<char*>(workspace), workspace_bytes};
    const DecodeBufs b = carve_decode(c, cv);
    if (!cv.ok) return IVLM_ERR_WORKSPACE;
    const int Hd = c->hidden, H = c->heads, D = Hd / H, I = c->inter;
    if (packed && ((Hd & 63) || (I & 63))) return IVLM_ERR_UNSUPPORTED;  // (every matrix must take the fragment layout)
    hipStream_t st = ivlm_stream(stream);
    static int cus = 0;
    if (!packed && cus == 0) {
        int dev = 0;
        IVLM_HIP_TRY(hipGetDevice(&dev));
        IVLM_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    }
    const bool fused = !packed && !cache_f16 && c->fuse_attn_oproj && attn_oproj_fits(H, D, cus);
    const bool split_kv = packed && !c->fuse_attn_oproj;
    const int64_t cache_layer = (int64_t)c->max_len * Hd;
    // the attention of every layer: what changes per layer is the cache slab and, in the fused form, the operands of o_proj
    DecodeAttnArgs at = decode_attn_args(b.qkv, 1, nullptr, nullptr, cache_f16, c->max_len, b.att, H, D, 0, pos_dev, c->theta,
                                         1.0f / sqrtf((float)D), cos_tab, sin_tab);
    at.scratch = b.parts;  // (split KV: the parts buffer)
    at.step_dev = b.words + 1; at.status = b.words; at.cus = cus;
    const float* x = x_in;
    int rc = 0;
    for (int l = 0; l < c->layers; ++l) {
        const Layer& L = layers_host[l];
        at.kcache = static_cast<bf16_t*>(kcache) + l * cache_layer;
        at.vcache = static_cast<bf16_t*>(vcache) + l * cache_layer;
        if ((rc = dec_linear(c, x, L.qkv, b.qkv, nullptr, 3 * Hd, Hd, ACT_NONE, L.ln1, stream))) return rc;
        float* x1 = (x == b.xa) ? b.xb : b.xa;
        if (fused) {
            if constexpr (!packed) {
                at.scratch = b.scratch + (size_t)l * Hd; at.wo = static_cast<const bf16_t*>(L.o); at.x = x; at.x_out = x1;
                at.counter = b.counters + l * 32;
                rc = decode_attn(DA_FUSED, at, st);
            }
        } else if (split_kv) {
            if constexpr (packed) {
                rc = decode_attn(DA_PARTS, at, st);
                if (!rc)
                    rc = ivlm_gemv1_bf12m_parts(b.parts, D, L.o.Pf, L.o.Ef, L.o.ebase, L.o.patch_ptr, L.o.patch_col, L.o.patch_val, x1,
                                                nullptr, x, Hd, Hd, ACT_NONE, 1, IVLM_GEMM_RES_F32, stream);
            }
        } else {
            rc = decode_attn(DA_ONE_BLOCK, at, st);
            if (!rc) rc = dec_linear(c, b.att, L.o, x1, x, Hd, Hd, ACT_NONE, nullptr, stream);
        }
        if (rc) return rc;
        if ((rc = dec_linear(c, x1, L.gu, b.hh, nullptr, 2 * I, Hd, ACT_SWIGLU, L.ln2, stream))) return rc;
        float* x2 = (x1 == b.xa) ? b.xb : b.xa;
        if ((rc = dec_linear(c, b.hh, L.down, x2, x1, Hd, I, ACT_NONE, nullptr, stream))) return rc;
        x = x2;
    }
    if ((rc = rmsnorm(x, 1, static_cast<const bf16_t*>(final_norm), hidden_out, 1, 1, Hd, c->eps, st))) return rc;
    // (position += 1; the fused launch also counts the tokens decoded so far)
    bump_kernel<<<1, 1, 0, st>>>(fused ? b.words + 1 : nullptr, advance ? pos_dev : nullptr);
    return ivlm_launch_status();
}

}  // namespace

extern "C" size_t ivlm_llama_decode_workspace_bytes(const ivlm_llama_cfg* c) {
    return cfg_ok(c) ? carved_bytes(carve_decode, c) : 0;
}

extern "C" int ivlm_llama_decode_step(const ivlm_llama_cfg* c, const ivlm_llama_layer* layers_host, const void* final_norm,
                                      void* kcache, void* vcache, const float* cos_tab, const float* sin_tab, const float* x_in,
                                      int32_t* pos_dev, int advance, float* hidden_out, void* workspace, size_t workspace_bytes,
                                      ivlm_stream_t stream) {
    return decode_step(c, layers_host, final_norm, kcache, vcache, 0, cos_tab, sin_tab, x_in, pos_dev, advance, hidden_out, workspace,
                       workspace_bytes, stream);
}

// ... against the fp16 KV cache ivlm_llama_prefill_f16 fills: the bf16 weights of layers_host (fp32 activations, exact products, as
// in every mode), K / V rows appended and read as IEEE halves (separate attention / o_proj launches).
extern "C" int ivlm_llama_decode_step_f16kv(const ivlm_llama_cfg* c, const ivlm_llama_layer* layers_host, const void* final_norm,
                                            void* kcache16, void* vcache16, const float* cos_tab, const float* sin_tab,
                                            const float* x_in, int32_t* pos_dev, int advance, float* hidden_out, void* workspace,
                                            size_t workspace_bytes, ivlm_stream_t stream) {
    return decode_step(c, layers_host, final_norm, kcache16, vcache16, 1, cos_tab, sin_tab, x_in, pos_dev, advance, hidden_out,
                       workspace, workspace_bytes, stream);
}

// The same step with the four linears of a layer on losslessly packed weights (ivlm_gemv1_bf12m): the default decode path of the host
// model.  fp16 or bf16 KV cache; split-KV attention merged by the o_proj prologue unless fuse_attn_oproj asks for the one-block form.
extern "C" int ivlm_llama_decode_step_bf12(const ivlm_llama_cfg* c, const ivlm_llama_layer_bf12* layers_host, const void* final_norm,
                                           void* kcache, void* vcache, int cache_dtype, const float* cos_tab, const float* sin_tab,
                                           const float* x_in, int32_t* pos_dev, int advance, float* hidden_out, void* workspace,
                                           size_t workspace_bytes, ivlm_stream_t stream) {
    if (cache_dtype != IVLM_BF16 && cache_dtype != IVLM_F16) return IVLM_ERR_INVALID_ARG;
    return decode_step(c, layers_host, final_norm, kcache, vcache, cache_dtype == IVLM_F16, cos_tab, sin_tab, x_in, pos_dev, advance,
                       hidden_out, workspace, workspace_bytes, stream);
}

// =====================================================================================================================
// Vision stages: ivlm_clip_encode (CLIPVisionTower.forward + feature_select, clip_encoder.py:31-60) and ivlm_sam_encode
// (ImageEncoderViT.forward, image_encoder.py:110-125) as C++ sequencers - the launch order of interactvlm_amd/llava.py
// ClipTower._forward and interactvlm_amd/sam.py SamImageEncoder._forward (bf16 operands, fp32 residual stream).
// =====================================================================================================================
namespace ivlm {
namespace {

// window_partition / window_unpartition row maps of SAM's ViT on the device (image_encoder.py:263-318): part[w] = image row
// of window position w (-1 = zero padding), unpart[r] = window position of image row r
__global__ void sam_window_maps_kernel(int V, int g, int ws, int nw, int32_t* __restrict__ part, int32_t* __restrict__ unpart) {
    const int S = ws * ws;
    const int64_t total = (int64_t)V * nw * nw * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ix = (int)(i % ws), iy = (int)((i / ws) % ws);
        const int wx = (int)((i / S) % nw), wy = (int)((i / ((int64_t)S * nw)) % nw), v = (int)(i / ((int64_t)S * nw * nw));
        const int y = wy * ws + iy, x = wx * ws + ix;
        const bool ok = y < g && x < g;
        const int src = (v * g + y) * g + x;
        part[i] = ok ? src : -1;
        if (ok) unpart[src] = (int32_t)i;
    }
}

// dst[r] = row wherever part[r] < 0 (the zero-padded window positions: their q|k|v rows are the bias)
__global__ void fill_pad_rows_kernel(bf16_t* __restrict__ dst, int64_t ldd, const int32_t* __restrict__ part, int64_t rows,
                                     const bf16_t* __restrict__ row, int cols) {
    const int c8n = cols >> 3;
    const int64_t total = rows * c8n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / c8n;
        if (part[r] >= 0) continue;
        const int c8 = (int)(i % c8n);
        *reinterpret_cast<uint4*>(dst + r * ldd + c8 * 8) = *reinterpret_cast<const uint4*>(row + c8 * 8);
    }
}

// generic tile-GEMM call of the sequencers (bias, activation, bf16 / fp32 residual with row modulo, row maps, split-K rule);
// flags: IVLM_GEMM_A_SPLIT (A rows are [hi(K) | lo(K)]), IVLM_GEMM_OUT_SPLIT (the fp32 result as [hi(N) | lo(N)] rows),
// IVLM_GEMM_F16 (A and W are IEEE halves), IVLM_GEMM_OUT_F16 (a 16-bit output is written as IEEE halves)
int gemm(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int out_f32, int64_t ldc, const void* bias,
         const void* res, int res_f32, int64_t ldr, int res_mod, int M, int N, int K, int act, const int32_t* out_rows,
         const int32_t* a_rows, const SkRegion& sk, hipStream_t st, int flags = 0) {
    const GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, bias, res, ldr, res_mod, M, N, K, act, out_f32,
                                 flags | (res_f32 ? IVLM_GEMM_RES_F32 : 0), out_rows, a_rows);
    const int sp = (out_rows || a_rows) ? 1 : gemm_splitk_choice(M, N, K, act, 0);
    if (sp > 1 && (ldc & 3) == 0 && sk.ws && sk.bytes >= (size_t)sp * M * N * 4)
        return sk_gemm(g, sp, sk, st);
    return linear_bf16(g, st);
}

// Non-causal attention of the vision towers over B batches of S rows: q / k / v (and their lo planes, or null) are rows of stride
// rs with the heads side by side, the output rows have stride o_rs ([hi | lo] halves of H * D each when k_lo is set); q is scaled
// before Q.K^T.  f16: IEEE halves, q_lo then enters the rel-pos table product only (level 1).  rel_h / rel_w: the fp32 rel-pos
// arrays of a side x side grid, or the [rel_pos_h ; rel_pos_w] table and null (table mode), or both null.
int attend(const bf16_t* q, const bf16_t* q_lo, const bf16_t* k, const bf16_t* k_lo, const bf16_t* v, const bf16_t* v_lo, int64_t rs,
           bf16_t* o, int64_t o_rs, int f16, int B, int H, int S, int D, const void* rel_h, const float* rel_w, int side,
           hipStream_t st) {
    AttnArgs a{};
    a.f16 = f16;
    a.q = q; a.k = k; a.v = v; a.o = o;
    a.q_lo = q_lo; a.k_lo = k_lo; a.v_lo = v_lo; a.o_lo = k_lo ? o + H * D : nullptr;
    a.q_lo_level = (f16 && q_lo) ? 1 : 0;
    a.q_bs = a.k_bs = a.v_bs = (int64_t)S * rs;
    a.q_hs = a.k_hs = a.v_hs = a.o_hs = D;
    a.q_rs = a.k_rs = a.v_rs = rs;
    a.o_bs = (int64_t)S * o_rs; a.o_rs = o_rs;
    a.B = B; a.H = H; a.Sq = S; a.Sk = S; a.D = D;
    a.scale = 1.0f / sqrtf((float)D);
    a.rel_h = static_cast<const float*>(rel_h); a.rel_w = rel_w; a.rel_kh = side; a.rel_kw = side;
    a.kv_batch_div = 1; a.prescale_q = 1;
    return attention_bf16(a, st);
}

struct ClipBufs { bf16_t* cols; float *xa, *xb; bf16_t *y, *qkv, *att, *hh; float* sk; size_t skb; };  // (as PrefillBufs)
ClipBufs carve_clip(const ivlm_clip_cfg* c, int B, Carver& cv) {
    const size_t T = c->tokens, h = c->hidden, in = c->inter, R = B * T, skb = 8 * R * std::max(3 * h, in) * 4;
    return {cv.get<bf16_t>(B * (T - 1) * c->kpad), cv.get<float>(R * h), cv.get<float>(R * h), cv.get<bf16_t>(R * h),
            cv.get<bf16_t>(R * 3 * h), cv.get<bf16_t>(R * h), cv.get<bf16_t>(R * in), cv.get<float>(skb / 4), skb};
}

}  // namespace
}  // namespace ivlm

extern "C" size_t ivlm_clip_encode_workspace_bytes(const ivlm_clip_cfg* c, int B) {
    return c && B > 0 ? carved_bytes(carve_clip, c, B) : 0;
}

static int clip_encode(const ivlm_clip_cfg* c, const ivlm_clip_head* hd, const ivlm_clip_layer* layers_host, const void* images, int B,
                       void* features_out, void* workspace, size_t workspace_bytes, ivlm_stream_t stream, const int f16) {
    ivlm_enter();
    if (!c || !hd || !layers_host || !images || !features_out || !workspace || B <= 0) return IVLM_ERR_INVALID_ARG;
    Carver cv{static_cast<char*>(workspace), workspace_bytes};
    auto [cols, xa, xb, y, qkv, att, hh, skw, skb] = carve_clip(c, B, cv);
    if (!cv.ok) return IVLM_ERR_WORKSPACE;
    const SkRegion sk{skw, skb, sk_fused_on()};
    hipStream_t st = ivlm_stream(stream);
    const int T = c->tokens, Hd = c->hidden, H = c->heads, D = Hd / H, I = c->inter, R = B * T;
    if (int rc0 = sk_counters_zero(sk, st)) return rc0;
    int rc;
    if ((rc = im2col_nchw(static_cast<const bf16_t*>(images), cols, B, 3, c->image_size, c->image_size, c->patch, c->patch, c->kpad, st))) return rc;
    for (int b = 0; b < B; ++b) {  // patch GEMM writes rows 1..T-1 (+ their position embeddings); row 0 = class + position 0
        float* xrow = xa + (size_t)b * T * Hd;
        if ((rc = gemm(cols + (size_t)b * (T - 1) * c->kpad, c->kpad, hd->patch_w, c->kpad, xrow + Hd, 1, Hd, nullptr,
                       static_cast<const bf16_t*>(hd->pos) + Hd, 0, Hd, 0, T - 1, Hd, c->kpad, ACT_NONE, nullptr, nullptr, sk, st)))
            return rc;
        if ((rc = gather_rows(xrow, 1, Hd, hd->cls_row, 1, Hd, nullptr, nullptr, 0, 0, 1, Hd, st))) return rc;
    }
    if ((rc = layernorm(xa, 1, static_cast<const bf16_t*>(hd->pre_ln_w), static_cast<const bf16_t*>(hd->pre_ln_b), xb, 1, R, Hd, c->eps, st))) return rc;
    float* x = xb;
    const int k16 = f16 ? 4 : 0;                                      // LayerNorm output kind: IEEE halves | bf16
    const int in16 = f16 ? IVLM_GEMM_F16 : 0, io16 = f16 ? IVLM_GEMM_F16 | IVLM_GEMM_OUT_F16 : 0;  // fp16 operands (and 16-bit output)
    for (int l = 0; l < c->layers_run; ++l) {
        const ivlm_clip_layer& L = layers_host[l];
        if ((rc = layernorm(x, 1, static_cast<const bf16_t*>(L.ln1_w), static_cast<const bf16_t*>(L.ln1_b), y, k16, R, Hd, c->eps, st))) return rc;
        if ((rc = gemm(y, Hd, L.qkv_w, Hd, qkv, 0, 3 * Hd, L.qkv_b, nullptr, 0, 0, 0, R, 3 * Hd, Hd, ACT_NONE, nullptr, nullptr, sk, st, io16))) return rc;
        if ((rc = attend(qkv, nullptr, qkv + Hd, nullptr, qkv + 2 * Hd, nullptr, 3 * Hd, att, Hd, f16, B, H, T, D, nullptr, nullptr, 0, st))) return rc;
        float* x1 = (x == xa) ? xb : xa;
        if ((rc = gemm(att, Hd, L.out_w, Hd, x1, 1, Hd, L.out_b, x, 1, Hd, 0, R, Hd, Hd, ACT_NONE, nullptr, nullptr, sk, st, in16))) return rc;
        if ((rc = layernorm(x1, 1, static_cast<const bf16_t*>(L.ln2_w), static_cast<const bf16_t*>(L.ln2_b), y, k16, R, Hd, c->eps, st))) return rc;
        if ((rc = gemm(y, Hd, L.fc1_w, Hd, hh, 0, I, L.fc1_b, nullptr, 0, 0, 0, R, I, Hd, ACT_QUICK_GELU, nullptr, nullptr, sk, st, io16))) return rc;
        float* x2 = (x1 == xa) ? xb : xa;
        if ((rc = gemm(hh, I, L.fc2_w, I, x2, 1, Hd, L.fc2_b, x1, 1, Hd, 0, R, Hd, I, ACT_NONE, nullptr, nullptr, sk, st, in16))) return rc;
        x = x2;
    }
    // drop the CLS row of every image, fp32 stream -> bf16 features (the mm_projector's operand); fp16 mode: [hi | lo] bf16 rows
    // of width 2 * hidden (the projector takes split rows there: 0.03 % of the image's FLOPs)
    const int fw = f16 ? 2 * Hd : Hd;
    for (int b = 0; b < B; ++b)
        if ((rc = gather_rows(static_cast<bf16_t*>(features_out) + (size_t)b * (T - 1) * fw, f16 ? 2 : 0, fw, x + ((size_t)b * T + 1) * Hd, 1, Hd,
                              nullptr, nullptr, 0, 0, T - 1, Hd, st)))
            return rc;
    return IVLM_OK;
}

extern "C" int ivlm_clip_encode(const ivlm_clip_cfg* c, const ivlm_clip_head* hd, const ivlm_clip_layer* layers_host,
                                const void* images, int B, void* features_out, void* workspace, size_t workspace_bytes,
                                ivlm_stream_t stream) {
    return clip_encode(c, hd, layers_host, images, B, features_out, workspace, workspace_bytes, stream, 0);
}

// The default precision of the host model (interactvlm_amd/llava.py ClipTower, precision "f16"): IEEE fp16 MFMA operands - the
// qkv_w / out_w / fc1_w / fc2_w pointers of layers16_host are fp16 copies of the bf16 weights (biases and LayerNorm weights stay
// bf16); features_out: bf16 [B, tokens-1, 2*hidden] = [hi | lo] rows of the fp32 features (the mm_projector's split operand).
extern "C" int ivlm_clip_encode_f16(const ivlm_clip_cfg* c, const ivlm_clip_head* hd, const ivlm_clip_layer* layers16_host,
                                    const void* images, int B, void* features_split_out, void* workspace, size_t workspace_bytes,
                                    ivlm_stream_t stream) {
    return clip_encode(c, hd, layers16_host, images, B, features_split_out, workspace, workspace_bytes, stream, 1);
}

namespace ivlm {
namespace {

// =====================================================================================================================
// ivlm_sam_encode*: ONE sequencer for the precision modes of interactvlm_amd/sam.py SamImageEncoder._forward, bit-identical to it
// in each.  kSamModes restates the _MODES table of sam.py (norm output kinds: 0 bf16, 2 [hi | lo] bf16, 4 fp16, 5 [hi | lo] fp16;
// GEMM flags as gemm() takes them; a GEMM on fp16 operands reads the fp16 copy of its weight):
//   default      bf16 MFMA operands
//   f16q         IEEE fp16 operands in one pass with the q path exact (the host model's default): norm1 -> [hi | lo] halves;
//                q = W_q . (hi + lo) from its own GEMM as [hi | lo] halves, k | v from a single-pass GEMM on the hi half; table-mode
//                attention with the lo half of q in the rel-pos table products; the neck on [hi | lo] bf16 operands
//   parity       every activation that feeds an MFMA travels as [hi | lo] bf16 rows: split LayerNorm outputs, split-operand /
//                split-output GEMMs, split-operand attention with fp32 rel-pos terms from q = hi + lo, split neck
//   parity-fast  parity with the two MLP GEMMs on fp16 operands (norm2 and the GELU epilogue write halves, one MFMA pass)
// =====================================================================================================================
enum SamAttn {
    ATT_BF16,   // q|k|v rows of width 3D; rel-pos by shape: table mode from rel_cat, the batched G GEMM + gather, or the dot kernel
    ATT_F16Q,   // [q hi | q lo] and [k | v] fp16 rows of width 2D; table mode from rel_cat16 (head dim 80, 64 x 64 grid, small windows)
    ATT_SPLIT,  // [q k v hi | q k v lo] rows of width 6D; fp32 rel-pos arrays from the dot kernel on q = hi + lo (head dim 80)
};
constexpr int kSplitA = IVLM_GEMM_A_SPLIT, kSplitAO = IVLM_GEMM_A_SPLIT | IVLM_GEMM_OUT_SPLIT, kF16 = IVLM_GEMM_F16,
              kF16O = IVLM_GEMM_F16 | IVLM_GEMM_OUT_F16;
struct SamMode {
    int n1, qkv;  // norm1's output kind, the flags of the q|k|v GEMM (ATT_F16Q: of its q part)
    SamAttn attn;
    int proj, n2, lin1, lin2;  // the flags of the proj GEMM, norm2's output kind, the flags of the two MLP GEMMs
    bool split_neck;           // the neck takes [hi | lo] operands
};
constexpr SamMode kSamDefault{0, 0, ATT_BF16, 0, 0, 0, 0, false};
constexpr SamMode kSamF16q{5, kSplitAO | kF16O, ATT_F16Q, kF16, 4, kF16O, kF16, true};
constexpr SamMode kSamParityFast{2, kSplitAO, ATT_SPLIT, kSplitA, 4, kF16O, kF16, true};
constexpr SamMode kSamParity{2, kSplitAO, ATT_SPLIT, kSplitA, 2, kSplitAO, kSplitA, true};

struct SamDims {
    int g, D, H, hdim, wsz, OC, MD, Kp, nw, g2, R, nwin, WR, npad;
    SamDims(const ivlm_sam_cfg* c, int V)
        : g(c->grid), D(c->embed_dim), H(c->heads), hdim(D / H), wsz(c->window), OC(c->out_chans), MD(c->mlp_dim),
          Kp(3 * c->patch * c->patch), nw((g + wsz - 1) / wsz), g2(g * g), R(V * g2), nwin(V * nw * nw), WR(nwin * wsz * wsz),
          npad((2 * (2 * g - 1) + 7) / 8 * 8) {}
};

// The buffers of a mode (they follow its attention kind; the two parity modes share one carve and one size).  Rows that hold
// [hi | lo] halves are twice as wide; the q|k|v and attention rows cover the padded window grid.
struct SamBufs {
    float* x;                                       // the fp32 residual stream
    bf16_t *cols, *xn, *q, *kv, *att, *hh;          // patch columns; norm output; q|k|v (ATT_F16Q: [q hi | q lo], [k | v]); attention; MLP hidden
    float *relh_g, *relw_g, *relh_w, *relw_w;       // fp32 rel-pos arrays of a global / of a windowed block
    bf16_t *G, *brow;                               // the rel-pos GEMM's output; the [bias | 0] row of the padded window positions
    int32_t *part, *unpart;                         // window_partition / window_unpartition row maps
    void* n0;                                       // neck: conv outputs (fp32 when it is split), LayerNorm2d output, 3x3 columns
    bf16_t *n1, *c3;
};
SamBufs carve_sam(const SamDims& d, int V, const SamMode& m, Carver& cv) {
    const size_t R = d.R, WR = d.WR, D = d.D, qrows = std::max(R, WR), w = m.attn == ATT_SPLIT ? 2 : 1, nk = m.split_neck ? 2 : 1;
    SamBufs b{};
    b.cols = cv.get<bf16_t>(R * d.Kp), b.x = cv.get<float>(R * D);
    b.xn = cv.get<bf16_t>(R * D * (m.attn == ATT_BF16 ? 1 : 2));
    b.q = cv.get<bf16_t>(qrows * D * (m.attn == ATT_F16Q ? 2 : 3 * w));
    if (m.attn == ATT_F16Q) b.kv = cv.get<bf16_t>(qrows * 2 * D);
    b.att = cv.get<bf16_t>(qrows * D * w), b.hh = cv.get<bf16_t>(R * d.MD * w);
    const size_t rel_g = (size_t)V * d.H * d.g2 * d.g, rel_w = WR * d.H * d.wsz;
    if (m.attn != ATT_F16Q)  // (table mode needs no arrays)
        b.relh_g = cv.get<float>(rel_g), b.relw_g = cv.get<float>(rel_g), b.relh_w = cv.get<float>(rel_w), b.relw_w = cv.get<float>(rel_w);
    if (m.attn == ATT_BF16) b.G = cv.get<bf16_t>((size_t)d.H * R * d.npad);
    b.part = cv.get<int32_t>(WR), b.unpart = cv.get<int32_t>(R);
    if (m.attn != ATT_BF16) b.brow = cv.get<bf16_t>(D * (m.attn == ATT_F16Q ? 2 : 6));
    b.n0 = cv.take(R * d.OC * 2 * nk), b.n1 = cv.get<bf16_t>(R * d.OC * nk), b.c3 = cv.get<bf16_t>(R * 9 * d.OC * nk);
    return b;
}
size_t sam_workspace_bytes(const ivlm_sam_cfg* c, int V, const SamMode& m) {
    return c && V > 0 ? carved_bytes(carve_sam, SamDims(c, V), V, m) : 0;
}

// w16(l): the fp16 tensors of block l as an ivlm_sam_block_f16 whose unused members are null
template <class W16>
int sam_encode(const ivlm_sam_cfg* c, const ivlm_sam_head* hd, const ivlm_sam_block* blocks_host, W16 w16, const SamMode& m,
               const void* images, int V, float* embeddings_out, void* workspace, size_t workspace_bytes, ivlm_stream_t stream) {
    ivlm_enter();
    if (!c || !hd || !blocks_host || !images || !embeddings_out || !workspace || V <= 0) return IVLM_ERR_INVALID_ARG;
    const SamDims d(c, V);
    Carver cv{static_cast<char*>(workspace), workspace_bytes};
    const SamBufs b = carve_sam(d, V, m, cv);
    if (!cv.ok) return IVLM_ERR_WORKSPACE;
    const int g = d.g, D = d.D, H = d.H, hdim = d.hdim, wsz = d.wsz, OC = d.OC, MD = d.MD, Kp = d.Kp, R = d.R, WR = d.WR;
    // (the split attention / rel-pos kernels are built for SAM's head dim; table-mode attention for its grid and windows too)
    if (m.attn != ATT_BF16 && hdim != 80) return IVLM_ERR_UNSUPPORTED;
    if (m.attn == ATT_F16Q && (g != 64 || 2 * wsz > 32)) return IVLM_ERR_UNSUPPORTED;
    for (int l = 0; l < c->depth; ++l) {  // a NULL table would silently drop the rel-pos bias, a NULL fp16 copy fault
        const ivlm_sam_block& Bk = blocks_host[l];
        const ivlm_sam_block_f16 B16 = w16(l);
        if (m.attn == ATT_BF16 && (!Bk.rel_cat || !Bk.rel_h || !Bk.rel_w)) return IVLM_ERR_INVALID_ARG;
        if (m.attn == ATT_F16Q && (!B16.qkv_w16 || !B16.qkv_b16 || !B16.rel_cat16)) return IVLM_ERR_INVALID_ARG;
        if (((m.proj & kF16) && !B16.proj_w16) || ((m.lin1 & kF16) && !B16.lin1_w16) || ((m.lin2 & kF16) && !B16.lin2_w16))
            return IVLM_ERR_INVALID_ARG;
    }
    hipStream_t st = ivlm_stream(stream);
    auto ln = [&](const void* x, int x_f32, const void* w, const void* bias, void* y, int kind, int cols) {
        return layernorm(x, x_f32, static_cast<const bf16_t*>(w), static_cast<const bf16_t*>(bias), y, kind, R, cols, 1e-6f, st);
    };
    // A [R, K] . W[N, K]^T + bias -> 16-bit rows of width ldc (act applied), or, with res, += onto the fp32 stream
    auto mm = [&](const void* A, int64_t lda, const void* W, void* C, int64_t ldc, const void* bias, float* res, int N, int K, int act,
                  const int32_t* out_rows, const int32_t* a_rows, int flags) {
        return gemm(A, lda, W, K, C, res != nullptr, ldc, bias, res, res != nullptr, res ? D : 0, 0, R, N, K, act, out_rows, a_rows,
                    SkRegion{}, st, flags);
    };
    auto wide = [](int flags, int split_flag, int n) { return (flags & split_flag) ? 2 * n : n; };  // row width of a GEMM operand
    // dst[r] = [bias | 0] (width elements) at every padded window position r
    auto fill_pad_rows = [&](bf16_t* dst, int width, const void* bias, int bias_cols) {
        if (width > bias_cols) {
            IVLM_HIP_TRY(hipMemsetAsync(b.brow, 0, (size_t)width * 2, st));
            IVLM_HIP_TRY(hipMemcpyAsync(b.brow, bias, (size_t)bias_cols * 2, hipMemcpyDeviceToDevice, st));
            bias = b.brow;
        }
        fill_pad_rows_kernel<<<2048, 256, 0, st>>>(dst, width, b.part, WR, static_cast<const bf16_t*>(bias), width);
        return ivlm_launch_status();
    };
    int rc;
    sam_window_maps_kernel<<<256, 256, 0, st>>>(V, g, wsz, d.nw, b.part, b.unpart);
    if ((rc = ivlm_launch_status())) return rc;
    if ((rc = im2col_nchw(static_cast<const bf16_t*>(images), b.cols, V, 3, c->img_size, c->img_size, c->patch, c->patch, Kp, st))) return rc;
    if ((rc = gemm(b.cols, Kp, hd->patch_w, Kp, b.x, 1, D, hd->patch_b, hd->pos_embed, 0, D, d.g2, R, D, Kp, ACT_NONE, nullptr, nullptr, SkRegion{}, st))) return rc;
    float* x = b.x;
    const int64_t lx = m.attn == ATT_BF16 ? D : 2 * D;  // row width of norm1's output
    for (int l = 0; l < c->depth; ++l) {
        const ivlm_sam_block& Bk = blocks_host[l];
        const ivlm_sam_block_f16 B16 = w16(l);
        const bool glob = Bk.global_attn;
        const int side = glob ? g : wsz, S = side * side, nb = glob ? V : d.nwin;
        // a windowed block runs both attention GEMMs on the real rows only: the q|k|v GEMM scatters them to their window positions
        // (the padded positions get the bias), the proj GEMM gathers them back (window_unpartition) + shortcut, in place
        const int32_t* wmap = glob ? nullptr : b.unpart;
        if ((rc = ln(x, 1, Bk.norm1_w, Bk.norm1_b, b.xn, m.n1, D))) return rc;
        const bf16_t *q = b.q, *k, *v, *q_lo = nullptr, *k_lo = nullptr, *v_lo = nullptr;
        int64_t rs;  // row stride of q / k / v
        if (m.attn == ATT_F16Q) {
            const bf16_t *wq = static_cast<const bf16_t*>(B16.qkv_w16), *bq = static_cast<const bf16_t*>(Bk.qkv_b),
                         *bq16 = static_cast<const bf16_t*>(B16.qkv_b16);
            rs = 2 * D; q_lo = q + D; k = b.kv; v = b.kv + D;
            if ((rc = mm(b.xn, lx, wq, b.q, rs, bq, nullptr, D, D, ACT_NONE, wmap, nullptr, m.qkv))) return rc;
            if ((rc = mm(b.xn, lx, wq + (size_t)D * D, b.kv, rs, bq + D, nullptr, 2 * D, D, ACT_NONE, wmap, nullptr, kF16O))) return rc;
            if (!glob && ((rc = fill_pad_rows(b.q, 2 * D, bq16, D)) || (rc = fill_pad_rows(b.kv, 2 * D, bq16 + D, 2 * D)))) return rc;
        } else {
            rs = wide(m.qkv, IVLM_GEMM_OUT_SPLIT, 3 * D); k = q + D; v = q + 2 * D;
            if (m.attn == ATT_SPLIT) { q_lo = q + 3 * D; k_lo = q + 4 * D; v_lo = q + 5 * D; }
            if ((rc = mm(b.xn, lx, Bk.qkv_w, b.q, rs, Bk.qkv_b, nullptr, 3 * D, D, ACT_NONE, wmap, nullptr, m.qkv))) return rc;
            if (!glob && (rc = fill_pad_rows(b.q, rs, Bk.qkv_b, 3 * D))) return rc;
        }
        // the decomposed rel-pos terms: the attention kernel's TABLE MODE (it computes them itself from [rel_pos_h ; rel_pos_w],
        // rel_w = null: windows of 2 * side <= 32 and the 64 x 64 grid at head dim 80), or fp32 arrays [nb * H, S, side]
        const void* rh;
        float* rw = nullptr;
        if (m.attn == ATT_F16Q) {
            rh = B16.rel_cat16;
        } else if (m.attn == ATT_BF16 && hdim == 80 &&
                   ((side == 64 && 2 * (2 * side - 1) <= d.npad) || (2 * side <= 32 && 2 * (2 * side - 1) <= 64))) {
            rh = Bk.rel_cat;
        } else if (m.attn == ATT_BF16 && side >= 32) {  // one batched GEMM over the heads against rel_cat + Toeplitz gather
            rh = b.relh_g; rw = b.relw_g;
            const int M = nb * S;
            GemmArgs gg = gemm_args(q, rs, Bk.rel_cat, hdim, b.G, d.npad, nullptr, nullptr, 0, 0, M, d.npad, hdim, ACT_NONE, 0, 0);
            gg.batch = H; gg.strideA = hdim; gg.strideW = 0; gg.strideC = (int64_t)M * d.npad;
            if ((rc = linear_bf16(gg, st))) return rc;
            if ((rc = ivlm_relpos_gather(b.G, (int64_t)M * d.npad, d.npad, nb, H, side, side, b.relh_g, rw, stream))) return rc;
        } else {  // the dot kernel (ATT_SPLIT: on q = hi + lo)
            // (ATT_BF16 has always written these into the window-sized pair, which a GLOBAL block below 32 x 32 overruns - into
            //  the next buffers of the carve, not out of the workspace: its terms are wrong there; kept as it is)
            const bool big = glob && m.attn == ATT_SPLIT;
            float* rhf = big ? b.relh_g : b.relh_w;
            rh = rhf; rw = big ? b.relw_g : b.relw_w;
            if ((rc = relpos_bias(q, (int64_t)S * rs, hdim, rs, static_cast<const bf16_t*>(Bk.rel_h), static_cast<const bf16_t*>(Bk.rel_w),
                                  nb, H, side, side, hdim, rhf, rw, st, q_lo)))
                return rc;
        }
        const int64_t la = wide(m.proj, IVLM_GEMM_A_SPLIT, D);  // row width of the attention output
        if ((rc = attend(q, q_lo, k, k_lo, v, v_lo, rs, b.att, la, m.attn == ATT_F16Q, nb, H, S, hdim, rh, rw, side, st))) return rc;
        if ((rc = mm(b.att, la, (m.proj & kF16) ? B16.proj_w16 : Bk.proj_w, x, D, Bk.proj_b, x, D, D, ACT_NONE, nullptr, wmap, m.proj))) return rc;
        if ((rc = ln(x, 1, Bk.norm2_w, Bk.norm2_b, b.xn, m.n2, D))) return rc;
        const int64_t lh = wide(m.lin1, IVLM_GEMM_OUT_SPLIT, MD);  // row width of the MLP hidden
        if ((rc = mm(b.xn, wide(m.lin1, IVLM_GEMM_A_SPLIT, D), (m.lin1 & kF16) ? B16.lin1_w16 : Bk.lin1_w, b.hh, lh, Bk.lin1_b, nullptr, MD,
                     D, ACT_GELU, nullptr, nullptr, m.lin1)))
            return rc;
        if ((rc = mm(b.hh, lh, (m.lin2 & kF16) ? B16.lin2_w16 : Bk.lin2_w, x, D, Bk.lin2_b, x, D, MD, ACT_NONE, nullptr, nullptr, m.lin2))) return rc;
    }
    // neck: 1x1 conv, LayerNorm2d, 3x3 conv, LayerNorm2d - on bf16 operands, or on [hi | lo] operands with fp32 conv outputs
    const int sp = m.split_neck ? 1 : 0, nf = sp ? kSplitA : 0, nw_ = sp ? 2 * OC : OC;  // nw_: row width of the LayerNorm2d output
    if ((rc = gather_rows(b.xn, sp ? 2 : 0, sp ? 2 * D : D, x, 1, D, nullptr, nullptr, 0, 0, R, D, st))) return rc;
    if ((rc = gemm(b.xn, sp ? 2 * D : D, hd->neck0_w, D, b.n0, sp, OC, nullptr, nullptr, 0, 0, 0, R, OC, D, ACT_NONE, nullptr, nullptr, SkRegion{}, st, nf))) return rc;
    if ((rc = ln(b.n0, sp, hd->neck1_w, hd->neck1_b, b.n1, sp ? 2 : 0, OC))) return rc;
    for (int half = 0; half <= sp; ++half)  // (the hi and the lo halves are gathered separately)
        if ((rc = im2col3x3_nhwc(b.n1 + half * OC, b.c3 + half * 9 * OC, V, g, g, OC, st, nw_, 9 * nw_))) return rc;
    if ((rc = gemm(b.c3, 9 * nw_, hd->neck2_w, 9 * OC, b.n0, sp, OC, nullptr, nullptr, 0, 0, 0, R, OC, 9 * OC, ACT_NONE, nullptr, nullptr, SkRegion{}, st, nf))) return rc;
    return ln(b.n0, sp, hd->neck3_w, hd->neck3_b, embeddings_out, 1, OC);
}

constexpr auto kNoF16 = [](int) { return ivlm_sam_block_f16{}; };

}  // namespace
}  // namespace ivlm

extern "C" size_t ivlm_sam_encode_workspace_bytes(const ivlm_sam_cfg* c, int V) { return sam_workspace_bytes(c, V, kSamDefault); }
extern "C" size_t ivlm_sam_encode_parity_workspace_bytes(const ivlm_sam_cfg* c, int V) { return sam_workspace_bytes(c, V, kSamParity); }
extern "C" size_t ivlm_sam_encode_f16_workspace_bytes(const ivlm_sam_cfg* c, int V) { return sam_workspace_bytes(c, V, kSamF16q); }

// mode "default"
extern "C" int ivlm_sam_encode(const ivlm_sam_cfg* c, const ivlm_sam_head* hd, const ivlm_sam_block* blocks_host, const void* images,
                               int V, float* embeddings_out, void* workspace, size_t workspace_bytes, ivlm_stream_t stream) {
    return sam_encode(c, hd, blocks_host, kNoF16, kSamDefault, images, V, embeddings_out, workspace, workspace_bytes, stream);
}

// mode "parity"
extern "C" int ivlm_sam_encode_parity(const ivlm_sam_cfg* c, const ivlm_sam_head* hd, const ivlm_sam_block* blocks_host,
                                      const void* images, int V, float* embeddings_out, void* workspace, size_t workspace_bytes,
                                      ivlm_stream_t stream) {
    return sam_encode(c, hd, blocks_host, kNoF16, kSamParity, images, V, embeddings_out, workspace, workspace_bytes, stream);
}

// mode "parity-fast": mlp16_host[l] = the fp16 copies of block l's lin1_w / lin2_w; the workspace of the parity stage
extern "C" int ivlm_sam_encode_parity_f16mlp(const ivlm_sam_cfg* c, const ivlm_sam_head* hd, const ivlm_sam_block* blocks_host,
                                             const ivlm_sam_mlp_f16* mlp16_host, const void* images, int V, float* embeddings_out,
                                             void* workspace, size_t workspace_bytes, ivlm_stream_t stream) {
    if (!mlp16_host) return IVLM_ERR_INVALID_ARG;
    auto w16 = [=](int l) { return ivlm_sam_block_f16{nullptr, nullptr, mlp16_host[l].lin1_w16, mlp16_host[l].lin2_w16, nullptr, nullptr}; };
    return sam_encode(c, hd, blocks_host, w16, kSamParityFast, images, V, embeddings_out, workspace, workspace_bytes, stream);
}

// mode "f16q": blocks16_host[l] = the fp16 copies of block l's four GEMM weights, of its q|k|v bias and of rel_cat (ivlm_bf16_to_f16)
extern "C" int ivlm_sam_encode_f16(const ivlm_sam_cfg* c, const ivlm_sam_head* hd, const ivlm_sam_block* blocks_host,
                                   const ivlm_sam_block_f16* blocks16_host, const void* images, int V, float* embeddings_out,
                                   void* workspace, size_t workspace_bytes, ivlm_stream_t stream) {
    if (!blocks16_host) return IVLM_ERR_INVALID_ARG;
    return sam_encode(c, hd, blocks_host, [=](int l) { return blocks16_host[l]; }, kSamF16q, images, V, embeddings_out, workspace,
                      workspace_bytes, stream);
}

// =====================================================================================================================
// ivlm_sam_decode: PromptEncoder.forward(text_embeds) + MaskDecoder.forward(multimask_output=False) (prompt_encoder.py:140-186,
// mask_decoder.py:75-164, transformer.py:62-242) with fp32 activations end to end - the launch order of
// interactvlm_amd/sam.py SamMaskDecoder._forward.  Every linear takes [hi | lo] bf16 rows against [W | W] weights.
// =====================================================================================================================
namespace ivlm {
namespace {

struct DecCtx {
    hipStream_t st;
    ivlm_stream_t stream;
    Carver* cv;
    SkRegion sk;
    int rc = 0;
    void* take(size_t b) {
        void* p = cv->take(b);
        if (!p && !rc) rc = IVLM_ERR_WORKSPACE;
        return p;
    }
    // fp32 rows -> [hi | lo] bf16 rows
    bf16_t* split(const float* x, int64_t rows, int cols) {
        bf16_t* o = static_cast<bf16_t*>(take((size_t)rows * 2 * cols * 2));
        if (o && !rc) rc = gather_rows(o, 2, 2 * cols, x, 1, cols, nullptr, nullptr, 0, 0, rows, cols, st);
        return o;
    }
    // (a + b[r % b_rows]) as fp32 rows or as split rows
    void* add(const float* a, const float* b, int64_t rows, int cols, int64_t b_rows, bool as_split) {
        void* o = take((size_t)rows * cols * 4);  // (split rows: 2 * cols bf16 = the same bytes)
        if (o && !rc) rc = add_rows(o, as_split ? 2 : 1, a, 1, b, 1, rows, cols, b_rows, st, 0);
        return o;
    }
    // act(x_split . [W|W]^T + bias) + residual -> fp32 [M, N]
    float* lin(const bf16_t* xs, const ivlm_lin& L, int M, int act, const float* res, float* dst = nullptr) {
        float* o = dst ? dst : static_cast<float*>(take((size_t)M * L.n * 4));
        if (o && !rc) rc = gemm(xs, 2 * L.k, L.w2, 2 * L.k, o, 1, L.n, L.b, res, 1, L.n, 0, M, L.n, 2 * L.k, act, nullptr, nullptr, sk, st);
        return o;
    }
    float* norm(const float* x, const void* w, const void* b, int64_t rows, int cols, float eps, int gelu = 0) {
        float* o = static_cast<float*>(take((size_t)rows * cols * 4));
        if (o && !rc) rc = layernorm(x, 1, static_cast<const bf16_t*>(w), static_cast<const bf16_t*>(b), o, 1, rows, cols, eps, st, gelu);
        return o;
    }
    // Attention.forward (transformer.py:220-242) up to, not including, out_proj; returns the split rows of its output
    bf16_t* attn(const ivlm_dec_attn& a, const bf16_t* qs, const bf16_t* ks, const bf16_t* vs, int B, int Sq, int Sk, int heads) {
        float* q = lin(qs, a.q, B * Sq, ACT_NONE, nullptr);
        float* k = lin(ks, a.k, B * Sk, ACT_NONE, nullptr);
        float* v = lin(vs, a.v, B * Sk, ACT_NONE, nullptr);
        const int inner = a.q.n, d = inner / heads;
        float* o = static_cast<float*>(take((size_t)B * Sq * inner * 4));
        if (rc) return nullptr;
        const int64_t s12[12] = {(int64_t)Sq * inner, d, inner, (int64_t)Sk * inner, d, inner, (int64_t)Sk * inner, d, inner,
                                 (int64_t)Sq * inner, d, inner};
        rc = attention_f32(q, k, v, o, s12, B, heads, Sq, Sk, d, 1.0f / sqrtf((float)d), 1, st);
        return split(o, (int64_t)B * Sq, inner);
    }
};

}  // namespace
}  // namespace ivlm

extern "C" size_t ivlm_sam_decode_workspace_bytes(int V, int grid, int C, int n_text, int mlp_dim) {
    if (V <= 0 || grid <= 0 || C <= 0 || n_text <= 0) return 0;
    const size_t HW = (size_t)grid * grid, rows = (size_t)V * HW;
    // every intermediate has its own slot (one call = one carve, nothing is reused): ~40 image-sized fp32 / split buffers of
    // [V*HW, C], the upscaler's [V*HW*4, 128] pair, and the token-sized ones
    return 48 * al(rows * C * 4) + 3 * al(rows * 4 * 128 * 4) + 64 * al((size_t)V * (5 + n_text) * std::max(mlp_dim, 2 * C) * 4) +
           al((size_t)8 * V * (5 + n_text) * std::max(mlp_dim, C) * 4) + (1 << 20);
}

extern "C" int ivlm_sam_decode(const ivlm_sam_dec* w, int V, int grid, int n_text, const float* image_embeddings,
                               const float* text_embeds, float* low_res_out, float* iou_out, void* workspace, size_t workspace_bytes,
                               ivlm_stream_t stream) {
    ivlm_enter();
    if (!w || !image_embeddings || !text_embeds || !low_res_out || !iou_out || !workspace || V <= 0 || grid <= 0 || n_text <= 0 ||
        w->depth <= 0 || w->depth > 4)
        return IVLM_ERR_INVALID_ARG;
    const int C = w->C, HW = grid * grid, Nt = 5 + n_text, heads = w->heads;
    if (workspace_bytes < ivlm_sam_decode_workspace_bytes(V, grid, C, n_text, w->layers[0].lin1.n)) return IVLM_ERR_WORKSPACE;
    hipStream_t st = ivlm_stream(stream);
    Carver cv{static_cast<char*>(workspace), workspace_bytes};
    DecCtx x;
    x.st = st; x.stream = stream; x.cv = &cv;
    x.sk.bytes = (size_t)8 * V * Nt * std::max(w->layers[0].lin1.n, C) * 4;
    x.sk.ws = static_cast<float*>(x.take(x.sk.bytes));
    x.sk.fused = sk_fused_on();
    if (x.sk.ws) {
        if (int rc0 = sk_counters_zero(x.sk, st)) return rc0;
    }
    // tokens = [iou token ; mask tokens ; text embeds], the same set for every view
    float* tokens = static_cast<float*>(x.take((size_t)Nt * C * 4));
    float* query_pe = static_cast<float*>(x.take((size_t)V * Nt * C * 4));
    if (x.rc) return x.rc;
    int rc;
    if ((rc = gather_rows(tokens, 1, C, w->out_tokens, 1, C, nullptr, nullptr, 0, 0, 5, C, st))) return rc;
    if ((rc = gather_rows(tokens + 5 * C, 1, C, text_embeds, 1, C, nullptr, nullptr, 0, 0, n_text, C, st))) return rc;
    for (int v = 0; v < V; ++v)
        if ((rc = gather_rows(query_pe + (size_t)v * Nt * C, 1, C, tokens, 1, C, nullptr, nullptr, 0, 0, Nt, C, st))) return rc;
    const float* queries = query_pe;
    const float* keys = static_cast<const float*>(x.add(image_embeddings, static_cast<const float*>(w->no_mask), (int64_t)V * HW, C, 1, false));
    const float* key_pe = static_cast<const float*>(w->key_pe);
    const bf16_t* k_split = nullptr;
    for (int li = 0; li < w->depth && !x.rc; ++li) {
        const ivlm_dec_layer& L = w->layers[li];
        if (li == 0) {  // skip_first_layer_pe: queries = self_attn(q = k = v = queries), no residual
            const bf16_t* qs = x.split(queries, (int64_t)V * Nt, C);
            queries = x.lin(x.attn(L.self_attn, qs, qs, qs, V, Nt, Nt, heads), L.self_attn.o, V * Nt, ACT_NONE, nullptr);
        } else {
            const bf16_t* q = static_cast<const bf16_t*>(x.add(queries, query_pe, (int64_t)V * Nt, C, (int64_t)V * Nt, true));
            const bf16_t* sa = x.attn(L.self_attn, q, q, x.split(queries, (int64_t)V * Nt, C), V, Nt, Nt, heads);
            queries = x.lin(sa, L.self_attn.o, V * Nt, ACT_NONE, queries);
        }
        queries = x.norm(queries, L.norm1_w, L.norm1_b, (int64_t)V * Nt, C, 1e-5f);
        const bf16_t* q = static_cast<const bf16_t*>(x.add(queries, query_pe, (int64_t)V * Nt, C, (int64_t)V * Nt, true));
        k_split = static_cast<const bf16_t*>(x.add(keys, key_pe, (int64_t)V * HW, C, HW, true));
        const bf16_t* ca = x.attn(L.t2i, q, k_split, x.split(keys, (int64_t)V * HW, C), V, Nt, HW, heads);
        queries = x.norm(x.lin(ca, L.t2i.o, V * Nt, ACT_NONE, queries), L.norm2_w, L.norm2_b, (int64_t)V * Nt, C, 1e-5f);
        const float* h1 = x.lin(x.split(queries, (int64_t)V * Nt, C), L.lin1, V * Nt, ACT_RELU, nullptr);
        const float* mlp = x.lin(x.split(h1, (int64_t)V * Nt, L.lin1.n), L.lin2, V * Nt, ACT_NONE, queries);
        queries = x.norm(mlp, L.norm3_w, L.norm3_b, (int64_t)V * Nt, C, 1e-5f);
        q = static_cast<const bf16_t*>(x.add(queries, query_pe, (int64_t)V * Nt, C, (int64_t)V * Nt, true));
        const bf16_t* ia = x.attn(L.i2t, k_split, q, x.split(queries, (int64_t)V * Nt, C), V, HW, Nt, heads);  // image attends to tokens
        keys = x.norm(x.lin(ia, L.i2t.o, V * HW, ACT_NONE, keys), L.norm4_w, L.norm4_b, (int64_t)V * HW, C, 1e-5f);
    }
    if (x.rc) return x.rc;
    const bf16_t* q = static_cast<const bf16_t*>(x.add(queries, query_pe, (int64_t)V * Nt, C, (int64_t)V * Nt, true));
    const bf16_t* k = static_cast<const bf16_t*>(x.add(keys, key_pe, (int64_t)V * HW, C, HW, true));
    const bf16_t* fa = x.attn(w->final_attn, q, k, x.split(keys, (int64_t)V * HW, C), V, Nt, HW, heads);
    const float* hs = x.norm(x.lin(fa, w->final_attn.o, V * Nt, ACT_NONE, queries), w->norm_final_w, w->norm_final_b, (int64_t)V * Nt, C, 1e-5f);
    float* iou_tok = static_cast<float*>(x.take((size_t)V * C * 4));
    float* mask_tok = static_cast<float*>(x.take((size_t)V * C * 4));
    if (x.rc) return x.rc;
    if ((rc = gather_rows(iou_tok, 1, C, hs, 1, (int64_t)Nt * C, nullptr, nullptr, 0, 0, V, C, st))) return rc;       // hs[:, 0, :]
    if ((rc = gather_rows(mask_tok, 1, C, hs + C, 1, (int64_t)Nt * C, nullptr, nullptr, 0, 0, V, C, st))) return rc;  // hs[:, 1, :]
    // output_upscaling: ConvT(C -> C/4) -> LayerNorm2d -> GELU -> ConvT(C/4 -> C/8) -> GELU, as GEMMs on pixels
    const float* u = x.lin(x.split(keys, (int64_t)V * HW, C), w->up0, V * HW, ACT_NONE, nullptr);  // [V*HW, (dy,dx,C/4)]
    const int cm = w->up0.n / 4;
    const float* un = x.norm(u, w->up_ln_w, w->up_ln_b, (int64_t)V * HW * 4, cm, 1e-6f, 1);
    const float* u2 = x.lin(x.split(un, (int64_t)V * HW * 4, cm), w->up1, V * HW * 4, ACT_GELU, nullptr);  // [V*HW*4, (dy2,dx2,C/8)]
    const float* h0 = x.lin(x.split(mask_tok, V, C), w->hyper[0], V, ACT_RELU, nullptr);
    const float* h1 = x.lin(x.split(h0, V, w->hyper[0].n), w->hyper[1], V, ACT_RELU, nullptr);
    const float* h2 = x.lin(x.split(h1, V, w->hyper[1].n), w->hyper[2], V, ACT_NONE, nullptr);  // [V, C/8]
    if (x.rc) return x.rc;
    if ((rc = mask_dot(u2, h2, 1, low_res_out, V, grid, grid, w->hyper[2].n, st))) return rc;
    const float* i0 = x.lin(x.split(iou_tok, V, C), w->iou[0], V, ACT_RELU, nullptr);
    const float* i1 = x.lin(x.split(i0, V, w->iou[0].n), w->iou[1], V, ACT_RELU, nullptr);
    x.lin(x.split(i1, V, w->iou[1].n), w->iou[2], V, ACT_NONE, nullptr, iou_out);  // [V, n_mask]: column 0 is the kept mask's IoU
    return x.rc;
}
