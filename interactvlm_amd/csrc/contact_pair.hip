// Contact-weighted human-object distance, the one term of the reference's joint fitting stage that consumes both contact
// vectors (optim/optimizer.py `contact_loss`), with both gradients and without the [N_o, N_h] distance matrix:
//
//   d_ij = |o_i - h_j|,  S = (sum p)(sum q),  L = sum_ij p_i q_j d_ij / S
//   dL/do_i = (p_i / S) sum_j q_j (o_i - h_j) / d_ij        dL/dh_j = (q_j / S) sum_i p_i (h_j - o_i) / d_ij
//
// Four launches, no atomics, every sum in a fixed order (the same bits every call):
//   pair_compact   one block per side: block_compact (fit_common.h) keeps the indices of the non-zero probabilities in order
//                  and their fp32 values; then the fp64 sum of those.  Everything after it walks the COMPACTED lists only, so
//                  rows and columns of probability 0 cost nothing and change no bit of the result: tiling and summation order
//                  are functions of the non-zero entries alone.
//   pair_sweep     the hot kernel.  A block keeps kStat "stationary" vertices in registers (kRows per thread) and sweeps one
//                  tile of kTile vertices of the other side, staged as {x, y, z, weight} float4 in LDS and read by all lanes
//                  at one address (a broadcast ds_read_b128: 4 LDS cycles per wave and entry, against ~60 VALU cycles).  The
//                  grid holds two roles: object-stationary blocks produce the value and the object gradient, human-stationary
//                  blocks the human gradient.  The pair arithmetic is done once per role instead of folding the human
//                  gradient across lanes: three 6-step wave reductions per swept vertex cost as much as the second pass at
//                  kRows = 2, and a fitter that moves the object only (the reference's case) launches no human role at all.
//                  Per (stationary vertex, tile) one float4 partial {gx, gy, gz, value} goes to the workspace.
//   pair_fold      per stationary vertex: the tile partials summed in tile order in fp64, scaled by 1 / S, scattered to the
//                  vertex's original index; per block of object vertices the fp64 sum of their value partials (block4_sum).
//   pair_value     per pose: the block sums by wave_fold, divided by S.
//
// Longest serial fp32 accumulation chain: the kTile = IVLM_CONTACT_PAIR_CHAIN terms one thread adds in the sweep.  The folds
// after it are fp64 and round to fp32 once.  Outside the chain a term carries at most 8 roundings of 2^-24 (to first order):
// the difference 1; 1 / d from the squared distance (half of its 2 + 2) 2, v_rsq_f32 to 1 ulp 2; the weight product 1; the
// stationary probability 1; the fp32 result 1 - the "+ 8" of the tests' bound (L_chain + 8) 2^-24 sum |terms|.
#include <algorithm>
#include <cfloat>

#include "fit_common.h"

namespace ivlm {
namespace {

constexpr int kTile = IVLM_CONTACT_PAIR_CHAIN;  // swept vertices per block
constexpr int kThreads = 128;
constexpr int kRows = 2;                    // stationary vertices per thread
constexpr int kStat = kThreads * kRows;     // stationary vertices per block
constexpr int kFold = 256;                  // threads (= vertices) of a fold block
constexpr int kMaxN = 1 << 20;

struct PairHeader {
    int32_t m[2];   // non-zero probabilities per side (0 = object, 1 = human)
    int32_t pad[2];
    double sum[2];  // their sums
};

// workspace carve, shared by the size query and the launcher
struct PairLayout {
    size_t hdr, idx[2], wt[2], part[2], blockval, total;
    int cb[2];  // tiles of side s when it is the swept side
    int sb[2];  // blocks of side s when it is the stationary side
    int fb;     // fold blocks of the object side
};

PairLayout pair_layout(int B, int n_o, int n_h) {
    PairLayout l;
    const int n[2] = {n_o, n_h};
    Carve c;
    l.hdr = c.take(sizeof(PairHeader));
    for (int s = 0; s < 2; ++s) {
        l.cb[s] = (n[s] + kTile - 1) / kTile;
        l.sb[s] = (n[s] + kStat - 1) / kStat;
        l.idx[s] = c.take((size_t)n[s] * 4);
        l.wt[s] = c.take((size_t)n[s] * 4);
    }
    for (int s = 0; s < 2; ++s) l.part[s] = c.take((size_t)B * l.cb[1 - s] * n[s] * 16);
    l.fb = (n_o + kFold - 1) / kFold;
    l.blockval = c.take((size_t)B * l.fb * 8);
    l.total = c.off;
    return l;
}

template <bool BF16>
__device__ __forceinline__ float load_prob(const void* p, int i) {
    if constexpr (BF16) return bf16_to_f32(static_cast<const bf16_t*>(p)[i]);
    else return static_cast<const float*>(p)[i];
}

// blockIdx.x = side.  idx[k] = index of the k-th non-zero probability, wt[k] = its value; hdr: their number and fp64 sum.
template <bool BF16>
__global__ __launch_bounds__(1024) void pair_compact_kernel(const void* __restrict__ p, const void* __restrict__ q, int n_o, int n_h,
                                                            PairHeader* __restrict__ hdr, int32_t* idx_o, float* wt_o,
                                                            int32_t* idx_h, float* wt_h) {
    __shared__ int32_t cnt[1024];
    __shared__ double red[16];
    const int side = blockIdx.x, t = threadIdx.x;
    const void* w = side ? q : p;
    const int n = side ? n_h : n_o;
    int32_t* idx = side ? idx_h : idx_o;
    float* wt = side ? wt_h : wt_o;
    const int m = block_compact(
        n, cnt, [&](int i) { return load_prob<BF16>(w, i) != 0.0f; },
        [&](int k, int i) {
            idx[k] = i;
            wt[k] = load_prob<BF16>(w, i);
        });
    __syncthreads();
    // the sum walks the compacted list, so that it is a function of the non-zero entries alone
    double s = 0.0;
    for (int j = t; j < m; j += 1024) s += (double)wt[j];
    s = wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        // NOT block4_sum's order: 16 waves, added one after the other from 0.0 - only the butterfly is the shared one
        double a = 0.0;
        for (int v = 0; v < 16; ++v) a += red[v];
        hdr->m[side] = m;
        hdr->sum[side] = a;
    }
}

struct PairArgs {
    const float* verts[2];   // object, human
    int64_t bstride[2];      // elements between poses (0: one pose shared by the batch)
    const PairHeader* hdr;
    const int32_t* idx[2];
    const float* wt[2];
    float4* part[2];
    int n[2], cb[2], sb[2];
    int role_blocks0;        // blocks of the object-stationary role (0 when it is not launched)
    int grad_o;              // object-stationary blocks also accumulate the gradient
};

// One block: stationary side S against tile `chunk` of the swept side W.
template <bool GRAD, bool VAL>
__device__ __forceinline__ void pair_sweep(const PairArgs& a, int S, int sblk, int chunk, int b, float4* tile) {
    const int W = 1 - S, t = threadIdx.x;
    const int m_s = a.hdr->m[S], m_w = a.hdr->m[W];
    if (sblk * kStat >= m_s || chunk * kTile >= m_w) return;  // block-uniform: nothing to do past the compacted lists
    const int count = min(kTile, m_w - chunk * kTile);
    const float* vw = a.verts[W] + (int64_t)b * a.bstride[W];
    for (int j = t; j < count; j += kThreads) {
        const int k = chunk * kTile + j;
        const float* v = vw + (int64_t)a.idx[W][k] * 3;
        tile[j] = make_float4(v[0], v[1], v[2], a.wt[W][k]);
    }
    const float* vs = a.verts[S] + (int64_t)b * a.bstride[S];
    float x[kRows], y[kRows], z[kRows], gx[kRows], gy[kRows], gz[kRows], val[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int k = sblk * kStat + r * kThreads + t;
        x[r] = y[r] = z[r] = 0.0f;
        if (k < m_s) {
            const float* v = vs + (int64_t)a.idx[S][k] * 3;
            x[r] = v[0];
            y[r] = v[1];
            z[r] = v[2];
        }
        gx[r] = gy[r] = gz[r] = val[r] = 0.0f;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < count; ++j) {
        const float4 e = tile[j];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const float dx = x[r] - e.x, dy = y[r] - e.y, dz = z[r] - e.z;
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            // a pair closer than sqrt(FLT_MIN) ~ 1e-19 counts as coincident: it contributes 0 to the value and to both gradients
            const float rinv = d2 >= FLT_MIN ? __builtin_amdgcn_rsqf(d2) : 0.0f;
            const float w = e.w * rinv;
            if constexpr (GRAD) {
                gx[r] = fmaf(w, dx, gx[r]);
                gy[r] = fmaf(w, dy, gy[r]);
                gz[r] = fmaf(w, dz, gz[r]);
            }
            if constexpr (VAL) val[r] = fmaf(w, d2, val[r]);  // q d = q d^2 / d
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int k = sblk * kStat + r * kThreads + t;
        if (k < m_s) {
            const float ws = a.wt[S][k];
            a.part[S][((int64_t)b * a.cb[W] + chunk) * a.n[S] + k] = make_float4(gx[r] * ws, gy[r] * ws, gz[r] * ws, val[r] * ws);
        }
    }
}

__global__ __launch_bounds__(kThreads) void pair_sweep_kernel(PairArgs a) {
    __shared__ float4 tile[kTile];
    int bx = blockIdx.x;
    const int b = blockIdx.y;
    if (bx < a.role_blocks0) {
        if (a.grad_o) pair_sweep<true, true>(a, 0, bx / a.cb[1], bx % a.cb[1], b, tile);
        else pair_sweep<false, true>(a, 0, bx / a.cb[1], bx % a.cb[1], b, tile);
    } else {
        bx -= a.role_blocks0;
        pair_sweep<true, false>(a, 1, bx / a.cb[0], bx % a.cb[0], b, tile);
    }
}

// blockIdx.x < fb_o: object vertices (compacted order) - gradient (if asked for) and the block's value sum; the blocks after
// them: human vertices (launched only with grad_h).  Gradients of zero-probability vertices were zeroed by the launcher.
__global__ __launch_bounds__(kFold) void pair_fold_kernel(PairArgs a, int fb_o, float* __restrict__ grad_o, float* __restrict__ grad_h,
                                                          double* __restrict__ blockval) {
    __shared__ double red[4][1];
    static_assert(kFold == 256, "block4_sum: four waves");
    const int b = blockIdx.y, t = threadIdx.x;
    const int S = (int)blockIdx.x >= fb_o, W = 1 - S;
    const int k = ((int)blockIdx.x - (S ? fb_o : 0)) * kFold + t;
    const int m_s = a.hdr->m[S], m_w = a.hdr->m[W];
    const int tiles = (m_w + kTile - 1) / kTile;
    const double inv = 1.0 / (a.hdr->sum[0] * a.hdr->sum[1]);
    float* grad = S ? grad_h : grad_o;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    if (k < m_s) {
        for (int c = 0; c < tiles; ++c) {
            const float4 v = a.part[S][((int64_t)b * a.cb[W] + c) * a.n[S] + k];
            g[0] += (double)v.x;
            g[1] += (double)v.y;
            g[2] += (double)v.z;
            g[3] += (double)v.w;
        }
        if (grad) {
            float* out = grad + ((int64_t)b * a.n[S] + a.idx[S][k]) * 3;
            out[0] = (float)(g[0] * inv);
            out[1] = (float)(g[1] * inv);
            out[2] = (float)(g[2] * inv);
        }
    }
    if (S == 0) {  // block-uniform
        double s[1] = {g[3]};
        block4_sum(s, red);
        if (t == 0) blockval[(int64_t)b * fb_o + blockIdx.x] = s[0];
    }
}

// one wave per pose: the block sums of the compacted object vertices
__global__ __launch_bounds__(64) void pair_value_kernel(const PairHeader* __restrict__ hdr, const double* __restrict__ blockval, int fb_o,
                                                        float* __restrict__ value) {
    const int b = blockIdx.x;
    const int nb = (hdr->m[0] + kFold - 1) / kFold;
    double s[1];
    wave_fold(blockval + (int64_t)b * fb_o, nb, s);
    if (threadIdx.x == 0) value[b] = (float)(s[0] / (hdr->sum[0] * hdr->sum[1]));
}

}  // namespace

size_t contact_pair_workspace_bytes(int B, int n_o, int n_h) {
    if (B <= 0 || n_o <= 0 || n_h <= 0 || n_o > kMaxN || n_h > kMaxN) return 0;
    return pair_layout(B, n_o, n_h).total;
}

int contact_pair(const float* o, const float* h, const void* p, const void* q, int p_dtype, int B, int n_o, int n_h,
                 int64_t o_bstride, int64_t h_bstride, float* value, float* grad_o, float* grad_h, void* ws, size_t ws_bytes,
                 hipStream_t st) {
    if (!o || !h || !p || !q || !value || !ws || B <= 0 || n_o <= 0 || n_h <= 0 || o_bstride < 0 || h_bstride < 0)
        return IVLM_ERR_INVALID_ARG;
    if ((p_dtype != IVLM_F32 && p_dtype != IVLM_BF16) || n_o > kMaxN || n_h > kMaxN || B > 65535) return IVLM_ERR_UNSUPPORTED;
    const PairLayout l = pair_layout(B, n_o, n_h);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    PairHeader* hdr = ws_at<PairHeader>(ws, l.hdr);
    int32_t* idx[2] = {ws_at<int32_t>(ws, l.idx[0]), ws_at<int32_t>(ws, l.idx[1])};
    float* wt[2] = {ws_at<float>(ws, l.wt[0]), ws_at<float>(ws, l.wt[1])};
    double* blockval = ws_at<double>(ws, l.blockval);
    PairArgs a;
    a.verts[0] = o;
    a.verts[1] = h;
    a.bstride[0] = o_bstride;
    a.bstride[1] = h_bstride;
    a.hdr = hdr;
    a.n[0] = n_o;
    a.n[1] = n_h;
    for (int s = 0; s < 2; ++s) {
        a.idx[s] = idx[s];
        a.wt[s] = wt[s];
        a.part[s] = ws_at<float4>(ws, l.part[s]);
        a.cb[s] = l.cb[s];
        a.sb[s] = l.sb[s];
    }
    a.role_blocks0 = l.sb[0] * l.cb[1];
    a.grad_o = grad_o != nullptr;
    const int role_blocks1 = grad_h ? l.sb[1] * l.cb[0] : 0;

    if (grad_o) IVLM_HIP_TRY(hipMemsetAsync(grad_o, 0, (size_t)B * n_o * 12, st));
    if (grad_h) IVLM_HIP_TRY(hipMemsetAsync(grad_h, 0, (size_t)B * n_h * 12, st));
    if (p_dtype == IVLM_BF16) pair_compact_kernel<true><<<2, 1024, 0, st>>>(p, q, n_o, n_h, hdr, idx[0], wt[0], idx[1], wt[1]);
    else pair_compact_kernel<false><<<2, 1024, 0, st>>>(p, q, n_o, n_h, hdr, idx[0], wt[0], idx[1], wt[1]);
    pair_sweep_kernel<<<dim3(a.role_blocks0 + role_blocks1, B), kThreads, 0, st>>>(a);
    const int fb_h = grad_h ? (n_h + kFold - 1) / kFold : 0;
    pair_fold_kernel<<<dim3(l.fb + fb_h, B), kFold, 0, st>>>(a, l.fb, grad_o, grad_h, blockval);
    pair_value_kernel<<<B, 64, 0, st>>>(hdr, blockval, l.fb, value);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_contact_pair_workspace_bytes(int B, int N_o, int N_h) { return ivlm::contact_pair_workspace_bytes(B, N_o, N_h); }
int ivlm_contact_pair(const float* o, const float* h, const void* p, const void* q, int p_dtype, int B, int N_o, int N_h,
                      int64_t o_batch_stride, int64_t h_batch_stride, float* value_out, float* grad_o, float* grad_h,
                      void* workspace, size_t workspace_bytes, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::contact_pair(o, h, p, q, p_dtype, B, N_o, N_h, o_batch_stride, h_batch_stride, value_out, grad_o, grad_h, workspace,
                              workspace_bytes, ivlm_stream(s));
}
}
