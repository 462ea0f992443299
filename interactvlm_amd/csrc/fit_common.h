// What the files of the object-pose fit (contact_pair.hip, contact_icp.hip, pose.hip, mesh_sdf.hip, fit_step.hip, fit_start.hip, and
// through screen_common.h silhouette.hip and depth_order.hip) share: on the host the workspace carve, its check and the typed pointer
// into it; on the device the fixed-order fp64 folds and the ordered compaction that "the same bits every call, for a pose whatever the
// batch" rests on (DESIGN 4.44 lists the orders).
// Every device function is inlined into its kernel and holds only integer and fp64 additions - no fp32 multiply-add that
// -ffp-contract could fuse - so it is the same arithmetic in the files built with -ffp-contract=off and in those built without.
// A sum that adds in another order than these stays written out in its kernel, with a comment that says so.
#pragma once
#include "kernels.h"

namespace ivlm {

// ---- host: the workspace ------------------------------------------------------------------------------------------------------
// offsets in bytes, every region 256-byte aligned; off = the bytes carved so far
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

// the caller's workspace holds `needed` bytes and starts on a multiple of `align` (a power of two)
inline bool workspace_ok(const void* ws, size_t held, size_t needed, uintptr_t align) {
    return held >= needed && !(reinterpret_cast<uintptr_t>(ws) & (align - 1));
}

template <typename T>
inline T* ws_at(void* ws, size_t off) {
    return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// ---- device: fp64 sums in a fixed order ------------------------------------------------------------------------------------------
// (wave_sum(double) is in ivlm_common.h: the xor butterfly of offsets 32, 16, .. 1, every lane gets the sum)

// The sum of v[k] over a block of 256 threads = four waves, for K values at once: the butterfly per wave, one LDS slot per wave and
// value, one barrier, then (wave 0 + wave 1) + (wave 2 + wave 3).  Every thread calls it and gets the sums in v.
template <int K>
__device__ __forceinline__ void block4_sum(double (&v)[K], double (&red)[4][K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// One wave (a block of 64 threads) folds n partials of K values each, part[j * K + k]: lane l adds j = l, l + 64, .. in ascending
// order from 0.0, then the butterfly.  Every lane gets the sums in s.
template <int K>
__device__ __forceinline__ void wave_fold(const double* __restrict__ part, int n, double (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int j = threadIdx.x; j < n; j += 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += part[(int64_t)j * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
}

// ---- device: ordered compaction ---------------------------------------------------------------------------------------------------
// One block of 1024 threads keeps, of k = 0 .. n - 1, those with keep(k), in index order: thread t owns the segment
// [t seg, (t + 1) seg) with seg = ceil(n / 1024), counts its kept entries, an inclusive Hillis-Steele scan of the counts in LDS
// (cnt[1024]) gives its first slot, and a second pass over the segment calls emit(slot, k) with slot = the number of kept entries
// before k.  keep must give the same answer in both passes.  -> the number kept, in every thread.  The list is a function of the
// kept entries alone.  emit's stores are not fenced here: the caller synchronises before the block reads them.
template <typename Keep, typename Emit>
__device__ __forceinline__ int block_compact(int n, int32_t* cnt, Keep keep, Emit emit) {
    const int t = threadIdx.x;
    const int seg = (n + 1023) / 1024;
    const int k0 = min(t * seg, n), k1 = min(k0 + seg, n);
    int c = 0;
    for (int k = k0; k < k1; ++k) c += keep(k) ? 1 : 0;
    cnt[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? cnt[t - off] : 0;
        __syncthreads();
        cnt[t] += v;
        __syncthreads();
    }
    int slot = cnt[t] - c;
    for (int k = k0; k < k1; ++k) {
        if (keep(k)) emit(slot++, k);
    }
    return cnt[1023];
}

}  // namespace ivlm
