// Host side of the tile GEMM family (gemm.hip, gemm256.hip, gemm320.hip): what a call is routed to, which kernels the build holds,
// and the one dispatch from a route to its kernel instantiation.
#pragma once
#include "kernels.h"

namespace ivlm {

// the benchmark / test switches of the GEMM dispatch (set by the hooks of ivlm_hip.h; not meant to change while GEMMs are in flight)
struct GemmSwitches {
    int tile_override = 0;  // ivlm_gemm_tile_override: a tile code for every call that sets no GemmArgs::tile of its own; 0 = automatic
    int tile320 = 1;        // ivlm_gemm_tile320: 0 = never pick the 256 x 320 tile automatically
    int nsplit = 1;         // ivlm_gemm_nsplit: 0 = never split N
    int skinny_min_m = 0;   // ivlm_gemv_mfma_min_m: > 0 = every M in [min_m, 16] with K, N >= 1024 takes the skinny MFMA kernel
};

enum GemmFamily : int { GEMM_TILE = 0, GEMM_256P = 1, GEMM_320 = 2 };  // gemm.hip | 8-phase 256 x 256 (gemm256.hip) | 256 x 320 (gemm320.hip)

// One launch of the family: the kernel instantiation <act, out_f32, (bm x bn), opk> of `family`, its grid and dynamic LDS bytes
struct GemmRoute {
    int rc = IVLM_OK;  // != IVLM_OK: the call is rejected with this code (nothing else is set)
    int family = GEMM_TILE, bm = 128, bn = 128;
    int opk = 0;       // operand kind: 0 bf16, 1 e4m3, 2 IEEE fp16
    int out_f32 = 0;   // the kernel's epilogue arithmetic / store: fp32 (also the split outputs) or 16-bit
    int act = ACT_NONE;
    int grid_x = 0, grid_z = 1, lds = 0;
};
constexpr int kGemm256LdsBytes = 128 * 1024, kGemm320LdsBytes = 144 * 1024;  // two K tiles of gemm256.hip / gemm320.hip
// Pure host logic: validated arguments + switches -> route.  A forced tile is GemmArgs::tile (the column split and the fused split-K
// path set it), else the switch, else the automatic choice.
GemmRoute gemm_route(const GemmArgs& g, const GemmSwitches& sw);

// fp16 / fp8 operands: the epilogues the three towers use (SAM encoder, CLIP, LLaMA prefill) - keeps the build small
constexpr bool gemm_tower_act(int act) { return act == ACT_NONE || act == ACT_GELU || act == ACT_QUICK_GELU || act == ACT_SWIGLU; }

// The kernels the build holds.  gemm_route names no other, the launchers compile no other.
constexpr bool gemm_instantiated(int family, int bm, int bn, int opk, int act) {
    if (act < ACT_NONE || act > ACT_SIGMOID || (opk != 0 && !gemm_tower_act(act))) return false;
    if (family == GEMM_256P) return bm == 256 && bn == 256;
    if (family == GEMM_320) return bm == 256 && bn == 320 && opk != 1 && (act == ACT_NONE || act == ACT_GELU);  // (the SAM encoder's)
    if (bm == 176 && bn == 128) return opk != 1 && (act == ACT_NONE || act == ACT_SWIGLU);  // (the epilogues the prefill uses)
    if ((bm == 256 && bn == 256) || (bm == 128 && bn == 96)) return opk == 0;
    return bm == 128 && (bn == 128 || bn == 64);
}

// The one activation / operand-kind dispatch: go.run<ACT, OPK>() for the instantiation the route names
template <int ACT, class Go>
int gemm_dispatch_opk(const GemmRoute& r, const Go& go) {
    switch (r.opk) {
        case 0: return go.template run<ACT, 0>();
        case 1: return go.template run<ACT, 1>();
        default: return go.template run<ACT, 2>();
    }
}
template <class Go>
int gemm_dispatch(const GemmRoute& r, const Go& go) {
    switch (r.act) {
        case ACT_NONE: return gemm_dispatch_opk<ACT_NONE>(r, go);
        case ACT_GELU: return gemm_dispatch_opk<ACT_GELU>(r, go);
        case ACT_QUICK_GELU: return gemm_dispatch_opk<ACT_QUICK_GELU>(r, go);
        case ACT_RELU: return gemm_dispatch_opk<ACT_RELU>(r, go);
        case ACT_SILU: return gemm_dispatch_opk<ACT_SILU>(r, go);
        case ACT_SWIGLU: return gemm_dispatch_opk<ACT_SWIGLU>(r, go);
        case ACT_SIGMOID: return gemm_dispatch_opk<ACT_SIGMOID>(r, go);
        default: return IVLM_ERR_INVALID_ARG;
    }
}

// ... and the launch of that instantiation (KF32 / K16: its fp32- and 16-bit-output kernels), its dynamic-LDS cap raised to what the
// route asks for on the first launch on each device
template <auto KF32, auto K16>
int gemm_launch(const GemmRoute& r, int threads, const GemmArgs& g, hipStream_t st) {
    const dim3 grid(r.grid_x, 1, r.grid_z), block(threads);
    if (r.out_f32) ivlm_launch_lds_cap<KF32>(r.lds, grid, block, r.lds, st, g);
    else ivlm_launch_lds_cap<K16>(r.lds, grid, block, r.lds, st, g);
    return ivlm_launch_status();
}

// the launchers of gemm256.hip / gemm320.hip (a route of their family)
int gemm256_launch(const GemmRoute& r, const GemmArgs& g, hipStream_t st);
int gemm320_launch(const GemmRoute& r, const GemmArgs& g, hipStream_t st);

}  // namespace ivlm
