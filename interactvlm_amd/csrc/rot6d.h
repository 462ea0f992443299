// The rot6d parameterisation of the object-pose fit, once: the Gram-Schmidt that makes R of the six numbers and the chain that takes
// dL/dR back to them, both in fp64 (pose.hip's transform and mesh_sdf.hip's intrusion term include this; pose.py's
// gram_schmidt_backward is the same chain in torch, as documentation).
//
//   a1, a2 = the two interleaved columns of rot6d;  b1 = a1 / max(|a1|, 1e-12);  u2 = a2 - (b1.a2) b1;  b2 = u2 / max(|u2|, 1e-12)
//   b3 = b1 x b2;  R = [b1 b2 b3] (columns)
//
// The functions hold fp64 multiply-adds, which -ffp-contract may fuse: a file built with -ffp-contract=off (mesh_sdf.hip) and one
// built without (pose.hip) get the same R within fp64 rounding, NOT the same bits in every case.  Nothing promises that they do.
#pragma once
#include <cmath>

namespace ivlm {

constexpr double kRot6dEps = 1e-12;  // F.normalize's clamp of the norm

struct Frame {
    double b1[3], b2[3], b3[3];  // the columns of R
    double a2[3], d, n1, n2;     // what the chain back to the six numbers needs
    bool clamp1, clamp2;         // the norm was clamped: the normalisation is a division by the constant
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ Frame gram_schmidt(const float* __restrict__ r6) {
    Frame f;
    double a1[3], u2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a1[i] = (double)r6[2 * i];
        f.a2[i] = (double)r6[2 * i + 1];
    }
    const double l1 = sqrt(dot3(a1, a1));
    f.clamp1 = !(l1 > kRot6dEps);
    f.n1 = f.clamp1 ? kRot6dEps : l1;
#pragma unroll
    for (int i = 0; i < 3; ++i) f.b1[i] = a1[i] / f.n1;
    f.d = dot3(f.b1, f.a2);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = f.a2[i] - f.d * f.b1[i];
    const double l2 = sqrt(dot3(u2, u2));
    f.clamp2 = !(l2 > kRot6dEps);
    f.n2 = f.clamp2 ? kRot6dEps : l2;
#pragma unroll
    for (int i = 0; i < 3; ++i) f.b2[i] = u2[i] / f.n2;
    cross3(f.b1, f.b2, f.b3);
    return f;
}

// dL/dR by columns (gb1, gb2, gb3; overwritten) -> dL/da1, dL/da2
__device__ __forceinline__ void gram_schmidt_backward(const Frame& f, double* gb1, double* gb2, const double* gb3, double* ga1, double* ga2) {
    double c[3], gu2[3];
    // b3 = b1 x b2
    cross3(f.b2, gb3, c);
#pragma unroll
    for (int i = 0; i < 3; ++i) gb1[i] += c[i];
    cross3(gb3, f.b1, c);
#pragma unroll
    for (int i = 0; i < 3; ++i) gb2[i] += c[i];
    // b2 = u2 / n2
    const double p2 = f.clamp2 ? 0.0 : dot3(f.b2, gb2);
#pragma unroll
    for (int i = 0; i < 3; ++i) gu2[i] = (gb2[i] - f.b2[i] * p2) / f.n2;
    // u2 = a2 - d b1,  d = b1 . a2
    const double gd = -dot3(f.b1, gu2);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gb1[i] += gd * f.a2[i] - f.d * gu2[i];
        ga2[i] = gu2[i] + gd * f.b1[i];
    }
    // b1 = a1 / n1
    const double p1 = f.clamp1 ? 0.0 : dot3(f.b1, gb1);
#pragma unroll
    for (int i = 0; i < 3; ++i) ga1[i] = (gb1[i] - f.b1[i] * p1) / f.n1;
}

}  // namespace ivlm
