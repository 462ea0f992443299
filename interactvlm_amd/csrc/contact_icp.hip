// Batched ICP between the object's and the human's contact points (the reference's optim/icp/icp.py `ICP` and
// `corresponding_points_alignment`, and the `filter_contacts` step of optim/fit.py), without any [N_o, N_h] array and without
// a host round trip inside the loop.  Row-vector convention as in the reference: s x R + T ~ y.
//
//   icp_nn_moments  grid (ceil(N_o / 256), B).  A block keeps kStat = 256 object points in registers (kRows = 2 per thread), forms
//                   their queries q_i = [s x_i R + T, n_i R] from pose b's fp64 transform (rounded once to fp32) and sweeps the
//                   targets t_j = [y_j, sign m_j] in LDS tiles of kTile = 512, each target two float4 read by all lanes at one
//                   address (a broadcast ds_read_b128).  d^2 is the direct sum of squared differences in fp32; (best d^2, best j)
//                   is kept with a strict < over ascending j, so the lowest index wins an exact tie whatever the tiling.  Then
//                   each thread fetches its neighbours and forms the weighted moments in fp64 from the fp32 coordinates - of the
//                   ORIGINAL object point x, as the reference aligns obj_init - and the block reduces them in a fixed order
//                   (wave_sum, then wave 0 + wave 1) into one fp64 partial of kMom values.  A second entry mode takes the
//                   correspondences as given and skips the sweep (points_align); a third stops after the sweep (contact_nearest).
//   icp_solve       one wave per pose: the block partials folded in block order in fp64, then one lane forms the centroids and
//                   the covariance exactly as the reference does,
//                       mu_x = sum w x / max(sum w, 1e-9),  Xc = w (x - mu_x),  Yc = w (y - mu_y)   (so the covariance carries w^2)
//                       C = Xc^T Yc / max(sum w, 1e-9) = U S V^T,  E = diag(1, 1, det(U V^T)) unless reflections are allowed
//                       R = U E V^T,  s = trace(E S) / max(sum |Xc|^2 / max(sum w, 1e-9), 1e-9) or 1,  T = mu_y - s mu_x R
//                   with the 3x3 SVD by one-sided Jacobi in fp64 (null directions completed to an orthonormal basis, so a
//                   degenerate covariance still gives an orthonormal R of determinant +1), the rmse
//                       sqrt(sum w |s x R + T - y|^2 / max(sum w, 1e-9))
//                   in closed form from the moments, the per-pose convergence flag, the fp64 transform of the next iteration, one
//                   row of the fp32 history and iterations[b].
//   normal_filter   the same stationary-versus-tile sweep in 3-D: per object normal the max and the min over the human normals of
//                   dot(o_i / |o_i|, -h_j / |h_j|); keep_i = (max > c_pos) or (min < c_neg).
//
// No atomics, every sum in a fixed order: the same bits every call, and a pose's bits do not depend on the batch around it.  The
// moments are taken about the first point of each side (x_0, y_0), which changes nothing in exact arithmetic and keeps the
// cancellation of the closed forms relative to the clouds' extent and not to their distance from the origin.
#include <cfloat>
#include <cmath>

#include "fit_common.h"

namespace ivlm {
namespace {

constexpr int kTile = 512;   // swept targets per LDS tile
constexpr int kThreads = 128;
constexpr int kRows = 2;     // stationary points per thread
constexpr int kStat = kThreads * kRows;
constexpr int kMaxN = 1 << 20;
constexpr double kEps = 1e-9;  // the reference's clamp of sum w and of Xcov

// moment slots of one partial: sums with weight w (0..17) and with weight w^2 (18..34)
enum { M_W = 0, M_X = 1, M_Y = 4, M_XY = 7, M_XX = 16, M_YY = 17, M2_W = 18, M2_X = 19, M2_Y = 22, M2_XY = 25, M2_XX = 34, kMom = 36 };
constexpr int kXf = 13;  // a transform in the workspace: R (9, row-major), T (3), s

enum { F_SCALE = 1, F_REFLECT = 2, F_REQUERY = 4 };

struct IcpArgs {
    const float* x;    // stationary points: row stride x_rs, pose stride x_bs (0 = shared by the batch)
    const float* xn;   // their normals (NULL: 3-D queries)
    const float* y;    // targets
    const float* yn;   // their normals, multiplied by yn_sign in the target
    const float* w;    // weights [B or 1, N_o] (NULL: 1)
    const float* yg;   // correspondences as given [B or 1, N_o, 3] (NULL: sweep)
    const double* xf;  // [B, kXf] current transforms (NULL: queries as given)
    const int32_t* done;  // [B] (NULL: every pose runs)
    int64_t x_bs, xn_bs, y_bs, yn_bs, w_bs, yg_bs;
    int x_rs, xn_rs, y_rs, yn_rs;
    float yn_sign;
    int rotate_normals;
    int n_o, n_h, nblk;
    int32_t* nn_idx;   // [B, N_o]
    float* nn_d2;      // [B, N_o] (may be NULL)
    double* part;      // [B, nblk, kMom] (NULL: no moments)
};

template <bool D6>
__global__ __launch_bounds__(kThreads) void icp_nn_moments_kernel(IcpArgs a) {
    __shared__ float4 tile[D6 ? 2 * kTile : kTile];
    __shared__ double red[kMom];
    const int b = blockIdx.y, t = threadIdx.x;
    if (a.done && a.done[b]) return;  // block-uniform
    const float* xb = a.x + (int64_t)b * a.x_bs;
    int best_j[kRows];
    float best_d[kRows];
    if (!a.yg) {
        double xf[kXf];
        if (a.xf) {
#pragma unroll
            for (int k = 0; k < kXf; ++k) xf[k] = a.xf[(int64_t)b * kXf + k];
        }
        float q[kRows][6];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int i = blockIdx.x * kStat + r * kThreads + t;
#pragma unroll
            for (int c = 0; c < 6; ++c) q[r][c] = 0.0f;
            if (i < a.n_o) {
                const float* p = xb + (int64_t)i * a.x_rs;
                const float px = p[0], py = p[1], pz = p[2];
                if (a.xf) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        q[r][c] = (float)(xf[12] * ((double)px * xf[c] + (double)py * xf[3 + c] + (double)pz * xf[6 + c]) + xf[9 + c]);
                } else {
                    q[r][0] = px;
                    q[r][1] = py;
                    q[r][2] = pz;
                }
                if constexpr (D6) {
                    const float* n = a.xn + (int64_t)b * a.xn_bs + (int64_t)i * a.xn_rs;
                    const float nx = n[0], ny = n[1], nz = n[2];
                    if (a.xf && a.rotate_normals) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) q[r][3 + c] = (float)((double)nx * xf[c] + (double)ny * xf[3 + c] + (double)nz * xf[6 + c]);
                    } else {
                        q[r][3] = nx;
                        q[r][4] = ny;
                        q[r][5] = nz;
                    }
                }
            }
            best_j[r] = 0;
            best_d[r] = INFINITY;
        }
        const float* yb = a.y + (int64_t)b * a.y_bs;
        const float* ynb = D6 ? a.yn + (int64_t)b * a.yn_bs : nullptr;
        for (int j0 = 0; j0 < a.n_h; j0 += kTile) {
            const int count = min(kTile, a.n_h - j0);
            __syncthreads();  // the previous tile has been read
            for (int j = t; j < count; j += kThreads) {
                const float* p = yb + (int64_t)(j0 + j) * a.y_rs;
                if constexpr (D6) {
                    const float* n = ynb + (int64_t)(j0 + j) * a.yn_rs;
                    tile[2 * j] = make_float4(p[0], p[1], p[2], a.yn_sign * n[0]);
                    tile[2 * j + 1] = make_float4(a.yn_sign * n[1], a.yn_sign * n[2], 0.0f, 0.0f);
                } else {
                    tile[j] = make_float4(p[0], p[1], p[2], 0.0f);
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < count; ++j) {
                const float4 e0 = tile[D6 ? 2 * j : j];
                float4 e1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (D6) e1 = tile[2 * j + 1];
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    const float dx = q[r][0] - e0.x, dy = q[r][1] - e0.y, dz = q[r][2] - e0.z;
                    float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    if constexpr (D6) {
                        const float da = q[r][3] - e0.w, db = q[r][4] - e1.x, dc = q[r][5] - e1.y;
                        d2 = fmaf(dc, dc, fmaf(db, db, fmaf(da, da, d2)));
                    }
                    if (d2 < best_d[r]) {  // strict: the lowest index wins a tie
                        best_d[r] = d2;
                        best_j[r] = j0 + j;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int i = blockIdx.x * kStat + r * kThreads + t;
            if (i < a.n_o) {
                a.nn_idx[(int64_t)b * a.n_o + i] = best_j[r];
                if (a.nn_d2) a.nn_d2[(int64_t)b * a.n_o + i] = best_d[r];
            }
        }
    }
    if (!a.part) return;

    // the weighted moments of (x_i, y_nn(i)) about (x_0, y_0), fp64 from the fp32 coordinates
    const float* ysrc = a.yg ? a.yg + (int64_t)b * a.yg_bs : a.y + (int64_t)b * a.y_bs;
    const int y_rs = a.yg ? 3 : a.y_rs;
    const double cx[3] = {(double)xb[0], (double)xb[1], (double)xb[2]};
    const double cy[3] = {(double)ysrc[0], (double)ysrc[1], (double)ysrc[2]};
    double m[kMom];
#pragma unroll
    for (int k = 0; k < kMom; ++k) m[k] = 0.0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int i = blockIdx.x * kStat + r * kThreads + t;
        if (i < a.n_o) {
            const float* p = xb + (int64_t)i * a.x_rs;
            const float* v = ysrc + (int64_t)(a.yg ? i : best_j[r]) * y_rs;
            const double w = a.w ? (double)a.w[(int64_t)b * a.w_bs + i] : 1.0;
            const double w2 = w * w;
            const double xs[3] = {(double)p[0] - cx[0], (double)p[1] - cx[1], (double)p[2] - cx[2]};
            const double ys[3] = {(double)v[0] - cy[0], (double)v[1] - cy[1], (double)v[2] - cy[2]};
            const double xx = xs[0] * xs[0] + xs[1] * xs[1] + xs[2] * xs[2];
            const double yy = ys[0] * ys[0] + ys[1] * ys[1] + ys[2] * ys[2];
            m[M_W] += w;
            m[M2_W] += w2;
            m[M_XX] += w * xx;
            m[M_YY] += w * yy;
            m[M2_XX] += w2 * xx;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                m[M_X + c] += w * xs[c];
                m[M_Y + c] += w * ys[c];
                m[M2_X + c] += w2 * xs[c];
                m[M2_Y + c] += w2 * ys[c];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    m[M_XY + 3 * c + d] += w * xs[c] * ys[d];
                    m[M2_XY + 3 * c + d] += w2 * xs[c] * ys[d];
                }
            }
        }
    }
    // NOT block4_sum's order: two waves, wave 0 + wave 1 - only the butterfly is the shared one
#pragma unroll
    for (int k = 0; k < kMom; ++k) m[k] = wave_sum(m[k]);
    if (t == 64) {
#pragma unroll
        for (int k = 0; k < kMom; ++k) red[k] = m[k];
    }
    __syncthreads();
    if (t == 0) {
        double* out = a.part + ((int64_t)b * a.nblk + blockIdx.x) * kMom;
#pragma unroll
        for (int k = 0; k < kMom; ++k) out[k] = m[k] + red[k];
    }
}

__device__ __forceinline__ double det3(const double* A) {
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// A (row-major 3x3) = U diag(S) V^T with S descending, U and V orthonormal whatever the rank of A (one-sided Jacobi on the columns)
__device__ void svd3(const double* A, double* U, double* S, double* V) {
    double G[9], W[9];
    for (int k = 0; k < 9; ++k) {
        G[k] = A[k];
        W[k] = (k % 4 == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; ++r) {
                    al += G[3 * r + p] * G[3 * r + p];
                    be += G[3 * r + q] * G[3 * r + q];
                    ga += G[3 * r + p] * G[3 * r + q];
                }
                if (ga == 0.0 || fabs(ga) <= 1e-16 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
                for (int r = 0; r < 3; ++r) {
                    const double gp = G[3 * r + p], gq = G[3 * r + q];
                    G[3 * r + p] = c * gp - s * gq;
                    G[3 * r + q] = s * gp + c * gq;
                    const double wp = W[3 * r + p], wq = W[3 * r + q];
                    W[3 * r + p] = c * wp - s * wq;
                    W[3 * r + q] = s * wp + c * wq;
                }
            }
        if (!rotated) break;
    }
    double sv[3];
    int ord[3] = {0, 1, 2};
    for (int k = 0; k < 3; ++k) sv[k] = sqrt(G[k] * G[k] + G[3 + k] * G[3 + k] + G[6 + k] * G[6 + k]);
    for (int i = 0; i < 2; ++i)  // descending, stable
        for (int j = 0; j < 2 - i; ++j)
            if (sv[ord[j]] < sv[ord[j + 1]]) {
                const int tmp = ord[j];
                ord[j] = ord[j + 1];
                ord[j + 1] = tmp;
            }
    int rank = 0;
    for (int k = 0; k < 3; ++k) {
        const int c = ord[k];
        S[k] = sv[c];
        for (int r = 0; r < 3; ++r) V[3 * r + k] = W[3 * r + c];
        // a direction below 1e-14 of the largest is null to fp64: its column of U comes from the completion below
        if (sv[c] > 0.0 && sv[c] >= 1e-14 * sv[ord[0]] && sv[c] >= DBL_MIN * 1e16 && rank == k) {
            for (int r = 0; r < 3; ++r) U[3 * r + k] = G[3 * r + c] / sv[c];
            rank = k + 1;
        }
    }
    if (rank == 0) {
        for (int k = 0; k < 9; ++k) U[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    if (rank == 1) {  // u1: a unit vector orthogonal to u0, built from the axis u0 is least aligned with
        const double a0 = fabs(U[0]), a1 = fabs(U[3]), a2 = fabs(U[6]);
        const int ax = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
        double e[3] = {0.0, 0.0, 0.0};
        e[ax] = 1.0;
        const double d = U[3 * ax];
        double v[3], nv = 0.0;
        for (int r = 0; r < 3; ++r) {
            v[r] = e[r] - d * U[3 * r];
            nv += v[r] * v[r];
        }
        nv = sqrt(nv);
        for (int r = 0; r < 3; ++r) U[3 * r + 1] = v[r] / nv;
    }
    if (rank <= 2) {  // u2 = u0 x u1
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

struct SolveArgs {
    const double* part;   // [B, nblk, kMom]
    const float* x;       // the first points of both sides: the origin of the moments
    const float* y;
    int64_t x_bs, y_bs;
    int nblk, flags, it, rows;  // this launch writes history rows it .. it + rows - 1
    int B;
    double thr;
    double* xf;           // [B, kXf] (NULL: not kept)
    double* prev;         // [B] rmse of the previous iteration
    int32_t* done;        // [B]
    float *R, *T, *s, *rmse;          // [B, ...] results (rmse may be NULL)
    int32_t *converged, *iterations;  // [B] (NULL: not a loop)
    float *hR, *hT, *hs;              // [rows_total, B, ...] history (NULL: none)
};

__global__ __launch_bounds__(64) void icp_solve_kernel(SolveArgs a) {
    __shared__ double mom[kMom];
    const int b = blockIdx.x, t = threadIdx.x;
    const bool was_done = a.done && a.it > 0 && a.done[b];
    if (!was_done && t < kMom) {
        double s = 0.0;
        for (int j = 0; j < a.nblk; ++j) s += a.part[((int64_t)b * a.nblk + j) * kMom + t];
        mom[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    double xf[kXf];
    if (was_done) {
        for (int k = 0; k < kXf; ++k) xf[k] = a.xf[(int64_t)b * kXf + k];
    } else {
        const double* m = mom;
        const double W = fmax(m[M_W], kEps);
        double mx[3], my[3], C[9];
        for (int c = 0; c < 3; ++c) {
            mx[c] = m[M_X + c] / W;
            my[c] = m[M_Y + c] / W;
        }
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d)
                C[3 * c + d] = (m[M2_XY + 3 * c + d] - mx[c] * m[M2_Y + d] - m[M2_X + c] * my[d] + m[M2_W] * mx[c] * my[d]) / W;
        double U[9], S[3], V[9], E2 = 1.0;
        svd3(C, U, S, V);
        if (!(a.flags & F_REFLECT)) E2 = det3(U) * det3(V) >= 0.0 ? 1.0 : -1.0;
        double* R = xf;
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) R[3 * c + d] = U[3 * c] * V[3 * d] + U[3 * c + 1] * V[3 * d + 1] + E2 * U[3 * c + 2] * V[3 * d + 2];
        double s = 1.0;
        if (a.flags & F_SCALE) {
            const double xcov = (m[M2_XX] - 2.0 * (mx[0] * m[M2_X] + mx[1] * m[M2_X + 1] + mx[2] * m[M2_X + 2]) +
                                 m[M2_W] * (mx[0] * mx[0] + mx[1] * mx[1] + mx[2] * mx[2])) / W;
            s = (S[0] + S[1] + E2 * S[2]) / fmax(xcov, kEps);
        }
        // T' = mu_y' - s mu_x' R about the origins (x_0, y_0); T = T' + y_0 - s x_0 R
        const float* x0 = a.x + (int64_t)b * a.x_bs;
        const float* y0 = a.y + (int64_t)b * a.y_bs;
        double Tp[3], sxR[3];
        for (int d = 0; d < 3; ++d) {
            Tp[d] = my[d] - s * (mx[0] * R[d] + mx[1] * R[3 + d] + mx[2] * R[6 + d]);
            xf[9 + d] = Tp[d] + (double)y0[d] - s * ((double)x0[0] * R[d] + (double)x0[1] * R[3 + d] + (double)x0[2] * R[6 + d]);
            sxR[d] = m[M_X] * R[d] + m[M_X + 1] * R[3 + d] + m[M_X + 2] * R[6 + d];
        }
        xf[12] = s;
        double rm = 0.0;
        for (int k = 0; k < 9; ++k) rm += R[k] * m[M_XY + k];
        double e = s * s * m[M_XX] + m[M_W] * (Tp[0] * Tp[0] + Tp[1] * Tp[1] + Tp[2] * Tp[2]) + m[M_YY] - 2.0 * s * rm;
        for (int d = 0; d < 3; ++d) e += 2.0 * Tp[d] * (s * sxR[d] - m[M_Y + d]);
        const double rmse = sqrt(fmax(e, 0.0) / W);
        if (a.xf)
            for (int k = 0; k < kXf; ++k) a.xf[(int64_t)b * kXf + k] = xf[k];
        for (int k = 0; k < 9; ++k) a.R[(int64_t)b * 9 + k] = (float)xf[k];
        for (int k = 0; k < 3; ++k) a.T[(int64_t)b * 3 + k] = (float)xf[9 + k];
        a.s[b] = (float)s;
        if (a.rmse) a.rmse[b] = (float)rmse;
        if (a.converged) {
            if (a.flags & F_REQUERY) {
                // pytorch3d's criterion on the position rmse; the first iteration has nothing to compare with
                const double rel = a.it > 0 ? (a.prev[b] - rmse) / a.prev[b] : 1.0;
                const int conv = rel <= a.thr || rmse == 0.0;
                a.prev[b] = rmse;
                a.done[b] = conv;
                a.converged[b] = conv;
                a.iterations[b] = a.it + 1;
            } else {
                // the reference's loop: its query never changes, so its second iteration repeats the first and "converges"
                a.converged[b] = a.rows >= 2;
                a.iterations[b] = a.rows < 2 ? a.rows : 2;
            }
        }
    }
    if (a.hR)
        for (int row = a.it; row < a.it + a.rows; ++row) {
            const int64_t o = (int64_t)row * a.B + b;
            for (int k = 0; k < 9; ++k) a.hR[o * 9 + k] = (float)xf[k];
            for (int k = 0; k < 3; ++k) a.hT[o * 3 + k] = (float)xf[9 + k];
            a.hs[o] = (float)xf[12];
        }
}

// [B, kXf] fp64 transforms from the caller's fp32 (R, T, s); NULL parts are the identity
__global__ void icp_init_kernel(const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ s, int B,
                                double* __restrict__ xf, int32_t* __restrict__ done) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    for (int k = 0; k < 9; ++k) xf[(int64_t)b * kXf + k] = R ? (double)R[(int64_t)b * 9 + k] : (k % 4 == 0 ? 1.0 : 0.0);
    for (int k = 0; k < 3; ++k) xf[(int64_t)b * kXf + 9 + k] = T ? (double)T[(int64_t)b * 3 + k] : 0.0;
    xf[(int64_t)b * kXf + 12] = s ? (double)s[b] : 1.0;
    done[b] = 0;
}

__global__ __launch_bounds__(kThreads) void normal_filter_kernel(const float* __restrict__ on, const float* __restrict__ hn, int n_o,
                                                                 int n_h, float c_pos, float c_neg, int has_neg,
                                                                 uint8_t* __restrict__ keep) {
    __shared__ float4 tile[kTile];
    const int t = threadIdx.x;
    float q[kRows][3], mx[kRows], mn[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int i = blockIdx.x * kStat + r * kThreads + t;
        q[r][0] = q[r][1] = q[r][2] = 0.0f;
        if (i < n_o) {
            const float* p = on + (int64_t)i * 3;
            const float inv = 1.0f / fmaxf(sqrtf(fmaf(p[2], p[2], fmaf(p[1], p[1], p[0] * p[0]))), 1e-12f);
            q[r][0] = p[0] * inv;
            q[r][1] = p[1] * inv;
            q[r][2] = p[2] * inv;
        }
        mx[r] = -INFINITY;
        mn[r] = INFINITY;
    }
    for (int j0 = 0; j0 < n_h; j0 += kTile) {
        const int count = min(kTile, n_h - j0);
        __syncthreads();
        for (int j = t; j < count; j += kThreads) {
            const float* p = hn + (int64_t)(j0 + j) * 3;
            const float inv = -1.0f / fmaxf(sqrtf(fmaf(p[2], p[2], fmaf(p[1], p[1], p[0] * p[0]))), 1e-12f);
            tile[j] = make_float4(p[0] * inv, p[1] * inv, p[2] * inv, 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < count; ++j) {
            const float4 e = tile[j];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const float d = fmaf(q[r][2], e.z, fmaf(q[r][1], e.y, q[r][0] * e.x));
                mx[r] = fmaxf(mx[r], d);
                mn[r] = fminf(mn[r], d);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int i = blockIdx.x * kStat + r * kThreads + t;
        if (i < n_o) keep[i] = (mx[r] > c_pos) || (has_neg && mn[r] < c_neg);
    }
}

struct IcpLayout {
    size_t part, xf, prev, done, d2, total;
    int nblk;
};

IcpLayout icp_layout(int B, int n_o) {
    IcpLayout l;
    Carve c;
    l.nblk = (n_o + kStat - 1) / kStat;
    l.part = c.take((size_t)B * l.nblk * kMom * 8);
    l.xf = c.take((size_t)B * kXf * 8);
    l.prev = c.take((size_t)B * 8);
    l.done = c.take((size_t)B * 4);
    l.d2 = c.take((size_t)B * n_o * 4);
    l.total = c.off;
    return l;
}

void launch_nn(const IcpArgs& a, int B, bool d6, hipStream_t st) {
    const dim3 grid(a.nblk, B);
    if (d6) icp_nn_moments_kernel<true><<<grid, kThreads, 0, st>>>(a);
    else icp_nn_moments_kernel<false><<<grid, kThreads, 0, st>>>(a);
}

bool sizes_ok(int B, int n_o, int n_h) { return n_o <= kMaxN && n_h <= kMaxN && B <= 65535; }

}  // namespace

size_t contact_icp_workspace_bytes(int B, int n_o) {
    if (B <= 0 || n_o <= 0 || n_o > kMaxN || B > 65535) return 0;
    return icp_layout(B, n_o).total;
}

int contact_icp(const float* x, const float* y, const float* xn, const float* yn, const float* w, const float* init_R, const float* init_T,
                const float* init_s, int B, int n_o, int n_h, int64_t x_bs, int64_t y_bs, int64_t xn_bs, int64_t yn_bs, int64_t w_bs,
                int max_iterations, float relative_rmse_thr, int flags, float* R, float* T, float* s, float* rmse, int32_t* converged,
                int32_t* iterations, int32_t* nn_idx, float* hist_R, float* hist_T, float* hist_s, void* ws, size_t ws_bytes,
                hipStream_t st) {
    if (!x || !y || !R || !T || !s || !rmse || !converged || !iterations || !nn_idx || !hist_R || !hist_T || !hist_s || !ws || B <= 0 ||
        n_o <= 0 || n_h <= 0 || max_iterations < 1 || x_bs < 0 || y_bs < 0 || xn_bs < 0 || yn_bs < 0 || w_bs < 0 || (xn == nullptr) != (yn == nullptr) ||
        (flags & ~(F_SCALE | F_REFLECT | F_REQUERY)))
        return IVLM_ERR_INVALID_ARG;
    if (!sizes_ok(B, n_o, n_h)) return IVLM_ERR_UNSUPPORTED;
    const IcpLayout l = icp_layout(B, n_o);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    double* xf = ws_at<double>(ws, l.xf);
    int32_t* done = ws_at<int32_t>(ws, l.done);
    IcpArgs a = {};
    a.x = x;
    a.xn = xn;
    a.y = y;
    a.yn = yn;
    a.w = w;
    a.xf = xf;
    a.done = done;
    a.x_bs = x_bs;
    a.xn_bs = xn_bs;
    a.y_bs = y_bs;
    a.yn_bs = yn_bs;
    a.w_bs = w_bs;
    a.x_rs = a.xn_rs = a.y_rs = a.yn_rs = 3;
    a.yn_sign = -1.0f;
    a.rotate_normals = (flags & F_REQUERY) != 0;  // the reference never rotates them
    a.n_o = n_o;
    a.n_h = n_h;
    a.nblk = l.nblk;
    a.nn_idx = nn_idx;
    a.nn_d2 = ws_at<float>(ws, l.d2);
    a.part = ws_at<double>(ws, l.part);
    SolveArgs sa = {};
    sa.part = a.part;
    sa.x = x;
    sa.y = y;
    sa.x_bs = x_bs;
    sa.y_bs = y_bs;
    sa.nblk = l.nblk;
    sa.flags = flags;
    sa.B = B;
    sa.thr = (double)relative_rmse_thr;
    sa.xf = xf;
    sa.prev = ws_at<double>(ws, l.prev);
    sa.done = done;
    sa.R = R;
    sa.T = T;
    sa.s = s;
    sa.rmse = rmse;
    sa.converged = converged;
    sa.iterations = iterations;
    sa.hR = hist_R;
    sa.hT = hist_T;
    sa.hs = hist_s;
    icp_init_kernel<<<(B + 63) / 64, 64, 0, st>>>(init_R, init_T, init_s, B, sa.xf, sa.done);
    const int loops = (flags & F_REQUERY) ? max_iterations : 1;
    for (int it = 0; it < loops; ++it) {
        launch_nn(a, B, xn != nullptr, st);
        sa.it = it;
        sa.rows = (flags & F_REQUERY) ? 1 : max_iterations;
        icp_solve_kernel<<<B, 64, 0, st>>>(sa);
    }
    return ivlm_launch_status();
}

int points_align(const float* X, const float* Y, const float* w, int B, int n, int64_t x_bs, int64_t y_bs, int64_t w_bs, int flags,
                 float* R, float* T, float* s, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!X || !Y || !R || !T || !s || !ws || B <= 0 || n <= 0 || x_bs < 0 || y_bs < 0 || w_bs < 0 || (flags & ~(F_SCALE | F_REFLECT)))
        return IVLM_ERR_INVALID_ARG;
    if (!sizes_ok(B, n, 1)) return IVLM_ERR_UNSUPPORTED;
    const IcpLayout l = icp_layout(B, n);
    if (!workspace_ok(ws, ws_bytes, l.total, 16)) return IVLM_ERR_WORKSPACE;
    IcpArgs a = {};
    a.x = X;
    a.yg = Y;
    a.w = w;
    a.x_bs = x_bs;
    a.yg_bs = y_bs;
    a.w_bs = w_bs;
    a.x_rs = 3;
    a.n_o = n;
    a.nblk = l.nblk;
    a.part = ws_at<double>(ws, l.part);
    launch_nn(a, B, false, st);
    SolveArgs sa = {};
    sa.part = a.part;
    sa.x = X;
    sa.y = Y;
    sa.x_bs = x_bs;
    sa.y_bs = y_bs;
    sa.nblk = l.nblk;
    sa.flags = flags;
    sa.B = B;
    sa.rows = 1;
    sa.R = R;
    sa.T = T;
    sa.s = s;
    icp_solve_kernel<<<B, 64, 0, st>>>(sa);
    return ivlm_launch_status();
}

int contact_nearest(const float* q, const float* t, int D, int B, int n_o, int n_h, int64_t q_bs, int64_t t_bs, int32_t* idx, float* d2,
                    hipStream_t st) {
    if (!q || !t || !idx || B <= 0 || n_o <= 0 || n_h <= 0 || q_bs < 0 || t_bs < 0) return IVLM_ERR_INVALID_ARG;
    if ((D != 3 && D != 6) || !sizes_ok(B, n_o, n_h)) return IVLM_ERR_UNSUPPORTED;
    IcpArgs a = {};
    a.x = q;
    a.y = t;
    a.x_bs = q_bs;
    a.y_bs = t_bs;
    a.x_rs = a.y_rs = D;
    if (D == 6) {
        a.xn = q + 3;
        a.yn = t + 3;
        a.xn_bs = q_bs;
        a.yn_bs = t_bs;
        a.xn_rs = a.yn_rs = 6;
    }
    a.yn_sign = 1.0f;
    a.n_o = n_o;
    a.n_h = n_h;
    a.nblk = (n_o + kStat - 1) / kStat;
    a.nn_idx = idx;
    a.nn_d2 = d2;
    launch_nn(a, B, D == 6, st);
    return ivlm_launch_status();
}

int contact_normal_filter(const float* on, const float* hn, int n_o, int n_h, float c_pos, float c_neg, int has_neg, uint8_t* keep,
                          hipStream_t st) {
    if (!on || !hn || !keep || n_o <= 0 || n_h <= 0) return IVLM_ERR_INVALID_ARG;
    if (n_o > kMaxN || n_h > kMaxN) return IVLM_ERR_UNSUPPORTED;
    normal_filter_kernel<<<(n_o + kStat - 1) / kStat, kThreads, 0, st>>>(on, hn, n_o, n_h, c_pos, c_neg, has_neg, keep);
    return ivlm_launch_status();
}

}  // namespace ivlm

extern "C" {
size_t ivlm_contact_icp_workspace_bytes(int B, int N_o) { return ivlm::contact_icp_workspace_bytes(B, N_o); }
int ivlm_contact_icp(const float* x, const float* y, const float* xn, const float* yn, const float* w, const float* init_R,
                     const float* init_T, const float* init_s, int B, int N_o, int N_h, int64_t x_batch_stride, int64_t y_batch_stride,
                     int64_t xn_batch_stride, int64_t yn_batch_stride, int64_t w_batch_stride, int max_iterations, float relative_rmse_thr,
                     int flags, float* R_out, float* T_out, float* s_out, float* rmse_out, int32_t* converged_out, int32_t* iterations_out,
                     int32_t* nn_idx_out, float* hist_R, float* hist_T, float* hist_s, void* workspace, size_t workspace_bytes,
                     ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::contact_icp(x, y, xn, yn, w, init_R, init_T, init_s, B, N_o, N_h, x_batch_stride, y_batch_stride, xn_batch_stride,
                             yn_batch_stride, w_batch_stride, max_iterations, relative_rmse_thr, flags, R_out, T_out, s_out, rmse_out,
                             converged_out, iterations_out, nn_idx_out, hist_R, hist_T, hist_s, workspace, workspace_bytes, ivlm_stream(s));
}
int ivlm_points_align(const float* X, const float* Y, const float* w, int B, int N, int64_t x_batch_stride, int64_t y_batch_stride,
                      int64_t w_batch_stride, int flags, float* R_out, float* T_out, float* s_out, void* workspace, size_t workspace_bytes,
                      ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::points_align(X, Y, w, B, N, x_batch_stride, y_batch_stride, w_batch_stride, flags, R_out, T_out, s_out, workspace,
                              workspace_bytes, ivlm_stream(s));
}
int ivlm_contact_nearest(const float* q, const float* t, int D, int B, int N_o, int N_h, int64_t q_batch_stride, int64_t t_batch_stride,
                         int32_t* idx_out, float* d2_out, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::contact_nearest(q, t, D, B, N_o, N_h, q_batch_stride, t_batch_stride, idx_out, d2_out, ivlm_stream(s));
}
int ivlm_contact_normal_filter(const float* obj_normals, const float* human_normals, int N_o, int N_h, float c_pos, float c_neg,
                               int has_neg, uint8_t* keep_out, ivlm_stream_t s) {
    ivlm_enter();
    return ivlm::contact_normal_filter(obj_normals, human_normals, N_o, N_h, c_pos, c_neg, has_neg, keep_out, ivlm_stream(s));
}
}
