// What the least-squares refits share (pose.hip, pose_h.hip: the poses; homography.hip: the homography refit; fundamental.hip: the
// rank-2 refit; polish.hip: the local optimisation's refit of every family): the refit source - the eigenvector of a pair's moments
// behind jacobi9.hpp's sweeps, or the winning model -, the projection onto the essential matrices with its decompositions, the rank-2
// truncation, the denormalisation's shared steps, and the homography's permutation and sign rule.  include/pats_amd.h states the
// definitions.
#pragma once
#include "common.hpp"
#include "epipolar.hpp"
#include "jacobi9.hpp"

namespace pats {

constexpr int POSE_SWEEPS = 16;                        // cap of both Jacobi loops (a sweep without a rotation ends them: the 7th or 8th)
constexpr int POSE_MIN_INLIERS = 8;
constexpr int HOM_SWEEPS = 16;                         // cap of the Jacobi loop (a sweep without a rotation ends it)
constexpr int HOM_MIN_INLIERS = 4;
constexpr int FUND_SWEEPS = 16;                        // cap of both Jacobi loops of the fundamental refit
constexpr int FUND_MIN_INLIERS = 8;

// behind jacobi9_sweeps: e = the unit eigenvector (column of V) of the smallest eigenvalue lmin (diagonal of A), the lowest index
// among equals; returns that index
__device__ __forceinline__ int refit_eigvec(const double (&sA)[9][9], const double (&sV)[9][9], double (&e)[9], double& lmin) {
    int m = 0;
    lmin = sA[0][0];
    for (int k = 1; k < 9; ++k) {                       // the smallest eigenvalue, the lowest index among equals
        const double l = sA[k][k];
        if (l < lmin) { lmin = l; m = k; }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) { e[k] = sV[k][m]; s += e[k] * e[k]; }
    const double inv = 1.0 / __builtin_sqrt(s);
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] *= inv;
    return m;
}

// the second smallest eigenvalue: the smallest over the indices other than m
__device__ __forceinline__ double refit_second(const double (&sA)[9][9], int m) {
    int m2 = m == 0 ? 1 : 0;
    double lsec = sA[m2][m2];
    for (int k = m2 + 1; k < 9; ++k) {                  // the second smallest
        const double l = sA[k][k];
        if (k != m && l < lsec) { lsec = l; m2 = k; }
    }
    return lsec;
}

// the two smallest eigenvalues behind refit_eigvec (its index m and lmin); false: one of them is not finite
__device__ __forceinline__ bool refit_spectrum(const double (&sA)[9][9], int m, double lmin, double (&ev)[2]) {
    ev[0] = lmin; ev[1] = refit_second(sA, m);
    return __builtin_isfinite(ev[0]) && __builtin_isfinite(ev[1]);
}

// ---- the refit source of pose.hip, pose_h.hip, homography.hip and fundamental.hip: moments, or models and best ------------------
// The workgroup's part: moments[p] (its upper triangle: symmetric whatever is stored) into sA, sV = I, s_bad raised by a moment that
// is not finite, then the sweeps.  EVERY thread of the THREADS of the workgroup calls it, under a workgroup-uniform condition and
// behind the barrier that follows the clearing of s_bad and s_rot; mine and sweeps are jacobi9_sweeps'
template <int THREADS>
__device__ __forceinline__ void refit_solve(const double* __restrict__ moments, int64_t p, double (&sA)[9][9], double (&sV)[9][9], int& s_bad,
                                            int& s_rot, int tid, bool mine, int sweeps) {
    for (int q = tid; q < 81; q += THREADS) {
        const int i = q / 9, j = q - 9 * i;
        const double v = moments[p * 81 + (i < j ? i * 9 + j : j * 9 + i)];
        sA[i][j] = v;
        sV[i][j] = i == j ? 1.0 : 0.0;
        if (!__builtin_isfinite(v)) s_bad = 1;          // the same value from every writer
    }
    wg_barrier();
    jacobi9_sweeps(sA, sV, s_rot, tid, mine, s_bad != 0, sweeps);
}

// One thread's part, behind refit_solve and a barrier: e = the refit of the moments (m and lmin: refit_eigvec's, for refit_spectrum) or,
// without moments, the winner of models promoted.  ok: the pair is live and no moment was bad; returns ok and nine finite values
__device__ __forceinline__ bool refit_source(bool ok, const double* __restrict__ moments, const double (&sA)[9][9], const double (&sV)[9][9],
                                             const float* __restrict__ models, int H, const int32_t* __restrict__ best, int64_t p,
                                             double (&e)[9], int& m, double& lmin) {
    m = 0;
    lmin = 0.0;
    if (ok && moments) {
        m = refit_eigvec(sA, sV, e, lmin);
    } else if (ok) {
        const float* w = epi_winner(models, H, best, p);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = (double)w[k];
    }
    if (ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) ok = ok && __builtin_isfinite(e[k]);
    }
    return ok;
}

// q = X N_l for a row-major 3x3 X and the left points' normalisation N_l = [[s0, 0, -c0 s0], [0, s1, -c1 s1], [0, 0, 1]]
__device__ __forceinline__ void refit_times_nl(const double (&x)[9], double c0l, double c1l, double s0l, double s1l, double (&q)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        q[3 * i] = x[3 * i] * s0l;
        q[3 * i + 1] = x[3 * i + 1] * s1l;
        q[3 * i + 2] = x[3 * i + 2] - (x[3 * i] * (c0l * s0l) + x[3 * i + 1] * (c1l * s1l));
    }
}

// g rescaled to Frobenius norm 1; false: g is zero or a value is not finite - no model
__device__ __forceinline__ bool refit_unit(double (&g)[9]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) s += g[k] * g[k];
    const double inv = 1.0 / __builtin_sqrt(s);
    bool ok = s > 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) { g[k] *= inv; ok = ok && __builtin_isfinite(g[k]); }
    return ok;
}

template <int P, int Q>
__device__ __forceinline__ bool pose_rot3(double (&B)[3][3], double (&W)[3][3]) {
    const double g = __builtin_fabs(B[P][Q]);
    if (g == 0.0) return false;
    if (jacobi_negligible(B[P][P], B[Q][Q], g)) {
        B[P][Q] = B[Q][P] = 0.0;
        return false;
    }
    double c, s;
    jacobi_cs(B[P][P], B[Q][Q], B[P][Q], c, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = B[k][P], y = B[k][Q];
        B[k][P] = c * x - s * y; B[k][Q] = s * x + c * y;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = B[P][k], y = B[Q][k];
        B[P][k] = c * x - s * y; B[Q][k] = s * x + c * y;
    }
    B[P][Q] = B[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = W[k][P], y = W[k][Q];
        W[k][P] = c * x - s * y; W[k][Q] = s * x + c * y;
    }
    return true;
}

// columns a and b of W and their eigenvalues exchanged if la < lb
template <int A_, int B_>
__device__ __forceinline__ void pose_order(double (&l)[3], double (&W)[3][3]) {
    const bool sw = l[A_] < l[B_];
    const double la = l[A_], lb = l[B_];
    l[A_] = sw ? lb : la; l[B_] = sw ? la : lb;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = W[k][A_], y = W[k][B_];
        W[k][A_] = sw ? y : x; W[k][B_] = sw ? x : y;
    }
}

__device__ __forceinline__ void pose_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// e (a 3x3 G, row-major) -> E = U diag(s, s, 0) V^T with |E|_F = 1, R1 = U W V^T, R2 = U W^T V^T, u = U[:,2]; false: no pose
__device__ __forceinline__ bool pose_decompose(const double (&e)[9], double (&E)[9], double (&R1)[9], double (&R2)[9], double (&u3)[3]) {
    double G[3][3], B[3][3], W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { G[i][j] = e[3 * i + j]; W[i][j] = i == j ? 1.0 : 0.0; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = G[0][i] * G[0][j] + G[1][i] * G[1][j] + G[2][i] * G[2][j];
    for (int sweep = 0; sweep < POSE_SWEEPS; ++sweep) {
        bool any = pose_rot3<0, 1>(B, W);
        any = pose_rot3<0, 2>(B, W) || any;
        any = pose_rot3<1, 2>(B, W) || any;
        if (!any) break;
    }
    double l[3] = {B[0][0], B[1][1], B[2][2]};
    pose_order<0, 1>(l, W);                             // descending: the columns of W become v_1, v_2, (v_3)
    pose_order<1, 2>(l, W);
    pose_order<0, 1>(l, W);
    double v1[3], v2[3], v3[3], u1[3], u2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v1[k] = W[k][0]; v2[k] = W[k][1]; }
    pose_cross(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = G[i][0] * v1[0] + G[i][1] * v1[1] + G[i][2] * v1[2];
        u2[i] = G[i][0] * v2[0] + G[i][1] * v2[1] + G[i][2] * v2[2];
    }
    const double s1 = __builtin_sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (!(s1 > 0.0)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] /= s1;
    const double d = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
    const double s2 = __builtin_sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (!(s2 > 0.0)) return false;                      // rank below 2: no essential matrix is nearest
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] /= s2;
    pose_cross(u1, u2, u3);
    const double h = 0.70710678118654752440;            // 1 / sqrt 2
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double a = u1[i] * v1[j] + u2[i] * v2[j], b = u2[i] * v1[j] - u1[i] * v2[j], c = u3[i] * v3[j];
            E[3 * i + j] = a * h;
            R1[3 * i + j] = b + c;                      // U W V^T,  W = [[0,-1,0],[1,0,0],[0,0,1]]
            R2[3 * i + j] = c - b;                      // U W^T V^T
            ok = ok && __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
        }
    return ok;
}

// e (a 3x3 G, row-major) -> F = U diag(s1, s2, 0) V^T rescaled to |F|_F = 1 and sig = the singular values of G, descending - the
// route of pose_decompose with both singular values kept and the third term dropped; false: rank below 2, no fundamental matrix
__device__ __forceinline__ bool fund_project(const double (&e)[9], double (&F)[9], double (&sig)[3]) {
    double G[3][3], B[3][3], W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { G[i][j] = e[3 * i + j]; W[i][j] = i == j ? 1.0 : 0.0; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = G[0][i] * G[0][j] + G[1][i] * G[1][j] + G[2][i] * G[2][j];
    for (int sweep = 0; sweep < FUND_SWEEPS; ++sweep) {
        bool any = pose_rot3<0, 1>(B, W);
        any = pose_rot3<0, 2>(B, W) || any;
        any = pose_rot3<1, 2>(B, W) || any;
        if (!any) break;
    }
    double l[3] = {B[0][0], B[1][1], B[2][2]};
    pose_order<0, 1>(l, W);                             // descending: the columns of W become v_1, v_2, (v_3)
    pose_order<1, 2>(l, W);
    pose_order<0, 1>(l, W);
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v1[k] = W[k][0]; v2[k] = W[k][1]; }
    pose_cross(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = G[i][0] * v1[0] + G[i][1] * v1[1] + G[i][2] * v1[2];
        u2[i] = G[i][0] * v2[0] + G[i][1] * v2[1] + G[i][2] * v2[2];
        u3[i] = G[i][0] * v3[0] + G[i][1] * v3[1] + G[i][2] * v3[2];
    }
    const double s1 = __builtin_sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (!(s1 > 0.0)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] /= s1;
    const double d = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
    const double s2 = __builtin_sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (!(s2 > 0.0)) return false;                      // rank below 2: no fundamental matrix is nearest
    sig[0] = s1; sig[1] = s2;
    sig[2] = __builtin_sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);               // |G v_3|: second order in the error of v_3
    double nn = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            F[3 * i + j] = s1 * (u1[i] * v1[j]) + u2[i] * v2[j];                           // u2 still carries s2
            nn += F[3 * i + j] * F[3 * i + j];
        }
    const double inv = 1.0 / __builtin_sqrt(nn);
    bool ok = nn > 0.0 && __builtin_isfinite(sig[2]);
#pragma unroll
    for (int k = 0; k < 9; ++k) { F[k] *= inv; ok = ok && __builtin_isfinite(F[k]); }
    return ok;
}

// behind jacobi9_sweeps, on one thread: e = the refit of the moments, ev = their two smallest eigenvalues, F and sig = fund_project
// of e - what the fundamental refit (fundamental.hip) and the local optimisation's refit of that family (polish.hip) both return
__device__ __forceinline__ bool fund_from_moments(const double (&sA)[9][9], const double (&sV)[9][9], double (&e)[9], double (&ev)[2],
                                                  double (&F)[9], double (&sig)[3]) {
    double lmin;
    const int m = refit_eigvec(sA, sV, e, lmin);
    const double lsec = refit_second(sA, m);
    ev[0] = lmin; ev[1] = lsec;
    bool ok = __builtin_isfinite(lmin) && __builtin_isfinite(lsec);
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && __builtin_isfinite(e[k]);
    return ok && fund_project(e, F, sig);
}

// out[k] = +-v[P k P]: the frame change (hom_perm, epipolar.hpp), then the sign rule judged on the values written (the lowest index among equals)
__device__ __forceinline__ void hom_write(const double (&v)[9], bool ok, int swapped, double* __restrict__ out) {
    double big = -1.0, at = 0.0;
    for (int k = 0; k < 9; ++k) {
        const double x = ok ? v[hom_perm(k, swapped)] : 0.0;
        if (__builtin_fabs(x) > big) { big = __builtin_fabs(x); at = x; }
    }
    const bool flip = at < 0.0;
    for (int k = 0; k < 9; ++k) {
        const double x = ok ? v[hom_perm(k, swapped)] : 0.0;
        out[k] = flip ? -x : x;
    }
}

// ---- the pose behind a homography (pose_h.hip; include/pats_amd.h, "Per-pair pose from a homography") ----------------------------
constexpr int HPOSE_SWEEPS = 16;                       // cap of the 3x3 Jacobi loop

// e (a 3x3 G, row-major) -> G^T G = V diag(lam) V^T, lam descending, the columns of V = v_1, v_2, v_1 x v_2;  Gp = G / sqrt(lam_2),
// l1 = max(lam_1 / lam_2, 1), l3 = min(max(lam_3 / lam_2, 0), 1);  false: lam_2 <= 0 or a value that is not finite
__device__ __forceinline__ bool hom_spectrum(const double (&e)[9], double (&Gp)[9], double (&V)[3][3], double& l1, double& l3) {
    double B[3][3], W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            B[i][j] = e[i] * e[j] + e[3 + i] * e[3 + j] + e[6 + i] * e[6 + j];
            W[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < HPOSE_SWEEPS; ++sweep) {
        bool any = pose_rot3<0, 1>(B, W);
        any = pose_rot3<0, 2>(B, W) || any;
        any = pose_rot3<1, 2>(B, W) || any;
        if (!any) break;
    }
    double l[3] = {B[0][0], B[1][1], B[2][2]};
    pose_order<0, 1>(l, W);                             // descending: the columns of W become v_1, v_2, (v_3)
    pose_order<1, 2>(l, W);
    pose_order<0, 1>(l, W);
    if (!(l[1] > 0.0) || !__builtin_isfinite(l[0]) || !__builtin_isfinite(l[1]) || !__builtin_isfinite(l[2])) return false;
    double v1[3], v2[3], v3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v1[k] = W[k][0]; v2[k] = W[k][1]; }
    pose_cross(v1, v2, v3);
#pragma unroll
    for (int k = 0; k < 3; ++k) { V[k][0] = v1[k]; V[k][1] = v2[k]; V[k][2] = v3[k]; }
    const double inv = 1.0 / __builtin_sqrt(l[1]);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) { Gp[k] = e[k] * inv; ok = ok && __builtin_isfinite(Gp[k]); }
    const double a = l[0] / l[1], c = l[2] / l[1];
    l1 = a > 1.0 ? a : 1.0;
    l3 = c < 1.0 ? (c > 0.0 ? c : 0.0) : 1.0;
    return ok && __builtin_isfinite(l1);
}

// y = G x for a row-major 3x3
__device__ __forceinline__ void hom_apply(const double (&G)[9], const double (&x)[3], double (&y)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = G[3 * i] * x[0] + G[3 * i + 1] * x[1] + G[3 * i + 2] * x[2];
}

// the rotation of a homography without a baseline: R = Gp V diag(1/sqrt(l1), 1, 1/sqrt(l3)) V^T (l3 > 0);  false: not finite
__device__ __forceinline__ bool hom_rotation(const double (&Gp)[9], const double (&V)[3][3], double l1, double l3, double (&R)[9]) {
    const double d[3] = {1.0 / __builtin_sqrt(l1), 1.0, 1.0 / __builtin_sqrt(l3)};
    double gv[3][3];                                    // gv[c] = Gp v_c
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v[3] = {V[0][c], V[1][c], V[2][c]};
        hom_apply(Gp, v, gv[c]);
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R[3 * i + j] = gv[0][i] * d[0] * V[j][0] + gv[1][i] * d[1] * V[j][1] + gv[2][i] * d[2] * V[j][2];
            ok = ok && __builtin_isfinite(R[3 * i + j]);
        }
    return ok;
}

// The two candidates s = +1, -1 of Gp = R + t n^T with Gp^T Gp = V diag(l1, 1, l3) V^T and l1 - l3 > 0 (the eigenvector form of the
// four-solution algorithm; the other two are (R_k, -t_k, -n_k)):
//   u = (sqrt(1 - l3) v1 + s sqrt(l1 - 1) v3) / sqrt(l1 - l3),  U = [v2, u, v2 x u],  W = [Gp v2, Gp u, (Gp v2) x (Gp u)]
//   R = W U^T,  n = v2 x u,  t = (Gp - R) n (not normalised),  E = [t / |t|]x R scaled to Frobenius norm 1
// false: a value that is not finite, or t = 0
__device__ __forceinline__ bool hom_decompose(const double (&Gp)[9], const double (&V)[3][3], double l1, double l3, double (&R)[2][9],
                                              double (&t)[2][3], double (&n)[2][3], double (&E)[2][9]) {
    const double a = __builtin_sqrt(1.0 - l3), b = __builtin_sqrt(l1 - 1.0), inv = 1.0 / __builtin_sqrt(l1 - l3);
    const double v2[3] = {V[0][1], V[1][1], V[2][1]};
    double w0[3];
    hom_apply(Gp, v2, w0);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double sb = k == 0 ? b : -b;
        double u[3], w1[3], w2[3], nn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) u[i] = (a * V[i][0] + sb * V[i][2]) * inv;
        pose_cross(v2, u, nn);
        hom_apply(Gp, u, w1);
        pose_cross(w0, w1, w2);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[k][3 * i + j] = w0[i] * v2[j] + w1[i] * u[j] + w2[i] * nn[j];
        double gn[3], rn[3], tt[3];
        hom_apply(Gp, nn, gn);
        hom_apply(R[k], nn, rn);
#pragma unroll
        for (int i = 0; i < 3; ++i) { tt[i] = gn[i] - rn[i]; t[k][i] = tt[i]; n[k][i] = nn[i]; }
        const double tn = __builtin_sqrt(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
        ok = ok && tn > 0.0 && __builtin_isfinite(tn);
        const double q[3] = {tt[0] / tn, tt[1] / tn, tt[2] / tn};
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {                   // [q]x R by rows
            E[k][j] = q[1] * R[k][6 + j] - q[2] * R[k][3 + j];
            E[k][3 + j] = q[2] * R[k][j] - q[0] * R[k][6 + j];
            E[k][6 + j] = q[0] * R[k][3 + j] - q[1] * R[k][j];
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) s += E[k][j] * E[k][j];
        const double es = 1.0 / __builtin_sqrt(s);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            E[k][j] *= es;
            ok = ok && __builtin_isfinite(E[k][j]) && __builtin_isfinite(R[k][j]);
        }
    }
    return ok;
}

}  // namespace pats
