// The float32 null vector of a 9x8 matrix A^T held in a thread's registers - the solve of the 8-point and the 4-point hypotheses
// (hypotheses.hip).  Every index is static once the loops are unrolled: no scratch, no LDS.
//   solve    Householder QR of A^T, no pivoting: the reflectors stay below the diagonal, R on and above it.  The null vector is the
//            last column of Q = H_0 .. H_7 e_8 - orthogonal to every column of A^T whatever its rank, so a degenerate sample still
//            gives a finite unit vector.  No component is pinned
//   refine   ONE step of iterative refinement: the residual of each column from the caller (through the factored form of its
//            constraint, fused multiply-adds on the float32 points: the error of rounding the matrix entries to float32 is not in
//            it), R^T y = res by forward substitution, e = z - Q (y, 0).  A step that does not end finite (a zero pivot) is dropped
#pragma once
#include "common.hpp"

namespace pats {

// z <- H_0 H_1 .. H_7 z with the reflectors H_k = I - tau_k v_k v_k^T, v_k = (1, M[k+1..8][k]) on rows k .. 8
__device__ __forceinline__ void apply_q(const float (&M)[9][8], const float (&tau)[8], float (&z)[9]) {
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        float d = z[k];
#pragma unroll
        for (int i = k + 1; i < 9; ++i) d = __builtin_fmaf(M[i][k], z[i], d);
        const float w = -(tau[k] * d);
        z[k] += w;
#pragma unroll
        for (int i = k + 1; i < 9; ++i) z[i] = __builtin_fmaf(w, M[i][k], z[i]);
    }
}

// z scaled to Frobenius norm 1; false unless every component ends finite
__device__ __forceinline__ bool unit(float (&z)[9]) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) s = __builtin_fmaf(z[k], z[k], s);
    const float inv = 1.0f / __builtin_sqrtf(s);
    bool ok = s > 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        z[k] *= inv;
        ok = ok && __builtin_isfinite(z[k]);
    }
    return ok;
}

// e = the unit null vector of M = A^T (factored in place); res(z, j) = the residual (column j of A^T) . z; false: no finite vector
template <class Res>
__device__ __forceinline__ bool null_vector_9x8(float (&M)[9][8], const Res& res, float (&e)[9]) {
    float tau[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float s = 0.0f;
#pragma unroll
        for (int i = k; i < 9; ++i) s = __builtin_fmaf(M[i][k], M[i][k], s);
        const float nrm = __builtin_sqrtf(s), x0 = M[k][k];
        const float beta = x0 >= 0.0f ? -nrm : nrm;                                    // x0 - beta never cancels
        const bool live = nrm > 0.0f;                                                  // a zero column: H_k = I
        tau[k] = live ? (beta - x0) / beta : 0.0f;
        const float inv = live ? 1.0f / (x0 - beta) : 0.0f;
#pragma unroll
        for (int i = k + 1; i < 9; ++i) M[i][k] *= inv;
        M[k][k] = beta;
#pragma unroll
        for (int j = k + 1; j < 8; ++j) {
            float d = M[k][j];
#pragma unroll
            for (int i = k + 1; i < 9; ++i) d = __builtin_fmaf(M[i][k], M[i][j], d);
            const float w = -(tau[k] * d);
            M[k][j] += w;
#pragma unroll
            for (int i = k + 1; i < 9; ++i) M[i][j] = __builtin_fmaf(w, M[i][k], M[i][j]);
        }
    }
    float z[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    apply_q(M, tau, z);
    // one refinement step: R^T y = res, e = z - Q (y, 0)
    float c[9];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float acc = res(z, j);
#pragma unroll
        for (int i = 0; i < j; ++i) acc = __builtin_fmaf(-M[i][j], c[i], acc);
        c[j] = acc / M[j][j];
    }
    c[8] = 0.0f;
    apply_q(M, tau, c);
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = z[k] - c[k];
    bool ok = unit(e);
    if (!ok) {                                          // the step met a zero pivot or overflowed: the QR vector as it is
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = z[k];
        ok = unit(e);
    }
    return ok;
}

}  // namespace pats
