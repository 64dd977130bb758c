// The ground-truth relative pose of a pair from its extrinsics, as include/pats_amd.h states it under pats_pose_error_by_pair_f64:
// written once for the two stages that score against it (pose_error.hip: the pose; match_error.hip: the matches).
#pragma once
#include "common.hpp"

namespace pats {

__device__ __forceinline__ bool gt_finite12(const double* __restrict__ T) {           // the upper 3 x 4 of a row-major 4 x 4
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && __builtin_isfinite(T[k]);
    return ok;
}

// pair p of T1 [pairs,4,4] and (optional) T0 [pairs,4,4] -> G = R_gt row-major, g = t_gt; returns whether every entry that was read
// is finite.  Without T0: R_gt = R1, t_gt = t1.  With T0: R_gt = R1 R0^T, t_gt = t1 - R_gt t0 (float64, no contraction, sums left
// to right)
__device__ __forceinline__ bool gt_relative_pose(const double* __restrict__ T1, const double* __restrict__ T0, int64_t p, double (&G)[9],
                                                 double (&g)[3]) {
    double A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = T1[p * 16 + k];
    bool gt_ok = gt_finite12(A);
    if (T0 != nullptr) {                                // R_gt = R1 R0^T, t_gt = t1 - R_gt t0
        double B[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) B[k] = T0[p * 16 + k];
        gt_ok = gt_ok && gt_finite12(B);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) G[i * 3 + j] = (A[i * 4] * B[j * 4] + A[i * 4 + 1] * B[j * 4 + 1]) + A[i * 4 + 2] * B[j * 4 + 2];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = A[i * 4 + 3] - ((G[i * 3] * B[3] + G[i * 3 + 1] * B[7]) + G[i * 3 + 2] * B[11]);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) G[i * 3 + j] = A[i * 4 + j];
            g[i] = A[i * 4 + 3];
        }
    }
    return gt_ok;
}

}  // namespace pats
