// The float64 cyclic Jacobi of a symmetric 9x9 matrix in LDS - the eigen-solve of the pose (pose.hip), of the homography refit
// (homography.hip) and of the local optimisation's refits (polish.hip) - and its rotation, which refit.hpp's 3x3 Jacobi in registers shares.
//   order   round-robin: a sweep is nine rounds of four disjoint rotations (p, q) = ((r + i) % 9, (r - i) % 9), i = 1 .. 4 - sixteen
//           lanes per rotation (the first 64 threads of the workgroup), lane k < 9 of a group updates row / column entry k
//   stop    a rotation whose off-diagonal entry no longer changes either diagonal entry when added to it is replaced by setting that
//           entry to zero; a sweep without a rotation ends the loop, `sweeps` caps it
#pragma once
#include "common.hpp"

namespace pats {

// the rotation that annihilates apq: J = [[c, s], [-s, c]] on (p, q), B = J^T A J  (apq != 0)
__device__ __forceinline__ void jacobi_cs(double app, double aqq, double apq, double& c, double& s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));   // 0 for a huge theta
    c = 1.0 / __builtin_sqrt(t * t + 1.0);
    s = t * c;
}

// apq is too small to change either diagonal entry
__device__ __forceinline__ bool jacobi_negligible(double app, double aqq, double g) {
    return __builtin_fabs(app) + g == __builtin_fabs(app) && __builtin_fabs(aqq) + g == __builtin_fabs(aqq);
}

// A <- V^T A V towards diagonal, V accumulates the rotations (the caller loaded A, set V = I and s_rot = 0, and passed a barrier).
// EVERY thread of the workgroup calls this and reaches every barrier: the trip counts depend on `bad` (workgroup-uniform) and the
// LDS flag s_rot alone.  mine: the thread is lane k = tid & 15 < 9 of one of the four groups tid >> 4 of the first 64 threads
__device__ __forceinline__ void jacobi9_sweeps(double (&sA)[9][9], double (&sV)[9][9], int& s_rot, int tid, bool mine, bool bad, int sweeps) {
    const int grp = tid >> 4, k = tid & 15;             // rotation grp of a round, entry k
    for (int sweep = 0; sweep < sweeps && !bad; ++sweep) {
        for (int r = 0; r < 9; ++r) {
            int pp = (r + grp + 1) % 9, qq = (r + 8 - grp) % 9;
            if (pp > qq) { const int x_ = pp; pp = qq; qq = x_; }
            double c = 1.0, s = 0.0, x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
            bool rot = false, zero = false;
            if (mine) {
                const double app = sA[pp][pp], aqq = sA[qq][qq], apq = sA[pp][qq];
                const double g = __builtin_fabs(apq);
                if (g != 0.0) {
                    if (jacobi_negligible(app, aqq, g)) {
                        zero = k == 0;
                    } else {
                        rot = true;
                        jacobi_cs(app, aqq, apq, c, s);
                    }
                }
                x = sA[k][pp]; y = sA[k][qq];
                vx = sV[k][pp]; vy = sV[k][qq];
            }
            wg_barrier();                               // every lane has read the round's entries
            if (zero) { sA[pp][qq] = 0.0; sA[qq][pp] = 0.0; }           // no other lane touches the two in this round
            if (rot) {                                  // A <- A J, V <- V J: the columns p and q
                sA[k][pp] = c * x - s * y; sA[k][qq] = s * x + c * y;
                sV[k][pp] = c * vx - s * vy; sV[k][qq] = s * vx + c * vy;
                s_rot = 1;
            }
            wg_barrier();
            if (rot) {                                  // A <- J^T A: the rows p and q; the annihilated pair is set, not computed
                x = sA[pp][k]; y = sA[qq][k];
                sA[pp][k] = k == qq ? 0.0 : c * x - s * y;
                sA[qq][k] = k == pp ? 0.0 : s * x + c * y;
            }
            wg_barrier();
        }
        const bool again = s_rot != 0;
        wg_barrier();
        if (tid == 0) s_rot = 0;
        if (!again) break;
    }
}

}  // namespace pats
