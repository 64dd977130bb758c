// Per-pair relative pose from the verified inliers: for every pair of a batch the least-squares refit of the winner's moments (the
// eigenvector of the 9x9 moment matrix for its smallest eigenvalue - or the winning model itself), its projection onto the essential
// matrices, the four (R, t) decompositions and the cheirality vote of the pair's inliers that picks one of them.  One launch (after
// the fill of the optional mask), no host read.  include/pats_amd.h states the definition; docs/kernels.md 4.9 the design.
//
//   one workgroup per pair, POSE_THREADS = 256 threads, decided by the sizes alone
//   solve   float64.  The 9x9 matrix A and the accumulated rotations V live in LDS; wave 0 runs the round-robin cyclic Jacobi of
//           jacobi9.hpp (shared with the homography refit), POSE_SWEEPS caps it.  Thread 0 then holds everything else in registers,
//           all indices static (refit.hpp, shared with polish.hip): the eigenvector, G^T G of it as a 3x3 G, a 3x3 Jacobi for the
//           right singular vectors, u_i = G v_i (Gram-Schmidt), u_3 = u_1 x u_2, v_3 = v_1 x v_2 (det U = det V = +1 by
//           construction), E, R1, R2, u.  They go to LDS in float64 and float32.
//   vote    the workgroup walks the segment with epi_load_masked; pose_front4 gives the four verdicts of a match as bits (R1 and R2
//           share everything up to the two signs); the count fold of epipolar.hpp, thread 0 picks the candidate and writes the
//           per-pair outputs, R, t and E in the frame `swapped` asks for (hom_perm, frame_perm, hom_write).
//   mask    a second walk with the same device function writes the chosen candidate's bit: front.sum() == front_count exactly.
#include "common.hpp"
#include "epipolar.hpp"
#include "jacobi9.hpp"
#include "refit.hpp"

namespace pats {

constexpr int POSE_THREADS = 256;
constexpr int POSE_WAVES = POSE_THREADS / WAVE;

// THE cheirality test - the vote and the mask both call it.  Bit k: the match lies in front of both cameras under candidate k of
// (R1, u), (R2, u), (R1, -u), (R2, -u).  A NaN l0 (a match that is not used) gives 0.
__device__ __forceinline__ unsigned pose_front4(const float (&R)[2][9], const float (&u)[3], float l0, float l1, float r0, float r1) {
    // b x t, b = (r0, r1, 1)
    const float bt0 = __builtin_fmaf(r1, u[2], -u[1]), bt1 = __builtin_fmaf(-r0, u[2], u[0]), bt2 = __builtin_fmaf(r0, u[1], -(r1 * u[0]));
    unsigned bits = 0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float a0 = __builtin_fmaf(R[j][0], l0, __builtin_fmaf(R[j][1], l1, R[j][2]));
        const float a1 = __builtin_fmaf(R[j][3], l0, __builtin_fmaf(R[j][4], l1, R[j][5]));
        const float a2 = __builtin_fmaf(R[j][6], l0, __builtin_fmaf(R[j][7], l1, R[j][8]));
        const float c0 = __builtin_fmaf(-a2, r1, a1), c1 = __builtin_fmaf(a2, r0, -a0), c2 = __builtin_fmaf(a0, r1, -(a1 * r0));   // a x b
        const float at0 = __builtin_fmaf(a1, u[2], -(a2 * u[1])), at1 = __builtin_fmaf(a2, u[0], -(a0 * u[2])),
                    at2 = __builtin_fmaf(a0, u[1], -(a1 * u[0]));                                                              // a x t
        const float cc = __builtin_fmaf(c0, c0, __builtin_fmaf(c1, c1, c2 * c2));
        const float dl = __builtin_fmaf(c0, bt0, __builtin_fmaf(c1, bt1, c2 * bt2));
        const float dr = __builtin_fmaf(c0, at0, __builtin_fmaf(c1, at1, c2 * at2));
        if (cc > 0.0f && dl > 0.0f && dr > 0.0f) bits |= 1u << j;
        if (cc > 0.0f && dl < 0.0f && dr < 0.0f) bits |= 4u << j;      // -u: both signs turn
    }
    return bits;
}

__global__ void __launch_bounds__(POSE_THREADS)
epipolar_pose_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const uint8_t* __restrict__ inlier,
                     const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                     const int64_t* __restrict__ best_count, const double* __restrict__ moments, const float* __restrict__ models, int H,
                     const int32_t* __restrict__ best, const float* __restrict__ norm, int swapped, double* __restrict__ E_out,
                     double* __restrict__ R_out, double* __restrict__ t_out, int32_t* __restrict__ front_counts,
                     int32_t* __restrict__ choice_out, int64_t* __restrict__ front_count, uint8_t* __restrict__ front,
                     double* __restrict__ e_refit) {
    __shared__ double sA[9][9], sV[9][9];
    __shared__ double sE[9], sR[2][9], sU[3];
    __shared__ float sRf[2][9], sUf[3];
    __shared__ int s_cnt[POSE_WAVES][4];
    __shared__ int s_bad, s_rot, s_ok, s_choice;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const bool live = best_count[p] >= POSE_MIN_INLIERS;  // workgroup-uniform
    if (tid == 0) { s_bad = 0; s_rot = 0; s_ok = 0; s_choice = 0; }
    wg_barrier();

    // ---- solve ------------------------------------------------------------------------------------------------------------------
    if (live && moments)                                // workgroup-uniform
        refit_solve<POSE_THREADS>(moments, p, sA, sV, s_bad, s_rot, tid, tid < 64 && (tid & 15) < 9, POSE_SWEEPS);
    if (tid == 0) {
        double e[9], lmin;
        int m;
        bool ok = refit_source(live && s_bad == 0, moments, sA, sV, models, H, best, p, e, m, lmin);
        if (e_refit) {
#pragma unroll
            for (int k = 0; k < 9; ++k) e_refit[p * 9 + k] = ok ? e[k] : 0.0;
        }
        double E[9], R1[9], R2[9], u[3];
        if (ok) ok = pose_decompose(e, E, R1, R2, u);
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                sE[k] = E[k]; sR[0][k] = R1[k]; sR[1][k] = R2[k];
                sRf[0][k] = (float)R1[k]; sRf[1][k] = (float)R2[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { sU[k] = u[k]; sUf[k] = (float)u[k]; }
            s_ok = 1;
        }
    }
    wg_barrier();
    const bool ok = s_ok != 0;                          // workgroup-uniform

    // ---- vote -------------------------------------------------------------------------------------------------------------------
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const uint8_t* inl = inlier + lo;
    const EpiNorm nm = epi_norm(norm, p);
    float Rf[2][9], uf[3];
    int cnt[4] = {0, 0, 0, 0};
    if (ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { Rf[0][k] = sRf[0][k]; Rf[1][k] = sRf[1][k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) uf[k] = sUf[k];
        for (uint32_t i0 = 0; i0 < n; i0 += POSE_THREADS) {
            float l0, l1, r0, r1;
            epi_load_masked(ml, mr, inl, i0 + tid, n, norm != nullptr, nm, l0, l1, r0, r1);
            const unsigned bits = pose_front4(Rf, uf, l0, l1, r0, r1);
#pragma unroll
            for (int c = 0; c < 4; ++c) cnt[c] += wave_count((bits >> c) & 1u);
        }
        wave_parts_store(s_cnt, wave, lane, cnt);
    }
    wg_barrier();
    if (tid == 0) {
        int tot[4] = {0, 0, 0, 0};
        int ch = 0, top = 0;
        if (ok) {
#pragma unroll
            for (int c = 0; c < 4; ++c) tot[c] = wave_parts_total(s_cnt, c);
            top = tot[0];
#pragma unroll
            for (int c = 1; c < 4; ++c)
                if (tot[c] > top) { top = tot[c]; ch = c; }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) front_counts[p * 4 + c] = tot[c];
        choice_out[p] = ch;
        front_count[p] = (int64_t)top;
        s_choice = ch;
    }
    wg_barrier();
    const int ch = s_choice;
    if (tid < 9) {                                      // the pose in the reference's frame: P R P, P t
        const int i = tid / 3, j = tid - 3 * i;
        R_out[p * 9 + tid] = ok ? sR[ch & 1][hom_perm(tid, swapped)] : (i == j ? 1.0 : 0.0);
        if (j == 0) t_out[p * 3 + i] = ok ? ((ch & 2) ? -sU[frame_perm(i, swapped)] : sU[frame_perm(i, swapped)]) : 0.0;
    }
    if (tid == 64) {                                    // E, its sign judged on the values written
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = ok ? sE[k] : 0.0;
        hom_write(E, ok, swapped, E_out + p * 9);
    }

    // ---- mask -------------------------------------------------------------------------------------------------------------------
    if (!front || !ok) return;                          // the mask was zeroed before the launch
    for (uint32_t i0 = 0; i0 < n; i0 += POSE_THREADS) {
        const uint32_t i = i0 + tid;
        float l0, l1, r0, r1;
        epi_load_masked(ml, mr, inl, i, n, norm != nullptr, nm, l0, l1, r0, r1);
        const unsigned bits = pose_front4(Rf, uf, l0, l1, r0, r1);
        if (i < n) front[lo + i] = (uint8_t)((bits >> ch) & 1u);
    }
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_epipolar_pose_workspace_bytes(int64_t pairs, int64_t cap) {
    (void)pairs; (void)cap;
    return 0;                                           // the solve lives in LDS and registers, the mask is a second walk
}

extern "C" int pats_epipolar_pose_by_pair_f64(const float* matches_l, const float* matches_r, const uint8_t* inlier, const int64_t* pair_off,
                                              int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap,
                                              const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                              const int32_t* best, const float* norm, int swapped, double* E, double* R, double* t,
                                              int32_t* front_counts, int32_t* choice, int64_t* front_count, uint8_t* front,
                                              double* e_refit, void* workspace, size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    const char* who = "epipolar_pose_by_pair";
    int rc = epi_check_args(who, {{"matches_l", matches_l, 8}, {"matches_r", matches_r, 8}, {"inlier", inlier, 1}, {"best_count", best_count, 8},
                                  {"E", E, 8}, {"R", R, 8}, {"t", t, 8}, {"front_counts", front_counts, 4}, {"choice", choice, 4},
                                  {"front_count", front_count, 8}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"moments", moments, 8}, {"models", models, 4}, {"best", best, 4}, {"norm", norm, 4}, {"pair_off", pair_off, 8},
                              {"counts_in", counts_in, 8}, {"e_refit", e_refit, 8}}, false);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    if ((rc = epi_check_refit_source(who, moments, models, best, H, swapped)) != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_epipolar_pose_workspace_bytes(pairs, cap), "%s: workspace too small", who);
    hipStream_t st = as_stream(stream);
    if (front) {
        rc = fill_bytes(front, 0, (size_t)cap, st);
        if (rc != PATS_OK) return rc;
    }
    hipLaunchKernelGGL(epipolar_pose_kernel, dim3((unsigned)pairs), dim3(POSE_THREADS), 0, st, matches_l, matches_r, inlier, pair_off,
                       counts_in, stride, cap, best_count, moments, models, (int)H, best, norm, swapped, E, R, t, front_counts, choice,
                       front_count, front, e_refit);
    return check_launch("epipolar_pose kernel");
}
