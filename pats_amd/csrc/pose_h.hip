// Per-pair pose from a verified homography, and the per-pair choice between the epipolar and the planar pose - what closes the planar
// branch the way pose.hip closes the epipolar one.  One launch each (after the fills of the masks), no host read.  include/pats_amd.h
// states the definitions ("Per-pair pose from a homography and the E-or-H decision"); docs/kernels.md 4.15 the design.
//
//   one workgroup per pair, HPOSE_THREADS = 256 threads, decided by the sizes alone
//   solve   float64.  The 9x9 moments and the accumulated rotations live in LDS; wave 0 runs the round-robin cyclic Jacobi of
//           jacobi9.hpp.  Thread 0 then holds the rest (refit.hpp: hom_spectrum, hom_rotation, hom_decompose) and hands G', V and the
//           two ratios over in LDS: the sign of G' is a vote of the workgroup that stands between the spectrum and the candidates.
//   walks   three over the segment with epi_load_masked, the first two closed by the count fold of epipolar.hpp: the sign vote, the
//           visibility and support counts, the mask.  hpose_side is THE visibility test: the counts and the mask both call it, so
//           front.sum() == front_count exactly.  The outputs go out in the frame `swapped` asks for (hom_perm, frame_perm, hom_write).
#include "common.hpp"
#include "epipolar.hpp"
#include "jacobi9.hpp"
#include "refit.hpp"
#include "verify.hpp"

namespace pats {

constexpr int HPOSE_THREADS = 256;
constexpr int HPOSE_WAVES = HPOSE_THREADS / WAVE;
constexpr int SELECT_THREADS = 256;

// n . x_l in float32, x_l = (l0, l1, 1); a NaN l0 gives a NaN: neither side
__device__ __forceinline__ float hpose_side(const float (&n)[3], float l0, float l1) {
    return __builtin_fmaf(n[0], l0, __builtin_fmaf(n[1], l1, n[2]));
}

__global__ void __launch_bounds__(HPOSE_THREADS)
homography_pose_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const uint8_t* __restrict__ inlier,
                       const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                       const int64_t* __restrict__ best_count, const double* __restrict__ moments, const float* __restrict__ models, int H,
                       const int32_t* __restrict__ best, const float* __restrict__ norm, const float* __restrict__ thr, int swapped,
                       double min_baseline, double* __restrict__ E_out, double* __restrict__ R_out, double* __restrict__ t_out,
                       double* __restrict__ n_out, double* __restrict__ baseline_out, int32_t* __restrict__ vis_out,
                       int32_t* __restrict__ sup_out, int32_t* __restrict__ choice_out, int32_t* __restrict__ status_out,
                       int64_t* __restrict__ front_count, double* __restrict__ cand_R, double* __restrict__ cand_t,
                       double* __restrict__ cand_n, uint8_t* __restrict__ front) {
    __shared__ double sA[9][9], sV[9][9];
    __shared__ double sG[9], sW[3][3], sL[2];
    __shared__ double sR[2][9], sT[2][3], sN[2][3], sE[2][9], sBase;
    __shared__ float sGf[9], sNf[2][3], sEf[2][9];
    __shared__ int s_cnt[HPOSE_WAVES][8];
    __shared__ int s_bad, s_rot, s_ok, s_status, s_choice;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const bool live = best_count[p] >= HOM_MIN_INLIERS; // workgroup-uniform
    if (tid == 0) { s_bad = 0; s_rot = 0; s_ok = 0; s_status = 0; s_choice = 0; }
    wg_barrier();

    // ---- solve: the refit and its spectrum -----------------------------------------------------------------------------------------
    if (live && moments)                                // workgroup-uniform
        refit_solve<HPOSE_THREADS>(moments, p, sA, sV, s_bad, s_rot, tid, tid < 64 && (tid & 15) < 9, HOM_SWEEPS);
    if (tid == 0) {
        double e[9], lmin;
        int m;
        bool ok = refit_source(live && s_bad == 0, moments, sA, sV, models, H, best, p, e, m, lmin);
        double Gp[9], V[3][3], l1 = 1.0, l3 = 1.0;
        if (ok) ok = hom_spectrum(e, Gp, V, l1, l3);
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) { sG[k] = Gp[k]; sGf[k] = (float)Gp[k]; sW[k / 3][k % 3] = V[k / 3][k % 3]; }
            sL[0] = l1; sL[1] = l3;
            s_ok = 1;
        }
    }
    wg_barrier();
    bool ok = s_ok != 0;                                // workgroup-uniform

    // ---- the sign vote ---------------------------------------------------------------------------------------------------------------
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const uint8_t* inl = inlier + lo;
    const EpiNorm nm = epi_norm(norm, p);
    if (ok) {
        float g[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) g[k] = sGf[k];
        int cnt[3] = {0, 0, 0};                         // used, q > 0, q < 0
        for (uint32_t i0 = 0; i0 < n; i0 += HPOSE_THREADS) {
            float l0, l1, r0, r1;
            epi_load_masked(ml, mr, inl, i0 + tid, n, norm != nullptr, nm, l0, l1, r0, r1);
            const float a0 = __builtin_fmaf(g[0], l0, __builtin_fmaf(g[1], l1, g[2]));
            const float a1 = __builtin_fmaf(g[3], l0, __builtin_fmaf(g[4], l1, g[5]));
            const float a2 = __builtin_fmaf(g[6], l0, __builtin_fmaf(g[7], l1, g[8]));
            const float q = __builtin_fmaf(r0, a0, __builtin_fmaf(r1, a1, a2));
            cnt[0] += wave_count(l0 == l0);
            cnt[1] += wave_count(q > 0.0f);
            cnt[2] += wave_count(q < 0.0f);
        }
        wave_parts_store(s_cnt, wave, lane, cnt);
    }
    wg_barrier();

    // ---- the candidates ----------------------------------------------------------------------------------------------------------------
    if (tid == 0 && ok) {
        const int pos = wave_parts_total(s_cnt, 1), neg = wave_parts_total(s_cnt, 2);
        double Gp[9], V[3][3];
#pragma unroll
        for (int k = 0; k < 9; ++k) { Gp[k] = neg > pos ? -sG[k] : sG[k]; V[k / 3][k % 3] = sW[k / 3][k % 3]; }
        const double l1 = sL[0], l3 = sL[1];
        const double base = __builtin_sqrt(l1) - __builtin_sqrt(l3);
        bool good = __builtin_isfinite(base);
        int status = 0;
        if (good && (l1 - l3 <= 0.0 || base <= min_baseline)) {
            double R[9];
            good = l3 > 0.0 && hom_rotation(Gp, V, l1, l3, R);
            if (good) {
#pragma unroll
                for (int k = 0; k < 9; ++k) sR[0][k] = R[k];
                status = 2;
            }
        } else if (good) {
            double R[2][9], t[2][3], nn[2][3], E[2][9];
            good = hom_decompose(Gp, V, l1, l3, R, t, nn, E);
            if (good) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) { sR[c][k] = R[c][k]; sE[c][k] = E[c][k]; sEf[c][k] = (float)E[c][k]; }
#pragma unroll
                    for (int k = 0; k < 3; ++k) { sT[c][k] = t[c][k]; sN[c][k] = nn[c][k]; sNf[c][k] = (float)nn[c][k]; }
                }
                status = 1;
            }
        }
        sBase = good ? base : 0.0;
        s_status = status;
    }
    wg_barrier();
    const int status = s_status;                        // workgroup-uniform; 0: no pose
    ok = status != 0;

    // ---- visibility and support --------------------------------------------------------------------------------------------------------
    float nf[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    if (status == 1) {
        float ef[2][9];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int k = 0; k < 9; ++k) ef[c][k] = sEf[c][k];
#pragma unroll
            for (int k = 0; k < 3; ++k) nf[c][k] = sNf[c][k];
        }
        const float th = thr ? thr[p] : -1.0f;
        const bool support = th >= 0.0f;                // false for a NaN
        const float t2 = th * th;
        int cnt[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t i0 = 0; i0 < n; i0 += HPOSE_THREADS) {
            float l0, l1, r0, r1;                       // the support is every finite match's: f0 is l0 before the mask
            const float f0 = epi_load_masked(ml, mr, inl, i0 + tid, n, norm != nullptr, nm, l0, l1, r0, r1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float d = hpose_side(nf[c], l0, l1);
                cnt[c] += wave_count(d > 0.0f);
                cnt[2 + c] += wave_count(d < 0.0f);
                if (support) {                          // workgroup-uniform
                    v2f s, lim, w;
                    Epipolar::test2(ef[c], t2, pk_splat(f0), pk_splat(l1), pk_splat(r0), pk_splat(r1), s, lim, w);
                    cnt[4 + c] += wave_count(w.x > 0.0f && s.x <= lim.x);
                }
            }
        }
        wave_parts_store(s_cnt, wave, lane, cnt, 2);   // column 0 keeps the used count
    }
    wg_barrier();
    if (tid == 0) {
        int vis[4] = {0, 0, 0, 0}, sup[4] = {0, 0, 0, 0};
        int ch = 0;
        if (status == 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { vis[c] = wave_parts_total(s_cnt, 2 + c); sup[c] = wave_parts_total(s_cnt, 6 + (c & 1)); }
#pragma unroll
            for (int c = 1; c < 4; ++c)
                if (vis[c] > vis[ch] || (vis[c] == vis[ch] && sup[c] > sup[ch])) ch = c;
        } else if (status == 2) {
#pragma unroll
            for (int c = 0; c < 4; ++c) vis[c] = wave_parts_total(s_cnt, 0);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) { vis_out[p * 4 + c] = vis[c]; sup_out[p * 4 + c] = sup[c]; }
        choice_out[p] = ch;
        status_out[p] = status;
        front_count[p] = (int64_t)vis[ch];
        baseline_out[p] = ok ? sBase : 0.0;
        s_choice = ch;
    }
    wg_barrier();
    const int ch = s_choice;
    if (tid < 9) {                                      // the pose in the reference's frame: P R P, P t, P n
        const int i = tid / 3, j = tid - 3 * i;
        const int si = frame_perm(i, swapped), k = hom_perm(tid, swapped);
        R_out[p * 9 + tid] = ok ? sR[ch & 1][k] : (i == j ? 1.0 : 0.0);
        if (j == 0) {
            double tv = 0.0, nv = 0.0;
            if (status == 1) {
                const double t0 = sT[ch & 1][0], t1 = sT[ch & 1][1], t2 = sT[ch & 1][2];
                const double tn = __builtin_sqrt(t0 * t0 + t1 * t1 + t2 * t2);          // > 0: hom_decompose checked it
                tv = sT[ch & 1][si] / tn;
                nv = sN[ch & 1][si];
                if (ch & 2) { tv = -tv; nv = -nv; }
            }
            t_out[p * 3 + i] = tv;
            n_out[p * 3 + i] = nv;
        }
        if (cand_R) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                cand_R[(p * 2 + c) * 9 + tid] = status == 1 ? sR[c][k] : (status == 2 ? sR[0][k] : (i == j ? 1.0 : 0.0));
                if (j == 0) {
                    cand_t[(p * 2 + c) * 3 + i] = status == 1 ? sT[c][si] : 0.0;
                    cand_n[(p * 2 + c) * 3 + i] = status == 1 ? sN[c][si] : 0.0;
                }
            }
        }
    }
    if (tid == 64) {                                    // E, its sign judged on the values written
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = status == 1 ? sE[ch & 1][k] : 0.0;
        hom_write(E, status == 1, swapped, E_out + p * 9);
    }

    // ---- mask ------------------------------------------------------------------------------------------------------------------------
    if (!front || !ok) return;                          // the mask was zeroed before the launch
    for (uint32_t i0 = 0; i0 < n; i0 += HPOSE_THREADS) {
        const uint32_t i = i0 + tid;
        float l0, l1, r0, r1;
        epi_load_masked(ml, mr, inl, i, n, norm != nullptr, nm, l0, l1, r0, r1);
        bool bit = l0 == l0;                            // rotation only: every used match
        if (status == 1) {
            const float d = hpose_side(nf[ch & 1], l0, l1);
            bit = (ch & 2) ? d < 0.0f : d > 0.0f;
        }
        if (i < n) front[lo + i] = bit ? (uint8_t)1 : (uint8_t)0;
    }
}

// branch per pair and the chosen branch's pose and masks; one workgroup per pair
__global__ void __launch_bounds__(SELECT_THREADS)
pose_select_kernel(const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                   const double* __restrict__ R_e, const double* __restrict__ t_e, const double* __restrict__ E_e,
                   const int64_t* __restrict__ fc_e, const uint8_t* __restrict__ front_e, const int64_t* __restrict__ bc_e,
                   const uint8_t* __restrict__ inl_e, const double* __restrict__ R_h, const double* __restrict__ t_h,
                   const double* __restrict__ E_h, const int64_t* __restrict__ fc_h, const uint8_t* __restrict__ front_h,
                   const int32_t* __restrict__ status_h, const int64_t* __restrict__ bc_h, const uint8_t* __restrict__ inl_h,
                   const float* __restrict__ ratio, double* __restrict__ R, double* __restrict__ t, double* __restrict__ E,
                   int64_t* __restrict__ front_count, int32_t* __restrict__ branch_out, uint8_t* __restrict__ inlier_sel,
                   uint8_t* __restrict__ front_sel) {
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const int64_t ce = bc_e[p], chh = bc_h[p];
    const int sh = status_h[p];
    const bool epi_ok = ce >= POSE_MIN_INLIERS, planar_ok = sh != 0;
    const bool planar = planar_ok && (!epi_ok || (double)chh >= (double)ratio[p] * (double)ce);       // false for a NaN ratio
    const int branch = planar ? (sh == 2 ? 3 : 2) : (epi_ok ? 1 : 0);                                  // workgroup-uniform
    if (tid < 9) {
        const int i = tid / 3, j = tid - 3 * i;
        R[p * 9 + tid] = branch == 0 ? (i == j ? 1.0 : 0.0) : (planar ? R_h[p * 9 + tid] : R_e[p * 9 + tid]);
        E[p * 9 + tid] = branch == 0 ? 0.0 : (planar ? E_h[p * 9 + tid] : E_e[p * 9 + tid]);
        if (tid < 3) t[p * 3 + tid] = branch == 0 ? 0.0 : (planar ? t_h[p * 3 + tid] : t_e[p * 3 + tid]);
    }
    if (tid == 0) {
        branch_out[p] = branch;
        front_count[p] = branch == 0 ? 0 : (planar ? fc_h[p] : fc_e[p]);
    }
    if (branch == 0) return;                            // the masks were zeroed before the launch
    const uint8_t* inl = planar ? inl_h : inl_e;
    const uint8_t* fr = planar ? front_h : front_e;
    for (uint32_t i = tid; i < n; i += SELECT_THREADS) {
        inlier_sel[lo + i] = inl[lo + i];
        if (front_sel) front_sel[lo + i] = fr[lo + i];
    }
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_homography_pose_workspace_bytes(int64_t pairs, int64_t cap) {
    (void)pairs; (void)cap;
    return 0;                                           // the solve lives in LDS and registers, the mask is a third walk
}

extern "C" int pats_homography_pose_by_pair_f64(const float* matches_l, const float* matches_r, const uint8_t* inlier, const int64_t* pair_off,
                                                int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap,
                                                const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                                const int32_t* best, const float* norm, const float* thr, int swapped, double min_baseline,
                                                double* E, double* R, double* t, double* n, double* baseline, int32_t* vis, int32_t* sup,
                                                int32_t* choice, int32_t* status, int64_t* front_count, double* cand_R, double* cand_t,
                                                double* cand_n, uint8_t* front, void* workspace, size_t workspace_bytes,
                                                pats_stream_t stream) {
    (void)workspace;
    const char* who = "homography_pose_by_pair";
    int rc = epi_check_args(who, {{"matches_l", matches_l, 8}, {"matches_r", matches_r, 8}, {"inlier", inlier, 1}, {"best_count", best_count, 8},
                                  {"E", E, 8}, {"R", R, 8}, {"t", t, 8}, {"n", n, 8}, {"baseline", baseline, 8}, {"vis", vis, 4}, {"sup", sup, 4},
                                  {"choice", choice, 4}, {"status", status, 4}, {"front_count", front_count, 8}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"moments", moments, 8}, {"models", models, 4}, {"best", best, 4}, {"norm", norm, 4}, {"thr", thr, 4},
                              {"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}, {"cand_R", cand_R, 8}, {"cand_t", cand_t, 8},
                              {"cand_n", cand_n, 8}}, false);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE((cand_R != nullptr) == (cand_t != nullptr) && (cand_R != nullptr) == (cand_n != nullptr),
                 "%s: cand_R, cand_t and cand_n must be given together", who);
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    if ((rc = epi_check_refit_source(who, moments, models, best, H, swapped)) != PATS_OK) return rc;
    PATS_REQUIRE(min_baseline >= 0.0, "%s: min_baseline = %g must be a number >= 0", who, min_baseline);     // false for a NaN
    PATS_REQUIRE(workspace_bytes >= pats_homography_pose_workspace_bytes(pairs, cap), "%s: workspace too small", who);
    hipStream_t st = as_stream(stream);
    if (front) {
        rc = fill_bytes(front, 0, (size_t)cap, st);
        if (rc != PATS_OK) return rc;
    }
    hipLaunchKernelGGL(homography_pose_kernel, dim3((unsigned)pairs), dim3(HPOSE_THREADS), 0, st, matches_l, matches_r, inlier, pair_off,
                       counts_in, stride, cap, best_count, moments, models, (int)H, best, norm, thr, swapped,
                       min_baseline, E, R, t, n, baseline, vis, sup, choice, status, front_count, cand_R, cand_t, cand_n, front);
    return check_launch("homography_pose kernel");
}

extern "C" size_t pats_pose_select_workspace_bytes(int64_t pairs, int64_t cap) {
    (void)pairs; (void)cap;
    return 0;
}

extern "C" int pats_pose_select_by_pair(const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap,
                                        const double* R_e, const double* t_e, const double* E_e, const int64_t* front_count_e,
                                        const uint8_t* front_e, const int64_t* best_count_e, const uint8_t* inlier_e, const double* R_h,
                                        const double* t_h, const double* E_h, const int64_t* front_count_h, const uint8_t* front_h,
                                        const int32_t* status_h, const int64_t* best_count_h, const uint8_t* inlier_h, const float* ratio,
                                        double* R, double* t, double* E, int64_t* front_count, int32_t* branch, uint8_t* inlier_sel,
                                        uint8_t* front_sel, void* workspace, size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    const char* who = "pose_select_by_pair";
    int rc = epi_check_args(who, {{"R_e", R_e, 8}, {"t_e", t_e, 8}, {"E_e", E_e, 8}, {"front_count_e", front_count_e, 8},
                                  {"best_count_e", best_count_e, 8}, {"inlier_e", inlier_e, 1}, {"R_h", R_h, 8}, {"t_h", t_h, 8}, {"E_h", E_h, 8},
                                  {"front_count_h", front_count_h, 8}, {"status_h", status_h, 4}, {"best_count_h", best_count_h, 8},
                                  {"inlier_h", inlier_h, 1}, {"ratio", ratio, 4}, {"R", R, 8}, {"t", t, 8}, {"E", E, 8},
                                  {"front_count", front_count, 8}, {"branch", branch, 4}, {"inlier_sel", inlier_sel, 1}}, true);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_args(who, {{"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}}, false)) != PATS_OK) return rc;
    PATS_REQUIRE(!front_sel || (front_e && front_h), "%s: front_sel needs front_e and front_h", who);
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_pose_select_workspace_bytes(pairs, cap), "%s: workspace too small", who);
    hipStream_t st = as_stream(stream);
    int rf = fill_bytes(inlier_sel, 0, (size_t)cap, st);
    if (rf != PATS_OK) return rf;
    if (front_sel) {
        rf = fill_bytes(front_sel, 0, (size_t)cap, st);
        if (rf != PATS_OK) return rf;
    }
    hipLaunchKernelGGL(pose_select_kernel, dim3((unsigned)pairs), dim3(SELECT_THREADS), 0, st, pair_off, counts_in, stride, cap, R_e, t_e, E_e,
                       front_count_e, front_e, best_count_e, inlier_e, R_h, t_h, E_h, front_count_h, front_h, status_h, best_count_h, inlier_h,
                       ratio, R, t, E, front_count, branch, inlier_sel, front_sel);
    return check_launch("pose_select kernel");
}
