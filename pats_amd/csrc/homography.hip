// Per-pair homographies on the hand-over's matches - the planar sibling of the epipolar stages.  This file holds what only that
// branch has: the least-squares refit of the winner's inliers with its denormalisation.  The 4-point hypotheses are hypotheses.hip's
// FourPoint family, the verification (squared forward transfer error against thr^2, without the division) epipolar.hip's Homography
// family.  No host read anywhere.  include/pats_amd.h states the definition ("Per-pair homographies"); docs/kernels.md 4.11 the design.
//
//   refit       one wave per pair, float64: the round-robin cyclic Jacobi of jacobi9.hpp on the moments in LDS (shared with pose.hip),
//               the two smallest eigenvalues, the eigenvector, the sign rule (refit.hpp, shared with polish.hip), the denormalisation
//               and the permutation
#include "common.hpp"
#include "epipolar.hpp"
#include "jacobi9.hpp"
#include "refit.hpp"

namespace pats {

constexpr int HOM_REFIT_THREADS = 64;

__global__ void __launch_bounds__(HOM_REFIT_THREADS)
homography_refit_kernel(const int64_t* __restrict__ best_count, const double* __restrict__ moments, const float* __restrict__ models,
                        int H, const int32_t* __restrict__ best, const float* __restrict__ norm, int swapped,
                        double* __restrict__ H_out, double* __restrict__ Hpx_out, double* __restrict__ eig_out) {
    __shared__ double sA[9][9], sV[9][9];
    __shared__ int s_bad, s_rot;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const bool live = best_count[p] >= HOM_MIN_INLIERS; // workgroup-uniform
    if (tid == 0) { s_bad = 0; s_rot = 0; }
    wg_barrier();
    if (live && moments)                                // workgroup-uniform
        refit_solve<HOM_REFIT_THREADS>(moments, p, sA, sV, s_bad, s_rot, tid, (tid & 15) < 9, HOM_SWEEPS);
    wg_barrier();
    if (tid != 0) return;
    double e[9], ev[2] = {0.0, 0.0}, lmin;
    int m;
    bool ok = refit_source(live && s_bad == 0, moments, sA, sV, models, H, best, p, e, m, lmin);
    if (ok && moments) ok = refit_spectrum(sA, m, lmin, ev);
    if (ok) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < 9; ++k) { ok = ok && __builtin_isfinite(e[k]); any = any || e[k] != 0.0; }
        ok = ok && any;                                 // the zero model is no model
    }
    hom_write(e, ok, swapped, H_out + p * 9);
    eig_out[p * 2] = ok ? ev[0] : 0.0;
    eig_out[p * 2 + 1] = ok ? ev[1] : 0.0;
    if (!Hpx_out) return;
    double g[9];
    bool okp = ok;
    if (ok) {
        const EpiNorm nm = epi_norm(norm, p);           // float32, widened exactly; the identity without norm
        const double c0r = nm.c0r, c1r = nm.c1r, s0r = nm.s0r, s1r = nm.s1r;
        if (norm) {
            double q[9];                                // H N_l
            refit_times_nl(e, nm.c0l, nm.c1l, nm.s0l, nm.s1l, q);
#pragma unroll
            for (int j = 0; j < 3; ++j) {               // N_r^-1 (H N_l),  N_r^-1 = [[1/s0, 0, c0], [0, 1/s1, c1], [0, 0, 1]]
                g[j] = q[j] / s0r + c0r * q[6 + j];
                g[3 + j] = q[3 + j] / s1r + c1r * q[6 + j];
                g[6 + j] = q[6 + j];
            }
            okp = refit_unit(g);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) g[k] = e[k];
        }
    }
    hom_write(g, okp, swapped, Hpx_out + p * 9);
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_homography_refit_workspace_bytes(int64_t pairs) {
    (void)pairs;
    return 0;                                           // the solve lives in LDS and registers
}

extern "C" int pats_homography_refit_by_pair_f64(const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                                 const int32_t* best, const float* norm, int64_t pairs, int swapped, double* H_out,
                                                 double* H_px, double* eig, void* workspace, size_t workspace_bytes,
                                                 pats_stream_t stream) {
    (void)workspace;
    const char* who = "homography_refit_by_pair";
    int rc = epi_check_args(who, {{"best_count", best_count, 8}, {"H_out", H_out, 8}, {"eig", eig, 8}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"moments", moments, 8}, {"models", models, 4}, {"best", best, 4}, {"norm", norm, 4}, {"H_px", H_px, 8}}, false);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(pairs >= 1 && pairs <= 0x7fffffff, "%s: pairs = %lld (1 .. 2^31 - 1)", who, (long long)pairs);
    if ((rc = epi_check_refit_source(who, moments, models, best, H, swapped)) != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_homography_refit_workspace_bytes(pairs), "%s: workspace too small", who);
    hipLaunchKernelGGL(homography_refit_kernel, dim3((unsigned)pairs), dim3(HOM_REFIT_THREADS), 0, as_stream(stream), best_count, moments,
                       models, (int)H, best, norm, swapped, H_out, H_px, eig);
    return check_launch("homography_refit kernel");
}
