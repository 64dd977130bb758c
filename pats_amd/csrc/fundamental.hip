// Per-pair fundamental matrices on the hand-over's matches - the uncalibrated result of the epipolar stages.  This file holds what
// only that branch has: the least-squares refit of the winner's inliers projected onto rank 2, with its denormalisation.  The 7-point
// hypotheses are hypotheses7.hip, the verification epipolar.hip's Epipolar family (the Sampson test does not care what the model is),
// the local optimisation polish.hip's Fundamental family.  No host read anywhere.  include/pats_amd.h states the definition
// ("Per-pair fundamental matrices"); docs/kernels.md 4.14 the design.
//
//   refit       one wave per pair, float64, the launch shape of the homography refit: the round-robin cyclic Jacobi of jacobi9.hpp
//               on the moments in LDS, the two smallest eigenvalues and the eigenvector, its rank-2 truncation by a 3x3 Jacobi in
//               registers (refit.hpp, shared with polish.hip), the denormalisation N_r^T F N_l, the permutation and the sign rule
#include "common.hpp"
#include "epipolar.hpp"
#include "jacobi9.hpp"
#include "refit.hpp"

namespace pats {

constexpr int FUND_REFIT_THREADS = 64;

__global__ void __launch_bounds__(FUND_REFIT_THREADS)
fundamental_refit_kernel(const int64_t* __restrict__ best_count, const double* __restrict__ moments, const float* __restrict__ models,
                         int H, const int32_t* __restrict__ best, const float* __restrict__ norm, int swapped,
                         double* __restrict__ F_out, double* __restrict__ Fpx_out, double* __restrict__ eig_out,
                         double* __restrict__ sigma_out, double* __restrict__ refit_out) {
    __shared__ double sA[9][9], sV[9][9];
    __shared__ int s_bad, s_rot;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const bool live = best_count[p] >= FUND_MIN_INLIERS;    // workgroup-uniform
    if (tid == 0) { s_bad = 0; s_rot = 0; }
    wg_barrier();
    if (live && moments)                                // workgroup-uniform
        refit_solve<FUND_REFIT_THREADS>(moments, p, sA, sV, s_bad, s_rot, tid, (tid & 15) < 9, FUND_SWEEPS);
    wg_barrier();
    if (tid != 0) return;
    double e[9] = {}, F[9] = {}, sig[3] = {}, ev[2] = {0.0, 0.0}, lmin;
    int m;
    bool ok = refit_source(live && s_bad == 0, moments, sA, sV, models, H, best, p, e, m, lmin);
    if (ok && moments) ok = refit_spectrum(sA, m, lmin, ev);
    ok = ok && fund_project(e, F, sig);                 // the zero model has rank 0: no model
    hom_write(F, ok, swapped, F_out + p * 9);
    eig_out[p * 2] = ok ? ev[0] : 0.0;
    eig_out[p * 2 + 1] = ok ? ev[1] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) sigma_out[p * 3 + k] = ok ? sig[k] : 0.0;
    if (refit_out) {
#pragma unroll
        for (int k = 0; k < 9; ++k) refit_out[p * 9 + k] = ok ? e[k] : 0.0;
    }
    if (!Fpx_out) return;
    double g[9];
    bool okp = ok;
    if (ok) {
        const EpiNorm nm = epi_norm(norm, p);           // float32, widened exactly; the identity without norm
        const double s0l = nm.s0l, s1l = nm.s1l, c0r = nm.c0r, c1r = nm.c1r, s0r = nm.s0r, s1r = nm.s1r;
        if (norm) {
            double q[9];                                // F N_l
            refit_times_nl(F, nm.c0l, nm.c1l, s0l, s1l, q);
#pragma unroll
            for (int j = 0; j < 3; ++j) {               // N_r^T (F N_l),  N_r^T = [[s0, 0, 0], [0, s1, 0], [-c0 s0, -c1 s1, 1]]
                g[j] = s0r * q[j];
                g[3 + j] = s1r * q[3 + j];
                g[6 + j] = q[6 + j] - ((c0r * s0r) * q[j] + (c1r * s1r) * q[3 + j]);
            }
            // a zero scale makes N singular: not a change of coordinates, no F_px
            okp = refit_unit(g) && s0l != 0.0 && s1l != 0.0 && s0r != 0.0 && s1r != 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) g[k] = F[k];
        }
    }
    hom_write(g, okp, swapped, Fpx_out + p * 9);
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_fundamental_refit_workspace_bytes(int64_t pairs) {
    (void)pairs;
    return 0;                                           // the solve lives in LDS and registers
}

extern "C" int pats_fundamental_refit_by_pair_f64(const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                                  const int32_t* best, const float* norm, int64_t pairs, int swapped, double* F,
                                                  double* F_px, double* eig, double* sigma, double* f_refit, void* workspace,
                                                  size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    const char* who = "fundamental_refit_by_pair";
    int rc = epi_check_args(who, {{"best_count", best_count, 8}, {"F", F, 8}, {"eig", eig, 8}, {"sigma", sigma, 8}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"moments", moments, 8}, {"models", models, 4}, {"best", best, 4}, {"norm", norm, 4}, {"F_px", F_px, 8},
                              {"f_refit", f_refit, 8}}, false);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(pairs >= 1 && pairs <= 0x7fffffff, "%s: pairs = %lld (1 .. 2^31 - 1)", who, (long long)pairs);
    if ((rc = epi_check_refit_source(who, moments, models, best, H, swapped)) != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_fundamental_refit_workspace_bytes(pairs), "%s: workspace too small", who);
    hipLaunchKernelGGL(fundamental_refit_kernel, dim3((unsigned)pairs), dim3(FUND_REFIT_THREADS), 0, as_stream(stream), best_count, moments,
                       models, (int)H, best, norm, swapped, F, F_px, eig, sigma, f_refit);
    return check_launch("fundamental_refit kernel");
}
