// Per-pair 7-point hypotheses, the uncalibrated sibling of hypotheses5.hip: for every pair and every sample h in 0 .. H-1 seven
// distinct matches of the pair's segment are drawn with the hypotheses' sampler (epi_draw of epipolar.hpp) and the real fundamental
// matrices through them - at most three, rank 2 by construction - are written as row-major 3x3 float32 models, compacted into the
// sample's lowest slots, the rest zero.  One launch, no host read, no workspace, deterministic.  include/pats_amd.h states the
// definition ("Per-pair 7-point hypotheses"), fundamental7.hpp holds the solver (float64 throughout), docs/kernels.md 4.14 the design
// and the measurements.
//
//   one THREAD per sample, 64 samples (one wave) per workgroup, grid = pairs x ceil(H / 64)
//   storage  the 9x7 float64 matrix of the Householder factorisation is indexed statically once its loops are unrolled: it lives in
//            registers (126 of the 512 a lane has at one wave per SIMD), and so do the basis and the cubic.  No LDS
//   figures  (-Rpass-analysis=kernel-resource-usage, gfx950) are in docs/kernels.md 4.14: no scratch, no spill
//   loops    every loop has a constant trip cap (fundamental7.hpp: 64 safeguarded Newton steps per root, 6 monotone pieces)
#include "common.hpp"
#include "epipolar.hpp"
#include "fundamental7.hpp"

namespace pats {

constexpr int F7_THREADS = 64;                         // samples per workgroup: one wave

__global__ void __launch_bounds__(F7_THREADS)
epipolar_hypotheses7_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                            const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks, int H,
                            const int64_t* __restrict__ pair_seed, const float* __restrict__ norm, int progressive,
                            float* __restrict__ models, int32_t* __restrict__ sample_idx, int32_t* __restrict__ n_models) {
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h = (int)(b % (uint32_t)chunks) * F7_THREADS + (int)threadIdx.x;
    if (h >= H) return;
    float* mo = models + (p * H + h) * (F7_MAX_MODELS * 9);
    double l0[7], l1[7], r0[7], r1[7];
    const EpiSample drawn = epi_sample<7>(ml_, mr_, pair_off, counts_in, stride, cap, pair_seed, norm, progressive, sample_idx, p, h, H, l0,
                                          l1, r0, r1);
    int count = 0;
    if (drawn == EPI_SAMPLE_READY) count = f7_solve(l0, l1, r0, r1, mo);
    for (int k = count * 9; k < F7_MAX_MODELS * 9; ++k) mo[k] = 0.0f;     // every slot of a short pair or a non-finite sample
    if (n_models) n_models[p * H + h] = count;
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_epipolar_hypotheses7_workspace_bytes(int64_t pairs, int64_t H) {
    (void)pairs; (void)H;
    return 0;                                           // a sample lives in its thread's registers
}

extern "C" int pats_epipolar_hypotheses7_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                     const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                     const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                     int32_t* sample_idx, int32_t* n_models, void* workspace, size_t workspace_bytes,
                                                     pats_stream_t stream) {
    (void)workspace;
    int64_t chunks;
    const int rc = epi_check_hypotheses("epipolar_hypotheses7_by_pair", {"matches_l", matches_l, 8}, matches_r, pair_off, stride, counts_in, pairs, cap,
                                        H, pair_seed, norm, progressive, models, sample_idx, n_models, F7_MAX_MODELS, F7_THREADS, chunks);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_epipolar_hypotheses7_workspace_bytes(pairs, H), "epipolar_hypotheses7_by_pair: workspace too small");
    hipLaunchKernelGGL(epipolar_hypotheses7_kernel, dim3((unsigned)(pairs * chunks)), dim3(F7_THREADS), 0, as_stream(stream), matches_l,
                       matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models, sample_idx,
                       n_models);
    return check_launch("epipolar_hypotheses7 kernel");
}
