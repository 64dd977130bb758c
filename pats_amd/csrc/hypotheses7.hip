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
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    float* mo = models + (p * H + h) * (F7_MAX_MODELS * 9);
    int32_t* so = sample_idx ? sample_idx + (p * H + h) * 7 : nullptr;
    int32_t* no = n_models ? n_models + (p * H + h) : nullptr;
    if (n < 7) {                                        // workgroup-uniform: zero models, no sample
        for (int k = 0; k < F7_MAX_MODELS * 9; ++k) mo[k] = 0.0f;
        if (so) {
#pragma unroll
            for (int t = 0; t < 7; ++t) so[t] = -1;
        }
        if (no) *no = 0;
        return;
    }
    uint32_t m = n;                                     // the pool: 7 <= m <= n
    if (progressive) {
        const int64_t q = ((int64_t)n * (h + 1) + H - 1) / H;
        m = q < 7 ? 7u : (q > (int64_t)n ? n : (uint32_t)q);
    }
    uint32_t idx[7];                                    // the draws in draw order
    epi_draw<7>((uint64_t)pair_seed[p], (uint32_t)h, m, idx);
    if (so) {
#pragma unroll
        for (int t = 0; t < 7; ++t) so[t] = (int32_t)idx[t];
    }
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const EpiNorm nm = epi_norm(norm, p);
    double l0[7], l1[7], r0[7], r1[7];
    bool finite = true;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        float2 a = ml[idx[t]], c = mr[idx[t]];          // idx < m <= n: inside the segment
        if (norm) {                                     // one subtract, one multiply (no contraction: -ffp-contract=off)
            a.x = (a.x - nm.c0l) * nm.s0l; a.y = (a.y - nm.c1l) * nm.s1l;
            c.x = (c.x - nm.c0r) * nm.s0r; c.y = (c.y - nm.c1r) * nm.s1r;
        }
        finite = finite && __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(c.x) && __builtin_isfinite(c.y);
        l0[t] = (double)a.x; l1[t] = (double)a.y; r0[t] = (double)c.x; r1[t] = (double)c.y;
    }
    int count = 0;
    if (finite) count = f7_solve(l0, l1, r0, r1, mo);
    for (int k = count * 9; k < F7_MAX_MODELS * 9; ++k) mo[k] = 0.0f;
    if (no) *no = count;
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
    PATS_REQUIRE_PTR("epipolar_hypotheses7_by_pair", matches_l, 8);
    PATS_REQUIRE_PTR("epipolar_hypotheses7_by_pair", matches_r, 8);
    PATS_REQUIRE_PTR("epipolar_hypotheses7_by_pair", pair_seed, 8);
    PATS_REQUIRE_PTR("epipolar_hypotheses7_by_pair", models, 4);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses7_by_pair", norm, 4);    // optional pointers: null is aligned
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses7_by_pair", sample_idx, 4);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses7_by_pair", n_models, 4);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses7_by_pair", pair_off, 8);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses7_by_pair", counts_in, 8);
    int rc = epi_check_segments("epipolar_hypotheses7_by_pair", pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h("epipolar_hypotheses7_by_pair", H);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(H <= pats_epipolar_max_h() / F7_MAX_MODELS, "epipolar_hypotheses7_by_pair: H = %lld gives 3 H = %lld models (<= max_h = %lld)",
                 (long long)H, (long long)(H * F7_MAX_MODELS), (long long)pats_epipolar_max_h());
    PATS_REQUIRE(progressive == 0 || progressive == 1, "epipolar_hypotheses7_by_pair: progressive = %d must be 0 or 1", progressive);
    PATS_REQUIRE(workspace_bytes >= pats_epipolar_hypotheses7_workspace_bytes(pairs, H), "epipolar_hypotheses7_by_pair: workspace too small");
    const int64_t chunks = ceil_div(H, F7_THREADS);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "epipolar_hypotheses7_by_pair: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)",
                 (long long)pairs, (long long)pairs, (long long)chunks);
    hipLaunchKernelGGL(epipolar_hypotheses7_kernel, dim3((unsigned)(pairs * chunks)), dim3(F7_THREADS), 0, as_stream(stream), matches_l,
                       matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models, sample_idx,
                       n_models);
    return check_launch("epipolar_hypotheses7 kernel");
}
