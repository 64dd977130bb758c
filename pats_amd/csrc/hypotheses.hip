// Per-pair minimal-sample hypotheses for the verification of epipolar.hip, both null-vector families: for every pair and every h in
// 0 .. H-1 K distinct matches of the pair's segment are drawn with a counter-based generator (a host reproduces the draws exactly)
// and the unit null vector of their 8x9 constraint matrix is written as a row-major 3x3 model.  One launch, no host read,
// deterministic.  include/pats_amd.h states the definitions; docs/kernels.md 4.8 (8-point) and 4.11 (4-point) the design.
//
//   one THREAD per hypothesis, 64 threads per workgroup, grid = pairs x ceil(H / 64).  Everything a thread holds is indexed
//   statically (every loop below is unrolled to constants), so the 9x8 matrix lives in registers: no scratch, no LDS.
//   sampler  K draws without replacement and without a rejection loop (epi_sample of epipolar.hpp, the front end of every generator)
//   solve    null_vector_9x8 of nullvec9x8.hpp: Householder QR of A^T and one step of iterative refinement.  The plain QR vector
//            alone sits at ~1.1 eps32 |A|_F in the worst of 2100 8-point samples; with the step at ~0.2 (docs/parity.md)
//   family   a struct with the sample size K, fill (A^T from the draws) and residual (column j of A^T times z through the factored
//            form of the constraint):
//            EightPoint  epipolar, K = 8: column t = vec(x_r x_l^T) of draw t, its residual x_r . (Z x_l)
//            FourPoint   homography, K = 4: columns 2t and 2t + 1 = the DLT rows A_t and B_t of draw t, A_t z = r0 a2 - a0,
//                        B_t z = r1 a2 - a1 with a = Z x_l
// A vector that is not finite at the end (coordinates whose squares overflow float32) is written as the zero model.
#include "common.hpp"
#include "epipolar.hpp"
#include "nullvec9x8.hpp"

namespace pats {

constexpr int HYP_THREADS = 64;                        // hypotheses per workgroup: one wave

struct EightPoint {
    static constexpr int K = 8;
    static constexpr const char* KERNEL = "epipolar_hypotheses kernel";
    // A^T: column t = q of draw t, q[3i + j] = x_r[i] x_l[j]
    static __device__ __forceinline__ void fill(float (&M)[9][8], const float (&l0)[K], const float (&l1)[K], const float (&r0)[K],
                                                const float (&r1)[K]) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            M[0][t] = r0[t] * l0[t]; M[1][t] = r0[t] * l1[t]; M[2][t] = r0[t];
            M[3][t] = r1[t] * l0[t]; M[4][t] = r1[t] * l1[t]; M[5][t] = r1[t];
            M[6][t] = l0[t];         M[7][t] = l1[t];         M[8][t] = 1.0f;
        }
    }
    static __device__ __forceinline__ float residual(const float (&z)[9], const float (&l0)[K], const float (&l1)[K], const float (&r0)[K],
                                                     const float (&r1)[K], int t) {
        const float a0 = __builtin_fmaf(z[0], l0[t], __builtin_fmaf(z[1], l1[t], z[2]));
        const float a1 = __builtin_fmaf(z[3], l0[t], __builtin_fmaf(z[4], l1[t], z[5]));
        const float a2 = __builtin_fmaf(z[6], l0[t], __builtin_fmaf(z[7], l1[t], z[8]));
        return __builtin_fmaf(r0[t], a0, __builtin_fmaf(r1[t], a1, a2));
    }
};

struct FourPoint {
    static constexpr int K = 4;
    static constexpr const char* KERNEL = "homography_hypotheses kernel";
    // A^T: column 2t = A_t, column 2t + 1 = B_t of draw t
    static __device__ __forceinline__ void fill(float (&M)[9][8], const float (&l0)[K], const float (&l1)[K], const float (&r0)[K],
                                                const float (&r1)[K]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            M[0][2 * t] = -l0[t];         M[1][2 * t] = -l1[t];         M[2][2 * t] = -1.0f;
            M[3][2 * t] = 0.0f;           M[4][2 * t] = 0.0f;           M[5][2 * t] = 0.0f;
            M[6][2 * t] = r0[t] * l0[t];  M[7][2 * t] = r0[t] * l1[t];  M[8][2 * t] = r0[t];
            M[0][2 * t + 1] = 0.0f;          M[1][2 * t + 1] = 0.0f;          M[2][2 * t + 1] = 0.0f;
            M[3][2 * t + 1] = -l0[t];        M[4][2 * t + 1] = -l1[t];        M[5][2 * t + 1] = -1.0f;
            M[6][2 * t + 1] = r1[t] * l0[t]; M[7][2 * t + 1] = r1[t] * l1[t]; M[8][2 * t + 1] = r1[t];
        }
    }
    static __device__ __forceinline__ float residual(const float (&z)[9], const float (&l0)[K], const float (&l1)[K], const float (&r0)[K],
                                                     const float (&r1)[K], int j) {
        const int t = j >> 1;
        const float a0 = __builtin_fmaf(z[0], l0[t], __builtin_fmaf(z[1], l1[t], z[2]));
        const float a1 = __builtin_fmaf(z[3], l0[t], __builtin_fmaf(z[4], l1[t], z[5]));
        const float a2 = __builtin_fmaf(z[6], l0[t], __builtin_fmaf(z[7], l1[t], z[8]));
        return (j & 1) ? __builtin_fmaf(r1[t], a2, -a1) : __builtin_fmaf(r0[t], a2, -a0);
    }
};

template <class F>
__global__ void __launch_bounds__(HYP_THREADS)
hypotheses_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                  const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks, int H,
                  const int64_t* __restrict__ pair_seed, const float* __restrict__ norm, int progressive,
                  float* __restrict__ models, int32_t* __restrict__ sample_idx) {
    constexpr int K = F::K;
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h = (int)(b % (uint32_t)chunks) * HYP_THREADS + (int)threadIdx.x;
    if (h >= H) return;
    float* mo = models + (p * H + h) * 9;
    float l0[K], l1[K], r0[K], r1[K];
    const EpiSample drawn = epi_sample<K>(ml_, mr_, pair_off, counts_in, stride, cap, pair_seed, norm, progressive, sample_idx, p, h, H, l0,
                                          l1, r0, r1);
    float e[9];
    bool ok = false;
    if (drawn == EPI_SAMPLE_READY) {
        float M[9][8];
        F::fill(M, l0, l1, r0, r1);
        ok = null_vector_9x8(M, [&](const float (&z)[9], int j) { return F::residual(z, l0, l1, r0, r1, j); }, e);
    }
    if (!ok) {                                          // a short pair, a non-finite coordinate or vector: the zero model
#pragma unroll
        for (int k = 0; k < 9; ++k) mo[k] = 0.0f;
        return;
    }
    float big = __builtin_fabsf(e[0]), at = e[0];       // the component of largest magnitude (the lowest index among equals)
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        const float v = __builtin_fabsf(e[k]);
        if (v > big) { big = v; at = e[k]; }
    }
    const bool flip = at < 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) mo[k] = flip ? -e[k] : e[k];
}

}  // namespace pats

using namespace pats;

// family F's generator; `who` = the entry point's name.  No workspace: a hypothesis lives in its thread's registers
template <class F>
static int hypotheses_by_pair(const char* who, const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                              const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed, const float* norm,
                              int progressive, float* models, int32_t* sample_idx, pats_stream_t stream) {
    int64_t chunks;
    const int rc = epi_check_hypotheses(who, {"matches_l", matches_l, 8}, matches_r, pair_off, stride, counts_in, pairs, cap, H, pair_seed, norm, progressive,
                                        models, sample_idx, nullptr, 1, HYP_THREADS, chunks);
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(hypotheses_kernel<F>, dim3((unsigned)(pairs * chunks)), dim3(HYP_THREADS), 0, as_stream(stream), matches_l,
                       matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models, sample_idx);
    return check_launch(F::KERNEL);
}

extern "C" size_t pats_epipolar_hypotheses_workspace_bytes(int64_t, int64_t) { return 0; }
extern "C" size_t pats_homography_hypotheses_workspace_bytes(int64_t, int64_t) { return 0; }

extern "C" int pats_epipolar_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                    const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                    const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                    int32_t* sample_idx, void*, size_t, pats_stream_t stream) {
    return hypotheses_by_pair<EightPoint>("epipolar_hypotheses_by_pair", matches_l, matches_r, pair_off, stride, counts_in, pairs, cap, H,
                                          pair_seed, norm, progressive, models, sample_idx, stream);
}

extern "C" int pats_homography_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off,
                                                      int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                      const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                      int32_t* sample_idx, void*, size_t, pats_stream_t stream) {
    return hypotheses_by_pair<FourPoint>("homography_hypotheses_by_pair", matches_l, matches_r, pair_off, stride, counts_in, pairs, cap, H,
                                         pair_seed, norm, progressive, models, sample_idx, stream);
}
