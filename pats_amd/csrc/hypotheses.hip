// Per-pair 8-point hypotheses for the verification of epipolar.hip: for every pair and every h in 0 .. H-1 eight distinct matches
// of the pair's segment are drawn with a counter-based generator (a host reproduces the draws exactly) and the unit null vector of
// their 8x9 epipolar constraint matrix is written as a row-major 3x3 model.  One launch, no host read, deterministic.
// include/pats_amd.h states the definition; docs/kernels.md 4.8 the design.
//
//   one THREAD per hypothesis, 64 threads per workgroup, grid = pairs x ceil(H / 64).  Everything a thread holds is indexed
//   statically (every loop below is unrolled to constants), so the 9x8 matrix lives in registers: no scratch, no LDS.
//   sampler  eight draws without replacement and without a rejection loop (epi_draw of epipolar.hpp, shared with hypotheses5.hip)
//   solve    Householder QR of A^T (9x8, column t = vec(x_r x_l^T) of draw t), no pivoting: the reflectors stay below the
//            diagonal, R on and above it.  The null vector is the last column of Q = H_0 .. H_7 e_8 - orthogonal to every column of
//            A^T whatever its rank, so a degenerate sample still gives a finite unit vector.  No component is pinned
//   refine   ONE step of iterative refinement: the residual of each draw through the factored form x_r . (E x_l) (fused multiply-
//            adds on the float32 points: the error of rounding the nine products to float32 is not in it), R^T y = res by forward
//            substitution, e -= Q (y, 0).  The plain QR vector alone sits at ~1.1 eps32 |A|_F in the worst of 2100 samples; with
//            the step at ~0.2 (docs/parity.md).  A step that does not end finite (a zero pivot) is dropped
// A vector that is not finite at the end (coordinates whose squares overflow float32) is written as the zero model.
#include "common.hpp"
#include "epipolar.hpp"

namespace pats {

constexpr int HYP_THREADS = 64;                        // hypotheses per workgroup: one wave

// z <- H_0 H_1 .. H_7 z with the reflectors H_k = I - tau_k v_k v_k^T, v_k = (1, M[k+1..8][k]) on rows k .. 8
__device__ __forceinline__ void hyp_apply_q(const float (&M)[9][8], const float (&tau)[8], float (&z)[9]) {
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
__device__ __forceinline__ bool hyp_unit(float (&z)[9]) {
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

__global__ void __launch_bounds__(HYP_THREADS)
epipolar_hypotheses_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                           const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks, int H,
                           const int64_t* __restrict__ pair_seed, const float* __restrict__ norm, int progressive,
                           float* __restrict__ models, int32_t* __restrict__ sample_idx) {
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h = (int)(b % (uint32_t)chunks) * HYP_THREADS + (int)threadIdx.x;
    if (h >= H) return;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    float* mo = models + (p * H + h) * 9;
    int32_t* so = sample_idx ? sample_idx + (p * H + h) * 8 : nullptr;
    if (n < 8) {                                        // workgroup-uniform: the zero model, no sample
#pragma unroll
        for (int k = 0; k < 9; ++k) mo[k] = 0.0f;
        if (so) {
#pragma unroll
            for (int t = 0; t < 8; ++t) so[t] = -1;
        }
        return;
    }
    uint32_t m = n;                                     // the pool: 8 <= m <= n
    if (progressive) {
        const int64_t q = ((int64_t)n * (h + 1) + H - 1) / H;
        m = q < 8 ? 8u : (q > (int64_t)n ? n : (uint32_t)q);
    }
    uint32_t idx[8];                                    // the draws in draw order (epipolar.hpp: the sampler)
    epi_draw<8>((uint64_t)pair_seed[p], (uint32_t)h, m, idx);
    if (so) {
#pragma unroll
        for (int t = 0; t < 8; ++t) so[t] = (int32_t)idx[t];
    }

    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const EpiNorm nm = epi_norm(norm, p);
    float l0[8], l1[8], r0[8], r1[8];
    bool finite = true;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        float2 a = ml[idx[t]], c = mr[idx[t]];          // idx < m <= n: inside the segment
        if (norm) {                                     // one subtract, one multiply (no contraction: -ffp-contract=off)
            a.x = (a.x - nm.c0l) * nm.s0l; a.y = (a.y - nm.c1l) * nm.s1l;
            c.x = (c.x - nm.c0r) * nm.s0r; c.y = (c.y - nm.c1r) * nm.s1r;
        }
        finite = finite && __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(c.x) && __builtin_isfinite(c.y);
        l0[t] = a.x; l1[t] = a.y; r0[t] = c.x; r1[t] = c.y;
    }
    float e[9];
    bool ok = false;
    if (finite) {
        float M[9][8], tau[8];                          // A^T: column t = q of draw t, q[3i + j] = x_r[i] x_l[j]
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            M[0][t] = r0[t] * l0[t]; M[1][t] = r0[t] * l1[t]; M[2][t] = r0[t];
            M[3][t] = r1[t] * l0[t]; M[4][t] = r1[t] * l1[t]; M[5][t] = r1[t];
            M[6][t] = l0[t];         M[7][t] = l1[t];         M[8][t] = 1.0f;
        }
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
        hyp_apply_q(M, tau, z);
        // one refinement step: res_t = x_r . (E x_l), R^T y = res, e = z - Q (y, 0)
        float c[9];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float a0 = __builtin_fmaf(z[0], l0[t], __builtin_fmaf(z[1], l1[t], z[2]));
            const float a1 = __builtin_fmaf(z[3], l0[t], __builtin_fmaf(z[4], l1[t], z[5]));
            const float a2 = __builtin_fmaf(z[6], l0[t], __builtin_fmaf(z[7], l1[t], z[8]));
            float acc = __builtin_fmaf(r0[t], a0, __builtin_fmaf(r1[t], a1, a2));
#pragma unroll
            for (int i = 0; i < t; ++i) acc = __builtin_fmaf(-M[i][t], c[i], acc);
            c[t] = acc / M[t][t];
        }
        c[8] = 0.0f;
        hyp_apply_q(M, tau, c);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = z[k] - c[k];
        ok = hyp_unit(e);
        if (!ok) {                                      // the step met a zero pivot or overflowed: the QR vector as it is
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = z[k];
            ok = hyp_unit(e);
        }
    }
    if (!ok) {
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

extern "C" size_t pats_epipolar_hypotheses_workspace_bytes(int64_t pairs, int64_t H) {
    (void)pairs; (void)H;
    return 0;                                           // a hypothesis lives in its thread's registers
}

extern "C" int pats_epipolar_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                    const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                    const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                    int32_t* sample_idx, void* workspace, size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    PATS_REQUIRE_PTR("epipolar_hypotheses_by_pair", matches_l, 8);
    PATS_REQUIRE_PTR("epipolar_hypotheses_by_pair", matches_r, 8);
    PATS_REQUIRE_PTR("epipolar_hypotheses_by_pair", pair_seed, 8);
    PATS_REQUIRE_PTR("epipolar_hypotheses_by_pair", models, 4);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses_by_pair", norm, 4);     // optional pointers: null is aligned
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses_by_pair", sample_idx, 4);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses_by_pair", pair_off, 8);
    PATS_REQUIRE_ALIGNED("epipolar_hypotheses_by_pair", counts_in, 8);
    int rc = epi_check_segments("epipolar_hypotheses_by_pair", pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h("epipolar_hypotheses_by_pair", H);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(progressive == 0 || progressive == 1, "epipolar_hypotheses_by_pair: progressive = %d must be 0 or 1", progressive);
    PATS_REQUIRE(workspace_bytes >= pats_epipolar_hypotheses_workspace_bytes(pairs, H), "epipolar_hypotheses_by_pair: workspace too small");
    const int64_t chunks = ceil_div(H, HYP_THREADS);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "epipolar_hypotheses_by_pair: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)",
                 (long long)pairs, (long long)pairs, (long long)chunks);
    hipLaunchKernelGGL(epipolar_hypotheses_kernel, dim3((unsigned)(pairs * chunks)), dim3(HYP_THREADS), 0, as_stream(stream), matches_l,
                       matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models, sample_idx);
    return check_launch("epipolar_hypotheses kernel");
}
