// Per-pair homographies on the hand-over's matches - the planar sibling of the epipolar stages: 4-point hypotheses, their
// verification (squared forward transfer error against thr^2, without the division), and the least-squares refit of the winner's
// inliers with its denormalisation.  No host read anywhere.  include/pats_amd.h states the definition ("Per-pair homographies");
// docs/kernels.md 4.11 the design.  The segments, the normalisation, a match's point and the sampler are epipolar.hpp's.
//
//   hypotheses  one THREAD per hypothesis, 64 threads per workgroup, grid = pairs x ceil(H / 64): four draws (epi_draw<4>), the
//               9x8 matrix A^T (two columns per match) in registers, Householder QR without pivoting, the null vector as the last
//               column of Q, one step of iterative refinement with the residuals formed from the factored test (fused multiply-
//               adds on the float32 points).  The solve is hypotheses.hip's, written again here: that file stays as it is
//   score       grid = tiles x pairs x model chunks, 256 threads - epipolar_score_kernel's plan: HOM_R = 8 matches per thread in
//               registers (four packed pairs), a model as nine wave-uniform floats loaded one model ahead, v_pk_fma_f32 per pair,
//               the verdicts as wave ballots counted on the scalar unit, lane h % 64 keeps the count of model h, ONE integer
//               atomic per workgroup and model with a non-zero sum;  <true>: one round of the adaptive verification (adaptive.hip)
//   argmax      one workgroup per pair: the largest count, the lowest index that holds it
//   mask        one workgroup per pair: the winner's verdicts with hom_test2 (the score kernel's device function: the mask's
//               population is best_count exactly) and the 9x9 moments in float64 in a fixed order
//   refit       one wave per pair, float64: cyclic Jacobi on the moments in LDS (pose.hip's round-robin scheme, written again
//               here), the two smallest eigenvalues, the eigenvector, the sign rule, the denormalisation and the permutation
#include "common.hpp"
#include "epipolar.hpp"

namespace pats {

constexpr int HOM_HYP_THREADS = 64;                    // hypotheses per workgroup: one wave
constexpr int HOM_THREADS = 256;
constexpr int HOM_WAVES = HOM_THREADS / WAVE;
constexpr int HOM_R = 8;                               // matches per thread
constexpr int HOM_TILE = HOM_THREADS * HOM_R;          // matches per workgroup
constexpr int HOM_CHUNK = 256;                         // models per workgroup
constexpr int HOM_MASK_THREADS = 512;
constexpr int HOM_MASK_WAVES = HOM_MASK_THREADS / WAVE;
constexpr int HOM_MOM = 45;                            // upper triangle of the 9x9 moment matrix
constexpr int HOM_REFIT_THREADS = 64;
constexpr int HOM_SWEEPS = 16;                         // cap of the Jacobi loop (a sweep without a rotation ends it)
constexpr int HOM_MIN_INLIERS = 4;

typedef float h2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ h2f hom_fma(h2f a, h2f b, h2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ h2f hom_splat(float v) { return h2f{v, v}; }

// ---- hypotheses -------------------------------------------------------------------------------------------------------------------
// z <- H_0 H_1 .. H_7 z with the reflectors H_k = I - tau_k v_k v_k^T, v_k = (1, M[k+1..8][k]) on rows k .. 8
__device__ __forceinline__ void hom_apply_q(const float (&M)[9][8], const float (&tau)[8], float (&z)[9]) {
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
__device__ __forceinline__ bool hom_unit(float (&z)[9]) {
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

__global__ void __launch_bounds__(HOM_HYP_THREADS)
homography_hypotheses_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                             const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks, int H,
                             const int64_t* __restrict__ pair_seed, const float* __restrict__ norm, int progressive,
                             float* __restrict__ models, int32_t* __restrict__ sample_idx) {
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h = (int)(b % (uint32_t)chunks) * HOM_HYP_THREADS + (int)threadIdx.x;
    if (h >= H) return;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    float* mo = models + (p * H + h) * 9;
    int32_t* so = sample_idx ? sample_idx + (p * H + h) * 4 : nullptr;
    if (n < 4) {                                        // workgroup-uniform: the zero model, no sample
#pragma unroll
        for (int k = 0; k < 9; ++k) mo[k] = 0.0f;
        if (so) {
#pragma unroll
            for (int t = 0; t < 4; ++t) so[t] = -1;
        }
        return;
    }
    uint32_t m = n;                                     // the pool: 4 <= m <= n
    if (progressive) {
        const int64_t q = ((int64_t)n * (h + 1) + H - 1) / H;
        m = q < 4 ? 4u : (q > (int64_t)n ? n : (uint32_t)q);
    }
    uint32_t idx[4];                                    // the draws in draw order (epipolar.hpp: the sampler)
    epi_draw<4>((uint64_t)pair_seed[p], (uint32_t)h, m, idx);
    if (so) {
#pragma unroll
        for (int t = 0; t < 4; ++t) so[t] = (int32_t)idx[t];
    }

    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const EpiNorm nm = epi_norm(norm, p);
    float l0[4], l1[4], r0[4], r1[4];
    bool finite = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
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
        float M[9][8], tau[8];                          // A^T: column 2t = A_t, column 2t + 1 = B_t of draw t
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            M[0][2 * t] = -l0[t];         M[1][2 * t] = -l1[t];         M[2][2 * t] = -1.0f;
            M[3][2 * t] = 0.0f;           M[4][2 * t] = 0.0f;           M[5][2 * t] = 0.0f;
            M[6][2 * t] = r0[t] * l0[t];  M[7][2 * t] = r0[t] * l1[t];  M[8][2 * t] = r0[t];
            M[0][2 * t + 1] = 0.0f;          M[1][2 * t + 1] = 0.0f;          M[2][2 * t + 1] = 0.0f;
            M[3][2 * t + 1] = -l0[t];        M[4][2 * t + 1] = -l1[t];        M[5][2 * t + 1] = -1.0f;
            M[6][2 * t + 1] = r1[t] * l0[t]; M[7][2 * t + 1] = r1[t] * l1[t]; M[8][2 * t + 1] = r1[t];
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
        hom_apply_q(M, tau, z);
        // one refinement step: res = A z through the factored form (A_t z = r0 a2 - a0, B_t z = r1 a2 - a1, a = Z x_l), R^T y = res,
        // e = z - Q (y, 0)
        float c[9];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float a0 = __builtin_fmaf(z[0], l0[t], __builtin_fmaf(z[1], l1[t], z[2]));
            const float a1 = __builtin_fmaf(z[3], l0[t], __builtin_fmaf(z[4], l1[t], z[5]));
            const float a2 = __builtin_fmaf(z[6], l0[t], __builtin_fmaf(z[7], l1[t], z[8]));
            float acc = __builtin_fmaf(r0[t], a2, -a0);
#pragma unroll
            for (int i = 0; i < 2 * t; ++i) acc = __builtin_fmaf(-M[i][2 * t], c[i], acc);
            c[2 * t] = acc / M[2 * t][2 * t];
            acc = __builtin_fmaf(r1[t], a2, -a1);
#pragma unroll
            for (int i = 0; i < 2 * t + 1; ++i) acc = __builtin_fmaf(-M[i][2 * t + 1], c[i], acc);
            c[2 * t + 1] = acc / M[2 * t + 1][2 * t + 1];
        }
        c[8] = 0.0f;
        hom_apply_q(M, tau, c);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = z[k] - c[k];
        ok = hom_unit(e);
        if (!ok) {                                      // the step met a zero pivot or overflowed: the QR vector as it is
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = z[k];
            ok = hom_unit(e);
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

// ---- verification -----------------------------------------------------------------------------------------------------------------
// two matches against one model: d0^2 + d1^2, thr^2 a2^2 and a2^2.  THE arithmetic of the test - the score and the mask kernel both
// call it; match k is an inlier iff w[k] > 0 and s[k] <= lim[k].
__device__ __forceinline__ void hom_test2(const float (&e)[9], float t2, h2f l0, h2f l1, h2f r0, h2f r1, h2f& s, h2f& lim, h2f& w) {
    const h2f a0 = hom_fma(hom_splat(e[0]), l0, hom_fma(hom_splat(e[1]), l1, hom_splat(e[2])));
    const h2f a1 = hom_fma(hom_splat(e[3]), l0, hom_fma(hom_splat(e[4]), l1, hom_splat(e[5])));
    const h2f a2 = hom_fma(hom_splat(e[6]), l0, hom_fma(hom_splat(e[7]), l1, hom_splat(e[8])));
    const h2f d0 = hom_fma(-r0, a2, a0);
    const h2f d1 = hom_fma(-r1, a2, a1);
    s = hom_fma(d0, d0, d1 * d1);
    w = a2 * a2;
    lim = hom_splat(t2) * w;
}

__device__ __forceinline__ void hom_model(const float* __restrict__ m, float (&e)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = m[k];
}

// ROUND = false: the fixed budget - models [0, H) in `chunks` chunks; h_begin, h_stop and stopped are not read.  ROUND = true: a round
// of the adaptive verification (adaptive.hip issues them) - models [h_begin, h_stop) in `chunks` chunks, and the workgroups of a
// pair whose stopped flag is set return at once
template <bool ROUND>
__global__ void __launch_bounds__(HOM_THREADS)
homography_score_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const float* __restrict__ conf_,
                        const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                        int pairs, int chunks, const float* __restrict__ models, int H, const float* __restrict__ thr,
                        const float* __restrict__ norm, int gate, float min_conf, int32_t* __restrict__ counts, int h_begin, int h_stop,
                        const int32_t* __restrict__ stopped) {
    __shared__ int wave_cnt[HOM_WAVES][HOM_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // block -> (tile, pair, chunk), the tile slowest: the blocks that find work come first
    const uint32_t b = blockIdx.x;
    const int chunk = (int)(b % (uint32_t)chunks);
    const int64_t p = (int64_t)((b / (uint32_t)chunks) % (uint32_t)pairs);
    const uint32_t tile = b / ((uint32_t)chunks * (uint32_t)pairs);
    if (ROUND && stopped[p]) return;                    // workgroup-uniform: the pair has met its confidence
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const uint64_t i0 = (uint64_t)tile * HOM_TILE;
    if (i0 >= n) return;                                // workgroup-uniform
    const float t = thr[p];
    if (!(t >= 0.0f)) return;                           // NaN or negative threshold: the pair has no inliers (counts are zeroed)
    const float t2 = t * t;

    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const float* conf = conf_ ? conf_ + lo : nullptr;
    const EpiNorm nm = epi_norm(norm, p);
    h2f l0[HOM_R / 2], l1[HOM_R / 2], r0[HOM_R / 2], r1[HOM_R / 2];
#pragma unroll
    for (int k = 0; k < HOM_R / 2; ++k) {
        float a0, a1, a2, a3, c0, c1, c2, c3;
        epi_load(ml, mr, conf, (uint32_t)i0 + (uint32_t)((2 * k) * HOM_THREADS + tid), n, norm != nullptr, nm, gate != 0, min_conf, a0, a1, a2, a3);
        epi_load(ml, mr, conf, (uint32_t)i0 + (uint32_t)((2 * k + 1) * HOM_THREADS + tid), n, norm != nullptr, nm, gate != 0, min_conf, c0, c1, c2, c3);
        l0[k] = h2f{a0, c0}; l1[k] = h2f{a1, c1}; r0[k] = h2f{a2, c2}; r1[k] = h2f{a3, c3};
    }

    const int h_lo = (ROUND ? h_begin : 0) + chunk * HOM_CHUNK;              // the fixed budget: every model, [0, H)
    const int h_end = ROUND ? h_stop : H;
    const int nmod = h_end - h_lo < HOM_CHUNK ? h_end - h_lo : HOM_CHUNK;     // >= 1: chunks = ceil((h_end - h_begin) / HOM_CHUNK)
    const float* m = models + ((int64_t)p * H + h_lo) * 9;
    float e[9];
    hom_model(m, e);
    for (int h0 = 0; h0 < nmod; h0 += WAVE) {
        const int jn = nmod - h0 < WAVE ? nmod - h0 : WAVE;
        int acc = 0;
        for (int j = 0; j < jn; ++j) {
            float en[9];
            const int hn = h0 + j + 1 < nmod ? h0 + j + 1 : h0 + j;            // one model ahead (the last one again: in bounds)
            hom_model(m + (int64_t)hn * 9, en);
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < HOM_R / 2; ++k) {
                h2f s, lim, w;
                hom_test2(e, t2, l0[k], l1[k], r0[k], r1[k], s, lim, w);
                // the two comparisons as ballots of their own, combined on the scalar unit
                cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(w.x > 0.0f) & __builtin_amdgcn_ballot_w64(s.x <= lim.x)) +
                       __builtin_popcountll(__builtin_amdgcn_ballot_w64(w.y > 0.0f) & __builtin_amdgcn_ballot_w64(s.y <= lim.y));
            }
            acc = lane == j ? cnt : acc;
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = en[k];
        }
        wave_cnt[wave][h0 + lane] = acc;                // h0 + lane < HOM_CHUNK; lanes past jn hold 0
    }
    wg_barrier();
    if (tid < nmod) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < HOM_WAVES; ++w) s += wave_cnt[w][tid];
        if (s) atomicAdd(&counts[(int64_t)p * H + h_lo + tid], s);
    }
}

// one workgroup per pair: the largest count of counts[p, :], the lowest index that holds it
__global__ void __launch_bounds__(256) homography_argmax_kernel(const int32_t* __restrict__ counts, int H, int32_t* __restrict__ best,
                                                                 int64_t* __restrict__ best_count) {
    __shared__ int sv[256], si[256];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t* c = counts + p * H;
    int v = -1, idx = 0x7fffffff;
    for (int h = tid; h < H; h += 256) {                // ascending h: a later equal count does not replace an earlier one
        const int x = c[h];
        if (x > v) { v = x; idx = h; }
    }
    sv[tid] = v; si[tid] = idx;
    wg_barrier();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const int ov = sv[tid + s], oi = si[tid + s];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        wg_barrier();
    }
    if (tid == 0) { best[p] = si[0]; best_count[p] = (int64_t)sv[0]; }
}

// one workgroup per pair: the winner's inlier mask (the rows outside the segments were zeroed before) and the moments
__global__ void __launch_bounds__(HOM_MASK_THREADS)
homography_mask_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const float* __restrict__ conf_,
                       const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                       const float* __restrict__ models, int H, const float* __restrict__ thr, const float* __restrict__ norm, int gate,
                       float min_conf, const int32_t* __restrict__ best, const int64_t* __restrict__ best_count,
                       uint8_t* __restrict__ inlier, double* __restrict__ moments) {
    __shared__ double part[HOM_MASK_WAVES][HOM_MOM];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const float t = thr[p];
    const bool live = t >= 0.0f && best_count[p] > 0;  // otherwise no match is an inlier: the mask stays zero, the moments are zero
    double acc[HOM_MOM];
#pragma unroll
    for (int k = 0; k < HOM_MOM; ++k) acc[k] = 0.0;
    if (live) {                                         // workgroup-uniform
        const float t2 = t * t;
        int h = best[p];
        h = h < 0 ? 0 : (h >= H ? H - 1 : h);
        float e[9];
        hom_model(models + ((int64_t)p * H + h) * 9, e);
        const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
        const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
        const float* conf = conf_ ? conf_ + lo : nullptr;
        const EpiNorm nm = epi_norm(norm, p);
        for (uint32_t i0 = 0; i0 < n; i0 += HOM_MASK_THREADS) {
            const uint32_t i = i0 + tid;
            float xl0, xl1, xr0, xr1;
            epi_load(ml, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, xl0, xl1, xr0, xr1);
            h2f s, lim, w;
            hom_test2(e, t2, hom_splat(xl0), hom_splat(xl1), hom_splat(xr0), hom_splat(xr1), s, lim, w);
            const bool in0 = w.x > 0.0f && s.x <= lim.x;
            if (i < n) inlier[lo + i] = in0 ? 1 : 0;
            if (moments && in0) {
                const double a0 = (double)xl0, a1 = (double)xl1, b0 = (double)xr0, b1 = (double)xr1;
                // the rows A_i and B_i: the products of two float32 are exact in float64
                const double qa[9] = {-a0, -a1, -1.0, 0.0, 0.0, 0.0, b0 * a0, b0 * a1, b0};
                const double qb[9] = {0.0, 0.0, 0.0, -a0, -a1, -1.0, b1 * a0, b1 * a1, b1};
                int k = 0;
#pragma unroll
                for (int u = 0; u < 9; ++u)
#pragma unroll
                    for (int v = u; v < 9; ++v) acc[k++] += qa[u] * qa[v] + qb[u] * qb[v];
            }
        }
    }
    if (!moments) return;
#pragma unroll
    for (int k = 0; k < HOM_MOM; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) part[wave][k] = v;
    }
    wg_barrier();
    if (tid < HOM_MOM) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < HOM_MASK_WAVES; ++w) s += part[w][tid];
        int u = 0, k = tid;                             // entry tid of the upper triangle -> (u, v)
        while (k >= 9 - u) { k -= 9 - u; ++u; }
        const int v = u + k;
        double* mo = moments + p * 81;
        mo[u * 9 + v] = s;
        mo[v * 9 + u] = s;
    }
}

// ---- refit ------------------------------------------------------------------------------------------------------------------------
// the rotation that annihilates apq: J = [[c, s], [-s, c]] on (p, q), B = J^T A J  (apq != 0)
__device__ __forceinline__ void hom_cs(double app, double aqq, double apq, double& c, double& s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));   // 0 for a huge theta
    c = 1.0 / __builtin_sqrt(t * t + 1.0);
    s = t * c;
}

// apq is too small to change either diagonal entry
__device__ __forceinline__ bool hom_negligible(double app, double aqq, double g) {
    return __builtin_fabs(app) + g == __builtin_fabs(app) && __builtin_fabs(aqq) + g == __builtin_fabs(aqq);
}

// k -> P k for the permutation P = [[0,1,0],[1,0,0],[0,0,1]] applied to rows and columns of a row-major 3x3
__device__ __forceinline__ int hom_perm(int k, int swapped) {
    const int i = k / 3, j = k - 3 * i;
    const int si = swapped ? (i == 2 ? 2 : 1 - i) : i, sj = swapped ? (j == 2 ? 2 : 1 - j) : j;
    return si * 3 + sj;
}

// out[k] = +-v[P k]: the permutation, then the sign rule judged on the values written (the lowest index among equals)
__device__ __forceinline__ void hom_write(const double (&v)[9], bool ok, int swapped, double* __restrict__ out) {
    double big = -1.0, at = 0.0;
    for (int k = 0; k < 9; ++k) {
        const double x = ok ? v[hom_perm(k, swapped)] : 0.0;
        if (__builtin_fabs(x) > big) { big = __builtin_fabs(x); at = x; }
    }
    const bool flip = at < 0.0;
    for (int k = 0; k < 9; ++k) {
        const double x = ok ? v[hom_perm(k, swapped)] : 0.0;
        out[k] = flip ? -x : x;
    }
}

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
    if (live && moments) {                              // workgroup-uniform
        for (int q = tid; q < 81; q += HOM_REFIT_THREADS) {
            const int i = q / 9, j = q - 9 * i;
            const double v = moments[p * 81 + (i < j ? i * 9 + j : j * 9 + i)];    // the upper triangle: symmetric whatever is stored
            sA[i][j] = v;
            sV[i][j] = i == j ? 1.0 : 0.0;
            if (!__builtin_isfinite(v)) s_bad = 1;      // the same value from every writer
        }
        wg_barrier();
        const bool bad = s_bad != 0;
        const int grp = tid >> 4, k = tid & 15;         // rotation grp of a round, entry k
        const bool mine = k < 9;
        for (int sweep = 0; sweep < HOM_SWEEPS && !bad; ++sweep) {
            for (int r = 0; r < 9; ++r) {
                int pp = (r + grp + 1) % 9, qq = (r + 8 - grp) % 9;
                if (pp > qq) { const int x_ = pp; pp = qq; qq = x_; }
                double c = 1.0, s = 0.0, x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
                bool rot = false, zero = false;
                if (mine) {
                    const double app = sA[pp][pp], aqq = sA[qq][qq], apq = sA[pp][qq];
                    const double g = __builtin_fabs(apq);
                    if (g != 0.0) {
                        if (hom_negligible(app, aqq, g)) {
                            zero = k == 0;
                        } else {
                            rot = true;
                            hom_cs(app, aqq, apq, c, s);
                        }
                    }
                    x = sA[k][pp]; y = sA[k][qq];
                    vx = sV[k][pp]; vy = sV[k][qq];
                }
                wg_barrier();                           // every lane has read the round's entries
                if (zero) { sA[pp][qq] = 0.0; sA[qq][pp] = 0.0; }       // no other lane touches the two in this round
                if (rot) {                              // A <- A J, V <- V J: the columns p and q
                    sA[k][pp] = c * x - s * y; sA[k][qq] = s * x + c * y;
                    sV[k][pp] = c * vx - s * vy; sV[k][qq] = s * vx + c * vy;
                    s_rot = 1;
                }
                wg_barrier();
                if (rot) {                              // A <- J^T A: the rows p and q; the annihilated pair is set, not computed
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
    wg_barrier();
    if (tid != 0) return;
    double e[9], ev[2] = {0.0, 0.0};
    bool ok = live && s_bad == 0;
    if (ok && moments) {
        int m = 0;
        double lmin = sA[0][0];
        for (int k = 1; k < 9; ++k) {                   // the smallest eigenvalue, the lowest index among equals
            const double l = sA[k][k];
            if (l < lmin) { lmin = l; m = k; }
        }
        int m2 = m == 0 ? 1 : 0;
        double lsec = sA[m2][m2];
        for (int k = m2 + 1; k < 9; ++k) {              // the second smallest
            const double l = sA[k][k];
            if (k != m && l < lsec) { lsec = l; m2 = k; }
        }
        ev[0] = lmin; ev[1] = lsec;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) { e[k] = sV[k][m]; s += e[k] * e[k]; }
        const double inv = 1.0 / __builtin_sqrt(s);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] *= inv;
        ok = __builtin_isfinite(lmin) && __builtin_isfinite(lsec);
    } else if (ok) {
        int h = best[p];
        h = h < 0 ? 0 : (h >= H ? H - 1 : h);
        const float* m = models + (p * H + h) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = (double)m[k];
    }
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
        const double c0l = nm.c0l, c1l = nm.c1l, s0l = nm.s0l, s1l = nm.s1l, c0r = nm.c0r, c1r = nm.c1r, s0r = nm.s0r, s1r = nm.s1r;
        if (norm) {
            double q[9];                                // H N_l
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                q[3 * i] = e[3 * i] * s0l;
                q[3 * i + 1] = e[3 * i + 1] * s1l;
                q[3 * i + 2] = e[3 * i + 2] - (e[3 * i] * (c0l * s0l) + e[3 * i + 1] * (c1l * s1l));
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {               // N_r^-1 (H N_l),  N_r^-1 = [[1/s0, 0, c0], [0, 1/s1, c1], [0, 0, 1]]
                g[j] = q[j] / s0r + c0r * q[6 + j];
                g[3 + j] = q[3 + j] / s1r + c1r * q[6 + j];
                g[6 + j] = q[6 + j];
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) s += g[k] * g[k];
            const double inv = 1.0 / __builtin_sqrt(s);
            okp = s > 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) { g[k] *= inv; okp = okp && __builtin_isfinite(g[k]); }
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) g[k] = e[k];
        }
    }
    hom_write(g, okp, swapped, Hpx_out + p * 9);
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_homography_hypotheses_workspace_bytes(int64_t pairs, int64_t H) {
    (void)pairs; (void)H;
    return 0;                                           // a hypothesis lives in its thread's registers
}

extern "C" int pats_homography_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off,
                                                      int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                      const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                      int32_t* sample_idx, void* workspace, size_t workspace_bytes,
                                                      pats_stream_t stream) {
    (void)workspace;
    PATS_REQUIRE_PTR("homography_hypotheses_by_pair", matches_l, 8);
    PATS_REQUIRE_PTR("homography_hypotheses_by_pair", matches_r, 8);
    PATS_REQUIRE_PTR("homography_hypotheses_by_pair", pair_seed, 8);
    PATS_REQUIRE_PTR("homography_hypotheses_by_pair", models, 4);
    PATS_REQUIRE_ALIGNED("homography_hypotheses_by_pair", norm, 4);     // optional pointers: null is aligned
    PATS_REQUIRE_ALIGNED("homography_hypotheses_by_pair", sample_idx, 4);
    PATS_REQUIRE_ALIGNED("homography_hypotheses_by_pair", pair_off, 8);
    PATS_REQUIRE_ALIGNED("homography_hypotheses_by_pair", counts_in, 8);
    int rc = epi_check_segments("homography_hypotheses_by_pair", pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h("homography_hypotheses_by_pair", H);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(progressive == 0 || progressive == 1, "homography_hypotheses_by_pair: progressive = %d must be 0 or 1", progressive);
    PATS_REQUIRE(workspace_bytes >= pats_homography_hypotheses_workspace_bytes(pairs, H), "homography_hypotheses_by_pair: workspace too small");
    const int64_t chunks = ceil_div(H, HOM_HYP_THREADS);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "homography_hypotheses_by_pair: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)",
                 (long long)pairs, (long long)pairs, (long long)chunks);
    hipLaunchKernelGGL(homography_hypotheses_kernel, dim3((unsigned)(pairs * chunks)), dim3(HOM_HYP_THREADS), 0, as_stream(stream),
                       matches_l, matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models,
                       sample_idx);
    return check_launch("homography_hypotheses kernel");
}

extern "C" size_t pats_homography_score_workspace_bytes(int64_t pairs, int64_t H, int64_t cap) {
    (void)pairs; (void)H; (void)cap;
    return 0;                                           // the counts are accumulated in the output itself
}

extern "C" int pats_homography_score_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                 int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                                 int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                                 int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                                 void* workspace, size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    PATS_REQUIRE_PTR("homography_score_by_pair", matches_l, 8);
    PATS_REQUIRE_PTR("homography_score_by_pair", matches_r, 8);
    PATS_REQUIRE_PTR("homography_score_by_pair", models, 4);
    PATS_REQUIRE_PTR("homography_score_by_pair", thr, 4);
    PATS_REQUIRE_PTR("homography_score_by_pair", counts, 4);
    PATS_REQUIRE_PTR("homography_score_by_pair", best, 4);
    PATS_REQUIRE_PTR("homography_score_by_pair", best_count, 8);
    PATS_REQUIRE(inlier, "homography_score_by_pair: null inlier");
    PATS_REQUIRE_ALIGNED("homography_score_by_pair", conf, 4);     // optional pointers: null is aligned
    PATS_REQUIRE_ALIGNED("homography_score_by_pair", norm, 4);
    PATS_REQUIRE_ALIGNED("homography_score_by_pair", pair_off, 8);
    PATS_REQUIRE_ALIGNED("homography_score_by_pair", counts_in, 8);
    PATS_REQUIRE_ALIGNED("homography_score_by_pair", moments, 8);
    int rc = epi_check_segments("homography_score_by_pair", pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h("homography_score_by_pair", H);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(!use_min_conf || conf, "homography_score_by_pair: min_conf needs conf");
    PATS_REQUIRE(!use_min_conf || min_conf >= 0.0f, "homography_score_by_pair: min_conf = %g must be a non-negative number", (double)min_conf);
    PATS_REQUIRE(workspace_bytes >= pats_homography_score_workspace_bytes(pairs, H, cap), "homography_score_by_pair: workspace too small");
    const int64_t longest = counts_in ? stride : cap;   // the grid comes from the sizes alone: no host read of the counts
    const int64_t tiles = ceil_div(longest, HOM_TILE), chunks = ceil_div(H, HOM_CHUNK);
    PATS_REQUIRE(tiles * chunks <= 0x7fffffff / pairs, "homography_score_by_pair: pairs = %lld gives a grid of %lld x %lld x %lld workgroups (< 2^31)",
                 (long long)pairs, (long long)tiles, (long long)pairs, (long long)chunks);
    hipStream_t st = as_stream(stream);
    rc = fill_bytes(counts, 0, (size_t)pairs * (size_t)H * sizeof(int32_t), st);
    if (rc != PATS_OK) return rc;
    rc = fill_bytes(inlier, 0, (size_t)cap, st);
    if (rc != PATS_OK) return rc;
    const float* cf = use_min_conf ? conf : nullptr;    // without a threshold the confidence is not read
    if (tiles > 0) {
        hipLaunchKernelGGL(homography_score_kernel<false>, dim3((unsigned)(tiles * pairs * chunks)), dim3(HOM_THREADS), 0, st, matches_l,
                           matches_r, cf, pair_off, counts_in, stride, cap, (int)pairs, (int)chunks, models, (int)H, thr, norm, use_min_conf, min_conf,
                           counts, 0, (int)H, nullptr);
        rc = check_launch("homography_score kernel");
        if (rc != PATS_OK) return rc;
    }
    hipLaunchKernelGGL(homography_argmax_kernel, dim3((unsigned)pairs), dim3(256), 0, st, counts, (int)H, best, best_count);
    rc = check_launch("homography_argmax kernel");
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(homography_mask_kernel, dim3((unsigned)pairs), dim3(HOM_MASK_THREADS), 0, st, matches_l, matches_r, cf, pair_off,
                       counts_in, stride, cap, models, (int)H, thr, norm, use_min_conf, min_conf, best, best_count, inlier, moments);
    return check_launch("homography_mask kernel");
}

// ---- adaptive verification: this branch's two launchers for adaptive.hip's host side ------------------------------------------------
static_assert(HOM_TILE == ADAPTIVE_TILE && HOM_CHUNK == ADAPTIVE_CHUNK, "adaptive.hip sizes the rounds' grids");

static int hom_adaptive_round(const AdaptiveCall& c, const float* conf, int tiles, int h_lo, int h_hi, const int32_t* stopped,
                              hipStream_t st) {
    const int64_t chunks = ceil_div(h_hi - h_lo, HOM_CHUNK);
    hipLaunchKernelGGL(homography_score_kernel<true>, dim3((unsigned)(tiles * c.pairs * chunks)), dim3(HOM_THREADS), 0, st, c.matches_l,
                       c.matches_r, conf, c.pair_off, c.counts_in, c.stride, c.cap, (int)c.pairs, (int)chunks, c.models, (int)c.H, c.thr,
                       c.norm, c.use_min_conf, c.min_conf, c.counts, h_lo, h_hi, stopped);
    return check_launch("homography_score kernel (a round)");
}

static int hom_adaptive_mask(const AdaptiveCall& c, const float* conf, hipStream_t st) {
    hipLaunchKernelGGL(homography_mask_kernel, dim3((unsigned)c.pairs), dim3(HOM_MASK_THREADS), 0, st, c.matches_l, c.matches_r, conf,
                       c.pair_off, c.counts_in, c.stride, c.cap, c.models, (int)c.H, c.thr, c.norm, c.use_min_conf, c.min_conf, c.best,
                       c.best_count, c.inlier, c.moments);
    return check_launch("homography_mask kernel");
}

extern "C" size_t pats_homography_score_adaptive_workspace_bytes(int64_t pairs, int64_t H, int64_t cap) {
    (void)H; (void)cap;
    return adaptive_workspace_bytes(pairs);
}

extern "C" int pats_homography_score_adaptive_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf,
        const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models, int64_t H,
        const float* thr, const float* norm, int use_min_conf, float min_conf, int32_t* counts, int32_t* best, int64_t* best_count,
        uint8_t* inlier, double* moments, void* workspace, size_t workspace_bytes, pats_stream_t stream, double confidence,
        int sample_size, int models_per_sample, int64_t round_models, int32_t* used, int32_t* participating) {
    const AdaptiveCall c{matches_l, matches_r, conf, pair_off, stride, counts_in, pairs, cap, models, H, thr, norm, use_min_conf, min_conf,
                         counts, best, best_count, inlier, moments, workspace, workspace_bytes, stream, confidence, sample_size,
                         models_per_sample, round_models, used, participating};
    return adaptive_score_by_pair("homography_score_adaptive_by_pair", c, hom_adaptive_round, hom_adaptive_mask);
}

extern "C" size_t pats_homography_refit_workspace_bytes(int64_t pairs) {
    (void)pairs;
    return 0;                                           // the solve lives in LDS and registers
}

extern "C" int pats_homography_refit_by_pair_f64(const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                                 const int32_t* best, const float* norm, int64_t pairs, int swapped, double* H_out,
                                                 double* H_px, double* eig, void* workspace, size_t workspace_bytes,
                                                 pats_stream_t stream) {
    (void)workspace;
    PATS_REQUIRE_PTR("homography_refit_by_pair", best_count, 8);
    PATS_REQUIRE_PTR("homography_refit_by_pair", H_out, 8);
    PATS_REQUIRE_PTR("homography_refit_by_pair", eig, 8);
    PATS_REQUIRE_ALIGNED("homography_refit_by_pair", moments, 8);     // optional pointers: null is aligned
    PATS_REQUIRE_ALIGNED("homography_refit_by_pair", models, 4);
    PATS_REQUIRE_ALIGNED("homography_refit_by_pair", best, 4);
    PATS_REQUIRE_ALIGNED("homography_refit_by_pair", norm, 4);
    PATS_REQUIRE_ALIGNED("homography_refit_by_pair", H_px, 8);
    PATS_REQUIRE(pairs >= 1 && pairs <= 0x7fffffff, "homography_refit_by_pair: pairs = %lld (1 .. 2^31 - 1)", (long long)pairs);
    PATS_REQUIRE(swapped == 0 || swapped == 1, "homography_refit_by_pair: swapped = %d must be 0 or 1", swapped);
    PATS_REQUIRE(moments || (models && best), "homography_refit_by_pair: the refit needs moments, or models and best (the winning model)");
    if (models) {
        const int rc = epi_check_h("homography_refit_by_pair", H);
        if (rc != PATS_OK) return rc;
    }
    PATS_REQUIRE(workspace_bytes >= pats_homography_refit_workspace_bytes(pairs), "homography_refit_by_pair: workspace too small");
    hipLaunchKernelGGL(homography_refit_kernel, dim3((unsigned)pairs), dim3(HOM_REFIT_THREADS), 0, as_stream(stream), best_count, moments,
                       moments ? nullptr : models, moments ? 1 : (int)H, best, norm, swapped, H_out, H_px, eig);
    return check_launch("homography_refit kernel");
}
