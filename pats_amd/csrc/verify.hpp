// The two model families of the per-pair verification, the mask kernel's moment reduction and the count argmax - what epipolar.hip's
// kernels and polish.hip's local optimisation both run, and what absolute.hip takes of it (the packed FMAs, the argmax), written once.
// include/pats_amd.h states the definitions; docs/kernels.md 4.7 / 4.11 the design.
//
// A family is a struct with the two things that differ: test2, THE arithmetic of its test (two matches against one model), and
// accumulate, a match's contribution to the moments.
//   Epipolar    squared Sampson error against thr^2, without the division; the moments of q = vec(x_r x_l^T)
//   Homography  squared forward transfer error against thr^2, without the division; the moments of the two DLT rows A_i, B_i
#pragma once
#include "common.hpp"

namespace pats {

constexpr int EPI_MASK_THREADS = 512;               // the walk whose order fixes the moments' bits
constexpr int EPI_MASK_WAVES = EPI_MASK_THREADS / WAVE;
constexpr int EPI_MOM = 45;                         // upper triangle of the 9x9 moment matrix

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f pk_splat(float v) { return v2f{v, v}; }

// The families.  test2: two matches against one model - match k is an inlier iff w[k] > 0 and s[k] <= lim[k]; the score and the mask
// kernel both call it.  accumulate: an inlier's 45 products in float64 (the products of two float32 are exact).  The strings are the
// names the launch checks report.
struct Epipolar {
    static constexpr const char *SCORE = "epipolar_score kernel", *SCORE_MSAC = "epipolar_score kernel (MSAC)", *ROUND = "epipolar_score kernel (a round)",
                                *ARGMAX = "epipolar_argmax kernel", *MASK = "epipolar_mask kernel", *POLISH = "epipolar_polish kernel";
    // s = r^2, lim = thr^2 den, w = den
    static __device__ __forceinline__ void test2(const float (&e)[9], float t2, v2f l0, v2f l1, v2f r0, v2f r1, v2f& s, v2f& lim, v2f& w) {
        const v2f a0 = pk_fma(pk_splat(e[0]), l0, pk_fma(pk_splat(e[1]), l1, pk_splat(e[2])));
        const v2f a1 = pk_fma(pk_splat(e[3]), l0, pk_fma(pk_splat(e[4]), l1, pk_splat(e[5])));
        const v2f a2 = pk_fma(pk_splat(e[6]), l0, pk_fma(pk_splat(e[7]), l1, pk_splat(e[8])));
        const v2f b0 = pk_fma(pk_splat(e[0]), r0, pk_fma(pk_splat(e[3]), r1, pk_splat(e[6])));
        const v2f b1 = pk_fma(pk_splat(e[1]), r0, pk_fma(pk_splat(e[4]), r1, pk_splat(e[7])));
        const v2f r = pk_fma(r0, a0, pk_fma(r1, a1, a2));
        w = pk_fma(a0, a0, pk_fma(a1, a1, pk_fma(b0, b0, b1 * b1)));
        s = r * r;
        lim = pk_splat(t2) * w;
    }
    static __device__ __forceinline__ void accumulate(float xl0, float xl1, float xr0, float xr1, double (&acc)[EPI_MOM]) {
        const double a0 = (double)xl0, a1 = (double)xl1, b0 = (double)xr0, b1 = (double)xr1;
        const double q[9] = {b0 * a0, b0 * a1, b0, b1 * a0, b1 * a1, b1, a0, a1, 1.0};       // vec(x_r x_l^T): exact products
        int k = 0;
#pragma unroll
        for (int u = 0; u < 9; ++u)
#pragma unroll
            for (int v = u; v < 9; ++v) acc[k++] += q[u] * q[v];
    }
};

// the uncalibrated branch: the Epipolar test and moments, its own refit in the local optimisation (polish.hip)
struct Fundamental : Epipolar {
    static constexpr const char* POLISH = "fundamental_polish kernel";
};

struct Homography {
    static constexpr const char *SCORE = "homography_score kernel", *SCORE_MSAC = "homography_score kernel (MSAC)", *ROUND = "homography_score kernel (a round)",
                                *ARGMAX = "homography_argmax kernel", *MASK = "homography_mask kernel", *POLISH = "homography_polish kernel";
    // s = d0^2 + d1^2, lim = thr^2 a2^2, w = a2^2
    static __device__ __forceinline__ void test2(const float (&e)[9], float t2, v2f l0, v2f l1, v2f r0, v2f r1, v2f& s, v2f& lim, v2f& w) {
        const v2f a0 = pk_fma(pk_splat(e[0]), l0, pk_fma(pk_splat(e[1]), l1, pk_splat(e[2])));
        const v2f a1 = pk_fma(pk_splat(e[3]), l0, pk_fma(pk_splat(e[4]), l1, pk_splat(e[5])));
        const v2f a2 = pk_fma(pk_splat(e[6]), l0, pk_fma(pk_splat(e[7]), l1, pk_splat(e[8])));
        const v2f d0 = pk_fma(-r0, a2, a0);
        const v2f d1 = pk_fma(-r1, a2, a1);
        s = pk_fma(d0, d0, d1 * d1);
        w = a2 * a2;
        lim = pk_splat(t2) * w;
    }
    static __device__ __forceinline__ void accumulate(float xl0, float xl1, float xr0, float xr1, double (&acc)[EPI_MOM]) {
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
};

// The MSAC gain of one cell from what test2 returned (include/pats_amd.h, "Per-pair MSAC scoring"): 2^20 - q for an inlier,
// q = min(floor(u 2^20), 2^20), u = s / lim as ONE hardware reciprocal (v_rcp_f32, 1 ulp) and one multiply; 0 for every other cell.
// The scaling by 2^20 is exact, the conversion truncates (u >= 0), and fminf drops a NaN u (0 x inf: s = 0 against a lim so small
// that its reciprocal overflows) in favour of 2^20: that cell gains nothing.
constexpr int MSAC_GAIN_BITS = 20;
__device__ __forceinline__ uint32_t verify_gain(bool inlier, float s, float lim) {
    constexpr float ONE = (float)(1u << MSAC_GAIN_BITS);
    const float u = lim > 0.0f ? s * __builtin_amdgcn_rcpf(lim) : 0.0f;
    const uint32_t q = (uint32_t)fminf(u * ONE, ONE);
    return inlier ? (1u << MSAC_GAIN_BITS) - q : 0u;
}

__device__ __forceinline__ void verify_model(const float* __restrict__ m, float (&e)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = m[k];
}

// The winner by count, one kernel for every family (epipolar.hip and absolute.hip launch it): one workgroup of THREADS =
// ARGMAX_THREADS per pair, the largest count of counts[p, :], the lowest index that holds it.  A template, so that each translation
// unit that launches it carries its own copy
constexpr int ARGMAX_THREADS = 256;

template <int THREADS>
__global__ void __launch_bounds__(THREADS) verify_argmax_kernel(const int32_t* __restrict__ counts, int H, int32_t* __restrict__ best,
                                                                 int64_t* __restrict__ best_count) {
    __shared__ int sv[THREADS], si[THREADS];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t* c = counts + p * H;
    int v = -1, idx = 0x7fffffff;
    for (int h = tid; h < H; h += THREADS) {            // ascending h: a later equal count does not replace an earlier one
        const int x = c[h];
        if (x > v) { v = x; idx = h; }
    }
    sv[tid] = v; si[tid] = idx;
    wg_barrier();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int ov = sv[tid + s], oi = si[tid + s];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        wg_barrier();
    }
    if (tid == 0) { best[p] = si[0]; best_count[p] = (int64_t)sv[0]; }
}

// The moments' fixed order behind the thread-local sums of an EPI_MASK_THREADS walk: an xor tree over the wave, then the waves in
// order.  EVERY thread of the workgroup calls this (one barrier inside); thread k < EPI_MOM gets entry k of the upper triangle.
__device__ __forceinline__ double verify_moments_sum(const double (&acc)[EPI_MOM], double (&part)[EPI_MASK_WAVES][EPI_MOM], int tid, int lane,
                                                     int wave) {
#pragma unroll
    for (int k = 0; k < EPI_MOM; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) part[wave][k] = v;
    }
    wg_barrier();
    double s = 0.0;
    if (tid < EPI_MOM) {
#pragma unroll
        for (int w = 0; w < EPI_MASK_WAVES; ++w) s += part[w][tid];
    }
    return s;
}

// entry k of the upper triangle -> (u, v), u <= v
__device__ __forceinline__ void verify_triangle(int k, int& u, int& v) {
    u = 0;
    while (k >= 9 - u) { k -= 9 - u; ++u; }
    v = u + k;
}

}  // namespace pats
