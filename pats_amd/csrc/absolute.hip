// The absolute-pose branch of the per-pair stages: a match of the left (database) image is lifted through that image's depth map to a
// metric 3-D point, the right (query) camera is hypothesised from three lifted matches (P3P) and verified by reprojection.  Three
// entry points, each a fixed number of launches for the whole batch and no host read.  include/pats_amd.h states the definitions
// ("Per-pair absolute pose from depth"); docs/kernels.md 4.21 the design.
//
//   lift        absolute_lift_kernel: one workgroup of ABS_LIFT_THREADS per pair walks the segment; abs_lift_one is the whole
//               definition of one match (float32, no contraction).  Every row of the segment is stored (a point, or three NaNs), the
//               rows outside every segment were zeroed before the launch; the count is ballots + popcounts
//   hypotheses  absolute_hypotheses_kernel: one thread per pair and sample; epi_draw<3> on the pair's pool, the three points and right
//               points widened to float64, p3p_solve (p3p.hpp), the kept solutions rounded to float32
//   score       absolute_score_kernel: grid = pairs x model chunks, ABS_THREADS threads.  The workgroup stages the pair's segment ONCE
//               in LDS (five planes X0, X1, X2, r0, r1 of stage_n floats; a match that does not take part carries a NaN X0) and walks
//               the ABS_CHUNK models of its chunk over it, two models per pass so that one LDS read feeds two tests: a model is
//               twelve wave-uniform floats, a thread takes two neighbouring matches per trip (five 8-byte LDS reads) through
//               abs_test2's packed FMAs, the verdicts are wave ballots whose popcounts lane h % 64 keeps; every 64 models the
//               register goes to LDS, at the end the waves are added and counts[p, h] is STORED (a workgroup owns its models: no
//               atomics, nothing to zero, the same bits every run).  A segment longer than ABS_STAGE is read through abs_load from
//               global memory every pass instead: the same values
//   argmax      absolute_argmax_kernel: the verification's rule - the largest count, the lowest index that holds it (0 for no inlier)
//   mask        absolute_mask_kernel: the winner's verdict for every match with abs_test2, so the mask's sum is best_count exactly
#include "common.hpp"
#include "epipolar.hpp"
#include "p3p.hpp"

namespace pats {

typedef float abs_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ abs_v2f abs_fma(abs_v2f a, abs_v2f b, abs_v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ abs_v2f abs_splat(float v) { return abs_v2f{v, v}; }

// ---- lift ------------------------------------------------------------------------------------------------------------------------
constexpr int ABS_LIFT_THREADS = 256;
constexpr int ABS_LIFT_WAVES = ABS_LIFT_THREADS / WAVE;

struct AbsMap { const float* d; int64_t h, w, ld; };

// a tap of the map; (i, j) is inside it
__device__ __forceinline__ float abs_tap(const AbsMap& m, int64_t i, int64_t j) { return m.d[i * m.ld + j]; }

// THE definition of one match (include/pats_amd.h): (p0, p1) = the stored (c0, c1) pixel, (x0, x1) = it normalised.  -> valid, d
__device__ __forceinline__ bool abs_lift_one(const AbsMap& m, float p0, float p1, int interp, bool has_max, float max_depth, bool has_jump,
                                             float max_jump, float& d) {
    d = 0.0f;
    if (!(__builtin_isfinite(p0) && __builtin_isfinite(p1))) return false;
    const double hh = (double)m.h, ww = (double)m.w;    // exact for every size a map can have
    if (interp == 0) {
        const float fi = __builtin_rintf(p0), fj = __builtin_rintf(p1);         // round half to even
        if (!(fi >= 0.0f && (double)fi < hh && fj >= 0.0f && (double)fj < ww)) return false;
        d = abs_tap(m, (int64_t)fi, (int64_t)fj);
        if (!(__builtin_isfinite(d) && d > 0.0f)) return false;
    } else {
        const float fi = __builtin_floorf(p0), fj = __builtin_floorf(p1);
        const float a = p0 - fi, b = p1 - fj;
        const bool row1 = a > 0.0f, col1 = b > 0.0f;    // a tap whose weight is zero is not used
        if (!(fi >= 0.0f && (double)fi < hh && fj >= 0.0f && (double)fj < ww)) return false;
        if ((row1 && !((double)fi + 1.0 < hh)) || (col1 && !((double)fj + 1.0 < ww))) return false;
        const int64_t i = (int64_t)fi, j = (int64_t)fj;
        const float d00 = abs_tap(m, i, j), d01 = col1 ? abs_tap(m, i, j + 1) : 0.0f, d10 = row1 ? abs_tap(m, i + 1, j) : 0.0f,
                    d11 = row1 && col1 ? abs_tap(m, i + 1, j + 1) : 0.0f;
        bool ok = __builtin_isfinite(d00) && d00 > 0.0f;
        float mx = d00, mn = d00;
        if (col1) { ok = ok && __builtin_isfinite(d01) && d01 > 0.0f; mx = fmaxf(mx, d01); mn = fminf(mn, d01); }
        if (row1) { ok = ok && __builtin_isfinite(d10) && d10 > 0.0f; mx = fmaxf(mx, d10); mn = fminf(mn, d10); }
        if (row1 && col1) { ok = ok && __builtin_isfinite(d11) && d11 > 0.0f; mx = fmaxf(mx, d11); mn = fminf(mn, d11); }
        if (!ok) return false;
        const float wa = 1.0f - a, wb = 1.0f - b;
        const float w00 = wa * wb, w01 = wa * b, w10 = a * wb, w11 = a * b;
        d = ((w00 * d00 + w01 * d01) + w10 * d10) + w11 * d11;                  // left to right, every product and sum rounded once
        if (has_jump && mx - mn > max_jump * mn) return false;
    }
    if (has_max && d > max_depth) return false;         // a NaN limit does not limit
    return true;
}

__global__ void __launch_bounds__(ABS_LIFT_THREADS)
absolute_lift_kernel(const float* __restrict__ matches_, const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in,
                     int64_t stride, int64_t cap, const float* __restrict__ norm, const int64_t* __restrict__ depth_table,
                     const float* __restrict__ max_depth, int interp, int has_jump, float max_jump, float* __restrict__ points,
                     uint8_t* __restrict__ valid, int64_t* __restrict__ lift_count) {
    __shared__ int s_cnt[ABS_LIFT_WAVES];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const int64_t* row = depth_table + p * 4;
    const AbsMap m{reinterpret_cast<const float*>((uintptr_t)row[0]), row[1], row[2], row[3]};
    const bool has_map = m.d != nullptr && m.h >= 1 && m.w >= 1;                // workgroup-uniform
    const EpiNorm nm = epi_norm(norm, p);
    const bool has_max = max_depth != nullptr;
    const float lim = has_max ? max_depth[p] : 0.0f;
    const float2* ml = reinterpret_cast<const float2*>(matches_) + lo;
    const float nan = __builtin_nanf("");
    int cnt = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += ABS_LIFT_THREADS) {
        const uint32_t i = i0 + tid;
        bool ok = false;
        float d = 0.0f, x0 = 0.0f, x1 = 0.0f;
        if (i < n) {
            const float2 q = ml[i];
            ok = has_map && abs_lift_one(m, q.x, q.y, interp, has_max, lim, has_jump != 0, max_jump, d);
            x0 = q.x; x1 = q.y;
            if (norm) { x0 = (x0 - nm.c0l) * nm.s0l; x1 = (x1 - nm.c1l) * nm.s1l; }     // one subtract, one multiply
        }
        cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
        if (i < n) {
            const int64_t r = lo + i;
            points[r * 3 + 0] = ok ? x0 * d : nan;
            points[r * 3 + 1] = ok ? x1 * d : nan;
            points[r * 3 + 2] = ok ? d : nan;
            valid[r] = ok ? (uint8_t)1 : (uint8_t)0;
        }
    }
    if (lane == 0) s_cnt[wave] = cnt;
    wg_barrier();
    if (tid == 0) {
        int64_t total = 0;
#pragma unroll
        for (int w = 0; w < ABS_LIFT_WAVES; ++w) total += s_cnt[w];
        lift_count[p] = total;
    }
}

// ---- hypotheses ------------------------------------------------------------------------------------------------------------------
constexpr int ABS_HYP_THREADS = 64;                     // samples per workgroup: one wave
constexpr int ABS_SLOTS = 4;                            // models per sample

__global__ void __launch_bounds__(ABS_HYP_THREADS)
absolute_hypotheses_kernel(const float* __restrict__ points, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                           const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks, int H,
                           const int64_t* __restrict__ pair_seed, const float* __restrict__ norm, int progressive,
                           float* __restrict__ models, int32_t* __restrict__ sample_idx, int32_t* __restrict__ n_models) {
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h = (int)(b % (uint32_t)chunks) * ABS_HYP_THREADS + (int)threadIdx.x;
    if (h >= H) return;                                 // no barrier below
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    float* out = models + ((int64_t)p * H + h) * (ABS_SLOTS * 12);
    int32_t* so = sample_idx ? sample_idx + ((int64_t)p * H + h) * 3 : nullptr;
    int kept = 0;
    double Rt[ABS_SLOTS][12];
    if (n < 3) {
        if (so) { so[0] = -1; so[1] = -1; so[2] = -1; }
    } else {
        uint32_t m = n;                                 // the pool: 3 <= m <= n
        if (progressive) {
            const int64_t q = ((int64_t)n * (h + 1) + H - 1) / H;
            m = q < 3 ? 3u : (q > (int64_t)n ? n : (uint32_t)q);
        }
        uint32_t idx[3];
        epi_draw<3>((uint64_t)pair_seed[p], (uint32_t)h, m, idx);
        if (so) { so[0] = (int32_t)idx[0]; so[1] = (int32_t)idx[1]; so[2] = (int32_t)idx[2]; }
        const float* X_ = points + lo * 3;
        const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
        const EpiNorm nm = epi_norm(norm, p);
        double X[3][3], r[3][2];
        bool finite = true;
#pragma unroll
        for (int t = 0; t < 3; ++t) {                   // idx < m <= n: inside the segment
            const float x0 = X_[(int64_t)idx[t] * 3], x1 = X_[(int64_t)idx[t] * 3 + 1], x2 = X_[(int64_t)idx[t] * 3 + 2];
            float2 c = mr[idx[t]];
            if (norm) { c.x = (c.x - nm.c0r) * nm.s0r; c.y = (c.y - nm.c1r) * nm.s1r; }
            finite = finite && __builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2) && __builtin_isfinite(c.x) &&
                     __builtin_isfinite(c.y);
            X[t][0] = (double)x0; X[t][1] = (double)x1; X[t][2] = (double)x2;
            r[t][0] = (double)c.x; r[t][1] = (double)c.y;
        }
        if (finite) kept = p3p_solve(X, r, Rt);
    }
#pragma unroll
    for (int s = 0; s < ABS_SLOTS; ++s)
#pragma unroll
        for (int k = 0; k < 12; ++k) out[s * 12 + k] = s < kept ? (float)Rt[s][k] : 0.0f;
    if (n_models) n_models[(int64_t)p * H + h] = kept;
}

// ---- score -----------------------------------------------------------------------------------------------------------------------
constexpr int ABS_THREADS = 256;
constexpr int ABS_WAVES = ABS_THREADS / WAVE;
constexpr int ABS_CHUNK = 64;                           // models per workgroup: small, so that a batch fills the CUs several times over
constexpr int ABS_STAGE = 6144;                         // matches a workgroup keeps in LDS: 120 KiB of the CU's 160
constexpr int ABS_LDS = ABS_STAGE * 5 * (int)sizeof(float);
constexpr int ABS_MASK_THREADS = 256;

// match i of the segment as (X, x_r); X0 = NaN unless the match takes part: X and x_r finite, the confidence gate passed
__device__ __forceinline__ void abs_load(const float* __restrict__ X_, const float2* __restrict__ mr, const float* __restrict__ conf,
                                         uint32_t i, uint32_t n, bool has_norm, const EpiNorm& nm, bool gate, float min_conf, float& X0,
                                         float& X1, float& X2, float& r0, float& r1) {
    X0 = __builtin_nanf("");
    X1 = X2 = r0 = r1 = 0.0f;
    if (i >= n) return;
    const float a0 = X_[(int64_t)i * 3], a1 = X_[(int64_t)i * 3 + 1], a2 = X_[(int64_t)i * 3 + 2];
    float2 b = mr[i];
    if (has_norm) { b.x = (b.x - nm.c0r) * nm.s0r; b.y = (b.y - nm.c1r) * nm.s1r; }    // one subtract, one multiply
    bool ok = __builtin_isfinite(a0) && __builtin_isfinite(a1) && __builtin_isfinite(a2) && __builtin_isfinite(b.x) && __builtin_isfinite(b.y);
    if (gate) ok = ok && conf[i] >= min_conf;           // false for a NaN confidence
    if (ok) { X0 = a0; X1 = a1; X2 = a2; r0 = b.x; r1 = b.y; }
}

// THE arithmetic of the test, two matches against one model m = [R | t] row-major: Y_k = fma(m[4k], X0, fma(m[4k+1], X1,
// fma(m[4k+2], X2, m[4k+3]))), d_k = fma(-r_k, Y2, Y_k), s = fma(d0, d0, d1 d1), lim = t2 (Y2 Y2); inlier iff Y2 > 0 and s <= lim
__device__ __forceinline__ void abs_test2(const float (&m)[12], float t2, abs_v2f X0, abs_v2f X1, abs_v2f X2, abs_v2f r0, abs_v2f r1, abs_v2f& s,
                                          abs_v2f& lim, abs_v2f& y2) {
    const abs_v2f y0 = abs_fma(abs_splat(m[0]), X0, abs_fma(abs_splat(m[1]), X1, abs_fma(abs_splat(m[2]), X2, abs_splat(m[3]))));
    const abs_v2f y1 = abs_fma(abs_splat(m[4]), X0, abs_fma(abs_splat(m[5]), X1, abs_fma(abs_splat(m[6]), X2, abs_splat(m[7]))));
    y2 = abs_fma(abs_splat(m[8]), X0, abs_fma(abs_splat(m[9]), X1, abs_fma(abs_splat(m[10]), X2, abs_splat(m[11]))));
    const abs_v2f d0 = abs_fma(-r0, y2, y0);
    const abs_v2f d1 = abs_fma(-r1, y2, y1);
    s = abs_fma(d0, d0, d1 * d1);
    lim = abs_splat(t2) * (y2 * y2);
}

__device__ __forceinline__ int abs_count2(abs_v2f s, abs_v2f lim, abs_v2f y2) {
    return __builtin_popcountll(__builtin_amdgcn_ballot_w64(y2.x > 0.0f) & __builtin_amdgcn_ballot_w64(s.x <= lim.x)) +
           __builtin_popcountll(__builtin_amdgcn_ballot_w64(y2.y > 0.0f) & __builtin_amdgcn_ballot_w64(s.y <= lim.y));
}

__device__ __forceinline__ void abs_model(const float* __restrict__ m, float (&e)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) e[k] = m[k];
}

// matches 2 q and 2 q + 1 of the segment (q = a trip's pair index) from the staged planes or through abs_load
__device__ __forceinline__ void abs_fetch2(bool staged, const float* __restrict__ stage, int stage_n, const float* __restrict__ X_,
                                           const float2* __restrict__ mr, const float* __restrict__ conf, uint32_t q, uint32_t n, bool has_norm,
                                           const EpiNorm& nm, bool gate, float min_conf, abs_v2f& X0, abs_v2f& X1, abs_v2f& X2, abs_v2f& r0,
                                           abs_v2f& r1) {
    if (staged) {                                       // stage_n is even and the planes are padded with NaN X0 up to it: 2 q + 1 < stage_n
        const abs_v2f* s2 = reinterpret_cast<const abs_v2f*>(stage);
        const int half = stage_n / 2;
        X0 = s2[q]; X1 = s2[half + q]; X2 = s2[2 * half + q]; r0 = s2[3 * half + q]; r1 = s2[4 * half + q];
    } else {
        float a[5], c[5];
        abs_load(X_, mr, conf, 2 * q, n, has_norm, nm, gate, min_conf, a[0], a[1], a[2], a[3], a[4]);
        abs_load(X_, mr, conf, 2 * q + 1, n, has_norm, nm, gate, min_conf, c[0], c[1], c[2], c[3], c[4]);
        X0 = abs_v2f{a[0], c[0]}; X1 = abs_v2f{a[1], c[1]}; X2 = abs_v2f{a[2], c[2]}; r0 = abs_v2f{a[3], c[3]}; r1 = abs_v2f{a[4], c[4]};
    }
}

// stage_n = the (even) number of match slots per plane the launch allocated: min(longest possible segment rounded up to 2, ABS_STAGE)
__global__ void __launch_bounds__(ABS_THREADS)
absolute_score_kernel(const float* __restrict__ points, const float* __restrict__ mr_, const float* __restrict__ conf_,
                      const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks,
                      const float* __restrict__ models, int M, const float* __restrict__ thr, const float* __restrict__ norm, int gate,
                      float min_conf, int stage_n, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) float abs_stage[];
    __shared__ int wave_cnt[ABS_WAVES][ABS_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h_lo = (int)(b % (uint32_t)chunks) * ABS_CHUNK;
    const int nmod = M - h_lo < ABS_CHUNK ? M - h_lo : ABS_CHUNK;               // >= 1
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const float t = thr[p];
    int32_t* out = counts + (int64_t)p * M + h_lo;
    if (!(t >= 0.0f) || n == 0) {                       // workgroup-uniform: NaN or negative threshold, or no match - no inliers
        for (int h = tid; h < nmod; h += ABS_THREADS) out[h] = 0;
        return;
    }
    const float t2 = t * t;
    const float* X_ = points + lo * 3;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const float* conf = conf_ ? conf_ + lo : nullptr;
    const EpiNorm nm = epi_norm(norm, p);
    const bool staged = n <= (uint32_t)stage_n;         // workgroup-uniform
    const uint32_t n2 = (n + 1) / 2;                    // pairs of matches

    if (staged) {                                       // rows n .. 2 n2 - 1 (at most one) get the NaN X0 of a match that takes no part
        for (uint32_t i = tid; i < 2 * n2; i += ABS_THREADS) {
            float a[5];
            abs_load(X_, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, a[0], a[1], a[2], a[3], a[4]);
#pragma unroll
            for (int k = 0; k < 5; ++k) abs_stage[k * stage_n + i] = a[k];
        }
    }
    wg_barrier();

    const float* m = models + ((int64_t)p * M + h_lo) * 12;
    for (int h0 = 0; h0 < nmod; h0 += WAVE) {
        const int jn = nmod - h0 < WAVE ? nmod - h0 : WAVE;
        int acc = 0;
        for (int j = 0; j < jn; j += 2) {               // two models per pass over the matches
            float ea[12], eb[12];
            const int ha = h0 + j, hb = ha + 1 < nmod ? ha + 1 : ha;            // the last one again: in bounds, its count is dropped
            abs_model(m + (int64_t)ha * 12, ea);
            abs_model(m + (int64_t)hb * 12, eb);
            int ca = 0, cb = 0;
            for (uint32_t q0 = 0; q0 < n2; q0 += ABS_THREADS) {
                const uint32_t q = q0 + tid;
                abs_v2f X0 = abs_splat(__builtin_nanf("")), X1 = abs_splat(0.0f), X2 = X1, r0 = X1, r1 = X1;
                if (q < n2) abs_fetch2(staged, abs_stage, stage_n, X_, mr, conf, q, n, norm != nullptr, nm, gate != 0, min_conf, X0, X1, X2, r0, r1);
                abs_v2f s, lim, y2;
                abs_test2(ea, t2, X0, X1, X2, r0, r1, s, lim, y2);
                ca += abs_count2(s, lim, y2);
                abs_test2(eb, t2, X0, X1, X2, r0, r1, s, lim, y2);
                cb += abs_count2(s, lim, y2);
            }
            acc = lane == j ? ca : (lane == j + 1 ? cb : acc);
        }
        wave_cnt[wave][h0 + lane] = acc;                // h0 + lane < ABS_CHUNK; lanes past jn hold 0 or a dropped count
    }
    wg_barrier();
    if (tid < nmod) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < ABS_WAVES; ++w) s += wave_cnt[w][tid];
        out[tid] = s;
    }
}

// one workgroup per pair: the largest count of counts[p, :], the lowest index that holds it
__global__ void __launch_bounds__(256) absolute_argmax_kernel(const int32_t* __restrict__ counts, int M, int32_t* __restrict__ best,
                                                               int64_t* __restrict__ best_count) {
    __shared__ int sv[256], si[256];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t* c = counts + p * M;
    int v = -1, idx = 0x7fffffff;
    for (int h = tid; h < M; h += 256) {                // ascending h: a later equal count does not replace an earlier one
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

// one workgroup per pair: the winner's inlier mask (zeroed before the launch)
__global__ void __launch_bounds__(ABS_MASK_THREADS)
absolute_mask_kernel(const float* __restrict__ points, const float* __restrict__ mr_, const float* __restrict__ conf_,
                     const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                     const float* __restrict__ models, int M, const float* __restrict__ thr, const float* __restrict__ norm, int gate,
                     float min_conf, const int32_t* __restrict__ best, const int64_t* __restrict__ best_count, uint8_t* __restrict__ inlier) {
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const float t = thr[p];
    if (!(t >= 0.0f) || best_count[p] <= 0) return;     // workgroup-uniform: no match is an inlier, the mask stays zero
    const float t2 = t * t;
    int h = best[p];
    h = h < 0 ? 0 : (h >= M ? M - 1 : h);
    float e[12];
    abs_model(models + ((int64_t)p * M + h) * 12, e);
    const float* X_ = points + lo * 3;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const float* conf = conf_ ? conf_ + lo : nullptr;
    const EpiNorm nm = epi_norm(norm, p);
    for (uint32_t i = tid; i < n; i += ABS_MASK_THREADS) {
        float a[5];
        abs_load(X_, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, a[0], a[1], a[2], a[3], a[4]);
        abs_v2f s, lim, y2;
        abs_test2(e, t2, abs_splat(a[0]), abs_splat(a[1]), abs_splat(a[2]), abs_splat(a[3]), abs_splat(a[4]), s, lim, y2);
        inlier[lo + i] = y2.x > 0.0f && s.x <= lim.x ? 1 : 0;
    }
}

// the staging can exceed the 64 KiB a launch gets unasked: raised once per device
static bool abs_lds_ready() {
    static int state[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return false; }
    if (state[dev] == 0) {
        const bool ok = hipFuncSetAttribute((const void*)absolute_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ABS_LDS) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        state[dev] = ok ? 1 : -1;
    }
    return state[dev] == 1;
}

}  // namespace pats

using namespace pats;

// ---- the entry points (include/pats_amd.h) ---------------------------------------------------------------------------------------
extern "C" int pats_lift_by_pair_f32(const float* matches, const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs,
                                     int64_t cap, const float* norm, const int64_t* depth_table, const float* max_depth, int interp,
                                     int use_max_jump, float max_jump, float* points, uint8_t* valid, int64_t* lift_count,
                                     pats_stream_t stream) {
    PATS_REQUIRE_PTR("lift_by_pair", matches, 8);
    PATS_REQUIRE_PTR("lift_by_pair", depth_table, 8);
    PATS_REQUIRE_PTR("lift_by_pair", points, 4);
    PATS_REQUIRE(valid, "lift_by_pair: null valid");
    PATS_REQUIRE_PTR("lift_by_pair", lift_count, 8);
    PATS_REQUIRE_ALIGNED("lift_by_pair", norm, 4);      // optional pointers: null is aligned
    PATS_REQUIRE_ALIGNED("lift_by_pair", max_depth, 4);
    PATS_REQUIRE_ALIGNED("lift_by_pair", pair_off, 8);
    PATS_REQUIRE_ALIGNED("lift_by_pair", counts_in, 8);
    int rc = epi_check_segments("lift_by_pair", pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(interp == 0 || interp == 1, "lift_by_pair: interp = %d must be 0 (nearest) or 1 (bilinear)", interp);
    PATS_REQUIRE(use_max_jump == 0 || use_max_jump == 1, "lift_by_pair: use_max_jump = %d must be 0 or 1", use_max_jump);
    hipStream_t st = as_stream(stream);
    // every byte of both per-match outputs is defined: zeros here, the kernel stores every row of every segment
    if ((rc = fill_bytes(points, 0, (size_t)cap * 3 * sizeof(float), st)) != PATS_OK) return rc;
    if ((rc = fill_bytes(valid, 0, (size_t)cap, st)) != PATS_OK) return rc;
    hipLaunchKernelGGL(absolute_lift_kernel, dim3((unsigned)pairs), dim3(ABS_LIFT_THREADS), 0, st, matches, pair_off, counts_in, stride, cap,
                       norm, depth_table, max_depth, interp, use_max_jump, max_jump, points, valid, lift_count);
    return check_launch("absolute_lift kernel");
}

extern "C" int pats_absolute_hypotheses_by_pair_f32(const float* points, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                    const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                    const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                    int32_t* sample_idx, int32_t* n_models, pats_stream_t stream) {
    const char* who = "absolute_hypotheses_by_pair";
    EPI_REQUIRE_PTR(points, 4);
    EPI_REQUIRE_PTR(matches_r, 8);
    EPI_REQUIRE_PTR(pair_seed, 8);
    EPI_REQUIRE_PTR(models, 4);
    EPI_REQUIRE_ALIGNED(norm, 4);                       // optional pointers: null is aligned
    EPI_REQUIRE_ALIGNED(sample_idx, 4);
    EPI_REQUIRE_ALIGNED(n_models, 4);
    EPI_REQUIRE_ALIGNED(pair_off, 8);
    EPI_REQUIRE_ALIGNED(counts_in, 8);
    int rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h(who, H);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(H <= pats_epipolar_max_h() / ABS_SLOTS, "%s: H = %lld gives %d H = %lld models (<= max_h = %lld)", who, (long long)H,
                 ABS_SLOTS, (long long)(H * ABS_SLOTS), (long long)pats_epipolar_max_h());
    PATS_REQUIRE(progressive == 0 || progressive == 1, "%s: progressive = %d must be 0 or 1", who, progressive);
    const int64_t chunks = ceil_div(H, ABS_HYP_THREADS);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "%s: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)", who, (long long)pairs,
                 (long long)pairs, (long long)chunks);
    hipLaunchKernelGGL(absolute_hypotheses_kernel, dim3((unsigned)(pairs * chunks)), dim3(ABS_HYP_THREADS), 0, as_stream(stream), points,
                       matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models, sample_idx,
                       n_models);
    return check_launch("absolute_hypotheses kernel");
}

extern "C" int pats_absolute_score_by_pair_f32(const float* points, const float* matches_r, const float* conf, const int64_t* pair_off,
                                               int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                               int64_t M, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                               int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, pats_stream_t stream) {
    const char* who = "absolute_score_by_pair";
    EPI_REQUIRE_PTR(points, 4);
    EPI_REQUIRE_PTR(matches_r, 8);
    EPI_REQUIRE_PTR(models, 4);
    EPI_REQUIRE_PTR(thr, 4);
    EPI_REQUIRE_PTR(counts, 4);
    EPI_REQUIRE_PTR(best, 4);
    EPI_REQUIRE_PTR(best_count, 8);
    PATS_REQUIRE(inlier, "%s: null inlier", who);
    EPI_REQUIRE_ALIGNED(conf, 4);                       // optional pointers: null is aligned
    EPI_REQUIRE_ALIGNED(norm, 4);
    EPI_REQUIRE_ALIGNED(pair_off, 8);
    EPI_REQUIRE_ALIGNED(counts_in, 8);
    int rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h(who, M);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(!use_min_conf || conf, "%s: min_conf needs conf", who);
    PATS_REQUIRE(!use_min_conf || min_conf >= 0.0f, "%s: min_conf = %g must be a non-negative number", who, (double)min_conf);
    const int64_t chunks = ceil_div(M, ABS_CHUNK);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "%s: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)", who, (long long)pairs,
                 (long long)pairs, (long long)chunks);
    const int64_t longest = counts_in ? stride : cap;   // the staging comes from the sizes alone: no host read of the counts
    const int64_t even = (longest + 1) / 2 * 2;
    const int stage_n = (int)(even < ABS_STAGE ? (even < 2 ? 2 : even) : ABS_STAGE);
    if (!abs_lds_ready()) {
        set_error("%s: the device refused %d bytes of dynamic LDS per workgroup", who, ABS_LDS);
        return PATS_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    rc = fill_bytes(inlier, 0, (size_t)cap, st);
    if (rc != PATS_OK) return rc;
    const float* cf = use_min_conf ? conf : nullptr;    // without a threshold the confidence is not read
    hipLaunchKernelGGL(absolute_score_kernel, dim3((unsigned)(pairs * chunks)), dim3(ABS_THREADS), (size_t)stage_n * 5 * sizeof(float), st,
                       points, matches_r, cf, pair_off, counts_in, stride, cap, (int)chunks, models, (int)M, thr, norm, use_min_conf, min_conf,
                       stage_n, counts);
    rc = check_launch("absolute_score kernel");
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(absolute_argmax_kernel, dim3((unsigned)pairs), dim3(256), 0, st, counts, (int)M, best, best_count);
    rc = check_launch("absolute_argmax kernel");
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(absolute_mask_kernel, dim3((unsigned)pairs), dim3(ABS_MASK_THREADS), 0, st, points, matches_r, cf, pair_off, counts_in,
                       stride, cap, models, (int)M, thr, norm, use_min_conf, min_conf, best, best_count, inlier);
    return check_launch("absolute_mask kernel");
}
