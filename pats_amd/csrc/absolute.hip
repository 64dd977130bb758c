// The absolute-pose branch of the per-pair stages: a match of the left (database) image is lifted through that image's depth map to a
// metric 3-D point, the right (query) camera is hypothesised from three lifted matches (P3P) and verified by reprojection, and the
// winner is refitted on its inliers.  Four entry points, each a fixed number of launches for the whole batch and no host read.
// include/pats_amd.h states the definitions ("Per-pair absolute pose from depth", "Per-pair absolute local optimisation");
// docs/kernels.md 4.21 and 4.22 the design.
//
//   lift        absolute_lift_kernel: one workgroup of ABS_LIFT_THREADS per pair walks the segment; abs_lift_one is the whole
//               definition of one match (float32, no contraction).  Every row of the segment is stored (a point, or three NaNs), the
//               rows outside every segment were zeroed before the launch; the count is the count fold of epipolar.hpp
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
//   argmax      verify_argmax_kernel (verify.hpp), the verification's own: the largest count, the lowest index that holds it (0 for no
//               inlier)
//   mask        absolute_mask_kernel: the winner's verdict for every match with abs_test2, so the mask's sum is best_count exactly
//   polish      absolute_polish_kernel ("Per-pair absolute local optimisation"; docs/kernels.md 4.22): one workgroup of
//               ABS_POLISH_THREADS per pair walks ALL rounds "refit the winner on its inliers, verify the refit" in one launch.  The
//               segment is staged once through abs_load into the score kernel's five planes (a longer one is walked in global memory:
//               the same values).  A pass tests every match with abs_test2 against the round's float32 model - the count, and the
//               mask of all the round's passes: recomputed, never stored - and adds an inlier's 28 float64 sums (J^T J, J^T e, |e|^2 of
//               the reprojection error) at the float64 model the next Gauss-Newton step starts from; the sums are reduced in a FIXED
//               order (thread-local in index order, the xor tree over the wave, the waves in order), thread 0 solves the 6 x 6 system
//               by Cholesky and applies the Rodrigues update; behind the last step R is made orthonormal and the model cast to
//               float32.  The best round's model stays in LDS; one last pass writes its mask.  No atomics, no workspace
#include "common.hpp"
#include "epipolar.hpp"
#include "p3p.hpp"
#include "verify.hpp"

namespace pats {

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
        cnt += wave_count(ok);
        if (i < n) {
            const int64_t r = lo + i;
            points[r * 3 + 0] = ok ? x0 * d : nan;
            points[r * 3 + 1] = ok ? x1 * d : nan;
            points[r * 3 + 2] = ok ? d : nan;
            valid[r] = ok ? (uint8_t)1 : (uint8_t)0;
        }
    }
    wave_parts_store(s_cnt, wave, lane, cnt);
    wg_barrier();
    if (tid == 0) lift_count[p] = (int64_t)wave_parts_total(s_cnt);
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

// The workgroup of `threads` stages matches 0 .. count - 1 of the segment through abs_load into the five planes of stage_n slots each:
// count = n, or - the score kernel's two-match trips - n rounded up to even, whose last slot then holds the NaN X0 of a match that
// takes no part.  count <= stage_n; the caller's barrier follows
__device__ __forceinline__ void abs_stage_segment(float* __restrict__ stage, int stage_n, uint32_t count, int tid, int threads,
                                                  const float* __restrict__ X_, const float2* __restrict__ mr, const float* __restrict__ conf,
                                                  uint32_t n, bool has_norm, const EpiNorm& nm, bool gate, float min_conf) {
    for (uint32_t i = tid; i < count; i += threads) {
        float a[5];
        abs_load(X_, mr, conf, i, n, has_norm, nm, gate, min_conf, a[0], a[1], a[2], a[3], a[4]);
#pragma unroll
        for (int k = 0; k < 5; ++k) stage[k * stage_n + i] = a[k];
    }
}

// THE arithmetic of the test, two matches against one model m = [R | t] row-major: Y_k = fma(m[4k], X0, fma(m[4k+1], X1,
// fma(m[4k+2], X2, m[4k+3]))), d_k = fma(-r_k, Y2, Y_k), s = fma(d0, d0, d1 d1), lim = t2 (Y2 Y2); inlier iff Y2 > 0 and s <= lim
__device__ __forceinline__ void abs_test2(const float (&m)[12], float t2, v2f X0, v2f X1, v2f X2, v2f r0, v2f r1, v2f& s,
                                          v2f& lim, v2f& y2) {
    const v2f y0 = pk_fma(pk_splat(m[0]), X0, pk_fma(pk_splat(m[1]), X1, pk_fma(pk_splat(m[2]), X2, pk_splat(m[3]))));
    const v2f y1 = pk_fma(pk_splat(m[4]), X0, pk_fma(pk_splat(m[5]), X1, pk_fma(pk_splat(m[6]), X2, pk_splat(m[7]))));
    y2 = pk_fma(pk_splat(m[8]), X0, pk_fma(pk_splat(m[9]), X1, pk_fma(pk_splat(m[10]), X2, pk_splat(m[11]))));
    const v2f d0 = pk_fma(-r0, y2, y0);
    const v2f d1 = pk_fma(-r1, y2, y1);
    s = pk_fma(d0, d0, d1 * d1);
    lim = pk_splat(t2) * (y2 * y2);
}

__device__ __forceinline__ int abs_count2(v2f s, v2f lim, v2f y2) {
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
                                           const EpiNorm& nm, bool gate, float min_conf, v2f& X0, v2f& X1, v2f& X2, v2f& r0,
                                           v2f& r1) {
    if (staged) {                                       // stage_n is even and the planes are padded with NaN X0 up to it: 2 q + 1 < stage_n
        const v2f* s2 = reinterpret_cast<const v2f*>(stage);
        const int half = stage_n / 2;
        X0 = s2[q]; X1 = s2[half + q]; X2 = s2[2 * half + q]; r0 = s2[3 * half + q]; r1 = s2[4 * half + q];
    } else {
        float a[5], c[5];
        abs_load(X_, mr, conf, 2 * q, n, has_norm, nm, gate, min_conf, a[0], a[1], a[2], a[3], a[4]);
        abs_load(X_, mr, conf, 2 * q + 1, n, has_norm, nm, gate, min_conf, c[0], c[1], c[2], c[3], c[4]);
        X0 = v2f{a[0], c[0]}; X1 = v2f{a[1], c[1]}; X2 = v2f{a[2], c[2]}; r0 = v2f{a[3], c[3]}; r1 = v2f{a[4], c[4]};
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

    if (staged) abs_stage_segment(abs_stage, stage_n, 2 * n2, tid, ABS_THREADS, X_, mr, conf, n, norm != nullptr, nm, gate != 0, min_conf);
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
                v2f X0 = pk_splat(__builtin_nanf("")), X1 = pk_splat(0.0f), X2 = X1, r0 = X1, r1 = X1;
                if (q < n2) abs_fetch2(staged, abs_stage, stage_n, X_, mr, conf, q, n, norm != nullptr, nm, gate != 0, min_conf, X0, X1, X2, r0, r1);
                v2f s, lim, y2;
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
        v2f s, lim, y2;
        abs_test2(e, t2, pk_splat(a[0]), pk_splat(a[1]), pk_splat(a[2]), pk_splat(a[3]), pk_splat(a[4]), s, lim, y2);
        inlier[lo + i] = y2.x > 0.0f && s.x <= lim.x ? 1 : 0;
    }
}

// ---- local optimisation (include/pats_amd.h, "Per-pair absolute local optimisation") ----------------------------------------------
constexpr int ABS_POLISH_THREADS = 512;                 // the walk whose width fixes the sums' bits
constexpr int ABS_POLISH_WAVES = ABS_POLISH_THREADS / WAVE;
constexpr int ABS_POLISH_MAX_ROUNDS = 16;
constexpr int ABS_POLISH_MAX_STEPS = 8;
constexpr int ABS_POLISH_MIN_INLIERS = 4;
constexpr int ABS_SUMS = 28;                            // A's upper triangle row by row (21), b (6), S (1)

// match i of the segment as the passes see it: from the staged planes, or through abs_load (staged is workgroup-uniform)
__device__ __forceinline__ void abs_fetch1(bool staged, const float* __restrict__ stage, int stage_n, const float* __restrict__ X_,
                                           const float2* __restrict__ mr, const float* __restrict__ conf, uint32_t i, uint32_t n, bool has_norm,
                                           const EpiNorm& nm, bool gate, float min_conf, float (&a)[5]) {
    if (staged) {
        a[0] = __builtin_nanf("");
        a[1] = a[2] = a[3] = a[4] = 0.0f;
        if (i < n) {                                    // n <= stage_n, the slots per plane the launch allocated
#pragma unroll
            for (int k = 0; k < 5; ++k) a[k] = stage[k * stage_n + i];
        }
    } else {
        abs_load(X_, mr, conf, i, n, has_norm, nm, gate, min_conf, a[0], a[1], a[2], a[3], a[4]);
    }
}

// THE sums of one inlier at the float64 model m = [R | t]: every sum and product rounded once, left to right
__device__ __forceinline__ void abs_polish_accumulate(const double (&m)[12], const float (&a)[5], double (&acc)[ABS_SUMS]) {
    const double X0 = (double)a[0], X1 = (double)a[1], X2 = (double)a[2];
    const double Y0 = ((m[0] * X0 + m[1] * X1) + m[2] * X2) + m[3];
    const double Y1 = ((m[4] * X0 + m[5] * X1) + m[6] * X2) + m[7];
    const double Y2 = ((m[8] * X0 + m[9] * X1) + m[10] * X2) + m[11];
    const double iz = 1.0 / Y2, u = Y0 * iz, v = Y1 * iz;
    const double e0 = u - (double)a[3], e1 = v - (double)a[4];
    const double uv = u * v;
    const double J0[6] = {-uv, 1.0 + u * u, -v, iz, 0.0, -(u * iz)};
    const double J1[6] = {-(1.0 + v * v), uv, u, 0.0, iz, -(v * iz)};
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) acc[k++] += J0[r] * J0[c] + J1[r] * J1[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] += J0[r] * e0 + J1[r] * e1;
    acc[27] += e0 * e0 + e1 * e1;
}

// one Gauss-Newton step on the reduced sums s, on ONE thread: A = L L^T in index order without pivoting, d = -A^-1 b, the left
// update by Rodrigues' formula.  false = "no step" (m is then not to be used)
__device__ __forceinline__ bool abs_polish_step(const double (&s)[ABS_SUMS], double (&m)[12]) {
    double A[6][6], L[6][6], y[6], d[6];
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) { A[r][c] = s[k]; A[c][r] = s[k]; ++k; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double p = A[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) p -= L[j][q] * L[j][q];
        ok = ok && __builtin_isfinite(p) && p > 1e-12 * A[j][j];
        const double l = __builtin_sqrt(p);
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double x = A[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) x -= L[i][q] * L[j][q];
            L[i][j] = x / l;
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {                       // L y = -b
        double x = -s[21 + i];
#pragma unroll
        for (int q = 0; q < i; ++q) x -= L[i][q] * y[q];
        y[i] = x / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                      // L^T d = y
        double x = y[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) x -= L[q][i] * d[q];
        d[i] = x / L[i][i];
    }
    // exp([w]x) = I + a [w]x + b [w]x^2,  a = sin(th) / th,  b = 2 sin^2(th / 2) / th^2,  [w]x^2 = w w^T - th^2 I
    const double w0 = d[0], w1 = d[1], w2 = d[2];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    double E[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    if (th2 > 0.0) {
        const double th = __builtin_sqrt(th2), sh = sin(0.5 * th);
        const double a = sin(th) / th, b = 2.0 * (sh * sh) / th2;
        E[0][0] = 1.0 + b * (w0 * w0 - th2); E[0][1] = b * (w0 * w1) - a * w2;     E[0][2] = b * (w0 * w2) + a * w1;
        E[1][0] = b * (w0 * w1) + a * w2;     E[1][1] = 1.0 + b * (w1 * w1 - th2); E[1][2] = b * (w1 * w2) - a * w0;
        E[2][0] = b * (w0 * w2) - a * w1;     E[2][1] = b * (w1 * w2) + a * w0;     E[2][2] = 1.0 + b * (w2 * w2 - th2);
    }
    double o[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[4 * r + c] = (E[r][0] * m[c] + E[r][1] * m[4 + c]) + E[r][2] * m[8 + c];
        o[4 * r + 3] = ((E[r][0] * m[3] + E[r][1] * m[7]) + E[r][2] * m[11]) + d[3 + r];
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) { ok = ok && __builtin_isfinite(o[q]); m[q] = o[q]; }
    return ok;
}

// R <- R + R (I - R^T R) / 2: one Newton step towards the nearest rotation.  The steps leave R^T R where the float32 input had it
// (eps32 off the identity), the step squares that distance
__device__ __forceinline__ void abs_polish_orthonormal(double (&m)[12]) {
    double G[3][3], o[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = (r == c ? 1.0 : 0.0) - ((m[r] * m[c] + m[4 + r] * m[4 + c]) + m[8 + r] * m[8 + c]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = m[4 * r + c] + 0.5 * ((m[4 * r] * G[0][c] + m[4 * r + 1] * G[1][c]) + m[4 * r + 2] * G[2][c]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[4 * r + c] = o[3 * r + c];
}

// One workgroup per pair walks all rounds.  A round's passes over the segment: the first tests with m_r (abs_test2, the count) and sums
// at m_r widened; passes 2 .. G sum at the stepped float64 model over the SAME matches - the mask is m_r's verdict again, not a copy.
// Every pass reduces its ABS_SUMS thread-local sums (ascending i, stride ABS_POLISH_THREADS) by the xor tree over the wave, then the
// waves in order; thread 0 takes the step.  stage_n = the slots per plane of dynamic LDS: min(longest possible segment, ABS_STAGE)
__global__ void __launch_bounds__(ABS_POLISH_THREADS)
absolute_polish_kernel(const float* __restrict__ points, const float* __restrict__ mr_, const float* __restrict__ conf_,
                       const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                       const float* __restrict__ models, int M, const float* __restrict__ thr, const float* __restrict__ norm, int gate,
                       float min_conf, const int32_t* __restrict__ best, int rounds, int steps, int stage_n, float* __restrict__ model_out,
                       int64_t* __restrict__ best_count, uint8_t* __restrict__ inlier, int32_t* __restrict__ best_round,
                       int32_t* __restrict__ counts_out, double* __restrict__ cost_out) {
    extern __shared__ __attribute__((aligned(16))) float abs_polish_stage[];
    __shared__ double part[ABS_POLISH_WAVES][ABS_SUMS];
    __shared__ double s_sum[ABS_SUMS];
    __shared__ double s_m64[12];
    __shared__ float s_model[12], s_model_best[12];
    __shared__ int s_wcnt[ABS_POLISH_WAVES];
    __shared__ int s_state;                             // after a step: 0 = step on, 1 = a new model is in s_model, 2 = the walk has ended
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const float t = thr[p];
    const bool live_t = t >= 0.0f;                      // NaN or negative threshold: no match is an inlier of any model
    const float t2 = t * t;
    const float* X_ = points + lo * 3;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const float* conf = conf_ ? conf_ + lo : nullptr;
    const EpiNorm nm = epi_norm(norm, p);
    const bool staged = n <= (uint32_t)stage_n;         // workgroup-uniform

    // ---- stage, and round 0's model -----------------------------------------------------------------------------------------
    if (staged) abs_stage_segment(abs_polish_stage, stage_n, n, tid, ABS_POLISH_THREADS, X_, mr, conf, n, norm != nullptr, nm, gate != 0, min_conf);
    if (tid < 12) {
        int h = best ? best[p] : 0;                     // a null best: M == 1
        h = h < 0 ? 0 : (h >= M ? M - 1 : h);
        s_model[tid] = models[((int64_t)p * M + h) * 12 + tid];
    }
    wg_barrier();

    int best_c = -1, best_r = 0;                        // workgroup-uniform: every thread computes every count and cost
    double best_S = 0.0, last_S = 0.0;
    int last_r = 0, last_c = 0;
#pragma unroll 1
    for (int r = 0; r <= ABS_POLISH_MAX_ROUNDS; ++r) {
        float e[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) e[k] = s_model[k];
        const float mine_m = tid < 12 ? s_model[tid] : 0.0f;
        bool ended = false;
#pragma unroll 1
        for (int g = 0; g < ABS_POLISH_MAX_STEPS; ++g) {
            // ---- one pass: support(m_r) and the sums at the model the next step starts from -------------------------------------
            double m[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) m[k] = g == 0 ? (double)e[k] : s_m64[k];
            double acc[ABS_SUMS];
#pragma unroll
            for (int k = 0; k < ABS_SUMS; ++k) acc[k] = 0.0;
            int wcnt = 0;
            if (live_t) {                               // workgroup-uniform
                for (uint32_t i0 = 0; i0 < n; i0 += ABS_POLISH_THREADS) {
                    float a[5];
                    abs_fetch1(staged, abs_polish_stage, stage_n, X_, mr, conf, i0 + tid, n, norm != nullptr, nm, gate != 0, min_conf, a);
                    v2f s, lim, y2;
                    abs_test2(e, t2, pk_splat(a[0]), pk_splat(a[1]), pk_splat(a[2]), pk_splat(a[3]), pk_splat(a[4]), s, lim, y2);
                    const bool in = y2.x > 0.0f && s.x <= lim.x;
                    wcnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
                    if (in) abs_polish_accumulate(m, a, acc);
                }
            }
#pragma unroll
            for (int k = 0; k < ABS_SUMS; ++k) {
                double v = acc[k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                if (lane == 0) part[wave][k] = v;
            }
            if (lane == 0) s_wcnt[wave] = wcnt;
            wg_barrier();
            if (tid < ABS_SUMS) {
                double v = 0.0;
#pragma unroll
                for (int w = 0; w < ABS_POLISH_WAVES; ++w) v += part[w][tid];
                s_sum[tid] = v;
            }
            wg_barrier();
            int c = 0;
#pragma unroll
            for (int w = 0; w < ABS_POLISH_WAVES; ++w) c += s_wcnt[w];
            if (g == 0) {                               // (c_r, S_r): the best rule, and the walk's end
                const double S = s_sum[27];
                if (tid == 0) { counts_out[p * (rounds + 1) + r] = c; cost_out[p * (rounds + 1) + r] = S; }
                last_r = r; last_c = c; last_S = S;
                if (c > best_c || (c == best_c && S < best_S)) {
                    best_c = c; best_S = S; best_r = r;
                    if (tid < 12) s_model_best[tid] = mine_m;
                }
                if (r >= rounds) { ended = true; break; }
            }
            // ---- thread 0: the step; behind the last one the cast, and whether the model repeats ------------------------------
            if (tid == 0) {
                double sm[ABS_SUMS], mm[12];
#pragma unroll
                for (int k = 0; k < ABS_SUMS; ++k) sm[k] = s_sum[k];
#pragma unroll
                for (int k = 0; k < 12; ++k) mm[k] = m[k];
                bool ok = c >= ABS_POLISH_MIN_INLIERS && abs_polish_step(sm, mm);
                int state = 0;
                if (ok && g + 1 < steps) {
#pragma unroll
                    for (int k = 0; k < 12; ++k) s_m64[k] = mm[k];
                } else {
                    float f[12];
                    if (ok) {
                        abs_polish_orthonormal(mm);
#pragma unroll
                        for (int k = 0; k < 12; ++k) { f[k] = (float)mm[k]; ok = ok && __builtin_isfinite(f[k]); }
                    }
                    bool same = true;                   // "no refit" returns m_r itself
                    if (ok) {
#pragma unroll
                        for (int k = 0; k < 12; ++k) {
                            same = same && __float_as_uint(f[k]) == __float_as_uint(s_model[k]);
                            s_model[k] = f[k];
                        }
                    }
                    state = same ? 2 : 1;
                }
                s_state = state;
            }
            wg_barrier();
            if (s_state != 0) { ended = s_state == 2; break; }
        }
        if (ended) break;
    }
    if (tid == 0) {                                     // a walk that ended early: every later round repeats the last one scored
        for (int q = last_r + 1; q <= rounds; ++q) { counts_out[p * (rounds + 1) + q] = last_c; cost_out[p * (rounds + 1) + q] = last_S; }
    }
    wg_barrier();                                       // the best model is in LDS

    // ---- outputs, and the best round's mask ----------------------------------------------------------------------------------
    if (tid < 12) model_out[p * 12 + tid] = s_model_best[tid];
    if (tid == 0) { best_count[p] = (int64_t)best_c; best_round[p] = best_r; }
    if (!live_t || best_c <= 0) return;                 // the mask was zeroed before the launch
    float e[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) e[k] = s_model_best[k];
    for (uint32_t i0 = 0; i0 < n; i0 += ABS_POLISH_THREADS) {
        const uint32_t i = i0 + tid;
        float a[5];
        abs_fetch1(staged, abs_polish_stage, stage_n, X_, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, a);
        v2f s, lim, y2;
        abs_test2(e, t2, pk_splat(a[0]), pk_splat(a[1]), pk_splat(a[2]), pk_splat(a[3]), pk_splat(a[4]), s, lim, y2);
        if (i < n) inlier[lo + i] = y2.x > 0.0f && s.x <= lim.x ? 1 : 0;
    }
}

// stage_n, the slots per plane of dynamic LDS a launch allocates: the longest possible segment - from the sizes alone: no host read of
// the counts - rounded up to `granule` (2 for the score kernel's two-match trips), at least one granule and at most ABS_STAGE
static int abs_stage_slots(const int64_t* counts_in, int64_t stride, int64_t cap, int granule) {
    const int64_t longest = counts_in ? stride : cap;
    const int64_t slots = (longest + granule - 1) / granule * granule;
    return (int)(slots < ABS_STAGE ? (slots < granule ? granule : slots) : ABS_STAGE);
}

}  // namespace pats

using namespace pats;

// ---- the entry points (include/pats_amd.h) ---------------------------------------------------------------------------------------
extern "C" int pats_lift_by_pair_f32(const float* matches, const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs,
                                     int64_t cap, const float* norm, const int64_t* depth_table, const float* max_depth, int interp,
                                     int use_max_jump, float max_jump, float* points, uint8_t* valid, int64_t* lift_count,
                                     pats_stream_t stream) {
    const char* who = "lift_by_pair";
    int rc = epi_check_args(who, {{"matches", matches, 8}, {"depth_table", depth_table, 8}, {"points", points, 4}, {"valid", valid, 1},
                                  {"lift_count", lift_count, 8}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"norm", norm, 4}, {"max_depth", max_depth, 4}, {"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}}, false);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    PATS_REQUIRE(interp == 0 || interp == 1, "%s: interp = %d must be 0 (nearest) or 1 (bilinear)", who, interp);
    PATS_REQUIRE(use_max_jump == 0 || use_max_jump == 1, "%s: use_max_jump = %d must be 0 or 1", who, use_max_jump);
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
    int64_t chunks;
    const int rc = epi_check_hypotheses("absolute_hypotheses_by_pair", {"points", points, 4}, matches_r, pair_off, stride, counts_in, pairs, cap, H,
                                        pair_seed, norm, progressive, models, sample_idx, n_models, ABS_SLOTS, ABS_HYP_THREADS, chunks);
    if (rc != PATS_OK) return rc;
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
    int rc = epi_check_scored(who, {"points", points, 4}, matches_r, models, thr,
                              {{"counts", counts, 4}, {"best", best, 4}, {"best_count", best_count, 8}, {"inlier", inlier, 1}}, conf, norm, pair_off,
                              stride, counts_in, pairs, cap, M, use_min_conf, min_conf);
    if (rc != PATS_OK) return rc;
    const int64_t chunks = ceil_div(M, ABS_CHUNK);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "%s: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)", who, (long long)pairs,
                 (long long)pairs, (long long)chunks);
    const int stage_n = abs_stage_slots(counts_in, stride, cap, 2);
    static DeviceGrants grants;
    if (!grants.get({{(const void*)absolute_score_kernel, ABS_LDS}}).granted) {
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
    hipLaunchKernelGGL(verify_argmax_kernel<ARGMAX_THREADS>, dim3((unsigned)pairs), dim3(ARGMAX_THREADS), 0, st, counts, (int)M, best, best_count);
    rc = check_launch("absolute_argmax kernel");
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(absolute_mask_kernel, dim3((unsigned)pairs), dim3(ABS_MASK_THREADS), 0, st, points, matches_r, cf, pair_off, counts_in,
                       stride, cap, models, (int)M, thr, norm, use_min_conf, min_conf, best, best_count, inlier);
    return check_launch("absolute_mask kernel");
}

extern "C" int pats_absolute_polish_by_pair_f32(const float* points, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                                int64_t M, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                                const int32_t* best, int rounds, int steps, float* model, int64_t* best_count,
                                                uint8_t* inlier, int32_t* best_round, int32_t* counts, double* cost, pats_stream_t stream) {
    const char* who = "absolute_polish_by_pair";
    int rc = epi_check_scored(who, {"points", points, 4}, matches_r, models, thr,
                              {{"model", model, 4}, {"best_count", best_count, 8}, {"inlier", inlier, 1}, {"best_round", best_round, 4},
                               {"counts", counts, 4}, {"cost", cost, 8}},
                              conf, norm, pair_off, stride, counts_in, pairs, cap, M, use_min_conf, min_conf, {"best", best, 4});
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(rounds >= 1 && rounds <= ABS_POLISH_MAX_ROUNDS, "%s: rounds = %d (1 .. %d)", who, rounds, ABS_POLISH_MAX_ROUNDS);
    PATS_REQUIRE(steps >= 1 && steps <= ABS_POLISH_MAX_STEPS, "%s: steps = %d (1 .. %d)", who, steps, ABS_POLISH_MAX_STEPS);
    PATS_REQUIRE(best || M == 1, "%s: null best needs M == 1, got M = %lld", who, (long long)M);
    const int stage_n = abs_stage_slots(counts_in, stride, cap, 1);
    static DeviceGrants grants;
    if (!grants.get({{(const void*)absolute_polish_kernel, ABS_LDS}}).granted) {
        set_error("%s: the device refused %d bytes of dynamic LDS per workgroup", who, ABS_LDS);
        return PATS_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    rc = fill_bytes(inlier, 0, (size_t)cap, st);
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(absolute_polish_kernel, dim3((unsigned)pairs), dim3(ABS_POLISH_THREADS), (size_t)stage_n * 5 * sizeof(float), st, points,
                       matches_r, use_min_conf ? conf : nullptr, pair_off, counts_in, stride, cap, models, (int)M, thr, norm, use_min_conf,
                       min_conf, best, rounds, steps, stage_n, model, best_count, inlier, best_round, counts, cost);
    return check_launch("absolute_polish kernel");
}
