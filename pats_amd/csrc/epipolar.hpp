// What the per-pair stages share (epipolar.hip: verification; hypotheses.hip, hypotheses5.hip, hypotheses7.hip: the 8-, 4-, 5- and
// 7-point hypotheses; pose.hip, pose_h.hip: the poses; homography.hip, fundamental.hip: the refits; polish.hip: the local optimisation):
// how a pair's segment of the match lists, its normalisation, a match's point and the winning model are read, the hypotheses' sampler
// with the front end of every minimal-sample kernel, and the host side: the checks of the generators, of the verifications and local
// optimisations and of the refit source, and the raising of a kernel's dynamic LDS limit (absolute.hip is a caller of these too).
// include/pats_amd.h states all of it.
#pragma once
#include "common.hpp"

namespace pats {

// the segment of pair p: ragged (pair_off) or strided (stride, counts_in); always inside [0, cap]
__device__ __forceinline__ void epi_segment(const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride,
                                            int64_t cap, int64_t p, int64_t& lo, uint32_t& n) {
    if (counts_in) {                                    // pairs * stride <= cap (checked on the host)
        int64_t c = counts_in[p];
        c = c < 0 ? 0 : (c > stride ? stride : c);
        lo = p * stride;
        n = (uint32_t)c;
    } else {
        int64_t a = pair_off[p], b = pair_off[p + 1];
        a = a < 0 ? 0 : (a > cap ? cap : a);
        b = b < 0 ? 0 : (b > cap ? cap : b);
        lo = a;
        n = b > a ? (uint32_t)(b - a) : 0u;             // cap < 2^31 (checked on the host)
    }
}

struct EpiNorm { float c0l, c1l, s0l, s1l, c0r, c1r, s0r, s1r; };

__device__ __forceinline__ EpiNorm epi_norm(const float* __restrict__ norm, int64_t p) {
    EpiNorm m{0.0f, 0.0f, 1.0f, 1.0f, 0.0f, 0.0f, 1.0f, 1.0f};
    if (norm) {
        const float* q = norm + p * 8;
        m = EpiNorm{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
    }
    return m;
}

// match i of the segment as (x_l, x_r); l0 = NaN unless the match participates
__device__ __forceinline__ void epi_load(const float2* __restrict__ ml, const float2* __restrict__ mr, const float* __restrict__ conf,
                                         uint32_t i, uint32_t n, bool has_norm, const EpiNorm& nm, bool gate, float min_conf,
                                         float& l0, float& l1, float& r0, float& r1) {
    l0 = __builtin_nanf("");
    l1 = r0 = r1 = 0.0f;
    if (i >= n) return;
    float2 a = ml[i], b = mr[i];
    if (has_norm) {                                     // one subtract, one multiply (no contraction: -ffp-contract=off)
        a.x = (a.x - nm.c0l) * nm.s0l; a.y = (a.y - nm.c1l) * nm.s1l;
        b.x = (b.x - nm.c0r) * nm.s0r; b.y = (b.y - nm.c1r) * nm.s1r;
    }
    bool ok = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(b.x) && __builtin_isfinite(b.y);
    if (gate) ok = ok && conf[i] >= min_conf;           // false for a NaN confidence
    l1 = a.y; r0 = b.x; r1 = b.y;
    if (ok) l0 = a.x;
}

// match i of the segment for a walk behind a byte mask (the verification's inliers, a pose's front mask): epi_load without the
// confidence gate, then THE mask rule - a match whose mask byte is 0 is not used: l0 = NaN.  Returns l0 as it was before the mask
// (NaN unless the four coordinates are finite), for the one walk that also tests the unmasked match
__device__ __forceinline__ float epi_load_masked(const float2* __restrict__ ml, const float2* __restrict__ mr, const uint8_t* __restrict__ mask,
                                                 uint32_t i, uint32_t n, bool has_norm, const EpiNorm& nm, float& l0, float& l1, float& r0,
                                                 float& r1) {
    epi_load(ml, mr, nullptr, i, n, has_norm, nm, false, 0.0f, l0, l1, r0, r1);
    const float unmasked = l0;
    if (i < n && mask[i] == 0) l0 = __builtin_nanf("");
    return unmasked;
}

// ---- the frame change of `swapped` (include/pats_amd.h): P = [[0,1,0],[1,0,0],[0,0,1]] exchanges the first two components ------
// i -> P i for the index of a 3-vector (P t), k -> P k P for the index of a row-major 3x3 (P R P: rows and columns)
__device__ __forceinline__ int frame_perm(int i, int swapped) { return swapped ? (i == 2 ? 2 : 1 - i) : i; }
__device__ __forceinline__ int hom_perm(int k, int swapped) {
    const int i = k / 3, j = k - 3 * i;
    return frame_perm(i, swapped) * 3 + frame_perm(j, swapped);
}

// ---- what a one-workgroup-per-pair walk folds: counts (integers: no order) and float64 sums (a FIXED order) --------------------
// the lanes of this wave whose pred holds, in every lane
__device__ __forceinline__ int wave_count(bool pred) { return __builtin_popcountll(__builtin_amdgcn_ballot_w64(pred)); }

// lane 0 of every wave stores the wave's partial - a count, or a sum lane 0 holds - to its slot of s (one partial per wave), or its
// C partials to columns at .. at + C - 1 of its row of s; behind a wg_barrier() whichever thread needs a total adds the waves in
// index order with wave_parts_total.  The total is added in the partials' own type: a count of matches fits it because a pair has
// fewer than 2^31 matches (epi_check_segments)
template <int WAVES, class T>
__device__ __forceinline__ void wave_parts_store(T (&s)[WAVES], int wave, int lane, T part) {
    if (lane == 0) s[wave] = part;
}
template <int C, int WAVES, int COLS, class T>
__device__ __forceinline__ void wave_parts_store(T (&s)[WAVES][COLS], int wave, int lane, const T (&part)[C], int at = 0) {
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) s[wave][at + c] = part[c];
    }
}
template <int WAVES, class T>
__device__ __forceinline__ T wave_parts_total(const T (&s)[WAVES]) {
    T total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += s[w];
    return total;
}
template <int WAVES, int COLS, class T>
__device__ __forceinline__ T wave_parts_total(const T (&s)[WAVES][COLS], int c) {
    T total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += s[w][c];
    return total;
}

// the float64 sum of a wave by a fixed tree - lane l takes lane l + 32, then + 16, ... + 1: lane 0 holds
// ((l0 + l32) + (l16 + l48)) + ..., the other lanes hold partial trees.  With the waves added in index order a sum depends on the
// sizes alone, never on the scheduling.  This is also the xor tree (lane ^ 32, ^ 16, ...) of include/pats_amd.h as lane 0 sees it:
// every lane that feeds lane 0 holds at each step what the xor form gives it, and a + b is b + a bit for bit
__device__ __forceinline__ double wave_sum_tree_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// the winner of pair p among its H models: model h clamped into 0 .. H - 1, h = best[p]
__device__ __forceinline__ const float* epi_winner(const float* __restrict__ models, int H, int h, int64_t p) {
    h = h < 0 ? 0 : (h >= H ? H - 1 : h);
    return models + (p * H + h) * 9;
}
__device__ __forceinline__ const float* epi_winner(const float* __restrict__ models, int H, const int32_t* __restrict__ best, int64_t p) {
    return epi_winner(models, H, best[p], p);
}

// ---- the hypotheses' sampler (include/pats_amd.h, "Per-pair hypotheses"): uint32 arithmetic that wraps ------------------------
__device__ __forceinline__ uint32_t epi_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// K draws of hypothesis h out of 0 .. m - 1 (K <= m) without replacement and without a rejection loop, in draw order: draw t takes
// the j_t-th index not drawn before, found by walking the earlier draws in ascending order (a sorted register array kept by
// insertion; every index below is a constant once the loops are unrolled)
template <int K>
__device__ __forceinline__ void epi_draw(uint64_t seed, uint32_t h, uint32_t m, uint32_t (&idx)[K]) {
    const uint32_t key = epi_mix(epi_mix(epi_mix((uint32_t)seed) ^ (uint32_t)(seed >> 32)) + h);
    uint32_t srt[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const uint32_t u = epi_mix(key + 0x9e3779b9u * (uint32_t)(t + 1));
        uint32_t j = (uint32_t)(((uint64_t)u * (uint64_t)(m - (uint32_t)t)) >> 32);        // < m - t
#pragma unroll
        for (int i = 0; i < t; ++i) j += srt[i] <= j ? 1u : 0u;                            // the j-th index not drawn before: < m
        idx[t] = j;
        srt[t] = j;
#pragma unroll
        for (int i = t - 1; i >= 0; --i) {
            const uint32_t lo_ = srt[i] < srt[i + 1] ? srt[i] : srt[i + 1], hi_ = srt[i] < srt[i + 1] ? srt[i + 1] : srt[i];
            srt[i] = lo_; srt[i + 1] = hi_;
        }
    }
}

// The front end of a minimal-sample kernel, one thread per sample h of pair p: the K draws of the pair's pool (progressive: the first
// max(K, ceil(n (h + 1) / H)) matches) go to the sample's row of sample_idx (if given) and their points, normalised if norm is given,
// to l0 .. r1.  EPI_SAMPLE_SHORT: the pair has fewer than K matches (workgroup-uniform), the row is -1 and nothing was drawn
enum EpiSample { EPI_SAMPLE_SHORT, EPI_SAMPLE_NOT_FINITE, EPI_SAMPLE_READY };

template <int K, class T>
__device__ __forceinline__ EpiSample epi_sample(const float* __restrict__ ml_, const float* __restrict__ mr_,
                                                const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride,
                                                int64_t cap, const int64_t* __restrict__ pair_seed, const float* __restrict__ norm,
                                                int progressive, int32_t* __restrict__ sample_idx, int64_t p, int h, int H, T (&l0)[K],
                                                T (&l1)[K], T (&r0)[K], T (&r1)[K]) {
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    int32_t* so = sample_idx ? sample_idx + (p * H + h) * K : nullptr;
    if (n < K) {
        if (so) {
#pragma unroll
            for (int t = 0; t < K; ++t) so[t] = -1;
        }
        return EPI_SAMPLE_SHORT;
    }
    uint32_t m = n;                                     // the pool: K <= m <= n
    if (progressive) {
        const int64_t q = ((int64_t)n * (h + 1) + H - 1) / H;
        m = q < K ? (uint32_t)K : (q > (int64_t)n ? n : (uint32_t)q);
    }
    uint32_t idx[K];                                    // the draws in draw order
    epi_draw<K>((uint64_t)pair_seed[p], (uint32_t)h, m, idx);
    if (so) {
#pragma unroll
        for (int t = 0; t < K; ++t) so[t] = (int32_t)idx[t];
    }
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const EpiNorm nm = epi_norm(norm, p);
    float2 xl[K], xr[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { xl[t] = ml[idx[t]]; xr[t] = mr[idx[t]]; }    // idx < m <= n: inside the segment
    __builtin_amdgcn_sched_barrier(0);                  // all 2 K loads are in flight before the first is waited for
    bool finite = true;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        float2 a = xl[t], c = xr[t];
        if (norm) {                                     // one subtract, one multiply (no contraction: -ffp-contract=off)
            a.x = (a.x - nm.c0l) * nm.s0l; a.y = (a.y - nm.c1l) * nm.s1l;
            c.x = (c.x - nm.c0r) * nm.s0r; c.y = (c.y - nm.c1r) * nm.s1r;
        }
        finite = finite && __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(c.x) && __builtin_isfinite(c.y);
        l0[t] = (T)a.x; l1[t] = (T)a.y; r0[t] = (T)c.x; r1[t] = (T)c.y;
    }
    return finite ? EPI_SAMPLE_READY : EPI_SAMPLE_NOT_FINITE;
}

// ---- host side: what every per-pair stage checks of its arguments before any launch (`what` = the entry point's name); the
// pointers go through epi_check_args (common.hpp) ------------------------------------------------------------------------------
// exactly one segment form, and sizes the kernels' 32-bit indices and epi_segment's clamps rely on
inline int epi_check_segments(const char* what, const int64_t* pair_off, const int64_t* counts_in, int64_t stride, int64_t pairs,
                              int64_t cap) {
    PATS_REQUIRE((pair_off != nullptr) != (counts_in != nullptr),
                 "%s: exactly one of pair_off (ragged segments) and counts_in (strided segments) must be given", what);
    PATS_REQUIRE(pairs >= 1 && pairs <= 0x7fffffff, "%s: pairs = %lld (1 .. 2^31 - 1)", what, (long long)pairs);
    PATS_REQUIRE(cap >= 0 && cap < 0x7fffffff, "%s: cap = %lld (0 .. 2^31 - 2)", what, (long long)cap);
    if (counts_in) {
        PATS_REQUIRE(stride >= 1, "%s: stride = %lld must be at least 1", what, (long long)stride);
        PATS_REQUIRE(stride <= cap && pairs <= cap / stride, "%s: pairs * stride = %lld * %lld exceeds cap = %lld", what,
                     (long long)pairs, (long long)stride, (long long)cap);
    }
    return PATS_OK;
}

// the number of models per pair
inline int epi_check_h(const char* what, int64_t H) {
    PATS_REQUIRE(H >= 1 && H <= pats_epipolar_max_h(), "%s: H = %lld (1 .. max_h = %lld)", what, (long long)H,
                 (long long)pats_epipolar_max_h());
    return PATS_OK;
}

// what the minimal-sample generators check alike (first = the first list, by its name: matches_l, or the absolute branch's points;
// models_per_sample = 1, 10, 3 or 4 slots; n_models is null where the entry has none); chunks = the workgroups of `threads` samples per pair
inline int epi_check_hypotheses(const char* who, const EpiArg& first, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed, const float* norm,
                                int progressive, const float* models, const int32_t* sample_idx, const int32_t* n_models,
                                int models_per_sample, int threads, int64_t& chunks) {
    int rc = epi_check_args(who, {first, {"matches_r", matches_r, 8}, {"pair_seed", pair_seed, 8}, {"models", models, 4}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"norm", norm, 4}, {"sample_idx", sample_idx, 4}, {"n_models", n_models, 4}, {"pair_off", pair_off, 8},
                              {"counts_in", counts_in, 8}}, false);
    if (rc != PATS_OK) return rc;
    rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap);
    if (rc != PATS_OK) return rc;
    rc = epi_check_h(who, H);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(H <= pats_epipolar_max_h() / models_per_sample, "%s: H = %lld gives %d H = %lld models (<= max_h = %lld)", who,
                 (long long)H, models_per_sample, (long long)(H * models_per_sample), (long long)pats_epipolar_max_h());
    PATS_REQUIRE(progressive == 0 || progressive == 1, "%s: progressive = %d must be 0 or 1", who, progressive);
    chunks = ceil_div(H, threads);
    PATS_REQUIRE(chunks <= 0x7fffffff / pairs, "%s: pairs = %lld gives a grid of %lld x %lld workgroups (< 2^31)", who, (long long)pairs,
                 (long long)pairs, (long long)chunks);
    return PATS_OK;
}

// What every verification and local optimisation checks alike before it launches, in this order: the required pointers - the first
// list (by its name), matches_r, models, thr, then the entry's `outputs` in its own order -, the alignment of the optional ones (conf,
// norm, pair_off, counts_in, then `optional`, the entry's own: moments, or best; null is aligned), the segments, the number of models
// and the two rules of the confidence gate
inline int epi_check_scored(const char* who, const EpiArg& first, const float* matches_r, const float* models, const float* thr,
                            std::initializer_list<EpiArg> outputs, const float* conf, const float* norm, const int64_t* pair_off,
                            int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, int use_min_conf, float min_conf,
                            const EpiArg& optional = {"", nullptr, 1}) {
    int rc = epi_check_args(who, {first, {"matches_r", matches_r, 8}, {"models", models, 4}, {"thr", thr, 4}}, true);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_args(who, outputs, true)) != PATS_OK) return rc;
    rc = epi_check_args(who, {{"conf", conf, 4}, {"norm", norm, 4}, {"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}, optional}, false);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    if ((rc = epi_check_h(who, H)) != PATS_OK) return rc;
    PATS_REQUIRE(!use_min_conf || conf, "%s: min_conf needs conf", who);
    PATS_REQUIRE(!use_min_conf || min_conf >= 0.0f, "%s: min_conf = %g must be a non-negative number", who, (double)min_conf);
    return PATS_OK;
}

// the source of a refit - moments, or models and best - and its frame flag.  With moments the kernels get no models: models is
// nulled and H set to 1, the launch's arguments
inline int epi_check_refit_source(const char* who, const double* moments, const float*& models, const int32_t* best, int64_t& H, int swapped) {
    PATS_REQUIRE(swapped == 0 || swapped == 1, "%s: swapped = %d must be 0 or 1", who, swapped);
    PATS_REQUIRE(moments || (models && best), "%s: the refit needs moments, or models and best (the winning model)", who);
    if (models) {
        const int rc = epi_check_h(who, H);
        if (rc != PATS_OK) return rc;
    }
    if (moments) { models = nullptr; H = 1; }
    return PATS_OK;
}

// ---- adaptive verification (adaptive.hip): the arguments of pats_*_score_adaptive_by_pair_f32 and the two launchers a branch hands
// to the shared host side - its score kernel restricted to the models [h_lo, h_hi) of pairs that have not stopped, and its mask kernel
struct AdaptiveCall {
    const float *matches_l, *matches_r, *conf;
    const int64_t* pair_off;
    int64_t stride;
    const int64_t* counts_in;
    int64_t pairs, cap;
    const float* models;
    int64_t H;
    const float *thr, *norm;
    int use_min_conf;
    float min_conf;
    int32_t *counts, *best;
    int64_t* best_count;
    uint8_t* inlier;
    double* moments;
    void* workspace;
    size_t workspace_bytes;
    pats_stream_t stream;
    double confidence;
    int sample_size, models_per_sample;
    int64_t round_models;
    int32_t *used, *participating;
};
constexpr int ADAPTIVE_TILE = 2048;                    // matches per score workgroup and models per score workgroup (epipolar.hip asserts it)
constexpr int ADAPTIVE_CHUNK = 256;
// conf = the confidence list if it gates, else null; tiles = ceil(longest segment / ADAPTIVE_TILE) >= 1
typedef int (*AdaptiveScoreRound)(const AdaptiveCall& c, const float* conf, int tiles, int h_lo, int h_hi, const int32_t* stopped,
                                  hipStream_t st);
typedef int (*AdaptiveMask)(const AdaptiveCall& c, const float* conf, hipStream_t st);
size_t adaptive_workspace_bytes(int64_t pairs);
int adaptive_score_by_pair(const char* who, const AdaptiveCall& c, AdaptiveScoreRound score_round, AdaptiveMask mask);

}  // namespace pats
