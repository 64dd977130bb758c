// Per-pair verification of candidate models against the hand-over's matches, written once for both model families: for every pair of
// a batch H 3x3 models are tested against every match of the pair's segment, the model with the most inliers wins (lowest index on a
// tie), its inlier mask is written beside the match lists and - on request - the 9x9 moment matrix of its inliers, the input of a
// least-squares refit.  The MSAC entries rank by gain instead (the sum over a model's inliers of 1 - e^2 / thr^2, in units of 2^-20).
// No host read.  include/pats_amd.h states the definitions; docs/kernels.md 4.7 the design (4.11: the homographies, 4.12: the
// adaptive rounds).
// The file and the EPI_ constants are named like epipolar.hpp's epi_ helpers, which the homography branch shares as well.
//
// A family (verify.hpp, shared with polish.hip) is a struct with the two things that differ: test2, THE arithmetic of its test (two
// matches against one model), and accumulate, a match's contribution to the moments.
//   Epipolar    squared Sampson error against thr^2, without the division; the moments of q = vec(x_r x_l^T)
//   Homography  squared forward transfer error against thr^2, without the division; the moments of the two DLT rows A_i, B_i
//
//   score   verify_score_kernel<T, ROUND, GAIN>: grid = tiles x pairs x model chunks, 256 threads.  A thread keeps EPI_R = 8 matches
//           (normalised once, as four packed pairs of float2 lanes) in registers and walks the EPI_CHUNK = 256 models of its chunk;
//           a model is nine wave-uniform floats (scalar loads, one model ahead).  Per model: v_pk_fma_f32 on the four pairs, the
//           verdicts as wave ballots, their popcounts added on the scalar unit and kept by lane h % 64 in a counter register; every
//           64 models the register goes to LDS, at the end the four waves' counters are added and ONE integer atomic per workgroup
//           and model with a non-zero count goes to counts[p, h] (integer adds: the order does not matter).  Blocks past a segment's
//           end return.  ROUND: <false> is the fixed budget; <true> is one round of the adaptive verification (adaptive.hip) - the
//           models [h_begin, h_stop) only, and the workgroups of a pair that has stopped return on its flag.
//           GAIN (fixed budget only): <T, false, true> is the MSAC entries' kernel - beside the counts every lane turns its eight cells
//           into integer gains (verify_gain), the 64-lane integer sum of a model is taken one model behind (its crossbar steps wait
//           under the next model's arithmetic), lane h % 64 keeps it, and a second LDS array and ONE 64-bit integer atomic per
//           workgroup and model with a non-zero gain carry it to gains[p, h].  The <T, ROUND, false> kernels hold none of this.
//   argmax  verify_argmax_kernel (verify.hpp: the absolute branch launches it too), one for every family: one workgroup per pair over
//           counts[p, :], the largest count, the lowest index that holds it
//           verify_argmax_gain_kernel: the same over the int64 gains[p, :]; it reads counts[p, best] for best_count
//   mask    verify_mask_kernel<T>: one workgroup per pair, the winner's verdict for every match of the segment with the arithmetic of
//           the score kernel (same device function: the mask and the winner's count agree exactly), the moments in float64 in a fixed
//           order (thread-local in index order, an xor tree over the wave, the waves in order)
// A match that does not participate (outside the segment, gated by min_conf, a non-finite coordinate) carries a NaN x_l: every
// comparison with it is false, the inner loop needs no mask.
#include "common.hpp"
#include "epipolar.hpp"
#include "lane_reduce.hpp"
#include "verify.hpp"

namespace pats {

constexpr int EPI_THREADS = 256;
constexpr int EPI_WAVES = EPI_THREADS / WAVE;
constexpr int EPI_R = 8;                            // matches per thread
constexpr int EPI_TILE = EPI_THREADS * EPI_R; // matches per workgroup
constexpr int EPI_CHUNK = 256;                      // models per workgroup
constexpr int EPI_MAX_H = 65536;
static_assert(EPI_TILE == ADAPTIVE_TILE && EPI_CHUNK == ADAPTIVE_CHUNK, "adaptive.hip sizes the rounds' grids");

// ROUND = false: the fixed budget - models [0, H) in `chunks` chunks; h_begin, h_stop and stopped are not read.  ROUND = true: a round
// of the adaptive verification (adaptive.hip issues them) - models [h_begin, h_stop) in `chunks` chunks, and the workgroups of a
// pair whose stopped flag is set return at once.  GAIN = true (fixed budget only): the MSAC gains beside the counts - gains is not read
// otherwise, and the <T, ROUND, false> kernels hold none of its code
template <class T, bool ROUND, bool GAIN>
__global__ void __launch_bounds__(EPI_THREADS)
verify_score_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const float* __restrict__ conf_,
                    const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                    int pairs, int chunks, const float* __restrict__ models, int H, const float* __restrict__ thr,
                    const float* __restrict__ norm, int gate, float min_conf, int32_t* __restrict__ counts, int h_begin, int h_stop,
                    const int32_t* __restrict__ stopped, int64_t* __restrict__ gains) {
    static_assert(!(ROUND && GAIN), "the adaptive rounds' stopping rule is defined on counts");
    static_assert((int64_t)EPI_TILE << MSAC_GAIN_BITS <= (int64_t)1 << 31, "a workgroup's gain per model fits uint32");
    __shared__ int wave_cnt[EPI_WAVES][EPI_CHUNK];
    __shared__ uint32_t wave_gain[GAIN ? EPI_WAVES : 1][GAIN ? EPI_CHUNK : 1];
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
    const uint64_t i0 = (uint64_t)tile * EPI_TILE;
    if (i0 >= n) return;                                // workgroup-uniform
    const float t = thr[p];
    if (!(t >= 0.0f)) return;                           // NaN or negative threshold: the pair has no inliers (counts are zeroed)
    const float t2 = t * t;

    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const float* conf = conf_ ? conf_ + lo : nullptr;
    const EpiNorm nm = epi_norm(norm, p);
    v2f l0[EPI_R / 2], l1[EPI_R / 2], r0[EPI_R / 2], r1[EPI_R / 2];
#pragma unroll
    for (int k = 0; k < EPI_R / 2; ++k) {
        float a0, a1, a2, a3, c0, c1, c2, c3;
        epi_load(ml, mr, conf, (uint32_t)i0 + (uint32_t)((2 * k) * EPI_THREADS + tid), n, norm != nullptr, nm, gate != 0, min_conf, a0, a1, a2, a3);
        epi_load(ml, mr, conf, (uint32_t)i0 + (uint32_t)((2 * k + 1) * EPI_THREADS + tid), n, norm != nullptr, nm, gate != 0, min_conf, c0, c1, c2, c3);
        l0[k] = v2f{a0, c0}; l1[k] = v2f{a1, c1}; r0[k] = v2f{a2, c2}; r1[k] = v2f{a3, c3};
    }

    const int h_lo = (ROUND ? h_begin : 0) + chunk * EPI_CHUNK;           // the fixed budget: every model, [0, H)
    const int h_end = ROUND ? h_stop : H;
    const int nmod = h_end - h_lo < EPI_CHUNK ? h_end - h_lo : EPI_CHUNK;     // >= 1: chunks = ceil((h_end - h_begin) / EPI_CHUNK)
    const float* m = models + ((int64_t)p * H + h_lo) * 9;
    float e[9];
    verify_model(m, e);
    for (int h0 = 0; h0 < nmod; h0 += WAVE) {
        const int jn = nmod - h0 < WAVE ? nmod - h0 : WAVE;
        int acc = 0;
        uint32_t gacc = 0, gprev = 0;                 // gprev: this lane's sum for model j - 1, not yet added over the wave
        for (int j = 0; j < jn; ++j) {
            if (GAIN) {                                 // one model behind: the two crossbar steps wait under this model's arithmetic
                const uint32_t gs = wave_sum_u32(gprev, lane);                  // at most 512 x 2^20
                gacc = lane == j - 1 ? gs : gacc;
            }
            float en[9];
            const int hn = h0 + j + 1 < nmod ? h0 + j + 1 : h0 + j;            // one model ahead (the last one again: in bounds)
            verify_model(m + (int64_t)hn * 9, en);
            int cnt = 0;
            uint32_t g = 0;                                                     // this lane's eight cells: at most 8 x 2^20
#pragma unroll
            for (int k = 0; k < EPI_R / 2; ++k) {
                v2f s, lim, w;
                T::test2(e, t2, l0[k], l1[k], r0[k], r1[k], s, lim, w);
                // the two comparisons as ballots of their own, combined on the scalar unit
                cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(w.x > 0.0f) & __builtin_amdgcn_ballot_w64(s.x <= lim.x)) +
                       __builtin_popcountll(__builtin_amdgcn_ballot_w64(w.y > 0.0f) & __builtin_amdgcn_ballot_w64(s.y <= lim.y));
                if (GAIN) g += verify_gain(w.x > 0.0f && s.x <= lim.x, s.x, lim.x) + verify_gain(w.y > 0.0f && s.y <= lim.y, s.y, lim.y);
            }
            acc = lane == j ? cnt : acc;
            gprev = g;
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = en[k];
        }
        wave_cnt[wave][h0 + lane] = acc;                // h0 + lane < EPI_CHUNK; lanes past jn hold 0
        if (GAIN) {
            const uint32_t gs = wave_sum_u32(gprev, lane);                      // the group's last model
            wave_gain[wave][h0 + lane] = lane == jn - 1 ? gs : gacc;
        }
    }
    wg_barrier();
    if (tid < nmod) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < EPI_WAVES; ++w) s += wave_cnt[w][tid];
        if (s) atomicAdd(&counts[(int64_t)p * H + h_lo + tid], s);
        if (GAIN) {
            uint32_t gs = 0;
#pragma unroll
            for (int w = 0; w < EPI_WAVES; ++w) gs += wave_gain[w][tid];
            if (gs) atomicAdd(reinterpret_cast<unsigned long long*>(&gains[(int64_t)p * H + h_lo + tid]), (unsigned long long)gs);
        }
    }
}

// the MSAC sibling: the largest gain of gains[p, :], the lowest index that holds it (0 when every gain is 0), and that model's count
__global__ void __launch_bounds__(256) verify_argmax_gain_kernel(const int64_t* __restrict__ gains, const int32_t* __restrict__ counts, int H,
                                                                  int32_t* __restrict__ best, int64_t* __restrict__ best_gain,
                                                                  int64_t* __restrict__ best_count) {
    __shared__ int64_t sv[256];
    __shared__ int si[256];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t* g = gains + p * H;
    int64_t v = -1;
    int idx = 0x7fffffff;
    for (int h = tid; h < H; h += 256) {                // ascending h: a later equal gain does not replace an earlier one
        const int64_t x = g[h];
        if (x > v) { v = x; idx = h; }
    }
    sv[tid] = v; si[tid] = idx;
    wg_barrier();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const int64_t ov = sv[tid + s];
            const int oi = si[tid + s];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        wg_barrier();
    }
    if (tid == 0) { best[p] = si[0]; best_gain[p] = sv[0]; best_count[p] = (int64_t)counts[p * H + si[0]]; }
}

// one workgroup per pair: the winner's inlier mask (the rows outside the segments were zeroed before) and the moments
template <class T>
__global__ void __launch_bounds__(EPI_MASK_THREADS)
verify_mask_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const float* __restrict__ conf_,
                   const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                   const float* __restrict__ models, int H, const float* __restrict__ thr, const float* __restrict__ norm, int gate,
                   float min_conf, const int32_t* __restrict__ best, const int64_t* __restrict__ best_count,
                   uint8_t* __restrict__ inlier, double* __restrict__ moments) {
    __shared__ double part[EPI_MASK_WAVES][EPI_MOM];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const float t = thr[p];
    const bool live = t >= 0.0f && best_count[p] > 0;  // otherwise no match is an inlier: the mask stays zero, the moments are zero
    double acc[EPI_MOM];
#pragma unroll
    for (int k = 0; k < EPI_MOM; ++k) acc[k] = 0.0;
    if (live) {                                         // workgroup-uniform
        const float t2 = t * t;
        float e[9];
        verify_model(epi_winner(models, H, best, p), e);
        const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
        const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
        const float* conf = conf_ ? conf_ + lo : nullptr;
        const EpiNorm nm = epi_norm(norm, p);
        for (uint32_t i0 = 0; i0 < n; i0 += EPI_MASK_THREADS) {
            const uint32_t i = i0 + tid;
            float xl0, xl1, xr0, xr1;
            epi_load(ml, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, xl0, xl1, xr0, xr1);
            v2f s, lim, w;
            T::test2(e, t2, pk_splat(xl0), pk_splat(xl1), pk_splat(xr0), pk_splat(xr1), s, lim, w);
            const bool in0 = w.x > 0.0f && s.x <= lim.x;
            if (i < n) inlier[lo + i] = in0 ? 1 : 0;
            if (moments && in0) T::accumulate(xl0, xl1, xr0, xr1, acc);
        }
    }
    if (!moments) return;
    const double s = verify_moments_sum(acc, part, tid, lane, wave);
    if (tid < EPI_MOM) {
        int u, v;
        verify_triangle(tid, u, v);
        double* mo = moments + p * 81;
        mo[u * 9 + v] = s;
        mo[v * 9 + u] = s;
    }
}

}  // namespace pats

using namespace pats;

// the fixed budget of family T; `who` = the entry point's name.  No workspace: the counts are accumulated in the output itself.
// GAIN: the MSAC entries - gains and best_gain are outputs too and the winner is the model with the largest gain; without it the
// two pointers are not looked at
template <class T, bool GAIN>
static int verify_score_by_pair(const char* who, const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models, int64_t H,
                                const float* thr, const float* norm, int use_min_conf, float min_conf, int32_t* counts, int32_t* best,
                                int64_t* best_count, uint8_t* inlier, double* moments, pats_stream_t stream, int64_t* gains,
                                int64_t* best_gain) {
    int rc = epi_check_scored(who, {"matches_l", matches_l, 8}, matches_r, models, thr,
                              {{"counts", counts, 4}, {"best", best, 4}, {"best_count", best_count, 8}, {"inlier", inlier, 1}}, conf, norm, pair_off,
                              stride, counts_in, pairs, cap, H, use_min_conf, min_conf, {"moments", moments, 8});
    if (rc != PATS_OK) return rc;
    const int64_t longest = counts_in ? stride : cap;   // the grid comes from the sizes alone: no host read of the counts
    const int64_t tiles = ceil_div(longest, EPI_TILE), chunks = ceil_div(H, EPI_CHUNK);
    PATS_REQUIRE(tiles * chunks <= 0x7fffffff / pairs, "%s: pairs = %lld gives a grid of %lld x %lld x %lld workgroups (< 2^31)", who,
                 (long long)pairs, (long long)tiles, (long long)pairs, (long long)chunks);
    if (GAIN) {                                         // behind everything the count entries refuse, in their order
        if ((rc = epi_check_args(who, {{"gains", gains, 8}, {"best_gain", best_gain, 8}}, true)) != PATS_OK) return rc;
    }
    hipStream_t st = as_stream(stream);
    rc = fill_bytes(counts, 0, (size_t)pairs * (size_t)H * sizeof(int32_t), st);
    if (rc != PATS_OK) return rc;
    if (GAIN) {
        rc = fill_bytes(gains, 0, (size_t)pairs * (size_t)H * sizeof(int64_t), st);
        if (rc != PATS_OK) return rc;
    }
    rc = fill_bytes(inlier, 0, (size_t)cap, st);
    if (rc != PATS_OK) return rc;
    const float* cf = use_min_conf ? conf : nullptr;    // without a threshold the confidence is not read
    if (tiles > 0) {
        hipLaunchKernelGGL((verify_score_kernel<T, false, GAIN>), dim3((unsigned)(tiles * pairs * chunks)), dim3(EPI_THREADS), 0, st,
                           matches_l, matches_r, cf, pair_off, counts_in, stride, cap, (int)pairs, (int)chunks, models, (int)H, thr, norm,
                           use_min_conf, min_conf, counts, 0, (int)H, nullptr, GAIN ? gains : nullptr);
        rc = check_launch(GAIN ? T::SCORE_MSAC : T::SCORE);
        if (rc != PATS_OK) return rc;
    }
    if (GAIN)
        hipLaunchKernelGGL(verify_argmax_gain_kernel, dim3((unsigned)pairs), dim3(256), 0, st, gains, counts, (int)H, best, best_gain,
                           best_count);
    else
        hipLaunchKernelGGL(verify_argmax_kernel<ARGMAX_THREADS>, dim3((unsigned)pairs), dim3(ARGMAX_THREADS), 0, st, counts, (int)H, best,
                           best_count);
    rc = check_launch(T::ARGMAX);
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(verify_mask_kernel<T>, dim3((unsigned)pairs), dim3(EPI_MASK_THREADS), 0, st, matches_l, matches_r, cf, pair_off,
                       counts_in, stride, cap, models, (int)H, thr, norm, use_min_conf, min_conf, best, best_count, inlier, moments);
    return check_launch(T::MASK);
}

// the two launchers of family T for adaptive.hip's host side
template <class T>
static int verify_adaptive_round(const AdaptiveCall& c, const float* conf, int tiles, int h_lo, int h_hi, const int32_t* stopped,
                                 hipStream_t st) {
    const int64_t chunks = ceil_div(h_hi - h_lo, EPI_CHUNK);
    hipLaunchKernelGGL((verify_score_kernel<T, true, false>), dim3((unsigned)(tiles * c.pairs * chunks)), dim3(EPI_THREADS), 0, st,
                       c.matches_l, c.matches_r, conf, c.pair_off, c.counts_in, c.stride, c.cap, (int)c.pairs, (int)chunks, c.models,
                       (int)c.H, c.thr, c.norm, c.use_min_conf, c.min_conf, c.counts, h_lo, h_hi, stopped, nullptr);
    return check_launch(T::ROUND);
}

template <class T>
static int verify_adaptive_mask(const AdaptiveCall& c, const float* conf, hipStream_t st) {
    hipLaunchKernelGGL(verify_mask_kernel<T>, dim3((unsigned)c.pairs), dim3(EPI_MASK_THREADS), 0, st, c.matches_l, c.matches_r, conf,
                       c.pair_off, c.counts_in, c.stride, c.cap, c.models, (int)c.H, c.thr, c.norm, c.use_min_conf, c.min_conf, c.best,
                       c.best_count, c.inlier, c.moments);
    return check_launch(T::MASK);
}

// ---- the entry points (include/pats_amd.h) ---------------------------------------------------------------------------------------
extern "C" int64_t pats_epipolar_max_h(void) { return EPI_MAX_H; }

// the fixed budget needs no workspace (the counts are accumulated in the output itself), the adaptive one the stopped flags
extern "C" size_t pats_epipolar_workspace_bytes(int64_t, int64_t, int64_t) { return 0; }
extern "C" size_t pats_homography_score_workspace_bytes(int64_t, int64_t, int64_t) { return 0; }
extern "C" size_t pats_epipolar_score_adaptive_workspace_bytes(int64_t pairs, int64_t, int64_t) { return adaptive_workspace_bytes(pairs); }
extern "C" size_t pats_homography_score_adaptive_workspace_bytes(int64_t pairs, int64_t, int64_t) { return adaptive_workspace_bytes(pairs); }

extern "C" int pats_epipolar_score_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                               int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                               int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                               int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                               void*, size_t, pats_stream_t stream) {
    return verify_score_by_pair<Epipolar, false>("epipolar_score_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in, pairs,
                                                 cap, models, H, thr, norm, use_min_conf, min_conf, counts, best, best_count, inlier, moments,
                                                 stream, nullptr, nullptr);
}

extern "C" int pats_homography_score_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                 int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                                 int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                                 int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                                 void*, size_t, pats_stream_t stream) {
    return verify_score_by_pair<Homography, false>("homography_score_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in, pairs,
                                                   cap, models, H, thr, norm, use_min_conf, min_conf, counts, best, best_count, inlier,
                                                   moments, stream, nullptr, nullptr);
}

// the MSAC entries: the count entries' arguments through stream, then gains and best_gain
extern "C" int64_t pats_msac_gain_one(void) { return (int64_t)1 << MSAC_GAIN_BITS; }

extern "C" int pats_epipolar_score_msac_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                    int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                                    int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                                    int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                                    void*, size_t, pats_stream_t stream, int64_t* gains, int64_t* best_gain) {
    return verify_score_by_pair<Epipolar, true>("epipolar_score_msac_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in, pairs,
                                                cap, models, H, thr, norm, use_min_conf, min_conf, counts, best, best_count, inlier, moments,
                                                stream, gains, best_gain);
}

extern "C" int pats_homography_score_msac_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                      int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                                      int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                                      int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                                      void*, size_t, pats_stream_t stream, int64_t* gains, int64_t* best_gain) {
    return verify_score_by_pair<Homography, true>("homography_score_msac_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in,
                                                  pairs, cap, models, H, thr, norm, use_min_conf, min_conf, counts, best, best_count, inlier,
                                                  moments, stream, gains, best_gain);
}

extern "C" int pats_epipolar_score_adaptive_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf,
        const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models, int64_t H,
        const float* thr, const float* norm, int use_min_conf, float min_conf, int32_t* counts, int32_t* best, int64_t* best_count,
        uint8_t* inlier, double* moments, void* workspace, size_t workspace_bytes, pats_stream_t stream, double confidence,
        int sample_size, int models_per_sample, int64_t round_models, int32_t* used, int32_t* participating) {
    const AdaptiveCall c{matches_l, matches_r, conf, pair_off, stride, counts_in, pairs, cap, models, H, thr, norm, use_min_conf, min_conf,
                         counts, best, best_count, inlier, moments, workspace, workspace_bytes, stream, confidence, sample_size,
                         models_per_sample, round_models, used, participating};
    return adaptive_score_by_pair("epipolar_score_adaptive_by_pair", c, verify_adaptive_round<Epipolar>, verify_adaptive_mask<Epipolar>);
}

extern "C" int pats_homography_score_adaptive_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf,
        const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models, int64_t H,
        const float* thr, const float* norm, int use_min_conf, float min_conf, int32_t* counts, int32_t* best, int64_t* best_count,
        uint8_t* inlier, double* moments, void* workspace, size_t workspace_bytes, pats_stream_t stream, double confidence,
        int sample_size, int models_per_sample, int64_t round_models, int32_t* used, int32_t* participating) {
    const AdaptiveCall c{matches_l, matches_r, conf, pair_off, stride, counts_in, pairs, cap, models, H, thr, norm, use_min_conf, min_conf,
                         counts, best, best_count, inlier, moments, workspace, workspace_bytes, stream, confidence, sample_size,
                         models_per_sample, round_models, used, participating};
    return adaptive_score_by_pair("homography_score_adaptive_by_pair", c, verify_adaptive_round<Homography>, verify_adaptive_mask<Homography>);
}
