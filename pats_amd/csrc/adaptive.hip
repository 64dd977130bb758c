// Per-pair adaptive verification - what the epipolar and the homography branch share: the stopping rule, the per-pair update kernel
// that applies it after every round of models, and the host side that checks the arguments and issues the rounds.  The score and
// the mask kernels are epipolar.hip's (the fixed-budget kernels of the branch's family, restricted to a round's models); they reach
// this file as two launchers.  include/pats_amd.h states the definition ("Per-pair adaptive verification");
// docs/kernels.md 4.12 the design.
//
//   update  one workgroup per pair after round r, 256 threads: the argmax of counts[p, r B .. T_r) (the lowest index among equals)
//           merged into the running best (best / best_count: a later equal count never replaces it), then the rule on one thread
//           in float64 - w = c / participating, q = 1 - w^s, miss = q^k by square-and-multiply, the pair stops iff
//           miss <= 1 - confidence - and used / stopped.  Round 0's update also counts the matches that participate (epi_load's
//           rule, the one the score kernels apply).  A pair that has stopped returns at once.
// Nothing here waits for another workgroup: the order of the rounds is the stream's.
#include "common.hpp"
#include "epipolar.hpp"

namespace pats {

constexpr int ADP_THREADS = 256;
constexpr int ADP_MAX_ROUNDS = 256;
constexpr int ADP_MAX_SAMPLE = 16;                     // sample_size and models_per_sample: 1 .. 16

// THE rule: IEEE float64, multiplications and one subtraction in the order the header states (-ffp-contract=off: never fused)
__device__ __forceinline__ bool adaptive_stops(int c, int participating, int s, int k, double eta) {
    const double w = participating > 0 ? (double)c / (double)participating : 0.0;
    double ws = w;
    for (int i = 1; i < s; ++i) ws = ws * w;
    const double q = 1.0 - ws;
    double miss = 1.0;
    for (int b = k > 0 ? 31 - __builtin_clz((unsigned)k) : -1; b >= 0; --b) {     // from k's most significant bit
        miss = miss * miss;
        if ((k >> b) & 1) miss = miss * q;
    }
    return miss <= eta;
}

__global__ void __launch_bounds__(ADP_THREADS)
adaptive_update_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const float* __restrict__ conf_,
                       const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                       const float* __restrict__ thr, const float* __restrict__ norm, int gate, float min_conf,
                       const int32_t* __restrict__ counts, int H, int h_lo, int h_hi, double eta, int sample_size, int models_per_sample,
                       int32_t* __restrict__ best, int64_t* __restrict__ best_count, int32_t* __restrict__ used,
                       int32_t* __restrict__ participating, int32_t* __restrict__ stopped) {
    __shared__ int sv[ADP_THREADS], si[ADP_THREADS];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const bool first = h_lo == 0;
    if (!first && stopped[p]) return;                   // workgroup-uniform
    int part = 0;
    if (first) {                                        // the matches that take part: the score kernels' rule
        int64_t lo;
        uint32_t n;
        epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
        if (thr[p] >= 0.0f) {                           // workgroup-uniform; NaN or negative: no match takes part
            const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
            const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
            const float* conf = conf_ ? conf_ + lo : nullptr;
            const EpiNorm nm = epi_norm(norm, p);
            for (uint32_t i = tid; i < n; i += ADP_THREADS) {
                float l0, l1, r0, r1;
                epi_load(ml, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, l0, l1, r0, r1);
                part += l0 == l0 ? 1 : 0;
            }
        }
        sv[tid] = part;
        wg_barrier();
        for (int s = ADP_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) sv[tid] += sv[tid + s];
            wg_barrier();
        }
        part = sv[0];
        wg_barrier();                                   // sv is free for the argmax
    }
    const int32_t* c = counts + p * H;
    int v = -1, idx = 0x7fffffff;
    for (int h = h_lo + tid; h < h_hi; h += ADP_THREADS) {     // ascending h: a later equal count does not replace an earlier one
        const int x = c[h];
        if (x > v) { v = x; idx = h; }
    }
    sv[tid] = v; si[tid] = idx;
    wg_barrier();
    for (int s = ADP_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int ov = sv[tid + s], oi = si[tid + s];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        wg_barrier();
    }
    if (tid != 0) return;
    int bc = sv[0], bi = si[0];                         // h_lo < h_hi: the round holds a model
    if (first) {
        participating[p] = part;
    } else {
        part = participating[p];
        const int rc = (int)best_count[p];
        if (!(bc > rc)) { bc = rc; bi = best[p]; }      // the running best stays on an equal count
    }
    best[p] = bi;
    best_count[p] = (int64_t)bc;
    const bool stop = adaptive_stops(bc, part, sample_size, h_hi / models_per_sample, eta);
    if (first || stop) used[p] = stop ? h_hi : H;
    stopped[p] = stop ? 1 : 0;
}

}  // namespace pats

using namespace pats;

size_t pats::adaptive_workspace_bytes(int64_t pairs) {
    return pairs > 0 ? (size_t)pairs * sizeof(int32_t) : 0;     // the stopped flag of every pair
}

int pats::adaptive_score_by_pair(const char* who, const AdaptiveCall& c, AdaptiveScoreRound score_round, AdaptiveMask mask) {
    int rc = epi_check_scored(who, {"matches_l", c.matches_l, 8}, c.matches_r, c.models, c.thr,
                              {{"counts", c.counts, 4}, {"best", c.best, 4}, {"best_count", c.best_count, 8}, {"inlier", c.inlier, 1},
                               {"used", c.used, 4}, {"participating", c.participating, 4}},
                              c.conf, c.norm, c.pair_off, c.stride, c.counts_in, c.pairs, c.cap, c.H, c.use_min_conf, c.min_conf,
                              {"moments", c.moments, 8});
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(c.confidence > 0.0 && c.confidence < 1.0, "%s: confidence = %g must lie strictly between 0 and 1", who, c.confidence);
    PATS_REQUIRE(c.sample_size >= 1 && c.sample_size <= ADP_MAX_SAMPLE, "%s: sample_size = %d (1 .. %d)", who, c.sample_size, ADP_MAX_SAMPLE);
    PATS_REQUIRE(c.models_per_sample >= 1 && c.models_per_sample <= ADP_MAX_SAMPLE, "%s: models_per_sample = %d (1 .. %d)", who,
                 c.models_per_sample, ADP_MAX_SAMPLE);
    PATS_REQUIRE(c.round_models >= 64 && c.round_models % 64 == 0, "%s: round_models = %lld must be a positive multiple of 64", who,
                 (long long)c.round_models);
    const int64_t rounds = ceil_div(c.H, c.round_models);
    PATS_REQUIRE(rounds <= ADP_MAX_ROUNDS, "%s: round_models = %lld gives %lld rounds for H = %lld (at most %d)", who,
                 (long long)c.round_models, (long long)rounds, (long long)c.H, ADP_MAX_ROUNDS);
    const size_t need = adaptive_workspace_bytes(c.pairs);
    PATS_REQUIRE(c.workspace_bytes >= need, "%s: workspace too small", who);
    if ((rc = epi_check_args(who, {{"workspace", c.workspace, 4}}, true)) != PATS_OK) return rc;
    const int64_t longest = c.counts_in ? c.stride : c.cap;    // the grid comes from the sizes alone: no host read of the counts
    const int64_t span = c.round_models < c.H ? c.round_models : c.H;
    const int64_t tiles = ceil_div(longest, ADAPTIVE_TILE), chunks = ceil_div(span, ADAPTIVE_CHUNK);
    PATS_REQUIRE(tiles * chunks <= 0x7fffffff / c.pairs, "%s: pairs = %lld gives a grid of %lld x %lld x %lld workgroups (< 2^31)", who,
                 (long long)c.pairs, (long long)tiles, (long long)c.pairs, (long long)chunks);
    hipStream_t st = as_stream(c.stream);
    int32_t* stopped = static_cast<int32_t*>(c.workspace);
    rc = fill_bytes(c.counts, 0, (size_t)c.pairs * (size_t)c.H * sizeof(int32_t), st);
    if (rc != PATS_OK) return rc;
    rc = fill_bytes(c.inlier, 0, (size_t)c.cap, st);
    if (rc != PATS_OK) return rc;
    rc = fill_bytes(stopped, 0, need, st);
    if (rc != PATS_OK) return rc;
    const float* cf = c.use_min_conf ? c.conf : nullptr;       // without a threshold the confidence is not read
    const double eta = 1.0 - c.confidence;
    for (int64_t r = 0; r < rounds; ++r) {              // rounds after every pair has stopped still launch: their workgroups return
        const int h_lo = (int)(r * c.round_models);
        const int h_hi = (int)((r + 1) * c.round_models < c.H ? (r + 1) * c.round_models : c.H);
        if (tiles > 0) {
            rc = score_round(c, cf, (int)tiles, h_lo, h_hi, stopped, st);
            if (rc != PATS_OK) return rc;
        }
        hipLaunchKernelGGL(adaptive_update_kernel, dim3((unsigned)c.pairs), dim3(ADP_THREADS), 0, st, c.matches_l, c.matches_r, cf,
                           c.pair_off, c.counts_in, c.stride, c.cap, c.thr, c.norm, c.use_min_conf, c.min_conf, c.counts, (int)c.H, h_lo,
                           h_hi, eta, c.sample_size, c.models_per_sample, c.best, c.best_count, c.used, c.participating, stopped);
        rc = check_launch("adaptive_update kernel");
        if (rc != PATS_OK) return rc;
    }
    return mask(c, cf, st);
}
