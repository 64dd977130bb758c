// Per-pair match error against depth-and-pose ground truth: a lifted left match is carried through the ground-truth relative pose
// into the right image and the distance of the matched right point from that projection is measured, in pixels - the reprojection
// form of the check the reference's Compute_depth_label (datasets/megadepth.py) and Compute_label (utils/utils.py) make - with the
// covisibility test against the right depth map, the per-pair tallies, the precision at each threshold, a confidence sweep and the
// confusion against a mask.  ONE launch for the batch behind two fills, no host read, no workspace.  include/pats_amd.h states the
// definition ("Per-pair match error against ground truth"); docs/kernels.md 4.23 the design.
//
// One workgroup of MERR_THREADS per pair walks its segment; nothing crosses workgroups.  merr_one is the whole definition of one
// match (float64, no contraction).
//   walk    thread j takes matches j, j + MERR_THREADS, ... in that order: err and status are stored for every row of the segment;
//           the 19 integer tallies (7 status values, 8 thresholds, 4 confusion cells) and the float64 error sum stay in registers;
//           a scored match with a confidence at or above the lowest edge adds one to its bin's row of the LDS histogram
//           (bins x (1 + n_thr) uint32, integer LDS atomics: the order of arrival does not show)
//   reduce  the integer tallies over the wave by wave_sum_u32 (lane_reduce.hpp), the waves added by the thread that stores the
//           tally; the error sum by the FIXED tree the header states - wave_sum_tree_f64 (epipolar.hpp) is its xor tree as lane 0
//           sees it, and only lane 0's value is used -, the waves in index order
//   sweep   bins into ">= edge" counts: a suffix sum per column, one thread each
#include "common.hpp"
#include "epipolar.hpp"
#include "gt_pose.hpp"
#include "lane_reduce.hpp"

namespace pats {

constexpr int MERR_THREADS = 256;
constexpr int MERR_WAVES = MERR_THREADS / WAVE;
constexpr int MERR_MAX_THR = 8;
constexpr int MERR_MAX_BINS = 64;
constexpr int MERR_COLS = 1 + MERR_MAX_THR;             // a histogram row: the scored, then those within each threshold
constexpr int MERR_TALLY = 8;                           // slots of tally[p]: the status values 0 .. 6, slot 7 zero
constexpr int MERR_COUNTERS = MERR_TALLY + MERR_MAX_THR + 4;

struct MerrArgs {
    const float* points; const float* mr; const float* conf; const uint8_t* mask;
    const int64_t* pair_off; const int64_t* counts_in; int64_t stride, cap;
    const float* norm; const double* T1; const double* T0; const int64_t* depth_r; const float* size_r;
    double occl_rel;
    int swapped, gate, n_thr, B;
    float min_conf;
    double thr[MERR_MAX_THR];
    float edges[MERR_MAX_BINS];
    double* err; uint8_t* status; int64_t* tally; int64_t* correct; double* err_sum; int64_t* sweep; int64_t* confusion;
};

// what a pair's matches share: the ground truth in the frame of the points, the right half of the normalisation, the right
// image's content and its depth map
struct MerrPair {
    double R[9], t[3];
    double c0, c1, s0, s1;
    double h1, w1;                                      // size_r - 1
    const float* map; int64_t mh, mw, mld;
    double occl_rel;
    bool has_norm, has_size, has_map;
};

// THE definition of one match that takes part (include/pats_amd.h): X the lifted point, (p0, p1) the stored right point -> status, err
__device__ __forceinline__ int merr_one(const MerrPair& g, float X0f, float X1f, float X2f, float p0f, float p1f, double& err) {
    err = __builtin_nan("");
    if (!(__builtin_isfinite(X0f) && __builtin_isfinite(X1f) && __builtin_isfinite(X2f))) return 2;
    const double X0 = (double)X0f, X1 = (double)X1f, X2 = (double)X2f;
    const double Y0 = ((g.R[0] * X0 + g.R[1] * X1) + g.R[2] * X2) + g.t[0];
    const double Y1 = ((g.R[3] * X0 + g.R[4] * X1) + g.R[5] * X2) + g.t[1];
    const double Y2 = ((g.R[6] * X0 + g.R[7] * X1) + g.R[8] * X2) + g.t[2];
    if (!(__builtin_isfinite(Y0) && __builtin_isfinite(Y1) && __builtin_isfinite(Y2)) || Y2 <= 0.0) return 3;
    double q0 = Y0 / Y2, q1 = Y1 / Y2;
    if (g.has_norm) { q0 = q0 / g.s0 + g.c0; q1 = q1 / g.s1 + g.c1; }
    if (g.has_size && !(q0 >= 0.0 && q0 <= g.h1 && q1 >= 0.0 && q1 <= g.w1)) return 4;
    if (g.has_map) {
        const double fi = __builtin_rint(q0), fj = __builtin_rint(q1);           // round half to even
        if (!(fi >= 0.0 && fi < (double)g.mh && fj >= 0.0 && fj < (double)g.mw)) return 5;   // false for a NaN: the tap is inside the map below
        const float tap = g.map[(int64_t)fi * g.mld + (int64_t)fj];
        if (!(__builtin_isfinite(tap) && tap > 0.0f)) return 5;
        const double d1 = (double)tap;
        if (__builtin_fabs(Y2 - d1) > g.occl_rel * d1) return 6;
    }
    const double e0 = q0 - (double)p0f, e1 = q1 - (double)p1f;
    err = __builtin_sqrt(e0 * e0 + e1 * e1);
    return 1;
}

// the number of edges <= c (0 for a NaN c): the match counts for the bins 0 .. that number - 1.  edges ascend strictly
__device__ __forceinline__ int merr_bins_at_or_below(const float* __restrict__ edges, int B, float c) {
    int lo = 0, hi = B;                                 // edges[0 .. lo) <= c, not edges[hi .. B) <= c
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(MERR_THREADS) match_error_kernel(MerrArgs a) {
    __shared__ uint32_t s_hist[MERR_MAX_BINS * MERR_COLS];
    __shared__ float s_edges[MERR_MAX_BINS];
    __shared__ uint32_t s_cnt[MERR_WAVES][MERR_COUNTERS];
    __shared__ double s_sum[MERR_WAVES];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_thr = a.n_thr, B = a.B;
    int64_t lo;
    uint32_t n;
    epi_segment(a.pair_off, a.counts_in, a.stride, a.cap, p, lo, n);

    // ---- the pair ---------------------------------------------------------------------------------------------------------------
    MerrPair g;
    {
        double G[9], t[3];
        (void)gt_relative_pose(a.T1, a.T0, p, G, t);    // a ground truth that is not finite gives a Y that is not: status 3
#pragma unroll
        for (int k = 0; k < 9; ++k) g.R[k] = a.swapped ? G[hom_perm(k, 1)] : G[k];            // P R_gt P, P t_gt
#pragma unroll
        for (int i = 0; i < 3; ++i) g.t[i] = a.swapped ? t[frame_perm(i, 1)] : t[i];
    }
    g.has_norm = a.norm != nullptr;
    g.c0 = g.c1 = 0.0; g.s0 = g.s1 = 1.0;
    if (g.has_norm) {
        const float* q = a.norm + p * 8 + 4;            // the RIGHT half
        g.c0 = (double)q[0]; g.c1 = (double)q[1]; g.s0 = (double)q[2]; g.s1 = (double)q[3];
    }
    g.has_size = a.size_r != nullptr;
    g.h1 = g.w1 = 0.0;
    if (g.has_size) { g.h1 = (double)a.size_r[p * 2] - 1.0; g.w1 = (double)a.size_r[p * 2 + 1] - 1.0; }
    g.map = nullptr; g.mh = g.mw = g.mld = 0;
    if (a.depth_r != nullptr) {
        const int64_t* row = a.depth_r + p * 4;
        g.map = reinterpret_cast<const float*>((uintptr_t)row[0]); g.mh = row[1]; g.mw = row[2]; g.mld = row[3];
    }
    g.has_map = g.map != nullptr && g.mh >= 1 && g.mw >= 1;                     // workgroup-uniform
    g.occl_rel = a.occl_rel;

    const bool sweep = a.sweep != nullptr;
    if (sweep) {
        for (int c = tid; c < B * MERR_COLS; c += MERR_THREADS) s_hist[c] = 0u;
        for (int b = tid; b < B; b += MERR_THREADS) s_edges[b] = a.edges[b];
        wg_barrier();
    }

    // ---- walk -------------------------------------------------------------------------------------------------------------------
    const float* X_ = a.points + lo * 3;
    const float2* mr = reinterpret_cast<const float2*>(a.mr) + lo;
    const float* conf = a.conf ? a.conf + lo : nullptr;
    const uint8_t* mask = a.mask ? a.mask + lo : nullptr;
    double* err_out = a.err + lo;
    uint8_t* st_out = a.status + lo;
    uint32_t cnt[MERR_COUNTERS];
#pragma unroll
    for (int k = 0; k < MERR_COUNTERS; ++k) cnt[k] = 0u;
    double sum = 0.0;
    for (uint32_t i = tid; i < n; i += MERR_THREADS) {
        const float2 pr = mr[i];
        const float x0 = X_[(int64_t)i * 3], x1 = X_[(int64_t)i * 3 + 1], x2 = X_[(int64_t)i * 3 + 2];
        const float cf = conf ? conf[i] : 0.0f;
        const bool in_mask = mask ? mask[i] != 0 : false;
        bool part = __builtin_isfinite(pr.x) && __builtin_isfinite(pr.y);
        if (a.gate) part = part && cf >= a.min_conf;    // false for a NaN confidence
        double e = __builtin_nan("");
        const int st = part ? merr_one(g, x0, x1, x2, pr.x, pr.y, e) : 0;
        err_out[i] = e;
        st_out[i] = (uint8_t)st;
#pragma unroll
        for (int s = 0; s < 7; ++s) cnt[s] += st == s ? 1u : 0u;
        if (st == 1) {
            sum += e;
            uint32_t within = 0u;                       // bit k: err <= thr[k]
#pragma unroll
            for (int k = 0; k < MERR_MAX_THR; ++k) {
                const bool ok = k < n_thr && e <= a.thr[k];
                cnt[MERR_TALLY + k] += ok ? 1u : 0u;
                within |= ok ? 1u << k : 0u;
            }
            if (mask) {
                const bool good = (within & 1u) != 0u;
                cnt[MERR_TALLY + MERR_MAX_THR + 0] += in_mask && good ? 1u : 0u;
                cnt[MERR_TALLY + MERR_MAX_THR + 1] += in_mask && !good ? 1u : 0u;
                cnt[MERR_TALLY + MERR_MAX_THR + 2] += !in_mask && good ? 1u : 0u;
                cnt[MERR_TALLY + MERR_MAX_THR + 3] += !in_mask && !good ? 1u : 0u;
            }
            if (sweep) {
                const int j = merr_bins_at_or_below(s_edges, B, cf);
                if (j > 0) {                            // j - 1 < B: inside the histogram
                    uint32_t* row = s_hist + (j - 1) * MERR_COLS;
                    atomicAdd(row, 1u);
#pragma unroll
                    for (int k = 0; k < MERR_MAX_THR; ++k)
                        if (within & (1u << k)) atomicAdd(row + 1 + k, 1u);
                }
            }
        }
    }

    // ---- reduce -----------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < MERR_COUNTERS; ++k) cnt[k] = wave_sum_u32(cnt[k], lane);      // every counter < 2^31 for the pair: n < 2^31
    wave_parts_store(s_cnt, wave, lane, cnt);
    wave_parts_store(s_sum, wave, lane, wave_sum_tree_f64(sum));
    wg_barrier();
    if (tid < MERR_COUNTERS) {
        const int64_t total = (int64_t)wave_parts_total(s_cnt, tid);
        if (tid < MERR_TALLY) a.tally[p * MERR_TALLY + tid] = total;             // slot 7 was never counted: zero
        else if (tid < MERR_TALLY + MERR_MAX_THR) { if (tid - MERR_TALLY < n_thr) a.correct[p * n_thr + (tid - MERR_TALLY)] = total; }
        else if (a.confusion != nullptr) a.confusion[p * 4 + (tid - MERR_TALLY - MERR_MAX_THR)] = total;
    }
    if (tid == 0) a.err_sum[p] = wave_parts_total(s_sum);

    // ---- sweep: bin b of column c counts conf in [edges[b], edges[b + 1]); the suffix sum counts conf >= edges[b] -----------------
    if (sweep && tid <= n_thr) {                        // the histogram is complete: the barrier above follows the walk
        int64_t run = 0;
        int64_t* col = a.sweep + p * B * (1 + n_thr) + tid;
        for (int b = B - 1; b >= 0; --b) {
            run += (int64_t)s_hist[b * MERR_COLS + tid];
            col[(int64_t)b * (1 + n_thr)] = run;
        }
    }
}

}  // namespace pats

using namespace pats;

extern "C" int pats_match_error_by_pair_f64(const float* points, const float* matches_r, const float* conf, const int64_t* pair_off,
                                            int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* norm,
                                            const double* T1, const double* T0, int swapped, const int64_t* depth_r_table, double occl_rel,
                                            const float* size_r, int use_min_conf, float min_conf, const double* thr, int64_t n_thr,
                                            const float* edges, int64_t B, const uint8_t* mask, double* err, uint8_t* status, int64_t* tally,
                                            int64_t* correct, double* err_sum, int64_t* sweep, int64_t* confusion, pats_stream_t stream) {
    const char* who = "match_error_by_pair";
    int rc = epi_check_args(who, {{"points", points, 4}, {"matches_r", matches_r, 8}, {"T1", T1, 8}, {"err", err, 8}, {"status", status, 1},
                                  {"tally", tally, 8}, {"correct", correct, 8}, {"err_sum", err_sum, 8}}, true);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(thr, "%s: null thr", who);
    rc = epi_check_args(who, {{"conf", conf, 4}, {"norm", norm, 4}, {"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}, {"T0", T0, 8},
                              {"depth_r_table", depth_r_table, 8}, {"size_r", size_r, 4}, {"mask", mask, 1}, {"sweep", sweep, 8},
                              {"confusion", confusion, 8}}, false);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    PATS_REQUIRE(!use_min_conf || conf, "%s: min_conf needs conf", who);
    PATS_REQUIRE(!use_min_conf || min_conf >= 0.0f, "%s: min_conf = %g must be a non-negative number", who, (double)min_conf);
    PATS_REQUIRE(swapped == 0 || swapped == 1, "%s: swapped = %d must be 0 or 1", who, swapped);
    PATS_REQUIRE(!depth_r_table || (occl_rel > 0.0 && occl_rel <= 1.7976931348623157e308),
                 "%s: occl_rel = %g must be finite and positive", who, occl_rel);
    PATS_REQUIRE(n_thr >= 1 && n_thr <= MERR_MAX_THR, "%s: n_thr = %lld (1 .. %d)", who, (long long)n_thr, MERR_MAX_THR);
    MerrArgs a{};
    for (int64_t k = 0; k < n_thr; ++k) {
        const double v = thr[k];
        PATS_REQUIRE(v > 0.0 && v <= 1.7976931348623157e308, "%s: thr[%lld] = %g must be finite and positive", who, (long long)k, v);
        PATS_REQUIRE(k == 0 || v > thr[k - 1], "%s: thr[%lld] = %g does not ascend strictly", who, (long long)k, v);
        a.thr[k] = v;
    }
    PATS_REQUIRE((edges != nullptr) == (sweep != nullptr), "%s: edges and sweep go together", who);
    PATS_REQUIRE((mask != nullptr) == (confusion != nullptr), "%s: mask and confusion go together", who);
    if (edges) {
        PATS_REQUIRE(conf, "%s: edges need conf", who);
        PATS_REQUIRE(B >= 1 && B <= MERR_MAX_BINS, "%s: B = %lld (1 .. %d)", who, (long long)B, MERR_MAX_BINS);
        for (int64_t b = 0; b < B; ++b) {
            const float v = edges[b];
            PATS_REQUIRE(v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f, "%s: edges[%lld] = %g must be finite", who, (long long)b,
                         (double)v);
            PATS_REQUIRE(b == 0 || v > edges[b - 1], "%s: edges[%lld] = %g does not ascend strictly", who, (long long)b, (double)v);
            a.edges[b] = v;
        }
    } else {
        B = 0;
    }
    a.points = points; a.mr = matches_r; a.conf = (use_min_conf || edges) ? conf : nullptr; a.mask = mask;
    a.pair_off = pair_off; a.counts_in = counts_in; a.stride = stride; a.cap = cap;
    a.norm = norm; a.T1 = T1; a.T0 = T0; a.depth_r = depth_r_table; a.size_r = size_r;
    a.occl_rel = occl_rel;
    a.swapped = swapped; a.gate = use_min_conf ? 1 : 0; a.n_thr = (int)n_thr; a.B = (int)B;
    a.min_conf = min_conf;
    a.err = err; a.status = status; a.tally = tally; a.correct = correct; a.err_sum = err_sum; a.sweep = sweep; a.confusion = confusion;
    hipStream_t st = as_stream(stream);
    // every byte of both per-match outputs is defined: zeros here, the kernel stores every row of every segment
    if ((rc = fill_bytes(err, 0, (size_t)cap * sizeof(double), st)) != PATS_OK) return rc;
    if ((rc = fill_bytes(status, 0, (size_t)cap, st)) != PATS_OK) return rc;
    hipLaunchKernelGGL(match_error_kernel, dim3((unsigned)pairs), dim3(MERR_THREADS), 0, st, a);
    return check_launch("match_error kernel");
}
