// Segmented top-K of the throughput path's hand-over: for every pair of a regrouped batch (pats_matches_by_*pair_summary_conf_f32:
// matches_l / matches_r / conf with pair p in rows pair_off[p] .. pair_off[p + 1]) its K most confident matches, exact and
// deterministic, in ONE launch and without a host read.  include/pats_amd.h states the definition; docs/kernels.md 4.6 the design.
//
// One workgroup of 1024 threads per pair; nothing crosses workgroups (no global atomics, no spinning), every loop is bounded by the
// segment length n.  With key = the order-preserving uint32 image of the float:
//   select   (n > TOPK_WHOLE and more than K eligible) MSB-first radix select, four 8-bit passes over the segment, each a 256-bin LDS
//            histogram of the keys that agree with the digits found so far: T = the K-th largest eligible key, r = how many of the
//            keys equal to T are wanted.  Otherwise (a short segment, or at most K are eligible) everything eligible
//            is taken: T = the threshold's key, r = unbounded
//   compact  one pass in index order: key > T, and the FIRST r with key == T (ballot + ordered prefix over the waves: ties go to the
//            lower index), as 64-bit composites key << 32 | (0xFFFFFFFF - i) into LDS
//   sort     bitonic, descending, on the next power of two (the composites are unique: any network gives the same answer)
//   write    rows 0 .. count - 1 gathered through the sorted indices, the tail filled (-1 / 0.0): every output byte is defined
#include "common.hpp"
#include "lane_reduce.hpp"
#include "topk_shared.hpp"

namespace pats {

constexpr int TOPK_SORT_CAP = 8192;             // composites the sort buffer holds = pats_topk_by_pair_max_k(): 64 KB of LDS
constexpr int TOPK_WHOLE = 4096;                // segments up to this length are sorted whole (no select): 78 sort steps at most
constexpr uint32_t TOPK_ALL = 0x7fffffffu;      // r = "every key equal to T" (a segment holds fewer rows than this)

struct TopkArgs {
    const float* ml; const float* mr; const float* conf; const int64_t* pair_off;
    int64_t cap; int K; uint32_t thr;           // thr = key(min_conf), 0 without a threshold: every key is >= 0
    float* top_l; float* top_r; float* top_conf; int32_t* top_idx; int64_t* top_count;
};

// one radix pass: hist[d] = number of eligible keys of the segment that agree with `prefix` above `shift + 8` and have digit d at
// `shift`.  Confidences cluster (most of a pair's share the exponent byte), so a wave whose active lanes all hold one digit adds
// its population once; mixed waves use one LDS atomic per lane (integer adds: the order does not matter).
__device__ __forceinline__ void topk_histogram(const uint32_t* __restrict__ bits, uint32_t n, uint32_t thr, uint32_t prefix, int shift,
                                               uint32_t* hist) {
    const uint32_t himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
    for (uint32_t i0 = 0; i0 < n; i0 += TOPK_THREADS) {
        const uint32_t i = i0 + threadIdx.x;
        bool in = false;
        uint32_t d = 0;
        if (i < n) {
            const uint32_t k = topk_key(bits[i]);
            in = k >= thr && ((k ^ prefix) & himask) == 0u;
            d = (k >> shift) & 255u;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(in);
        if (m == 0ull) continue;
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, __builtin_ctzll(m));
        if (__builtin_amdgcn_ballot_w64(in && d == d0) == m) {
            if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(&hist[d0], (uint32_t)__builtin_popcountll(m));
        } else if (in) {
            atomicAdd(&hist[d], 1u);
        }
    }
}

__global__ void __launch_bounds__(TOPK_THREADS) topk_by_pair_kernel(TopkArgs g) {
    __shared__ unsigned long long buf[TOPK_SORT_CAP];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wave_cnt[2][TOPK_WAVES][2];           // per tile (double-buffered), per wave: keys > T, keys == T
    __shared__ uint32_t sel[3];                               // the select's hand-over: digit, keys above it, eligible keys in all
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t K = (uint32_t)g.K;
    PATS_TOPK_SEGMENT(g.pair_off, p, g.cap);                  // lo, n: the pair's rows, inside the arrays whatever pair_off holds
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(g.conf) + lo;

    // ---- select: T and r ---------------------------------------------------------------------------------------------------
    uint32_t T = g.thr, r = TOPK_ALL;
    if (n > (uint32_t)TOPK_WHOLE) {                           // workgroup-uniform
        uint32_t prefix = 0, want = K;
        bool all = false;
        for (int shift = 24; shift >= 0 && !all; shift -= 8) {
            for (int b = tid; b < 256; b += TOPK_THREADS) hist[b] = 0u;
            wg_barrier();
            topk_histogram(bits, n, g.thr, prefix, shift, hist);
            wg_barrier();
            if (wave == 0) {                                  // lane l owns bins 255 - 4l .. 252 - 4l: a scan from the top digit down
                uint32_t c[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * lane - j]; s += c[j]; }
                const uint32_t incl = wave_scan_inclusive_u32(s, lane);
                uint32_t above = incl - s;
                // exactly one lane finds the crossing: the first pass counts more than K keys (else `all` below), a later one at
                // least `want` - the chosen bin of the pass before
                if (above < want && want <= incl) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (above < want && want <= above + c[j]) { sel[0] = (uint32_t)(255 - 4 * lane - j); sel[1] = above; }
                        above += c[j];
                    }
                }
                if (lane == 63) sel[2] = incl;
            }
            wg_barrier();
            if (shift == 24 && sel[2] <= K) all = true;       // at most K eligible: take them all (sel[0..1] were not written)
            else { prefix |= sel[0] << shift; want -= sel[1]; }
            wg_barrier();                                     // sel and hist are free for the next pass
        }
        if (!all) { T = prefix; r = want; }
    }

    // ---- compact, in index order ---------------------------------------------------------------------------------------------
    uint32_t gt_run = 0, eq_run = 0;                          // keys > T / == T in the tiles behind this one (same in every thread)
    int par = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += TOPK_THREADS, par ^= 1) {
        const uint32_t i = i0 + tid;
        uint32_t k = 0;
        bool gt = false, eq = false;
        if (i < n) {
            k = topk_key(bits[i]);
            gt = k > T;
            eq = k == T;                                      // T >= thr: both are eligible
        }
        const unsigned long long mg = __builtin_amdgcn_ballot_w64(gt), me = __builtin_amdgcn_ballot_w64(eq);
        if (lane == 0) { wave_cnt[par][wave][0] = (uint32_t)__builtin_popcountll(mg); wave_cnt[par][wave][1] = (uint32_t)__builtin_popcountll(me); }
        wg_barrier();
        uint32_t gt_before = gt_run, eq_before = eq_run, gt_tile = 0, eq_tile = 0;
#pragma unroll
        for (int w = 0; w < TOPK_WAVES; ++w) {
            const uint32_t a = wave_cnt[par][w][0], b = wave_cnt[par][w][1];
            if (w < wave) { gt_before += a; eq_before += b; }
            gt_tile += a; eq_tile += b;
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        gt_before += (uint32_t)__builtin_popcountll(mg & below);
        eq_before += (uint32_t)__builtin_popcountll(me & below);
        if (gt || (eq && eq_before < r)) {                    // slot = selected rows in front: all the greater, the first r equal
            const uint32_t slot = gt_before + (eq_before < r ? eq_before : r);
            if (slot < (uint32_t)TOPK_SORT_CAP)               // holds by construction (at most TOPK_WHOLE or K rows are selected)
                buf[slot] = topk_composite(k, i);
        }
        gt_run += gt_tile; eq_run += eq_tile;                 // the other buffer is written next: one barrier per tile
    }
    uint32_t m = gt_run + (eq_run < r ? eq_run : r);          // composites in the buffer
    m = m < (uint32_t)TOPK_SORT_CAP ? m : (uint32_t)TOPK_SORT_CAP;
    const uint32_t count = m < K ? m : K;

    // ---- sort, descending ----------------------------------------------------------------------------------------------------
    uint32_t S = 1;
    while (S < m) S <<= 1;
    for (uint32_t j = m + tid; j < S; j += TOPK_THREADS) buf[j] = 0ull;       // below every composite (i < 2^31: none is 0)
    wg_barrier();
    for (uint32_t size = 2; size <= S; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < (S >> 1); t += TOPK_THREADS) {
                const uint32_t a = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), b = a | stride;
                const unsigned long long x = buf[a], y = buf[b];
                const bool desc = (a & size) == 0u;
                if (desc ? x < y : x > y) { buf[a] = y; buf[b] = x; }
            }
            wg_barrier();
        }
    }

    // ---- write: K rows per output, the tail filled ---------------------------------------------------------------------------
    const float2* ml = reinterpret_cast<const float2*>(g.ml) + lo;
    const float2* mr = reinterpret_cast<const float2*>(g.mr) + lo;
    float2* tl = reinterpret_cast<float2*>(g.top_l) + p * (int64_t)K;
    float2* tr = reinterpret_cast<float2*>(g.top_r) + p * (int64_t)K;
    uint32_t* tc = reinterpret_cast<uint32_t*>(g.top_conf) + p * (int64_t)K;
    int32_t* ti = g.top_idx + p * (int64_t)K;
    for (uint32_t j = tid; j < K; j += TOPK_THREADS) {
        float2 l = make_float2(0.0f, 0.0f), rr = l;
        uint32_t cb = 0u;
        int32_t idx = -1;
        if (j < count) {
            const uint32_t i = 0xFFFFFFFFu - (uint32_t)buf[j];
            if (i < n) { idx = (int32_t)i; l = ml[i]; rr = mr[i]; cb = bits[i]; }      // always true; keeps the gather inside the segment
        }
        tl[j] = l; tr[j] = rr; tc[j] = cb; ti[j] = idx;
    }
    if (tid == 0) g.top_count[p] = (int64_t)count;
}

}  // namespace pats

using namespace pats;

extern "C" int64_t pats_topk_by_pair_max_k(void) { return TOPK_SORT_CAP; }

extern "C" size_t pats_topk_by_pair_workspace_bytes(int64_t pairs, int64_t K) {
    (void)pairs; (void)K;
    return 0;                                   // everything lives in LDS
}

extern "C" int pats_topk_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                     int64_t pairs, int64_t cap, int64_t K, int use_min_conf, float min_conf, float* top_l,
                                     float* top_r, float* top_conf, int32_t* top_idx, int64_t* top_count, void* workspace,
                                     size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    const int rc = topk_check_args("topk_by_pair", matches_l, matches_r, conf, pair_off, pairs, cap, K, use_min_conf, min_conf, top_l, top_r,
                                   top_conf, top_idx, top_count, workspace_bytes, pats_topk_by_pair_workspace_bytes(pairs, K));
    if (rc != PATS_OK) return rc;
    TopkArgs g{matches_l, matches_r, conf, pair_off, cap, (int)K, use_min_conf ? topk_key(__builtin_bit_cast(uint32_t, min_conf)) : 0u,
               top_l, top_r, top_conf, top_idx, top_count};
    hipLaunchKernelGGL(topk_by_pair_kernel, dim3((unsigned)pairs), dim3(TOPK_THREADS), 0, as_stream(stream), g);
    return check_launch("topk_by_pair kernel");
}
