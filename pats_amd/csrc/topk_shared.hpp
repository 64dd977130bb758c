// What the per-pair selections share (topk.hip: the K most confident matches; topk_spread.hip: the K most confident cell winners):
// the key, the composite, a pair's segment and the argument checks.
#pragma once
#include "common.hpp"

namespace pats {

constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_WAVES = TOPK_THREADS / WAVE;

__host__ __device__ __forceinline__ uint32_t topk_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

// the composite a selection sorts: unique per match, none is 0 (i < 2^31); a larger one is a larger key, or the same key at a lower i
__device__ __forceinline__ unsigned long long topk_composite(uint32_t k, uint32_t i) {
    return ((unsigned long long)k << 32) | (unsigned long long)(0xFFFFFFFFu - i);
}

// Pair p's segment as `lo` and `n` of the kernel that writes this: rows lo .. lo + n - 1.  A stale or corrupt pair_off never reaches
// outside the arrays: both ends clamped to [0, cap], hi <= lo = empty.  A macro, not a function: through a function, however it
// is written, hipcc schedules topk_by_pair_kernel's compact loop differently, and that kernel's code does not change with this split.
#define PATS_TOPK_SEGMENT(pair_off, p, cap)                                                                                           \
    int64_t lo = (pair_off)[p], hi = (pair_off)[(p) + 1];                                                                            \
    lo = lo < 0 ? 0 : (lo > (cap) ? (cap) : lo);                                                                                      \
    hi = hi < 0 ? 0 : (hi > (cap) ? (cap) : hi);                                                                                      \
    const uint32_t n = hi > lo ? (uint32_t)(hi - lo) : 0u /* cap < 2^31 (checked on the host) */

// The arguments both entry points take, refused in one order and wording (who = the entry's name; need = its workspace query's answer)
inline int topk_check_args(const char* who, const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                           int64_t pairs, int64_t cap, int64_t K, int use_min_conf, float min_conf, const float* top_l, const float* top_r,
                           const float* top_conf, const int32_t* top_idx, const int64_t* top_count, size_t workspace_bytes, size_t need) {
    const int rc = epi_check_args(who, {{"matches_l", matches_l, 8}, {"matches_r", matches_r, 8}, {"conf", conf, 4}, {"pair_off", pair_off, 8},
                                        {"top_l", top_l, 8}, {"top_r", top_r, 8}, {"top_conf", top_conf, 4}, {"top_idx", top_idx, 4},
                                        {"top_count", top_count, 8}}, true);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(pairs >= 1 && pairs <= 0x7fffffff, "%s: pairs = %lld (1 .. 2^31 - 1)", who, (long long)pairs);
    PATS_REQUIRE(cap >= 0 && cap < 0x7fffffff, "%s: cap = %lld (0 .. 2^31 - 2: top_idx is int32)", who, (long long)cap);
    PATS_REQUIRE(K >= 1 && K <= pats_topk_by_pair_max_k(), "%s: K = %lld (1 .. max_k = %lld)", who, (long long)K,
                 (long long)pats_topk_by_pair_max_k());
    PATS_REQUIRE(!use_min_conf || min_conf >= 0.0f, "%s: min_conf = %g must be a non-negative number", who, (double)min_conf);
    PATS_REQUIRE(workspace_bytes >= need, "%s: workspace too small", who);
    return PATS_OK;
}

}  // namespace pats
