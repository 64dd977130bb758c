// Per-pair spread top-K: the sibling of topk.hip that spreads the shortlist over the image.  A grid of square cells lies over the
// points of one side; every cell keeps its most confident eligible match (the winner), and the K most confident winners are the
// pair's selection, in the form topk_by_pair leaves.  ONE launch for the batch, no host read, no workspace.  include/pats_amd.h
// states the definition; docs/kernels.md 4.19 the design.
//
// One workgroup of 1024 threads per pair; nothing crosses workgroups (no global atomics, no spinning); every loop is bounded by the
// segment length n, by the grid or by K.  The pair's cell table - grid0 * grid1 64-bit slots - lives in dynamic LDS:
//   clear    the table
//   contest  ONE pass over the segment: an eligible match takes its composite key << 32 | (0xFFFFFFFF - i) to table[cellid] with an
//            LDS atomicMax (one ds_max_u64).  The composites are unique, so the maximum does not depend on the order of arrival: a
//            slot ends as the cell's largest key at the lowest i, or 0 (no composite is 0) for a cell without an eligible match
//   compact  the non-zero slots to the front of the table, tile by tile in place (a slot never moves up, and a tile is read whole
//            before anything of it is written): occupied = their number, and the sort below runs on the winners, not on the grid
//   sort     bitonic, descending, on the next power of two above occupied (topk.hip's)
//   write    topk.hip's write phase over the first min(K, occupied) winners, then top_count and occupied
#include "common.hpp"
#include "topk_shared.hpp"

namespace pats {

constexpr int TOPK_SPREAD_MAX_CELLS = 16384;    // = pats_topk_spread_by_pair_max_cells(): 8 bytes per cell, 128 KiB of the 160 a workgroup may allocate
constexpr int TOPK_SPREAD_MAX_CELL = 65536;     // pixels along a cell's edge
constexpr int TOPK_SPREAD_LDS = TOPK_SPREAD_MAX_CELLS * 8;
constexpr int TOPK_SPREAD_LDS_UNASKED = 65536;  // the dynamic LDS a launch gets unasked (common.hpp, DeviceGrants)

struct TopkSpreadArgs {
    const float* ml; const float* mr; const float* conf; const int64_t* pair_off;
    int64_t cap; int K; uint32_t thr;           // thr = key(min_conf), 0 without a threshold: every key is >= 0
    int side; uint32_t cell, grid0, grid1;
    float* top_l; float* top_r; float* top_conf; int32_t* top_idx; int64_t* top_count; int64_t* occupied;
};

// the cell of a coordinate along one component: floor of the float (exact: u <= 2^24 after the clamp), a NaN, a negative value and
// -inf give 0; a point outside the grid falls into the edge cell
__device__ __forceinline__ uint32_t spread_cell(float u, uint32_t cell, uint32_t grid) {
    const uint32_t q = u > 0.0f ? (uint32_t)(int)(u < 16777216.0f ? u : 16777216.0f) : 0u;
    const uint32_t c = q / cell;
    return c < grid - 1u ? c : grid - 1u;
}

// topk.hip's sort and write phases as functions.  (topk.hip keeps its own text: called as functions there they change the
// schedule of topk_by_pair_kernel, whose code stays what it was.)
// buf[0 .. m) descending, bitonic on the next power of two (the composites are unique: any network gives the same answer).  buf
// holds that power of two; called by all threads, buf[0 .. m) written and no barrier behind the writes yet
__device__ __forceinline__ void topk_sort_desc(unsigned long long* buf, uint32_t m) {
    const uint32_t tid = threadIdx.x;
    uint32_t S = 1;
    while (S < m) S <<= 1;
    for (uint32_t j = m + tid; j < S; j += TOPK_THREADS) buf[j] = 0ull;       // below every composite
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
}

// write: K rows per output of pair p, rows 0 .. count - 1 gathered through the sorted composites, the tail filled (-1 / 0.0)
__device__ __forceinline__ void topk_write(const unsigned long long* buf, uint32_t count, uint32_t K, int64_t p, int64_t lo, uint32_t n,
                                           const float* ml_, const float* mr_, const uint32_t* bits, float* top_l, float* top_r,
                                           float* top_conf, int32_t* top_idx) {
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    float2* tl = reinterpret_cast<float2*>(top_l) + p * (int64_t)K;
    float2* tr = reinterpret_cast<float2*>(top_r) + p * (int64_t)K;
    uint32_t* tc = reinterpret_cast<uint32_t*>(top_conf) + p * (int64_t)K;
    int32_t* ti = top_idx + p * (int64_t)K;
    for (uint32_t j = threadIdx.x; j < K; j += TOPK_THREADS) {
        float2 l = make_float2(0.0f, 0.0f), rr = l;
        uint32_t cb = 0u;
        int32_t idx = -1;
        if (j < count) {
            const uint32_t i = 0xFFFFFFFFu - (uint32_t)buf[j];
            if (i < n) { idx = (int32_t)i; l = ml[i]; rr = mr[i]; cb = bits[i]; }      // always true; keeps the gather inside the segment
        }
        tl[j] = l; tr[j] = rr; tc[j] = cb; ti[j] = idx;
    }
}

__global__ void __launch_bounds__(TOPK_THREADS) topk_spread_by_pair_kernel(TopkSpreadArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long spread_table[];     // the next power of two above cells
    __shared__ uint32_t wave_cnt[2][TOPK_WAVES];              // per tile (double-buffered), per wave: non-zero slots
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t K = (uint32_t)g.K, cells = g.grid0 * g.grid1;
    PATS_TOPK_SEGMENT(g.pair_off, p, g.cap);                  // lo, n: the pair's rows, inside the arrays whatever pair_off holds
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(g.conf) + lo;
    const float2* pts = reinterpret_cast<const float2*>(g.side ? g.mr : g.ml) + lo;

    // ---- clear ---------------------------------------------------------------------------------------------------------------
    for (uint32_t c = tid; c < cells; c += TOPK_THREADS) spread_table[c] = 0ull;
    wg_barrier();

    // ---- contest: one pass over the segment -------------------------------------------------------------------------------------
    for (uint32_t i = tid; i < n; i += TOPK_THREADS) {
        const uint32_t k = topk_key(bits[i]);
        if (k < g.thr) continue;
        const float2 u = pts[i];
        const uint32_t id = spread_cell(u.x, g.cell, g.grid0) * g.grid1 + spread_cell(u.y, g.cell, g.grid1);      // < cells
        atomicMax(&spread_table[id], topk_composite(k, i));
    }
    wg_barrier();

    // ---- compact the winners to the front, in place ----------------------------------------------------------------------------
    // tile t0 is read into registers before the barrier; its winners land at or below their own slots, inside this tile or the
    // tiles behind it, which every thread has read
    uint32_t run = 0;                                         // winners in the tiles behind this one (same in every thread)
    int par = 0;
    for (uint32_t t0 = 0; t0 < cells; t0 += TOPK_THREADS, par ^= 1) {
        const uint32_t c = t0 + tid;
        const unsigned long long v = c < cells ? spread_table[c] : 0ull;
        const unsigned long long mk = __builtin_amdgcn_ballot_w64(v != 0ull);
        if (lane == 0) wave_cnt[par][wave] = (uint32_t)__builtin_popcountll(mk);
        wg_barrier();
        uint32_t before = run, tile = 0;
#pragma unroll
        for (int w = 0; w < TOPK_WAVES; ++w) {
            const uint32_t a = wave_cnt[par][w];
            if (w < wave) before += a;
            tile += a;
        }
        before += (uint32_t)__builtin_popcountll(mk & ((1ull << lane) - 1ull));
        if (v != 0ull) spread_table[before] = v;              // before <= c
        run += tile;                                          // the other buffer is written next: one barrier per tile
    }
    const uint32_t occ = run;                                 // <= cells
    const uint32_t count = occ < K ? occ : K;

    // ---- sort, descending; write: K rows per output, the tail filled ----------------------------------------------------------
    topk_sort_desc(spread_table, occ);
    topk_write(spread_table, count, K, p, lo, n, g.ml, g.mr, bits, g.top_l, g.top_r, g.top_conf, g.top_idx);
    if (tid == 0) { g.top_count[p] = (int64_t)count; g.occupied[p] = (int64_t)occ; }
}

}  // namespace pats

using namespace pats;

extern "C" int64_t pats_topk_spread_by_pair_max_cells(void) { return TOPK_SPREAD_MAX_CELLS; }

extern "C" size_t pats_topk_spread_by_pair_workspace_bytes(int64_t pairs, int64_t K, int64_t grid0, int64_t grid1) {
    (void)pairs; (void)K; (void)grid0; (void)grid1;
    return 0;                                   // everything lives in LDS
}

extern "C" int pats_topk_spread_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                            int64_t pairs, int64_t cap, int64_t K, int use_min_conf, float min_conf, int side,
                                            int64_t cell, int64_t grid0, int64_t grid1, float* top_l, float* top_r, float* top_conf,
                                            int32_t* top_idx, int64_t* top_count, int64_t* occupied, void* workspace,
                                            size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    int rc = topk_check_args("topk_spread_by_pair", matches_l, matches_r, conf, pair_off, pairs, cap, K, use_min_conf, min_conf, top_l, top_r,
                             top_conf, top_idx, top_count, workspace_bytes, pats_topk_spread_by_pair_workspace_bytes(pairs, K, grid0, grid1));
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_arg("topk_spread_by_pair", {"occupied", occupied, 8}, true)) != PATS_OK) return rc;
    PATS_REQUIRE(side == 0 || side == 1, "topk_spread_by_pair: side = %d (0 = matches_l, 1 = matches_r)", side);
    PATS_REQUIRE(cell >= 1 && cell <= TOPK_SPREAD_MAX_CELL, "topk_spread_by_pair: cell = %lld (1 .. %d pixels)", (long long)cell,
                 TOPK_SPREAD_MAX_CELL);
    PATS_REQUIRE(grid0 >= 1, "topk_spread_by_pair: grid0 = %lld must be at least 1", (long long)grid0);
    PATS_REQUIRE(grid1 >= 1, "topk_spread_by_pair: grid1 = %lld must be at least 1", (long long)grid1);
    // each factor first: the product of two int64 above max_cells could wrap
    PATS_REQUIRE(grid0 <= TOPK_SPREAD_MAX_CELLS && grid1 <= TOPK_SPREAD_MAX_CELLS && grid0 * grid1 <= TOPK_SPREAD_MAX_CELLS,
                 "topk_spread_by_pair: grid0 * grid1 = %lld x %lld cells exceed max_cells = %d (take a larger cell)", (long long)grid0,
                 (long long)grid1, TOPK_SPREAD_MAX_CELLS);
    uint32_t slots = 1;                         // the table the sort may use: the next power of two above the cells
    while (slots < (uint32_t)(grid0 * grid1)) slots <<= 1;
    const size_t lds = (size_t)slots * sizeof(unsigned long long);
    static DeviceGrants grants;                 // grids above 64 KiB of table exceed what a launch gets unasked
    if (lds > (size_t)TOPK_SPREAD_LDS_UNASKED && !grants.get({{(const void*)topk_spread_by_pair_kernel, TOPK_SPREAD_LDS}}).granted) {
        set_error("topk_spread_by_pair: the device refused %d bytes of dynamic LDS per workgroup", TOPK_SPREAD_LDS);
        return PATS_ERR_UNSUPPORTED;
    }
    TopkSpreadArgs g{matches_l, matches_r, conf, pair_off, cap, (int)K, use_min_conf ? topk_key(__builtin_bit_cast(uint32_t, min_conf)) : 0u,
                     side, (uint32_t)cell, (uint32_t)grid0, (uint32_t)grid1, top_l, top_r, top_conf, top_idx, top_count, occupied};
    hipLaunchKernelGGL(topk_spread_by_pair_kernel, dim3((unsigned)pairs), dim3(TOPK_THREADS), lds, as_stream(stream), g);
    return check_launch("topk_spread_by_pair kernel");
}
