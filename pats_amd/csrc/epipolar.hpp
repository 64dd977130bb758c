// What the per-pair epipolar stages share (epipolar.hip: verification; hypotheses.hip: the 8-point hypotheses): how a pair's segment
// of the match lists and its normalisation are read.  include/pats_amd.h states both.
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

}  // namespace pats
