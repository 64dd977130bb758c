// Device-side body of ThirdLayer.Compute_result + the match label for ONE 65x65 problem, executed
// by one wave (models/third_layer.py:161-170,184-217).  `Sp` may point to global memory or LDS and
// holds the plan (or the log-plan when input_is_log) with row stride 65.  Shared by
// compute_result_kernel (third.hip) and the fused third-level kernel (sinkhorn.hip).
#pragma once
#include "common.hpp"

namespace pats {

struct ComputeResultOut {
    float* mk0;            // [P,16,2]
    float* mk1;            // [P,16,2]
    float* wl_raw;         // [P,16] or null
    float* label;          // [P*16,2]
    uint8_t* ifm;          // [P,16]
    int* count;            // global count of whole_loss >= 1e-2, or null
};

// arguments of the register-block fused third-level kernel (third_fused.hip)
struct Fused65Args {
    const float* d0;             // [P,D,65] descriptors of `dtype` elements: a kernel instantiated for the element type T
    const float* d1;             // reads them as (const T*)
    int D;
    int64_t P;
    const float* ns;             // [P,64] target areas
    const float* one;
    int iters, linear;
    const float* scale_x;
    const float* scale_y;
    const int64_t* p_s;
    const int64_t* p_t;
    int outdoor;
    ComputeResultOut cr;
    int stagger;
    unsigned long long* fallbacks;   // guard-trip counter or null
    int scan;                        // third_fused_kernel: re-solve only the problems flagged THIRD_REDO
    const int64_t* P_dev;            // throughput mode: the launch covers the capacity P, *P_dev problems exist (or null)
    int fingerprint;                 // libpats_amd_diag.so only: leave a fingerprint of the score matrix in label[p*16][1]
    int lds_poison_on;               // libpats_amd_diag.so only: fill the workgroup's LDS with lds_poison first
    unsigned lds_poison;
    int reverse_blocks;              // libpats_amd_diag.so only: workgroup b solves problem P - 1 - b (round-6 first-launch experiment)
    int dtype;                       // pats_map_dtype_t of d0 / d1 (0 = float32): picks the instantiation, no kernel reads it
};
// number of problems that exist: min(capacity, device-side count)
__device__ __forceinline__ int64_t live_problems(const Fused65Args& g) {
    if (!g.P_dev) return g.P;
    const int64_t n = *g.P_dev;
    return n < g.P ? n : g.P;
}
constexpr uint8_t THIRD_REDO = 0xEE; // if_matching1[p*16] of a problem the log-domain kernel must redo
// conf: [P,16] per-match confidence or null.  Not a member of Fused65Args: the *_conf_kernel instantiations take it as a kernel
// argument of their own, so the plain kernels' argument block - and with it their code - stays what it was.
int launch_third_fused(const Fused65Args& g, hipStream_t st, float* conf = nullptr);      // third_fused.hip
// its linear-domain solve (third_fused3.hip): flags the problems that leave the guard band with THIRD_REDO
int launch_third_fused3(const Fused65Args& g0, hipStream_t st, float* conf);

// ---- shared by the two register-block files (third_fused.hip, third_fused3.hip) ---------------------------------------------
constexpr int SST = 36;                 // staging row stride (floats): 16-byte aligned rows

// Every problem takes the same time, so without this all resident waves stay phase-locked: the
// chip alternates between "everyone streams descriptors" (HBM-bound, VALU idle) and "everyone
// sweeps" (VALU/LDS-bound, HBM idle) and the phase times ADD.  A hashed one-off start delay for
// the first wave-front (the first FRONT workgroups) spreads the phases; later blocks inherit the
// spread from the slot they take over.  Purely a scheduling aid - no effect on results.
// stagger: the delay unit in s_sleep(127) periods (0 = off).
template <unsigned FRONT>
__device__ __forceinline__ void dephase_first_front(int stagger) {
    if (stagger > 0 && blockIdx.x < FRONT) {
        const unsigned slots = (blockIdx.x * 2654435761u) >> 29;         // 0..7
        for (unsigned q = 0; q < slots * (unsigned)stagger; ++q) __builtin_amdgcn_s_sleep(127);
    }
}

// The re-solve walk of the kernels that run behind third_fused3_kernel: the W workgroups of the launch share the problems
// INTERLEAVED - workgroup w looks at w, w + W, w + 2 W, ... (64 candidates per ballot) and calls solve(p) for those whose
// if_matching1 slot carries THIRD_REDO (left there by third_fused3_kernel's guard).  Flagged problems come in runs (the points
// of one wild fine row are consecutive): with contiguous blocks of 64 per workgroup - round 3 - one wave re-solved a whole run
// serially while the rest of the GPU idled (9.1 ms per step for 8 000 flagged problems, profiles/r04_wild10_step_kernel_stats.md);
// interleaved, a run of 64 goes to 64 different waves.  tests/test_third_redo_walk_gpu.py models this loop.
template <class Solve>
__device__ __forceinline__ void third_redo_walk(const Fused65Args& g, int lane, Solve&& solve) {
    const int64_t W = gridDim.x, live = live_problems(g);
    for (int64_t first = blockIdx.x; first < live; first += 64 * W) {
        const int64_t cand = first + (int64_t)lane * W;
        const bool redo = cand < live && g.cr.ifm[cand * 16] == THIRD_REDO;
        unsigned long long todo = __ballot(redo);
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            wg_barrier();
            solve(first + (int64_t)k * W);
        }
    }
}
// the walk's grid: two rounds of the 3 072 wave slots, so that flagged runs spread out; at least one workgroup
inline unsigned third_walk_grid(int64_t P) { return (unsigned)(P < 1 ? 1 : P < 6144 ? P : 6144); }

// row-level (16-lane) all-reduces: 4 DPP steps, no LDS traffic
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<DPP_QUAD_XOR1>(v);
    v += dpp_f<DPP_QUAD_XOR2>(v);
    v += dpp_f<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_f<DPP_ROW_MIRROR>(v);
    return v;
}
template <int CTRL>
__device__ __forceinline__ void argmax_step(float& v, int& i) {
    const float ov = dpp_f<CTRL>(v);
    const int oi = dpp_i<CTRL>(i);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }     // first index wins ties
}
__device__ __forceinline__ void row16_argmax(float& v, int& i) {
    argmax_step<DPP_QUAD_XOR1>(v, i);
    argmax_step<DPP_QUAD_XOR2>(v, i);
    argmax_step<DPP_ROW_HALF_MIRROR>(v, i);
    argmax_step<DPP_ROW_MIRROR>(v, i);
}

// winmass / rowmass, at most 1 (the two fp32 sums are taken in different orders: a window that holds the whole row's mass may
// come out an ulp above it); a NaN or a 0 / 0 stays what the division gives
__device__ __forceinline__ float confidence_ratio(float winmass, float rowmass) {
    const float c = winmass / rowmass;
    return c > 1.0f ? 1.0f : c;
}

// One wave, one problem.  The 16 centre rows are processed four at a time: each 16-lane DPP row
// of the wave owns one centre row (lane t of the group holds targets t, t+16, t+32, t+48), so the
// argmax / sums are 4-step row-level DPP reductions and the 5x5 taps are two per lane, gathered
// from the plan by address.  sx / sy are indexable [64] scale vectors (global or LDS).
// `compact_stride` == 0: Sp is the full 65 x 65 matrix (row stride 65); > 0: Sp holds only the 16
// centre rows, row q at Sp + q * compact_stride; < 0: see below.
// CONF: conf[p*16 + q] = (plan mass inside the 5x5 window) / (mass of the whole row, dustbin included) - the two terms of
// third_layer.py:212-213 as a ratio; both sums exist here for whole_loss.  CONF = 0 compiles to what it was.
template <int CONF = 0>
__device__ __forceinline__ void compute_result_problem(const float* Sp, int input_is_log, int64_t p,
                                                       const float* sx, const float* sy, float ps0,
                                                       float ps1, float pt0, float pt1, int outdoor,
                                                       const ComputeResultOut& o, int lane,
                                                       int compact_stride = 0, bool scale_is_area = false,
                                                       float* conf = nullptr) {
    constexpr int W = 8, T = 5, NN = 65;
    const int grp = lane >> 4, t = lane & 15;
    int local_count = 0;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int q = pass * 4 + grp;
        const int qy = q / 4 + 2, qx = q % 4 + 2;                    // [:, 2:6, 2:6]  (:186,188)
        // compact_stride > 0: row q at q * stride; < 0: the four block rows 2..5 with all eight local rows each,
        // row (qy - 2) * 8 + qx at stride -compact_stride (third_fused3.hip)
        const float* row = compact_stride > 0 ? Sp + q * compact_stride
                         : compact_stride < 0 ? Sp + ((qy - 2) * 8 + qx) * (-compact_stride)
                                              : Sp + (qy * W + qx) * NN;
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = row[t + 16 * k];
            if (input_is_log) x[k] = expf(x[k]);
        }
        float xd = row[64];                                           // dustbin column
        if (input_is_log) xd = expf(xd);
        // argmax over the 64 real columns (:188); the all-column argmax of (row + 1e-8) (:167-168)
        // hits the dustbin only if it is strictly larger than every real entry
        float bv = x[0];
        int bi = t;
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (x[k] > bv) { bv = x[k]; bi = t + 16 * k; }
        row16_argmax(bv, bi);
        const int max0 = bi;
        const bool matching = !((xd + 1e-8f) > (bv + 1e-8f));
        const float rowsum = row16_sum((x[0] + x[1]) + (x[2] + x[3])) + xd;
        const int mx = max0 % W, my = max0 / W;
        // 5x5 taps, two per lane (tap ids t and t + 16)
        float wpx = 0.f, wpy = 0.f, sumx = 0.f, sumy = 0.f, unfold = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int tap = t + 16 * h;
            if (tap < T * T) {
                const int tx = tap % T, ty = tap / T;
                const int ux = mx + tx - 2, uy = my + ty - 2;         // index3 on the pad-2 map (:189-191)
                const bool inside = ux >= 0 && ux < W && uy >= 0 && uy < W;
                const int src = inside ? uy * W + ux : 0;
                float sbv = row[src];
                if (input_is_log) sbv = expf(sbv);
                sbv = inside ? sbv : 0.0f;                            // ZeroPad2d(2)           (:185)
                // scale_is_area: sx = sy = the OT's target areas and scale_x = scale_y = sqrt(area + 1e-8) is formed here
                // (third_layer.py:153-154) instead of by the caller
                float scx = inside ? sx[src] : 1e-2f;                 // ConstantPad2d(2, 1e-2) (:195-196)
                float scy = inside ? sy[src] : 1e-2f;
                if (scale_is_area && inside) scx = scy = sqrtf(scx + 1e-8f);
                const float root = sqrtf(sbv + 1e-7f);
                const float fx = root / scx, fy = root / scy;         // :197-198
                wpx += fx * ((float)tx * 2.0f - (float)(T - 1));      // meshgrid * 2 - (T - 1)  (:199)
                wpy += fy * ((float)ty * 2.0f - (float)(T - 1));
                sumx += fx;
                sumy += fy;
                unfold += sbv;
            }
        }
        wpx = row16_sum(wpx); wpy = row16_sum(wpy);
        sumx = row16_sum(sumx); sumy = row16_sum(sumy); unfold = row16_sum(unfold);
        if (t == 0) {
            const int64_t oo = (p * 16 + q) * 2;
            const float m1x = wpx / sumx + ((float)mx + 0.5f - (float)W / 2) * 2.0f;   // :206
            const float m1y = wpy / sumy + ((float)my + 0.5f - (float)W / 2) * 2.0f;   // :207
            o.mk1[oo + 0] = m1x + pt0;                                                  // :208
            o.mk1[oo + 1] = m1y + pt1;
            o.mk0[oo + 0] = ps0 + (float)(q % 4) * 2.0f - 3.0f;                         // :209-210
            o.mk0[oo + 1] = ps1 + (float)(q / 4) * 2.0f - 3.0f;
            const float wl = rowsum - unfold;                                           // :213
            if (o.wl_raw) o.wl_raw[p * 16 + q] = wl;
            if (CONF) conf[p * 16 + q] = confidence_ratio(unfold, rowsum);
            if (wl >= 1e-2f) local_count += 1;
            o.ifm[p * 16 + q] = matching ? 1 : 0;
            float l0 = 1e8f;                                                            // :161
            if (!outdoor) {
                const bool select = (q == 5 || q == 15 || q == 7 || q == 13);           // :163-166
                l0 = select ? l0 : -10.0f;
            } else {
                l0 = matching ? l0 : -10.0f;                                            // :169-170
            }
            o.label[oo + 0] = l0;
            o.label[oo + 1] = 1e8f;
        }
    }
    if (o.count) {
        // lanes with t == 0 (4 per wave) hold the counts
        int c = local_count;
        c += __shfl_xor(c, 16);
        c += __shfl_xor(c, 32);
        if (lane == 0 && c) atomicAdd(o.count, c);
    }
}

}  // namespace pats
