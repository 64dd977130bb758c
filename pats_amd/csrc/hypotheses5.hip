// Per-pair 5-point hypotheses, the calibrated sibling of hypotheses.hip: for every pair and every sample h in 0 .. H-1 five distinct
// matches of the pair's segment are drawn with the hypotheses' sampler (epi_draw of epipolar.hpp) and the real essential matrices
// through them - at most ten - are written as row-major 3x3 float32 models, compacted into the sample's lowest slots, the rest zero.
// One launch, no host read, no workspace, deterministic.  include/pats_amd.h states the definition ("Per-pair 5-point hypotheses"),
// essential5.hpp holds the solver (float64 throughout), docs/kernels.md 4.10 the design and the measurements.
//
//   one THREAD per sample, 64 samples (one wave) per workgroup, grid = pairs x ceil(H / 64)
//   storage  the 10x20 float64 matrix of the ten cubic constraints is pivoted with a per-lane row index, which registers cannot
//            take without scratch: it lives in LDS, with the null-space basis behind it - 236 doubles per sample, slot i of lane l at
//            double i * 64 + l, so every access of a wave is one conflict-free 512-byte row whatever rows its lanes pivot on.
//            64 samples x 1888 B = 120832 B: ONE workgroup, one wave, per CU.  A batch of 48 x 100 samples is 96 workgroups on 256
//            CUs, so the occupancy costs nothing there; 32 samples per workgroup would halve the LDS and idle half of each wave
//   figures  (-Rpass-analysis=kernel-resource-usage, gfx950) are in docs/kernels.md 4.10: no scratch, no spill
//   loops    every loop has a constant trip cap (essential5.hpp: 64 bisection and 6 Newton steps per root, 10 roots); a sample that
//            does not get there yields zeros
#include "common.hpp"
#include "epipolar.hpp"
#include "essential5.hpp"

namespace pats {

constexpr int E5_THREADS = 64;                         // samples per workgroup: one wave
constexpr int E5_LDS = E5_SLOTS * E5_THREADS * (int)sizeof(double);

struct E5Lds {                                         // slot i of this lane
    double* base;
    __device__ __forceinline__ double& operator()(int i) const { return base[i * E5_THREADS]; }
};

__global__ void __launch_bounds__(E5_THREADS)
epipolar_hypotheses5_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                            const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int chunks, int H,
                            const int64_t* __restrict__ pair_seed, const float* __restrict__ norm, int progressive,
                            float* __restrict__ models, int32_t* __restrict__ sample_idx, int32_t* __restrict__ n_models) {
    extern __shared__ __attribute__((aligned(16))) double e5_lds[];
    const uint32_t b = blockIdx.x;
    const int64_t p = (int64_t)(b / (uint32_t)chunks);
    const int h = (int)(b % (uint32_t)chunks) * E5_THREADS + (int)threadIdx.x;
    if (h >= H) return;                                 // no barrier below: a lane's LDS slots are its own
    float* mo = models + (p * H + h) * (E5_MAX_MODELS * 9);
    double l0[5], l1[5], r0[5], r1[5];
    const EpiSample drawn = epi_sample<5>(ml_, mr_, pair_off, counts_in, stride, cap, pair_seed, norm, progressive, sample_idx, p, h, H, l0,
                                          l1, r0, r1);
    int count = 0;
    if (drawn == EPI_SAMPLE_READY) count = e5_solve(l0, l1, r0, r1, E5Lds{e5_lds + threadIdx.x}, mo);
    for (int k = count * 9; k < E5_MAX_MODELS * 9; ++k) mo[k] = 0.0f;     // every slot of a short pair or a non-finite sample
    if (n_models) n_models[p * H + h] = count;
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_epipolar_hypotheses5_workspace_bytes(int64_t pairs, int64_t H) {
    (void)pairs; (void)H;
    return 0;                                           // a sample lives in its thread's registers and LDS slots
}

extern "C" int pats_epipolar_hypotheses5_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                     const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                     const int64_t* pair_seed, const float* norm, int progressive, float* models,
                                                     int32_t* sample_idx, int32_t* n_models, void* workspace, size_t workspace_bytes,
                                                     pats_stream_t stream) {
    (void)workspace;
    int64_t chunks;
    const int rc = epi_check_hypotheses("epipolar_hypotheses5_by_pair", {"matches_l", matches_l, 8}, matches_r, pair_off, stride, counts_in, pairs, cap,
                                        H, pair_seed, norm, progressive, models, sample_idx, n_models, E5_MAX_MODELS, E5_THREADS, chunks);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_epipolar_hypotheses5_workspace_bytes(pairs, H), "epipolar_hypotheses5_by_pair: workspace too small");
    static DeviceGrants grants;                         // the kernel's LDS is above the 64 KiB a launch gets unasked
    if (!grants.get({{(const void*)epipolar_hypotheses5_kernel, E5_LDS}}).granted) {
        set_error("epipolar_hypotheses5_by_pair: the device refused %d bytes of LDS per workgroup", E5_LDS);
        return PATS_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(epipolar_hypotheses5_kernel, dim3((unsigned)(pairs * chunks)), dim3(E5_THREADS), E5_LDS, as_stream(stream), matches_l,
                       matches_r, pair_off, counts_in, stride, cap, (int)chunks, (int)H, pair_seed, norm, progressive, models, sample_idx,
                       n_models);
    return check_launch("epipolar_hypotheses5 kernel");
}
