// Per-pair plane-and-parallax (DEGENSAC) stage of the uncalibrated branch: when most of a pair's matches lie on one plane, a 7-point
// sample with five or more of them gives a whole family of fundamental matrices, and the one verification crowns explains the plane
// and a few accidental points.  The plane's homography H and two matches off the plane fix the epipolar geometry instead (Chum, Werner,
// Matas, CVPR 2005): a_i = H x_i, l_i = x'_i x a_i (the line through the match and its transfer: it holds the epipole), e = l_1 x l_2,
// F = [e]x H.  Two kernels, each one workgroup per pair and one launch for the batch, no host read, no workspace, deterministic.
// include/pats_amd.h states the definition ("Per-pair plane-and-parallax hypotheses and hand-over"), docs/kernels.md 4.25 the design.
//
//   hypotheses  plane_parallax_hypotheses_kernel: the pair's matches off the plane - finite after norm, and outside the homography
//               verification's own test (Homography::test2 of verify.hpp) at parallax * thr - are compacted IN SEGMENT ORDER into an
//               LDS index list: per tile of PP_THREADS matches an inclusive scan inside each wave (lane_reduce.hpp), the waves'
//               totals through LDS and added in wave order (epipolar.hpp), no atomics - the list has the same bits on every run.
//               Then the threads stride over the H hypotheses: two draws of the hypotheses' sampler on the list, the solve in
//               float64, one model each
//   hand-over   plane_parallax_select_kernel: the standing verification is kept unless the plane-and-parallax models'
//               best_count is strictly larger; the kept count, mask, moments and model are written in the verification's standard
//               form, with `replaced` and `overlap` - the standing inliers that the plane explains at thr - beside them
//   LDS         PP_POOL_MAX = 8192 indices = 32 KiB of the list + two rows of wave totals: four workgroups fit a CU
//   loops       the tile walk and the hypothesis walk are bounded by n and H; the solver has no loop
#include "common.hpp"
#include "epipolar.hpp"
#include "lane_reduce.hpp"
#include "verify.hpp"

namespace pats {

constexpr int PP_THREADS = 256;
constexpr int PP_WAVES = PP_THREADS / WAVE;
constexpr int PP_POOL_MAX = 8192;                      // indices the LDS list holds: a longer pool keeps its first PP_POOL_MAX members
static_assert((size_t)PP_POOL_MAX * sizeof(uint32_t) <= 64 * 1024, "the pool list takes at most 64 KiB of LDS");
constexpr double PP_COINCIDE = 1e-9;                   // |e| <= PP_COINCIDE |l_1| |l_2|: the two parallax lines coincide

// the plane of pair p: the winner of its homographies; nine exact zeros are no plane
__device__ __forceinline__ bool pp_plane(const float* __restrict__ models_h, int Mh, const int32_t* __restrict__ best_h, int64_t p,
                                         float (&e)[9]) {
    verify_model(epi_winner(models_h, Mh, best_h, p), e);
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) any = any || e[k] != 0.0f;
    return any;
}

__device__ __forceinline__ void pp_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// F = [e]x H from the plane and two matches off it, |F|_F = 1, the component of largest magnitude positive (the lowest index among
// equals, judged on the float32 values), rounded to float32 -> true; false: the lines coincide or a value is not finite
__device__ __forceinline__ bool pp_solve(const float (&hf)[9], const double (&xl)[2][2], const double (&xr)[2][2], float (&out)[9]) {
    double Hd[9], l[2][3], nl[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hd[k] = (double)hf[k];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const double a[3] = {Hd[0] * xl[t][0] + Hd[1] * xl[t][1] + Hd[2], Hd[3] * xl[t][0] + Hd[4] * xl[t][1] + Hd[5],
                             Hd[6] * xl[t][0] + Hd[7] * xl[t][1] + Hd[8]};
        const double x[3] = {xr[t][0], xr[t][1], 1.0};
        pp_cross(x, a, l[t]);
        nl[t] = __builtin_sqrt(l[t][0] * l[t][0] + l[t][1] * l[t][1] + l[t][2] * l[t][2]);
    }
    double e[3];
    pp_cross(l[0], l[1], e);
    const double ne = __builtin_sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    if (!(ne > PP_COINCIDE * nl[0] * nl[1])) return false;                               // also for a NaN
    double F[9], nn = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {                       // column j of F = e x (column j of H)
        F[j] = e[1] * Hd[6 + j] - e[2] * Hd[3 + j];
        F[3 + j] = e[2] * Hd[j] - e[0] * Hd[6 + j];
        F[6 + j] = e[0] * Hd[3 + j] - e[1] * Hd[j];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) nn += F[k] * F[k];
    const double inv = 1.0 / __builtin_sqrt(nn);
    bool good = nn > 0.0;
    float bigf = -1.0f, atf = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        out[k] = (float)(F[k] * inv);
        good = good && __builtin_isfinite(out[k]);
        const float v = __builtin_fabsf(out[k]);
        if (v > bigf) { bigf = v; atf = out[k]; }
    }
    if (!good) return false;
    if (atf < 0.0f) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = -out[k];
    }
    return true;
}

__global__ void __launch_bounds__(PP_THREADS)
plane_parallax_hypotheses_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                                 const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, int H,
                                 const int64_t* __restrict__ pair_seed, const float* __restrict__ norm,
                                 const float* __restrict__ models_h, int Mh, const int32_t* __restrict__ best_h,
                                 const float* __restrict__ thr, float parallax, float* __restrict__ models,
                                 int32_t* __restrict__ sample_idx, int32_t* __restrict__ pool) {
    __shared__ uint32_t pool_idx[PP_POOL_MAX];
    __shared__ uint32_t wave_tot[2][PP_WAVES];          // two rows: tile k + 1 stores while a slow wave still adds tile k
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    float hf[9];
    const bool plane = pp_plane(models_h, Mh, best_h, p, hf);                            // workgroup-uniform
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const EpiNorm nm = epi_norm(norm, p);
    const float tp = parallax * thr[p];
    const float t2 = tp * tp;

    // the pool, in segment order
    uint32_t m_all = 0;                                 // the pool's size before clamping: the same in every thread
    int row = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += PP_THREADS, row ^= 1) {
        const uint32_t i = i0 + (uint32_t)tid;
        float xl0, xl1, xr0, xr1;
        epi_load(ml, mr, nullptr, i, n, norm != nullptr, nm, false, 0.0f, xl0, xl1, xr0, xr1);       // xl0 = NaN: not finite, or i >= n
        v2f s, lim, w;
        Homography::test2(hf, t2, pk_splat(xl0), pk_splat(xl1), pk_splat(xr0), pk_splat(xr1), s, lim, w);
        const bool off = xl0 == xl0 && (s.x > lim.x || w.x == 0.0f);
        const uint32_t incl = wave_scan_inclusive_u32(off ? 1u : 0u, lane);
        wave_parts_store(wave_tot[row], wave, lane, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63));      // the wave's total
        wg_barrier();
        uint32_t before = m_all, total = 0;
#pragma unroll
        for (int k = 0; k < PP_WAVES; ++k) {
            before += k < wave ? wave_tot[row][k] : 0u;
            total += wave_tot[row][k];
        }
        const uint32_t at = before + incl - 1u;
        if (off && at < (uint32_t)PP_POOL_MAX) pool_idx[at] = i;
        m_all += total;
    }
    wg_barrier();                                       // the list is complete (also orders the last tile's stores before the reads)
    if (tid == 0) pool[p] = (int32_t)m_all;             // m_all <= n < 2^31
    const uint32_t m = m_all < (uint32_t)PP_POOL_MAX ? m_all : (uint32_t)PP_POOL_MAX;
    const bool solve = plane && m >= 2;

    for (int h = tid; h < H; h += PP_THREADS) {
        float* mo = models + (p * H + h) * 9;
        int32_t* so = sample_idx ? sample_idx + (p * H + h) * 2 : nullptr;
        float out[9];
        bool good = false;
        int32_t s0 = -1, s1 = -1;
        if (solve) {
            uint32_t idx[2];
            epi_draw<2>((uint64_t)pair_seed[p], (uint32_t)h, m, idx);                    // idx < m <= PP_POOL_MAX
            const uint32_t seg[2] = {pool_idx[idx[0]], pool_idx[idx[1]]};               // < n: inside the segment
            s0 = (int32_t)seg[0]; s1 = (int32_t)seg[1];
            double xl[2][2], xr[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float a0, a1, b0, b1;
                epi_load(ml, mr, nullptr, seg[t], n, norm != nullptr, nm, false, 0.0f, a0, a1, b0, b1);   // finite: a pool member
                xl[t][0] = (double)a0; xl[t][1] = (double)a1; xr[t][0] = (double)b0; xr[t][1] = (double)b1;
            }
            good = pp_solve(hf, xl, xr, out);
        }
        if (so) { so[0] = s0; so[1] = s1; }
#pragma unroll
        for (int k = 0; k < 9; ++k) mo[k] = good ? out[k] : 0.0f;
    }
}

// the hand-over: standing (a) against plane-and-parallax (b)
__global__ void __launch_bounds__(PP_THREADS)
plane_parallax_select_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const int64_t* __restrict__ pair_off,
                             const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap, const float* __restrict__ norm,
                             const float* __restrict__ models_h, int Mh, const int32_t* __restrict__ best_h, const float* __restrict__ thr,
                             const float* __restrict__ models_a, int Ha, const int32_t* __restrict__ best_a,
                             const int64_t* __restrict__ best_count_a, const uint8_t* __restrict__ inlier_a,
                             const double* __restrict__ moments_a, const float* __restrict__ models_b, int Hb,
                             const int32_t* __restrict__ best_b, const int64_t* __restrict__ best_count_b,
                             const uint8_t* __restrict__ inlier_b, const double* __restrict__ moments_b, float* __restrict__ model,
                             int64_t* __restrict__ best_count, uint8_t* __restrict__ inlier, double* __restrict__ moments,
                             uint8_t* __restrict__ replaced, int32_t* __restrict__ overlap) {
    __shared__ int wave_cnt[PP_WAVES];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const int64_t ca = best_count_a[p], cb = best_count_b[p];
    const bool take = cb > ca;                          // strictly: a tie keeps the standing verification (workgroup-uniform)
    float hf[9];
    pp_plane(models_h, Mh, best_h, p, hf);              // the zero model has no inliers: a2^2 = 0
    const float t = thr[p];
    const bool plane_live = t >= 0.0f;                  // as the verification: a NaN or negative threshold has no inliers
    const float t2 = t * t;
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const EpiNorm nm = epi_norm(norm, p);
    const uint8_t* kept = (take ? inlier_b : inlier_a) + lo;
    int count = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += PP_THREADS) {
        const uint32_t i = i0 + (uint32_t)tid;
        float xl0, xl1, xr0, xr1;
        epi_load_masked(ml, mr, inlier_a + lo, i, n, norm != nullptr, nm, xl0, xl1, xr0, xr1);       // xl0 = NaN off the standing mask
        v2f s, lim, w;
        Homography::test2(hf, t2, pk_splat(xl0), pk_splat(xl1), pk_splat(xr0), pk_splat(xr1), s, lim, w);
        count += wave_count(plane_live && w.x > 0.0f && s.x <= lim.x);
        if (i < n) inlier[lo + i] = kept[i] ? 1 : 0;
    }
    wave_parts_store(wave_cnt, wave, lane, count);
    wg_barrier();
    if (tid == 0) {
        best_count[p] = take ? cb : ca;
        replaced[p] = take ? 1 : 0;
        overlap[p] = wave_parts_total(wave_cnt);
    }
    if (tid < 9) model[p * 9 + tid] = (take ? epi_winner(models_b, Hb, best_b, p) : epi_winner(models_a, Ha, best_a, p))[tid];
    if (moments && tid < 81) moments[p * 81 + tid] = (take ? moments_b : moments_a)[p * 81 + tid];
}

}  // namespace pats

using namespace pats;

extern "C" int64_t pats_plane_parallax_pool_max(void) { return PP_POOL_MAX; }

extern "C" size_t pats_plane_parallax_hypotheses_workspace_bytes(int64_t pairs, int64_t H) {
    (void)pairs; (void)H;
    return 0;                                           // the pool lives in LDS, a sample in its thread's registers
}

// the plane's arguments, checked alike by both entries behind what their siblings check
static int pp_check_plane(const char* who, const float* models_h, int64_t Mh, const int32_t* best_h, const float* thr) {
    PATS_REQUIRE(Mh >= 1 && Mh <= pats_epipolar_max_h(), "%s: Mh = %lld (1 .. max_h = %lld)", who, (long long)Mh,
                 (long long)pats_epipolar_max_h());
    return epi_check_args(who, {{"models_h", models_h, 4}, {"best_h", best_h, 4}, {"thr", thr, 4}}, true);
}

extern "C" int pats_plane_parallax_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off,
                                                          int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H,
                                                          const int64_t* pair_seed, const float* norm, const float* models_h, int64_t Mh,
                                                          const int32_t* best_h, const float* thr, float parallax, float* models,
                                                          int32_t* sample_idx, int32_t* pool, void* workspace, size_t workspace_bytes,
                                                          pats_stream_t stream) {
    (void)workspace;
    const char* who = "plane_parallax_hypotheses_by_pair";
    int64_t chunks;
    int rc = epi_check_hypotheses(who, {"matches_l", matches_l, 8}, matches_r, pair_off, stride, counts_in, pairs, cap, H, pair_seed, norm, 0,
                                  models, sample_idx, nullptr, 1, PP_THREADS, chunks);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(workspace_bytes >= pats_plane_parallax_hypotheses_workspace_bytes(pairs, H), "%s: workspace too small", who);
    PATS_REQUIRE(__builtin_isfinite(parallax) && parallax >= 1.0f, "%s: parallax = %g must be a finite number >= 1", who, (double)parallax);
    if ((rc = pp_check_plane(who, models_h, Mh, best_h, thr)) != PATS_OK) return rc;
    if ((rc = epi_check_arg(who, {"pool", pool, 4}, true)) != PATS_OK) return rc;
    hipLaunchKernelGGL(plane_parallax_hypotheses_kernel, dim3((unsigned)pairs), dim3(PP_THREADS), 0, as_stream(stream), matches_l, matches_r,
                       pair_off, counts_in, stride, cap, (int)H, pair_seed, norm, models_h, (int)Mh, best_h, thr, parallax, models,
                       sample_idx, pool);
    return check_launch("plane_parallax_hypotheses kernel");
}

extern "C" int pats_plane_parallax_select_by_pair(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                  const int64_t* counts_in, int64_t pairs, int64_t cap, const float* norm,
                                                  const float* models_h, int64_t Mh, const int32_t* best_h, const float* thr,
                                                  const float* models_a, int64_t Ha, const int32_t* best_a, const int64_t* best_count_a,
                                                  const uint8_t* inlier_a, const double* moments_a, const float* models_b, int64_t Hb,
                                                  const int32_t* best_b, const int64_t* best_count_b, const uint8_t* inlier_b,
                                                  const double* moments_b, float* model, int64_t* best_count, uint8_t* inlier,
                                                  double* moments, uint8_t* replaced, int32_t* overlap, pats_stream_t stream) {
    const char* who = "plane_parallax_select_by_pair";
    int rc = epi_check_args(who, {{"matches_l", matches_l, 8}, {"matches_r", matches_r, 8}, {"models_a", models_a, 4}, {"best_a", best_a, 4},
                                  {"best_count_a", best_count_a, 8}, {"inlier_a", inlier_a, 1}, {"models_b", models_b, 4}, {"best_b", best_b, 4},
                                  {"best_count_b", best_count_b, 8}, {"inlier_b", inlier_b, 1}, {"model", model, 4},
                                  {"best_count", best_count, 8}, {"inlier", inlier, 1}, {"replaced", replaced, 1}, {"overlap", overlap, 4}},
                            true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"norm", norm, 4}, {"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}, {"moments_a", moments_a, 8},
                              {"moments_b", moments_b, 8}, {"moments", moments, 8}}, false);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    PATS_REQUIRE(Ha >= 1 && Ha <= pats_epipolar_max_h(), "%s: Ha = %lld (1 .. max_h = %lld)", who, (long long)Ha, (long long)pats_epipolar_max_h());
    PATS_REQUIRE(Hb >= 1 && Hb <= pats_epipolar_max_h(), "%s: Hb = %lld (1 .. max_h = %lld)", who, (long long)Hb, (long long)pats_epipolar_max_h());
    PATS_REQUIRE(!moments || (moments_a && moments_b), "%s: moments needs moments_a and moments_b", who);
    if ((rc = pp_check_plane(who, models_h, Mh, best_h, thr)) != PATS_OK) return rc;
    hipStream_t st = as_stream(stream);
    if ((rc = fill_bytes(inlier, 0, (size_t)cap, st)) != PATS_OK) return rc;           // the rows outside the segments
    hipLaunchKernelGGL(plane_parallax_select_kernel, dim3((unsigned)pairs), dim3(PP_THREADS), 0, st, matches_l, matches_r, pair_off, counts_in,
                       stride, cap, norm, models_h, (int)Mh, best_h, thr, models_a, (int)Ha, best_a, best_count_a, inlier_a, moments_a, models_b,
                       (int)Hb, best_b, best_count_b, inlier_b, moments_b, model, best_count, inlier, moments, replaced, overlap);
    return check_launch("plane_parallax_select kernel");
}
