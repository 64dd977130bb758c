// Per-pair local optimisation: the rounds "refit the winner's inliers, verify the refit" that follow a verification, walked by ONE
// launch with the pair's matches resident in LDS, the best round kept.  Every value is one the existing entry points produce - the
// support of a model is the verification's (H = 1, moments), the refit the pose's E, the fundamental refit's F or the homography
// refit's H cast to float32 - so the result equals that chain of calls bit for bit.  include/pats_amd.h states the definition ("Per-pair local optimisation");
// docs/kernels.md 4.13 the design.
//
//   verify_polish_kernel<T>: one workgroup per pair, EPI_MASK_THREADS = 512 threads (the walk whose order fixes the moments' bits),
//   decided by the sizes alone.
//   stage   the segment is read ONCE with epi_load (normalised, gated; a match that does not take part carries a NaN x_l) into LDS,
//           16 bytes per match, up to POLISH_STAGE matches (dynamic LDS, sized by the launch from the longest possible segment).  A
//           longer segment is walked in global memory through epi_load every round instead: the same values.
//   round   one pass gives the count (ballots) and the 45 moment sums (T::test2 and T::accumulate of verify.hpp, thread-local in index
//           order); verify_moments_sum reduces them in the mask kernel's order straight into the Jacobi's matrix in LDS;
//           jacobi9_sweeps; thread 0 runs the family's refit (refit.hpp) and casts it to float32: the next round's model.  A refit
//           that repeats its input bit for bit ends the walk - every later round would repeat it.
//   best    the lowest round with the largest count: its model and its 45 moments stay in LDS
//   mask    one last pass with the best model writes the inlier bytes (zero-filled before the launch): the same test function, so
//           the mask's sum over the segment is best_count exactly
// No round touches global memory but for its counts[p, r] store (and the walk of a segment too long to stage).
#include "common.hpp"
#include "epipolar.hpp"
#include "verify.hpp"
#include "jacobi9.hpp"
#include "refit.hpp"

namespace pats {

constexpr int POLISH_THREADS = EPI_MASK_THREADS;
constexpr int POLISH_WAVES = EPI_MASK_WAVES;
constexpr int POLISH_STAGE = 8192;                     // matches a workgroup keeps in LDS: 128 KiB of the CU's 160
constexpr int POLISH_MAX_ROUNDS = 16;
constexpr int POLISH_LDS = POLISH_STAGE * (int)sizeof(float4);

// the families' refits, on one thread behind jacobi9_sweeps: what pats_epipolar_pose_by_pair_f64 / pats_homography_refit_by_pair_f64 /
// pats_fundamental_refit_by_pair_f64 return for (moments, best_count, swapped = 0), cast to float32.  live: the count reaches the family's minimum; bad: a non-finite moment
template <class T> struct PolishRefit;

template <> struct PolishRefit<Epipolar> {
    static constexpr int MIN_INLIERS = POSE_MIN_INLIERS, SWEEPS = POSE_SWEEPS;
    static __device__ __forceinline__ void refit(const double (&sA)[9][9], const double (&sV)[9][9], bool live, bool bad, double (&out)[9]) {
        double e[9], E[9], R1[9], R2[9], u[3];
        bool ok = live && !bad;
        if (ok) {
            double lmin;
            refit_eigvec(sA, sV, e, lmin);
#pragma unroll
            for (int k = 0; k < 9; ++k) ok = ok && __builtin_isfinite(e[k]);
        }
        if (ok) ok = pose_decompose(e, E, R1, R2, u);
        hom_write(E, ok, 0, out);                       // the pose's sign rule is the homography's
    }
};

template <> struct PolishRefit<Homography> {
    static constexpr int MIN_INLIERS = HOM_MIN_INLIERS, SWEEPS = HOM_SWEEPS;
    static __device__ __forceinline__ void refit(const double (&sA)[9][9], const double (&sV)[9][9], bool live, bool bad, double (&out)[9]) {
        double e[9];
        bool ok = live && !bad;
        if (ok) {
            double lmin;
            const int m = refit_eigvec(sA, sV, e, lmin);
            const double lsec = refit_second(sA, m);
            ok = __builtin_isfinite(lmin) && __builtin_isfinite(lsec);
        }
        if (ok) {
            bool any = false;
#pragma unroll
            for (int k = 0; k < 9; ++k) { ok = ok && __builtin_isfinite(e[k]); any = any || e[k] != 0.0; }
            ok = ok && any;                             // the zero model is no model
        }
        hom_write(e, ok, 0, out);
    }
};

// pats_fundamental_refit_by_pair_f64's F: the refit truncated to rank 2 instead of projected onto the essential matrices
template <> struct PolishRefit<Fundamental> {
    static constexpr int MIN_INLIERS = FUND_MIN_INLIERS, SWEEPS = FUND_SWEEPS;
    static __device__ __forceinline__ void refit(const double (&sA)[9][9], const double (&sV)[9][9], bool live, bool bad, double (&out)[9]) {
        double e[9], F[9], sig[3], ev[2];
        bool ok = live && !bad;
        if (ok) ok = fund_from_moments(sA, sV, e, ev, F, sig);
        hom_write(F, ok, 0, out);
    }
};

// match i of the segment as the passes see it: from the staged copy, or through epi_load (staged is workgroup-uniform)
__device__ __forceinline__ void polish_fetch(bool staged, const float4* __restrict__ stage, const float2* __restrict__ ml,
                                             const float2* __restrict__ mr, const float* __restrict__ conf, uint32_t i, uint32_t n,
                                             bool has_norm, const EpiNorm& nm, bool gate, float min_conf, float& l0, float& l1, float& r0,
                                             float& r1) {
    if (staged) {
        l0 = __builtin_nanf("");
        l1 = r0 = r1 = 0.0f;
        if (i < n) {                                    // n <= the slots the launch allocated
            const float4 q = stage[i];
            l0 = q.x; l1 = q.y; r0 = q.z; r1 = q.w;
        }
    } else {
        epi_load(ml, mr, conf, i, n, has_norm, nm, gate, min_conf, l0, l1, r0, r1);
    }
}

// stage_n = the slots of dynamic LDS the launch allocated: min(longest possible segment, POLISH_STAGE)
template <class T>
__global__ void __launch_bounds__(POLISH_THREADS)
verify_polish_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const float* __restrict__ conf_,
                     const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                     const float* __restrict__ thr, const float* __restrict__ norm, int gate, float min_conf,
                     const float* __restrict__ models, int H, const int32_t* __restrict__ best, int rounds, int stage_n,
                     float* __restrict__ model_out, int64_t* __restrict__ best_count, uint8_t* __restrict__ inlier,
                     double* __restrict__ moments, int32_t* __restrict__ best_round, int32_t* __restrict__ counts_out) {
    extern __shared__ __attribute__((aligned(16))) float4 polish_stage[];
    __shared__ double sA[9][9], sV[9][9];
    __shared__ double part[POLISH_WAVES][EPI_MOM];
    __shared__ double s_mom_best[EPI_MOM];
    __shared__ float s_model[9], s_model_best[9];
    __shared__ int s_wcnt[POLISH_WAVES];
    __shared__ int s_bad, s_rot, s_same;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    const float t = thr[p];
    const bool live_t = t >= 0.0f;                      // NaN or negative threshold: no match is an inlier of any model
    const float t2 = t * t;
    const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
    const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
    const float* conf = conf_ ? conf_ + lo : nullptr;
    const EpiNorm nm = epi_norm(norm, p);
    const bool staged = n <= (uint32_t)stage_n;         // workgroup-uniform

    // ---- stage, and round 0's model -----------------------------------------------------------------------------------------
    if (staged) {
        for (uint32_t i = tid; i < n; i += POLISH_THREADS) {            // at most POLISH_STAGE / POLISH_THREADS trips
            float l0, l1, r0, r1;
            epi_load(ml, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, l0, l1, r0, r1);
            polish_stage[i] = float4{l0, l1, r0, r1};
        }
    }
    if (tid < 9) s_model[tid] = epi_winner(models, H, best ? best[p] : 0, p)[tid];     // a null best: H == 1
    wg_barrier();

    int best_c = -1, best_r = 0;                        // workgroup-uniform: every thread computes every count
#pragma unroll 1
    for (int r = 0; r <= POLISH_MAX_ROUNDS; ++r) {
        // ---- support(m_r): one pass -----------------------------------------------------------------------------------------
        float e[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = s_model[k];
        const float mine_m = tid < 9 ? s_model[tid] : 0.0f;
        double acc[EPI_MOM];
#pragma unroll
        for (int k = 0; k < EPI_MOM; ++k) acc[k] = 0.0;
        int wcnt = 0;
        if (live_t) {                                   // workgroup-uniform
            for (uint32_t i0 = 0; i0 < n; i0 += POLISH_THREADS) {
                float xl0, xl1, xr0, xr1;
                polish_fetch(staged, polish_stage, ml, mr, conf, i0 + tid, n, norm != nullptr, nm, gate != 0, min_conf, xl0, xl1, xr0, xr1);
                v2f s, lim, w;
                T::test2(e, t2, pk_splat(xl0), pk_splat(xl1), pk_splat(xr0), pk_splat(xr1), s, lim, w);
                const bool in0 = w.x > 0.0f && s.x <= lim.x;
                wcnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in0));
                if (in0) T::accumulate(xl0, xl1, xr0, xr1, acc);
            }
        }
        if (lane == 0) s_wcnt[wave] = wcnt;
        if (tid == 0) { s_bad = 0; s_rot = 0; s_same = 0; }
        const double ms = verify_moments_sum(acc, part, tid, lane, wave);   // one barrier inside
        if (tid < EPI_MOM) {                            // the moments where the Jacobi wants them
            int u, v;
            verify_triangle(tid, u, v);
            sA[u][v] = ms;
            sA[v][u] = ms;
            if (!__builtin_isfinite(ms)) s_bad = 1;     // the same value from every writer
        }
        if (tid < 81) {
            const int i = tid / 9, j = tid - 9 * i;
            sV[i][j] = i == j ? 1.0 : 0.0;
        }
        int c = 0;
#pragma unroll
        for (int w = 0; w < POLISH_WAVES; ++w) c += s_wcnt[w];
        if (tid == 0) counts_out[p * (rounds + 1) + r] = c;
        if (c > best_c) {                               // the lowest round with the largest count
            best_c = c; best_r = r;
            if (tid < EPI_MOM) s_mom_best[tid] = ms;
            if (tid < 9) s_model_best[tid] = mine_m;
        }
        wg_barrier();
        if (r >= rounds) break;

        // ---- m_{r+1} = refit(M_r, c_r) --------------------------------------------------------------------------------------
        const bool live = c >= PolishRefit<T>::MIN_INLIERS;             // workgroup-uniform
        if (live) jacobi9_sweeps(sA, sV, s_rot, tid, tid < 64 && (tid & 15) < 9, s_bad != 0, PolishRefit<T>::SWEEPS);
        if (tid == 0) {
            double m[9];
            PolishRefit<T>::refit(sA, sV, live, s_bad != 0, m);
            bool same = true;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float f = (float)m[k];
                same = same && __float_as_uint(f) == __float_as_uint(s_model[k]);
                s_model[k] = f;
            }
            if (same) {                                 // every later round repeats this one
                s_same = 1;
                for (int q = r + 1; q <= rounds && q <= POLISH_MAX_ROUNDS; ++q) counts_out[p * (rounds + 1) + q] = c;
            }
        }
        wg_barrier();
        if (s_same != 0) break;
    }
    wg_barrier();                                       // the best model and moments are in LDS

    // ---- outputs, and the best round's mask ----------------------------------------------------------------------------------
    if (tid < EPI_MOM) {
        int u, v;
        verify_triangle(tid, u, v);
        const double ms = s_mom_best[tid];
        double* mo = moments + p * 81;
        mo[u * 9 + v] = ms;
        mo[v * 9 + u] = ms;
    }
    if (tid < 9) model_out[p * 9 + tid] = s_model_best[tid];
    if (tid == 0) { best_count[p] = (int64_t)best_c; best_round[p] = best_r; }
    if (!live_t || best_c <= 0) return;                 // the mask was zeroed before the launch
    float e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = s_model_best[k];
    for (uint32_t i0 = 0; i0 < n; i0 += POLISH_THREADS) {
        const uint32_t i = i0 + tid;
        float xl0, xl1, xr0, xr1;
        polish_fetch(staged, polish_stage, ml, mr, conf, i, n, norm != nullptr, nm, gate != 0, min_conf, xl0, xl1, xr0, xr1);
        v2f s, lim, w;
        T::test2(e, t2, pk_splat(xl0), pk_splat(xl1), pk_splat(xr0), pk_splat(xr1), s, lim, w);
        if (i < n) inlier[lo + i] = w.x > 0.0f && s.x <= lim.x ? 1 : 0;
    }
}

}  // namespace pats

using namespace pats;

// family T's entry point; `who` = its name.  No workspace: a pair's walk lives in its workgroup's LDS and registers
template <class T>
static int verify_polish_by_pair(const char* who, const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                 int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr, const float* norm,
                                 int use_min_conf, float min_conf, const float* models, int64_t H, const int32_t* best, int rounds,
                                 float* model, int64_t* best_count, uint8_t* inlier, double* moments, int32_t* best_round, int32_t* counts,
                                 pats_stream_t stream) {
    int rc = epi_check_scored(who, {"matches_l", matches_l, 8}, matches_r, models, thr,
                              {{"model", model, 4}, {"best_count", best_count, 8}, {"inlier", inlier, 1}, {"moments", moments, 8},
                               {"best_round", best_round, 4}, {"counts", counts, 4}},
                              conf, norm, pair_off, stride, counts_in, pairs, cap, H, use_min_conf, min_conf, {"best", best, 4});
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(rounds >= 1 && rounds <= POLISH_MAX_ROUNDS, "%s: rounds = %d (1 .. %d)", who, rounds, POLISH_MAX_ROUNDS);
    PATS_REQUIRE(best || H == 1, "%s: null best needs H == 1, got H = %lld", who, (long long)H);
    const int64_t longest = counts_in ? stride : cap;   // the staging comes from the sizes alone: no host read of the counts
    const int stage_n = (int)(longest < POLISH_STAGE ? longest : POLISH_STAGE);
    static DeviceGrants grants;                         // (one per T) the staging can exceed what a launch gets unasked
    if (!grants.get({{(const void*)verify_polish_kernel<T>, POLISH_LDS}}).granted) {
        set_error("%s: the device refused %d bytes of dynamic LDS per workgroup", who, POLISH_LDS);
        return PATS_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    rc = fill_bytes(inlier, 0, (size_t)cap, st);
    if (rc != PATS_OK) return rc;
    hipLaunchKernelGGL(verify_polish_kernel<T>, dim3((unsigned)pairs), dim3(POLISH_THREADS), (size_t)stage_n * sizeof(float4), st, matches_l,
                       matches_r, use_min_conf ? conf : nullptr, pair_off, counts_in, stride, cap, thr, norm, use_min_conf, min_conf, models,
                       (int)H, best, rounds, stage_n, model, best_count, inlier, moments, best_round, counts);
    return check_launch(T::POLISH);
}

// ---- the entry points (include/pats_amd.h) ---------------------------------------------------------------------------------------
extern "C" size_t pats_epipolar_polish_workspace_bytes(int64_t, int64_t, int64_t) { return 0; }
extern "C" size_t pats_homography_polish_workspace_bytes(int64_t, int64_t, int64_t) { return 0; }
extern "C" size_t pats_fundamental_polish_workspace_bytes(int64_t, int64_t, int64_t) { return 0; }

extern "C" int pats_epipolar_polish_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr,
                                                const float* norm, int use_min_conf, float min_conf, const float* models, int64_t H,
                                                const int32_t* best, int rounds, float* model, int64_t* best_count, uint8_t* inlier,
                                                double* moments, int32_t* best_round, int32_t* counts, void*, size_t, pats_stream_t stream) {
    return verify_polish_by_pair<Epipolar>("epipolar_polish_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in, pairs, cap, thr,
                                           norm, use_min_conf, min_conf, models, H, best, rounds, model, best_count, inlier, moments, best_round,
                                           counts, stream);
}

extern "C" int pats_homography_polish_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                  int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr,
                                                  const float* norm, int use_min_conf, float min_conf, const float* models, int64_t H,
                                                  const int32_t* best, int rounds, float* model, int64_t* best_count, uint8_t* inlier,
                                                  double* moments, int32_t* best_round, int32_t* counts, void*, size_t, pats_stream_t stream) {
    return verify_polish_by_pair<Homography>("homography_polish_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in, pairs, cap,
                                             thr, norm, use_min_conf, min_conf, models, H, best, rounds, model, best_count, inlier, moments,
                                             best_round, counts, stream);
}

extern "C" int pats_fundamental_polish_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                                   int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr,
                                                   const float* norm, int use_min_conf, float min_conf, const float* models, int64_t H,
                                                   const int32_t* best, int rounds, float* model, int64_t* best_count, uint8_t* inlier,
                                                   double* moments, int32_t* best_round, int32_t* counts, void*, size_t, pats_stream_t stream) {
    return verify_polish_by_pair<Fundamental>("fundamental_polish_by_pair", matches_l, matches_r, conf, pair_off, stride, counts_in, pairs, cap,
                                              thr, norm, use_min_conf, min_conf, models, H, best, rounds, model, best_count, inlier, moments,
                                              best_round, counts, stream);
}
