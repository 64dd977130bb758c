// Per-pair pose error and its AUC: what the reference's evaluation does with a pose (utils/metrics.py: angle_error_mat,
// angle_error_vec with the 180-degree fold, error_auc), on the device, no host read.  include/pats_amd.h states both definitions;
// docs/kernels.md 4.9.2 the design.
//
//   pose_error_kernel   one THREAD per pair, PERR_THREADS per workgroup: 33 float64 loads, two acos, four stores.  The stage is
//                       bound by its launch; nothing crosses threads.  Unlike every other stage +inf is a VALUE here - the
//                       reference's error of a pair it cannot score - and a NaN never is
//   pose_auc_kernel     ONE workgroup of AUC_THREADS threads: the errors go to LDS as order-preserving 64-bit keys (a NaN as +inf's),
//                       padded to the next power of two with the largest key and sorted ascending by a bitonic network (equal keys
//                       are equal values: any network gives the same list); a thread per threshold finds k by bisection; the
//                       trapezoids are added per thread with a stride of AUC_THREADS, the lanes of a wave by wave_sum_tree_f64
//                       (epipolar.hpp), the waves in index order by the threshold's thread: the order depends on n alone, no
//                       atomics.  Dynamic LDS: 8 bytes per slot, 128 KiB at AUC_MAX_N
#include "common.hpp"
#include "epipolar.hpp"
#include "gt_pose.hpp"

namespace pats {

constexpr int PERR_THREADS = 64;                       // pairs per workgroup (one wave)
constexpr int AUC_THREADS = 1024;
constexpr int AUC_WAVES = AUC_THREADS / WAVE;
constexpr int AUC_MAX_N = 16384;                       // = pats_pose_auc_max_n(): 128 KiB of the CU's 160
constexpr int AUC_MAX_THR = 8;
constexpr int AUC_LDS = AUC_MAX_N * (int)sizeof(unsigned long long);
constexpr double DEG_PER_RAD = 57.29577951308232;      // 180 / pi rounded to float64
constexpr double PERR_INF = __builtin_huge_val();

// acos(clip(c)) in degrees; a NaN c stays a NaN (both comparisons are false)
__device__ __forceinline__ double perr_angle(double c) {
    c = c < -1.0 ? -1.0 : c;
    c = c > 1.0 ? 1.0 : c;
    return acos(c) * DEG_PER_RAD;
}

__global__ void __launch_bounds__(PERR_THREADS)
pose_error_kernel(const double* __restrict__ R_in, const double* __restrict__ t_in, const double* __restrict__ T1, const double* __restrict__ T0,
                  const int64_t* __restrict__ counts, int64_t pairs, int64_t min_matches, double min_gt_t, double* __restrict__ err_R,
                  double* __restrict__ err_t, double* __restrict__ err, int32_t* __restrict__ status) {
    const int64_t p = (int64_t)blockIdx.x * PERR_THREADS + threadIdx.x;
    if (p >= pairs) return;
    double R[9], t[3];
    bool pose_ok = true, moves = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) { R[k] = R_in[p * 9 + k]; pose_ok = pose_ok && __builtin_isfinite(R[k]); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { t[k] = t_in[p * 3 + k]; pose_ok = pose_ok && __builtin_isfinite(t[k]); moves = moves || t[k] != 0.0; }
    double G[9], g[3];
    const bool gt_ok = gt_relative_pose(T1, T0, p, G, g);           // gt_pose.hpp: R_gt = R1 R0^T, t_gt = t1 - R_gt t0
    int st = 0;
    if (counts != nullptr && counts[p] < min_matches) st = 1;
    else if (!pose_ok || !moves) st = 2;
    else if (!gt_ok) st = 3;
    double eR = PERR_INF, eT = PERR_INF;
    if (st == 0) {
        double s = R[0] * G[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) s = s + R[k] * G[k];
        eR = perr_angle((s - 1.0) / 2.0);
        const double ng = __builtin_sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        if (ng <= min_gt_t) {
            eT = 0.0;                                   // the direction of t_gt carries no information
        } else {
            const double d = (t[0] * g[0] + t[1] * g[1]) + t[2] * g[2];
            const double nt = __builtin_sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
            const double e = perr_angle(d / (nt * ng)), f = 180.0 - e;
            eT = f < e ? f : e;                         // a NaN e: both NaN, eT = NaN, +inf below
        }
        if (eR != eR) eR = PERR_INF;
        if (eT != eT) eT = PERR_INF;
    }
    err_R[p] = eR;
    err_t[p] = eT;
    err[p] = eR > eT ? eR : eT;
    status[p] = st;
}

// the order-preserving image of a float64; a NaN of either sign is +inf, -0.0 is +0.0 (equal keys must be equal values)
__host__ __device__ __forceinline__ unsigned long long auc_key(double v) {
    if (v != v) v = __builtin_huge_val();
    if (v == 0.0) v = 0.0;
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}
__device__ __forceinline__ double auc_value(unsigned long long k) {
    return __builtin_bit_cast(double, k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull));
}

struct AucArgs {
    const double* errors; int n; int S; int n_thr;     // S = the power of two >= max(n, 1): the slots of dynamic LDS
    double thr[AUC_MAX_THR];
    double* auc; int64_t* below; double* sorted;
};

__global__ void __launch_bounds__(AUC_THREADS) pose_auc_kernel(AucArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long auc_keys[];
    __shared__ double s_part[AUC_WAVES][AUC_MAX_THR];
    __shared__ int s_k[AUC_MAX_THR];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = g.n, S = g.S;
    if (n == 0) {                                       // workgroup-uniform
        if (tid < g.n_thr) { g.auc[tid] = 0.0; g.below[tid] = 0; }
        return;
    }
    for (int i = tid; i < S; i += AUC_THREADS) auc_keys[i] = i < n ? auc_key(g.errors[i]) : 0xFFFFFFFFFFFFFFFFull;
    wg_barrier();

    // ---- sort, ascending ---------------------------------------------------------------------------------------------------------
    for (int size = 2; size <= S; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int c = tid; c < (S >> 1); c += AUC_THREADS) {
                const int a = ((c & ~(stride - 1)) << 1) | (c & (stride - 1)), b = a | stride;
                const unsigned long long x = auc_keys[a], y = auc_keys[b];
                const bool asc = (a & size) == 0;
                if (asc ? x > y : x < y) { auc_keys[a] = y; auc_keys[b] = x; }
            }
            wg_barrier();
        }
    }
    if (g.sorted != nullptr) {
        for (int i = tid; i < n; i += AUC_THREADS) g.sorted[i] = auc_value(auc_keys[i]);
    }

    // ---- k per threshold: the number of errors strictly below it (bisection over the sorted keys) ----------------------------------
    if (tid < g.n_thr) {
        const unsigned long long kt = auc_key(g.thr[tid]);
        int lo = 0, hi = n;                             // keys[0 .. lo) < kt <= keys[hi .. n)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (auc_keys[mid] < kt) lo = mid + 1; else hi = mid;
        }
        s_k[tid] = lo;
    }
    wg_barrier();

    // ---- the trapezoids: x_0 = 0, x_i = e_(i), y_i = i * (1 / n); term i = ((x_{i+1} - x_i) * (y_i + y_{i+1})) * 0.5, i < k ---------
    const double inv = 1.0 / (double)n;
    for (int j = 0; j < g.n_thr; ++j) {
        const int k = s_k[j];
        double sum = 0.0;
        for (int i = tid; i < k; i += AUC_THREADS) {
            const double x0 = i == 0 ? 0.0 : auc_value(auc_keys[i - 1]), x1 = auc_value(auc_keys[i]);
            sum += ((x1 - x0) * ((double)i * inv + (double)(i + 1) * inv)) * 0.5;
        }
        sum = wave_sum_tree_f64(sum);
        if (lane == 0) s_part[wave][j] = sum;
    }
    wg_barrier();
    if (tid < g.n_thr) {
        const int k = s_k[tid];
        double area = wave_parts_total(s_part, tid);
        const double xk = k == 0 ? 0.0 : auc_value(auc_keys[k - 1]);
        area += (g.thr[tid] - xk) * ((double)k * inv);
        g.auc[tid] = area / g.thr[tid];
        g.below[tid] = (int64_t)k;
    }
}

}  // namespace pats

using namespace pats;

extern "C" int pats_pose_error_by_pair_f64(const double* R, const double* t, const double* T1, const double* T0, const int64_t* counts,
                                           int64_t pairs, int64_t min_matches, double min_gt_t, double* err_R, double* err_t, double* err,
                                           int32_t* status, pats_stream_t stream) {
    const char* who = "pose_error_by_pair";
    int rc = epi_check_args(who, {{"R", R, 8}, {"t", t, 8}, {"T1", T1, 8}, {"err_R", err_R, 8}, {"err_t", err_t, 8}, {"err", err, 8},
                                  {"status", status, 4}}, true);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_args(who, {{"T0", T0, 8}, {"counts", counts, 8}}, false)) != PATS_OK) return rc;
    PATS_REQUIRE(pairs >= 1 && pairs <= 0x7fffffff, "%s: pairs = %lld (1 .. 2^31 - 1)", who, (long long)pairs);
    PATS_REQUIRE(min_matches >= 0, "%s: min_matches = %lld must not be negative", who, (long long)min_matches);
    PATS_REQUIRE(min_gt_t >= 0.0, "%s: min_gt_t = %g must be a non-negative number", who, min_gt_t);                   // false for a NaN
    hipLaunchKernelGGL(pose_error_kernel, dim3((unsigned)ceil_div(pairs, PERR_THREADS)), dim3(PERR_THREADS), 0, as_stream(stream), R, t, T1,
                       T0, counts, pairs, min_matches, min_gt_t, err_R, err_t, err, status);
    return check_launch("pose_error kernel");
}

extern "C" int64_t pats_pose_auc_max_n(void) { return AUC_MAX_N; }

extern "C" int pats_pose_auc_f64(const double* errors, int64_t n, const double* thresholds, int64_t n_thr, double* auc, int64_t* below,
                                 double* sorted, pats_stream_t stream) {
    int rc = epi_check_args("pose_auc", {{"errors", errors, 8}, {"thresholds", thresholds, 1}, {"auc", auc, 8}, {"below", below, 8}}, true);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_arg("pose_auc", {"sorted", sorted, 8}, false)) != PATS_OK) return rc;
    PATS_REQUIRE(n >= 0 && n <= AUC_MAX_N, "pose_auc: n = %lld (0 .. max_n = %d)", (long long)n, AUC_MAX_N);
    PATS_REQUIRE(n_thr >= 1 && n_thr <= AUC_MAX_THR, "pose_auc: n_thr = %lld (1 .. %d)", (long long)n_thr, AUC_MAX_THR);
    AucArgs g{};
    for (int64_t j = 0; j < n_thr; ++j) {
        const double v = thresholds[j];
        PATS_REQUIRE(v > 0.0 && v <= 1.7976931348623157e308, "pose_auc: thresholds[%lld] = %g must be finite and positive", (long long)j, v);
        g.thr[j] = v;
    }
    int S = 1;
    while (S < (int)n) S <<= 1;
    g.errors = errors; g.n = (int)n; g.S = S; g.n_thr = (int)n_thr;
    g.auc = auc; g.below = below; g.sorted = sorted;
    const size_t lds = (size_t)S * sizeof(unsigned long long);
    // the keys (plus the kernel's static LDS) can exceed the 64 KiB a launch gets unasked.  Asked for at every n, as polish.hip
    // does: static + dynamic LDS passes 64 KiB from n = 4097 on
    static DeviceGrants grants;
    if (!grants.get({{(const void*)pose_auc_kernel, AUC_LDS}}).granted) {
        set_error("pose_auc: the device refused %d bytes of dynamic LDS per workgroup", AUC_LDS);
        return PATS_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(pose_auc_kernel, dim3(1), dim3(AUC_THREADS), lds, as_stream(stream), g);
    return check_launch("pose_auc kernel");
}
