// Per-pair triangulation: for every pair of a batch the 3-D point of each masked match under the pair's pose - the midpoint of the
// common perpendicular of the two rays, the two depths, the squared reprojection error and the cosine of the triangulation angle -
// with the per-pair count of valid points and the sum of their errors.  One launch (after the fills of the per-match outputs), no
// host read.  include/pats_amd.h states the definition; docs/kernels.md 4.9.1 the design.
//
//   one workgroup per pair, TRI_THREADS = 256 threads, decided by the sizes alone (the pose's vote walk)
//   pose    twelve threads bring R_p, t_p (the pose in the frame of the points: hom_perm, frame_perm) to LDS in float64 and judge
//           it: a non-finite entry or t = 0 leaves the pair without a valid match
//   walk    the workgroup walks the segment with epi_load_masked.  tri_match is the whole definition of one match, float64, no
//           contraction.  Only valid rows are stored: the fills defined everything else
//   count   the count fold of epipolar.hpp
//   sum     a thread adds the e2 of its valid matches in walk order, the lanes of a wave by wave_sum_tree_f64, thread 0 adds the
//           waves in index order: the order depends on the sizes alone, no atomics
#include "common.hpp"
#include "epipolar.hpp"

namespace pats {

constexpr int TRI_THREADS = 256;
constexpr int TRI_WAVES = TRI_THREADS / WAVE;

struct TriMatch {
    double X[3], lambda, mu, e2, cosp;
    bool valid;
};

__device__ __forceinline__ bool tri_fits_f32(double v) { return __builtin_fabs(v) <= 3.4028234663852886e38; }     // FLT_MAX; false for a NaN

// THE definition of one match (include/pats_amd.h, "Per-pair triangulation").  A NaN l0 (a match that is not used) is not valid.
// lim_r2 = max_reproj^2 and lim_cos in float64; has_* says whether the limit applies (a NaN limit fails its comparison).
__device__ __forceinline__ TriMatch tri_match(const double (&R)[9], const double (&t)[3], float l0f, float l1f, float r0f, float r1f,
                                              bool has_r, double lim_r2, bool has_c, double lim_cos) {
    const double l0 = (double)l0f, l1 = (double)l1f, r0 = (double)r0f, r1 = (double)r1f;
    TriMatch m;
    const double a0 = (R[0] * l0 + R[1] * l1) + R[2], a1 = (R[3] * l0 + R[4] * l1) + R[5], a2 = (R[6] * l0 + R[7] * l1) + R[8];
    const double c0 = a1 - a2 * r1, c1 = a2 * r0 - a0, c2 = a0 * r1 - a1 * r0;                               // a x b, b = (r0, r1, 1)
    const double bt0 = r1 * t[2] - t[1], bt1 = t[0] - r0 * t[2], bt2 = r0 * t[1] - r1 * t[0];                 // b x t
    const double at0 = a1 * t[2] - a2 * t[1], at1 = a2 * t[0] - a0 * t[2], at2 = a0 * t[1] - a1 * t[0];       // a x t
    const double cc = (c0 * c0 + c1 * c1) + c2 * c2;
    const double dl = (c0 * bt0 + c1 * bt1) + c2 * bt2, dr = (c0 * at0 + c1 * at1) + c2 * at2;
    m.lambda = dl / cc;
    m.mu = dr / cc;
    // the midpoint in the right camera's frame, then with the translation taken off: X_r - t = (lambda a + t + mu b) / 2 - t
    const double q0 = ((m.lambda * a0 + t[0]) + m.mu * r0) * 0.5 - t[0], q1 = ((m.lambda * a1 + t[1]) + m.mu * r1) * 0.5 - t[1],
                 q2 = ((m.lambda * a2 + t[2]) + m.mu) * 0.5 - t[2];
    m.X[0] = (R[0] * q0 + R[3] * q1) + R[6] * q2;                                                             // R^T q
    m.X[1] = (R[1] * q0 + R[4] * q1) + R[7] * q2;
    m.X[2] = (R[2] * q0 + R[5] * q1) + R[8] * q2;
    const double Y0 = ((R[0] * m.X[0] + R[1] * m.X[1]) + R[2] * m.X[2]) + t[0], Y1 = ((R[3] * m.X[0] + R[4] * m.X[1]) + R[5] * m.X[2]) + t[1],
                 Y2 = ((R[6] * m.X[0] + R[7] * m.X[1]) + R[8] * m.X[2]) + t[2];
    const double dl0 = m.X[0] / m.X[2] - l0, dl1 = m.X[1] / m.X[2] - l1, dr0 = Y0 / Y2 - r0, dr1 = Y1 / Y2 - r1;
    m.e2 = (dl0 * dl0 + dl1 * dl1) + (dr0 * dr0 + dr1 * dr1);
    const double ab = (a0 * r0 + a1 * r1) + a2, aa = (a0 * a0 + a1 * a1) + a2 * a2, bb = (r0 * r0 + r1 * r1) + 1.0;
    m.cosp = ab / (__builtin_sqrt(aa) * __builtin_sqrt(bb));
    bool ok = cc > 0.0 && m.lambda > 0.0 && m.mu > 0.0 && m.X[2] > 0.0 && Y2 > 0.0;                           // false for a NaN l0
    ok = ok && __builtin_isfinite(Y0) && __builtin_isfinite(Y1) && __builtin_isfinite(Y2);
    ok = ok && tri_fits_f32(m.X[0]) && tri_fits_f32(m.X[1]) && tri_fits_f32(m.X[2]) && tri_fits_f32(m.lambda) && tri_fits_f32(m.mu) &&
         tri_fits_f32(m.e2) && tri_fits_f32(m.cosp);
    if (has_r) ok = ok && m.e2 <= lim_r2;
    if (has_c) ok = ok && m.cosp <= lim_cos;
    m.valid = ok;
    return m;
}

__global__ void __launch_bounds__(TRI_THREADS)
epipolar_triangulate_kernel(const float* __restrict__ ml_, const float* __restrict__ mr_, const uint8_t* __restrict__ mask,
                            const int64_t* __restrict__ pair_off, const int64_t* __restrict__ counts_in, int64_t stride, int64_t cap,
                            const float* __restrict__ norm, const double* __restrict__ R_in, const double* __restrict__ t_in, int swapped,
                            const float* __restrict__ max_reproj, const float* __restrict__ max_cos, float* __restrict__ points,
                            float* __restrict__ depths, float* __restrict__ reproj, float* __restrict__ cos_parallax,
                            uint8_t* __restrict__ valid, int64_t* __restrict__ tri_count, double* __restrict__ reproj_sum) {
    __shared__ double sR[9], sT[3];
    __shared__ double s_sum[TRI_WAVES];
    __shared__ int s_cnt[TRI_WAVES];
    __shared__ int s_bad, s_moves;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t lo;
    uint32_t n;
    epi_segment(pair_off, counts_in, stride, cap, p, lo, n);
    if (tid == 0) { s_bad = 0; s_moves = 0; }
    wg_barrier();

    // ---- pose -------------------------------------------------------------------------------------------------------------------
    if (tid < 9) {                                      // R_p = P R P, t_p = P t for swapped
        const double v = R_in[p * 9 + hom_perm(tid, swapped)];
        sR[tid] = v;
        if (!__builtin_isfinite(v)) s_bad = 1;          // the same value from every writer
    } else if (tid < 12) {
        const int i = tid - 9;
        const double v = t_in[p * 3 + frame_perm(i, swapped)];
        sT[i] = v;
        if (!__builtin_isfinite(v)) s_bad = 1;
        if (v != 0.0) s_moves = 1;
    }
    wg_barrier();
    const bool ok = s_bad == 0 && s_moves != 0;         // workgroup-uniform; t = 0 is pose_by_pair's "no pose"

    // ---- walk -------------------------------------------------------------------------------------------------------------------
    int cnt = 0;
    double sum = 0.0;
    if (ok) {
        const float2* ml = reinterpret_cast<const float2*>(ml_) + lo;
        const float2* mr = reinterpret_cast<const float2*>(mr_) + lo;
        const uint8_t* msk = mask + lo;
        const EpiNorm nm = epi_norm(norm, p);
        double R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = sR[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = sT[k];
        const bool has_r = max_reproj != nullptr, has_c = max_cos != nullptr;
        const double lr = has_r ? (double)max_reproj[p] : 0.0, lim_r2 = lr * lr, lim_cos = has_c ? (double)max_cos[p] : 0.0;
        for (uint32_t i0 = 0; i0 < n; i0 += TRI_THREADS) {
            const uint32_t i = i0 + tid;
            float l0, l1, r0, r1;
            epi_load_masked(ml, mr, msk, i, n, norm != nullptr, nm, l0, l1, r0, r1);
            const TriMatch m = tri_match(R, t, l0, l1, r0, r1, has_r, lim_r2, has_c, lim_cos);
            cnt += wave_count(m.valid);
            if (m.valid) {                              // i < n: a row past the segment carries the NaN l0
                const int64_t row = lo + i;
                sum += m.e2;
                // with swapped the point goes out in the reference's frame: P X
                points[row * 3 + 0] = (float)(swapped ? m.X[1] : m.X[0]);
                points[row * 3 + 1] = (float)(swapped ? m.X[0] : m.X[1]);
                points[row * 3 + 2] = (float)m.X[2];
                if (depths) { depths[row * 2 + 0] = (float)m.lambda; depths[row * 2 + 1] = (float)m.mu; }
                if (reproj) reproj[row] = (float)m.e2;
                if (cos_parallax) cos_parallax[row] = (float)m.cosp;
                valid[row] = (uint8_t)1;
            }
        }
        sum = wave_sum_tree_f64(sum);
    }
    wave_parts_store(s_cnt, wave, lane, cnt);
    wave_parts_store(s_sum, wave, lane, sum);
    wg_barrier();
    if (tid == 0) {
        tri_count[p] = (int64_t)wave_parts_total(s_cnt);
        reproj_sum[p] = wave_parts_total(s_sum);
    }
}

}  // namespace pats

using namespace pats;

extern "C" size_t pats_epipolar_triangulate_workspace_bytes(int64_t pairs, int64_t cap) {
    (void)pairs; (void)cap;
    return 0;                                           // the pose lives in LDS, the partial sums too
}

extern "C" int pats_epipolar_triangulate_by_pair_f64(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                                     const int64_t* counts_in, int64_t pairs, int64_t cap, const uint8_t* mask,
                                                     const float* norm, const double* R, const double* t, int swapped,
                                                     const float* max_reproj, const float* max_cos, float* points, float* depths,
                                                     float* reproj, float* cos_parallax, uint8_t* valid, int64_t* tri_count,
                                                     double* reproj_sum, void* workspace, size_t workspace_bytes, pats_stream_t stream) {
    (void)workspace;
    const char* who = "epipolar_triangulate_by_pair";
    int rc = epi_check_args(who, {{"matches_l", matches_l, 8}, {"matches_r", matches_r, 8}, {"mask", mask, 1}, {"R", R, 8}, {"t", t, 8},
                                  {"points", points, 4}, {"valid", valid, 1}, {"tri_count", tri_count, 8}, {"reproj_sum", reproj_sum, 8}}, true);
    if (rc != PATS_OK) return rc;
    rc = epi_check_args(who, {{"norm", norm, 4}, {"max_reproj", max_reproj, 4}, {"max_cos", max_cos, 4}, {"depths", depths, 4},
                              {"reproj", reproj, 4}, {"cos_parallax", cos_parallax, 4}, {"pair_off", pair_off, 8}, {"counts_in", counts_in, 8}},
                        false);
    if (rc != PATS_OK) return rc;
    if ((rc = epi_check_segments(who, pair_off, counts_in, stride, pairs, cap)) != PATS_OK) return rc;
    PATS_REQUIRE(swapped == 0 || swapped == 1, "%s: swapped = %d must be 0 or 1", who, swapped);
    PATS_REQUIRE(workspace_bytes >= pats_epipolar_triangulate_workspace_bytes(pairs, cap), "%s: workspace too small", who);
    hipStream_t st = as_stream(stream);
    // every byte of every per-match output is defined: zeros here, the kernel stores the valid rows
    if ((rc = fill_bytes(points, 0, (size_t)cap * 3 * sizeof(float), st)) != PATS_OK) return rc;
    if ((rc = fill_bytes(valid, 0, (size_t)cap, st)) != PATS_OK) return rc;
    if (depths && (rc = fill_bytes(depths, 0, (size_t)cap * 2 * sizeof(float), st)) != PATS_OK) return rc;
    if (reproj && (rc = fill_bytes(reproj, 0, (size_t)cap * sizeof(float), st)) != PATS_OK) return rc;
    if (cos_parallax && (rc = fill_bytes(cos_parallax, 0, (size_t)cap * sizeof(float), st)) != PATS_OK) return rc;
    hipLaunchKernelGGL(epipolar_triangulate_kernel, dim3((unsigned)pairs), dim3(TRI_THREADS), 0, st, matches_l, matches_r, mask, pair_off,
                       counts_in, stride, cap, norm, R, t, swapped, max_reproj, max_cos, points, depths, reproj, cos_parallax, valid,
                       tri_count, reproj_sum);
    return check_launch("epipolar_triangulate kernel");
}
