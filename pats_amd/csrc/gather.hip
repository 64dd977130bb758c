// Descriptor gathers feeding the fine / third-level cost builds, for PATS on gfx950.
//
//   fine level   SecondLayer.forward, models/second_layer.py:71-86: AvgPool2d(2,1,1) on the two
//                high-resolution maps, sample the 12x12 grid at ((pos + 0.5) * stride) for strides
//                4, 2, 1, concat 64 + 64 + 128 channels, prepend the 8-channel "title", append the
//                dustbin feature column  ->  desc [2, B, 264, 145]
//   third level  ThirdLayer.forward, models/third_layer.py:121-146: round the coarse points to the
//                4-px lattice, gather the 8x8 window of the padded 52x52 half-resolution map around
//                each point in both crops, add the keypoint encoding, append the dustbin feature
//                -> feat_unfold [P, 128, 65] x 2 (the layout the MFMA cost build consumes)
//
// Both are pure index arithmetic + copies (HBM-bound on the output write).  Output rows are written
// by consecutive lanes; source windows are short contiguous runs of a feature-map row (L2-resident).
#include "common.hpp"

#include <cstdlib>
#include <type_traits>

namespace pats {

// Cache policy of the gathers' accesses (round 4).  tools/granule_probe.hip -> profiles/r04_granule_probe.txt: the memory side always
// moves whole 128-byte lines (32 bytes of every 128 cost what the whole line costs: the NCHW kernels' over-fetch is the layout's),
// and NON-TEMPORAL loads of data used once stream 9 % faster than plain ones (6.28 against 5.74 TB/s dense).  In the kernels
// (tools/gather_nt_ab.sh -> profiles/r04_gather_nt_ab.txt, inside the bench's steps): the CHANNELS-LAST kernels, whose outputs leave
// as whole lines of a linear 16-byte stream, gain 6 % / 9 % from non-temporal STORES (4.10 -> 3.85, 2.94 -> 2.67 ms; non-temporal
// loads alone change nothing there); the NCHW kernels LOSE with either - their taps re-visit lines through the L1 the policy
// bypasses (6.2 -> 6.7, 4.9 -> 6.8 ms with such loads) and their 4-byte stores into rows of 145 / 65 floats end lines partially
// (-> 7.3, 8.0 ms with such stores).  POL bit 0: map reads non-temporal; bit 1: output stores non-temporal.  Defaults: 0 on NCHW
// maps, 3 on channels-last maps; PATS_GATHER_NT = 0..3 overrides both (read once per process).
template <int POL, typename T>
__device__ __forceinline__ T ldm(const T* p) {
    if (POL & 1) return __builtin_nontemporal_load(p);
    return *p;
}
template <int POL, typename T>
__device__ __forceinline__ void stm(T* p, T v) {
    if (POL & 2) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// two neighbouring floats as ONE 8-byte access at 4-byte alignment (gfx950 global memory takes unaligned dwordx2; the pooled taps of
// map 0 start at an odd element): half the load instructions of the pooling loops
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
template <int POL>
__device__ __forceinline__ f2u ldm2(const float* p) {
    const f2u* q = reinterpret_cast<const f2u*>(p);
    if (POL & 1) return __builtin_nontemporal_load(q);
    return *q;
}

// ---- map element types ---------------------------------------------------------------------------------------------------
// Every kernel takes its maps in one pats_map_dtype_t DT (include/pats_amd.h): float32, or float16 / bfloat16 from a backbone
// run in half precision, held as their raw 16 bits.  A half element is widened to fp32 EXACTLY at the load (every f16 / bf16
// value, subnormals, infinities and NaNs included, is a float); from there on every output element is formed by the same
// operations in the same order - the AvgPool2d(2,1,1) sum (((a + b) + c) + d) / 4, the kenc add, the dustbin column - so the
// outputs on half maps are the outputs on maps.float(), bit for bit, and stay float32.  Only the access shapes change with the
// element size: map 0's pooled taps become 4-byte pairs at 2-byte alignment, a third-level window row becomes 16 contiguous
// bytes (4 lanes x 2 cells instead of 8 lanes x 1 cell), and a 16-byte load of a channels-last pixel carries 8 channels
// instead of 4 (other lane -> (node, channel) maps, still whole lines per load).  Maps 4-byte aligned (NCHW) / 16-byte aligned
// (channels-last half maps; channels-last fp32: the fine level 16, the third level 4).
template <int DT> struct map_elem { using type = uint16_t; };
template <> struct map_elem<PATS_MAP_F32> { using type = float; };
template <int DT> using map_t = typename map_elem<DT>::type;

template <int DT>
__device__ __forceinline__ float widen(uint32_t h) {          // the low 16 bits of h
    if (DT == PATS_MAP_BF16) return __uint_as_float(h << 16);
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}
template <int DT>
__device__ __forceinline__ float widen_hi(uint32_t h) {       // the high 16 bits of h
    if (DT == PATS_MAP_BF16) return __uint_as_float(h & 0xffff0000u);
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(h >> 16));
}
// two neighbouring halves as ONE 4-byte access at 2-byte alignment (map 0's pooled taps start at an odd element)
typedef uint32_t u32u __attribute__((aligned(2)));
template <int POL>
__device__ __forceinline__ uint32_t ldh2(const uint16_t* p) {
    const u32u* q = reinterpret_cast<const u32u*>(p);
    if (POL & 1) return __builtin_nontemporal_load(q);
    return *q;
}
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f2s __attribute__((ext_vector_type(2), aligned(4)));
template <int POL>
__device__ __forceinline__ void stm2(float* p, f2s v) {      // two neighbouring floats as ONE 8-byte store at 4-byte alignment
    f2s* q = reinterpret_cast<f2s*>(p);
    if (POL & 2) __builtin_nontemporal_store(v, q);
    else *q = v;
}

// ---- output element types -------------------------------------------------------------------------------------------------
// Every kernel writes its descriptors in one pats_map_dtype_t OT, independent of DT and of the maps' layout: float32, or
// float16 / bfloat16 as their raw 16 bits.  The float32 value the fp32-output kernel would have stored exists in a register
// (NCHW kernels) or in the fp32 LDS tile (channels-last kernels) and is rounded ONCE, to nearest even, where it leaves - what
// tensor.to(dtype) does: fp16 overflows to inf above 65 520 and keeps its subnormals, +-0 / +-inf pass, a NaN stays a NaN.  The
// casts below are the hardware's RNE conversions (v_cvt_f16_f32 / v_cvt_pk_f16_f32, v_cvt_pk_bf16_f32), never the packed
// round-toward-zero one.  OT == PATS_MAP_F32 compiles to the code there was before the parameter existed.  Only the store
// shapes change with the element size: rows of 145 / 65 halves start at 2 mod 4 bytes on every other channel, so the NCHW
// kernels' pairs are 4-byte stores at 2-byte alignment, and the channels-last kernels' linear copies carry 8 elements per 16
// bytes (every block - 8 x 145, 64 x 145, 128 x 65 halves - is still a multiple of 16 bytes).
template <int OT> using out_t = map_t<OT>;
template <int OT>
__device__ __forceinline__ out_t<OT> narrow(float v) {
    if constexpr (OT == PATS_MAP_F32) return v;
    else if constexpr (OT == PATS_MAP_F16) return __builtin_bit_cast(uint16_t, (_Float16)v);
    else return __builtin_bit_cast(uint16_t, (__bf16)v);
}
template <int OT>
__device__ __forceinline__ uint32_t narrow2(float lo, float hi) {      // two neighbouring half outputs as one 32-bit word
    return (uint32_t)narrow<OT>(lo) | ((uint32_t)narrow<OT>(hi) << 16);
}
template <int POL>
__device__ __forceinline__ void sth2(uint16_t* p, uint32_t v) {        // ... stored as ONE 4-byte write at 2-byte alignment
    u32u* q = reinterpret_cast<u32u*>(p);
    if (POL & 2) __builtin_nontemporal_store(v, q);
    else *q = v;
}
// eight consecutive floats of a 32-byte aligned LDS tile -> eight half outputs, one 16-byte word of the linear copy
template <int OT>
__device__ __forceinline__ u4 narrow8(const float* t) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 a = *reinterpret_cast<const f4*>(t), b = *reinterpret_cast<const f4*>(t + 4);
    u4 r;
    r.x = narrow2<OT>(a.x, a.y); r.y = narrow2<OT>(a.z, a.w);
    r.z = narrow2<OT>(b.x, b.y); r.w = narrow2<OT>(b.z, b.w);
    return r;
}

// ---- fine level ------------------------------------------------------------------------------
// the AvgPool2d(2,1,1) sample over the taps q, q + 1 (one pair load) and q + row, q + row + 1             second_layer.py:73-79
template <int DT, int POL>
__device__ __forceinline__ float pooled_tap(const map_t<DT>* q, int row) {
    if constexpr (DT == PATS_MAP_F32) {
        const f2u a = ldm2<POL>(q), c2 = ldm2<POL>(q + row);
        return (((a.x + a.y) + c2.x) + c2.y) / 4.0f;
    } else {
        const uint32_t a = ldh2<POL>(q), c2 = ldh2<POL>(q + row);
        return (((widen<DT>(a) + widen_hi<DT>(a)) + widen<DT>(c2)) + widen_hi<DT>(c2)) / 4.0f;
    }
}
template <int DT, int POL>
__device__ __forceinline__ float single_tap(const map_t<DT>* q) {
    if constexpr (DT == PATS_MAP_F32) return ldm<POL>(q);
    else return widen<DT>(ldm<POL>(q));
}

// One 256-thread workgroup per stacked image n = s * B + b (left crops first).  Wave w takes channels w, w + 4, ...;
// a lane owns the points l, l + 64, l + 128 (< 145) of every channel it visits, so the source offsets of the three maps are
// computed ONCE per lane (no division in the channel loop) and a channel's 145 outputs leave as three coalesced stores.
// The channel loop is split by source (title / map 0 / map 1 / map 2): wave-uniform, branch-free bodies.
// Half output: a lane owns the NEIGHBOURING points 2l, 2l + 1 (< 128) and 128 + l (< 145) instead, so that a channel leaves as
// one 4-byte pair store per lane (at 2-byte alignment in the odd channels) and one 2-byte store of 17 lanes.
template <int DT, int POL, int OT>
__global__ void __launch_bounds__(256)
fine_desc_kernel(const map_t<DT>* __restrict__ f0, const map_t<DT>* __restrict__ f1,
                 const map_t<DT>* __restrict__ f2, const float* __restrict__ title,
                 const float* __restrict__ rubbish, int64_t B, out_t<OT>* __restrict__ desc,
                 const int64_t* __restrict__ B_live) {
    const int64_t n = blockIdx.x;              // s * B + b : index into the stacked maps
    const int64_t b = n % B;
    if (B_live && b >= *B_live) return;        // counted launch: rows past the device-side total are padding
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    out_t<OT>* o = desc + n * 264 * 145;
    int pt[3], off0[3], off1[3];
    bool live[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int p = OT == PATS_MAP_F32 ? lane + 64 * g : (g < 2 ? 2 * lane + g : 128 + lane);
        live[g] = p < 145;
        pt[g] = p < 144 ? p : 0;                               // positions (k // 12, k % 12); the dustbin column reads nothing
        const int r = pt[g] / 12, c = pt[g] - r * 12;
        off0[g] = (4 * r + 1) * 48 + 4 * c + 1;                // map 0: avgpool(2,1,1) -> 49x49, sample (4r+2, 4c+2)   :73-79
        off1[g] = (2 * r) * 24 + 2 * c;                        // map 1: avgpool -> 25x25, sample (2r+1, 2c+1)
    }
    const bool dust = lane == 16;                              // group 2 of lane 16 is point 144: the dustbin feature column
    auto put = [&](int ch, float v0, float v1, float v2) {
        out_t<OT>* row = o + ch * 145;
        if constexpr (OT == PATS_MAP_F32) {
            stm<POL>(row + lane, v0);
            stm<POL>(row + lane + 64, v1);
            if (live[2]) stm<POL>(row + lane + 128, dust ? rubbish[b * 264 + ch] : v2);       // second_layer.py:83,85
        } else {
            sth2<POL>(row + 2 * lane, narrow2<OT>(v0, v1));
            if (live[2]) stm<POL>(row + lane + 128, narrow<OT>(dust ? rubbish[b * 264 + ch] : v2));
        }
    };
    for (int ch = wave; ch < 8; ch += 4) {                     // the 8-channel "title"                         :82,84
        const float v = title[b * 8 + ch];
        put(ch, v, v, v);
    }
#pragma unroll 2
    for (int ch = 8 + wave; ch < 72; ch += 4) {                // map 0: [.,64,48,48]
        const map_t<DT>* m = f0 + (n * 64 + (ch - 8)) * 48 * 48;
        float v[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) v[g] = pooled_tap<DT, POL>(m + off0[g], 48);
        put(ch, v[0], v[1], v[2]);
    }
#pragma unroll 2
    for (int ch = 72 + wave; ch < 136; ch += 4) {              // map 1: [.,64,24,24]
        const map_t<DT>* m = f1 + (n * 64 + (ch - 72)) * 24 * 24;
        float v[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) v[g] = pooled_tap<DT, POL>(m + off1[g], 24);
        put(ch, v[0], v[1], v[2]);
    }
#pragma unroll 4
    for (int ch = 136 + wave; ch < 264; ch += 4) {             // map 2: [.,128,12,12], no pooling, sample (r, c)
        const map_t<DT>* m = f2 + (n * 128 + (ch - 136)) * 144;
        put(ch, single_tap<DT, POL>(m + pt[0]), single_tap<DT, POL>(m + pt[1]), single_tap<DT, POL>(m + pt[2]));
    }
}

// ---- third level -----------------------------------------------------------------------------
__device__ __forceinline__ long long round_half_even_div(float x, float d) {
    return (long long)rintf(x / d);      // torch.round = round half to even = rintf in the default mode
}

// The third-level index arithmetic of every third-level kernel for point p (third_layer.py:124-133, 141-144): the rounded
// points (written when `write`), the NHWC-view row of window cell (0, 0) of each side, and the dustbin feature's (image, cell).
struct third_point {
    long long i00[2], bb2, i2;
};
__device__ __forceinline__ third_point third_point_at(const float* __restrict__ mk0, const float* __restrict__ mk1,
                                                      int64_t p, int64_t b, int64_t B, bool write,
                                                      int64_t* __restrict__ ps_out, int64_t* __restrict__ pt_out) {
    constexpr int W = 8, M = 52;
    // mkpts0_c = round(mkpts0_c / 4) * 4                                                                                 :124
    const long long s0 = round_half_even_div(mk0[p * 2 + 0], 4.0f) * 4, s1 = round_half_even_div(mk0[p * 2 + 1], 4.0f) * 4;
    // mkpts1_c clamped to [0, 96] then rounded the same way                                                              :128-130
    float t0 = mk1[p * 2 + 0], t1 = mk1[p * 2 + 1];
    t0 = t0 >= 96.f ? 96.f : t0; t1 = t1 >= 96.f ? 96.f : t1;
    t0 = t0 <= 0.f ? 0.f : t0;   t1 = t1 <= 0.f ? 0.f : t1;
    const long long q0 = round_half_even_div(t0, 4.0f) * 4, q1 = round_half_even_div(t1, 4.0f) * 4;
    if (write) {
        if (ps_out) { ps_out[p * 2] = s0; ps_out[p * 2 + 1] = s1; }
        if (pt_out) { pt_out[p * 2] = q0; pt_out[p * 2 + 1] = q1; }
    }
    auto fdiv2 = [](long long v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); };      // python floor division
    // row of the NHWC view of window cell (0, 0): b M M + (y // 2 - W/2 + 2) M + (x // 2 - W/2 + 2)      :125-127,131-133
    third_point r;
    r.i00[0] = b * M * M + (fdiv2(s1) - W / 2 + 2) * M + (fdiv2(s0) - W / 2 + 2);
    r.i00[1] = b * M * M + (fdiv2(q1) - W / 2 + 2) * M + (fdiv2(q0) - W / 2 + 2);
    // dustbin feature: rubbish[b, :, y2*12 + x2], x2 = round(mk0x / 8), y2 = round(mk0y / 8)   :141-144
    // as a row of the flattened [B*144, 128] view, like the reference: cell 11 of a patch (round(92 / 8) = 12) reads the NEXT
    // patch's feature (PATS itself never sends the border ring here: second_layer.py:140-149,176-184)
    long long i2 = b * 144 + round_half_even_div((float)s1, 8.0f) * 12 + round_half_even_div((float)s0, 8.0f);
    i2 = i2 < 0 ? 0 : (i2 > B * 144 - 1 ? B * 144 - 1 : i2);      // memory safety (torch.gather would raise out of range)
    r.bb2 = i2 / 144;
    r.i2 = i2 - r.bb2 * 144;
    return r;
}

// The per-point kernel (the default until round 7; pats_set_third_gather(1) selects it): one workgroup (256 threads = 4 waves)
// per point; wave w handles channels 32w .. 32w+31, eight at a time (sixteen window loads in flight, then sixteen stores);
// lane = window cell.  The dustbin feature column is written once per wave by 32 lanes (one channel each) instead of by
// lane 0 inside the channel loop.  Half output on NCHW fp32 maps is this kernel's (the point-tiled one stays float32 only): a
// lane's window cell is one 2-byte store, which any half output's alignment takes.
template <int POL, int OT>
__global__ void __launch_bounds__(256)
third_desc_point_kernel(const float* __restrict__ ff0, const float* __restrict__ ff1,
                  const float* __restrict__ mk0, const float* __restrict__ mk1,
                  const int64_t* __restrict__ b_ids, const float* __restrict__ kenc,
                  const float* __restrict__ rubbish, int64_t P, int64_t B,
                  out_t<OT>* __restrict__ out0, out_t<OT>* __restrict__ out1, int64_t* __restrict__ ps_out,
                  int64_t* __restrict__ pt_out, const int64_t* __restrict__ P_dev) {
    constexpr int W = 8, M = 52, C = 128;
    // throughput mode: the launch covers the capacity, the count is on the device.
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), and the points of one fine
    // row - consecutive p - read overlapping windows of the same two maps (neighbouring cells are 2 map pixels apart, a
    // window row is 32 bytes of a 128-byte line): workgroup k takes point (k % 8) * ceil(P / 8) + k / 8, so that
    // neighbours in p run on the SAME XCD one after the other and meet in its L2 instead of each fetching its own lines.
    int64_t live = P;
    if (P_dev) { const int64_t n = *P_dev; live = n < P ? n : P; }
    const int64_t per = (live + 7) >> 3, p = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= per || p >= live) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = b_ids[p];
    const third_point tp = third_point_at(mk0, mk1, p, b, B, threadIdx.x == 0, ps_out, pt_out);
    const int wx = lane % W, wy = lane / W;
    long long i0 = tp.i00[0] + wy * M + wx, i1 = tp.i00[1] + wy * M + wx;       // rows of the NHWC view
    const long long lim = B * M * M - 1;
    i0 = i0 < 0 ? 0 : (i0 > lim ? lim : i0);      // memory safety (torch.gather would raise out of range)
    i1 = i1 < 0 ? 0 : (i1 > lim ? lim : i1);
    // NHWC row index -> (batch, y, x) of the NCHW map
    const long long bb0 = i0 / (M * M), r0 = i0 - bb0 * (M * M);
    const long long bb1 = i1 / (M * M), r1 = i1 - bb1 * (M * M);
    out_t<OT>* o0 = out0 + p * C * 65;
    out_t<OT>* o1 = out1 + p * C * 65;
    const float* src0 = ff0 + bb0 * C * (M * M) + r0;
    const float* src1 = ff1 + bb1 * C * (M * M) + r1;
#pragma unroll 1
    for (int c0 = 32 * wave; c0 < 32 * wave + 32; c0 += 8) {
        float a[8], c[8], ke[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k] = ldm<POL>(src0 + (int64_t)(c0 + k) * (M * M));
            c[k] = ldm<POL>(src1 + (int64_t)(c0 + k) * (M * M));
            ke[k] = kenc[(c0 + k) * 64 + lane];                                  // + self.kenc(kpts)   :139-140
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            stm<POL>(o0 + (c0 + k) * 65 + lane, narrow<OT>(a[k] + ke[k]));
            stm<POL>(o1 + (c0 + k) * 65 + lane, narrow<OT>(c[k] + ke[k]));
        }
    }
    if (lane < 32) {
        const int ch = 32 * wave + lane;
        const float rb = rubbish[(tp.bb2 * C + ch) * 144 + tp.i2];
        o0[ch * 65 + 64] = narrow<OT>(rb);                                       // :145-146
        o1[ch * 65 + 64] = narrow<OT>(rb);
    }
}

constexpr int THIRD_TILE = 8;      // points per workgroup of third_desc_kernel

// third level, NCHW, point-tiled (the default): one workgroup per tile of T = 8 consecutive points, wave w owns points
// 8 tile + 2w and 8 tile + 2w + 1.  third_inputs_kernel emits the points of a fine row consecutively (8 per row on average
// at the bench's workload) and the windows of neighbouring cells overlap by half, so the CHANNEL loop is outermost: the four
// waves read the same eight channel planes of neighbouring windows at about the same time and the shared 128-byte lines are
// hit in the CU's L1 / the XCD's L2 instead of being fetched again by another workgroup later (tools/third_gather_lines.py
// counts the lines: profiles/r07_third_gather_lines.txt).  Lane = window cell as in third_desc_point_kernel, 32 window loads
// in flight per chunk.  Each (point, side, chunk) of 8 x 65 outputs - the dustbin value in column 64 - is staged in a
// wave-private LDS slice and leaves as ONE linear span of 2 080 bytes (130 float4; 16-byte aligned: p * 33 280 +
// chunk * 2 080 from an aligned base, which the launcher checks), instead of 4-byte stores into rows of 65 floats.  Every
// element is the same a + ke add (or the same copied dustbin value) as in the per-point kernel: bit-identical by
// construction.  Points past the count in the last tile re-read the last live point and store nothing.  Tiles of 4 and 16
// points and a workgroup barrier per chunk measured within 2 % of this (profiles/r07_third_gather_ab.txt).
template <int POL>
__global__ void __launch_bounds__(256)
third_desc_kernel(const float* __restrict__ ff0, const float* __restrict__ ff1,
                  const float* __restrict__ mk0, const float* __restrict__ mk1,
                  const int64_t* __restrict__ b_ids, const float* __restrict__ kenc,
                  const float* __restrict__ rubbish, int64_t P, int64_t B,
                  float* __restrict__ out0, float* __restrict__ out1, int64_t* __restrict__ ps_out,
                  int64_t* __restrict__ pt_out, const int64_t* __restrict__ P_dev) {
    constexpr int PW = THIRD_TILE / 4;
    constexpr int M = 52, C = 128, NT = 65, T = THIRD_TILE, SPAN = 8 * NT;
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float stage[4 * PW * SPAN];
    int64_t live = P;
    if (P_dev) { const int64_t n = *P_dev; live = n < P ? n : P; }
    // XCD-aware tile order as in third_desc_point_kernel: tiles k and k + 1 run on the same XCD one after the other
    const int64_t tiles = (live + T - 1) / T, per = (tiles + 7) >> 3, tile = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= per || tile >= tiles) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long lim = B * M * M - 1;
    int64_t pp[PW];
    bool on[PW];
    const float* src[PW][2];
    const float* rub[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        const int64_t p = tile * T + wave * PW + j;
        on[j] = p < live;
        pp[j] = on[j] ? p : live - 1;
        const int64_t b = b_ids[pp[j]];
        const third_point tp = third_point_at(mk0, mk1, pp[j], b, B, on[j] && lane == 0, ps_out, pt_out);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            long long i = tp.i00[s] + (lane >> 3) * M + (lane & 7);
            i = i < 0 ? 0 : (i > lim ? lim : i);      // memory safety (torch.gather would raise out of range)
            const long long bb = i / (M * M);
            src[j][s] = (s ? ff1 : ff0) + bb * C * (M * M) + (i - bb * (M * M));
        }
        rub[j] = rubbish + tp.bb2 * C * 144 + tp.i2;
    }
    float* slice = stage + wave * PW * SPAN;
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += 8) {
        float a[PW][2][8], ke[8], rb[PW];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int j = 0; j < PW; ++j) {
                a[j][0][k] = ldm<POL>(src[j][0] + (int64_t)(c0 + k) * (M * M));
                a[j][1][k] = ldm<POL>(src[j][1] + (int64_t)(c0 + k) * (M * M));
            }
            ke[k] = kenc[(c0 + k) * 64 + lane];                                      // + self.kenc(kpts)   :139-140
        }
#pragma unroll
        for (int j = 0; j < PW; ++j) rb[j] = lane < 8 ? rub[j][(c0 + lane) * 144] : 0.f;      // :141-146
#pragma unroll
        for (int j = 0; j < PW; ++j) {
            float* sl = slice + j * SPAN;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int k = 0; k < 8; ++k) sl[k * NT + lane] = a[j][s][k] + ke[k];
                if (lane < 8) sl[lane * NT + 64] = rb[j];
                wave_lds_sync();
                const f4* v = reinterpret_cast<const f4*>(sl);
                f4* o = reinterpret_cast<f4*>((s ? out1 : out0) + pp[j] * (C * NT) + c0 * NT);
                if (on[j]) {
                    stm<POL>(o + lane, v[lane]);
                    stm<POL>(o + lane + 64, v[lane + 64]);
                    if (lane < SPAN / 4 - 128) stm<POL>(o + lane + 128, v[lane + 128]);
                }
                wave_lds_sync();                      // the next writes of the slice come after these reads
            }
        }
    }
}

// third level, NCHW, half maps: a window row of 8 cells is 16 contiguous bytes of a map row, so a lane takes TWO neighbouring
// cells as one 4-byte pair - lanes 0..31 one channel's 8x8 window, lanes 32..63 the next channel's - and stores them as one
// 8-byte write.  A pair starts at an even row i of the NHWC view (s0, q0 are multiples of 4, M is even), so it never straddles
// two images, and the clamp of third_desc_kernel treats both cells alike: a pair below row 0 reads row 0 twice, one past the
// last row reads the last row twice.  Wave w handles channels 32w .. 32w+31, sixteen at a time (eight pairs per side in
// flight, then sixteen stores); XCD-aware order and the dustbin column as in third_desc_point_kernel.  Half output: the pair
// leaves as one 4-byte write at 2-byte alignment (rows of 65 halves), the dustbin store stays scalar.
template <int DT, int POL, int OT>
__global__ void __launch_bounds__(256)
third_desc_half_kernel(const uint16_t* __restrict__ ff0, const uint16_t* __restrict__ ff1,
                       const float* __restrict__ mk0, const float* __restrict__ mk1,
                       const int64_t* __restrict__ b_ids, const float* __restrict__ kenc,
                       const float* __restrict__ rubbish, int64_t P, int64_t B,
                       out_t<OT>* __restrict__ out0, out_t<OT>* __restrict__ out1, int64_t* __restrict__ ps_out,
                       int64_t* __restrict__ pt_out, const int64_t* __restrict__ P_dev) {
    constexpr int M = 52, C = 128;
    int64_t live = P;
    if (P_dev) { const int64_t n = *P_dev; live = n < P ? n : P; }
    const int64_t per = (live + 7) >> 3, p = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= per || p >= live) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cp = lane & 31, sub = lane >> 5;                 // cells 2 cp, 2 cp + 1 (row cp / 4) of channel c0 + 2 k + sub
    const int64_t b = b_ids[p];
    const third_point tp = third_point_at(mk0, mk1, p, b, B, threadIdx.x == 0, ps_out, pt_out);
    const long long lim = B * M * M - 1;
    const uint16_t* src[2];
    bool below[2], above[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const long long i = tp.i00[s] + (cp >> 2) * M + 2 * (cp & 3);
        below[s] = i < 0;
        above[s] = i > lim;
        const long long j = below[s] ? 0 : (above[s] ? lim - 1 : i);
        const long long bb = j / (M * M);
        src[s] = (s ? ff1 : ff0) + bb * C * (M * M) + (j - bb * (M * M));
    }
    auto fix = [](uint32_t u, bool lo, bool hi) {              // a clamped pair: both cells read the one row it clamps to
        u = lo ? (u & 0xffffu) * 0x10001u : u;
        return hi ? (u >> 16) * 0x10001u : u;
    };
    out_t<OT>* o0 = out0 + p * C * 65 + 2 * cp;
    out_t<OT>* o1 = out1 + p * C * 65 + 2 * cp;
#pragma unroll 1
    for (int c0 = 32 * wave + sub; c0 < 32 * wave + 32; c0 += 16) {
        uint32_t a[8], c[8];
        f2s ke[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k] = ldm<POL>(reinterpret_cast<const uint32_t*>(src[0] + (int64_t)(c0 + 2 * k) * (M * M)));
            c[k] = ldm<POL>(reinterpret_cast<const uint32_t*>(src[1] + (int64_t)(c0 + 2 * k) * (M * M)));
            ke[k] = *reinterpret_cast<const f2s*>(kenc + (c0 + 2 * k) * 64 + 2 * cp);        // + self.kenc(kpts)   :139-140
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t u = fix(a[k], below[0], above[0]), v = fix(c[k], below[1], above[1]);
            f2s x, y;
            x.x = widen<DT>(u) + ke[k].x; x.y = widen_hi<DT>(u) + ke[k].y;
            y.x = widen<DT>(v) + ke[k].x; y.y = widen_hi<DT>(v) + ke[k].y;
            if constexpr (OT == PATS_MAP_F32) {
                stm2<POL>(o0 + (c0 + 2 * k) * 65, x);
                stm2<POL>(o1 + (c0 + 2 * k) * 65, y);
            } else {
                sth2<POL>(o0 + (c0 + 2 * k) * 65, narrow2<OT>(x.x, x.y));
                sth2<POL>(o1 + (c0 + 2 * k) * 65, narrow2<OT>(y.x, y.y));
            }
        }
    }
    if (lane < 32) {
        const int ch = 32 * wave + lane;
        const float rb = rubbish[(tp.bb2 * C + ch) * 144 + tp.i2];
        out0[p * C * 65 + ch * 65 + 64] = narrow<OT>(rb);                         // :145-146
        out1[p * C * 65 + ch * 65 + 64] = narrow<OT>(rb);
    }
}


// ---- the same two gathers on CHANNELS-LAST maps ----------------------------------------------------------------------
// The reference gathers from `feat.permute(0, 2, 3, 1).reshape(-1, C)` (third_layer.py:139-140) and samples single pixels
// of AvgPool'd maps (second_layer.py:73-79): per-PIXEL reads of all channels.  On the NCHW tensors a torch conv emits by
// default a pixel's channels lie H*W*4 bytes apart - a third-level window row is 32 bytes of every 208-byte map row (2.75
// 64-byte HBM granules fetched per 32 bytes used, measured), the stride-4 samples of the 48x48 map touch half of its
// granules for a sixteenth of its pixels.  A backbone run in torch.channels_last (MIOpen's native layout; the logical
// shape stays [B,C,H,W]) puts a pixel's channels in ONE contiguous run of 256 / 512 bytes: every granule fetched is
// used in full.  Lanes then run over channels while the outputs want lanes over nodes ([C, nodes] rows for the MFMA cost
// builds), so the tile turns through LDS and leaves as one linear, 16-byte-vectorised copy.  Same values, same
// operation order per element as the NCHW kernels: bit-identical outputs (tests/test_gpu_parity.py).

// one workgroup per (point, side): 64 pixels x 128 channels in, [128, 65] out.  Only the stage that brings the window into
// LDS depends on the map element type.  Half output: the fp32 tile leaves as 1 040 words of 16 bytes, eight elements each
// rounded after their kenc add (out0 / out1 16-byte aligned then; a point's block is 16 640 bytes).
template <int DT, int POL, int OT>
__global__ void __launch_bounds__(256)
third_desc_nhwc_kernel(const map_t<DT>* __restrict__ ff0, const map_t<DT>* __restrict__ ff1,
                       const float* __restrict__ mk0, const float* __restrict__ mk1,
                       const int64_t* __restrict__ b_ids, const float* __restrict__ kenc,
                       const float* __restrict__ rubbish, int64_t P, int64_t B,
                       out_t<OT>* __restrict__ out0, out_t<OT>* __restrict__ out1, int64_t* __restrict__ ps_out,
                       int64_t* __restrict__ pt_out, const int64_t* __restrict__ P_dev) {
    constexpr int M = 52, C = 128, NT = 65;
    __shared__ __attribute__((aligned(16))) float tile[C * NT];
    int64_t live = P;
    if (P_dev) { const int64_t n = *P_dev; live = n < P ? n : P; }
    // XCD-aware order as in third_desc_point_kernel; the two sides of a point follow each other on the same XCD (they share
    // the dustbin feature's lines)
    const unsigned k = blockIdx.x >> 3;
    const int side = k & 1;
    const int64_t per = (live + 7) >> 3, p = (int64_t)(blockIdx.x & 7) * per + (k >> 1);
    if ((int64_t)(k >> 1) >= per || p >= live) return;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t b = b_ids[p];
    const third_point tp = third_point_at(mk0, mk1, p, b, B, t == 0 && side == 0, ps_out, pt_out);
    const long long lim = B * M * M - 1;
    const map_t<DT>* __restrict__ ff = side ? ff1 : ff0;
    float rb = 0.f;
    if (t < C) rb = rubbish[(tp.bb2 * C + t) * 144 + tp.i2];
    // the window's registers: fp32 lanes hold channels l and l + 64 of 16 cells, half lanes channels 8 cg .. 8 cg + 7 of 4 cells
    const int cg = lane >> 2;
    std::conditional_t<DT == PATS_MAP_F32, float[2][16], u4[4]> v;
    if constexpr (DT == PATS_MAP_F32) {
        // wave w brings window cells 16w .. 16w+15, lane l channels l and l + 64 of each: 32 loads of 256 contiguous bytes in flight
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            long long i = (side ? tp.i00[1] : tp.i00[0]) + (2 * wave + (j >> 3)) * M + (j & 7);
            i = i < 0 ? 0 : (i > lim ? lim : i);          // memory safety (torch.gather would raise out of range)
            const float* src = ff + i * C;
            v[0][j] = ldm<POL>(src + lane);
            v[1][j] = ldm<POL>(src + lane + 64);
        }
    } else {
        // a pixel's 128 channels are 256 bytes = 16 lanes x 16 bytes; lane l of wave w loads channels 8 (l / 4) .. +7 of window
        // cells 16 j + 4 w + l % 4 (j < 4): each load instruction reads four whole pixels, and the LDS writes of a half-wave hit
        // 16 banks twice at most
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cell = 16 * j + 4 * wave + (lane & 3);
            long long i = (side ? tp.i00[1] : tp.i00[0]) + (cell >> 3) * M + (cell & 7);
            i = i < 0 ? 0 : (i > lim ? lim : i);          // memory safety (torch.gather would raise out of range)
            v[j] = ldm<POL>(reinterpret_cast<const u4*>(ff + i * C + 8 * cg));
        }
    }
    // + self.kenc(kpts) rides on the way out: element e = c * 65 + n of the output takes kenc[c, n]       :139-140
    constexpr int KE = OT == PATS_MAP_F32 ? 33 : 40;       // half output: lane t takes elements 8 (t + 256 r) .. + 7, r < 5
    float ke[KE];
    if constexpr (OT == PATS_MAP_F32) {
#pragma unroll
        for (int r = 0; r < 33; ++r) {
            const int e = t + 256 * r, c = e / NT, n = e - c * NT;
            ke[r] = kenc[(e < C * NT && n < 64) ? c * 64 + n : 0];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 5; ++r) {
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const int e0 = 8 * (t + 256 * r), c0 = e0 / NT, n0 = e0 - c0 * NT + h;      // a word spans two rows at most
                const int c = n0 < NT ? c0 : c0 + 1, n = n0 < NT ? n0 : n0 - NT;
                ke[8 * r + h] = kenc[(e0 < C * NT && n < 64) ? c * 64 + n : 0];
            }
        }
    }
    if constexpr (DT == PATS_MAP_F32) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            tile[lane * NT + 16 * wave + j] = v[0][j];
            tile[(lane + 64) * NT + 16 * wave + j] = v[1][j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cell = 16 * j + 4 * wave + (lane & 3);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                tile[(8 * cg + 2 * h) * NT + cell] = widen<DT>(v[j][h]);
                tile[(8 * cg + 2 * h + 1) * NT + cell] = widen_hi<DT>(v[j][h]);
            }
        }
    }
    if (t < C) tile[t * NT + 64] = rb;                                                                      // :145-146
    wg_barrier();
    out_t<OT>* o = (side ? out1 : out0) + p * C * NT;
    if constexpr (OT == PATS_MAP_F32) {
#pragma unroll
        for (int r = 0; r < 33; ++r) {
            const int e = t + 256 * r, c = e / NT, n = e - c * NT;
            if (e < C * NT) stm<POL>(o + e, n < 64 ? tile[e] + ke[r] : tile[e]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int q = t + 256 * r;
            if (q < C * NT / 8) {
                float x[8];
                const int n0 = (8 * q) % NT;
#pragma unroll
                for (int h = 0; h < 8; ++h)           // column n0 + h (mod 65) of its row: 64 is the dustbin value
                    x[h] = n0 + h != 64 ? tile[8 * q + h] + ke[8 * r + h] : tile[8 * q + h];
                u4 w;
                w.x = narrow2<OT>(x[0], x[1]); w.y = narrow2<OT>(x[2], x[3]);
                w.z = narrow2<OT>(x[4], x[5]); w.w = narrow2<OT>(x[6], x[7]);
                stm<POL>(reinterpret_cast<u4*>(o) + q, w);
            }
        }
    }
}

// one workgroup per stacked image; the 264 output channels leave in four 64-channel tiles (map 0, map 1, the two halves of
// map 2), each gathered with 16-byte loads, pooled in registers, turned in LDS and copied out as float4.  `cpp` = channels
// per pixel of the map, `ch0` = first of the 64 channels this pass takes.  The gather into LDS has one lane map per element
// size:
//   fp32  lane = (node % 4, four channels); 9 or 12 loads of 16 bytes in flight per lane
//   half  64 channels of a pixel are 128 bytes = 8 lanes x 16 bytes: lane = (node % 8, eight channels), a wave takes 8 nodes,
//         the workgroup 32 per group, 4.5 groups of the 144 nodes (waves 2 and 3 sit out the last one).  Every load
//         instruction reads 8 whole 128-byte lines.
// The LDS tile is float32 for every output type; half output is rounded in the copy (eight elements per 16-byte word).
template <int DT, int TAPS, int POL, int OT>
__device__ __forceinline__ void fine_tile_pass(const map_t<DT>* __restrict__ img, int cpp, int ch0, int rowpix, int step,
                                               int first, float* tile, out_t<OT>* __restrict__ o,
                                               const float* __restrict__ rub, int t) {
    constexpr int NP = 145;
    typedef float f4 __attribute__((ext_vector_type(4)));
    float dust = 0.f;
    if (t < 64) dust = rub[t];                                                                   // second_layer.py:83,85
    if constexpr (DT == PATS_MAP_F32) {
        const int lane = t & 63, wave = t >> 6, cg = lane & 15, sub = lane >> 4;
        constexpr int GR = TAPS == 1 ? 9 : 3;          // node groups per round
#pragma unroll 1
        for (int g0 = 0; g0 < 9; g0 += GR) {
            f4 q[GR][TAPS];
#pragma unroll
            for (int g = 0; g < GR; ++g) {
                const int nd = 16 * (g0 + g) + 4 * wave + sub, r = nd / 12, c = nd - 12 * r;   // positions (k // 12, k % 12)
                const float* px = img + ((step * r + first) * rowpix + step * c + first) * cpp + ch0 + 4 * cg;
#pragma unroll
                for (int tap = 0; tap < TAPS; ++tap)
                    q[g][tap] = ldm<POL>(reinterpret_cast<const f4*>(px + ((tap >> 1) * rowpix + (tap & 1)) * cpp));
            }
#pragma unroll
            for (int g = 0; g < GR; ++g) {
                const int nd = 16 * (g0 + g) + 4 * wave + sub;
                f4 v = q[g][0];
                if (TAPS == 4) v = (((q[g][0] + q[g][1]) + q[g][2]) + q[g][3]) / 4.0f;          // AvgPool2d(2, 1, 1)  :73-79
                tile[(4 * cg + 0) * NP + nd] = v.x;
                tile[(4 * cg + 1) * NP + nd] = v.y;
                tile[(4 * cg + 2) * NP + nd] = v.z;
                tile[(4 * cg + 3) * NP + nd] = v.w;
            }
        }
    } else {
        const int lane = t & 63, wave = t >> 6, cg = lane & 7, sub = lane >> 3;
        u4 q[5][TAPS];
#pragma unroll
        for (int g = 0; g < 5; ++g) {
            const int nd = 32 * g + 8 * wave + sub, r = nd / 12, c = nd - 12 * r;               // positions (k // 12, k % 12)
            if (g < 4 || wave < 2) {
                const uint16_t* px = img + ((step * r + first) * rowpix + step * c + first) * cpp + ch0 + 8 * cg;
#pragma unroll
                for (int tap = 0; tap < TAPS; ++tap)
                    q[g][tap] = ldm<POL>(reinterpret_cast<const u4*>(px + ((tap >> 1) * rowpix + (tap & 1)) * cpp));
            }
        }
#pragma unroll
        for (int g = 0; g < 5; ++g) {
            const int nd = 32 * g + 8 * wave + sub;
            if (g < 4 || wave < 2) {
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    float v;
                    if (TAPS == 4) {                                                             // AvgPool2d(2, 1, 1)  :73-79
                        float x[4];
#pragma unroll
                        for (int tap = 0; tap < 4; ++tap)
                            x[tap] = h & 1 ? widen_hi<DT>(q[g][tap][h >> 1]) : widen<DT>(q[g][tap][h >> 1]);
                        v = (((x[0] + x[1]) + x[2]) + x[3]) / 4.0f;
                    } else {
                        v = h & 1 ? widen_hi<DT>(q[g][0][h >> 1]) : widen<DT>(q[g][0][h >> 1]);
                    }
                    tile[(8 * cg + h) * NP + nd] = v;
                }
            }
        }
    }
    if (t < 64) tile[t * NP + 144] = dust;
    wg_barrier();
    if constexpr (OT == PATS_MAP_F32) {
        const f4* src = reinterpret_cast<const f4*>(tile);
        f4* dst = reinterpret_cast<f4*>(o);
        for (int e = t; e < 64 * NP / 4; e += 256) stm<POL>(dst + e, src[e]);
    } else {
        u4* dst = reinterpret_cast<u4*>(o);
        for (int e = t; e < 64 * NP / 8; e += 256) stm<POL>(dst + e, narrow8<OT>(tile + 8 * e));
    }
    wg_barrier();
}

template <int DT, int POL, int OT>
__global__ void __launch_bounds__(256)
fine_desc_nhwc_kernel(const map_t<DT>* __restrict__ f0, const map_t<DT>* __restrict__ f1,
                      const map_t<DT>* __restrict__ f2, const float* __restrict__ title,
                      const float* __restrict__ rubbish, int64_t B, out_t<OT>* __restrict__ desc,
                      const int64_t* __restrict__ B_live) {
    constexpr int NP = 145;
    __shared__ __attribute__((aligned(16))) float tile[64 * NP];
    const int64_t n = blockIdx.x;              // s * B + b : index into the stacked maps
    const int64_t b = n % B;
    if (B_live && b >= *B_live) return;        // counted launch: rows past the device-side total are padding
    const int t = threadIdx.x;
    out_t<OT>* o = desc + n * 264 * NP;
    const float* rub = rubbish + b * 264;
    for (int e = t; e < 8 * NP; e += 256) {                    // the 8-channel "title"                         :82,84
        const int ch = e / NP, p = e - ch * NP;
        o[e] = narrow<OT>(p == 144 ? rub[ch] : title[b * 8 + ch]);
    }
    // map 0 [.,48,48,64]: avgpool(2,1,1) -> 49x49, sample (4r+2, 4c+2) = mean of pixels (4r+1.., 4c+1..)
    fine_tile_pass<DT, 4, POL, OT>(f0 + n * 48 * 48 * 64, 64, 0, 48, 4, 1, tile, o + 8 * NP, rub + 8, t);
    // map 1 [.,24,24,64]: avgpool -> 25x25, sample (2r+1, 2c+1) = mean of pixels (2r.., 2c..)
    fine_tile_pass<DT, 4, POL, OT>(f1 + n * 24 * 24 * 64, 64, 0, 24, 2, 0, tile, o + 72 * NP, rub + 72, t);
    // map 2 [.,12,12,128]: no pooling, sample (r, c)
    fine_tile_pass<DT, 1, POL, OT>(f2 + n * 144 * 128, 128, 0, 12, 1, 0, tile, o + 136 * NP, rub + 136, t);
    fine_tile_pass<DT, 1, POL, OT>(f2 + n * 144 * 128, 128, 64, 12, 1, 0, tile, o + 200 * NP, rub + 200, t);
}

// PATS_GATHER_NT = 0..3 (see ldm / stm above), read once per process; without it 0 on NCHW maps, 3 on channels-last maps
static int gather_policy(bool channels_last) {
    static const int pol = [] { const char* e = env_switch("PATS_GATHER_NT"); return e ? (atoi(e) & 3) : -1; }();
    return pol >= 0 ? pol : (channels_last ? 3 : 0);
}

template <int V> using int_c = std::integral_constant<int, V>;
// f(int_c<DT>, int_c<POL>, int_c<OT>) for the maps' and the outputs' pats_map_dtype_t (validated before) and the store policy of
// the maps' layout
template <typename F>
static void with_gather(int dt, int ot, bool channels_last, F&& f) {
    auto pol = [&](auto d, auto o) {
        switch (gather_policy(channels_last)) {
            case 0: f(d, int_c<0>{}, o); break;
            case 1: f(d, int_c<1>{}, o); break;
            case 2: f(d, int_c<2>{}, o); break;
            default: f(d, int_c<3>{}, o); break;
        }
    };
    auto out = [&](auto d) {
        switch (ot) {
            case PATS_MAP_F16: pol(d, int_c<PATS_MAP_F16>{}); break;
            case PATS_MAP_BF16: pol(d, int_c<PATS_MAP_BF16>{}); break;
            default: pol(d, int_c<PATS_MAP_F32>{}); break;
        }
    };
    switch (dt) {
        case PATS_MAP_F16: out(int_c<PATS_MAP_F16>{}); break;
        case PATS_MAP_BF16: out(int_c<PATS_MAP_BF16>{}); break;
        default: out(int_c<PATS_MAP_F32>{}); break;
    }
}

// a15 over B stacked-image pairs (2 B workgroups); B_dev: the device-side row count of a counted launch, or null; desc in
// elements of `ot`
static int launch_fine(const void* f0, const void* f1, const void* f2, int dt, bool channels_last, const float* title,
                       const float* rubbish, int64_t B, const int64_t* B_dev, void* desc, int ot, pats_stream_t stream) {
    with_gather(dt, ot, channels_last, [&](auto d, auto pol, auto o) {
        constexpr int DT = decltype(d)::value, POL = decltype(pol)::value, OT = decltype(o)::value;
        using T = map_t<DT>;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)(2 * B)), dim3(256), 0, as_stream(stream), (const T*)f0, (const T*)f1,
                               (const T*)f2, title, rubbish, B, (out_t<OT>*)desc, B_dev);
        };
        if (channels_last) go(fine_desc_nhwc_kernel<DT, POL, OT>);
        else go(fine_desc_kernel<DT, POL, OT>);
    });
    return check_launch(channels_last ? "fine_desc_nhwc_kernel" : "fine_desc_kernel");
}

// a16 over a capacity of P points; P_dev: the device-side point count, or null.  The NCHW fp32 maps take the point-tiled
// third_desc_kernel, or - pats_set_third_gather(1), or outputs that are not 16-byte aligned - third_desc_point_kernel.  Same
// store policy default as the other NCHW gathers: non-temporal stores measured within 1 % of plain ones here
// (profiles/r07_third_gather_ab.txt).  out0 / out1 in elements of `ot`; half output on these maps is always the per-point
// kernel's (2-byte stores: whatever alignment a half output has, and whatever pats_set_third_gather says).
static int g_third_gather = 0;
static int launch_third(const void* f0, const void* f1, int dt, bool channels_last, const float* mkpts0_c,
                        const float* mkpts1_c, const int64_t* b_ids, const float* kenc, const float* rubbish, int64_t P_cap,
                        const int64_t* P_dev, int64_t B, void* out0, void* out1, int ot, int64_t* p_s_out, int64_t* p_t_out,
                        pats_stream_t stream) {
    const char* name = "third_desc_nhwc_kernel";
    with_gather(dt, ot, channels_last, [&](auto d, auto pol, auto o) {
        constexpr int DT = decltype(d)::value, POL = decltype(pol)::value, OT = decltype(o)::value;
        using T = map_t<DT>;
        auto go = [&](auto kernel, const char* kname, int64_t blocks, auto* o0, auto* o1) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const T*)f0, (const T*)f1,
                               mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P_cap, B, o0, o1, p_s_out, p_t_out, P_dev);
            name = kname;
        };
        out_t<OT>* const o0 = (out_t<OT>*)out0;
        out_t<OT>* const o1 = (out_t<OT>*)out1;
        if (channels_last)
            go(third_desc_nhwc_kernel<DT, POL, OT>, "third_desc_nhwc_kernel", (P_cap + 7) / 8 * 16, o0, o1);
        else if constexpr (DT != PATS_MAP_F32)
            go(third_desc_half_kernel<DT, POL, OT>, "third_desc_half_kernel", (P_cap + 7) / 8 * 8, o0, o1);
        else if constexpr (OT != PATS_MAP_F32)
            go(third_desc_point_kernel<POL, OT>, "third_desc_point_kernel", (P_cap + 7) / 8 * 8, o0, o1);
        else if (g_third_gather == 1 || ((uintptr_t)out0 | (uintptr_t)out1) % 16 != 0)
            go(third_desc_point_kernel<POL, OT>, "third_desc_point_kernel", (P_cap + 7) / 8 * 8, o0, o1);
        else
            go(third_desc_kernel<POL>, "third_desc_kernel", ((P_cap + THIRD_TILE - 1) / THIRD_TILE + 7) / 8 * 8, o0, o1);
    });
    return check_launch(name);
}

}  // namespace pats

using namespace pats;

extern "C" int pats_set_third_gather(int mode) {
    const int prev = g_third_gather;
    if (mode == 0 || mode == 1) g_third_gather = mode;
    return prev;
}

extern "C" int pats_fine_descriptors_f32(const float* feat0, const float* feat1, const float* feat2,
                                         const float* title, const float* rubbish, int64_t B,
                                         float* desc, pats_stream_t stream) {
    PATS_REQUIRE(B >= 0, "fine_descriptors: bad shape");
    if (B == 0) return PATS_OK;
    PATS_REQUIRE(feat0 && feat1 && feat2 && title && rubbish && desc, "fine_descriptors: null pointer");
    return launch_fine(feat0, feat1, feat2, PATS_MAP_F32, false, title, rubbish, B, nullptr, desc, PATS_MAP_F32, stream);
}

// a15 launched over a CAPACITY of B_cap rows with the number of rows in use on the device (throughput mode: the fine level's
// row table): workgroups of rows >= *B_dev return at once, their desc blocks are left untouched.
extern "C" int pats_fine_descriptors_counted_f32(const float* feat0, const float* feat1, const float* feat2,
                                                 const float* title, const float* rubbish, int64_t B_cap,
                                                 const int64_t* B_dev, int channels_last, float* desc, pats_stream_t stream) {
    PATS_REQUIRE(B_cap >= 0, "fine_descriptors_counted: bad shape");
    if (B_cap == 0) return PATS_OK;
    PATS_REQUIRE(B_dev && feat0 && feat1 && feat2 && title && rubbish && desc, "fine_descriptors_counted: null pointer");
    if (channels_last)
        PATS_REQUIRE(((uintptr_t)feat0 | (uintptr_t)feat1 | (uintptr_t)feat2 | (uintptr_t)desc) % 16 == 0,
                     "fine_descriptors_counted: channels-last maps and desc must be 16-byte aligned");
    return launch_fine(feat0, feat1, feat2, PATS_MAP_F32, channels_last, title, rubbish, B_cap, B_dev, desc, PATS_MAP_F32, stream);
}

extern "C" int pats_third_descriptors_f32(const float* feat_f0, const float* feat_f1,
                                          const float* mkpts0_c, const float* mkpts1_c,
                                          const int64_t* b_ids, const float* kenc, const float* rubbish,
                                          int64_t P, int64_t B, float* out0, float* out1,
                                          int64_t* p_s_out, int64_t* p_t_out, pats_stream_t stream) {
    PATS_REQUIRE(P >= 0 && B > 0, "third_descriptors: bad shape");
    if (P == 0) return PATS_OK;
    PATS_REQUIRE(feat_f0 && feat_f1 && mkpts0_c && mkpts1_c && b_ids && kenc && rubbish && out0 && out1,
                 "third_descriptors: null pointer");
    return launch_third(feat_f0, feat_f1, PATS_MAP_F32, false, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P, nullptr, B, out0,
                        out1, PATS_MAP_F32, p_s_out, p_t_out, stream);
}

extern "C" int pats_third_descriptors_counted_f32(const float* feat_f0, const float* feat_f1,
                                                  const float* mkpts0_c, const float* mkpts1_c,
                                                  const int64_t* b_ids, const float* kenc, const float* rubbish,
                                                  int64_t P_cap, const int64_t* P_dev, int64_t B, float* out0, float* out1,
                                                  int64_t* p_s_out, int64_t* p_t_out, pats_stream_t stream) {
    PATS_REQUIRE(P_cap >= 0 && B > 0, "third_descriptors_counted: bad shape");
    if (P_cap == 0) return PATS_OK;
    PATS_REQUIRE(P_dev && feat_f0 && feat_f1 && mkpts0_c && mkpts1_c && b_ids && kenc && rubbish && out0 && out1,
                 "third_descriptors_counted: null pointer");
    return launch_third(feat_f0, feat_f1, PATS_MAP_F32, false, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P_cap, P_dev, B, out0,
                        out1, PATS_MAP_F32, p_s_out, p_t_out, stream);
}

extern "C" int pats_fine_descriptors_nhwc_f32(const float* feat0, const float* feat1, const float* feat2,
                                              const float* title, const float* rubbish, int64_t B,
                                              float* desc, pats_stream_t stream) {
    PATS_REQUIRE(B >= 0, "fine_descriptors_nhwc: bad shape");
    if (B == 0) return PATS_OK;
    PATS_REQUIRE(feat0 && feat1 && feat2 && title && rubbish && desc, "fine_descriptors_nhwc: null pointer");
    PATS_REQUIRE(((uintptr_t)feat0 | (uintptr_t)feat1 | (uintptr_t)feat2 | (uintptr_t)desc) % 16 == 0,
                 "fine_descriptors_nhwc: maps and desc must be 16-byte aligned");
    return launch_fine(feat0, feat1, feat2, PATS_MAP_F32, true, title, rubbish, B, nullptr, desc, PATS_MAP_F32, stream);
}

extern "C" int pats_third_descriptors_nhwc_f32(const float* feat_f0, const float* feat_f1,
                                               const float* mkpts0_c, const float* mkpts1_c,
                                               const int64_t* b_ids, const float* kenc, const float* rubbish,
                                               int64_t P_cap, const int64_t* P_dev, int64_t B, float* out0, float* out1,
                                               int64_t* p_s_out, int64_t* p_t_out, pats_stream_t stream) {
    PATS_REQUIRE(P_cap >= 0 && B > 0, "third_descriptors_nhwc: bad shape");
    if (P_cap == 0) return PATS_OK;
    PATS_REQUIRE(feat_f0 && feat_f1 && mkpts0_c && mkpts1_c && b_ids && kenc && rubbish && out0 && out1,
                 "third_descriptors_nhwc: null pointer");
    return launch_third(feat_f0, feat_f1, PATS_MAP_F32, true, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P_cap, P_dev, B, out0,
                        out1, PATS_MAP_F32, p_s_out, p_t_out, stream);
}


// a15 / a16 on maps of any pats_map_dtype_t, either memory format, with or without the device-side count.  Every refusal comes
// before any launch.
extern "C" int pats_fine_descriptors_typed(const void* feat0, const void* feat1, const void* feat2, pats_map_dtype_t dtype,
                                           int channels_last, const float* title, const float* rubbish, int64_t B_cap,
                                           const int64_t* B_dev, float* desc, pats_stream_t stream) {
    PATS_REQUIRE(dtype == PATS_MAP_F32 || dtype == PATS_MAP_F16 || dtype == PATS_MAP_BF16,
                 "fine_descriptors_typed: unknown map dtype %d", (int)dtype);
    PATS_REQUIRE(B_cap >= 0, "fine_descriptors_typed: bad shape");
    if (B_cap == 0) return PATS_OK;
    PATS_REQUIRE(feat0 && feat1 && feat2 && title && rubbish && desc, "fine_descriptors_typed: null pointer");
    const uintptr_t maps = (uintptr_t)feat0 | (uintptr_t)feat1 | (uintptr_t)feat2;
    if (channels_last)      // 16-byte map loads, 16-byte stores of desc
        PATS_REQUIRE((maps | (uintptr_t)desc) % 16 == 0, "fine_descriptors_typed: channels-last maps and desc must be 16-byte aligned");
    else                    // 4-byte pair / float loads (f32: 8-byte pairs at 4-byte alignment)
        PATS_REQUIRE(maps % 4 == 0, "fine_descriptors_typed: NCHW maps must be 4-byte aligned");
    return launch_fine(feat0, feat1, feat2, dtype, channels_last, title, rubbish, B_cap, B_dev, desc, PATS_MAP_F32, stream);
}

extern "C" int pats_third_descriptors_typed(const void* feat_f0, const void* feat_f1, pats_map_dtype_t dtype, int channels_last,
                                            const float* mkpts0_c, const float* mkpts1_c, const int64_t* b_ids,
                                            const float* kenc, const float* rubbish, int64_t P_cap, const int64_t* P_dev,
                                            int64_t B, float* out0, float* out1, int64_t* p_s_out, int64_t* p_t_out,
                                            pats_stream_t stream) {
    PATS_REQUIRE(dtype == PATS_MAP_F32 || dtype == PATS_MAP_F16 || dtype == PATS_MAP_BF16,
                 "third_descriptors_typed: unknown map dtype %d", (int)dtype);
    PATS_REQUIRE(P_cap >= 0 && B > 0, "third_descriptors_typed: bad shape");
    if (P_cap == 0) return PATS_OK;
    PATS_REQUIRE(feat_f0 && feat_f1 && mkpts0_c && mkpts1_c && b_ids && kenc && rubbish && out0 && out1,
                 "third_descriptors_typed: null pointer");
    const uintptr_t maps = (uintptr_t)feat_f0 | (uintptr_t)feat_f1;
    if (channels_last)      // 16-byte loads of half pixels (f32: 4-byte loads, aligned as the NCHW rule)
        PATS_REQUIRE(maps % (dtype == PATS_MAP_F32 ? 4 : 16) == 0, "third_descriptors_typed: channels-last maps must be %d-byte aligned",
                     dtype == PATS_MAP_F32 ? 4 : 16);
    else                    // 4-byte float / cell-pair loads
        PATS_REQUIRE(maps % 4 == 0, "third_descriptors_typed: NCHW maps must be 4-byte aligned");
    return launch_third(feat_f0, feat_f1, dtype, channels_last, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P_cap, P_dev, B, out0,
                        out1, PATS_MAP_F32, p_s_out, p_t_out, stream);
}


// The two entries above with the OUTPUT element type selectable too: each element is the float32 value the fp32-output kernel
// stores, rounded once to `out_dtype` (nearest even) at the store.  PATS_MAP_F32 is the call above.
extern "C" int pats_fine_descriptors_typed_out(const void* feat0, const void* feat1, const void* feat2, pats_map_dtype_t dtype,
                                               int channels_last, const float* title, const float* rubbish, int64_t B_cap,
                                               const int64_t* B_dev, void* desc, pats_map_dtype_t out_dtype,
                                               pats_stream_t stream) {
    PATS_REQUIRE(out_dtype == PATS_MAP_F32 || out_dtype == PATS_MAP_F16 || out_dtype == PATS_MAP_BF16,
                 "fine_descriptors_typed_out: unknown output dtype %d", (int)out_dtype);
    if (out_dtype == PATS_MAP_F32)
        return pats_fine_descriptors_typed(feat0, feat1, feat2, dtype, channels_last, title, rubbish, B_cap, B_dev, (float*)desc,
                                           stream);
    PATS_REQUIRE(dtype == PATS_MAP_F32 || dtype == PATS_MAP_F16 || dtype == PATS_MAP_BF16,
                 "fine_descriptors_typed_out: unknown map dtype %d", (int)dtype);
    PATS_REQUIRE(B_cap >= 0, "fine_descriptors_typed_out: bad shape");
    if (B_cap == 0) return PATS_OK;
    PATS_REQUIRE(feat0 && feat1 && feat2 && title && rubbish && desc, "fine_descriptors_typed_out: null pointer");
    const uintptr_t maps = (uintptr_t)feat0 | (uintptr_t)feat1 | (uintptr_t)feat2;
    if (channels_last) {    // 16-byte map loads, 16-byte stores of desc
        PATS_REQUIRE((maps | (uintptr_t)desc) % 16 == 0,
                     "fine_descriptors_typed_out: channels-last maps and desc must be 16-byte aligned");
    } else {                // 4-byte pair / float loads; pair stores at 2-byte alignment
        PATS_REQUIRE(maps % 4 == 0, "fine_descriptors_typed_out: NCHW maps must be 4-byte aligned");
        PATS_REQUIRE((uintptr_t)desc % 2 == 0, "fine_descriptors_typed_out: a half desc must be 2-byte aligned");
    }
    return launch_fine(feat0, feat1, feat2, dtype, channels_last, title, rubbish, B_cap, B_dev, desc, out_dtype, stream);
}

extern "C" int pats_third_descriptors_typed_out(const void* feat_f0, const void* feat_f1, pats_map_dtype_t dtype,
                                                int channels_last, const float* mkpts0_c, const float* mkpts1_c,
                                                const int64_t* b_ids, const float* kenc, const float* rubbish, int64_t P_cap,
                                                const int64_t* P_dev, int64_t B, void* out0, void* out1,
                                                pats_map_dtype_t out_dtype, int64_t* p_s_out, int64_t* p_t_out,
                                                pats_stream_t stream) {
    PATS_REQUIRE(out_dtype == PATS_MAP_F32 || out_dtype == PATS_MAP_F16 || out_dtype == PATS_MAP_BF16,
                 "third_descriptors_typed_out: unknown output dtype %d", (int)out_dtype);
    if (out_dtype == PATS_MAP_F32)
        return pats_third_descriptors_typed(feat_f0, feat_f1, dtype, channels_last, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P_cap,
                                            P_dev, B, (float*)out0, (float*)out1, p_s_out, p_t_out, stream);
    PATS_REQUIRE(dtype == PATS_MAP_F32 || dtype == PATS_MAP_F16 || dtype == PATS_MAP_BF16,
                 "third_descriptors_typed_out: unknown map dtype %d", (int)dtype);
    PATS_REQUIRE(P_cap >= 0 && B > 0, "third_descriptors_typed_out: bad shape");
    if (P_cap == 0) return PATS_OK;
    PATS_REQUIRE(feat_f0 && feat_f1 && mkpts0_c && mkpts1_c && b_ids && kenc && rubbish && out0 && out1,
                 "third_descriptors_typed_out: null pointer");
    const uintptr_t maps = (uintptr_t)feat_f0 | (uintptr_t)feat_f1, outs = (uintptr_t)out0 | (uintptr_t)out1;
    if (channels_last) {    // 16-byte loads of half pixels (f32: 4-byte loads); 16-byte stores of the half outputs
        PATS_REQUIRE(maps % (dtype == PATS_MAP_F32 ? 4 : 16) == 0,
                     "third_descriptors_typed_out: channels-last maps must be %d-byte aligned", dtype == PATS_MAP_F32 ? 4 : 16);
        PATS_REQUIRE(outs % 16 == 0, "third_descriptors_typed_out: half outputs of channels-last maps must be 16-byte aligned");
    } else {                // 4-byte float / cell-pair loads; 2-byte stores or pair stores at 2-byte alignment
        PATS_REQUIRE(maps % 4 == 0, "third_descriptors_typed_out: NCHW maps must be 4-byte aligned");
        PATS_REQUIRE(outs % 2 == 0, "third_descriptors_typed_out: half outputs must be 2-byte aligned");
    }
    return launch_third(feat_f0, feat_f1, dtype, channels_last, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, P_cap, P_dev, B, out0,
                        out1, out_dtype, p_s_out, p_t_out, stream);
}
