// The image front end: raw decoded uint8 images -> the cropped, resized, zero-padded canvases of a MixedPack's flat stores, in ONE
// launch for all 2 * pairs images of a batch.  include/pats_amd.h ("Image front end") states the definition - the centre crop of
// the reference's Resize_img, the fixed-point bilinear arithmetic of OpenCV's portable uint8 path (or its 2 x 2 mean at an exact
// halving) and the zero pad of copyMakeBorder; docs/kernels.md 4.20 the design.
//
//   prepare_kernel<T>   blockIdx.y = the image, blockIdx.x * PREP_THREADS + threadIdx.x = a 16-byte CHUNK of its canvas counted
//                       row-major: a lane owns PREP_LANE_BYTES contiguous output bytes of one canvas row (16 uint8, 8 half or 4
//                       float32 values - a row is 96 * (W / 32) values, so chunks never cross rows and every store is aligned) and
//                       writes them with one 16-byte store.  The values of a chunk belong to at most NPIX pixels; the lane forms the
//                       x coefficients once per pixel and the y coefficients once, in float64 / float32 exactly as defined, reads the
//                       four taps of every value it needs as byte loads (the caches serve them: neighbouring lanes read neighbouring
//                       source bytes) and picks its VALS values out of the NPIX * 3 by its phase (first value's channel).  Chunks
//                       below or right of the target are the pad: zeros, no load.  No LDS, no barrier, nothing crosses lanes.
#include "common.hpp"

namespace pats {

constexpr int PREP_THREADS = 256;                      // lanes per workgroup
constexpr int PREP_LANE_BYTES = 16;                    // output bytes per lane: one global_store_dwordx4
constexpr int PREP_MAX_SIDE = 16384;                   // = pats_prepare_images_max_side(): a canvas has fewer than 2^31 chunks
constexpr float PREP_COEF_ONE = 2048.0f;               // OpenCV's INTER_RESIZE_COEF_SCALE

struct PrepAxis { int s, t, a0, a1; };                 // the two taps and their weights

// the per-axis coefficients of destination sample d; scale = 1.0 / (double(dn) / double(sn)) comes with the image's table entry
__device__ __forceinline__ PrepAxis prep_axis(int d, double scale, int sn) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);         // float64, contraction off, one rounding to float32
    const float fl = __builtin_floorf(f);
    int s = (int)fl;
    f = f - fl;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= sn - 1) { s = sn - 1; f = 0.0f; }
    PrepAxis r;
    r.s = s;
    r.t = s + 1 < sn ? s + 1 : sn - 1;
    r.a0 = (int)__builtin_rintf((1.0f - f) * PREP_COEF_ONE);   // ties to even
    r.a1 = (int)__builtin_rintf(f * PREP_COEF_ONE);
    return r;
}

// 0 .. 255 in the store's element type, as raw bits (exact in all four)
template <typename T> __device__ __forceinline__ uint32_t prep_bits(int v);
template <> __device__ __forceinline__ uint32_t prep_bits<uint8_t>(int v) { return (uint32_t)v; }
template <> __device__ __forceinline__ uint32_t prep_bits<float>(int v) { return __float_as_uint((float)v); }
template <> __device__ __forceinline__ uint32_t prep_bits<_Float16>(int v) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)(float)v); }
template <> __device__ __forceinline__ uint32_t prep_bits<bf16_t>(int v) { return __float_as_uint((float)v) >> 16; }

template <typename T>
__global__ void __launch_bounds__(PREP_THREADS)
prepare_kernel(const pats_prepare_image_t* __restrict__ tab, T* __restrict__ left, T* __restrict__ right) {
    constexpr int VALS = PREP_LANE_BYTES / (int)sizeof(T);      // values per lane
    constexpr int NPIX = (VALS + 1) / 3 + 1;                    // pixels VALS consecutive values can touch
    constexpr int PER_WORD = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    const pats_prepare_image_t im = tab[blockIdx.y];            // workgroup-uniform
    const uint32_t row_chunks = (uint32_t)(im.W * 3 / VALS);
    const uint32_t chunk = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (chunk >= (uint32_t)im.H * row_chunks) return;
    const int y = (int)(chunk / row_chunks), v0 = (int)(chunk - (uint32_t)y * row_chunks) * VALS;
    const int xp = v0 / 3, phase = v0 - 3 * xp;                 // the first value's pixel and channel
    int px[NPIX * 3];
#pragma unroll
    for (int i = 0; i < NPIX * 3; ++i) px[i] = 0;
    if (y < im.h_t && xp < im.w_t) {
        const int64_t rs = (int64_t)im.w0 * 3;
        const uint8_t* __restrict__ S = im.src + ((int64_t)im.y0 * im.w0 + im.x0) * 3;       // the window's first byte
        const bool area = im.w_c == 2 * im.w_t && im.h_c == 2 * im.h_t;                       // workgroup-uniform
        PrepAxis b;
        if (area) { b.s = 2 * y; b.t = 2 * y + 1; b.a0 = b.a1 = 0; }
        else b = prep_axis(y, im.scale_y, im.h_c);
        const uint8_t* __restrict__ r0 = S + (int64_t)b.s * rs;
        const uint8_t* __restrict__ r1 = S + (int64_t)b.t * rs;
#pragma unroll
        for (int k = 0; k < NPIX; ++k) {
            const int x = xp + k;
            if (x >= im.w_t) continue;                          // the pad right of the target
            PrepAxis a;
            if (area) { a.s = 2 * x; a.t = 2 * x + 1; a.a0 = a.a1 = 0; }
            else a = prep_axis(x, im.scale_x, im.w_c);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * k + c;
                if (i < phase || i >= phase + VALS) continue;   // a value of a neighbouring lane
                const int cc = im.bgr ? 2 - c : c;
                const int s00 = r0[a.s * 3 + cc], s01 = r0[a.t * 3 + cc], s10 = r1[a.s * 3 + cc], s11 = r1[a.t * 3 + cc];
                int v;
                if (area) {
                    v = (s00 + s01 + s10 + s11 + 2) >> 2;
                } else {
                    const int h0 = s00 * a.a0 + s01 * a.a1, h1 = s10 * a.a0 + s11 * a.a1;
                    v = (((b.a0 * (h0 >> 4)) >> 16) + ((b.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                }
                px[i] = v;
            }
        }
    }
    uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < VALS; ++j) {
        const int v = phase == 0 ? px[j] : (phase == 1 ? px[j + 1] : px[j + 2]);
        q[j / PER_WORD] |= prep_bits<T>(v) << (BITS * (j % PER_WORD) & 31);
    }
    T* __restrict__ dst = (im.side ? right : left) + im.dst + ((int64_t)y * im.W * 3 + v0);
    *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
}

template <typename T>
static void prepare_launch(const pats_prepare_image_t* tab, int64_t n_img, int64_t max_chunks, void* left, void* right, hipStream_t st) {
    hipLaunchKernelGGL(prepare_kernel<T>, dim3((unsigned)ceil_div(max_chunks, PREP_THREADS), (unsigned)n_img), dim3(PREP_THREADS), 0, st,
                       tab, (T*)left, (T*)right);
}

}  // namespace pats

using namespace pats;

extern "C" int64_t pats_prepare_images_max_side(void) { return PREP_MAX_SIDE; }

extern "C" int pats_prepare_images_u8(const pats_prepare_image_t* images_host, const pats_prepare_image_t* images, int64_t n_img,
                                      void* left, int64_t left_elems, void* right, int64_t right_elems, pats_img_dtype_t dtype,
                                      pats_stream_t stream) {
    const int rc = epi_check_args("prepare_images", {{"images_host", images_host, 1}, {"images", images, 8}, {"left", left, 16},
                                                     {"right", right, 16}}, true);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(dtype == PATS_IMG_F32 || dtype == PATS_IMG_F16 || dtype == PATS_IMG_BF16 || dtype == PATS_IMG_U8,
                 "prepare_images: unknown output dtype %d", (int)dtype);
    PATS_REQUIRE(n_img >= 1 && n_img <= 65535, "prepare_images: n_img = %lld (1 .. 65535)", (long long)n_img);
    PATS_REQUIRE(left_elems >= 0 && right_elems >= 0, "prepare_images: negative store size");
    const int esize = dtype == PATS_IMG_F32 ? 4 : (dtype == PATS_IMG_U8 ? 1 : 2);
    int64_t max_chunks = 0;
    for (int64_t i = 0; i < n_img; ++i) {
        const pats_prepare_image_t& im = images_host[i];
        const long long n = (long long)i;
        PATS_REQUIRE(im.src, "prepare_images: image %lld has a null source", n);
        PATS_REQUIRE(im.h0 >= 1 && im.w0 >= 1 && im.h0 <= PREP_MAX_SIDE && im.w0 <= PREP_MAX_SIDE,
                     "prepare_images: image %lld has the source size %d x %d (1 .. max_side = %d)", n, im.h0, im.w0, PREP_MAX_SIDE);
        PATS_REQUIRE(im.h_c >= 1 && im.w_c >= 1 && im.y0 >= 0 && im.x0 >= 0 && (int64_t)im.y0 + im.h_c <= im.h0 &&
                     (int64_t)im.x0 + im.w_c <= im.w0,
                     "prepare_images: image %lld: the window rows [%d, +%d) columns [%d, +%d) leaves its %d x %d source", n, im.y0,
                     im.h_c, im.x0, im.w_c, im.h0, im.w0);
        PATS_REQUIRE(im.H >= 32 && im.W >= 32 && im.H % 32 == 0 && im.W % 32 == 0 && im.H <= PREP_MAX_SIDE && im.W <= PREP_MAX_SIDE,
                     "prepare_images: image %lld has the canvas %d x %d (multiples of 32, up to max_side = %d)", n, im.H, im.W,
                     PREP_MAX_SIDE);
        PATS_REQUIRE(im.h_t >= 1 && im.w_t >= 1 && im.h_t <= im.H && im.w_t <= im.W,
                     "prepare_images: image %lld: the target %d x %d does not fit its canvas %d x %d", n, im.h_t, im.w_t, im.H, im.W);
        PATS_REQUIRE(im.side == 0 || im.side == 1, "prepare_images: image %lld: side = %d (0 left, 1 right)", n, im.side);
        PATS_REQUIRE(im.bgr == 0 || im.bgr == 1, "prepare_images: image %lld: bgr = %d (0 / 1)", n, im.bgr);
        PATS_REQUIRE(im.scale_x == 1.0 / ((double)im.w_t / (double)im.w_c) && im.scale_y == 1.0 / ((double)im.h_t / (double)im.h_c),
                     "prepare_images: image %lld: scale_x / scale_y are not 1.0 / (double(target) / double(window))", n);
        const int64_t elems = (int64_t)im.H * im.W * 3, cap = im.side ? right_elems : left_elems;
        PATS_REQUIRE(im.dst >= 0 && im.dst <= cap - elems, "prepare_images: image %lld: the canvas at element %lld leaves its store of %lld",
                     n, (long long)im.dst, (long long)cap);
        PATS_REQUIRE(im.dst * esize % PREP_LANE_BYTES == 0, "prepare_images: image %lld: the canvas does not start on a 16-byte boundary", n);
        const int64_t chunks = elems * esize / PREP_LANE_BYTES;
        max_chunks = chunks > max_chunks ? chunks : max_chunks;
    }
    const hipStream_t st = as_stream(stream);
    switch (dtype) {
        case PATS_IMG_U8: prepare_launch<uint8_t>(images, n_img, max_chunks, left, right, st); break;
        case PATS_IMG_F16: prepare_launch<_Float16>(images, n_img, max_chunks, left, right, st); break;
        case PATS_IMG_BF16: prepare_launch<bf16_t>(images, n_img, max_chunks, left, right, st); break;
        default: prepare_launch<float>(images, n_img, max_chunks, left, right, st); break;
    }
    return check_launch("prepare_images kernel");
}
