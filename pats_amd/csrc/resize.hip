// Patch-subdivision gather for PATS on gfx950: crop bounds, left fixed-grid crops, and the
// batched crop + bilinear resize that replaces the reference's only native component.
//
//   bounds      Compute_imgs                      utils/utils.py:1350-1382
//   left crops  origin_extract on the padded left utils/utils.py:1300-1318, caller :1383-1384
//   resize      tensor_resize / resize            setup/library.cpp:47-66 (binding :92-93)
//
// The reference's resize is a serial C++ loop with five `.item()` device->host syncs per crop
// around narrow + upsample_bilinear2d + index_put_; here all K crops are one launch that reads
// the bounds from device memory.  Output pixels map to consecutive lanes (coalesced 384-byte row
// stores); source taps of one output row fall in at most two source rows, served by L1/L2.
#include "common.hpp"

#include <cmath>
#include <cstdlib>
#include <type_traits>

#ifndef PATS_CROPS_NT_DEFAULT
#define PATS_CROPS_NT_DEFAULT 1
#endif

namespace pats {

// ---- bounds + ordered compaction of the matched patches --------------------------------------
__device__ __forceinline__ void
imgs_bounds_block(const float* __restrict__ x_scale, const float* __restrict__ y_scale,
                  const float* __restrict__ average_point, const uint8_t* __restrict__ ifn, int Np,
                  int height, int width, int img, int64_t* __restrict__ bound5,
                  int64_t* __restrict__ K_out, float* __restrict__ xsn, float* __restrict__ ysn,
                  float* __restrict__ avn) {
    __shared__ int wave_tot[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float ps = 32.0f, margin = 128.0f;
    const float board1 = (float)(32 * height - 1), board3 = (float)(32 * width);   // :1351
    if (tid == 0) base_s = 0;
    wg_barrier();
    for (int k0 = 0; k0 < Np; k0 += 1024) {
        const int k = k0 + tid;
        int flag = 0;
        long long l0 = 0, l1 = 0, l2 = 0, l3 = 0;
        if (k < Np) {
            const float ay = average_point[2 * k], ax = average_point[2 * k + 1];
            float b0 = (ay - y_scale[k] * 3.0f / 2.0f) * ps + margin;    // :1360-1363
            float b1 = (ay + y_scale[k] * 3.0f / 2.0f) * ps + margin;
            float b2 = (ax - x_scale[k] * 3.0f / 2.0f) * ps + margin;
            float b3 = (ax + x_scale[k] * 3.0f / 2.0f) * ps + margin;
            b0 = b0 >= 0 ? b0 : 0.0f;                                     // :1364
            b1 = b1 >= 0 ? b1 : 0.0f;
            b2 = b2 >= 0 ? b2 : 0.0f;
            b3 = b3 >= 0 ? b3 : 0.0f;
            b1 = (b1 < (float)(32 * height + 256)) ? b1 : board1;          // :1365
            b3 = (b3 < (float)(32 * width + 256)) ? b3 : board3;           // :1366
            xsn[2 * k] = (b1 - b0 + 1.0f) / 96.0f;                         // :1367
            xsn[2 * k + 1] = 1.0f;                                         // :1378-1381
            ysn[2 * k] = (b3 - b2 + 1.0f) / 96.0f;                         // :1368
            ysn[2 * k + 1] = 1.0f;
            l0 = (long long)b0; l1 = (long long)b1; l2 = (long long)b2; l3 = (long long)b3;  // :1369
            avn[2 * k + 1] = (float)(l1 + l0) / 2.0f - 128.0f + 0.5f;      // :1371
            avn[2 * k + 0] = (float)(l2 + l3) / 2.0f - 128.0f + 0.5f;      // :1372
            flag = ifn[k] ? 0 : 1;
        }
        // ordered compaction: ballot within the wave, scan of wave totals across the block
        const unsigned long long mask = __ballot(flag);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(mask);
        wg_barrier();
        int wbase = base_s;
        for (int q = 0; q < wave; ++q) wbase += wave_tot[q];
        if (flag) {
            const int64_t o = (int64_t)(wbase + before) * 5;
            bound5[o + 0] = l0; bound5[o + 1] = l1; bound5[o + 2] = l2; bound5[o + 3] = l3;
            bound5[o + 4] = (int64_t)img * 10000 + k;                      // :1374-1377
        }
        wg_barrier();
        if (tid == 0) {
            int tot = 0;
            for (int q = 0; q < 16; ++q) tot += wave_tot[q];
            base_s += tot;
        }
        wg_barrier();
    }
    if (tid == 0 && K_out) *K_out = base_s;
}

__global__ void __launch_bounds__(1024)
imgs_bounds_kernel(const float* __restrict__ x_scale, const float* __restrict__ y_scale,
                   const float* __restrict__ average_point, const uint8_t* __restrict__ ifn, int Np,
                   int height, int width, int img, int64_t* __restrict__ bound5,
                   int64_t* __restrict__ K_out, float* __restrict__ xsn, float* __restrict__ ysn,
                   float* __restrict__ avn) {
    imgs_bounds_block(x_scale, y_scale, average_point, ifn, Np, height, width, img, bound5, K_out, xsn, ysn, avn);
}

// A batch of images in one launch, no host-side counts: block i first sums the match flags of the
// images before it (its row offset into the compacted bound table; flags are one byte per patch, so
// even hundreds of images cost a few hundred KB of L2 reads), then compacts its own patches.
// K_img[i] = matches of image i; K_total (written by the last block) = rows of bound5 that are valid.
// A ragged batch (PairShapes::shape set): image i has its own grid and owns the packed cells [base(i), base(i) + ncell(i)).
__global__ void __launch_bounds__(1024)
imgs_bounds_batch_kernel(const float* __restrict__ x_scale, const float* __restrict__ y_scale,
                         const float* __restrict__ average_point, const uint8_t* __restrict__ ifn, PairShapes ps,
                         int64_t* __restrict__ bound5, int64_t* __restrict__ K_img,
                         int64_t* __restrict__ K_total, float* __restrict__ xsn, float* __restrict__ ysn,
                         float* __restrict__ avn) {
    __shared__ int part[16];
    __shared__ int64_t off_s;
    const int img = blockIdx.x, tid = threadIdx.x;
    const int64_t cb = ps.base(img);
    const int Np = (int)ps.ncell(img), height = ps.hp(img), width = ps.wp(img);
    int cnt = 0;
    for (int64_t k = tid; k < cb; k += 1024) cnt += ifn[k] ? 0 : 1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) part[tid >> 6] = cnt;
    wg_barrier();
    if (tid == 0) {
        int64_t o = 0;
        for (int q = 0; q < 16; ++q) o += part[q];
        off_s = o;
    }
    wg_barrier();
    const int64_t off = off_s;
    wg_barrier();
    const int64_t i = img;
    imgs_bounds_block(x_scale + cb, y_scale + cb, average_point + cb * 2, ifn + cb, Np, height, width,
                      img, bound5 + off * 5, K_img + i, xsn + cb * 2, ysn + cb * 2, avn + cb * 2);
    if (tid == 0 && img == (int)gridDim.x - 1 && K_total) *K_total = off + K_img[i];
}

// ---- element types and output formats of the crops ---------------------------------------------------------------------
// The crops read images of float32, float16, bfloat16 or uint8 elements (pats_img_dtype_t).  Every element is widened to
// fp32 EXACTLY at the load (each of those values is a float), and everything after the load is the fp32 code in its order
// (the taps, l0 / l1, the two-level lerp), so a crop computed in fp32 is the fp32 kernels' crop of images.float(), bit for
// bit.  The output format (pats_crop_format_t) then applies, per element and in fp32: the optional normalisation
// (x - mean[c]) / std[c] - a subtraction, then an IEEE division (torchvision's Normalize: sub_, then div_) - and ONE
// rounding to the output type at the store (round-to-nearest-even; plain conversions, v_cvt_pk_bf16_f32 for bf16).
// Layout hwc = [K,96,96,3], chw = [K,3,96,96].  The default format (fp32, hwc, no normalisation) on fp32 images is the
// instantiation the _f32 entry points launch; its code is the code those kernels always had.  bf16_t / widen_px: common.hpp.
template <typename T> __device__ __forceinline__ uint32_t narrow_bits(float v);                      // 2-byte outputs
template <> __device__ __forceinline__ uint32_t narrow_bits<_Float16>(float v) {
    return __builtin_bit_cast(uint16_t, (_Float16)v);
}
template <> __device__ __forceinline__ uint32_t narrow_bits<bf16_t>(float v) {
    return __builtin_bit_cast(uint16_t, (__bf16)v);
}
template <typename T> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    return narrow_bits<T>(lo) | (narrow_bits<T>(hi) << 16);
}

struct CropNorm {
    float mean[3], std[3];
};
__device__ __forceinline__ float sel3(const float (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }
template <bool NORM>
__device__ __forceinline__ float norm_px(float v, const CropNorm& nm, int c) {
    if (!NORM) return v;
    return (v - sel3(nm.mean, c)) / sel3(nm.std, c);
}

// four consecutive elements of a source row as fp32; the widest load the address allows (uint8 rows start at any byte)
template <typename TI>
__device__ __forceinline__ void load4(const TI* q, float (&v)[4]) {
    if (sizeof(TI) == 1) {
        if (((uintptr_t)q & 3) == 0) {
            const uint32_t u = *reinterpret_cast<const uint32_t*>(q);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (float)((u >> (8 * e)) & 0xffu);
            return;
        }
    } else if (sizeof(TI) == 2) {
        if (((uintptr_t)q & 7) == 0) {
            typedef uint32_t u2s __attribute__((ext_vector_type(2)));
            const u2s u = *reinterpret_cast<const u2s*>(q);
            const TI* h = reinterpret_cast<const TI*>(&u);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = widen_px(h + e);
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = widen_px(q + e);
}

// four consecutive output elements (16 / 8 / 4 bytes, aligned to their size)
template <typename TO, bool NT>
__device__ __forceinline__ void store4(TO* o, const float (&v)[4]) {
    if constexpr (sizeof(TO) == 4) {
        typedef float f4s __attribute__((ext_vector_type(4)));
        const f4s d = {v[0], v[1], v[2], v[3]};
        if (NT) __builtin_nontemporal_store(d, reinterpret_cast<f4s*>(o));
        else *reinterpret_cast<f4s*>(o) = d;
    } else if constexpr (sizeof(TO) == 2) {
        typedef uint32_t u2s __attribute__((ext_vector_type(2)));
        const u2s d = {pack2<TO>(v[0], v[1]), pack2<TO>(v[2], v[3])};
        if (NT) __builtin_nontemporal_store(d, reinterpret_cast<u2s*>(o));
        else *reinterpret_cast<u2s*>(o) = d;
    } else {                                          // uint8 left crops of uint8 images: exact copies
        const uint32_t d = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        if (NT) __builtin_nontemporal_store(d, reinterpret_cast<uint32_t*>(o));
        else *reinterpret_cast<uint32_t*>(o) = d;
    }
}

// ---- left crops: 96x96 windows on the fixed grid of the 32-px zero-padded left image ---------
template <typename TI, typename TO, bool CHW, bool NORM, bool NT>
__global__ void __launch_bounds__(288)
left_crops_kernel(const TI* __restrict__ left_all, int n_img, PairShapes ps, const int64_t* __restrict__ bound5,
                  TO* __restrict__ out, const int64_t* __restrict__ K_dev, CropNorm nm) {
    const int64_t k = blockIdx.x;
    if (K_dev && k >= *K_dev) return;          // launched over the capacity: rows past the device-side count
    const int64_t seq = bound5[k * 5 + 4];                 // img * 10000 + patch, utils.py:1374-1377
    const int patch = (int)(seq % 10000);
    const int64_t img = min(max(seq / 10000, (int64_t)0), (int64_t)n_img - 1);
    const int H = ps.Hpx(img), W = ps.Wpx(img), width = ps.wp(img);    // the image's own size: outside it is padding
    const TI* left = left_all + ps.img(img);
    const int r = patch / width, c = patch - r * width;
    // a row of the window is 288 contiguous elements of the source (or zeros): 72 lanes x 4 elements, four rows per pass of
    // the 288 threads; the source offset is only element-aligned in general (W * 3 elements per image row).
    // chw: lane j writes 4 pixels of channel j / 24 (24 lanes per channel row of a plane), read as 4 strided elements.
    const int t = threadIdx.x, j = t % 72, sub = t / 72;
    typedef float f4a __attribute__((ext_vector_type(4), aligned(4)));
    TO* o = out + k * (96 * 96 * 3);
    const int ix0 = c * 32 - 32;                // first source pixel of the row
    for (int y = blockIdx.y * 8 + sub; y < blockIdx.y * 8 + 8; y += 4) {
        const int iy = r * 32 + y - 32;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (CHW) {
            const int ch = j / 24, p0 = 4 * (j - 24 * ch);
            if (iy >= 0 && iy < H) {
                const TI* row = left + (int64_t)iy * W * 3;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int x = ix0 + p0 + q;
                    if (x >= 0 && x < W) v[q] = widen_px(row + 3 * x + ch);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = norm_px<NORM>(v[q], nm, ch);
            store4<TO, NT>(o + ch * (96 * 96) + y * 96 + p0, v);
            continue;
        }
        if (iy >= 0 && iy < H) {
            const TI* row = left + (int64_t)iy * W * 3;
            const int e0 = ix0 * 3 + 4 * j;                            // element offset inside the source row
            if (e0 >= 0 && e0 + 3 < W * 3) {
                if constexpr (sizeof(TI) == 4) {
                    const f4a u = *reinterpret_cast<const f4a*>(row + e0);
                    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
                } else {
                    load4(row + e0, v);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = e0 + q;
                    if (e >= 0 && e < W * 3) v[q] = widen_px(row + e);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = norm_px<NORM>(v[q], nm, (4 * j + q) % 3);
        store4<TO, NT>(o + y * 288 + 4 * j, v);
    }
}

// ---- tensor_resize ---------------------------------------------------------------------------
struct CropGeom {
    long long y0, x0, ih, iw, img;
    bool ok;
};
__device__ __forceinline__ CropGeom crop_geom(const int64_t* __restrict__ bound, int64_t i, int n_img,
                                              int Hp, int Wp) {
    CropGeom g;
    g.y0 = bound[i * 5];
    const long long y1 = bound[i * 5 + 1];
    g.x0 = bound[i * 5 + 2];
    const long long x1 = bound[i * 5 + 3];
    g.img = bound[i * 5 + 4] / 10000;            // library.cpp:55-56
    g.ih = y1 - g.y0;                            // narrow(1, y0, y1 - y0)        library.cpp:57-58
    g.iw = x1 - g.x0 + 1;                        // narrow(2, x0, x1 - x0 + 1)    library.cpp:58-59
    g.ok = g.ih > 0 && g.iw > 0 && g.y0 >= 0 && g.x0 >= 0 && g.y0 + g.ih <= Hp &&
           g.x0 + g.iw <= Wp && g.img >= 0 && g.img < n_img;
    return g;
}

// ATen upsample_bilinear2d(align_corners=true): scale = (in-1)/(out-1); src = scale * dst
struct Tap {
    int i1, ip;
    float l0, l1;
};
__device__ __forceinline__ Tap make_tap(float scale, int dst, long long in_size) {
    const float f = scale * (float)dst;
    Tap t;
    t.i1 = (int)f;
    t.ip = (t.i1 < in_size - 1) ? 1 : 0;
    t.l1 = f - (float)t.i1;
    t.l0 = 1.0f - t.l1;
    return t;
}

// CHW source (the padded tensor of utils.py:1352), CHW output [K,C,96,96].  2-byte outputs: two pixels per lane and pass,
// one dword store.  A bad crop is written as the format's value of a zero pixel.
template <typename TI, typename TO, bool NORM>
__global__ void __launch_bounds__(256)
resize_chw_kernel(const TI* __restrict__ input, int n_img, int C, int Hp, int Wp,
                  const int64_t* __restrict__ bound, TO* __restrict__ out,
                  int32_t* __restrict__ status, const int64_t* __restrict__ K_dev, CropNorm nm) {
    const int64_t i = blockIdx.x;
    if (K_dev && i >= *K_dev) return;
    const int c = blockIdx.y, slab = blockIdx.z;
    const CropGeom g = crop_geom(bound, i, n_img, Hp, Wp);
    TO* o = out + ((i * C + c) * 96) * 96;
    if (!g.ok) {
        if (status && threadIdx.x == 0) atomicOr(status, 1);
        if constexpr (sizeof(TO) == 4) {
            for (int idx = threadIdx.x; idx < 24 * 96; idx += 256) o[slab * 24 * 96 + idx] = norm_px<NORM>(0.f, nm, c);
        } else {
            const float z = norm_px<NORM>(0.f, nm, c);
            for (int idx = threadIdx.x; idx < 12 * 96; idx += 256)
                reinterpret_cast<uint32_t*>(o + slab * 24 * 96)[idx] = pack2<TO>(z, z);
        }
        return;
    }
    const float sh = (float)(g.ih - 1) / 95.0f, sw = (float)(g.iw - 1) / 95.0f;
    const TI* src = input + (((int64_t)g.img * C + c) * Hp + g.y0) * Wp + g.x0;
    auto px = [&](int idx) {
        const int oy = slab * 24 + idx / 96, ox = idx % 96;
        const Tap ty = make_tap(sh, oy, g.ih), tx = make_tap(sw, ox, g.iw);
        const TI* p = src + (int64_t)ty.i1 * Wp + tx.i1;
        const float p00 = widen_px(p), p01 = widen_px(p + tx.ip), p10 = widen_px(p + (int64_t)ty.ip * Wp),
                    p11 = widen_px(p + (int64_t)ty.ip * Wp + tx.ip);
        return norm_px<NORM>(ty.l0 * (tx.l0 * p00 + tx.l1 * p01) + ty.l1 * (tx.l0 * p10 + tx.l1 * p11), nm, c);
    };
    if constexpr (sizeof(TO) == 4) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const int idx = threadIdx.x + 256 * q;
            const int oy = slab * 24 + idx / 96, ox = idx % 96;
            const Tap ty = make_tap(sh, oy, g.ih), tx = make_tap(sw, ox, g.iw);
            const TI* p = src + (int64_t)ty.i1 * Wp + tx.i1;
            const float p00 = widen_px(p), p01 = widen_px(p + tx.ip), p10 = widen_px(p + (int64_t)ty.ip * Wp),
                        p11 = widen_px(p + (int64_t)ty.ip * Wp + tx.ip);
            o[oy * 96 + ox] = norm_px<NORM>(ty.l0 * (tx.l0 * p00 + tx.l1 * p01) + ty.l1 * (tx.l0 * p10 + tx.l1 * p11), nm, c);
        }
    } else {
        for (int pr = threadIdx.x; pr < 12 * 96; pr += 256)
            reinterpret_cast<uint32_t*>(o + slab * 24 * 96)[pr] = pack2<TO>(px(2 * pr), px(2 * pr + 1));
    }
}

// HWC unpadded source [n_img,H,W,3] with a virtual zero margin, HWC output [K,96,96,3]:
// fuses F.pad (utils.py:1352), the NCHW permute and the caller's permute(0,2,3,1) (utils.py:1385).
// Other formats: fp32 one pixel per lane and pass (chw: three 4-byte stores, one per plane); 2-byte outputs two pixels per
// lane and pass, so that every store is whole dwords (hwc: 12 bytes = 6 halves, chw: one dword per plane).
template <typename TI, typename TO, bool CHW, bool NORM, bool NT>
__global__ void __launch_bounds__(256)
resize_hwc_kernel(const TI* __restrict__ right, int n_img, PairShapes ps, int margin,
                  const int64_t* __restrict__ bound, TO* __restrict__ out,
                  int32_t* __restrict__ status, const int64_t* __restrict__ K_dev, CropNorm nm) {
    constexpr bool F32HWC = sizeof(TO) == 4 && !CHW;
    constexpr int PX = sizeof(TO) == 4 ? 1 : 2;          // pixels per lane and pass
    const int64_t i = blockIdx.x;
    if (K_dev && i >= *K_dev) return;
    const int slab = blockIdx.y;
    const int64_t im = min(max(bound[i * 5 + 4] / 10000, (int64_t)0), (int64_t)n_img - 1);   // an index outside: !g.ok below
    const int H = ps.Hpx(im), W = ps.Wpx(im);
    const int Hp = H + 2 * margin, Wp = W + 2 * margin;
    const CropGeom g = crop_geom(bound, i, n_img, Hp, Wp);
    TO* o = out + i * (96 * 96 * 3);
    typedef float f3a __attribute__((ext_vector_type(3), aligned(4)));
    typedef uint32_t u3a __attribute__((ext_vector_type(3), aligned(4)));
    // PX pixels (oy, ox0 + u) of fp32 channel values -> the output
    auto put = [&](int oy, int ox0, const float (&d)[PX][3]) {
        if constexpr (F32HWC) {
            const f3a v = {norm_px<NORM>(d[0][0], nm, 0), norm_px<NORM>(d[0][1], nm, 1), norm_px<NORM>(d[0][2], nm, 2)};
            f3a* dp = reinterpret_cast<f3a*>(o + oy * 288 + 3 * ox0);   // one 12-byte store: a wave's 64 pixels are 768 contiguous bytes
            if (NT) __builtin_nontemporal_store(v, dp);
            else *dp = v;
        } else if constexpr (sizeof(TO) == 4) {                           // fp32 chw
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float* dp = o + ch * (96 * 96) + oy * 96 + ox0;
                const float v = norm_px<NORM>(d[0][ch], nm, ch);
                if (NT) __builtin_nontemporal_store(v, dp);
                else *dp = v;
            }
        } else if constexpr (!CHW) {                                      // 2-byte hwc: 6 halves = 3 dwords
            float n[6];
#pragma unroll
            for (int e = 0; e < 6; ++e) n[e] = norm_px<NORM>(d[e / 3][e % 3], nm, e % 3);
            const u3a v = {pack2<TO>(n[0], n[1]), pack2<TO>(n[2], n[3]), pack2<TO>(n[4], n[5])};
            u3a* dp = reinterpret_cast<u3a*>(o + oy * 288 + 3 * ox0);
            if (NT) __builtin_nontemporal_store(v, dp);
            else *dp = v;
        } else {                                                          // 2-byte chw: one dword per plane
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                uint32_t* dp = reinterpret_cast<uint32_t*>(o + ch * (96 * 96) + oy * 96 + ox0);
                const uint32_t v = pack2<TO>(norm_px<NORM>(d[0][ch], nm, ch), norm_px<NORM>(d[1][ch], nm, ch));
                if (NT) __builtin_nontemporal_store(v, dp);
                else *dp = v;
            }
        }
    };
    if (!g.ok) {
        if (status && threadIdx.x == 0) atomicOr(status, 1);
        if constexpr (F32HWC && !NORM) {
            for (int idx = threadIdx.x; idx < 24 * 288; idx += 256) o[slab * 24 * 288 + idx] = 0.f;
        } else {
            const float z[PX][3] = {};
            for (int px = threadIdx.x; px < 24 * 96 / PX; px += 256) put(slab * 24 + (PX * px) / 96, (PX * px) % 96, z);
        }
        return;
    }
    const float sh = (float)(g.ih - 1) / 95.0f, sw = (float)(g.iw - 1) / 95.0f;
    const TI* img = right + ps.img(g.img);
    // one output PIXEL per thread and pass (taps, bounds tests and addresses once for the three channels; the three
    // elements of a tap are contiguous); coordinates fit 32 bits once the crop geometry has been validated
    const int y0 = (int)g.y0 - margin, x0 = (int)g.x0 - margin, ih = (int)g.ih, iw = (int)g.iw;
    struct Px { float r, g, b; };
    auto at = [&](int y, int x) {
        Px v{0.f, 0.f, 0.f};
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const TI* q = img + ((int64_t)y * W + x) * 3;
            v.r = widen_px(q); v.g = widen_px(q + 1); v.b = widen_px(q + 2);
        }
        return v;
    };
    auto pixel = [&](int oy, int ox, float (&d)[3]) {
        const Tap ty = make_tap(sh, oy, ih), tx = make_tap(sw, ox, iw);
        const int y = y0 + ty.i1, x = x0 + tx.i1;
        const Px p00 = at(y, x), p01 = at(y, x + tx.ip), p10 = at(y + ty.ip, x), p11 = at(y + ty.ip, x + tx.ip);
        d[0] = ty.l0 * (tx.l0 * p00.r + tx.l1 * p01.r) + ty.l1 * (tx.l0 * p10.r + tx.l1 * p11.r);
        d[1] = ty.l0 * (tx.l0 * p00.g + tx.l1 * p01.g) + ty.l1 * (tx.l0 * p10.g + tx.l1 * p11.g);
        d[2] = ty.l0 * (tx.l0 * p00.b + tx.l1 * p01.b) + ty.l1 * (tx.l0 * p10.b + tx.l1 * p11.b);
    };
    if constexpr (F32HWC && !NORM) {          // the default format: one 12-byte store per pixel, as it always was
        for (int px = threadIdx.x; px < 24 * 96; px += 256) {
            const int oy = slab * 24 + px / 96, ox = px % 96;
            const Tap ty = make_tap(sh, oy, ih), tx = make_tap(sw, ox, iw);
            const int y = y0 + ty.i1, x = x0 + tx.i1;
            const Px p00 = at(y, x), p01 = at(y, x + tx.ip), p10 = at(y + ty.ip, x), p11 = at(y + ty.ip, x + tx.ip);
            const f3a d = {ty.l0 * (tx.l0 * p00.r + tx.l1 * p01.r) + ty.l1 * (tx.l0 * p10.r + tx.l1 * p11.r),
                           ty.l0 * (tx.l0 * p00.g + tx.l1 * p01.g) + ty.l1 * (tx.l0 * p10.g + tx.l1 * p11.g),
                           ty.l0 * (tx.l0 * p00.b + tx.l1 * p01.b) + ty.l1 * (tx.l0 * p10.b + tx.l1 * p11.b)};
            f3a* dp = reinterpret_cast<f3a*>(o + oy * 288 + 3 * ox);       // a wave's 64 pixels are 768 contiguous bytes
            if (NT) __builtin_nontemporal_store(d, dp);
            else *dp = d;
        }
        return;
    }
    for (int px = threadIdx.x; px < 24 * 96 / PX; px += 256) {
        const int oy = slab * 24 + (PX * px) / 96, ox0 = (PX * px) % 96;
        float d[PX][3];
#pragma unroll
        for (int u = 0; u < PX; ++u) pixel(oy, ox0 + u, d[u]);
        put(oy, ox0, d);
    }
}

// the crops are written once and read by another kernel much later (2.3 GB per side and step): non-temporal stores of whole
// lines (see gather.hip).  PATS_CROPS_NT = 0 / 1, read once per process; it applies to every format.
static bool crops_nt() {
    static const bool nt = [] { const char* e = env_switch("PATS_CROPS_NT"); return e ? atoi(e) != 0 : PATS_CROPS_NT_DEFAULT != 0; }();
    return nt;
}

// run f(bool_constant<a>, bool_constant<b>, bool_constant<c>)
template <typename F>
static void with_flags(bool a, bool b, bool c, F&& f) {
    using T = std::true_type;
    using N = std::false_type;
    if (a) {
        if (b) { if (c) f(T{}, T{}, T{}); else f(T{}, T{}, N{}); }
        else { if (c) f(T{}, N{}, T{}); else f(T{}, N{}, N{}); }
    } else {
        if (b) { if (c) f(N{}, T{}, T{}); else f(N{}, T{}, N{}); }
        else { if (c) f(N{}, N{}, T{}); else f(N{}, N{}, N{}); }
    }
}

struct Fmt {
    int out;           // pats_img_dtype_t of the output
    bool chw, norm;
    CropNorm nm;
};
static const Fmt kF32Hwc = {PATS_IMG_F32, false, false, {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}}};

template <typename T> struct tag { using type = T; };
// f(tag<element type>) for a pats_img_dtype_t (validated before)
template <typename F>
static void with_dtype(int dt, F&& f) {
    switch (dt) {
        case PATS_IMG_F16: f(tag<_Float16>{}); break;
        case PATS_IMG_BF16: f(tag<bf16_t>{}); break;
        case PATS_IMG_U8: f(tag<uint8_t>{}); break;
        default: f(tag<float>{}); break;
    }
}

template <typename TI>
static int launch_left_crops(const TI* left, int n_img, const PairShapes& ps, const int64_t* bound5, int64_t K,
                             const int64_t* K_dev, const Fmt& f, void* out, hipStream_t st) {
    auto go = [&](auto to) {
        using TO = typename decltype(to)::type;
        with_flags(f.chw, f.norm, crops_nt(), [&](auto chw, auto norm, auto nt) {
            hipLaunchKernelGGL((left_crops_kernel<TI, TO, decltype(chw)::value, decltype(norm)::value, decltype(nt)::value>),
                               dim3((unsigned)K, 12), dim3(288), 0, st, left, n_img, ps, bound5, static_cast<TO*>(out), K_dev,
                               f.nm);
        });
    };
    if constexpr (std::is_same<TI, uint8_t>::value) {
        if (f.out == PATS_IMG_U8) go(tag<uint8_t>{});
        else with_dtype(f.out, go);
    } else {
        with_dtype(f.out, go);          // uint8 output of other images is refused by check_format
    }
    return check_launch("left_crops_kernel");
}

template <typename TI>
static int launch_resize_hwc(const TI* right, int n_img, const PairShapes& ps, int margin, const int64_t* bound, int64_t K,
                             const int64_t* K_dev, const Fmt& f, void* out, int32_t* status, hipStream_t st) {
    with_dtype(f.out, [&](auto to) {
        using TO = typename decltype(to)::type;
        if constexpr (!std::is_same<TO, uint8_t>::value) {          // uint8 right crops are refused by check_format
            with_flags(f.chw, f.norm, crops_nt(), [&](auto chw, auto norm, auto nt) {
                hipLaunchKernelGGL((resize_hwc_kernel<TI, TO, decltype(chw)::value, decltype(norm)::value, decltype(nt)::value>),
                                   dim3((unsigned)K, 4), dim3(256), 0, st, right, n_img, ps, margin, bound, static_cast<TO*>(out),
                                   status, K_dev, f.nm);
            });
        }
    });
    return check_launch("resize_hwc_kernel");
}

template <typename TI>
static int launch_resize_chw(const TI* input, int n_img, int C, int Hp, int Wp, const int64_t* bound, int64_t K,
                             const int64_t* K_dev, const Fmt& f, void* out, int32_t* status, hipStream_t st) {
    with_dtype(f.out, [&](auto to) {
        using TO = typename decltype(to)::type;
        if constexpr (!std::is_same<TO, uint8_t>::value) {
            with_flags(f.norm, false, false, [&](auto norm, auto, auto) {
                hipLaunchKernelGGL((resize_chw_kernel<TI, TO, decltype(norm)::value>), dim3((unsigned)K, (unsigned)C, 4), dim3(256),
                                   0, st, input, n_img, C, Hp, Wp, bound, static_cast<TO*>(out), status, K_dev, f.nm);
            });
        }
    });
    return check_launch("resize_chw_kernel");
}

static size_t elem_bytes(int dt) { return dt == PATS_IMG_U8 ? 1 : (dt == PATS_IMG_F32 ? 4 : 2); }

// the refusals of the typed entry points (include/pats_amd.h), before any launch
static int check_format(const pats_crop_format_t* fmt, int in_dtype, bool left, Fmt* f, const char* what) {
    PATS_REQUIRE(in_dtype >= PATS_IMG_F32 && in_dtype <= PATS_IMG_U8, "%s: unknown image dtype %d", what, in_dtype);
    PATS_REQUIRE(fmt, "%s: null pointer (crop format)", what);
    PATS_REQUIRE(fmt->dtype >= PATS_IMG_F32 && fmt->dtype <= PATS_IMG_U8, "%s: unknown crop dtype %d", what, (int)fmt->dtype);
    PATS_REQUIRE(fmt->layout == PATS_CROP_HWC || fmt->layout == PATS_CROP_CHW, "%s: unknown crop layout %d", what, (int)fmt->layout);
    if (fmt->dtype == PATS_IMG_U8) {
        PATS_REQUIRE(left, "%s: uint8 output is for left crops only", what);
        PATS_REQUIRE(in_dtype == PATS_IMG_U8, "%s: uint8 output needs uint8 images", what);
        PATS_REQUIRE(!fmt->normalize, "%s: uint8 output cannot be normalised", what);
    }
    if (fmt->normalize) {
        for (int c = 0; c < 3; ++c)
            PATS_REQUIRE(std::isfinite(fmt->mean[c]) && std::isfinite(fmt->std[c]) && fmt->std[c] != 0.f,
                         "%s: normalisation needs a finite mean and a finite, non-zero std (channel %d)", what, c);
    }
    f->out = fmt->dtype;
    f->chw = fmt->layout == PATS_CROP_CHW;
    f->norm = fmt->normalize != 0;
    for (int c = 0; c < 3; ++c) {
        f->nm.mean[c] = f->norm ? fmt->mean[c] : 0.f;
        f->nm.std[c] = f->norm ? fmt->std[c] : 1.f;
    }
    return PATS_OK;
}

static int check_ptrs(const void* img, int in_dtype, const void* out, const char* what) {
    PATS_REQUIRE((uintptr_t)img % elem_bytes(in_dtype) == 0, "%s: images must be %d-byte aligned", what, (int)elem_bytes(in_dtype));
    PATS_REQUIRE((uintptr_t)out % 16 == 0, "%s: out must be 16-byte aligned", what);
    return PATS_OK;
}

}  // namespace pats

using namespace pats;

extern "C" int pats_compute_imgs_bounds_f32(const float* x_scale, const float* y_scale,
                                            const float* average_point, const uint8_t* if_nomatching,
                                            int Np, int height, int width, int img, int64_t* bound5,
                                            int64_t* K_out, float* x_scale_new, float* y_scale_new,
                                            float* average_new, pats_stream_t stream) {
    PATS_REQUIRE(Np > 0 && height > 0 && width > 0, "compute_imgs_bounds: bad shape");
    PATS_REQUIRE(x_scale && y_scale && average_point && if_nomatching && bound5 && K_out &&
                     x_scale_new && y_scale_new && average_new, "compute_imgs_bounds: null pointer");
    hipLaunchKernelGGL(imgs_bounds_kernel, dim3(1), dim3(1024), 0, as_stream(stream), x_scale,
                       y_scale, average_point, if_nomatching, Np, height, width, img, bound5, K_out,
                       x_scale_new, y_scale_new, average_new);
    return check_launch("imgs_bounds_kernel");
}

extern "C" int pats_left_crops_f32(const float* left, int n_img, int H, int W, const int64_t* bound5, int64_t K,
                                   int height, int width, float* out, pats_stream_t stream) {
    PATS_REQUIRE(K >= 0 && n_img > 0 && H > 0 && W > 0 && height > 0 && width > 0, "left_crops: bad shape");
    if (K == 0) return PATS_OK;
    PATS_REQUIRE(left && bound5 && out, "left_crops: null pointer");
    return launch_left_crops(left, n_img, uniform_shapes(n_img, height, width, 0, H, W), bound5, K, nullptr, kF32Hwc, out,
                             as_stream(stream));
}

extern "C" int pats_compute_imgs_bounds_batch_f32(const float* x_scale, const float* y_scale,
                                                  const float* average_point, const uint8_t* if_nomatching,
                                                  int n_img, int Np, int height, int width, int64_t* bound5,
                                                  int64_t* K_img, int64_t* K_total, float* x_scale_new,
                                                  float* y_scale_new, float* average_new, pats_stream_t stream) {
    PATS_REQUIRE(n_img > 0 && n_img <= 10000 && Np > 0 && height > 0 && width > 0, "compute_imgs_bounds_batch: bad shape");
    PATS_REQUIRE(x_scale && y_scale && average_point && if_nomatching && bound5 && K_img && x_scale_new &&
                     y_scale_new && average_new, "compute_imgs_bounds_batch: null pointer");
    hipLaunchKernelGGL(imgs_bounds_batch_kernel, dim3((unsigned)n_img), dim3(1024), 0, as_stream(stream), x_scale,
                       y_scale, average_point, if_nomatching, uniform_shapes(n_img, height, width, Np), bound5, K_img, K_total,
                       x_scale_new, y_scale_new, average_new);
    return check_launch("imgs_bounds_batch_kernel");
}

extern "C" int pats_left_crops_counted_f32(const float* left, int n_img, int H, int W, const int64_t* bound5,
                                           int64_t K_cap, const int64_t* K_dev, int height, int width, float* out,
                                           pats_stream_t stream) {
    PATS_REQUIRE(K_cap >= 0 && n_img > 0 && H > 0 && W > 0 && height > 0 && width > 0, "left_crops_counted: bad shape");
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(left && bound5 && out && K_dev, "left_crops_counted: null pointer");
    return launch_left_crops(left, n_img, uniform_shapes(n_img, height, width, 0, H, W), bound5, K_cap, K_dev, kF32Hwc, out,
                             as_stream(stream));
}

extern "C" int pats_tensor_resize_f32(const float* input, int n_img, int C, int Hp, int Wp,
                                      const int64_t* bound, int64_t K, float* out, int32_t* status,
                                      pats_stream_t stream) {
    PATS_REQUIRE(K >= 0 && n_img > 0 && C > 0 && Hp > 0 && Wp > 0, "tensor_resize: bad shape");
    if (K == 0) return PATS_OK;     // empty [0,C,96,96] result, like the reference when nothing matches
    PATS_REQUIRE(input && bound && out, "tensor_resize: null pointer");
    PATS_REQUIRE(C <= 65535, "tensor_resize: too many channels");
    return launch_resize_chw(input, n_img, C, Hp, Wp, bound, K, nullptr, kF32Hwc, out, status, as_stream(stream));
}

extern "C" int pats_tensor_resize_hwc_f32(const float* right, int n_img, int H, int W, int margin,
                                          const int64_t* bound, int64_t K, float* out,
                                          int32_t* status, pats_stream_t stream) {
    PATS_REQUIRE(K >= 0 && n_img > 0 && H > 0 && W > 0 && margin >= 0, "tensor_resize_hwc: bad shape");
    if (K == 0) return PATS_OK;
    PATS_REQUIRE(right && bound && out, "tensor_resize_hwc: null pointer");
    return launch_resize_hwc(right, n_img, uniform_shapes(n_img, H / 32, W / 32, 0, H, W), margin, bound, K, nullptr, kF32Hwc, out,
                             status, as_stream(stream));
}

extern "C" int pats_tensor_resize_hwc_counted_f32(const float* right, int n_img, int H, int W, int margin,
                                                  const int64_t* bound, int64_t K_cap, const int64_t* K_dev,
                                                  float* out, int32_t* status, pats_stream_t stream) {
    PATS_REQUIRE(K_cap >= 0 && n_img > 0 && H > 0 && W > 0 && margin >= 0, "tensor_resize_hwc_counted: bad shape");
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(right && bound && out && K_dev, "tensor_resize_hwc_counted: null pointer");
    return launch_resize_hwc(right, n_img, uniform_shapes(n_img, H / 32, W / 32, 0, H, W), margin, bound, K_cap, K_dev, kF32Hwc,
                             out, status, as_stream(stream));
}

// ---- ragged batches: the same three kernels, each pair on its own grid and image (include/pats_amd.h) ----
extern "C" int pats_compute_imgs_bounds_ragged_f32(const pats_pair_table_t* tab, const float* x_scale, const float* y_scale,
                                                   const float* average_point, const uint8_t* if_nomatching, int64_t* bound5,
                                                   int64_t* K_img, int64_t* K_total, float* x_scale_new, float* y_scale_new,
                                                   float* average_new, pats_stream_t stream) {
    PairShapes ps;
    const int rc = ragged_shapes(tab, &ps, nullptr, "compute_imgs_bounds_ragged");
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(ps.pairs <= 10000, "compute_imgs_bounds_ragged: more than 10000 images");
    PATS_REQUIRE(x_scale && y_scale && average_point && if_nomatching && bound5 && K_img && x_scale_new && y_scale_new && average_new,
                 "compute_imgs_bounds_ragged: null pointer");
    hipLaunchKernelGGL(imgs_bounds_batch_kernel, dim3((unsigned)ps.pairs), dim3(1024), 0, as_stream(stream), x_scale, y_scale,
                       average_point, if_nomatching, ps, bound5, K_img, K_total, x_scale_new, y_scale_new, average_new);
    return check_launch("imgs_bounds_batch_kernel");
}

extern "C" int pats_left_crops_ragged_f32(const pats_pair_table_t* tab, const float* left, const int64_t* bound5, int64_t K_cap,
                                          const int64_t* K_dev, float* out, pats_stream_t stream) {
    PairShapes ps;
    const int rc = ragged_shapes(tab, &ps, nullptr, "left_crops_ragged");
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(K_cap >= 0 && K_cap < (1ll << 31), "left_crops_ragged: bad K_cap");
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(left && bound5 && out && K_dev, "left_crops_ragged: null pointer");
    return launch_left_crops(left, (int)ps.pairs, ps, bound5, K_cap, K_dev, kF32Hwc, out, as_stream(stream));
}

extern "C" int pats_tensor_resize_hwc_ragged_f32(const pats_pair_table_t* tab, const float* right, int margin, const int64_t* bound5,
                                                 int64_t K_cap, const int64_t* K_dev, float* out, int32_t* status,
                                                 pats_stream_t stream) {
    PairShapes ps;
    const int rc = ragged_shapes(tab, &ps, nullptr, "tensor_resize_hwc_ragged");
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(K_cap >= 0 && K_cap < (1ll << 31) && margin >= 0, "tensor_resize_hwc_ragged: bad shape");
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(right && bound5 && out && K_dev, "tensor_resize_hwc_ragged: null pointer");
    return launch_resize_hwc(right, (int)ps.pairs, ps, margin, bound5, K_cap, K_dev, kF32Hwc, out, status, as_stream(stream));
}

// ---- the crops on images of any pats_img_dtype_t, written in any pats_crop_format_t (include/pats_amd.h) ----
static int shapes_of(const pats_pair_table_t* tab, int n_img, int height, int width, int H, int W, PairShapes* ps, int* pairs,
                     const char* what) {
    if (tab) {
        const int rc = ragged_shapes(tab, ps, nullptr, what);
        if (rc != PATS_OK) return rc;
        *pairs = (int)ps->pairs;
        return PATS_OK;
    }
    PATS_REQUIRE(n_img > 0 && H > 0 && W > 0 && height > 0 && width > 0, "%s: bad shape", what);
    *ps = uniform_shapes(n_img, height, width, 0, H, W);
    *pairs = n_img;
    return PATS_OK;
}

extern "C" int pats_left_crops_typed(const pats_pair_table_t* tab, const void* left, pats_img_dtype_t dtype, int n_img, int H, int W,
                                     int height, int width, const int64_t* bound5, int64_t K_cap, const int64_t* K_dev,
                                     const pats_crop_format_t* fmt, void* out, pats_stream_t stream) {
    const char* what = "left_crops_typed";
    Fmt f;
    int rc = check_format(fmt, dtype, true, &f, what);
    if (rc != PATS_OK) return rc;
    PairShapes ps;
    int pairs = 0;
    rc = shapes_of(tab, n_img, height, width, H, W, &ps, &pairs, what);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(K_cap >= 0 && K_cap < (1ll << 31), "%s: bad K_cap", what);
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(left && bound5 && out, "%s: null pointer", what);
    rc = check_ptrs(left, dtype, out, what);
    if (rc != PATS_OK) return rc;
    with_dtype(dtype, [&](auto ti) {
        using TI = typename decltype(ti)::type;
        rc = launch_left_crops(static_cast<const TI*>(left), pairs, ps, bound5, K_cap, K_dev, f, out, as_stream(stream));
    });
    return rc;
}

extern "C" int pats_tensor_resize_hwc_typed(const pats_pair_table_t* tab, const void* right, pats_img_dtype_t dtype, int n_img, int H,
                                            int W, int margin, const int64_t* bound5, int64_t K_cap, const int64_t* K_dev,
                                            const pats_crop_format_t* fmt, void* out, int32_t* status, pats_stream_t stream) {
    const char* what = "tensor_resize_hwc_typed";
    Fmt f;
    int rc = check_format(fmt, dtype, false, &f, what);
    if (rc != PATS_OK) return rc;
    PairShapes ps;
    int pairs = 0;
    rc = shapes_of(tab, n_img, H / 32, W / 32, H, W, &ps, &pairs, what);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(K_cap >= 0 && K_cap < (1ll << 31) && margin >= 0, "%s: bad shape", what);
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(right && bound5 && out, "%s: null pointer", what);
    rc = check_ptrs(right, dtype, out, what);
    if (rc != PATS_OK) return rc;
    with_dtype(dtype, [&](auto ti) {
        using TI = typename decltype(ti)::type;
        rc = launch_resize_hwc(static_cast<const TI*>(right), pairs, ps, margin, bound5, K_cap, K_dev, f, out, status,
                               as_stream(stream));
    });
    return rc;
}

extern "C" int pats_tensor_resize_typed(const void* input, pats_img_dtype_t dtype, int n_img, int C, int Hp, int Wp,
                                        const int64_t* bound, int64_t K_cap, const int64_t* K_dev, const pats_crop_format_t* fmt,
                                        void* out, int32_t* status, pats_stream_t stream) {
    const char* what = "tensor_resize_typed";
    Fmt f;
    int rc = check_format(fmt, dtype, false, &f, what);
    if (rc != PATS_OK) return rc;
    PATS_REQUIRE(fmt->layout == PATS_CROP_CHW, "%s: the output of tensor_resize is [K,C,96,96]: layout must be chw", what);
    PATS_REQUIRE(K_cap >= 0 && K_cap < (1ll << 31) && n_img > 0 && C > 0 && Hp > 0 && Wp > 0, "%s: bad shape", what);
    PATS_REQUIRE(C <= 65535, "%s: too many channels", what);
    PATS_REQUIRE(!f.norm || C == 3, "%s: normalisation needs C == 3, got %d", what, C);
    if (K_cap == 0) return PATS_OK;
    PATS_REQUIRE(input && bound && out, "%s: null pointer", what);
    rc = check_ptrs(input, dtype, out, what);
    if (rc != PATS_OK) return rc;
    with_dtype(dtype, [&](auto ti) {
        using TI = typename decltype(ti)::type;
        rc = launch_resize_chw(static_cast<const TI*>(input), n_img, C, Hp, Wp, bound, K_cap, K_dev, f, out, status,
                               as_stream(stream));
    });
    return rc;
}
