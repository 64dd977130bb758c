// The fp16-split contraction's primitives: THE home of the split's constants, vector types and small device functions.
//
// The contract.  An fp32 operand x enters the matrix pipe as two fp16 halves, x * 2^6 = hi + lo (both round-to-nearest, so the pair
// carries 22 mantissa bits).  A product takes THREE exact-product MFMA passes with fp32 accumulation, the small terms first
// (lo.hi, hi.lo, then hi.hi); lo.lo <= 2^-22 |x y| is dropped.  Accumulators come out scaled by 2^12 and UNS undoes that exactly.
// The fp16 range is the price: |x| > 1023 makes hi infinite (every user detects that and redoes the work in fp32), and the matrix
// pipe flushes fp16 subnormals, so below |x| = 0.004 an operand is carried with an absolute error <= 2^-20.
// The model that tests this contract - the "keep / flush" study of the subnormal halves and what another pre-scale does to the
// error - is tests/attention_cases.py::split_model, written up in docs/parity.md ("Attention cores on non-uniform softmax rows").
//
// Left apart on purpose: mfma_tile.hpp::split2 (two channels, the residual by an fma on the value before the pre-scale) and
// cost65_device.hpp::split_pair (a packed pair of columns) are not split4 (four channels, subtracting from the scaled value) -
// other instruction sequences, which their kernels were tuned with; they share the constants only.  The load4 of gnn_fused.hip (four scalar loads) and of gnn_fine.hip (one 16-byte load) have different alignment
// contracts, and the two store_tf write different layouts: all four stay in their files.
#pragma once
#include "common.hpp"

namespace pats {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
// explicitly GLOBAL: the integer round trip of uniform_ptr() would otherwise leave a generic pointer and flat_load (which also
// counts on lgkmcnt)
typedef const __attribute__((address_space(1))) h8v* gptr_h8;

constexpr float PRE = 64.0f;                  // 1023 * 64 < 65504, the largest fp16
constexpr float UNS = 1.0f / (PRE * PRE);     // 1 / 4096: exact power of two

__device__ __forceinline__ void split4(const f4v v, h4v& hi, h4v& lo) {
    const f4v s = v * PRE;
    hi = __builtin_convertvector(s, h4v);
    lo = __builtin_convertvector(s - __builtin_convertvector(hi, f4v), h4v);
}
// the same for a value that already carries the factor PRE (the epilogues fold it - a power of two - into their one fma)
__device__ __forceinline__ void split4_pre(const f4v s, h4v& hi, h4v& lo) {
    hi = __builtin_convertvector(s, h4v);
    lo = __builtin_convertvector(s - __builtin_convertvector(hi, f4v), h4v);
}
__device__ __forceinline__ void split8(const f4v a, const f4v b, h8v& hi, h8v& lo) {
    h4v ah, al, bh, bl;
    split4(a, ah, al);
    split4(b, bh, bl);
    hi = h8v{ah.x, ah.y, ah.z, ah.w, bh.x, bh.y, bh.z, bh.w};
    lo = h8v{al.x, al.y, al.z, al.w, bl.x, bl.y, bl.z, bl.w};
}
__device__ __forceinline__ f4v mfma3(const h8v ah, const h8v al, const h8v bh, const h8v bl, f4v c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);       // small terms first
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
}
__device__ __forceinline__ f4v fma4(const f4v a, const f4v b, const f4v c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f4v bcast4(float x) { return f4v{x, x, x, x}; }

// A weight fragment's address is wave-uniform + lane * 16: the uniform part is forced into SGPRs (readfirstlane), so that a load is
// `global_load_dwordx4 v, v_lane, s[base] offset:0 | 1024`.  Left to itself the compiler kept one 64-bit VECTOR address per
// load, spilled them, and every reload put an s_waitcnt vmcnt(0) in front of the next weight load - no prefetch at all.
__device__ __forceinline__ gptr_h8 uniform_ptr(const h8v* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (gptr_h8)(((uint64_t)hi << 32) | lo);
}

}  // namespace pats
