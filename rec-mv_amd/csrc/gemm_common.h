// Device helpers that both halves of the f32 products use: gemm_f32.hip (NT) and gemm_tn.hip (TN).
// Everything sits in an anonymous namespace, like the kernels that use it.
#pragma once
#include "common.h"
#include "gemm_route.h"
#include "activation.h"

namespace recmv {
using route::BM;      // large NT tile and the TN kernels' tile
using route::BN;
using route::BK;
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- 3-way bf16 split of f32 operands (optional matrix mode "bf16x6") ------------------------------------------
// x = h + m + l exactly, each piece a bf16 (round-to-nearest at every step: |m| <= 2^-9 |x|, |l| <= 2^-17 |x|).
// A product x*y is then formed from the six piece products of weight >= 2^-18 (hh, hm, mh, hl, lh, mm) on the bf16
// matrix pipe (16x the f32 matrix rate) with f32 accumulation; the dropped products are <= 2^-25 relative, below
// f32 rounding.  Each piece product is exact in f32, so the result differs from the f32 MFMA only by the order of
// the f32 accumulation.
struct Pieces {
  bf16x8 h, m, l;
};
// Two f32 -> one packed pair of bf16, round to nearest even.  Default: the hardware conversion (v_cvt_pk_bf16_f32, new in gfx950).
// -DRECMV_SPLIT_INT: the same rounding in integer arithmetic (finite operands; the A/B build of tools/def_regu_stress.py).
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
#ifdef RECMV_SPLIT_INT
  unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  ua += 0x7fffu + ((ua >> 16) & 1u);
  ub += 0x7fffu + ((ub >> 16) & 1u);
  return (ua >> 16) | (ub & 0xffff0000u);
#else
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
#endif
}
__device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = pack_bf16(x0, x1);
  const f32x2 r = {x0 - __uint_as_float(h << 16), x1 - __uint_as_float(h & 0xffff0000u)};
  m = pack_bf16(r.x, r.y);
  const f32x2 q = {r.x - __uint_as_float(m << 16), r.y - __uint_as_float(m & 0xffff0000u)};
  l = pack_bf16(q.x, q.y);
}
__device__ __forceinline__ Pieces split8(float4 a, float4 b) {
  unsigned h[4], m[4], l[4];
  split2(a.x, a.y, h[0], m[0], l[0]);
  split2(a.z, a.w, h[1], m[1], l[1]);
  split2(b.x, b.y, h[2], m[2], l[2]);
  split2(b.z, b.w, h[3], m[3], l[3]);
  Pieces p;
  p.h = __builtin_bit_cast(bf16x8, (u32x4){h[0], h[1], h[2], h[3]});
  p.m = __builtin_bit_cast(bf16x8, (u32x4){m[0], m[1], m[2], m[3]});
  p.l = __builtin_bit_cast(bf16x8, (u32x4){l[0], l[1], l[2], l[3]});
  return p;
}

constexpr int kBlk = 256;

__device__ __forceinline__ int64_t xcd_remap(int64_t b, int64_t nb) {
  const int64_t per = nb / kNumXCD;
  if (b >= per * kNumXCD) return b;
  return (b % kNumXCD) * per + b / kNumXCD;
}

// 4 consecutive floats of a row, zero-filled past `limit` (elements left in the row).
__device__ __forceinline__ float4 load4_guard(const float* __restrict__ p, int64_t limit, bool vec_ok) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (limit >= 4 && vec_ok) {
    v = *reinterpret_cast<const float4*>(p);
  } else {
    if (limit > 0) v.x = p[0];
    if (limit > 1) v.y = p[1];
    if (limit > 2) v.z = p[2];
    if (limit > 3) v.w = p[3];
  }
  return v;
}

// 4 consecutive floats at a 4-byte aligned address, zero-filled past `limit`: whole groups as ONE load whose type promises only
// dword alignment (the compiler picks the widest access the target allows for it), the row tail element by element
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ float4 load4_dword(const float* __restrict__ p, int limit) {
  if (limit >= 4) {
    const f32x4_a4 v = *reinterpret_cast<const f32x4_a4*>(p);
    return make_float4(v.x, v.y, v.z, v.w);
  }
  return load4_guard(p, limit, false);
}

// the first `limit` of 4 consecutive elements, the others zero (they may be row padding: anything, NaN included)
__device__ __forceinline__ float4 keep4(float4 v, int limit) {
  return make_float4(limit > 0 ? v.x : 0.f, limit > 1 ? v.y : 0.f, limit > 2 ? v.z : 0.f, limit > 3 ? v.w : 0.f);
}

}  // namespace
}  // namespace recmv
