// host stand-in for csrc/common.h: one lane per wave, kernels called as functions, one thread after the other
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
struct Idx { unsigned x, y, z; };
static Idx threadIdx, blockIdx, blockDim, gridDim;
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
template <class T> static inline T __shfl(T v, int, int) { return v; }
template <class T> static inline T __shfl_xor(T v, int, int) { return v; }
static inline unsigned long long __ballot(bool b) { return b ? 1ull : 0ull; }
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
static inline int atomicAdd(int32_t* p, int v) { int o = *p; *p += v; return o; }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { auto o = *p; *p += v; return o; }
static inline int atomicMin(int32_t* p, int v) { int o = *p; if (v < o) *p = v; return o; }
// the relaxed loads and stores of mesh_topology.hip's compression
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __hip_atomic_store(p, v, order, scope) (*(p) = (v))
static inline void __syncthreads() {}
using std::max;
namespace recmv {
constexpr int kWave = 1;
static inline void set_error(const char*, ...) {}          // the kernels' callers report through it; the checks read the results
}
