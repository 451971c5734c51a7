// The plumbing under the mesh kernels: lane-group sums, the (value, index) minimum, fixed-order block reductions, clamped
// CSR rows, index tests and the f64 3-vector helpers with half_cot, shared so that every mesh operation compiles the one
// body.  Include it inside namespace recmv after `#pragma clang fp contract(off)`, like closest_tri.h: a helper defined before the pragma
// would be compiled with contraction on, and its f64 products would fuse.  Device code only: no RECMV_REQUIRE and no HIP
// calls, so that the host checks of tools/ compile it under tools/host_check/common.h (kWave = 1, __shfl_xor the identity);
// tests/host_check.py refuses an includer that breaks the pragma rule.
#pragma once

// ---- indices ---------------------------------------------------------------------------------------------------------------
// i in [0, n), in one unsigned comparison.  An `||` chain of failed tests keeps the casts, here in tri_valid and at a
// dozen sites of the kernels: the compiler folds such a chain's branches before it inlines a call, and the kernel's
// instructions would change with it.
__device__ __forceinline__ bool index_in(int64_t i, int64_t n) { return (uint64_t)i < (uint64_t)n; }

__device__ __forceinline__ int64_t clamp_i64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// A face row that can be used: three indices in [0, V), all distinct.
__device__ __forceinline__ bool tri_valid(const int64_t* row, int64_t V) {
  if ((uint64_t)row[0] >= (uint64_t)V || (uint64_t)row[1] >= (uint64_t)V || (uint64_t)row[2] >= (uint64_t)V) return false;
  return row[0] != row[1] && row[0] != row[2] && row[1] != row[2];
}

// Row i of a CSR table of `len` entries as [k0, k1): k0 clamped at 0 and k1 at len.
__device__ __forceinline__ void csr_range(const int32_t* off, int64_t i, int64_t len, int64_t& k0, int64_t& k1) {
  k0 = off[i];
  k1 = off[i + 1];
  if (k0 < 0) k0 = 0;
  if (k1 > len) k1 = len;
}

// The same row with k1 clamped into [0, len] and then k0 into [0, k1]: the same loop on any table, other instructions.
struct CsrRow {
  int64_t k0, k1;
};

template <class Off>
__device__ __forceinline__ CsrRow csr_range_ordered(const Off* off, int64_t i, int64_t len) {
  const int64_t k1 = clamp_i64(off[i + 1], 0, len);
  return CsrRow{clamp_i64(off[i], 0, k1), k1};
}

// ---- lane groups -----------------------------------------------------------------------------------------------------------
// The sum over an aligned group of G lanes (a power of two, at most kWave) by an xor butterfly: the same tree whatever the
// data, the sum in every lane of the group.
template <int G, class T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) { return group_sum<kWave>(v); }

// (best, bidx) <- the smaller of it and (d, k) in the order (value, index); NaN never wins.
template <class T>
__device__ __forceinline__ void take_min(T d, int k, T& best, int& bidx) {
  if (d < best || (d == best && k < bidx)) {
    best = d;
    bidx = k;
  }
}

// ---- block reductions in a fixed order -------------------------------------------------------------------------------------
// Block sums of K doubles per thread to partials[K * blockIdx.x + k]; BLOCK threads.
template <int K, int BLOCK>
__device__ __forceinline__ void block_partials(double (&acc)[K], double* __restrict__ partials) {
  __shared__ double sh[K][BLOCK / kWave];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = wave_sum(acc[k]);
    if (lane == 0) sh[k][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double t = 0.;
    for (int w = 0; w < BLOCK / kWave; ++w) t += sh[threadIdx.x][w];
    partials[K * blockIdx.x + threadIdx.x] = t;
  }
}

// One workgroup of BLOCK threads: the K sums over nslots slots into out[K] (valid in thread 0).
template <int K, int BLOCK>
__device__ __forceinline__ void reduce_slots(const double* __restrict__ partials, int nslots, double (&out)[K]) {
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.;
  for (int s = threadIdx.x; s < nslots; s += BLOCK) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += partials[K * s + k];
  }
  __shared__ double sh[K][BLOCK / kWave];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = wave_sum(acc[k]);
    if (lane == 0) sh[k][wave] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.;
  if (threadIdx.x == 0) {
    for (int w = 0; w < BLOCK / kWave; ++w)
#pragma unroll
      for (int k = 0; k < K; ++k) out[k] += sh[k][w];
  }
}

// ---- f64 3-vectors and finiteness ------------------------------------------------------------------------------------------
__device__ __forceinline__ void load3(const float* v, int64_t i, double* out) {
  out[0] = v[3 * i]; out[1] = v[3 * i + 1]; out[2] = v[3 * i + 2];
}

__device__ __forceinline__ void cross3(const double* u, const double* w, double* n) {
  n[0] = u[1] * w[2] - u[2] * w[1];
  n[1] = u[2] * w[0] - u[0] * w[2];
  n[2] = u[0] * w[1] - u[1] * w[0];
}

__device__ __forceinline__ double dot3(const double* u, const double* w) { return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]; }

__device__ __forceinline__ double length3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

__device__ __forceinline__ bool finite(double x) { return x > -__builtin_inf() && x < __builtin_inf(); }

__device__ __forceinline__ bool finite_positive(double x) { return x > 0. && x < __builtin_inf(); }

// all three finite
__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {   // of three f32 widened to f64
  const double sum = x + y + z;                            // (a finite sum cannot hide an inf or a NaN; three f32 never overflow)
  return sum - sum == 0.;
}

// 1/2 max(0, cot) of the angle at corner c (0..2) of the face with corners p, in the face's cyclic order; 0 when the cross
// product at that corner has no finite positive length
__device__ __forceinline__ double half_cot(const double p[3][3], int c) {
  const int a = (c + 1) % 3, b = (c + 2) % 3;
  const double e1[3] = {p[a][0] - p[c][0], p[a][1] - p[c][1], p[a][2] - p[c][2]};
  const double e2[3] = {p[b][0] - p[c][0], p[b][1] - p[c][1], p[b][2] - p[c][2]};
  double n[3];
  cross3(e1, e2, n);
  const double len = sqrt(dot3(n, n));
  if (!finite_positive(len)) return 0.;
  const double cot = dot3(e1, e2) / len;
  return cot > 0. ? 0.5 * cot : 0.;
}
