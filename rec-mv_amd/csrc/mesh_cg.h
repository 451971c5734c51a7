// The part of a float64 Jacobi-preconditioned conjugate-gradient solve that depends neither on the operator nor on the launch
// schedule: the per-column state, its three steps, the reported residuals and the carve of a workspace into 256-byte aligned
// pieces.  lap_align.hip (three columns, five launches an iteration) and mesh_param.hip (two columns, a two-launch and a
// one-workgroup route) bring q = A p and the sums; tests/cg_reference.py restates the recurrence.  Include it like
// mesh_device.h, inside namespace recmv after `#pragma clang fp contract(off)`; no RECMV_REQUIRE and no HIP calls, so the
// host checks of tools/ compile it under tools/host_check/common.h.
#pragma once
#include "mesh_device.h"                                   // finite

constexpr int kCgBatch = 32;                 // iterations queued between two reads of the state

template <int C>
struct CgState {
  double rz[C];                              // r.z of the current residual
  double bb[C];                              // |b|^2 of the right-hand side
  double rr[C];                              // |r|^2
  double alpha[C];
  double beta[C];
  int32_t active[C];                         // 1 while the column iterates
  int32_t done;                              // no column active, or max_iter reached
  int32_t iters;                             // updates applied
  int32_t max_iter;
  int32_t zero_rows;                         // mesh_param.hip's alone (free vertices whose weights sum to 0); no step touches it
};

// from the first sums b.b, r.z and r.r (C each): a column whose residual is already small never starts
template <int C>
__device__ __forceinline__ void cg_begin(CgState<C>& st, const double* bb, const double* rz, const double* rr, double tol,
                                         int max_iter) {
  int any = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    st.bb[c] = bb[c];
    st.rz[c] = rz[c];
    st.rr[c] = rr[c];
    st.alpha[c] = 0.;
    st.beta[c] = 0.;                         // the first p = z + 0 * p = z
    st.active[c] = rr[c] > tol * tol * bb[c] ? 1 : 0;
    any |= st.active[c];
  }
  st.iters = 0;
  st.max_iter = max_iter;
  st.done = (any == 0 || max_iter <= 0) ? 1 : 0;
}

// alpha = (r.z) / (p.q) per active column; a column whose p.q is not positive or whose alpha is not finite freezes
template <int C>
__device__ __forceinline__ void cg_alpha(CgState<C>& st, const double* pq) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double al = st.rz[c] / pq[c];
    const bool ok = st.active[c] && pq[c] > 0. && finite(al);
    st.alpha[c] = ok ? al : 0.;
    if (!ok) st.active[c] = 0;
  }
  st.iters += 1;
}

// from r.z and r.r (C each) of the updated residual: beta, convergence, "done"; a column whose beta is not finite freezes
template <int C>
__device__ __forceinline__ void cg_head(CgState<C>& st, const double* rz, const double* rr, double tol) {
  int any = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (st.active[c]) {
      const double be = st.rz[c] != 0. ? rz[c] / st.rz[c] : 0.;
      st.beta[c] = be;
      st.rz[c] = rz[c];
      st.rr[c] = rr[c];
      if (!(rr[c] > tol * tol * st.bb[c]) || !finite(be)) st.active[c] = 0;
    }
    if (!st.active[c]) st.beta[c] = 0.;
    any |= st.active[c];
  }
  st.done = (any == 0 || st.iters >= st.max_iter) ? 1 : 0;
}

// each column's relative residual |r| / |b| (|r| where b = 0), on the host from a state read back
template <int C>
inline void cg_residuals(const CgState<C>& st, double* out) {
  for (int c = 0; c < C; ++c) out[c] = st.bb[c] > 0. ? sqrt(st.rr[c] / st.bb[c]) : (st.rr[c] > 0. ? sqrt(st.rr[c]) : 0.);
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Consecutive 256-byte aligned pieces of a workspace; with base = nullptr only the size is counted.
struct Carver {
  char* base;
  int64_t offset = 0;
  template <class T>
  T* take(int64_t count) {
    T* ptr = base ? (T*)(base + offset) : nullptr;
    offset += align256(count * (int64_t)sizeof(T));
    return ptr;
  }
};
