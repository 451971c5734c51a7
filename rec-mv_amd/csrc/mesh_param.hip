// Mesh parameterisation: the fixed-vertex solve of a weighted graph Laplacian (two routes), per-face flat frames, the ARAP
// local step with the global step's right-hand side, and per-face distortion — gfx950.  Not in the reference.
//
// What it computes: the GPU work of recmv.param; include/recmv_hip.h has the definitions (the system, the CG recurrence, the
// summation order, the frames, the ARAP step, the Jacobian) down to the order of the operations.  All float64, un-contracted,
// only + - * / sqrt, gathers over CSR tables, no float atomics: both routes and tests/param_reference.py give the same bits
// and the same iteration count.
//
// The summation order, once (the header restates it): term i of a dot product belongs to slot i / 256, wave (i % 256) / 64,
// lane i % 64.  block_partials<K, 256> makes a slot: the xor butterfly over a wave's 64 lanes, then the four waves from 0.
// reduce_slots<K, 256> adds the slots: accumulator t takes slots t, t + 256, ... from 0, then the 256 accumulators like one
// slot.  The launch route runs exactly these two (one thread per vertex, a grid of ceil(V / 256) workgroups, so a workgroup
// IS a slot); the lds route's param_lds_waves / param_lds_total walk the same tree from its own workgroup size.
// The CG state, its three steps (begin, alpha, head), the residuals and the workspace carve are csrc/mesh_cg.h's, shared with
// lap_align.hip; both routes call the same steps.
//
// How:
//   * Work: a vertex has about 6 neighbours; an iteration gathers 2 doubles per neighbour and does a dozen flops per
//     neighbour and column.  At a few thousand vertices that is microseconds of work: the solve is bound by what stands
//     between two dependent reductions, a launch (launch route) or a workgroup barrier (lds route).
//   * launch route, two launches per iteration where lap_align.hip has five.  Every workgroup reduces the previous launch's
//     slots itself (the same order, so the same value everywhere) instead of waiting for a one-workgroup launch:
//       (1) direction: beta and the convergence test from the slots of r.z, r.r; p' = z + beta p; q = A p'; slots of p.q
//           (a thread recomputes its neighbours' p' from z and the old p, the same f64 operations; p ping-pongs)
//       (2) update: alpha from the slots of p.q; u += alpha p, r -= alpha q, z = r / d; slots of r.z, r.r
//     The CG state ping-pongs between two structs (a launch reads one, workgroup 0 writes the other), so no workgroup reads
//     what another writes in the same launch.  Evaluating the head of (1) again on the same inputs gives the same state, which
//     is what the one-workgroup check launch at the end of a batch does for the host's read-back.  After "done" both
//     launches return at once.  The redundant reduction reads ceil(V / 256) slots per workgroup: 65 at 129 x 129 vertices;
//     it would dominate beyond about 10^6 vertices, far from what a garment has.
//   * lds route (V <= kParamLdsMaxV): one workgroup, u, r, p, q (two columns each) and 1 / d in LDS, 72 bytes per vertex; the
//     CSR, the weights and the mask come from global memory every iteration (L2 hits).  Three barriers per iteration: every
//     wave adds the chunks' sums itself, so no wave waits for one that does.
//   * frames, ARAP and distortion: one thread per face or vertex.  The rotations go through a [F,2] buffer: the face pass is
//     needed anyway for the energy, and recomputing a rotation in each of a vertex's six faces would fit it six times.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)
#include "mesh_device.h"
#include "mesh_cg.h"

constexpr int kParamBlock = 256;
// The lds route's capacity: a single workgroup may have all of a CU's 160 KiB of LDS (163 840 bytes), and there is only one.
// A vertex costs 4 x 16 bytes (u, r, p, q: two f64 columns) + 8 bytes (1 / d) = 72; 4096 bytes stay for the wave sums of the
// reductions (8 sums x 35 chunks of 64 vertices x 8 bytes = 2240).  (163840 - 4096) / 72 = 2218.
constexpr int kParamLdsBytes = 163840;
constexpr int kParamLdsReserve = 4096;
constexpr int kParamLdsPerVertex = 72;
constexpr int kParamLdsMaxV = (kParamLdsBytes - kParamLdsReserve) / kParamLdsPerVertex;
constexpr int kParamLdsBlockMax = 1024;
constexpr int kParamLdsChunks = (kParamLdsMaxV + kWave - 1) / kWave;               // 35 (one per vertex under the host stand-in)
constexpr int kParamLdsSums = 8;
constexpr int kParamLdsTail = 8 * kParamLdsSums * kParamLdsChunks;
static_assert(kParamLdsMaxV == 2218, "the capacity of include/recmv_hip.h");
static_assert(kWave != 64 || kParamLdsTail <= kParamLdsReserve, "the reductions' scratch must fit its reserve");
// Where route 'auto' changes over: the lds route for V <= kParamAutoMaxV.  Measured on an MI355X
// (profiles/param_timing.json, tools/param_timing.py): the cotangent harmonic solve of square grids lifted to a sphere, tol
// 1e-12, whole solves between device events (the launch route with its read-back every 32 iterations), medians of 7,
// microseconds, lds / launch (and per iteration):
//   V =   25 (  2 it.):    71 /   335        V = 1089 ( 81 it.):  1085 /  1443  (13.4 / 17.8)
//   V =   81 ( 12 it.):   132 /   394        V = 1600 ( 99 it.):  1521 /  2006  (15.4 / 20.3)
//   V =  289 ( 38 it.):   331 /   805        V = 2209 (117 it.):  2229 /  2214  (19.0 / 18.9)
//   V =  529 ( 55 it.):   513 /   960        launch alone: V = 4225: 3684 (22.6), V = 16641: 11158 (34.3)
// An iteration of one workgroup costs 9 us while a thread holds one vertex and grows with the passes beyond 1024 vertices; two
// launches cost 17 - 20 us whatever the size.  1600 is the largest measured size at which the lds route's median is below
// the launch route's; at 2209 the two are level.  'lds' can be forced up to kParamLdsMaxV.
constexpr int kParamAutoMaxV = 1600;

struct ParamCg : CgState<2> {};              // (a name of its own keeps the kernels' symbols)

struct ParamArgs {
  const int32_t *off, *nbr;
  const double* w;
  int64_t V, nnz;
};

// entry k of row i counts: its neighbour in [0, V) and not i, its weight finite and > 0
__device__ __forceinline__ bool param_counts(const ParamArgs& a, int64_t i, int64_t k, int64_t& j, double& wk) {
  j = a.nbr[k];
  wk = a.w[k];
  return index_in(j, a.V) && j != i && finite_positive(wk);
}

// the state from the set-up's sums s = (b.b, r.z, r.r) x 2 columns, the zero-row count, unused; the same code on both routes
__device__ __forceinline__ void param_cg_begin(ParamCg& st, const double* s, double tol, int max_iter) {
  cg_begin<2>(st, s, s + 2, s + 4, tol, max_iter);
  st.zero_rows = (int32_t)s[6];
}

// d_i, whether vertex i is active, and for an active vertex r = rhs - A u and b (both columns)
__device__ __forceinline__ bool param_first_residual(const ParamArgs& a, const uint8_t* __restrict__ fixed,
                                                     const double* __restrict__ rhs, int64_t i, double ui0, double ui1,
                                                     const double* u, double& dinv, double* r, double* b, bool& zero_row) {
  const CsrRow row = csr_range_ordered(a.off, i, a.nnz);
  double d = 0., au[2] = {0., 0.}, fx[2] = {0., 0.};
  for (int64_t k = row.k0; k < row.k1; ++k) {
    int64_t j;
    double wk;
    if (!param_counts(a, i, k, j, wk)) continue;
    d += wk;
    const double uj0 = u[2 * j], uj1 = u[2 * j + 1];
    au[0] += wk * (ui0 - uj0);
    au[1] += wk * (ui1 - uj1);
    if (fixed[j]) {
      fx[0] += wk * uj0;
      fx[1] += wk * uj1;
    }
  }
  const bool free_vertex = fixed[i] == 0;
  zero_row = free_vertex && !(d > 0.);
  const bool act = free_vertex && d > 0.;
  dinv = act ? 1. / d : 0.;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    r[c] = act ? rhs[2 * i + c] - au[c] : 0.;
    b[c] = act ? rhs[2 * i + c] + fx[c] : 0.;
  }
  return act;
}

// ================================================================================================ launch route
__global__ void __launch_bounds__(kParamBlock)
param_init_kernel(ParamArgs a, const uint8_t* __restrict__ fixed, const double* __restrict__ rhs,
                  const double* __restrict__ u, double* __restrict__ dinv, double* __restrict__ r, double* __restrict__ z,
                  double* __restrict__ p0, double* __restrict__ p1, double* __restrict__ partials) {
  double acc[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.V) {
    double di, rc[2], bc[2];
    bool zero_row;
    param_first_residual(a, fixed, rhs, i, u[2 * i], u[2 * i + 1], u, di, rc, bc, zero_row);
    dinv[i] = di;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double zc = rc[c] * di;
      r[2 * i + c] = rc[c];
      z[2 * i + c] = zc;
      p0[2 * i + c] = 0.;
      p1[2 * i + c] = 0.;
      acc[c] = bc[c] * bc[c];
      acc[2 + c] = rc[c] * zc;
      acc[4 + c] = rc[c] * rc[c];
    }
    acc[6] = zero_row ? 1. : 0.;
  }
  block_partials<8, kParamBlock>(acc, partials);
}

__global__ void __launch_bounds__(kParamBlock)
param_init_reduce_kernel(const double* __restrict__ partials, int nslots, double tol, int max_iter, ParamCg* st) {
  double s[8];
  reduce_slots<8, kParamBlock>(partials, nslots, s);
  if (threadIdx.x == 0) {
    ParamCg x;
    param_cg_begin(x, s, tol, max_iter);
    *st = x;
  }
}

// The state after the head of an iteration, in every workgroup: `first` takes *sin as it is (the set-up made it), otherwise
// the slots of r.z, r.r are reduced and the head applied.  Workgroup 0 stores it to *sout.
__device__ __forceinline__ ParamCg param_head_state(int first, const ParamCg* sin, ParamCg* sout,
                                                    const double* __restrict__ prz, int nslots, double tol) {
  __shared__ ParamCg sh_state;
  double s[4] = {0., 0., 0., 0.};
  if (!first) reduce_slots<4, kParamBlock>(prz, nslots, s);
  if (threadIdx.x == 0) {
    ParamCg x = *sin;
    if (!first && !x.done) cg_head<2>(x, s, s + 2, tol);
    sh_state = x;
    if (blockIdx.x == 0) *sout = x;
  }
  __syncthreads();
  return sh_state;
}

// (1) beta and convergence; p' = z + beta p; q = A p'; slots of p.q
__global__ void __launch_bounds__(kParamBlock)
param_cg_direction_kernel(ParamArgs a, int first, const ParamCg* sin, ParamCg* sout, const double* __restrict__ prz,
                          int nslots, double tol, const double* __restrict__ dinv, const double* __restrict__ z,
                          const double* __restrict__ pold, double* __restrict__ pnew, double* __restrict__ q,
                          double* __restrict__ ppq) {
  const ParamCg st = param_head_state(first, sin, sout, prz, nslots, tol);
  if (st.done) return;
  const double be0 = st.beta[0], be1 = st.beta[1];
  double acc[2] = {0., 0.};
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.V) {
    double pi0 = 0., pi1 = 0., s0 = 0., s1 = 0.;
    if (dinv[i] > 0.) {
      pi0 = z[2 * i] + be0 * pold[2 * i];
      pi1 = z[2 * i + 1] + be1 * pold[2 * i + 1];
      const CsrRow row = csr_range_ordered(a.off, i, a.nnz);
      for (int64_t k = row.k0; k < row.k1; ++k) {
        int64_t j;
        double wk;
        if (!param_counts(a, i, k, j, wk)) continue;
        const double pj0 = z[2 * j] + be0 * pold[2 * j];
        const double pj1 = z[2 * j + 1] + be1 * pold[2 * j + 1];
        s0 += wk * (pi0 - pj0);
        s1 += wk * (pi1 - pj1);
      }
    }
    pnew[2 * i] = pi0;
    pnew[2 * i + 1] = pi1;
    q[2 * i] = s0;
    q[2 * i + 1] = s1;
    acc[0] = pi0 * s0;
    acc[1] = pi1 * s1;
  }
  block_partials<2, kParamBlock>(acc, ppq);
}

// (2) alpha; u += alpha p, r -= alpha q, z = r / d; slots of r.z and r.r
__global__ void __launch_bounds__(kParamBlock)
param_cg_update_kernel(int64_t V, const ParamCg* sin, ParamCg* sout, const double* __restrict__ ppq, int nslots,
                       const double* __restrict__ dinv, const double* __restrict__ p, const double* __restrict__ q,
                       double* __restrict__ u, double* __restrict__ r, double* __restrict__ z, double* __restrict__ prz) {
  __shared__ ParamCg sh_state;
  double pq[2];
  reduce_slots<2, kParamBlock>(ppq, nslots, pq);
  if (threadIdx.x == 0) {
    ParamCg x = *sin;
    if (!x.done) {
      cg_alpha<2>(x, pq);
      if (blockIdx.x == 0) *sout = x;
    }
    sh_state = x;
  }
  __syncthreads();
  if (sh_state.done) return;
  const double al0 = sh_state.alpha[0], al1 = sh_state.alpha[1];
  double acc[4] = {0., 0., 0., 0.};
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < V) {
    const double di = dinv[i];
    if (di > 0.) {                                         // a vertex that is not active keeps its bits
      u[2 * i] = u[2 * i] + al0 * p[2 * i];
      u[2 * i + 1] = u[2 * i + 1] + al1 * p[2 * i + 1];
      const double r0 = r[2 * i] - al0 * q[2 * i], r1 = r[2 * i + 1] - al1 * q[2 * i + 1];
      const double z0 = r0 * di, z1 = r1 * di;
      r[2 * i] = r0;
      r[2 * i + 1] = r1;
      z[2 * i] = z0;
      z[2 * i + 1] = z1;
      acc[0] = r0 * z0;
      acc[1] = r1 * z1;
      acc[2] = r0 * r0;
      acc[3] = r1 * r1;
    }
  }
  block_partials<4, kParamBlock>(acc, prz);
}

// the head once more, by one workgroup, for the host's read-back at the end of a batch
__global__ void __launch_bounds__(kParamBlock)
param_cg_check_kernel(const ParamCg* sin, ParamCg* report, const double* __restrict__ prz, int nslots, double tol) {
  param_head_state(0, sin, report, prz, nslots, tol);
}

// ================================================================================================ lds route
// The wave sums of K terms per thread for the chunk of kWave vertices that begins at vertex i0 (the same for the whole wave).
template <int K>
__device__ __forceinline__ void param_lds_waves(const double (&acc)[K], int64_t i0, double* wsum) {
  const int lane = threadIdx.x % kWave;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = wave_sum(acc[k]);
    if (lane == 0) wsum[k * kParamLdsChunks + i0 / kWave] = t;
  }
}

// Every wave adds the chunks' sums in the canonical order (slots of kParamBlock vertices, kParamBlock accumulators) into
// tot[K], the same value in every lane of every wave: no wave waits for another to do it.  After the barrier behind the
// chunks' stores.  An accumulator wave beyond the last slot holds +0 in every lane and its butterfly adds +0 to a total that
// is never -0 (it began as +0 plus the first wave's sum), so those waves are left out.
template <int K>
__device__ __forceinline__ void param_lds_total(const double* wsum, int nchunks, double (&tot)[K]) {
  constexpr int W = kParamBlock / kWave;
  const int lane = threadIdx.x % kWave, nslots = (nchunks + W - 1) / W;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double total = 0.;
    for (int w = 0; w < W && (w == 0 || w * kWave < nslots); ++w) {
      double acc = 0.;
      for (int s = w * kWave + lane; s < nslots; s += kParamBlock) {
        double slot = 0.;
        for (int c = 0; c < W; ++c) {
          const int ch = s * W + c;
          slot += ch < nchunks ? wsum[k * kParamLdsChunks + ch] : 0.;
        }
        acc += slot;
      }
      total += wave_sum(acc);
    }
    tot[k] = total;
  }
}

__global__ void __launch_bounds__(kParamLdsBlockMax)
param_solve_lds_kernel(ParamArgs a, const uint8_t* __restrict__ fixed, const double* __restrict__ rhs, double* __restrict__ u,
                       double tol, int max_iter, ParamCg* report) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kParamLdsPerVertex * kParamLdsMaxV + kParamLdsTail];
  if (a.V > kParamLdsMaxV) return;                         // (the whole workgroup; the entry point refuses it)
  const int n = (int)a.V, tid = (int)threadIdx.x, step = (int)blockDim.x, lane = tid % kWave;
  const int nchunks = (n + kWave - 1) / kWave;
  double* ul = (double*)smem;                              // [n][2]
  double* rl = ul + 2 * n;
  double* pl = rl + 2 * n;
  double* ql = pl + 2 * n;
  double* dl = ql + 2 * n;                                 // [n]
  double* wsum = (double*)(smem + kParamLdsPerVertex * kParamLdsMaxV);             // [kParamLdsSums][kParamLdsChunks]
  double* wsum_pq = wsum;                                  // sums 0, 1: written after barrier (1), read after (2)
  double* wsum_rz = wsum + 2 * kParamLdsChunks;            // sums 2 .. 5: written after barrier (2), read after (3)
  for (int i = tid; i < n; i += step) {
    ul[2 * i] = u[2 * i];
    ul[2 * i + 1] = u[2 * i + 1];
  }
  __syncthreads();
  for (int base = 0; base < n; base += step) {
    const int i = base + tid, i0 = i - lane;
    if (i0 >= n) continue;                                 // the whole wave
    double acc[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (i < n) {
      double di, rc[2], bc[2];
      bool zero_row;
      param_first_residual(a, fixed, rhs, i, ul[2 * i], ul[2 * i + 1], ul, di, rc, bc, zero_row);
      dl[i] = di;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        rl[2 * i + c] = rc[c];
        pl[2 * i + c] = 0.;
        acc[c] = bc[c] * bc[c];
        acc[2 + c] = rc[c] * (rc[c] * di);
        acc[4 + c] = rc[c] * rc[c];
      }
      acc[6] = zero_row ? 1. : 0.;
    }
    param_lds_waves<8>(acc, i0, wsum);
  }
  __syncthreads();
  ParamCg st;                                              // every thread carries the same state
  {
    double s[8];
    param_lds_total<8>(wsum, nchunks, s);
    param_cg_begin(st, s, tol, max_iter);
  }
  CsrRow own{0, 0};                                        // the row of the thread's first vertex, read once
  if (tid < n) own = csr_range_ordered(a.off, tid, a.nnz);
  // Three barriers per iteration.  A buffer is never written while a slower wave may still read it: p and the chunks of p.q
  // are read between (1) and (3) and written after (3) / (1); the chunks of r.z, r.r are read after (3) and written after (2).
  while (!st.done) {
    // p = z + beta p
    for (int i = tid; i < n; i += step) {
      const double di = dl[i];
      if (di > 0.) {
        pl[2 * i] = rl[2 * i] * di + st.beta[0] * pl[2 * i];
        pl[2 * i + 1] = rl[2 * i + 1] * di + st.beta[1] * pl[2 * i + 1];
      }
    }
    __syncthreads();                                       // (1)
    // q = A p, p.q
    for (int base = 0; base < n; base += step) {
      const int i = base + tid, i0 = i - lane;
      if (i0 >= n) continue;
      double acc[2] = {0., 0.};
      if (i < n) {
        double s0 = 0., s1 = 0.;
        const double pi0 = pl[2 * i], pi1 = pl[2 * i + 1];
        if (dl[i] > 0.) {
          const CsrRow row = base == 0 ? own : csr_range_ordered(a.off, i, a.nnz);
          for (int64_t k = row.k0; k < row.k1; ++k) {
            int64_t j;
            double wk;
            if (!param_counts(a, i, k, j, wk)) continue;
            s0 += wk * (pi0 - pl[2 * j]);
            s1 += wk * (pi1 - pl[2 * j + 1]);
          }
        }
        ql[2 * i] = s0;
        ql[2 * i + 1] = s1;
        acc[0] = pi0 * s0;
        acc[1] = pi1 * s1;
      }
      param_lds_waves<2>(acc, i0, wsum_pq);
    }
    __syncthreads();                                       // (2)
    {
      double pq[2];
      param_lds_total<2>(wsum_pq, nchunks, pq);
      cg_alpha<2>(st, pq);
    }
    // u += alpha p, r -= alpha q, r.z and r.r
    for (int base = 0; base < n; base += step) {
      const int i = base + tid, i0 = i - lane;
      if (i0 >= n) continue;
      double acc[4] = {0., 0., 0., 0.};
      if (i < n) {
        const double di = dl[i];
        if (di > 0.) {
          ul[2 * i] = ul[2 * i] + st.alpha[0] * pl[2 * i];
          ul[2 * i + 1] = ul[2 * i + 1] + st.alpha[1] * pl[2 * i + 1];
          const double r0 = rl[2 * i] - st.alpha[0] * ql[2 * i], r1 = rl[2 * i + 1] - st.alpha[1] * ql[2 * i + 1];
          rl[2 * i] = r0;
          rl[2 * i + 1] = r1;
          acc[0] = r0 * (r0 * di);
          acc[1] = r1 * (r1 * di);
          acc[2] = r0 * r0;
          acc[3] = r1 * r1;
        }
      }
      param_lds_waves<4>(acc, i0, wsum_rz);
    }
    __syncthreads();                                       // (3)
    {
      double s[4];
      param_lds_total<4>(wsum_rz, nchunks, s);
      cg_head<2>(st, s, s + 2, tol);
    }
  }
  for (int i = tid; i < n; i += step) {
    if (dl[i] > 0.) {
      u[2 * i] = ul[2 * i];
      u[2 * i + 1] = ul[2 * i + 1];
    }
  }
  if (tid == 0) *report = st;
}

// ================================================================================================ frames, ARAP, distortion
__global__ void __launch_bounds__(kParamBlock)
param_face_frames_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F,
                         double* __restrict__ frames, double* __restrict__ cots) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= F) return;
  double fr[4] = {0., 0., 0., 0.}, ct[3] = {0., 0., 0.};
  const int64_t* row = f + 3 * t;
  if (tri_valid(row, V)) {
    double p[3][3];
    load3(v, row[0], p[0]);
    load3(v, row[1], p[1]);
    load3(v, row[2], p[2]);
    if (finite3(p[0][0], p[0][1], p[0][2]) && finite3(p[1][0], p[1][1], p[1][2]) && finite3(p[2][0], p[2][1], p[2][2])) {
      const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
      const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
      double n[3];
      cross3(e1, e2, n);
      const double len = sqrt(dot3(n, n)), x1 = sqrt(dot3(e1, e1));
      if (finite_positive(len) && finite_positive(x1)) {
        fr[0] = x1;
        fr[1] = dot3(e1, e2) / x1;
        fr[2] = len / x1;
        fr[3] = 0.5 * len;
#pragma unroll
        for (int c = 0; c < 3; ++c) ct[c] = half_cot(p, c);                 // recmv_cotan_weights' corner expression
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) frames[4 * t + k] = fr[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) cots[3 * t + k] = ct[k];
}

// whether face t takes part, and then its flat corners X [3][2]
__device__ __forceinline__ bool param_flat(const int64_t* __restrict__ f, int64_t V, const double* __restrict__ frames,
                                           int64_t t, double X[3][2]) {
  if (!tri_valid(f + 3 * t, V) || !(frames[4 * t + 3] > 0.)) return false;
  X[0][0] = 0.; X[0][1] = 0.;
  X[1][0] = frames[4 * t]; X[1][1] = 0.;
  X[2][0] = frames[4 * t + 1]; X[2][1] = frames[4 * t + 2];
  return true;
}

// the local step: a face's closest rotation and its energy; slots of the energy
__global__ void __launch_bounds__(kParamBlock)
param_arap_faces_kernel(const int64_t* __restrict__ f, int64_t F, const double* __restrict__ frames,
                        const double* __restrict__ cots, const double* __restrict__ uv, int64_t V, double* __restrict__ rot,
                        double* __restrict__ partials) {
  double acc[1] = {0.};
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < F) {
    double ra = 1., rb = 0., X[3][2];
    if (param_flat(f, V, frames, t, X)) {
      double du[3][2], dx[3][2], S[4] = {0., 0., 0., 0.};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const int64_t va = f[3 * t + a], vb = f[3 * t + b];
        const double ck = cots[3 * t + k];
        du[k][0] = uv[2 * va] - uv[2 * vb];
        du[k][1] = uv[2 * va + 1] - uv[2 * vb + 1];
        dx[k][0] = X[a][0] - X[b][0];
        dx[k][1] = X[a][1] - X[b][1];
        S[0] += ck * (du[k][0] * dx[k][0]);
        S[1] += ck * (du[k][0] * dx[k][1]);
        S[2] += ck * (du[k][1] * dx[k][0]);
        S[3] += ck * (du[k][1] * dx[k][1]);
      }
      const double ca = S[0] + S[3], cb = S[2] - S[1];
      const double len = sqrt(ca * ca + cb * cb);
      if (finite_positive(len)) {
        ra = ca / len;
        rb = cb / len;
      }
      double e = 0.;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double d0 = du[k][0] - (ra * dx[k][0] - rb * dx[k][1]);
        const double d1 = du[k][1] - (rb * dx[k][0] + ra * dx[k][1]);
        e += cots[3 * t + k] * (d0 * d0 + d1 * d1);
      }
      acc[0] = e;
    }
    rot[2 * t] = ra;
    rot[2 * t + 1] = rb;
  }
  block_partials<1, kParamBlock>(acc, partials);
}

__global__ void __launch_bounds__(kParamBlock)
param_energy_kernel(const double* __restrict__ partials, int nslots, double* __restrict__ energy) {
  double s[1];
  reduce_slots<1, kParamBlock>(partials, nslots, s);
  if (threadIdx.x == 0) energy[0] = s[0];
}

// the right-hand side of the global step: a gather over the vertex -> corner-slot table
__global__ void __launch_bounds__(kParamBlock)
param_arap_rhs_kernel(const int64_t* __restrict__ f, int64_t F, const double* __restrict__ frames,
                      const double* __restrict__ cots, const double* __restrict__ rot, int64_t V,
                      const int64_t* __restrict__ soff, const int64_t* __restrict__ slots, double* __restrict__ rhs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  double s0 = 0., s1 = 0.;
  const CsrRow fan = csr_range_ordered(soff, i, 3 * F);
  for (int64_t s = fan.k0; s < fan.k1; ++s) {
    const int64_t slot = slots[s];
    if (!index_in(slot, 3 * F)) continue;
    const int64_t t = slot / 3;
    const int k = (int)(slot % 3);
    double X[3][2];
    if (f[slot] != i || !param_flat(f, V, frames, t, X)) continue;
    const double ra = rot[2 * t], rb = rot[2 * t + 1];
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    const double c1 = cots[3 * t + k2], c2 = cots[3 * t + k1];                     // the edge (k, k + 1) is opposite corner k + 2
    const double a0 = X[k][0] - X[k1][0], a1 = X[k][1] - X[k1][1];
    const double b0 = X[k][0] - X[k2][0], b1 = X[k][1] - X[k2][1];
    s0 += c1 * (ra * a0 - rb * a1);
    s1 += c1 * (rb * a0 + ra * a1);
    s0 += c2 * (ra * b0 - rb * b1);
    s1 += c2 * (rb * b0 + ra * b1);
  }
  rhs[2 * i] = s0;
  rhs[2 * i + 1] = s1;
}

__global__ void __launch_bounds__(kParamBlock)
param_distortion_kernel(const int64_t* __restrict__ f, int64_t F, const double* __restrict__ frames,
                        const double* __restrict__ uv, int64_t V, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= F) return;
  double X[3][2];
  double s1 = __builtin_nan(""), s2 = __builtin_nan(""), det = 0.;
  if (param_flat(f, V, frames, t, X)) {
    const int64_t v0 = f[3 * t], v1 = f[3 * t + 1], v2 = f[3 * t + 2];
    const double a0 = uv[2 * v1] - uv[2 * v0], a1 = uv[2 * v1 + 1] - uv[2 * v0 + 1];
    const double b0 = uv[2 * v2] - uv[2 * v0], b1 = uv[2 * v2 + 1] - uv[2 * v0 + 1];
    const double x1 = X[1][0], x2 = X[2][0], y2 = X[2][1];
    const double J00 = a0 / x1, J10 = a1 / x1;
    const double J01 = (b0 - J00 * x2) / y2, J11 = (b1 - J10 * x2) / y2;
    const double E = (J00 + J11) * 0.5, Fh = (J00 - J11) * 0.5, G = (J10 + J01) * 0.5, H = (J10 - J01) * 0.5;
    const double Q = sqrt(E * E + H * H), R = sqrt(Fh * Fh + G * G);
    s1 = Q + R;
    s2 = Q > R ? Q - R : R - Q;
    det = J00 * J11 - J01 * J10;
  }
  out[3 * t] = s1;
  out[3 * t + 1] = s2;
  out[3 * t + 2] = det;
}

inline int64_t param_slots(int64_t n) { return (n + kParamBlock - 1) / kParamBlock; }

// Workspace: state [2], report | slots of the set-up [*, 8], of p.q [*, 2], of r.z and r.r [*, 4] | 1 / d [V] | r, z, q, p0, p1
// [V,2], all f64, 256-byte aligned pieces.
struct ParamWorkspace {
  ParamCg *st[2], *report;
  double *pinit, *ppq, *prz, *dinv, *r, *z, *q, *p[2];
};

inline int64_t param_layout(int64_t V, char* base, ParamWorkspace* w) {
  Carver c{base};
  const int64_t slots = param_slots(V);
  ParamWorkspace x;
  x.st[0] = c.take<ParamCg>(1);
  x.st[1] = c.take<ParamCg>(1);
  x.report = c.take<ParamCg>(1);
  x.pinit = c.take<double>(slots * 8);
  x.ppq = c.take<double>(slots * 2);
  x.prz = c.take<double>(slots * 4);
  x.dinv = c.take<double>(V);
  x.r = c.take<double>(2 * V);
  x.z = c.take<double>(2 * V);
  x.q = c.take<double>(2 * V);
  x.p[0] = c.take<double>(2 * V);
  x.p[1] = c.take<double>(2 * V);
  if (w) *w = x;
  return c.offset;
}

// the arguments both solve routes share; false with a message
bool param_solve_args(const char* who, const int32_t* off, const int32_t* nbr, const double* w, int64_t V, int64_t nnz,
                      const uint8_t* fixed, const double* rhs, const double* u, double tol, int32_t max_iter,
                      const int32_t* iterations, const double* residuals, const int32_t* zero_rows) {
  if (V < 0 || nnz < 0) {
    set_error("%s: V=%lld, nnz=%lld must not be negative", who, (long long)V, (long long)nnz);
    return false;
  }
  if (V >= (1ll << 31) || nnz >= (1ll << 31)) {
    set_error("%s: at most 2^31 - 1 vertices and neighbour entries", who);
    return false;
  }
  if (!(tol >= 0.) || max_iter < 0) {
    set_error("%s: tol=%g and max_iter=%d must not be negative", who, tol, (int)max_iter);
    return false;
  }
  if (!iterations || !residuals || !zero_rows) {
    set_error("%s: NULL iterations / residuals / zero_rows (host pointers)", who);
    return false;
  }
  if (V > 0 && (!off || !fixed || !rhs || !u)) {
    set_error("%s: NULL pointer", who);
    return false;
  }
  if (V > 0 && nnz > 0 && (!nbr || !w)) {
    set_error("%s: NULL neighbour list or weights", who);
    return false;
  }
  return true;
}

void param_results(const ParamCg& st, int32_t* iterations, double* residuals, int32_t* zero_rows) {
  *iterations = st.iters;
  *zero_rows = st.zero_rows;
  cg_residuals<2>(st, residuals);
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_param_lds_max_vertices(void) { return kParamLdsMaxV; }
extern "C" int64_t recmv_param_auto_max_vertices(void) { return kParamAutoMaxV; }

extern "C" int64_t recmv_param_solve_workspace_bytes(int64_t V) {
  if (V < 0 || V >= (1ll << 31)) {
    set_error("param_solve_workspace_bytes: V=%lld must be 0 .. 2^31 - 1", (long long)V);
    return -1;
  }
  return V > 0 ? param_layout(V, nullptr, nullptr) : 0;
}

extern "C" int recmv_param_solve(const int32_t* nbr_offsets, const int32_t* nbr_idx, const double* weights, int64_t V,
                                 int64_t nnz, const uint8_t* fixed, const double* rhs, double* u, double tol, int32_t max_iter,
                                 int32_t batch, int32_t* iterations, double* residuals, int32_t* zero_rows, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  if (!param_solve_args("param_solve", nbr_offsets, nbr_idx, weights, V, nnz, fixed, rhs, u, tol, max_iter, iterations,
                        residuals, zero_rows))
    return RECMV_ERR_ARG;
  if (V == 0) {
    *iterations = 0;
    *zero_rows = 0;
    residuals[0] = residuals[1] = 0.;
    return RECMV_OK;
  }
  RECMV_REQUIRE(workspace, "param_solve: NULL workspace");
  RECMV_REQUIRE(workspace_bytes >= param_layout(V, nullptr, nullptr), "param_solve: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)param_layout(V, nullptr, nullptr));
  RECMV_REQUIRE(((uintptr_t)workspace & 255) == 0, "param_solve: workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ParamWorkspace w;
  param_layout(V, (char*)workspace, &w);
  const ParamArgs a{nbr_offsets, nbr_idx, weights, V, nnz};
  const int slots = (int)param_slots(V);
  const int per_batch = batch > 0 ? batch : kCgBatch;
  param_init_kernel<<<slots, kParamBlock, 0, s>>>(a, fixed, rhs, u, w.dinv, w.r, w.z, w.p[0], w.p[1], w.pinit);
  int rc = check_launch("param_init");
  if (rc != RECMV_OK) return rc;
  param_init_reduce_kernel<<<1, kParamBlock, 0, s>>>(w.pinit, slots, tol, (int)max_iter, w.st[0]);
  rc = check_launch("param_init_reduce");
  if (rc != RECMV_OK) return rc;
  ParamCg host;
  RECMV_HIP_TRY(hipMemcpyAsync(&host, w.st[0], sizeof(ParamCg), hipMemcpyDeviceToHost, s));
  RECMV_HIP_TRY(hipStreamSynchronize(s));
  int queued = 0;
  while (!host.done && queued < max_iter) {
    const int n = max_iter - queued < per_batch ? max_iter - queued : per_batch;
    for (int k = 0; k < n; ++k, ++queued) {
      double* pold = w.p[queued & 1];
      double* pnew = w.p[(queued + 1) & 1];
      param_cg_direction_kernel<<<slots, kParamBlock, 0, s>>>(a, queued == 0, w.st[0], w.st[1], w.prz, slots, tol, w.dinv,
                                                              w.z, pold, pnew, w.q, w.ppq);
      param_cg_update_kernel<<<slots, kParamBlock, 0, s>>>(V, w.st[1], w.st[0], w.ppq, slots, w.dinv, pnew, w.q, u, w.r, w.z,
                                                           w.prz);
    }
    param_cg_check_kernel<<<1, kParamBlock, 0, s>>>(w.st[0], w.report, w.prz, slots, tol);
    rc = check_launch("param_cg_iteration");
    if (rc != RECMV_OK) return rc;
    RECMV_HIP_TRY(hipMemcpyAsync(&host, w.report, sizeof(ParamCg), hipMemcpyDeviceToHost, s));
    RECMV_HIP_TRY(hipStreamSynchronize(s));
  }
  param_results(host, iterations, residuals, zero_rows);
  return RECMV_OK;
}

extern "C" int recmv_param_solve_lds(const int32_t* nbr_offsets, const int32_t* nbr_idx, const double* weights, int64_t V,
                                     int64_t nnz, const uint8_t* fixed, const double* rhs, double* u, double tol,
                                     int32_t max_iter, int32_t* iterations, double* residuals, int32_t* zero_rows, void* report,
                                     void* stream) {
  if (!param_solve_args("param_solve_lds", nbr_offsets, nbr_idx, weights, V, nnz, fixed, rhs, u, tol, max_iter, iterations,
                        residuals, zero_rows))
    return RECMV_ERR_ARG;
  RECMV_REQUIRE(V <= kParamLdsMaxV, "param_solve_lds: V=%lld, the lds route takes at most %d vertices", (long long)V,
                kParamLdsMaxV);
  if (V == 0) {
    *iterations = 0;
    *zero_rows = 0;
    residuals[0] = residuals[1] = 0.;
    return RECMV_OK;
  }
  RECMV_REQUIRE(report, "param_solve_lds: NULL report");
  RECMV_REQUIRE(((uintptr_t)report & 7) == 0, "param_solve_lds: report must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const ParamArgs a{nbr_offsets, nbr_idx, weights, V, nnz};
  int block = (int)ceil_div(V, kWave) * kWave;
  if (block > kParamLdsBlockMax) block = kParamLdsBlockMax;
  param_solve_lds_kernel<<<1, block, 0, s>>>(a, fixed, rhs, u, tol, (int)max_iter, (ParamCg*)report);
  const int rc = check_launch("param_solve_lds");
  if (rc != RECMV_OK) return rc;
  ParamCg host;
  RECMV_HIP_TRY(hipMemcpyAsync(&host, report, sizeof(ParamCg), hipMemcpyDeviceToHost, s));
  RECMV_HIP_TRY(hipStreamSynchronize(s));
  param_results(host, iterations, residuals, zero_rows);
  return RECMV_OK;
}

extern "C" int recmv_param_face_frames(const float* verts, int64_t V, const int64_t* faces, int64_t F, double* frames,
                                       double* cots, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "param_face_frames: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31), "param_face_frames: at most 2^31 - 1 vertices and faces");
  if (F == 0) return RECMV_OK;
  RECMV_REQUIRE(faces && frames && cots && (V == 0 || verts), "param_face_frames: NULL pointer");
  param_face_frames_kernel<<<(unsigned)param_slots(F), kParamBlock, 0, (hipStream_t)stream>>>(verts, V, faces, F, frames, cots);
  return check_launch("param_face_frames");
}

extern "C" int recmv_param_arap_rhs(const int64_t* faces, int64_t F, const double* frames, const double* cots, const double* uv,
                                    int64_t V, const int64_t* slot_offsets, const int64_t* slots, double* rot, double* rhs,
                                    double* partials, double* energy, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "param_arap_rhs: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31), "param_arap_rhs: at most 2^31 - 1 vertices and faces");
  RECMV_REQUIRE(energy, "param_arap_rhs: NULL energy");
  RECMV_REQUIRE(F == 0 || (faces && frames && cots && rot && partials && slots), "param_arap_rhs: NULL pointer of the faces");
  RECMV_REQUIRE(V == 0 || (uv && slot_offsets && rhs), "param_arap_rhs: NULL pointer of the vertices");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (F > 0) {
    param_arap_faces_kernel<<<(unsigned)param_slots(F), kParamBlock, 0, s>>>(faces, F, frames, cots, uv, V, rot, partials);
    if ((rc = check_launch("param_arap_faces")) != RECMV_OK) return rc;
  }
  param_energy_kernel<<<1, kParamBlock, 0, s>>>(partials, (int)param_slots(F), energy);
  if ((rc = check_launch("param_energy")) != RECMV_OK) return rc;
  if (V > 0) {
    param_arap_rhs_kernel<<<(unsigned)param_slots(V), kParamBlock, 0, s>>>(faces, F, frames, cots, rot, V, slot_offsets, slots,
                                                                          rhs);
    if ((rc = check_launch("param_arap_rhs")) != RECMV_OK) return rc;
  }
  return RECMV_OK;
}

extern "C" int recmv_param_distortion(const int64_t* faces, int64_t F, const double* frames, const double* uv, int64_t V,
                                      double* out, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "param_distortion: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31), "param_distortion: at most 2^31 - 1 vertices and faces");
  if (F == 0) return RECMV_OK;
  RECMV_REQUIRE(faces && frames && out && (V == 0 || uv), "param_distortion: NULL pointer");
  param_distortion_kernel<<<(unsigned)param_slots(F), kParamBlock, 0, (hipStream_t)stream>>>(faces, F, frames, uv, V, out);
  return check_launch("param_distortion");
}
