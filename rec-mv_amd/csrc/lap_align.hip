// Laplacian alignment of a garment template to its feature curves (sparse solve and smoothing pass) — gfx950.
//
// What it computes: the solve and the smoothing of one epoch of the reference's `Laplacian_Optimizer`
// (engineer/optimizer/lap_deform_optimizer.py:25-190), which inverts the dense normal matrix with torch.linalg.inv.
//   * recmv_lap_align_solve: u = argmin |L u - L v|^2 + w |C u - t|^2, i.e. the normal equations
//       (L^T L + diag(cw)) u = L^T (L v) + cwt
//     for the three coordinates at once, with L pytorch3d 0.4.0's `laplacian_packed` (L_ij = 1/deg_i on an edge, L_ii = -1;
//     an isolated vertex's row is -1 on the diagonal), cw_j = w * (constraints on j) and cwt_j = w * (sum of their targets).
//   * recmv_lap_smooth: one pass u'_i = (1/deg_i) sum_{j in N(i)} u_j (L with its diagonal zeroed; an isolated vertex -> 0).
//
// How: L is applied matrix-free over the symmetric neighbour CSR, with gathers only:
//     (L x)_i   = (1/deg_i) sum_{j in N(i)} x_j - x_i
//     (L^T y)_j = sum_{i in N(j)} y_i / deg_i - y_j
// so there are no scatters and no float atomics.  Jacobi-preconditioned conjugate gradients in float64, diagonal
// 1 + sum_{i in N(j)} 1/deg_i^2 + cw_j, started at u = v, one alpha / beta / convergence test per column; a converged column
// freezes (alpha = beta = 0).  The first residual is formed as cwt - cw v (the L^T L v terms cancel exactly), so a connected
// component without a constraint has r = p = 0 throughout and keeps its vertices bit for bit.
// One iteration is five launches and no host synchronisation:
//   (1) p <- z + beta p (into the other p buffer) and t = L p      one thread per vertex; every thread recomputes its
//                                                                  neighbours' new p from z and the old p, the same f64 ops
//   (2) q = L^T t + cw p, per-workgroup partials of p.q            fixed slot per workgroup (the grid depends on V only)
//   (3) one workgroup: alpha = (r.z) / (p.q), the iteration count
//   (4) u += alpha p, r -= alpha q, z = r / diag, partials of r.z and r.r
//   (5) one workgroup: beta, convergence (|r| <= tol |rhs| per column) and the "done" flag.
// Every launch returns at once when "done" is set, so the host queues iterations in batches and reads the flag once a batch.
// The reductions add fixed slots in a fixed order: results are bitwise reproducible.  The CG state, its three steps (begin,
// alpha, beta with convergence), the residuals and the workspace carve are csrc/mesh_cg.h's, shared with mesh_param.hip.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "mesh_device.h"                                   // csr_range, index_in, block_partials, reduce_slots
#include "mesh_cg.h"                                       // CgState, cg_begin, cg_alpha, cg_head, cg_residuals, Carver

constexpr int kLapBlock = 256;
using LapCg = CgState<3>;

struct LapArgs {
  const int32_t *off, *nbr;
  int64_t V, nnz;
  const double* invdeg;
  LapCg* st;
};

// ---------------------------------------------------------------------------------------------- set-up
// 1/deg_i, u = v (f64) and t = L v
__global__ void __launch_bounds__(kLapBlock)
lap_init_kernel(LapArgs a, const float* __restrict__ v, double* __restrict__ invdeg, double* __restrict__ u,
                double* __restrict__ t) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.V; i += stride) {
    int64_t k0, k1;
    csr_range(a.off, i, a.nnz, k0, k1);
    const double id = k1 > k0 ? 1. / (double)(k1 - k0) : 0.;
    invdeg[i] = id;
    double s[3] = {0., 0., 0.};
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t j = a.nbr[k];
      if (!index_in(j, a.V)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += (double)v[3 * j + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double vi = (double)v[3 * i + c];
      u[3 * i + c] = vi;
      t[3 * i + c] = s[c] * id - vi;
    }
  }
}

// rhs = L^T t + cwt (only its norm is needed), r = cwt - cw v, diag^-1, z = r / diag, p = z; partials of |rhs|^2, r.z, r.r
__global__ void __launch_bounds__(kLapBlock)
lap_init_residual_kernel(LapArgs a, const float* __restrict__ v, const double* __restrict__ cw,
                         const double* __restrict__ cwt, const double* __restrict__ t, double* __restrict__ r,
                         double* __restrict__ z, double* __restrict__ p, double* __restrict__ dinv,
                         double* __restrict__ partials) {
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.V; j += stride) {
    int64_t k0, k1;
    csr_range(a.off, j, a.nnz, k0, k1);
    double s[3] = {0., 0., 0.}, d = 1.;
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t i = a.nbr[k];
      if (!index_in(i, a.V)) continue;
      const double w = a.invdeg[i];
      d += w * w;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += t[3 * i + c] * w;
    }
    const double cj = cw[j];
    d += cj;
    const double di = 1. / d;
    dinv[j] = di;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double b = (s[c] - t[3 * j + c]) + cwt[3 * j + c];
      const double rc = cwt[3 * j + c] - cj * (double)v[3 * j + c];
      const double zc = rc * di;
      r[3 * j + c] = rc;
      z[3 * j + c] = zc;
      p[3 * j + c] = zc;
      acc[c] += b * b;
      acc[3 + c] += rc * zc;
      acc[6 + c] += rc * rc;
    }
  }
  block_partials<9, kLapBlock>(acc, partials);
}

__global__ void __launch_bounds__(kLapBlock)
lap_init_reduce_kernel(const double* __restrict__ partials, int nslots, double tol, int max_iter, LapCg* st) {
  double s[9];
  reduce_slots<9, kLapBlock>(partials, nslots, s);
  if (threadIdx.x == 0) cg_begin(*st, s, s + 3, s + 6, tol, max_iter);
}

// ---------------------------------------------------------------------------------------------- one iteration
// (1) pn = z + beta p_old, t = L pn
__global__ void __launch_bounds__(kLapBlock)
lap_cg_direction_kernel(LapArgs a, const double* __restrict__ z, const double* __restrict__ pold,
                        double* __restrict__ pnew, double* __restrict__ t) {
  if (a.st->done) return;
  const double be[3] = {a.st->beta[0], a.st->beta[1], a.st->beta[2]};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.V; i += stride) {
    int64_t k0, k1;
    csr_range(a.off, i, a.nnz, k0, k1);
    double s[3] = {0., 0., 0.};
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t j = a.nbr[k];
      if (!index_in(j, a.V)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += z[3 * j + c] + be[c] * pold[3 * j + c];
    }
    const double id = a.invdeg[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double pi = z[3 * i + c] + be[c] * pold[3 * i + c];
      pnew[3 * i + c] = pi;
      t[3 * i + c] = s[c] * id - pi;
    }
  }
}

// (2) q = L^T t + cw p, partials of p.q
__global__ void __launch_bounds__(kLapBlock)
lap_cg_apply_kernel(LapArgs a, const double* __restrict__ cw, const double* __restrict__ p,
                    const double* __restrict__ t, double* __restrict__ q, double* __restrict__ partials) {
  if (a.st->done) return;
  double acc[3] = {0., 0., 0.};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.V; j += stride) {
    int64_t k0, k1;
    csr_range(a.off, j, a.nnz, k0, k1);
    double s[3] = {0., 0., 0.};
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t i = a.nbr[k];
      if (!index_in(i, a.V)) continue;
      const double w = a.invdeg[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += t[3 * i + c] * w;
    }
    const double cj = cw[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double pc = p[3 * j + c];
      const double qc = (s[c] - t[3 * j + c]) + cj * pc;
      q[3 * j + c] = qc;
      acc[c] += pc * qc;
    }
  }
  block_partials<3, kLapBlock>(acc, partials);
}

// (3) alpha = (r.z) / (p.q) per active column, the iteration count
__global__ void __launch_bounds__(kLapBlock)
lap_cg_alpha_kernel(const double* __restrict__ partials, int nslots, LapCg* st) {
  if (st->done) return;
  double pq[3];
  reduce_slots<3, kLapBlock>(partials, nslots, pq);
  if (threadIdx.x == 0) cg_alpha(*st, pq);
}

// (4) u += alpha p, r -= alpha q, z = r / diag; partials of r.z and r.r
__global__ void __launch_bounds__(kLapBlock)
lap_cg_update_kernel(LapArgs a, const double* __restrict__ dinv, const double* __restrict__ p,
                     const double* __restrict__ q, double* __restrict__ u, double* __restrict__ r,
                     double* __restrict__ z, double* __restrict__ partials) {
  if (a.st->done) return;
  const double al[3] = {a.st->alpha[0], a.st->alpha[1], a.st->alpha[2]};
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.V; i += stride) {
    const double di = dinv[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      u[3 * i + c] = u[3 * i + c] + al[c] * p[3 * i + c];
      const double rc = r[3 * i + c] - al[c] * q[3 * i + c];
      const double zc = rc * di;
      r[3 * i + c] = rc;
      z[3 * i + c] = zc;
      acc[c] += rc * zc;
      acc[3 + c] += rc * rc;
    }
  }
  block_partials<6, kLapBlock>(acc, partials);
}

// (5) beta, convergence per column, "done"
__global__ void __launch_bounds__(kLapBlock)
lap_cg_beta_kernel(const double* __restrict__ partials, int nslots, double tol, LapCg* st) {
  if (st->done) return;
  double s[6];
  reduce_slots<6, kLapBlock>(partials, nslots, s);
  if (threadIdx.x == 0) cg_head(*st, s, s + 3, tol);
}

__global__ void __launch_bounds__(kLapBlock)
lap_output_kernel(const double* __restrict__ u, int64_t n, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) out[k] = (float)u[k];
}

// ---------------------------------------------------------------------------------------------- smoothing
__global__ void __launch_bounds__(kLapBlock)
lap_smooth_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ nbr, int64_t V, int64_t nnz,
                  const float* __restrict__ u, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    int64_t k0, k1;
    csr_range(off, i, nnz, k0, k1);
    double s[3] = {0., 0., 0.};
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t j = nbr[k];
      if (!index_in(j, V)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += (double)u[3 * j + c];
    }
    const double id = k1 > k0 ? 1. / (double)(k1 - k0) : 0.;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = (float)(s[c] * id);
  }
}

inline int64_t lap_slots(int64_t V) { return stream_grid(V, kLapBlock); }

// Workspace: LapCg | partials [slots, 9] | invdeg, dinv [V] | u, r, z, p0, p1, t, q [V,3], all f64, 256-byte aligned pieces.
struct LapWorkspace {
  LapCg* st;
  double *partials, *invdeg, *dinv, *u, *r, *z, *p[2], *t, *q;
};

inline int64_t lap_layout(int64_t V, char* base, LapWorkspace* w) {
  Carver c{base};
  LapWorkspace x;
  x.st = c.take<LapCg>(1);
  x.partials = c.take<double>(lap_slots(V) * 9);
  x.invdeg = c.take<double>(V);
  x.dinv = c.take<double>(V);
  x.u = c.take<double>(3 * V);
  x.r = c.take<double>(3 * V);
  x.z = c.take<double>(3 * V);
  x.p[0] = c.take<double>(3 * V);
  x.p[1] = c.take<double>(3 * V);
  x.t = c.take<double>(3 * V);
  x.q = c.take<double>(3 * V);
  if (w) *w = x;
  return c.offset;
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_lap_align_workspace_bytes(int64_t V) { return V > 0 ? lap_layout(V, nullptr, nullptr) : 0; }

extern "C" int recmv_lap_align_solve(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz,
                                     const float* v, const double* cw, const double* cwt, double tol, int32_t max_iter,
                                     float* u, int32_t* iterations, double* residuals, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(V >= 0 && nnz >= 0, "lap_align_solve: V=%lld, nnz=%lld must not be negative", (long long)V,
                (long long)nnz);
  RECMV_REQUIRE(V < (1ll << 31) && nnz < (1ll << 31), "lap_align_solve: at most 2^31 - 1 vertices and neighbour entries");
  RECMV_REQUIRE(tol >= 0. && max_iter >= 0, "lap_align_solve: tol=%g and max_iter=%d must not be negative", tol,
                (int)max_iter);
  RECMV_REQUIRE(iterations && residuals, "lap_align_solve: NULL iterations / residuals (host pointers)");
  if (V == 0) {
    *iterations = 0;
    residuals[0] = residuals[1] = residuals[2] = 0.;
    return RECMV_OK;
  }
  RECMV_REQUIRE(nbr_offsets && v && cw && cwt && u && workspace, "lap_align_solve: NULL pointer");
  RECMV_REQUIRE(nnz == 0 || nbr_idx, "lap_align_solve: NULL neighbour list");
  RECMV_REQUIRE(workspace_bytes >= recmv_lap_align_workspace_bytes(V),
                "lap_align_solve: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)recmv_lap_align_workspace_bytes(V));
  RECMV_REQUIRE(((uintptr_t)workspace & 255) == 0, "lap_align_solve: workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  LapWorkspace w;
  lap_layout(V, (char*)workspace, &w);
  LapArgs a{nbr_offsets, nbr_idx, V, nnz, w.invdeg, w.st};
  const int slots = (int)lap_slots(V);
  lap_init_kernel<<<slots, kLapBlock, 0, s>>>(a, v, w.invdeg, w.u, w.t);
  int rc = check_launch("lap_init");
  if (rc != RECMV_OK) return rc;
  lap_init_residual_kernel<<<slots, kLapBlock, 0, s>>>(a, v, cw, cwt, w.t, w.r, w.z, w.p[0], w.dinv, w.partials);
  rc = check_launch("lap_init_residual");
  if (rc != RECMV_OK) return rc;
  lap_init_reduce_kernel<<<1, kLapBlock, 0, s>>>(w.partials, slots, tol, (int)max_iter, w.st);
  rc = check_launch("lap_init_reduce");
  if (rc != RECMV_OK) return rc;
  LapCg host;
  RECMV_HIP_TRY(hipMemcpyAsync(&host, w.st, sizeof(LapCg), hipMemcpyDeviceToHost, s));
  RECMV_HIP_TRY(hipStreamSynchronize(s));
  int queued = 0;
  while (!host.done && queued < max_iter) {
    const int n = max_iter - queued < kCgBatch ? max_iter - queued : kCgBatch;
    for (int k = 0; k < n; ++k, ++queued) {
      double* pold = w.p[queued & 1];
      double* pnew = w.p[(queued + 1) & 1];
      lap_cg_direction_kernel<<<slots, kLapBlock, 0, s>>>(a, w.z, pold, pnew, w.t);
      lap_cg_apply_kernel<<<slots, kLapBlock, 0, s>>>(a, cw, pnew, w.t, w.q, w.partials);
      lap_cg_alpha_kernel<<<1, kLapBlock, 0, s>>>(w.partials, slots, w.st);
      lap_cg_update_kernel<<<slots, kLapBlock, 0, s>>>(a, w.dinv, pnew, w.q, w.u, w.r, w.z, w.partials);
      lap_cg_beta_kernel<<<1, kLapBlock, 0, s>>>(w.partials, slots, tol, w.st);
    }
    rc = check_launch("lap_cg_iteration");
    if (rc != RECMV_OK) return rc;
    RECMV_HIP_TRY(hipMemcpyAsync(&host, w.st, sizeof(LapCg), hipMemcpyDeviceToHost, s));
    RECMV_HIP_TRY(hipStreamSynchronize(s));
  }
  lap_output_kernel<<<stream_grid(3 * V, kLapBlock), kLapBlock, 0, s>>>(w.u, 3 * V, u);
  rc = check_launch("lap_output");
  if (rc != RECMV_OK) return rc;
  *iterations = host.iters;
  cg_residuals(host, residuals);
  return RECMV_OK;
}

extern "C" int recmv_lap_smooth(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz,
                                const float* u, float* out, void* stream) {
  RECMV_REQUIRE(V >= 0 && nnz >= 0, "lap_smooth: V=%lld, nnz=%lld must not be negative", (long long)V, (long long)nnz);
  RECMV_REQUIRE(V < (1ll << 31) && nnz < (1ll << 31), "lap_smooth: at most 2^31 - 1 vertices and neighbour entries");
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(nbr_offsets && u && out, "lap_smooth: NULL pointer");
  RECMV_REQUIRE(nnz == 0 || nbr_idx, "lap_smooth: NULL neighbour list");
  RECMV_REQUIRE(u != out, "lap_smooth: out must not alias u");
  lap_smooth_kernel<<<stream_grid(V, kLapBlock), kLapBlock, 0, (hipStream_t)stream>>>(nbr_offsets, nbr_idx, V, nnz, u, out);
  return check_launch("lap_smooth");
}
