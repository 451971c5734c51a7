// Mesh smoothing (the kernels of recmv.smooth) — gfx950.
//
// What it computes (not in the reference, whose marching-cubes exports were smoothed by hand in MeshLab):
//   * recmv_cotan_weights: one float64 weight per entry of the vertex -> neighbour CSR: w[i->j] = the sum over the faces that hold
//     the edge (i, j), ascending, of 1/2 max(0, cot of the angle opposite the edge).  cot at corner c of a face is
//     dot(e1, e2) / |cross(e1, e2)| with e1 = x[next(c)] - x[c], e2 = x[prev(c)] - x[c] in the face's own cyclic order, float64
//     from the f32 coordinates.  Both ends of an edge evaluate that one expression over the same faces in the same order, so
//     w[i->j] == w[j->i] bit for bit.  A face with an index outside [0, V), a repeated corner, a corner that is not finite or a
//     cross product (at its first corner) that is not > 0 adds nothing and is counted once.
//   * recmv_laplacian_step: x' = x + lambda (sum_j w_ij x_j / sum_j w_ij - x) over the neighbour CSR (weights NULL: the mean of the
//     valid neighbours).  A fixed vertex, one without a valid neighbour or with a weight sum that is not > 0 is copied.  With a
//     boundary-neighbour table [V,2] a boundary vertex moves toward the midpoint of its two boundary neighbours with the same
//     lambda, or is copied when it does not have two.  lambda may be negative (Taubin's mu step).
//   * recmv_face_normal_filter: one iteration of bilateral normal filtering (Zheng, Fu, Au, Tai 2011) over the face -> face CSR:
//     n'_i = normalize(sum over i, then its neighbours ascending, of A_j exp(-|c_i - c_j|^2 / 2 sigma_c^2)
//     exp(-|n_i - n_j|^2 / 2 sigma_s^2) n_j); a face whose sum has no finite positive length keeps its normal.
//   * recmv_vertex_from_normals: one iteration of x'_i = x_i + 1/|F_i| sum_{f in F_i} n_f (n_f . (c_f - x_i)), c_f the centroid of
//     the face in the current x, F_i the valid faces of the vertex -> corner-slot CSR.
//
// How: iso_relax_kernel's shape — one thread per output row, grid-stride, every float64 sum one thread's loop in CSR order, one
// rounding to f32 at the store, no float atomics: the bits repeat from run to run.  The only atomic counts invalid faces (int32).
// Every index read from a table is checked against its array before it is followed and row ranges are clamped.  Input and
// output are different buffers.
//
// Size per row (marching-cubes output: 6 neighbours, 6 faces at a vertex, 3 neighbours of a face), unique bytes:
//   cotan weights    6 slots x (8 B slot + 24 B face row + 36 B corners) + 24 B neighbour row, writes 48 B: about 0.5 kB / vertex
//   laplacian step   4 + 6 x (4 B index + 12 B position [+ 8 B weight]) + 12 B own, writes 12 B: 0.12 - 0.17 kB / vertex
//   normal filter    4 + 4 x (4 B index + 12 B normal + 8 B area + 24 B centroid), writes 12 B: about 0.2 kB / face, 8 exp
//   vertex update    6 slots x (8 B slot + 24 B face row + 36 B corners + 12 B normal), writes 12 B: about 0.5 kB / vertex
// All are chains of dependent gathers (row -> index -> position), bound by the latency of those loads like iso_relax and the
// quadric kernels, far below the HBM rate in unique bytes.  DESIGN.md has what was measured.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

constexpr int kSmoothBlock = 256;

#include "mesh_device.h"                                   // tri_valid, index_in, csr_range_ordered, load3, cross3, dot3, finite, finite_positive, half_cot

// The three corners of face `row` when it takes part: valid indices, finite corners and a cross product at the first corner
// whose length is finite and > 0.
__device__ __forceinline__ bool sm_face_corners(const float* v, int64_t V, const int64_t* row, double p[3][3]) {
  if (!tri_valid(row, V)) return false;
  load3(v, row[0], p[0]); load3(v, row[1], p[1]); load3(v, row[2], p[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (!finite(p[c][0]) || !finite(p[c][1]) || !finite(p[c][2])) return false;
  const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
  const double w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
  double n[3];
  cross3(u, w, n);
  return finite_positive(sqrt(dot3(n, n)));
}

// where j stands in the ascending row nbr[k0, k1), or -1
__device__ __forceinline__ int64_t sm_find(const int32_t* nbr, int64_t k0, int64_t k1, int64_t j) {
  int64_t lo = k0, hi = k1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)nbr[mid] < j) lo = mid + 1; else hi = mid;
  }
  return (lo < k1 && (int64_t)nbr[lo] == j) ? lo : -1;
}

__global__ void __launch_bounds__(kSmoothBlock)
cotan_weights_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F,
                     const int64_t* __restrict__ vs_off, const int64_t* __restrict__ vs_idx, int64_t n_vs,
                     const int32_t* __restrict__ off, const int32_t* __restrict__ nbr, int64_t nnz, double* __restrict__ w,
                     int32_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double p[3][3];
  for (int64_t k = first; k < F; k += stride)
    if (!sm_face_corners(v, V, f + 3 * k, p)) atomicAdd(counts, 1);
  for (int64_t i = first; i < V; i += stride) {
    const CsrRow nb = csr_range_ordered(off, i, nnz);
    const int64_t k0 = nb.k0, k1 = nb.k1;
    for (int64_t k = k0; k < k1; ++k) w[k] = 0.;           // the row belongs to this thread alone
    if (n_vs <= 0) continue;
    const CsrRow fan = csr_range_ordered(vs_off, i, n_vs);
    for (int64_t s = fan.k0; s < fan.k1; ++s) {
      const int64_t slot = vs_idx[s];
      if ((uint64_t)slot >= (uint64_t)(3 * F)) continue;
      const int64_t face = slot / 3;
      const int c = (int)(slot - 3 * face);
      const int64_t* row = f + 3 * face;
      if (row[c] != i) continue;
      if (!sm_face_corners(v, V, row, p)) continue;
      const int cj = (c + 1) % 3, ck = (c + 2) % 3;
      const int64_t kj = sm_find(nbr, k0, k1, row[cj]), kk = sm_find(nbr, k0, k1, row[ck]);
      if (kj >= 0) w[kj] += half_cot(p, ck);            // the angle opposite the edge (i, j) is at k
      if (kk >= 0) w[kk] += half_cot(p, cj);
    }
  }
}

__global__ void __launch_bounds__(kSmoothBlock)
laplacian_step_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ nbr, int64_t V, int64_t nnz,
                      const float* __restrict__ x, const double* __restrict__ w, const uint8_t* __restrict__ fixed,
                      const int64_t* __restrict__ bnbr, double lambda, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    const double p[3] = {(double)x[3 * i], (double)x[3 * i + 1], (double)x[3 * i + 2]};
    double m[3];
    bool move = !(fixed && fixed[i]);
    const int64_t b0 = bnbr ? bnbr[2 * i] : -1, b1 = bnbr ? bnbr[2 * i + 1] : -1;
    if (move && (b0 >= 0 || b1 >= 0)) {                    // boundary: along its own curve, or not at all
      move = index_in(b0, V) && index_in(b1, V);
      if (move) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = 0.5 * ((double)x[3 * b0 + c] + (double)x[3 * b1 + c]);
      }
    } else if (move) {
      const CsrRow nb = csr_range_ordered(off, i, nnz);
      const int64_t k0 = nb.k0, k1 = nb.k1;
      double s[3] = {0., 0., 0.}, sum = 0.;
      int64_t cnt = 0;
      for (int64_t k = k0; k < k1; ++k) {
        const int64_t j = nbr[k];
        if (!index_in(j, V)) continue;
        if (w) {
          const double wk = w[k];
          if (!finite_positive(wk)) continue;              // (a weight of 0 adds nothing either way)
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] += wk * (double)x[3 * j + c];
          sum += wk;
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] += (double)x[3 * j + c];
        }
        ++cnt;
      }
      if (!w) sum = (double)cnt;
      move = cnt > 0 && finite_positive(sum);
      if (move) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = s[c] / sum;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = move ? (float)(p[c] + lambda * (m[c] - p[c])) : x[3 * i + c];
  }
}

__global__ void __launch_bounds__(kSmoothBlock)
face_normal_filter_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ nbr, int64_t F, int64_t nnz,
                          const float* __restrict__ n, const double* __restrict__ area, const double* __restrict__ cen,
                          double inv2c, double inv2s, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < F; i += stride) {
    double ni[3], ci[3];
    load3(n, i, ni);
    ci[0] = cen[3 * i]; ci[1] = cen[3 * i + 1]; ci[2] = cen[3 * i + 2];
    const double a = area[i];
    double s[3] = {a * ni[0], a * ni[1], a * ni[2]};        // the face itself: both exponentials are 1
    const CsrRow nb = csr_range_ordered(off, i, nnz);
    for (int64_t k = nb.k0; k < nb.k1; ++k) {
      const int64_t j = nbr[k];
      if ((uint64_t)j >= (uint64_t)F || j == i) continue;
      double nj[3];
      load3(n, j, nj);
      const double dc[3] = {ci[0] - cen[3 * j], ci[1] - cen[3 * j + 1], ci[2] - cen[3 * j + 2]};
      const double dn[3] = {ni[0] - nj[0], ni[1] - nj[1], ni[2] - nj[2]};
      const double wj = area[j] * exp(-(dot3(dc, dc) * inv2c)) * exp(-(dot3(dn, dn) * inv2s));
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += wj * nj[c];
    }
    const double len = sqrt(dot3(s, s));
    const bool ok = finite_positive(len);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = ok ? (float)(s[c] / len) : n[3 * i + c];
  }
}

__global__ void __launch_bounds__(kSmoothBlock)
vertex_from_normals_kernel(const float* __restrict__ x, int64_t V, const int64_t* __restrict__ f, int64_t F,
                           const int64_t* __restrict__ vs_off, const int64_t* __restrict__ vs_idx, int64_t n_vs,
                           const float* __restrict__ n, const uint8_t* __restrict__ fixed, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    double p[3];
    load3(x, i, p);
    double s[3] = {0., 0., 0.};
    int64_t cnt = 0;
    if (n_vs > 0 && !(fixed && fixed[i])) {
      const CsrRow fan = csr_range_ordered(vs_off, i, n_vs);
      for (int64_t t = fan.k0; t < fan.k1; ++t) {
        const int64_t slot = vs_idx[t];
        if (!index_in(slot, 3 * F)) continue;
        const int64_t face = slot / 3;
        const int64_t* row = f + 3 * face;
        if (row[slot - 3 * face] != i || !tri_valid(row, V)) continue;
        double nf[3], q[3][3];
        load3(n, face, nf);
        load3(x, row[0], q[0]); load3(x, row[1], q[1]); load3(x, row[2], q[2]);
        double d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (q[0][c] + q[1][c] + q[2][c]) / 3. - p[c];
        const double h = dot3(nf, d);
        if (!finite(h) || !finite_positive(dot3(nf, nf))) continue;   // a corner or normal that is not finite, or no normal
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += nf[c] * h;
        ++cnt;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = cnt > 0 ? (float)(p[c] + s[c] / (double)cnt) : x[3 * i + c];
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int recmv_cotan_weights(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* vs_offsets,
                                   const int64_t* vs_slots, int64_t n_vs, const int32_t* nbr_offsets, const int32_t* nbr_idx,
                                   int64_t nnz, double* weights, int32_t* counts, void* stream) {
  const char* what = "cotan_weights";
  RECMV_REQUIRE(V >= 0 && F >= 0 && n_vs >= 0 && nnz >= 0, "%s: V=%lld, F=%lld, n_vs=%lld, nnz=%lld must not be negative", what,
                (long long)V, (long long)F, (long long)n_vs, (long long)nnz);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31) && nnz < (1ll << 31) && n_vs < 3 * (1ll << 31),
                "%s: at most 2^31 - 1 vertices, faces and neighbour entries", what);
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(verts && nbr_offsets && counts, "%s: NULL pointer", what);
  RECMV_REQUIRE(F == 0 || faces, "%s: NULL faces", what);
  RECMV_REQUIRE(n_vs == 0 || (vs_offsets && vs_slots), "%s: NULL vertex -> slot table", what);
  RECMV_REQUIRE(nnz == 0 || (nbr_idx && weights), "%s: NULL neighbour list or weights", what);
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t), s));
  cotan_weights_kernel<<<stream_grid(V > F ? V : F, kSmoothBlock), kSmoothBlock, 0, s>>>(
      verts, V, faces, F, vs_offsets, vs_slots, n_vs, nbr_offsets, nbr_idx, nnz, weights, counts);
  return check_launch(what);
}

extern "C" int recmv_laplacian_step(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz,
                                    const float* verts, const double* weights, const uint8_t* fixed,
                                    const int64_t* boundary_nbrs, double lambda, float* out, void* stream) {
  const char* what = "laplacian_step";
  RECMV_REQUIRE(V >= 0 && nnz >= 0, "%s: V=%lld, nnz=%lld must not be negative", what, (long long)V, (long long)nnz);
  RECMV_REQUIRE(V < (1ll << 31) && nnz < (1ll << 31), "%s: at most 2^31 - 1 vertices and neighbour entries", what);
  RECMV_REQUIRE(lambda > -__builtin_inf() && lambda < __builtin_inf(), "%s: lambda=%g must be finite", what, lambda);
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(nbr_offsets && verts && out, "%s: NULL pointer", what);
  RECMV_REQUIRE(nnz == 0 || nbr_idx, "%s: NULL neighbour list", what);
  RECMV_REQUIRE(out != verts, "%s: out must not alias verts", what);
  laplacian_step_kernel<<<stream_grid(V, kSmoothBlock), kSmoothBlock, 0, (hipStream_t)stream>>>(
      nbr_offsets, nbr_idx, V, nnz, verts, weights, fixed, boundary_nbrs, lambda, out);
  return check_launch(what);
}

extern "C" int recmv_face_normal_filter(const int32_t* ff_offsets, const int32_t* ff_idx, int64_t F, int64_t nnz,
                                        const float* normals, const double* areas, const double* centroids, double sigma_c,
                                        double sigma_s, float* out, void* stream) {
  const char* what = "face_normal_filter";
  RECMV_REQUIRE(F >= 0 && nnz >= 0, "%s: F=%lld, nnz=%lld must not be negative", what, (long long)F, (long long)nnz);
  RECMV_REQUIRE(F < (1ll << 31) && nnz < (1ll << 31), "%s: at most 2^31 - 1 faces and neighbour entries", what);
  RECMV_REQUIRE(sigma_c > 0. && sigma_c < __builtin_inf(), "%s: sigma_c=%g must be finite and > 0", what, sigma_c);
  RECMV_REQUIRE(sigma_s > 0. && sigma_s < __builtin_inf(), "%s: sigma_s=%g must be finite and > 0", what, sigma_s);
  if (F == 0) return RECMV_OK;
  RECMV_REQUIRE(ff_offsets && normals && areas && centroids && out, "%s: NULL pointer", what);
  RECMV_REQUIRE(nnz == 0 || ff_idx, "%s: NULL neighbour list", what);
  RECMV_REQUIRE(out != normals, "%s: out must not alias normals", what);
  face_normal_filter_kernel<<<stream_grid(F, kSmoothBlock), kSmoothBlock, 0, (hipStream_t)stream>>>(
      ff_offsets, ff_idx, F, nnz, normals, areas, centroids, 1. / (2. * sigma_c * sigma_c), 1. / (2. * sigma_s * sigma_s), out);
  return check_launch(what);
}

extern "C" int recmv_vertex_from_normals(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                         const int64_t* vs_offsets, const int64_t* vs_slots, int64_t n_vs, const float* normals,
                                         const uint8_t* fixed, float* out, void* stream) {
  const char* what = "vertex_from_normals";
  RECMV_REQUIRE(V >= 0 && F >= 0 && n_vs >= 0, "%s: V=%lld, F=%lld, n_vs=%lld must not be negative", what, (long long)V,
                (long long)F, (long long)n_vs);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31) && n_vs < 3 * (1ll << 31), "%s: at most 2^31 - 1 vertices and faces", what);
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(verts && out, "%s: NULL pointer", what);
  RECMV_REQUIRE(n_vs == 0 || (faces && normals && vs_offsets && vs_slots), "%s: NULL vertex -> slot table, faces or normals", what);
  RECMV_REQUIRE(out != verts, "%s: out must not alias verts", what);
  vertex_from_normals_kernel<<<stream_grid(V, kSmoothBlock), kSmoothBlock, 0, (hipStream_t)stream>>>(
      verts, V, faces, F, vs_offsets, vs_slots, n_vs, normals, fixed, out);
  return check_launch(what);
}
