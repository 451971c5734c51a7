// Quadric-error edge collapse (the kernels of recmv.simplify) — gfx950.
//
// What it computes (not in the reference, which thinned its meshes by hand in MeshLab; Garland & Heckbert 1997):
//   * recmv_vertex_quadrics: Q [V,11] float64 per vertex = the 10 upper-triangle entries (xx xy xz xw yy yz yw zz zw ww) of the
//     4x4 quadric and a weight.  Every incident face adds area * (n, d)(n, d)^T for its unit-normal plane (through its first
//     corner) and its area to the weight; every incident boundary edge adds boundary_weight * |e|^2 * (m, d)(m, d)^T, m the unit
//     vector in the plane of the edge's one face perpendicular to the edge, the plane through the edge's lower end; nothing to
//     the weight.  A face without area, an invalid face (an index outside [0, V) or repeated; counted) or one with a corner
//     that is not finite adds nothing.
//   * recmv_edge_collapse_cost: for candidate edges (a, b) and a placement code the point the collapse puts the vertex at
//     (f32), its cost x^T (Q[a] + Q[b]) x (float64, evaluated at the rounded point, clamped at 0) and the weight
//     Q[a][10] + Q[b][10].  Code 1: the point is a; 2: b; anything else: the cheapest of, in this order, the solution of the 3x3
//     system (float64 cofactor inverse; csrc/inv3x3_one.h is its f32 relative), a, b and the midpoint — ties go to the earlier.
//     REACH RULE: the solved point takes part only when, rounded to f32, it is finite and lies within reach * |b - a| of the
//     edge's midpoint; a system that is singular or nearly so cannot throw a vertex across the mesh, and a, b and the midpoint
//     are always there.  No output is not finite for finite input.  An invalid edge (an index outside [0, V), a == b; counted)
//     gets the point 0, the largest finite cost and the weight 0.
//   * recmv_collapse_flip_check: ok [E] = no face that survives the collapse of (a, b) to pos turns over or loses its area:
//     over the faces of a, then of b, without those that hold both ends, n_old . n_new > 0 with both cross products in float64
//     from the f32 coordinates and the moved corner replaced by pos.
//
// How: one thread per vertex (quadrics) or per candidate edge (cost, flip check), grid-stride.  No float atomics and no sum
// split over lanes: every float64 sum is one thread's loop in CSR order (faces ascending, then boundary edges ascending), so
// the bits repeat from run to run and from card to card, and a hub vertex whose row is longer than a wave gives the bits of
// the plain in-order loop because it IS that loop — a row of n faces costs its one lane n iterations, which marching-cubes
// output (at most 12 faces at a vertex) never notices.  The only atomics count invalid rows (int32).  Every index read from a
// table is checked against its array before it is followed, and row ranges are clamped, so tables that are not what the
// header describes read nothing outside the arrays.
//
// Size (the bench scene's two garments together: V = 161 k, F = 336 k, E = 504 k edges, all of them candidates):
//   quadrics   reads 8.1 MB of faces, 1.9 MB of vertices, 8.1 + 1.3 MB of CSR, writes 14.2 MB: 34 MB, 5 us at HBM rate; every
//              face's plane is rebuilt at each of its 3 corners: 1.0 M planes x about 60 float64 operations = 60 MFLOP.
//   cost       reads 2 x 88 B of quadrics and 2 x 12 B of vertices per edge (gathered, every row about 6 times: served by L2),
//              16 + 1 B of edge and code, writes 28 B: 123 MB of requests, 14.2 + 1.9 + 8.6 + 14.1 = 39 MB unique; about 150
//              float64 operations per edge = 76 MFLOP.
//   flip check walks about 12 faces per edge: 12 x (8 B CSR + 24 B face + 36 B corners) = 0.8 kB of gathered requests per
//              edge, 410 MB in all against 20 MB of unique data (L2 / Infinity Cache hits); about 45 operations per face =
//              270 MFLOP.
// None is near the arithmetic rate (78 TFLOP/s float64) or, counted in unique bytes, the HBM rate: all three are chains of
// dependent gathers (CSR row -> face row -> corner), bound by the latency of those loads and, for the flip check, by the
// L2's rate for 4 - 24 B requests.  Measured on an MI355X (tools/mesh_simplify_timing.py, profiles/mesh_simplify_timing.json;
// V = 163 842, F = 327 680, E = 491 520, medians of 10, host clock around launch and synchronisation): quadrics 43 us (0.8 TB/s
// of unique bytes, an eighth of the HBM rate), cost 51 us, flip check 98 us (about 4 TB/s of gathered requests); their
// float64 torch restatements take 1.16 / 1.36 / 2.19 ms on the same card.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "mesh_device.h"                                   // tri_valid, index_in, csr_range_ordered, load3, cross3, dot3, finite_positive

constexpr int kSimpBlock = 256;
constexpr int kQuadric = 11;                               // 10 entries and the weight
constexpr double kInvalidCost = 1.7976931348623157e308;    // the largest finite float64

// (b - a) x (c - a) of face `row`
__device__ __forceinline__ void face_normal(const float* v, const int64_t* row, double* a, double* n) {
  double b[3], c[3];
  load3(v, row[0], a); load3(v, row[1], b); load3(v, row[2], c);
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  cross3(u, w, n);
}

// q += wgt * p p^T
__device__ __forceinline__ void add_plane(double* q, double wgt, const double* p) {
  const double w0 = wgt * p[0], w1 = wgt * p[1], w2 = wgt * p[2], w3 = wgt * p[3];
  q[0] += w0 * p[0]; q[1] += w0 * p[1]; q[2] += w0 * p[2]; q[3] += w0 * p[3];
  q[4] += w1 * p[1]; q[5] += w1 * p[2]; q[6] += w1 * p[3];
  q[7] += w2 * p[2]; q[8] += w2 * p[3];
  q[9] += w3 * p[3];
}

// the unit-normal plane of a valid face through its first corner and its area; false: the face adds nothing
__device__ __forceinline__ bool face_plane(const float* v, int64_t V, const int64_t* row, double* p, double* area) {
  if (!tri_valid(row, V)) return false;
  double a[3], n[3];
  face_normal(v, row, a, n);
  const double len = sqrt(dot3(n, n));
  if (!finite_positive(len)) return false;                 // no area, or a corner that is not finite
  p[0] = n[0] / len; p[1] = n[1] / len; p[2] = n[2] / len;
  p[3] = -(p[0] * a[0] + p[1] * a[1] + p[2] * a[2]);
  *area = 0.5 * len;
  return true;
}

// the plane through boundary edge (a, b) of face k that stands on the face: unit m = n x e / |n x e|, and |e|^2
__device__ __forceinline__ bool border_plane(const float* v, int64_t V, const int64_t* f, int64_t F, const int64_t* be,
                                             double* p, double* e2) {
  const int64_t a = be[0], b = be[1], k = be[2];
  if ((uint64_t)a >= (uint64_t)V || (uint64_t)b >= (uint64_t)V || a == b || (uint64_t)k >= (uint64_t)F) return false;
  if (!tri_valid(f + 3 * k, V)) return false;
  double c0[3], n[3], pa[3], pb[3], m[3];
  face_normal(v, f + 3 * k, c0, n);
  load3(v, a, pa); load3(v, b, pb);
  const double e[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  cross3(n, e, m);
  const double len = sqrt(dot3(m, m));
  if (!finite_positive(len)) return false;
  p[0] = m[0] / len; p[1] = m[1] / len; p[2] = m[2] / len;
  p[3] = -(p[0] * pa[0] + p[1] * pa[1] + p[2] * pa[2]);
  *e2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
  return true;
}

// ---- quadrics ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock)
vertex_quadrics_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F,
                       const int64_t* __restrict__ vf_off, const int64_t* __restrict__ vf_idx, int64_t n_vf,
                       const int64_t* __restrict__ border, int64_t B, const int64_t* __restrict__ vb_off,
                       const int64_t* __restrict__ vb_idx, int64_t n_vb, double boundary_weight, double* __restrict__ Q,
                       int32_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t k = first; k < F; k += stride)
    if (!tri_valid(f + 3 * k, V)) atomicAdd(counts, 1);
  for (int64_t i = first; i < V; i += stride) {
    double q[kQuadric];
#pragma unroll
    for (int t = 0; t < kQuadric; ++t) q[t] = 0.;
    double p[4], w;
    if (n_vf > 0) {                                        // (csr_range_ordered's rows, spelled out: this kernel's loop compare)
      const int64_t end = clamp_i64(vf_off[i + 1], 0, n_vf);
      for (int64_t j = clamp_i64(vf_off[i], 0, end); j < end; ++j) {
        const int64_t k = vf_idx[j];
        if (!index_in(k, F)) continue;
        if (!face_plane(v, V, f + 3 * k, p, &w)) continue;
        add_plane(q, w, p);
        q[10] += w;
      }
    }
    if (B > 0 && n_vb > 0) {
      const int64_t end = clamp_i64(vb_off[i + 1], 0, n_vb);
      for (int64_t j = clamp_i64(vb_off[i], 0, end); j < end; ++j) {
        const int64_t r = vb_idx[j];
        if (!index_in(r, B)) continue;
        if (!border_plane(v, V, f, F, border + 3 * r, p, &w)) continue;
        add_plane(q, boundary_weight * w, p);
      }
    }
#pragma unroll
    for (int t = 0; t < kQuadric; ++t) Q[i * kQuadric + t] = q[t];
  }
}

// ---- placement and cost --------------------------------------------------------------------------------------------------------
// x^T Q x at (x, y, z, 1), the ten terms in this order, clamped at 0
__device__ __forceinline__ double quadric_cost(const double* q, double x, double y, double z) {
  const double c = q[0] * x * x + 2. * q[1] * x * y + 2. * q[2] * x * z + 2. * q[3] * x + q[4] * y * y + 2. * q[5] * y * z +
                   2. * q[6] * y + q[7] * z * z + 2. * q[8] * z + q[9];
  return c > 0. ? c : 0.;
}

__device__ __forceinline__ void offer(const double* q, float x, float y, float z, float* best, double* best_cost, bool* have) {
  const double c = quadric_cost(q, (double)x, (double)y, (double)z);
  if (!*have || c < *best_cost) {                          // a tie keeps the earlier candidate
    best[0] = x; best[1] = y; best[2] = z;
    *best_cost = c;
    *have = true;
  }
}

__global__ void __launch_bounds__(kSimpBlock)
edge_collapse_cost_kernel(const double* __restrict__ Q, const float* __restrict__ v, int64_t V, const int64_t* __restrict__ edges,
                          int64_t E, const uint8_t* __restrict__ code, double reach2, float* __restrict__ pos,
                          double* __restrict__ cost, double* __restrict__ weight, int32_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += stride) {
    const int64_t a = edges[2 * i], b = edges[2 * i + 1];
    if ((uint64_t)a >= (uint64_t)V || (uint64_t)b >= (uint64_t)V || a == b) {
      pos[3 * i] = pos[3 * i + 1] = pos[3 * i + 2] = 0.f;
      cost[i] = kInvalidCost;
      weight[i] = 0.;
      atomicAdd(counts, 1);
      continue;
    }
    double q[kQuadric];
#pragma unroll
    for (int t = 0; t < kQuadric; ++t) q[t] = Q[a * kQuadric + t] + Q[b * kQuadric + t];
    const float ax = v[3 * a], ay = v[3 * a + 1], az = v[3 * a + 2];
    const float bx = v[3 * b], by = v[3 * b + 1], bz = v[3 * b + 2];
    float best[3] = {0.f, 0.f, 0.f};
    double best_cost = 0.;
    bool have = false;
    const int c = code[i];
    if (c == 1) {
      offer(q, ax, ay, az, best, &best_cost, &have);
    } else if (c == 2) {
      offer(q, bx, by, bz, best, &best_cost, &have);
    } else {
      const double mx = 0.5 * ((double)ax + (double)bx), my = 0.5 * ((double)ay + (double)by), mz = 0.5 * ((double)az + (double)bz);
      const double ex = (double)bx - (double)ax, ey = (double)by - (double)ay, ez = (double)bz - (double)az;
      const double len2 = ex * ex + ey * ey + ez * ez;
      // A x = r with A the upper 3x3 (symmetric) and r = -(xw, yw, zw): x = adj(A) r / det
      const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[2] * q[5] - q[1] * q[7], c02 = q[1] * q[5] - q[2] * q[4];
      const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
      const double det = q[0] * c00 + q[1] * c01 + q[2] * c02;
      if (det != 0. && det - det == 0.) {
        const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
        const double sx = (c00 * r0 + c01 * r1 + c02 * r2) / det;
        const double sy = (c01 * r0 + c11 * r1 + c12 * r2) / det;
        const double sz = (c02 * r0 + c12 * r1 + c22 * r2) / det;
        const double big = 3.0e38;                         // (inside float's range: the casts below are defined)
        if (sx > -big && sx < big && sy > -big && sy < big && sz > -big && sz < big) {
          const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
          const double dx = (double)fx - mx, dy = (double)fy - my, dz = (double)fz - mz;
          if (dx * dx + dy * dy + dz * dz <= reach2 * len2) offer(q, fx, fy, fz, best, &best_cost, &have);
        }
      }
      offer(q, ax, ay, az, best, &best_cost, &have);
      offer(q, bx, by, bz, best, &best_cost, &have);
      offer(q, (float)mx, (float)my, (float)mz, best, &best_cost, &have);
    }
    pos[3 * i] = best[0]; pos[3 * i + 1] = best[1]; pos[3 * i + 2] = best[2];
    cost[i] = best_cost;
    weight[i] = q[10];
  }
}

// ---- flip test -----------------------------------------------------------------------------------------------------------------
// the faces of `end` that do not hold both a and b, with `end` moved to p: false when one turns over or loses its area
__device__ __forceinline__ bool ring_keeps_its_side(const float* v, int64_t V, const int64_t* f, int64_t F, const int64_t* vf_off,
                                                    const int64_t* vf_idx, int64_t n_vf, int64_t end, int64_t a, int64_t b,
                                                    const double* p) {
  const CsrRow fan = csr_range_ordered(vf_off, end, n_vf);
  for (int64_t j = fan.k0; j < fan.k1; ++j) {
    const int64_t k = vf_idx[j];
    if (!index_in(k, F)) continue;
    const int64_t* row = f + 3 * k;
    if (!tri_valid(row, V)) continue;
    const bool has_a = row[0] == a || row[1] == a || row[2] == a, has_b = row[0] == b || row[1] == b || row[2] == b;
    if (has_a && has_b) continue;                          // the face vanishes with the edge
    double c[3][3], n_old[3], n_new[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) load3(v, row[t], c[t]);
    {
      const double u[3] = {c[1][0] - c[0][0], c[1][1] - c[0][1], c[1][2] - c[0][2]};
      const double w[3] = {c[2][0] - c[0][0], c[2][1] - c[0][1], c[2][2] - c[0][2]};
      cross3(u, w, n_old);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (row[t] == end) { c[t][0] = p[0]; c[t][1] = p[1]; c[t][2] = p[2]; }
    {
      const double u[3] = {c[1][0] - c[0][0], c[1][1] - c[0][1], c[1][2] - c[0][2]};
      const double w[3] = {c[2][0] - c[0][0], c[2][1] - c[0][1], c[2][2] - c[0][2]};
      cross3(u, w, n_new);
    }
    const double dot = n_old[0] * n_new[0] + n_old[1] * n_new[1] + n_old[2] * n_new[2];
    if (!(dot > 0.)) return false;
  }
  return true;
}

__global__ void __launch_bounds__(kSimpBlock)
collapse_flip_check_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F,
                           const int64_t* __restrict__ vf_off, const int64_t* __restrict__ vf_idx, int64_t n_vf,
                           const int64_t* __restrict__ edges, int64_t E, const float* __restrict__ pos, uint8_t* __restrict__ ok) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += stride) {
    const int64_t a = edges[2 * i], b = edges[2 * i + 1];
    if ((uint64_t)a >= (uint64_t)V || (uint64_t)b >= (uint64_t)V || a == b) {
      ok[i] = 0;
      continue;
    }
    const double p[3] = {(double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]};
    bool good = true;
    if (n_vf > 0) {
      good = ring_keeps_its_side(v, V, f, F, vf_off, vf_idx, n_vf, a, a, b, p);
      if (good) good = ring_keeps_its_side(v, V, f, F, vf_off, vf_idx, n_vf, b, a, b, p);
    }
    ok[i] = good ? 1 : 0;
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int recmv_vertex_quadrics(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* vf_offsets,
                                     const int64_t* vf_faces, int64_t n_vf, const int64_t* border, int64_t B,
                                     const int64_t* vb_offsets, const int64_t* vb_rows, int64_t n_vb, double boundary_weight,
                                     double* Q, int32_t* counts, void* stream) {
  const char* what = "vertex_quadrics";
  RECMV_REQUIRE(V >= 0 && F >= 0 && B >= 0, "%s: V=%lld, F=%lld, B=%lld must not be negative", what, (long long)V, (long long)F,
                (long long)B);
  RECMV_REQUIRE(n_vf >= 0 && n_vb >= 0, "%s: n_vf=%lld, n_vb=%lld must not be negative", what, (long long)n_vf, (long long)n_vb);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31) && B < (1ll << 31), "%s: at most 2^31 - 1 vertices, faces and boundary edges", what);
  RECMV_REQUIRE(boundary_weight >= 0. && boundary_weight < __builtin_inf(), "%s: boundary_weight=%g must be finite and not negative",
                what, boundary_weight);
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(verts && Q && counts, "%s: NULL pointer", what);
  RECMV_REQUIRE(F == 0 || faces, "%s: NULL faces", what);
  RECMV_REQUIRE(n_vf == 0 || (vf_offsets && vf_faces), "%s: NULL vertex -> face table", what);
  RECMV_REQUIRE(B == 0 || n_vb == 0 || (border && vb_offsets && vb_rows), "%s: NULL vertex -> boundary-edge table", what);
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t), s));
  vertex_quadrics_kernel<<<stream_grid(V > F ? V : F, kSimpBlock), kSimpBlock, 0, s>>>(
      verts, V, faces, F, vf_offsets, vf_faces, n_vf, border, B, vb_offsets, vb_rows, n_vb, boundary_weight, Q, counts);
  return check_launch(what);
}

extern "C" int recmv_edge_collapse_cost(const double* Q, const float* verts, int64_t V, const int64_t* edges, int64_t E,
                                        const uint8_t* code, double reach, float* pos, double* cost, double* weight,
                                        int32_t* counts, void* stream) {
  const char* what = "edge_collapse_cost";
  RECMV_REQUIRE(V >= 0 && E >= 0, "%s: V=%lld, E=%lld must not be negative", what, (long long)V, (long long)E);
  RECMV_REQUIRE(V < (1ll << 31) && E < (1ll << 31), "%s: at most 2^31 - 1 vertices and edges", what);
  RECMV_REQUIRE(reach >= 0. && reach < 1e150, "%s: reach=%g must be finite and not negative", what, reach);
  if (E == 0) return RECMV_OK;
  RECMV_REQUIRE(edges && code && pos && cost && weight && counts, "%s: NULL pointer", what);
  RECMV_REQUIRE(V == 0 || (Q && verts), "%s: NULL mesh pointer", what);
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t), s));
  edge_collapse_cost_kernel<<<stream_grid(E, kSimpBlock), kSimpBlock, 0, s>>>(Q, verts, V, edges, E, code, reach * reach, pos,
                                                                               cost, weight, counts);
  return check_launch(what);
}

extern "C" int recmv_collapse_flip_check(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                         const int64_t* vf_offsets, const int64_t* vf_faces, int64_t n_vf, const int64_t* edges,
                                         int64_t E, const float* pos, uint8_t* ok, void* stream) {
  const char* what = "collapse_flip_check";
  RECMV_REQUIRE(V >= 0 && F >= 0 && E >= 0 && n_vf >= 0, "%s: V=%lld, F=%lld, E=%lld, n_vf=%lld must not be negative", what,
                (long long)V, (long long)F, (long long)E, (long long)n_vf);
  RECMV_REQUIRE(V < (1ll << 31) && F < (1ll << 31) && E < (1ll << 31), "%s: at most 2^31 - 1 vertices, faces and edges", what);
  if (E == 0) return RECMV_OK;
  RECMV_REQUIRE(edges && pos && ok, "%s: NULL pointer", what);
  RECMV_REQUIRE(V == 0 || verts, "%s: NULL mesh pointer", what);
  RECMV_REQUIRE(n_vf == 0 || (faces && vf_offsets && vf_faces), "%s: NULL vertex -> face table", what);
  hipStream_t s = (hipStream_t)stream;
  collapse_flip_check_kernel<<<stream_grid(E, kSimpBlock), kSimpBlock, 0, s>>>(verts, V, faces, F, vf_offsets, vf_faces, n_vf,
                                                                               edges, E, pos, ok);
  return check_launch(what);
}
