// Fixed-radius neighbour search over points: every pair of vertices no farther apart than eps (the kernels of
// recmv.repair.points_within, which weld joins) — gfx950.
//
// What it computes (not in the reference, which never welds a mesh): for verts [V,3] f32 and eps >= 0 every pair (i, j), i < j,
// of FINITE vertices with d2 <= eps * eps, where d2 = (dx * dx + dy * dy) + dz * dz in float64 from the differences of the f32
// coordinates (exact in float64 whenever the exponents of the two coordinates are within 29 of each other, and a square does not
// see the sign of its argument, so the pair (i, j) and the pair (j, i) get one number).  Contraction is off: an O(V^2) loop with
// the same expression has the same members, bit for bit.  eps = 0 finds coincident vertices (+0.0 == -0.0).  A vertex with a
// NaN or inf coordinate is in no pair.
//
// How: a uniform grid of nx x ny x nz cubic cells of edge h over the bounding box of the finite vertices, chosen by the caller
// (recmv/repair.py: grid_layout) with h >= eps (1 + 2^-20) and at most 2^20 cells along an axis and 2^24 in all — a mesh of huge
// extent and tiny eps gets COARSER cells, never a table sized by its extent.
//   * recmv_points_within_cells: cell [V] int32 of every vertex, -1 for one that is not finite.  Along an axis the cell is
//     clamp(floor((x - o) / h), 0, n - 1) in float64: every step is monotone in x, and for |xi - xj| <= eps the exact quotients
//     differ by at most 1 / (1 + 2^-20) < 1 - 2^-21 while each computed one is within 2^21 * 2^-52 = 2^-31 of the exact one, so the
//     computed quotients differ by less than 1 and the cells by at most 1: the 27 cells round a vertex's own hold every partner.
//   * the caller sorts the finite vertices by cell (stable, so by id inside a cell) and passes their coordinates pts [n,3], their
//     ids [n] and cell_start [cells + 1] (the first sorted position of every cell).
//   * recmv_points_within_count / _fill: one thread per sorted position, grid-stride.  The three cells (cx - 1 .. cx + 1, y, z)
//     are neighbours in the table too, so the 27 cells are 9 contiguous ranges of sorted positions, walked in the order z, y,
//     position.  count writes counts[i] = the partners with a higher id; the caller takes the exclusive scan; fill writes the rows
//     (i, j) from offsets[i] on in the order they are met.  No atomic anywhere: the place of every row is a function of the input.
// Every value read from a table is checked before it is used as an index: ranges of cell_start are clamped to [0, n], an id
// outside [0, V) makes its thread (or that partner) do nothing, a row that would fall outside [0, P) is not written.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "mesh_device.h"                                   // finite3, index_in, clamp_i64

constexpr int kPointBlock = 256;
constexpr int64_t kPointMaxCells = 1ll << 24;
constexpr int32_t kPointMaxAxis = 1 << 20;

struct PointGrid {
  double ox, oy, oz, h;
  int32_t nx, ny, nz;
};

__device__ __forceinline__ int32_t cell_axis(double x, double o, double h, int32_t n) {
  const double t = floor((x - o) / h);
  if (!(t >= 0.)) return 0;
  if (t >= (double)n) return n - 1;
  return (int32_t)t;
}

__global__ void __launch_bounds__(kPointBlock)
points_cells_kernel(const float* __restrict__ v, int64_t V, PointGrid g, int32_t* __restrict__ cell) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    const double x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
    if (!finite3(x, y, z)) {
      cell[i] = -1;
      continue;
    }
    const int32_t cx = cell_axis(x, g.ox, g.h, g.nx), cy = cell_axis(y, g.oy, g.h, g.ny), cz = cell_axis(z, g.oz, g.h, g.nz);
    cell[i] = (cz * g.ny + cy) * g.nx + cx;
  }
}

// kFill = false: out = counts [V]; kFill = true: out = pairs [P,2], offsets [V] the exclusive scan of the counts
template <bool kFill>
__global__ void __launch_bounds__(kPointBlock)
points_within_kernel(const float* __restrict__ pts, const int64_t* __restrict__ ids, int64_t n, int64_t V, double eps2, PointGrid g,
                     const int32_t* __restrict__ cell_start, const int64_t* __restrict__ offsets, int64_t* __restrict__ out,
                     int64_t P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const int64_t i = ids[t];
    if (!index_in(i, V)) continue;
    const double x = pts[3 * t], y = pts[3 * t + 1], z = pts[3 * t + 2];
    if (!finite3(x, y, z)) {                               // (the caller sorts finite vertices only)
      if (!kFill) out[i] = 0;
      continue;
    }
    const int32_t cx = cell_axis(x, g.ox, g.h, g.nx), cy = cell_axis(y, g.oy, g.h, g.ny), cz = cell_axis(z, g.oz, g.h, g.nz);
    const int32_t x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.nx ? cx + 1 : g.nx - 1;
    int64_t found = 0;
    const int64_t base = kFill ? offsets[i] : 0;
    for (int32_t zz = cz > 0 ? cz - 1 : 0; zz <= cz + 1 && zz < g.nz; ++zz) {
      for (int32_t yy = cy > 0 ? cy - 1 : 0; yy <= cy + 1 && yy < g.ny; ++yy) {
        const int64_t row = ((int64_t)zz * g.ny + yy) * g.nx;
        const int64_t e = clamp_i64(cell_start[row + x1 + 1], 0, n);
        const int64_t b = clamp_i64(cell_start[row + x0], 0, e);
        for (int64_t u = b; u < e; ++u) {
          const double dx = (double)pts[3 * u] - x, dy = (double)pts[3 * u + 1] - y, dz = (double)pts[3 * u + 2] - z;
          const double d2 = dx * dx + dy * dy + dz * dz;
          if (!(d2 <= eps2)) continue;                     // most candidates end here: their id is never loaded
          const int64_t j = ids[u];
          if (j <= i || j >= V) continue;
          if (kFill) {
            const uint64_t at = (uint64_t)base + (uint64_t)found;                 // (unsigned: any offset may be read here)
            if (at < (uint64_t)P) {
              out[2 * at] = i;
              out[2 * at + 1] = j;
            }
          }
          ++found;
        }
      }
    }
    if (!kFill) out[i] = found;
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

static int point_grid_args(const char* what, double ox, double oy, double oz, double h, int32_t nx, int32_t ny, int32_t nz,
                           PointGrid* g) {
  RECMV_REQUIRE(ox - ox == 0. && oy - oy == 0. && oz - oz == 0., "%s: the grid's origin (%g, %g, %g) must be finite", what, ox, oy, oz);
  RECMV_REQUIRE(h > 0. && h - h == 0., "%s: cell=%g must be finite and above 0", what, h);
  RECMV_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= kPointMaxAxis && ny <= kPointMaxAxis && nz <= kPointMaxAxis,
                "%s: %d x %d x %d cells: every axis needs 1 .. 2^20", what, (int)nx, (int)ny, (int)nz);
  RECMV_REQUIRE((int64_t)nx * ny * nz <= kPointMaxCells, "%s: %d x %d x %d cells: at most 2^24 in all", what, (int)nx, (int)ny,
                (int)nz);
  *g = PointGrid{ox, oy, oz, h, nx, ny, nz};
  return RECMV_OK;
}

extern "C" int64_t recmv_points_within_max_cells(void) { return kPointMaxCells; }

extern "C" int recmv_points_within_cells(const float* verts, int64_t V, double ox, double oy, double oz, double cell, int32_t nx,
                                         int32_t ny, int32_t nz, int32_t* cell_of, void* stream) {
  const char* what = "points_within_cells";
  RECMV_REQUIRE(V >= 0, "%s: V=%lld must not be negative", what, (long long)V);
  RECMV_REQUIRE(V < (1ll << 31), "%s: at most 2^31 - 1 vertices", what);
  PointGrid g;
  int rc = point_grid_args(what, ox, oy, oz, cell, nx, ny, nz, &g);
  if (rc != RECMV_OK) return rc;
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(verts && cell_of, "%s: NULL pointer", what);
  points_cells_kernel<<<stream_grid(V, kPointBlock), kPointBlock, 0, (hipStream_t)stream>>>(verts, V, g, cell_of);
  return check_launch(what);
}

static int points_within_args(const char* what, const float* pts, const int64_t* ids, int64_t n, int64_t V, double eps, double ox,
                              double oy, double oz, double cell, int32_t nx, int32_t ny, int32_t nz, const int32_t* cell_start,
                              PointGrid* g) {
  RECMV_REQUIRE(n >= 0 && V >= 0, "%s: n=%lld, V=%lld must not be negative", what, (long long)n, (long long)V);
  RECMV_REQUIRE(V < (1ll << 31), "%s: at most 2^31 - 1 vertices", what);
  RECMV_REQUIRE(n <= V, "%s: n=%lld sorted vertices of V=%lld", what, (long long)n, (long long)V);
  RECMV_REQUIRE(eps >= 0. && eps - eps == 0., "%s: eps=%g must be finite and not negative", what, eps);
  int rc = point_grid_args(what, ox, oy, oz, cell, nx, ny, nz, g);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(cell >= eps, "%s: cell=%g is below eps=%g: the 27 cells round a vertex would miss partners", what, cell, eps);
  RECMV_REQUIRE(n == 0 || (pts && ids && cell_start), "%s: NULL pointer", what);
  return RECMV_OK;
}

extern "C" int recmv_points_within_count(const float* pts, const int64_t* ids, int64_t n, int64_t V, double eps, double ox, double oy,
                                         double oz, double cell, int32_t nx, int32_t ny, int32_t nz, const int32_t* cell_start,
                                         int64_t* counts, void* stream) {
  const char* what = "points_within_count";
  PointGrid g;
  int rc = points_within_args(what, pts, ids, n, V, eps, ox, oy, oz, cell, nx, ny, nz, cell_start, &g);
  if (rc != RECMV_OK) return rc;
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(counts, "%s: NULL counts", what);
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)V * sizeof(int64_t), s));       // (a vertex that is not finite has no thread)
  if (n == 0) return RECMV_OK;
  points_within_kernel<false><<<stream_grid(n, kPointBlock), kPointBlock, 0, s>>>(pts, ids, n, V, eps * eps, g, cell_start, nullptr,
                                                                                   counts, 0);
  return check_launch(what);
}

extern "C" int recmv_points_within_fill(const float* pts, const int64_t* ids, int64_t n, int64_t V, double eps, double ox, double oy,
                                        double oz, double cell, int32_t nx, int32_t ny, int32_t nz, const int32_t* cell_start,
                                        const int64_t* offsets, int64_t* pairs, int64_t P, void* stream) {
  const char* what = "points_within_fill";
  PointGrid g;
  int rc = points_within_args(what, pts, ids, n, V, eps, ox, oy, oz, cell, nx, ny, nz, cell_start, &g);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(P >= 0, "%s: P=%lld must not be negative", what, (long long)P);
  if (n == 0 || P == 0) return RECMV_OK;
  RECMV_REQUIRE(offsets && pairs, "%s: NULL pointer", what);
  points_within_kernel<true><<<stream_grid(n, kPointBlock), kPointBlock, 0, (hipStream_t)stream>>>(pts, ids, n, V, eps * eps, g,
                                                                                                    cell_start, offsets, pairs, P);
  return check_launch(what);
}
