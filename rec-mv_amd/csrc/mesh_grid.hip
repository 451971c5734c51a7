// Uniform grid over a triangle mesh and the exact closest point through it (the hot path of recmv.metrics) — gfx950.
//
// What it computes (not in the reference, whose tools/comparison_results.py stops after loading a mesh):
//   * recmv_mesh_grid_count / recmv_mesh_grid_fill: a grid of nx x ny x nz cubic cells of size h at `origin` (chosen by
//     the caller) over the mesh verts [V,3] f32 / faces [F,3] int64.  A face is binned into every cell its axis-aligned
//     box overlaps (conservative); a face with an index outside [0, V) is binned nowhere (load_tri's skip).  count writes
//     the per-cell counts and the number of (cell, face) entries, fill scans the counts into cell offsets [cells + 1],
//     writes the face ids of every cell into entries, and the faces as (a, b - a, c - a) into a table of three float4
//     per face: load_tri's values, so a (point, face) pair gives recmv_closest_point's bits.
//   * recmv_closest_point_grid: recmv_closest_point's outputs (face, point, squared distance; ties to the lowest face
//     id), found by visiting the Chebyshev rings of cells around the query's cell instead of every face.
//
// How: integer atomics only, no float atomics; the query's result does not depend on the order of a cell's entries.
//   * count / fill: one thread per face; both take the face's cell range from face_range(), so they cannot disagree, and
//     fill also clamps every slot against its cell's end and the entry capacity.  A face whose range holds more than
//     kBigFace cells is spread over the 64 lanes of its wave.  Entry order inside a cell follows an integer cursor.
//   * scan: block sums (1024 cells per workgroup), one workgroup scans the sums, a third launch writes the offsets.
//   * query: a group of G lanes (1, 8 or 64: `lanes`) per query point.  Ring r is the shell of cells at Chebyshev distance
//     r from the query's cell (clamped into the grid); the lanes of the group stride over the shell's cells, each runs
//     through its cell's entries with closest_tri.h, and the group meets in a shuffle minimum on (distance, face id).
//     A cell whose box is farther than the lane's best is skipped.  The search stops after the ring whose outside is
//     farther than the best (strictly: an equal distance continues, so that an equal face with a lower id still wins) or
//     when the rings cover the grid; r < max(nx, ny, nz) bounds the loop for any input.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "closest_tri.h"                                   // Tri, closest_st, load_tri
#include "grid_query.h"                                    // Grid, Range, face_range, the table; GridView, for_each_entry
#include "mesh_device.h"                                   // wave_sum, take_min, index_in

constexpr int kGridBlock = 256;
constexpr int kBigFace = 256;                              // cells of a face's range above which its wave shares the work
constexpr int kScanPer = 4;                                // cells per thread of the scan
constexpr int kScanTile = kGridBlock * kScanPer;           // cells per workgroup of the scan
constexpr float kEps32 = 1.1920929e-7f;                    // 2^-23

// op(cell, face) for every cell of the ranges the lanes of a wave hold.  Every lane of the wave must call it (ballot);
// small ranges run in their own lane, a range of more than kBigFace cells is spread over the wave.
template <class Op>
__device__ __forceinline__ void for_each_cell(const Range& r, bool valid, int face, const Grid& g, Op op) {
  const bool big = valid && range_cells(r) > kBigFace;
  if (valid && !big) {
    for (int z = r.z0; z <= r.z1; ++z)
      for (int y = r.y0; y <= r.y1; ++y)
        for (int x = r.x0; x <= r.x1; ++x) op(cell_id(g, x, y, z), face);
  }
  unsigned long long m = __ballot(big);
  const int lane = threadIdx.x % kWave;
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const Range b{__shfl(r.x0, src, kWave), __shfl(r.x1, src, kWave), __shfl(r.y0, src, kWave),
                  __shfl(r.y1, src, kWave), __shfl(r.z0, src, kWave), __shfl(r.z1, src, kWave)};
    const int fk = __shfl(face, src, kWave);
    const int64_t n = range_cells(b);
    for (int64_t c = lane; c < n; c += kWave) {
      int x, y, z;
      range_cell(b, c, x, y, z);
      op(cell_id(g, x, y, z), fk);
    }
  }
}

__global__ void __launch_bounds__(kGridBlock)
grid_count_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F, Grid g,
                  int32_t* __restrict__ counts, unsigned long long* __restrict__ total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  long long mine = 0;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < F; base += stride) {   // (uniform trip count per wave)
    const int64_t k = base + threadIdx.x;
    Range r{0, 0, 0, 0, 0, 0};
    const bool valid = k < F && face_range(v, f, V, k, g, r);
    if (valid) mine += range_cells(r);
    for_each_cell(r, valid, (int)k, g, [&](int cell, int) { atomicAdd(counts + cell, 1); });
  }
  mine = wave_sum(mine);
  if (threadIdx.x % kWave == 0 && mine) atomicAdd(total, (unsigned long long)mine);
}

__global__ void __launch_bounds__(kGridBlock)
grid_fill_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F, Grid g,
                 const int32_t* __restrict__ offsets, int32_t* __restrict__ cursor, int32_t* __restrict__ entries,
                 int64_t capacity, float4* __restrict__ tris) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < F; base += stride) {
    const int64_t k = base + threadIdx.x;
    Range r{0, 0, 0, 0, 0, 0};
    const bool valid = k < F && face_range(v, f, V, k, g, r);
    if (k < F) {
      Tri q;
      if (!load_tri(v, f, V, k, q)) {                      // never referenced (binned nowhere); NaN: it could not win
        q.ax = q.ay = q.az = __builtin_nanf("");
        q.bx = q.by = q.bz = q.cx = q.cy = q.cz = 0.f;
      }
      tri_table_store(tris, k, q);
    }
    for_each_cell(r, valid, (int)k, g, [&](int cell, int face) {
      const int slot = atomicAdd(cursor + cell, 1);
      // the cell's own end (the count pass saw the same range, so this holds) and the capacity the caller allocated
      if (slot >= 0 && slot < offsets[cell + 1] && (int64_t)slot < capacity) entries[slot] = face;
    });
  }
}

// ---- exclusive scan of the counts (int32, exact) ---------------------------------------------------------------------
__global__ void __launch_bounds__(kGridBlock)
scan_sums_kernel(const int32_t* __restrict__ counts, int64_t n, int32_t* __restrict__ sums) {
  __shared__ int32_t s[kGridBlock];
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  int32_t t = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) t += i0 + j < n ? counts[i0 + j] : 0;
  s[threadIdx.x] = t;
  __syncthreads();
  for (int off = kGridBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = s[0];
}

// inclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); returns the inclusive prefix
__device__ __forceinline__ int32_t block_scan_inclusive(int32_t t, int32_t* s) {
  s[threadIdx.x] = t;
  __syncthreads();
  for (int off = 1; off < kGridBlock; off <<= 1) {
    const int32_t add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  return s[threadIdx.x];
}

// one workgroup: sums [m] -> their exclusive scan in place, the grand total into offsets_end[0]
__global__ void __launch_bounds__(kGridBlock)
scan_of_sums_kernel(int32_t* __restrict__ sums, int64_t m, int32_t* __restrict__ offsets_end) {
  __shared__ int32_t s[kGridBlock];
  int32_t carry = 0;
  for (int64_t base = 0; base < m; base += kGridBlock) {
    const int64_t i = base + threadIdx.x;
    const int32_t t = i < m ? sums[i] : 0;
    const int32_t incl = block_scan_inclusive(t, s);
    if (i < m) sums[i] = carry + incl - t;
    carry += s[kGridBlock - 1];
    __syncthreads();                                       // s is rewritten by the next round
  }
  if (threadIdx.x == 0) offsets_end[0] = carry;
}

__global__ void __launch_bounds__(kGridBlock)
scan_apply_kernel(const int32_t* __restrict__ counts, int64_t n, const int32_t* __restrict__ sums,
                  int32_t* __restrict__ offsets, int32_t* __restrict__ cursor) {
  __shared__ int32_t s[kGridBlock];
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  int32_t c[kScanPer], t = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    c[j] = i0 + j < n ? counts[i0 + j] : 0;
    t += c[j];
  }
  int32_t at = sums[blockIdx.x] + block_scan_inclusive(t, s) - t;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    if (i0 + j < n) {
      offsets[i0 + j] = at;
      cursor[i0 + j] = at;
    }
    at += c[j];
  }
}

// ---- the query ---------------------------------------------------------------------------------------------------------
// Cell k of the shell at Chebyshev distance r around (cx, cy, cz): the two z slabs of (2r + 1)^2 cells, then for each of
// the 2r - 1 layers between them the 8r cells of the square's rim.  24 r^2 + 2 cells (1 for r = 0).
__device__ __forceinline__ void shell_cell(int64_t k, int r, int cx, int cy, int cz, int& x, int& y, int& z) {
  const int side = 2 * r + 1;
  const int64_t slab = (int64_t)side * side;
  if (k < 2 * slab) {
    const bool top = k >= slab;
    const int64_t j = top ? k - slab : k;
    z = top ? cz + r : cz - r;
    y = cy - r + (int)(j / side);
    x = cx - r + (int)(j % side);
    return;
  }
  k -= 2 * slab;
  const int rim = 8 * r;
  z = cz - r + 1 + (int)(k / rim);
  int j = (int)(k % rim);
  if (j < side) {
    y = cy - r; x = cx - r + j;
  } else if (j < 2 * side) {
    y = cy + r; x = cx - r + (j - side);
  } else {
    j -= 2 * side;
    const int inner = side - 2;
    x = j < inner ? cx - r : cx + r;
    y = cy - r + 1 + (j < inner ? j : j - inner);
  }
}

// The lower bounds.  A face a lane has not tested lies, with its closest point q, in a cell the lane has not visited, so
// its distance is at least the gap between the query and that cell's box.  Three things are rounded, and each is rounded
// DOWN here so that the bound stays one on the f32 distance closest_st returns:
//   * cell coordinates u = (x - o) / h carry two roundings, for the query and for q's binning alike: their difference is
//     off by at most eps32 (|u_p| + |u_q|), |u_q| <= max(nx, ny, nz) for a cell that is not at the grid's edge (an edge
//     cell is open outwards: it holds whatever was clamped into it, and no gap is taken on that side).  `mu` =
//     4 eps32 (max |u_p| + max(nx, ny, nz)) is subtracted from every gap in cell units;
//   * the squares, their sum and the products with h: under 8 roundings, a factor (1 - 8 eps32) on the square;
//   * closest_st's own error: its squared distance is within 16 eps32 R^2 of the exact one, R the largest distance from
//     the query to a corner of the face (the bound tests/test_gpu_animation.py derives), and R is at most the distance D
//     to the farthest corner of the grid: `m2` = 16 eps32 D^2 is subtracted from the square.
__device__ __forceinline__ float lower_bound2(float gx, float gy, float gz, float mu, float m2, float h) {
  gx = fmaxf(gx - mu, 0.f) * h;
  gy = fmaxf(gy - mu, 0.f) * h;
  gz = fmaxf(gz - mu, 0.f) * h;
  return (gx * gx + gy * gy + gz * gz) * (1.f - 8.f * kEps32) - m2;
}

// the gap along one axis between u and cell i of n, open outwards at the grid's edge
__device__ __forceinline__ float axis_gap(float u, int i, int n) {
  float gap = 0.f;
  if (i > 0) gap = fmaxf(gap, (float)i - u);
  if (i < n - 1) gap = fmaxf(gap, u - (float)(i + 1));
  return gap;
}

template <int G>
__global__ void __launch_bounds__(kGridBlock)
closest_point_grid_kernel(const float* __restrict__ p, int64_t P, const int64_t* __restrict__ order,
                          const float4* __restrict__ tris, int64_t F, GridView view, int64_t* __restrict__ face,
                          float* __restrict__ point, float* __restrict__ dist2) {
  const Grid& g = view.g;
  const int64_t slot = ((int64_t)blockIdx.x * kGridBlock + threadIdx.x) / G;
  const int sub = threadIdx.x % G;
  if (slot >= P) return;                                   // (a whole group at once: slot is the same in its lanes)
  const int64_t i = order ? order[slot] : slot;
  if ((uint64_t)i >= (uint64_t)P) return;
  const float px = p[3 * i], py = p[3 * i + 1], pz = p[3 * i + 2];
  const float ux = cell_coord(px, g.ox, g.inv_h), uy = cell_coord(py, g.oy, g.inv_h), uz = cell_coord(pz, g.oz, g.inv_h);
  const int cx = cell_index(ux, g.nx), cy = cell_index(uy, g.ny), cz = cell_index(uz, g.nz);
  const int maxdim = max(g.nx, max(g.ny, g.nz));
  const float mu = 4.f * kEps32 * (fmaxf(fmaxf(fabsf(ux), fabsf(uy)), fabsf(uz)) + (float)maxdim);
  const float fx = fmaxf(fabsf(ux), fabsf((float)g.nx - ux)) * g.h, fy = fmaxf(fabsf(uy), fabsf((float)g.ny - uy)) * g.h;
  const float fz = fmaxf(fabsf(uz), fabsf((float)g.nz - uz)) * g.h;
  const float m2 = 16.f * kEps32 * (fx * fx + fy * fy + fz * fz) * (1.f + 8.f * kEps32);
  float best = __builtin_inff();
  int bidx = -1;
  for (int r = 0; r < maxdim; ++r) {                       // after ring maxdim - 1 every cell has been visited
    const int64_t shell = r == 0 ? 1 : 24ll * r * r + 2;
    for (int64_t k = sub; k < shell; k += G) {
      int x, y, z;
      shell_cell(k, r, cx, cy, cz, x, y, z);
      if ((unsigned)x >= (unsigned)g.nx || (unsigned)y >= (unsigned)g.ny || (unsigned)z >= (unsigned)g.nz) continue;
      if (lower_bound2(axis_gap(ux, x, g.nx), axis_gap(uy, y, g.ny), axis_gap(uz, z, g.nz), mu, m2, g.h) > best) continue;
      for_each_entry(view, cell_id(g, x, y, z), F, [&](int k2) {
        const Tri q = tri_table_load(tris, k2);
        float s, t;
        take_min(closest_st(px, py, pz, q, s, t), k2, best, bidx);
      });
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {            // the group's minimum, in every lane of it
      const float ob = __shfl_xor(best, off, G);
      const int oi = __shfl_xor(bidx, off, G);
      take_min(ob, oi, best, bidx);
    }
    // what lies outside the visited box [c - r, c + r]: the nearest of its faces that still have cells behind them
    const bool lx = cx - r > 0, hx = cx + r < g.nx - 1, ly = cy - r > 0, hy = cy + r < g.ny - 1;
    const bool lz = cz - r > 0, hz = cz + r < g.nz - 1;
    if (!(lx || hx || ly || hy || lz || hz)) break;        // the rings cover the grid
    float gap = __builtin_inff();
    if (lx) gap = fminf(gap, ux - (float)(cx - r));
    if (hx) gap = fminf(gap, (float)(cx + r + 1) - ux);
    if (ly) gap = fminf(gap, uy - (float)(cy - r));
    if (hy) gap = fminf(gap, (float)(cy + r + 1) - uy);
    if (lz) gap = fminf(gap, uz - (float)(cz - r));
    if (hz) gap = fminf(gap, (float)(cz + r + 1) - uz);
    // strictly greater: at equality the next ring may hold an equal face with a lower id (NaN compares false: goes on)
    if (lower_bound2(gap, 0.f, 0.f, mu, m2, g.h) > best) break;
  }
  if (sub != 0) return;
  if (bidx >= 0) {
    const Tri q = tri_table_load(tris, bidx);
    float s, t;
    closest_st(px, py, pz, q, s, t);
    face[i] = bidx;
    point[3 * i] = q.ax + s * q.bx + t * q.cx;
    point[3 * i + 1] = q.ay + s * q.by + t * q.cy;
    point[3 * i + 2] = q.az + s * q.bz + t * q.cz;
    dist2[i] = best;
  } else {                                                 // no finite distance (non-finite inputs)
    face[i] = -1;
    point[3 * i] = point[3 * i + 1] = point[3 * i + 2] = __builtin_nanf("");
    dist2[i] = __builtin_inff();
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

#include "mesh_grid_host.h"                                // grid_view_args, lanes_ok, with_lanes

extern "C" int64_t recmv_mesh_grid_workspace_bytes(int64_t cells) {
  return cells > 0 ? (cells + ceil_div(cells, kScanTile)) * (int64_t)sizeof(int32_t) : 0;
}

extern "C" int recmv_mesh_grid_count(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                     const recmv_mesh_grid* grid, int32_t* counts, int64_t* total, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "mesh_grid_count: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31), "mesh_grid_count: at most 2^31 - 1 faces");
  GridView view;
  int rc = grid_view_args("mesh_grid_count", grid, kGridGeometry, view);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(counts && total, "mesh_grid_count: NULL output pointer");
  RECMV_REQUIRE(F == 0 || (faces && (V == 0 || verts)), "mesh_grid_count: NULL mesh pointer");
  RECMV_REQUIRE(((uintptr_t)total & 7) == 0, "mesh_grid_count: total must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)(grid->nx * grid->ny * grid->nz) * sizeof(int32_t), s));
  RECMV_HIP_TRY(hipMemsetAsync(total, 0, sizeof(int64_t), s));
  if (F == 0) return RECMV_OK;
  grid_count_kernel<<<stream_grid(F, kGridBlock), kGridBlock, 0, s>>>(verts, V, faces, F, view.g, counts,
                                                                       (unsigned long long*)total);
  return check_launch("mesh_grid_count");
}

extern "C" int recmv_mesh_grid_fill(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                    const recmv_mesh_grid* grid, const int32_t* counts, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "mesh_grid_fill: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31), "mesh_grid_fill: at most 2^31 - 1 faces");
  GridView view;
  int rc = grid_view_args("mesh_grid_fill", grid, kGridTables | (F ? kGridTris : 0), view);
  if (rc != RECMV_OK) return rc;
  const int64_t cells = grid->nx * grid->ny * grid->nz;
  RECMV_REQUIRE(counts && workspace, "mesh_grid_fill: NULL pointer");
  RECMV_REQUIRE(F == 0 || (faces && (V == 0 || verts)), "mesh_grid_fill: NULL mesh pointer");
  RECMV_REQUIRE(workspace_bytes >= recmv_mesh_grid_workspace_bytes(cells),
                "mesh_grid_fill: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)recmv_mesh_grid_workspace_bytes(cells));
  RECMV_REQUIRE(((uintptr_t)workspace & 3) == 0, "mesh_grid_fill: workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int32_t* cursor = (int32_t*)workspace;
  int32_t* sums = cursor + cells;
  const int64_t nb = ceil_div(cells, kScanTile);
  scan_sums_kernel<<<(unsigned)nb, kGridBlock, 0, s>>>(counts, cells, sums);
  rc = check_launch("mesh_grid_scan_sums");
  if (rc != RECMV_OK) return rc;
  scan_of_sums_kernel<<<1, kGridBlock, 0, s>>>(sums, nb, grid->offsets + cells);
  rc = check_launch("mesh_grid_scan_of_sums");
  if (rc != RECMV_OK) return rc;
  scan_apply_kernel<<<(unsigned)nb, kGridBlock, 0, s>>>(counts, cells, sums, grid->offsets, cursor);
  rc = check_launch("mesh_grid_scan_apply");
  if (rc != RECMV_OK || F == 0) return rc;
  grid_fill_kernel<<<stream_grid(F, kGridBlock), kGridBlock, 0, s>>>(verts, V, faces, F, view.g, grid->offsets, cursor,
                                                                      grid->entries, grid->n_entries, (float4*)grid->tris);
  return check_launch("mesh_grid_fill");
}

extern "C" int recmv_closest_point_grid(const float* p, int64_t P, const int64_t* order, int64_t F,
                                        const recmv_mesh_grid* grid, int32_t lanes, int64_t* face, float* point,
                                        float* dist2, void* stream) {
  const char* what = "closest_point_grid";
  RECMV_REQUIRE(P >= 0 && P < (1ll << 40), "%s: P=%lld must be in [0, 2^40)", what, (long long)P);
  RECMV_REQUIRE(F > 0, "%s: F=%lld: the surface must not be empty", what, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31), "%s: at most 2^31 - 1 faces", what);
  int rc = lanes_ok(what, lanes);
  if (rc != RECMV_OK) return rc;
  GridView view;
  rc = grid_view_args(what, grid, P ? kGridTables | kGridTris : kGridGeometry, view);
  if (rc != RECMV_OK || P == 0) return rc;
  RECMV_REQUIRE(p && face && point && dist2, "%s: NULL pointer", what);
  const int64_t nb = ceil_div(P * lanes, kGridBlock);
  RECMV_REQUIRE(nb < (1ll << 31), "%s: too many query points", what);
  hipStream_t s = (hipStream_t)stream;
  const float4* t4 = (const float4*)grid->tris;
  with_lanes(lanes, [&](auto G) {
    closest_point_grid_kernel<decltype(G)::value><<<(unsigned)nb, kGridBlock, 0, s>>>(p, P, order, t4, F, view, face, point,
                                                                                     dist2);
  });
  return check_launch(what);
}
