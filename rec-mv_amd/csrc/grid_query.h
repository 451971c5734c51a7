// The uniform grid over a triangle mesh: what its binning (mesh_grid.hip) and every query on it (mesh_grid.hip's closest
// point, mesh_intersect.hip's triangle pairs, segment_mesh.hip's segments) must compute alike, and the plumbing the queries
// share.  Include it inside namespace recmv after `#pragma clang fp contract(off)`, like closest_tri.h.  Device code only: no
// RECMV_REQUIRE and no HIP calls, so that the host checks of tools/ compile it under tools/host_check/common.h.
#pragma once
#include "closest_tri.h"                                   // Tri, for the triangle table
#include "mesh_device.h"                                   // index_in

struct Grid {
  float ox, oy, oz, h, inv_h;
  int nx, ny, nz;
};

struct Range {
  int x0, x1, y0, y1, z0, z1;
};

// A coordinate in cell units relative to the grid's origin: the ONE expression binning and query share.
__device__ __forceinline__ float cell_coord(float x, float o, float inv_h) { return (x - o) * inv_h; }

// The cell of a coordinate in cell units, clamped into [0, n) (NaN gives 0: fmaxf returns its other argument).
__device__ __forceinline__ int cell_index(float u, int n) {
  return (int)fminf(fmaxf(floorf(u), 0.f), (float)(n - 1));
}

// The linear index of cell (x, y, z).
__device__ __forceinline__ int cell_id(const Grid& g, int x, int y, int z) { return (z * g.ny + y) * g.nx + x; }

// The cells face k's axis-aligned box overlaps (false: an index outside [0, V), the face is binned nowhere).  Used by the
// count and the fill pass alike, and by the queries that need a face's range again.
__device__ __forceinline__ bool face_range(const float* __restrict__ v, const int64_t* __restrict__ f, int64_t V,
                                           int64_t k, const Grid& g, Range& r) {
  const int64_t i0 = f[3 * k], i1 = f[3 * k + 1], i2 = f[3 * k + 2];
  if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) return false;
  const float ax = v[3 * i0], ay = v[3 * i0 + 1], az = v[3 * i0 + 2];
  const float bx = v[3 * i1], by = v[3 * i1 + 1], bz = v[3 * i1 + 2];
  const float cx = v[3 * i2], cy = v[3 * i2 + 1], cz = v[3 * i2 + 2];
  r.x0 = cell_index(cell_coord(fminf(fminf(ax, bx), cx), g.ox, g.inv_h), g.nx);
  r.x1 = cell_index(cell_coord(fmaxf(fmaxf(ax, bx), cx), g.ox, g.inv_h), g.nx);
  r.y0 = cell_index(cell_coord(fminf(fminf(ay, by), cy), g.oy, g.inv_h), g.ny);
  r.y1 = cell_index(cell_coord(fmaxf(fmaxf(ay, by), cy), g.oy, g.inv_h), g.ny);
  r.z0 = cell_index(cell_coord(fminf(fminf(az, bz), cz), g.oz, g.inv_h), g.nz);
  r.z1 = cell_index(cell_coord(fmaxf(fmaxf(az, bz), cz), g.oz, g.inv_h), g.nz);
  if (r.x1 < r.x0) r.x1 = r.x0;                            // (non-finite coordinates)
  if (r.y1 < r.y0) r.y1 = r.y0;
  if (r.z1 < r.z0) r.z1 = r.z0;
  return true;
}

__device__ __forceinline__ int64_t range_cells(const Range& r) {
  return (int64_t)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) * (r.z1 - r.z0 + 1);
}

// Cell c of the range_cells(r) cells of a range, x fastest.
__device__ __forceinline__ void range_cell(const Range& r, int64_t c, int& x, int& y, int& z) {
  const int wx = r.x1 - r.x0 + 1, wy = r.y1 - r.y0 + 1;
  x = r.x0 + (int)(c % wx);
  y = r.y0 + (int)((c / wx) % wy);
  z = r.z0 + (int)(c / ((int64_t)wx * wy));
}

// The triangle table of a grid: face k as (a, b - a, c - a) — load_tri's values — in three float4, the last three floats 0.
__device__ __forceinline__ void tri_table_store(float4* __restrict__ tris, int64_t k, const Tri& q) {
  tris[3 * k] = make_float4(q.ax, q.ay, q.az, q.bx);
  tris[3 * k + 1] = make_float4(q.by, q.bz, q.cx, q.cy);
  tris[3 * k + 2] = make_float4(q.cz, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ Tri tri_table_load(const float4* __restrict__ tris, int64_t k) {
  const float4 t0 = tris[3 * k], t1 = tris[3 * k + 1], t2 = tris[3 * k + 2];
  return Tri{t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
}

// What a query reads of a built grid; passed to the kernels by value.
struct GridView {
  Grid g;
  const int32_t* offsets;                                  // [cells + 1]
  const int32_t* entries;                                  // [n_entries]
  int64_t n_entries;
};

// op(face) for every entry of a cell.  The cell's bounds are clamped into [0, n_entries] and an entry outside [0, F) is
// skipped: what keeps a query inside its buffers when it is handed a damaged table.
template <class Op>
__device__ __forceinline__ void for_each_entry(const GridView& v, int cell, int64_t F, Op op) {
  int e0 = v.offsets[cell], e1 = v.offsets[cell + 1];
  if (e0 < 0) e0 = 0;
  if ((int64_t)e1 > v.n_entries) e1 = (int)v.n_entries;
  for (int e = e0; e < e1; ++e) {
    const int k = v.entries[e];
    if (!index_in(k, F)) continue;
    op(k);
  }
}
