// Isotropic remeshing and Loop subdivision of a garment template (the geometric hot path) — gfx950.
//
// What it computes: the GPU work of recmv.iso_remesh, a port of the two MeshLab filters the reference runs between its
// coarse and refine NR-ICP passes (engineer/utils/garment_structure.py:440-458, `remesh_garment_mesh`).
//   * recmv_closest_point: the exact closest point on a triangle mesh (verts [V,3], faces [F,3] int64) of P query points:
//     face id, point and squared distance, in f32 with Ericson's point-triangle test (Real-Time Collision Detection,
//     §5.1.5).  Ties go to the lowest face id.  Used to project free vertices onto the frozen reference surface and to
//     check a collapse against `max_surf_dist`.
//   * recmv_iso_relax: the tangential relaxation p + (I - n n^T)(c - p), c the mean of the one-ring (neighbour CSR,
//     ascending), n the unit vertex normal; fixed vertices are copied.
//   * recmv_loop_subdivide: Loop's even (vertex) and odd (edge) rules into out [V + E, 3].
//
// How: no float atomics, so every result is bitwise reproducible.
//   * closest point: a workgroup holds 512 query points in registers (2 per lane) and streams one chunk of the faces
//     through LDS in tiles of 512 faces, staged as (a, b - a, c - a) so that every test works relative to vertex a (a
//     point on a vertex or on an edge gives an exact zero).  Chunks run in different workgroups (blockIdx.y) and meet in
//     one 64-bit integer atomicMin per (point, chunk) on (float bits of d^2) << 32 | face id — recmv_knn1's scheme.  A
//     second launch recomputes the closest point on the winning face with the same function.
//   * relax and Loop: one thread per vertex (per edge for the odd rule), f64 sums in CSR order, rounded once.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

constexpr int kCpBlock = 256;
constexpr int kCpPer = 2;                                  // query points per lane
constexpr int kCpSrc = kCpBlock * kCpPer;                  // query points per workgroup
constexpr int kCpTile = 512;                               // faces per LDS tile (3 float4 each: 24 KiB)
constexpr int kIsoBlock = 256;

#include "closest_tri.h"                                   // Tri, closest_st, load_tri
#include "mesh_device.h"                                   // csr_range, index_in

__global__ void __launch_bounds__(kCpBlock)
closest_point_kernel(const float* __restrict__ p, int64_t P, const float* __restrict__ v, int64_t V,
                     const int64_t* __restrict__ f, int64_t F, int64_t chunk, unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[3 * kCpTile];
  const int64_t base = (int64_t)blockIdx.x * kCpSrc;
  float px[kCpPer], py[kCpPer], pz[kCpPer], best[kCpPer];
  int64_t bidx[kCpPer];
#pragma unroll
  for (int k = 0; k < kCpPer; ++k) {
    const int64_t i = base + k * kCpBlock + threadIdx.x;
    const bool ok = i < P;
    px[k] = ok ? p[3 * i] : 0.f;
    py[k] = ok ? p[3 * i + 1] : 0.f;
    pz[k] = ok ? p[3 * i + 2] : 0.f;
    best[k] = __builtin_inff();
    bidx[k] = -1;
  }
  const int64_t f0 = (int64_t)blockIdx.y * chunk;
  const int64_t f1 = f0 + chunk < F ? f0 + chunk : F;
  for (int64_t fs = f0; fs < f1; fs += kCpTile) {
    const int cnt = (int)(f1 - fs < kCpTile ? f1 - fs : kCpTile);
    for (int j = threadIdx.x; j < cnt; j += kCpBlock) {
      Tri q;
      if (!load_tri(v, f, V, fs + j, q)) {                 // an invalid face never wins: NaN distance
        q.ax = q.ay = q.az = __builtin_nanf("");
        q.bx = q.by = q.bz = q.cx = q.cy = q.cz = 0.f;
      }
      tile[3 * j] = make_float4(q.ax, q.ay, q.az, q.bx);
      tile[3 * j + 1] = make_float4(q.by, q.bz, q.cx, q.cy);
      tile[3 * j + 2] = make_float4(q.cz, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float4 t0 = tile[3 * j], t1 = tile[3 * j + 1], t2 = tile[3 * j + 2];
      const Tri q{t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
#pragma unroll
      for (int k = 0; k < kCpPer; ++k) {
        float s, t;
        const float d = closest_st(px[k], py[k], pz[k], q, s, t);
        if (d < best[k]) {                                 // strict: the first (lowest) face of a tie stays; NaN never wins
          best[k] = d;
          bidx[k] = fs + j;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kCpPer; ++k) {
    const int64_t i = base + k * kCpBlock + threadIdx.x;
    if (i < P && bidx[k] >= 0) {
      const unsigned long long key =
          ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned long long)(uint32_t)bidx[k];
      atomicMin(keys + i, key);
    }
  }
}

__global__ void __launch_bounds__(256)
closest_point_finish_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ p, int64_t P,
                            const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F,
                            int64_t* __restrict__ face, float* __restrict__ point, float* __restrict__ dist2) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride) {
    const unsigned long long key = keys[i];
    const int64_t k = key != ~0ull ? (int64_t)(key & 0xffffffffull) : -1;
    Tri q;
    if (k >= 0 && k < F && load_tri(v, f, V, k, q)) {
      float s, t;
      closest_st(p[3 * i], p[3 * i + 1], p[3 * i + 2], q, s, t);
      face[i] = k;
      point[3 * i] = q.ax + s * q.bx + t * q.cx;
      point[3 * i + 1] = q.ay + s * q.by + t * q.cy;
      point[3 * i + 2] = q.az + s * q.bz + t * q.cz;
      dist2[i] = __uint_as_float((uint32_t)(key >> 32));
    } else {                                               // no finite distance (non-finite inputs)
      face[i] = -1;
      point[3 * i] = point[3 * i + 1] = point[3 * i + 2] = __builtin_nanf("");
      dist2[i] = __builtin_inff();
    }
  }
}

__global__ void __launch_bounds__(kIsoBlock)
iso_relax_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ nbr, int64_t V, int64_t nnz,
                 const float* __restrict__ x, const float* __restrict__ n, const uint8_t* __restrict__ fixed,
                 float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    const double p[3] = {(double)x[3 * i], (double)x[3 * i + 1], (double)x[3 * i + 2]};
    int64_t k0, k1;
    csr_range(off, i, nnz, k0, k1);
    double s[3] = {0., 0., 0.};
    int64_t cnt = 0;
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t j = nbr[k];
      if (!index_in(j, V)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += (double)x[3 * j + c];
      ++cnt;
    }
    if (fixed[i] || cnt == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[3 * i + c] = x[3 * i + c];
      continue;
    }
    const double nv[3] = {(double)n[3 * i], (double)n[3 * i + 1], (double)n[3 * i + 2]};
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = s[c] / (double)cnt - p[c];
    const double dn = d[0] * nv[0] + d[1] * nv[1] + d[2] * nv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = (float)(p[c] + (d[c] - dn * nv[c]));
  }
}

__global__ void __launch_bounds__(kIsoBlock)
loop_even_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ nbr, int64_t V, int64_t nnz,
                 const float* __restrict__ x, const int64_t* __restrict__ bnbr, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    const double p[3] = {(double)x[3 * i], (double)x[3 * i + 1], (double)x[3 * i + 2]};
    const int64_t b0 = bnbr[2 * i], b1 = bnbr[2 * i + 1];
    if (b0 >= 0 || b1 >= 0) {                              // boundary: 3/4 p + 1/8 each boundary neighbour
      if (index_in(b0, V) && index_in(b1, V)) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          out[3 * i + c] = (float)(0.75 * p[c] + 0.125 * ((double)x[3 * b0 + c] + (double)x[3 * b1 + c]));
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * i + c] = x[3 * i + c];
      }
      continue;
    }
    int64_t k0, k1;
    csr_range(off, i, nnz, k0, k1);
    double s[3] = {0., 0., 0.};
    int64_t cnt = 0;
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t j = nbr[k];
      if (!index_in(j, V)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += (double)x[3 * j + c];
      ++cnt;
    }
    if (cnt == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[3 * i + c] = x[3 * i + c];
      continue;
    }
    const double nd = (double)cnt;
    const double g = 0.375 + 0.25 * cos(2. * M_PI / nd);
    const double beta = (0.625 - g * g) / nd;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = (float)((1. - nd * beta) * p[c] + beta * s[c]);
  }
}

__global__ void __launch_bounds__(kIsoBlock)
loop_odd_kernel(const int64_t* __restrict__ etab, int64_t E, const float* __restrict__ x, int64_t V,
                float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
    const int64_t a = etab[4 * e], b = etab[4 * e + 1], c = etab[4 * e + 2], d = etab[4 * e + 3];
    float* o = out + 3 * (V + e);
    if ((uint64_t)a >= (uint64_t)V || (uint64_t)b >= (uint64_t)V) {
      o[0] = o[1] = o[2] = __builtin_nanf("");
      continue;
    }
    const bool interior = index_in(c, V) && index_in(d, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double ab = (double)x[3 * a + k] + (double)x[3 * b + k];
      o[k] = interior ? (float)(0.375 * ab + 0.125 * ((double)x[3 * c + k] + (double)x[3 * d + k])) : (float)(0.5 * ab);
    }
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_closest_point_workspace_bytes(int64_t P) {
  return P > 0 ? P * (int64_t)sizeof(uint64_t) : 0;
}

extern "C" int recmv_closest_point(const float* p, int64_t P, const float* verts, int64_t V, const int64_t* faces,
                                   int64_t F, int64_t* face, float* point, float* dist2, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(P >= 0, "closest_point: P=%lld < 0", (long long)P);
  RECMV_REQUIRE(V > 0 && F > 0, "closest_point: V=%lld, F=%lld: the surface must not be empty", (long long)V,
                (long long)F);
  RECMV_REQUIRE(F < (1ll << 31) && V < (1ll << 40) && P < (1ll << 40), "closest_point: at most 2^31 - 1 faces");
  if (P == 0) return RECMV_OK;
  RECMV_REQUIRE(p && verts && faces && face && point && dist2 && workspace, "closest_point: NULL pointer");
  RECMV_REQUIRE(workspace_bytes >= recmv_closest_point_workspace_bytes(P),
                "closest_point: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)recmv_closest_point_workspace_bytes(P));
  RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "closest_point: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int64_t nbx = ceil_div(P, kCpSrc);
  RECMV_REQUIRE(nbx < (1ll << 31), "closest_point: too many query points");
  // split the faces into chunks so that ~8 workgroups per CU run, each chunk a whole number of tiles
  int64_t chunks = ceil_div((int64_t)kNumCU * 8, nbx);
  const int64_t max_chunks = ceil_div(F, kCpTile);
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks > 65535) chunks = 65535;
  if (chunks < 1) chunks = 1;
  const int64_t chunk = ceil_div(ceil_div(F, chunks), kCpTile) * kCpTile;
  chunks = ceil_div(F, chunk);
  RECMV_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)P * sizeof(unsigned long long), s));
  closest_point_kernel<<<dim3((unsigned)nbx, (unsigned)chunks), kCpBlock, 0, s>>>(p, P, verts, V, faces, F, chunk, keys);
  int rc = check_launch("closest_point");
  if (rc != RECMV_OK) return rc;
  closest_point_finish_kernel<<<stream_grid(P, 256), 256, 0, s>>>(keys, p, P, verts, V, faces, F, face, point, dist2);
  return check_launch("closest_point_finish");
}

extern "C" int recmv_iso_relax(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz,
                               const float* verts, const float* normals, const uint8_t* fixed, float* out, void* stream) {
  RECMV_REQUIRE(V >= 0 && nnz >= 0, "iso_relax: V=%lld, nnz=%lld must not be negative", (long long)V, (long long)nnz);
  RECMV_REQUIRE(V < (1ll << 31) && nnz < (1ll << 31), "iso_relax: at most 2^31 - 1 vertices and neighbour entries");
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(nbr_offsets && verts && normals && fixed && out, "iso_relax: NULL pointer");
  RECMV_REQUIRE(nnz == 0 || nbr_idx, "iso_relax: NULL neighbour list");
  RECMV_REQUIRE(out != verts, "iso_relax: out must not alias verts");
  iso_relax_kernel<<<stream_grid(V, kIsoBlock), kIsoBlock, 0, (hipStream_t)stream>>>(nbr_offsets, nbr_idx, V, nnz, verts,
                                                                                    normals, fixed, out);
  return check_launch("iso_relax");
}

extern "C" int recmv_loop_subdivide(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz,
                                    const float* verts, const int64_t* boundary_nbrs, const int64_t* edge_table,
                                    int64_t E, float* out, void* stream) {
  RECMV_REQUIRE(V >= 0 && nnz >= 0 && E >= 0, "loop_subdivide: V=%lld, nnz=%lld, E=%lld must not be negative",
                (long long)V, (long long)nnz, (long long)E);
  RECMV_REQUIRE(V < (1ll << 31) && nnz < (1ll << 31) && E < (1ll << 31),
                "loop_subdivide: at most 2^31 - 1 vertices, neighbour entries and edges");
  if (V == 0 && E == 0) return RECMV_OK;
  RECMV_REQUIRE(nbr_offsets && verts && boundary_nbrs && out, "loop_subdivide: NULL pointer");
  RECMV_REQUIRE(nnz == 0 || nbr_idx, "loop_subdivide: NULL neighbour list");
  RECMV_REQUIRE(E == 0 || edge_table, "loop_subdivide: NULL edge table");
  RECMV_REQUIRE(out != verts, "loop_subdivide: out must not alias verts");
  hipStream_t s = (hipStream_t)stream;
  if (V > 0) {
    loop_even_kernel<<<stream_grid(V, kIsoBlock), kIsoBlock, 0, s>>>(nbr_offsets, nbr_idx, V, nnz, verts, boundary_nbrs,
                                                                      out);
    int rc = check_launch("loop_even");
    if (rc != RECMV_OK) return rc;
  }
  if (E == 0) return RECMV_OK;
  loop_odd_kernel<<<stream_grid(E, kIsoBlock), kIsoBlock, 0, s>>>(edge_table, E, verts, V, out);
  return check_launch("loop_odd");
}
