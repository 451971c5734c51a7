// Mesh voxelisation: the exact distance of every lattice node to a triangle mesh inside a narrow band, and the sign of
// the field by a walk along the lattice columns — gfx950.  Not in the reference.
//
// What it computes: the GPU work of recmv.voxelize.  The lattice is recmv_lattice (include/recmv_hip.h): node (i, j, k) sits
// at origin[a] + (float)idx[a] * step (one multiply and one add, un-contracted), node index (i * ny + j) * nz + k — the volume
// layout of recmv_mc_*.
//   * recmv_voxel_band_distance: per node the squared distance to and the id of the nearest face among the faces whose
//     distance d2 satisfies d2 <= band * band (the product formed once in f32); +inf and -1 when there is none.  The distance
//     is closest_tri.h's closest_st on load_tri's (a, b - a, c - a): the bits of recmv_closest_point.  Ties go to the lowest
//     face id; a face with an index outside [0, V) is skipped; NaN never wins.
//   * recmv_voxel_sign_fill: inside / outside of every node from the flags of the band nodes, and the signed, clamped distance.
//
// How (a scatter: the work scales with the surface, not with the volume):
//   * band distance: one wave per face.  The face's bounding box is dilated by `band`, turned into node indices, rounded
//     outwards by ONE FURTHER node and clipped to the lattice; the wave's lanes stride over the box's nodes, z fastest.  A node
//     with d2 <= band^2 does one 64-bit integer atomicMin on (float bits of d2) << 32 | face id — iso_remesh.hip's key — behind
//     a plain load that skips an atomic that cannot win (the key only ever falls, so a stale load skips nothing that could
//     win).  The minimum is commutative: the same bits whatever the arrival order.  No float atomics.
//     Why the box loses nothing: a node with d2 <= band^2 in f32 lies, in exact arithmetic, within band (1 + a few eps32) of
//     the face, hence within that of the face's box in every coordinate; the index of the box's edge is computed in f32 with a
//     relative error of a few eps32 of a coordinate, far below the one whole node the box is widened by as long as a step is
//     more than a few ulp of the coordinates — which a lattice with distinguishable nodes has.  A face with a NaN corner has a
//     NaN distance to every point (each of Ericson's tests fails and the interior branch divides by NaN) and is skipped; a face
//     with an infinite corner can still have a finite distance in its vertex regions and gets the whole lattice as its box.
//   * sign fill: one thread owns one (j, k) column and walks it along +x; k is the fastest index across threads, so every
//     step of the walk reads and writes one coalesced row.  A band node takes inside_band; a node outside the band takes the
//     value of the last band node before it in its column, outside if there is none — sound whenever band >= step, since a
//     lattice edge the surface crosses has both ends within one step of it.  open_columns counts the columns that END inside
//     (integer atomicAdd).
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

constexpr int kVoxBlock = 256;
constexpr int kVoxWaves = kVoxBlock / kWave;               // faces per workgroup and pass
constexpr int64_t kVoxMaxNodes = 1ll << 28;                // marching cubes' limit

#include "closest_tri.h"                                   // Tri, closest_st, load_tri
#include "mesh_device.h"                                   // finite3

struct Lat {
  float ox, oy, oz, step;
  int32_t nx, ny, nz;
};

// First and last node index along one axis of the box [lo - band, hi + band], one node wider on each side, clipped to
// [0, n - 1].  false: the box misses the lattice.  (lo, hi finite.)
__device__ __forceinline__ bool node_range(float lo, float hi, float band, float origin, float step, int32_t n, int32_t& i0,
                                           int32_t& i1) {
  float a = floorf(((lo - band) - origin) / step) - 1.f;
  float b = ceilf(((hi + band) - origin) / step) + 1.f;
  const float top = (float)(n - 1);
  if (!(a <= top) || !(b >= 0.f)) return false;            // also refuses NaN
  if (a < 0.f) a = 0.f;
  if (b > top) b = top;
  i0 = (int32_t)a;
  i1 = (int32_t)b;
  return i0 <= i1;
}

__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(a, fminf(b, c)); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(a, fmaxf(b, c)); }

__global__ void __launch_bounds__(kVoxBlock)
voxel_band_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F, Lat L, float band,
                  unsigned long long* __restrict__ keys) {
  const int lane = threadIdx.x % kWave;
  const int64_t stride = (int64_t)gridDim.x * kVoxWaves;
  const float band2 = band * band;
  for (int64_t k = (int64_t)blockIdx.x * kVoxWaves + threadIdx.x / kWave; k < F; k += stride) {
    Tri q;
    if (!load_tri(v, f, V, k, q)) continue;                // uniform over the wave
    const int64_t i0 = f[3 * k], i1 = f[3 * k + 1], i2 = f[3 * k + 2];
    const float x0 = q.ax, x1 = v[3 * i1], x2 = v[3 * i2];
    const float y0 = q.ay, y1 = v[3 * i1 + 1], y2 = v[3 * i2 + 1];
    const float z0 = q.az, z1 = v[3 * i1 + 2], z2 = v[3 * i2 + 2];
    if (x0 != x0 || x1 != x1 || x2 != x2 || y0 != y0 || y1 != y1 || y2 != y2 || z0 != z0 || z1 != z1 || z2 != z2) continue;
    int32_t a0 = 0, a1 = L.nx - 1, b0 = 0, b1 = L.ny - 1, c0 = 0, c1 = L.nz - 1;
    if (finite3(x0, x1, x2) && finite3(y0, y1, y2) && finite3(z0, z1, z2)) {
      if (!node_range(min3(x0, x1, x2), max3(x0, x1, x2), band, L.ox, L.step, L.nx, a0, a1)) continue;
      if (!node_range(min3(y0, y1, y2), max3(y0, y1, y2), band, L.oy, L.step, L.ny, b0, b1)) continue;
      if (!node_range(min3(z0, z1, z2), max3(z0, z1, z2), band, L.oz, L.step, L.nz, c0, c1)) continue;
    }
    const uint32_t nb = (uint32_t)(b1 - b0 + 1), nc = (uint32_t)(c1 - c0 + 1);
    const uint32_t total = (uint32_t)(a1 - a0 + 1) * nb * nc;                     // at most 2^28 nodes in the lattice
    const unsigned long long fid = (unsigned long long)(uint32_t)k;
    for (uint32_t t = (uint32_t)lane; t < total; t += kWave) {
      const uint32_t row = t / nc;
      const int32_t kk = c0 + (int32_t)(t - row * nc);
      const uint32_t ia = row / nb;
      const int32_t jj = b0 + (int32_t)(row - ia * nb);
      const int32_t ii = a0 + (int32_t)ia;
      const float px = L.ox + (float)ii * L.step;
      const float py = L.oy + (float)jj * L.step;
      const float pz = L.oz + (float)kk * L.step;
      float s, u;
      const float d = closest_st(px, py, pz, q, s, u);
      if (d <= band2) {                                    // NaN fails
        const int64_t n = ((int64_t)ii * L.ny + jj) * L.nz + kk;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | fid;
        if (key < keys[n]) atomicMin(keys + n, key);
      }
    }
  }
}

__global__ void __launch_bounds__(kVoxBlock)
voxel_band_finish_kernel(const unsigned long long* __restrict__ keys, int64_t N, float* __restrict__ dist2,
                         int64_t* __restrict__ face) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
    const unsigned long long key = keys ? keys[n] : ~0ull;
    if (key != ~0ull) {
      dist2[n] = __uint_as_float((uint32_t)(key >> 32));
      face[n] = (int64_t)(key & 0xffffffffull);
    } else {
      dist2[n] = __builtin_inff();
      face[n] = -1;
    }
  }
}

__global__ void __launch_bounds__(kVoxBlock)
voxel_sign_fill_kernel(const float* __restrict__ dist2, const uint8_t* __restrict__ inside_band, Lat L, float band,
                       int signed_field, float* __restrict__ sdf, uint8_t* __restrict__ inside,
                       unsigned long long* __restrict__ open_columns) {
  const int64_t columns = (int64_t)L.ny * L.nz;            // column (j, k) = j * nz + k: k fastest across threads
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= columns) return;
  const float band2 = band * band;
  uint8_t state = 0;
  for (int32_t i = 0; i < L.nx; ++i) {
    const int64_t n = (int64_t)i * columns + col;
    const float d2 = dist2[n];
    if (d2 <= band2) state = signed_field ? (uint8_t)(inside_band[n] != 0) : (uint8_t)0;
    const float d = fminf(sqrtf(d2), band);                // NaN and +inf give band
    sdf[n] = state ? -d : d;
    inside[n] = state;
  }
  if (state) atomicAdd(open_columns, 1ull);
}

// The lattice's node count, or -1 with a message when the descriptor is unusable.
int64_t lattice_nodes(const char* who, const recmv_lattice* l) {
  if (!l) {
    set_error("%s: NULL lattice", who);
    return -1;
  }
  if (!(l->step > 0.f) || !(l->step < __builtin_inff())) {
    set_error("%s: the lattice's step %g must be positive and finite", who, (double)l->step);
    return -1;
  }
  for (int a = 0; a < 3; ++a)
    if (!(l->origin[a] > -__builtin_inff() && l->origin[a] < __builtin_inff())) {
      set_error("%s: the lattice's origin must be finite", who);
      return -1;
    }
  if (l->nx < 0 || l->ny < 0 || l->nz < 0) {
    set_error("%s: dims=(%d,%d,%d) must not be negative", who, l->nx, l->ny, l->nz);
    return -1;
  }
  if (l->nx == 0 || l->ny == 0 || l->nz == 0) return 0;
  const int64_t xy = (int64_t)l->nx * l->ny;               // below 2^62
  if (xy > kVoxMaxNodes || xy * l->nz > kVoxMaxNodes) {
    set_error("%s: dims=(%d,%d,%d): at most 2^28 nodes", who, l->nx, l->ny, l->nz);
    return -1;
  }
  return xy * l->nz;
}

Lat lat_of(const recmv_lattice* l) { return Lat{l->origin[0], l->origin[1], l->origin[2], l->step, l->nx, l->ny, l->nz}; }

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_voxel_band_workspace_bytes(const recmv_lattice* lattice) {
  const int64_t N = lattice_nodes("voxel_band_workspace_bytes", lattice);
  return N < 0 ? -1 : N * (int64_t)sizeof(uint64_t);
}

extern "C" int recmv_voxel_band_distance(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                         const recmv_lattice* lattice, float band, float* dist2, int64_t* face,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "voxel_band_distance: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31) && V < (1ll << 40), "voxel_band_distance: at most 2^31 - 1 faces");
  RECMV_REQUIRE(band >= 0.f && band < __builtin_inff(), "voxel_band_distance: band=%g must be finite and not negative",
                (double)band);
  const int64_t N = lattice_nodes("voxel_band_distance", lattice);
  if (N < 0) return RECMV_ERR_ARG;
  if (N == 0) return RECMV_OK;
  RECMV_REQUIRE(dist2 && face, "voxel_band_distance: NULL output");
  const bool empty = F == 0 || V == 0;
  if (!empty) {
    RECMV_REQUIRE(verts && faces, "voxel_band_distance: NULL pointer of the mesh");
    RECMV_REQUIRE(workspace, "voxel_band_distance: NULL workspace");
    RECMV_REQUIRE(workspace_bytes >= N * (int64_t)sizeof(uint64_t), "voxel_band_distance: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)(N * (int64_t)sizeof(uint64_t)));
    RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "voxel_band_distance: workspace must be 8-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = empty ? nullptr : (unsigned long long*)workspace;
  if (!empty) {
    RECMV_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)N * sizeof(unsigned long long), s));
    voxel_band_kernel<<<stream_grid(F, kVoxWaves), kVoxBlock, 0, s>>>(verts, V, faces, F, lat_of(lattice), band, keys);
    int rc = check_launch("voxel_band");
    if (rc != RECMV_OK) return rc;
  }
  voxel_band_finish_kernel<<<stream_grid(N, kVoxBlock), kVoxBlock, 0, s>>>(keys, N, dist2, face);
  return check_launch("voxel_band_finish");
}

extern "C" int recmv_voxel_sign_fill(const float* dist2, const uint8_t* inside_band, const recmv_lattice* lattice, float band,
                                     int signed_field, float* sdf, uint8_t* inside, int64_t* open_columns, void* stream) {
  RECMV_REQUIRE(band >= 0.f && band < __builtin_inff(), "voxel_sign_fill: band=%g must be finite and not negative",
                (double)band);
  RECMV_REQUIRE(signed_field == 0 || signed_field == 1, "voxel_sign_fill: signed=%d must be 0 or 1", signed_field);
  const int64_t N = lattice_nodes("voxel_sign_fill", lattice);
  if (N < 0) return RECMV_ERR_ARG;
  RECMV_REQUIRE(open_columns, "voxel_sign_fill: NULL open_columns");
  if (N > 0) {
    RECMV_REQUIRE(dist2 && sdf && inside, "voxel_sign_fill: NULL pointer");
    RECMV_REQUIRE(!signed_field || inside_band, "voxel_sign_fill: signed=1 needs inside_band");
  }
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(open_columns, 0, sizeof(int64_t), s));
  if (N == 0) return RECMV_OK;
  const int64_t columns = (int64_t)lattice->ny * lattice->nz;
  voxel_sign_fill_kernel<<<(unsigned)ceil_div(columns, kVoxBlock), kVoxBlock, 0, s>>>(
      dist2, inside_band, lat_of(lattice), band, signed_field, sdf, inside, (unsigned long long*)open_columns);
  return check_launch("voxel_sign_fill");
}
