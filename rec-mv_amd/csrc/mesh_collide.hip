// Body-collision repair of posed garment meshes (the per-frame hot path of the animation on novel poses) — gfx950.
//
// What it computes (not in the reference, whose engineer/optimizer/surface_intesection.py stops after a ray cast):
//   * recmv_point_mesh_nearest: for B frames, the exact nearest triangle of frame b's body mesh (verts [B,V,3], one face
//     table [F,3] int64) to every garment vertex p [B,N,3]: face id and squared distance, in f32 with Ericson's
//     point-triangle test (closest_tri.h: all seven Voronoi regions).  Ties go to the lowest face id.
//   * recmv_collision_push: on the winning face, the closest point q = w0 a + w1 b + w2 c, the interpolated unit normal
//     n = normalize(w0 na + w1 nb + w2 nc) and the signed distance s = (p - q) . n.  s >= eps: the vertex is copied bit for
//     bit; -max_depth <= s < eps: p + (eps - s) n; s < -max_depth: copied and counted as unresolved.
//
// How: no float atomics, so every result is bitwise reproducible.
//   * nearest: recmv_closest_point's scheme with a frame axis.  A workgroup holds 512 garment vertices of one frame in
//     registers (2 per lane) and streams one chunk of the faces through LDS in tiles of 512 faces, each staged once per
//     tile as (a, b - a, c - a) in three float4 (24 KiB: six workgroups of a CU's 160 KiB; every lane reads the same
//     face, an LDS broadcast without bank conflicts).  Chunks run in different workgroups (blockIdx.y), frames in
//     blockIdx.z; chunks meet in one 64-bit integer atomicMin per (vertex, chunk) on (float bits of d^2) << 32 | face id.
//     A non-negative float orders like its bits, so the minimum is the smallest distance, then the lowest face id,
//     whatever order the workgroups run in.  A second launch unpacks the keys.
//   * push: one thread per vertex; the per-frame counts are summed per wave and added with one integer atomic per wave.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "closest_tri.h"
#include "mesh_device.h"                                   // wave_sum

constexpr int kNmBlock = 256;
constexpr int kNmPer = 2;                                  // garment vertices per lane
constexpr int kNmSrc = kNmBlock * kNmPer;                  // garment vertices per workgroup
constexpr int kNmTile = 512;                               // faces per LDS tile (3 float4 each: 24 KiB)
constexpr int kNmGroupsPerCU = 6;                          // 160 KiB of LDS / 24 KiB
constexpr int kPushBlock = 256;

__global__ void __launch_bounds__(kNmBlock)
mesh_nearest_kernel(const float* __restrict__ p, const float* __restrict__ verts, const int64_t* __restrict__ f,
                    int64_t N, int64_t V, int64_t F, int64_t chunk, unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[3 * kNmTile];
  const int64_t b = blockIdx.z;
  const float* __restrict__ pb = p + b * N * 3;
  const float* __restrict__ vb = verts + b * V * 3;
  const int64_t base = (int64_t)blockIdx.x * kNmSrc;
  float px[kNmPer], py[kNmPer], pz[kNmPer], best[kNmPer];
  int32_t bidx[kNmPer];
#pragma unroll
  for (int k = 0; k < kNmPer; ++k) {
    const int64_t i = base + k * kNmBlock + threadIdx.x;
    const bool ok = i < N;
    px[k] = ok ? pb[3 * i] : 0.f;
    py[k] = ok ? pb[3 * i + 1] : 0.f;
    pz[k] = ok ? pb[3 * i + 2] : 0.f;
    best[k] = __builtin_inff();
    bidx[k] = -1;
  }
  const int64_t f0 = (int64_t)blockIdx.y * chunk;
  const int64_t f1 = f0 + chunk < F ? f0 + chunk : F;
  for (int64_t fs = f0; fs < f1; fs += kNmTile) {
    const int cnt = (int)(f1 - fs < kNmTile ? f1 - fs : kNmTile);
    for (int j = threadIdx.x; j < cnt; j += kNmBlock) {
      Tri q;
      if (!load_tri(vb, f, V, fs + j, q)) {                // an invalid face never wins: NaN distance
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
      for (int k = 0; k < kNmPer; ++k) {
        float s, t;
        const float d = closest_st(px[k], py[k], pz[k], q, s, t);
        if (d < best[k]) {                                 // strict: the first (lowest) face of a tie stays; NaN never wins
          best[k] = d;
          bidx[k] = (int32_t)(fs + j);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kNmPer; ++k) {
    const int64_t i = base + k * kNmBlock + threadIdx.x;
    if (i < N && bidx[k] >= 0) {
      const unsigned long long key =
          ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned long long)(uint32_t)bidx[k];
      atomicMin(keys + b * N + i, key);
    }
  }
}

__global__ void __launch_bounds__(256)
mesh_nearest_unpack_kernel(const unsigned long long* __restrict__ keys, int64_t total, int64_t* __restrict__ face,
                           float* __restrict__ sqdist) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const unsigned long long key = keys[i];
    const bool found = key != ~0ull;                       // no finite distance (non-finite inputs, invalid faces only)
    face[i] = found ? (int64_t)(key & 0xffffffffull) : -1;
    sqdist[i] = found ? __uint_as_float((uint32_t)(key >> 32)) : __builtin_inff();
  }
}

// grid (x over the vertices, y = frame); p_out may be p (every thread reads and writes its own vertex only).
__global__ void __launch_bounds__(kPushBlock)
collision_push_kernel(const float* __restrict__ p, const float* __restrict__ verts, const float* __restrict__ vnormals,
                      const int64_t* __restrict__ f, const int64_t* __restrict__ face, int64_t N, int64_t V, int64_t F,
                      float eps, float max_depth, float* p_out, int32_t* __restrict__ moved,
                      int32_t* __restrict__ unresolved) {
  const int64_t b = blockIdx.y;
  const float* pb = p + b * N * 3;
  float* ob = p_out + b * N * 3;
  const float* __restrict__ vb = verts + b * V * 3;
  const float* __restrict__ nb = vnormals + b * V * 3;
  int n_moved = 0, n_unres = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const float x = pb[3 * i], y = pb[3 * i + 1], z = pb[3 * i + 2];
    float ox = x, oy = y, oz = z;
    const int64_t k = face[b * N + i];
    Tri q;
    if (k >= 0 && k < F && load_tri(vb, f, V, k, q)) {
      float s, t;
      closest_st(x, y, z, q, s, t);
      const int64_t i0 = f[3 * k], i1 = f[3 * k + 1], i2 = f[3 * k + 2];
      const float w0 = 1.f - s - t;
      float nx = w0 * nb[3 * i0] + s * nb[3 * i1] + t * nb[3 * i2];
      float ny = w0 * nb[3 * i0 + 1] + s * nb[3 * i1 + 1] + t * nb[3 * i2 + 1];
      float nz = w0 * nb[3 * i0 + 2] + s * nb[3 * i1 + 2] + t * nb[3 * i2 + 2];
      const float len = sqrtf(nx * nx + ny * ny + nz * nz);
      if (len > 0.f) {                                     // a vanishing or non-finite normal: the vertex is copied
        nx = nx / len; ny = ny / len; nz = nz / len;
        const float dx = (x - q.ax) - s * q.bx - t * q.cx;
        const float dy = (y - q.ay) - s * q.by - t * q.cy;
        const float dz = (z - q.az) - s * q.bz - t * q.cz;
        const float sd = dx * nx + dy * ny + dz * nz;
        if (sd < -max_depth) {
          ++n_unres;
        } else if (sd < eps) {
          const float step = eps - sd;
          ox = x + step * nx; oy = y + step * ny; oz = z + step * nz;
          ++n_moved;
        }
      }
    }
    ob[3 * i] = ox; ob[3 * i + 1] = oy; ob[3 * i + 2] = oz;
  }
  n_moved = wave_sum(n_moved);
  n_unres = wave_sum(n_unres);
  if (threadIdx.x % kWave == 0) {
    if (n_moved) atomicAdd(moved + b, n_moved);
    if (n_unres) atomicAdd(unresolved + b, n_unres);
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_point_mesh_nearest_workspace_bytes(int64_t B, int64_t N) {
  return B > 0 && N > 0 ? B * N * (int64_t)sizeof(uint64_t) : 0;
}

extern "C" int recmv_point_mesh_nearest(const float* p, const float* verts, const int64_t* faces, int64_t B, int64_t N,
                                        int64_t V, int64_t F, int64_t* face, float* sqdist, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(B >= 0 && N >= 0, "point_mesh_nearest: B=%lld, N=%lld < 0", (long long)B, (long long)N);
  RECMV_REQUIRE(V > 0 && F > 0, "point_mesh_nearest: V=%lld, F=%lld: the body mesh must not be empty", (long long)V,
                (long long)F);
  RECMV_REQUIRE(F < (1ll << 31) && V < (1ll << 31) && N < (1ll << 31) && B <= 65535,
                "point_mesh_nearest: at most 2^31 - 1 faces, vertices and points and 65535 frames");
  if (B == 0 || N == 0) return RECMV_OK;
  RECMV_REQUIRE(p && verts && faces && face && sqdist && workspace, "point_mesh_nearest: NULL pointer");
  RECMV_REQUIRE(workspace_bytes >= recmv_point_mesh_nearest_workspace_bytes(B, N),
                "point_mesh_nearest: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)recmv_point_mesh_nearest_workspace_bytes(B, N));
  RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "point_mesh_nearest: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int64_t nbx = ceil_div(N, kNmSrc);
  // split the faces into chunks so that about one round of resident workgroups runs, each chunk a whole number of tiles
  int64_t chunks = ceil_div((int64_t)kNumCU * kNmGroupsPerCU, nbx * B);
  const int64_t max_chunks = ceil_div(F, kNmTile);
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks > 65535) chunks = 65535;
  if (chunks < 1) chunks = 1;
  const int64_t chunk = ceil_div(ceil_div(F, chunks), kNmTile) * kNmTile;
  chunks = ceil_div(F, chunk);
  RECMV_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)(B * N) * sizeof(unsigned long long), s));
  mesh_nearest_kernel<<<dim3((unsigned)nbx, (unsigned)chunks, (unsigned)B), kNmBlock, 0, s>>>(p, verts, faces, N, V, F,
                                                                                             chunk, keys);
  int rc = check_launch("point_mesh_nearest");
  if (rc != RECMV_OK) return rc;
  mesh_nearest_unpack_kernel<<<stream_grid(B * N, 256), 256, 0, s>>>(keys, B * N, face, sqdist);
  return check_launch("point_mesh_nearest_unpack");
}

extern "C" int recmv_collision_push(const float* p, const float* verts, const float* vnormals, const int64_t* faces,
                                    const int64_t* face, int64_t B, int64_t N, int64_t V, int64_t F, float eps,
                                    float max_depth, float* p_out, int32_t* moved, int32_t* unresolved, void* stream) {
  RECMV_REQUIRE(B >= 0 && N >= 0, "collision_push: B=%lld, N=%lld < 0", (long long)B, (long long)N);
  RECMV_REQUIRE(V > 0 && F > 0, "collision_push: V=%lld, F=%lld: the body mesh must not be empty", (long long)V,
                (long long)F);
  RECMV_REQUIRE(F < (1ll << 31) && V < (1ll << 31) && N < (1ll << 31) && B <= 65535,
                "collision_push: at most 2^31 - 1 faces, vertices and points and 65535 frames");
  RECMV_REQUIRE(eps >= 0.f && max_depth >= 0.f, "collision_push: eps=%g, max_depth=%g must not be negative (or NaN)",
                (double)eps, (double)max_depth);
  if (B == 0) return RECMV_OK;
  RECMV_REQUIRE(moved && unresolved, "collision_push: NULL count pointer");
  RECMV_REQUIRE(N == 0 || (p && verts && vnormals && faces && face && p_out), "collision_push: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(moved, 0, (size_t)B * sizeof(int32_t), s));
  RECMV_HIP_TRY(hipMemsetAsync(unresolved, 0, (size_t)B * sizeof(int32_t), s));
  if (N == 0) return RECMV_OK;
  collision_push_kernel<<<dim3((unsigned)stream_grid(N, kPushBlock), (unsigned)B), kPushBlock, 0, s>>>(
      p, verts, vnormals, faces, face, N, V, F, eps, max_depth, p_out, moved, unresolved);
  return check_launch("collision_push");
}
