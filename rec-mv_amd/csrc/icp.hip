// The normal equations of one ICP iteration from given correspondences (recmv/align.py) — gfx950.
//
// What it computes (the reference's engineer/optimizer/icp_optimzier.py forms the 3x3 covariance of a rigid fit in torch):
// for the pairs (x_i, q_i) that pass the acceptance rules of include/recmv_hip.h the RECMV_ICP_SUMS float64 sums a closed-form
// point-to-point fit (Umeyama) and a Gauss-Newton point-to-plane step need, all about one centre.  q, face and dist2 are taken
// as the closest-point query returned them; only the border rule looks at the face again, through closest_tri.h's
// closest_st_region on the triangle load_tri forms: the search's own arithmetic, so the region is the one the search took.
//
// How: no float atomics, and a summation order that depends on P alone.
//   * icp_accumulate_kernel<PLANE>: block b's thread t takes the pairs (b * 256 + t) + k * (blocks * 256) and adds into
//     registers (19 doubles without the plane part, 55 with it: one wave per SIMD, no spill); a wave meets in a xor-shuffle
//     butterfly (32, 16, .., 1: every lane ends with the same bits), the block's four waves through LDS in wave order, and
//     the block stores one slab of 56 doubles in the workspace.
//   * icp_finish_kernel: behind the launch boundary, one block adds the slabs in block order and writes all 56 sums (zeros
//     for P = 0).
//   The number of blocks is min(ceil(P / 256), kIcpMaxBlocks): not the device's CU count, so the bits are the same on
//   every run and every card.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "closest_tri.h"                                   // Tri, closest_st_region, load_tri
#include "mesh_device.h"                                   // finite3, index_in

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kIcpMaxBlocks = 256;                         // 2 pairs per thread at the evaluation's 10^5 samples
constexpr int kSums = RECMV_ICP_SUMS;
constexpr int kPointSums = 19;                             // entries 0 .. 18: what the point metric needs

struct Centre {
  double x, y, z;
};

template <bool PLANE>
__global__ void __launch_bounds__(kBlock)
icp_accumulate_kernel(const float* __restrict__ x, const float* __restrict__ q, const int64_t* __restrict__ face,
                      const float* __restrict__ dist2, int64_t P, const float* __restrict__ verts, int64_t V,
                      const int64_t* __restrict__ faces, int64_t F, const uint8_t* __restrict__ border,
                      const float* __restrict__ max_dist2, Centre c, double* __restrict__ slabs) {
  constexpr int N = PLANE ? kSums - 1 : kPointSums;        // entry 55 is reserved: never accumulated
  __shared__ double lds[kWaves][kSums];
  double acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = 0.;
  const float limit = max_dist2 ? *max_dist2 : 0.f;
  const int64_t step = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += step) {
    const int64_t k = face[i];
    const float d2 = dist2[i];
    const float xx = x[3 * i], xy = x[3 * i + 1], xz = x[3 * i + 2];
    const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    if (!index_in(k, F)) continue;
    if (!finite3(xx, xy, xz) || !finite3(qx, qy, qz) || !__builtin_isfinite(d2)) continue;
    if (max_dist2 && !(d2 <= limit)) continue;             // (a NaN limit accepts nothing)
    Tri tri;
    if (!load_tri(verts, faces, V, k, tri)) continue;
    if (border) {
      float s, t;
      int region;
      closest_st_region(xx, xy, xz, tri, s, t, region);
      if (region != kInside && ((border[k] >> region) & 1)) continue;
    }
    double m[3];
    if (PLANE) {
      const int64_t i0 = faces[3 * k], i1 = faces[3 * k + 1], i2 = faces[3 * k + 2];     // in [0, V): load_tri looked
      const double ax = verts[3 * i0], ay = verts[3 * i0 + 1], az = verts[3 * i0 + 2];
      const double bx = (double)verts[3 * i1] - ax, by = (double)verts[3 * i1 + 1] - ay, bz = (double)verts[3 * i1 + 2] - az;
      const double cx = (double)verts[3 * i2] - ax, cy = (double)verts[3 * i2 + 1] - ay, cz = (double)verts[3 * i2 + 2] - az;
      m[0] = by * cz - bz * cy;
      m[1] = bz * cx - bx * cz;
      m[2] = bx * cy - by * cx;
      const double len = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
      if (!(len > 0.) || !__builtin_isfinite(len)) continue;                             // a face without area
      m[0] /= len; m[1] /= len; m[2] /= len;
    }
    const double u[3] = {(double)xx - c.x, (double)xy - c.y, (double)xz - c.z};
    const double w[3] = {(double)qx - c.x, (double)qy - c.y, (double)qz - c.z};
    const double e[3] = {u[0] - w[0], u[1] - w[1], u[2] - w[2]};
    acc[0] += 1.;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      acc[1 + a] += u[a];
      acc[4 + a] += w[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[7 + 3 * a + b] += u[a] * w[b];
    }
    acc[16] += u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    acc[17] += w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    acc[18] += e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    if (PLANE) {
      const double J[7] = {u[1] * m[2] - u[2] * m[1], u[2] * m[0] - u[0] * m[2], u[0] * m[1] - u[1] * m[0],
                           m[0], m[1], m[2], u[0] * m[0] + u[1] * m[1] + u[2] * m[2]};
      const double r = e[0] * m[0] + e[1] * m[1] + e[2] * m[2];
      int at = kPointSums;
#pragma unroll
      for (int a = 0; a < 7; ++a) {
#pragma unroll
        for (int b = a; b < 7; ++b) acc[at++] += J[a] * J[b];
      }
#pragma unroll
      for (int a = 0; a < 7; ++a) acc[47 + a] += J[a] * r;
      acc[54] += r * r;
    }
  }
  // the wave: a butterfly, the same tree whatever the data; every lane ends with the wave's sum (mesh_device.h's wave_sum,
  // written out: the call moves this kernel's schedule)
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, kWave);
  }
  if (threadIdx.x % kWave == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) lds[threadIdx.x / kWave][k] = acc[k];
  }
  __syncthreads();
  // the block: its waves in wave order; what this instance does not accumulate is an exact zero
  if (threadIdx.x < kSums) {
    double s = 0.;
    if ((int)threadIdx.x < N) {
      s = lds[0][threadIdx.x];
#pragma unroll
      for (int v = 1; v < kWaves; ++v) s += lds[v][threadIdx.x];
    }
    slabs[(int64_t)blockIdx.x * kSums + threadIdx.x] = s;
  }
}

// the slabs in block order (n_slabs = 0: zeros)
__global__ void __launch_bounds__(kWave)
icp_finish_kernel(const double* __restrict__ slabs, int n_slabs, double* __restrict__ sums) {
  if (threadIdx.x >= kSums) return;
  double s = 0.;
  for (int b = 0; b < n_slabs; ++b) s += slabs[(int64_t)b * kSums + threadIdx.x];
  sums[threadIdx.x] = s;
}

inline int64_t icp_blocks(int64_t P) {
  if (P <= 0) return 0;
  const int64_t nb = ceil_div(P, kBlock);
  return nb < kIcpMaxBlocks ? nb : kIcpMaxBlocks;
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_icp_accumulate_workspace_bytes(int64_t P) {
  return icp_blocks(P) * kSums * (int64_t)sizeof(double);
}

extern "C" int recmv_icp_accumulate(const float* x, const float* q, const int64_t* face, const float* dist2, int64_t P,
                                    const float* verts, int64_t V, const int64_t* faces, int64_t F, const uint8_t* border,
                                    const float* max_dist2, const double* centre, int32_t with_plane, double* sums,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "icp_accumulate";
  RECMV_REQUIRE(P >= 0 && V >= 0 && F >= 0, "%s: P=%lld, V=%lld, F=%lld must not be negative", what, (long long)P,
                (long long)V, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31) && V < (1ll << 40) && P < (1ll << 40), "%s: at most 2^31 - 1 faces, 2^40 - 1 points", what);
  RECMV_REQUIRE(P == 0 || (V > 0 && F > 0), "%s: V=%lld, F=%lld: the surface must not be empty", what, (long long)V,
                (long long)F);
  RECMV_REQUIRE(P == 0 || (x && q && face && dist2), "%s: NULL pointer of the pairs", what);
  RECMV_REQUIRE(P == 0 || (verts && faces), "%s: NULL pointer of the mesh", what);
  RECMV_REQUIRE(centre, "%s: NULL centre", what);
  RECMV_REQUIRE(sums && ((uintptr_t)sums & 7) == 0, "%s: sums must be given and 8-byte aligned", what);
  RECMV_REQUIRE(with_plane == 0 || with_plane == 1, "%s: with_plane=%d must be 0 or 1", what, (int)with_plane);
  const int64_t need = recmv_icp_accumulate_workspace_bytes(P);
  if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7) != 0)) {
    set_error("%s: workspace of %lld bytes at %p, %lld needed, 8-byte aligned", what, (long long)(workspace ? workspace_bytes : 0),
              workspace, (long long)need);
    return RECMV_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)icp_blocks(P);
  double* slabs = (double*)workspace;
  if (nb > 0) {
    const Centre c{centre[0], centre[1], centre[2]};
    if (with_plane)
      icp_accumulate_kernel<true><<<nb, kBlock, 0, st>>>(x, q, face, dist2, P, verts, V, faces, F, border, max_dist2, c, slabs);
    else
      icp_accumulate_kernel<false><<<nb, kBlock, 0, st>>>(x, q, face, dist2, P, verts, V, faces, F, border, max_dist2, c, slabs);
    const int rc = check_launch(what);
    if (rc != RECMV_OK) return rc;
  }
  icp_finish_kernel<<<1, kWave, 0, st>>>(slabs, nb, sums);
  return check_launch(what);
}
