// Non-rigid ICP of a garment template (exact 1-NN and one energy evaluation with its gradient) — gfx950.
//
// What it computes: the GPU work of one NR-ICP fit of the reference (engineer/optimizer/nricp_optimizer.py:242-452,
// `NRICP_Optimizer_AdamW.fitting`, with `Local_Affine` :35-112).
//   * recmv_knn1: pytorch3d `knn_points(p, q, K=1)` + `knn_gather` (:374-376): for every source point the index of its
//     nearest target point and the squared distance; ties go to the lowest target index.
//   * recmv_nricp_energy: one inner iteration's energy (:379-424) at the affine maps (A, b) and its gradient:
//       mask_i  = inv_ok(A_i) & interior_i & cos(nc_i, A_i^-T nx_i) > threshold    (Fast3x3Minv, F.cosine_similarity)
//       vert    = sum_i mask_i |A_i x_i + b_i - c_i|^2
//       stiff   = stiffness_weight * sum_{(i,j) in edges} |(W_i - W_j) G|_F^2,  W = [A|b], G = diag(1,1,1,gamma)
//       lap     = laplacian_weight * mean_i |(1/deg_i) sum_{j in N(i)} v_j - v_i|    (v = A x + b; deg 0: |-v_i|)
//       loss    = sqrt(vert + stiff) + lap
//     pytorch3d's uniform `mesh_laplacian_smoothing` and torch's norm backward (zero vector -> zero gradient) are restated.
//
// How: no float atomics, so every result is bitwise reproducible.
//   * knn1: a workgroup holds 1024 source points in registers (4 per lane) and streams one chunk of the targets through
//     LDS in tiles of 1024 (a broadcast read per target); the chunks of one source tile run in different workgroups and
//     meet in one 64-bit integer atomicMin per (source, chunk) on the key (float bits of d) << 32 | index.  A
//     non-negative float orders like its bits, so the minimum is the smallest distance, then the lowest index,
//     whatever order the workgroups run in.  A last pass unpacks the keys.
//   * energy: three launches and no host synchronisation.  (1) one thread per vertex: mask, its share of the three sums
//     (each edge counted at its first vertex) and the Laplacian's unit vector u_i = L_i v / |L_i v|; block sums in
//     double to a fixed slot per workgroup (the grid depends on N only).  (2) one workgroup adds the slots in a fixed
//     order and writes loss, components and 1 / (2 sqrt(vert + stiff)).  (3) one thread per vertex gathers its gradient
//     over the incident-edge and neighbour lists, reading that factor from device memory.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "inv3x3_one.h"
#include "mesh_device.h"                                   // csr_range, index_in, block_partials, reduce_slots

constexpr int kKnnBlock = 256;
constexpr int kKnnPer = 4;                                 // source points per lane
constexpr int kKnnSrc = kKnnBlock * kKnnPer;               // source points per workgroup
constexpr int kKnnTile = 1024;                             // target points per LDS tile (16 KiB)
constexpr int kEnergyBlock = 256;
constexpr float kCosEps = 1e-8f;                           // F.cosine_similarity's eps

__global__ void __launch_bounds__(kKnnBlock)
knn1_kernel(const float* __restrict__ p, const float* __restrict__ q, int64_t N, int64_t M, int64_t chunk,
            unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kKnnTile];
  const int64_t base = (int64_t)blockIdx.x * kKnnSrc;
  float px[kKnnPer], py[kKnnPer], pz[kKnnPer], best[kKnnPer];
  int64_t bidx[kKnnPer];
#pragma unroll
  for (int k = 0; k < kKnnPer; ++k) {
    const int64_t i = base + k * kKnnBlock + threadIdx.x;
    const bool ok = i < N;
    px[k] = ok ? p[3 * i] : 0.f;
    py[k] = ok ? p[3 * i + 1] : 0.f;
    pz[k] = ok ? p[3 * i + 2] : 0.f;
    best[k] = __builtin_inff();
    bidx[k] = -1;
  }
  const int64_t t0 = (int64_t)blockIdx.y * chunk;
  const int64_t t1 = t0 + chunk < M ? t0 + chunk : M;
  for (int64_t ts = t0; ts < t1; ts += kKnnTile) {
    const int cnt = (int)(t1 - ts < kKnnTile ? t1 - ts : kKnnTile);
    for (int j = threadIdx.x; j < cnt; j += kKnnBlock) {
      const int64_t g = ts + j;
      tile[j] = make_float4(q[3 * g], q[3 * g + 1], q[3 * g + 2], 0.f);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float4 t = tile[j];
#pragma unroll
      for (int k = 0; k < kKnnPer; ++k) {
        const float dx = px[k] - t.x, dy = py[k] - t.y, dz = pz[k] - t.z;
        const float d = dx * dx + dy * dy + dz * dz;
        if (d < best[k]) {                                 // strict: the first (lowest) index of a tie stays
          best[k] = d;
          bidx[k] = ts + j;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kKnnPer; ++k) {
    const int64_t i = base + k * kKnnBlock + threadIdx.x;
    if (i < N && bidx[k] >= 0) {
      const unsigned long long key =
          ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned long long)(uint32_t)bidx[k];
      atomicMin(keys + i, key);
    }
  }
}

__global__ void __launch_bounds__(256)
knn1_unpack_kernel(const unsigned long long* __restrict__ keys, int64_t N, int64_t* __restrict__ idx,
                   float* __restrict__ dist) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const unsigned long long key = keys[i];
    const bool found = key != ~0ull;                       // no finite distance (non-finite inputs)
    idx[i] = found ? (int64_t)(key & 0xffffffffull) : -1;
    dist[i] = found ? __uint_as_float((uint32_t)(key >> 32)) : __builtin_inff();
  }
}

struct EnergyArgs {
  const float *A, *b, *x, *c, *nc, *nx;
  const uint8_t* interior;
  const int64_t* edges;
  const int32_t *inc_off, *inc_edge, *nbr_off, *nbr_idx;
  int64_t N, E;
  float gamma, stiffness_weight, laplacian_weight, threshold;
};

__device__ __forceinline__ void load_affine(const EnergyArgs& a, int64_t i, float* Am, float* bv) {
#pragma unroll
  for (int k = 0; k < 9; ++k) Am[k] = a.A[9 * i + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) bv[k] = a.b[3 * i + k];
}

// v = A x + b (torch.matmul(A, x) + b)
__device__ __forceinline__ void position(const EnergyArgs& a, int64_t i, float* v) {
  float Am[9], bv[3];
  load_affine(a, i, Am, bv);
  const float x0 = a.x[3 * i], x1 = a.x[3 * i + 1], x2 = a.x[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) v[r] = Am[3 * r] * x0 + Am[3 * r + 1] * x1 + Am[3 * r + 2] * x2 + bv[r];
}

// Laplacian row L_i v: (1/deg_i) sum_j v_j - v_i, or -v_i for an isolated vertex (pytorch3d's laplacian_packed)
__device__ __forceinline__ void laplacian_row(const EnergyArgs& a, int64_t i, const float* vi, float* lv) {
  int64_t k0, k1;
  csr_range(a.nbr_off, i, 2 * a.E, k0, k1);
  const float inv_deg = k1 > k0 ? 1.f / (float)(k1 - k0) : 0.f;
  float s[3] = {0.f, 0.f, 0.f};
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t j = a.nbr_idx[k];
    if (!index_in(j, a.N)) continue;
    float vj[3];
    position(a, j, vj);
#pragma unroll
    for (int r = 0; r < 3; ++r) s[r] = s[r] + vj[r] * inv_deg;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) lv[r] = s[r] - vi[r];
}

__global__ void __launch_bounds__(kEnergyBlock)
energy_forward_kernel(EnergyArgs a, uint8_t* __restrict__ mask, float* __restrict__ u, double* __restrict__ partials) {
  double acc_v = 0., acc_s = 0., acc_l = 0.;
  const float g = a.gamma;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.N; i += stride) {
    float Am[9], bv[3], inv[9], v[3];
    load_affine(a, i, Am, bv);
    position(a, i, v);
    // weight mask: Fast3x3Minv validity, interior, cosine of the closest point's normal and the warped normal A^-T nx
    const bool inv_ok = inv_one(Am, inv);
    float wn[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      wn[r] = inv[r] * a.nx[3 * i] + inv[3 + r] * a.nx[3 * i + 1] + inv[6 + r] * a.nx[3 * i + 2];
    const float c0 = a.nc[3 * i], c1 = a.nc[3 * i + 1], c2 = a.nc[3 * i + 2];
    const float n1 = fmaxf(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), kCosEps);
    const float n2 = fmaxf(sqrtf(wn[0] * wn[0] + wn[1] * wn[1] + wn[2] * wn[2]), kCosEps);
    const float cosv = (c0 / n1) * (wn[0] / n2) + (c1 / n1) * (wn[1] / n2) + (c2 / n1) * (wn[2] / n2);
    const bool m = inv_ok && a.interior[i] != 0 && cosv > a.threshold;
    mask[i] = m ? 1 : 0;
    if (m) {
      const float r0 = v[0] - a.c[3 * i], r1 = v[1] - a.c[3 * i + 1], r2 = v[2] - a.c[3 * i + 2];
      acc_v += (double)(r0 * r0) + (double)(r1 * r1) + (double)(r2 * r2);
    }
    // stiffness: every edge once, at its first vertex
    int64_t k0, k1;
    csr_range(a.inc_off, i, 2 * a.E, k0, k1);
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t e = a.inc_edge[k];
      if ((uint64_t)e >= (uint64_t)a.E || a.edges[2 * e] != i) continue;
      const int64_t j = a.edges[2 * e + 1];
      if (!index_in(j, a.N)) continue;
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float d = Am[t] - a.A[9 * j + t];
        s = s + d * d;
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float d = (bv[t] - a.b[3 * j + t]) * g;
        s = s + d * d;
      }
      acc_s += (double)s;
    }
    // Laplacian: |L_i v| and its unit vector (zero for a zero row, torch's norm backward)
    float lv[3];
    laplacian_row(a, i, v, lv);
    const float nrm = sqrtf(lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2]);
    acc_l += (double)nrm;
#pragma unroll
    for (int r = 0; r < 3; ++r) u[3 * i + r] = nrm > 0.f ? lv[r] / nrm : 0.f;
  }
  // block_partials<3, kEnergyBlock> written out, the same sums in the same order: the call moves this kernel's schedule
  __shared__ double sh[3][kEnergyBlock / kWave];
  acc_v = wave_sum(acc_v);
  acc_s = wave_sum(acc_s);
  acc_l = wave_sum(acc_l);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0) {
    sh[0][wave] = acc_v;
    sh[1][wave] = acc_s;
    sh[2][wave] = acc_l;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.;
    for (int w = 0; w < kEnergyBlock / kWave; ++w) t += sh[threadIdx.x][w];
    partials[3 * blockIdx.x + threadIdx.x] = t;
  }
}

// One workgroup: the slots in a fixed order -> scalars [loss, vert, stiff, lap], factor = 1 / (2 sqrt(vert + stiff)).
__global__ void __launch_bounds__(kEnergyBlock)
energy_reduce_kernel(const double* __restrict__ partials, int nslots, int64_t N, float stiffness_weight,
                     float laplacian_weight, float* __restrict__ scalars, float* __restrict__ factor) {
  double t[3];
  reduce_slots<3, kEnergyBlock>(partials, nslots, t);
  if (threadIdx.x == 0) {
    const float vert = (float)t[0];
    const float stiff = (float)(t[1] * (double)stiffness_weight);
    const float lap = (float)(t[2] / (double)N * (double)laplacian_weight);
    const float root = sqrtf(vert + stiff);
    scalars[0] = root + lap;
    scalars[1] = vert;
    scalars[2] = stiff;
    scalars[3] = lap;
    *factor = 0.5f / root;
  }
}

// One thread per vertex k: dL/dA_k, dL/db_k.
__global__ void __launch_bounds__(kEnergyBlock)
energy_gradient_kernel(EnergyArgs a, const uint8_t* __restrict__ mask, const float* __restrict__ u,
                       const float* __restrict__ factor, float* __restrict__ dA, float* __restrict__ db) {
  const float fac = *factor;
  const float g2 = a.gamma * a.gamma;
  const float two_sw = 2.f * a.stiffness_weight;
  const float lap_scale = a.laplacian_weight / (float)a.N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.N; k += stride) {
    float Am[9], bv[3], v[3];
    load_affine(a, k, Am, bv);
    position(a, k, v);
    // point-to-point term: d/dv of |v - c|^2 where masked
    float gp[3] = {0.f, 0.f, 0.f};
    if (mask[k]) {
#pragma unroll
      for (int r = 0; r < 3; ++r) gp[r] = 2.f * (v[r] - a.c[3 * k + r]) * fac;
    }
    // Laplacian term: (laplacian_weight / N) (L^T u)_k = (lw / N) (-u_k + sum_{i in N(k)} u_i / deg_i)
    int64_t k0, k1;
    csr_range(a.nbr_off, k, 2 * a.E, k0, k1);
    float gl[3] = {-u[3 * k], -u[3 * k + 1], -u[3 * k + 2]};
    for (int64_t t = k0; t < k1; ++t) {
      const int64_t i = a.nbr_idx[t];
      if (!index_in(i, a.N)) continue;
      const int32_t di = a.nbr_off[i + 1] - a.nbr_off[i];
      if (di <= 0) continue;
      const float w = 1.f / (float)di;
#pragma unroll
      for (int r = 0; r < 3; ++r) gl[r] = gl[r] + u[3 * i + r] * w;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) gp[r] = gp[r] + gl[r] * lap_scale;
    // stiffness: 2 sw sum_{j adjacent} (W_k - W_j) G^2
    float sA[9], sb[3];
#pragma unroll
    for (int t = 0; t < 9; ++t) sA[t] = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) sb[t] = 0.f;
    csr_range(a.inc_off, k, 2 * a.E, k0, k1);
    for (int64_t t = k0; t < k1; ++t) {
      const int64_t e = a.inc_edge[t];
      if (!index_in(e, a.E)) continue;
      const int64_t e0 = a.edges[2 * e], e1 = a.edges[2 * e + 1];
      const int64_t j = e0 == k ? e1 : e0;
      if ((uint64_t)j >= (uint64_t)a.N || (e0 != k && e1 != k)) continue;
#pragma unroll
      for (int s = 0; s < 9; ++s) sA[s] = sA[s] + (Am[s] - a.A[9 * j + s]);
#pragma unroll
      for (int s = 0; s < 3; ++s) sb[s] = sb[s] + (bv[s] - a.b[3 * j + s]);
    }
    const float x0 = a.x[3 * k], x1 = a.x[3 * k + 1], x2 = a.x[3 * k + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      dA[9 * k + 3 * r + 0] = gp[r] * x0 + sA[3 * r + 0] * two_sw * fac;
      dA[9 * k + 3 * r + 1] = gp[r] * x1 + sA[3 * r + 1] * two_sw * fac;
      dA[9 * k + 3 * r + 2] = gp[r] * x2 + sA[3 * r + 2] * two_sw * fac;
      db[3 * k + r] = gp[r] + sb[r] * (two_sw * g2) * fac;
    }
  }
}

inline int64_t energy_slots(int64_t N) { return stream_grid(N, kEnergyBlock); }
inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_knn1_workspace_bytes(int64_t N) { return N > 0 ? N * (int64_t)sizeof(uint64_t) : 0; }

extern "C" int recmv_knn1(const float* p, int64_t N, const float* q, int64_t M, int64_t* idx, float* dist,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(N >= 0, "knn1: N=%lld < 0", (long long)N);
  RECMV_REQUIRE(M > 0, "knn1: M=%lld: the target cloud must not be empty", (long long)M);
  RECMV_REQUIRE(M < (1ll << 31) && N < (1ll << 40), "knn1: at most 2^31 - 1 target points");
  if (N == 0) return RECMV_OK;
  RECMV_REQUIRE(p && q && idx && dist && workspace, "knn1: NULL pointer");
  RECMV_REQUIRE(workspace_bytes >= recmv_knn1_workspace_bytes(N), "knn1: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)recmv_knn1_workspace_bytes(N));
  RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "knn1: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int64_t nbx = ceil_div(N, kKnnSrc);
  RECMV_REQUIRE(nbx < (1ll << 31), "knn1: too many source points");
  // split the targets into chunks so that ~8 workgroups per CU run, each chunk a whole number of tiles
  int64_t chunks = ceil_div((int64_t)kNumCU * 8, nbx);
  const int64_t max_chunks = ceil_div(M, kKnnTile);
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks > 65535) chunks = 65535;
  if (chunks < 1) chunks = 1;
  const int64_t chunk = ceil_div(ceil_div(M, chunks), kKnnTile) * kKnnTile;
  chunks = ceil_div(M, chunk);
  RECMV_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)N * sizeof(unsigned long long), s));
  knn1_kernel<<<dim3((unsigned)nbx, (unsigned)chunks), kKnnBlock, 0, s>>>(p, q, N, M, chunk, keys);
  int rc = check_launch("knn1");
  if (rc != RECMV_OK) return rc;
  knn1_unpack_kernel<<<stream_grid(N, 256), 256, 0, s>>>(keys, N, idx, dist);
  return check_launch("knn1_unpack");
}

extern "C" int64_t recmv_nricp_energy_workspace_bytes(int64_t N) {
  if (N <= 0) return 0;
  return align16(energy_slots(N) * 3 * (int64_t)sizeof(double)) + 16 + N * 3 * (int64_t)sizeof(float);
}

extern "C" int recmv_nricp_energy(const float* A, const float* b, const float* x, const float* c, const float* nc,
                                  const float* nx, const uint8_t* interior, const int64_t* edges, int64_t E,
                                  const int32_t* inc_offsets, const int32_t* inc_edges, const int32_t* nbr_offsets,
                                  const int32_t* nbr_idx, int64_t N, float gamma, float stiffness_weight,
                                  float laplacian_weight, float threshold, float* scalars, uint8_t* mask, float* dA,
                                  float* db, void* workspace, int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(N > 0, "nricp_energy: N=%lld: the template must have vertices", (long long)N);
  RECMV_REQUIRE(E >= 0, "nricp_energy: E=%lld < 0", (long long)E);
  RECMV_REQUIRE(N < (1ll << 31) && 2 * E < (1ll << 31), "nricp_energy: at most 2^31 - 1 vertices and 2^30 edges");
  RECMV_REQUIRE(A && b && x && c && nc && nx && interior && inc_offsets && nbr_offsets && scalars && mask && dA && db &&
                    workspace, "nricp_energy: NULL pointer");
  RECMV_REQUIRE(E == 0 || (edges && inc_edges && nbr_idx), "nricp_energy: NULL edge list");
  RECMV_REQUIRE(workspace_bytes >= recmv_nricp_energy_workspace_bytes(N),
                "nricp_energy: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)recmv_nricp_energy_workspace_bytes(N));
  RECMV_REQUIRE(((uintptr_t)workspace & 15) == 0, "nricp_energy: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  EnergyArgs a{A, b, x, c, nc, nx, interior, edges, inc_offsets, inc_edges, nbr_offsets, nbr_idx, N, E,
               gamma, stiffness_weight, laplacian_weight, threshold};
  const int slots = (int)energy_slots(N);
  double* partials = (double*)workspace;
  char* after = (char*)workspace + align16((int64_t)slots * 3 * (int64_t)sizeof(double));
  float* factor = (float*)after;
  float* u = (float*)(after + 16);
  energy_forward_kernel<<<slots, kEnergyBlock, 0, s>>>(a, mask, u, partials);
  int rc = check_launch("nricp_energy_forward");
  if (rc != RECMV_OK) return rc;
  energy_reduce_kernel<<<1, kEnergyBlock, 0, s>>>(partials, slots, N, stiffness_weight, laplacian_weight, scalars,
                                                  factor);
  rc = check_launch("nricp_energy_reduce");
  if (rc != RECMV_OK) return rc;
  energy_gradient_kernel<<<slots, kEnergyBlock, 0, s>>>(a, mask, u, factor, dA, db);
  return check_launch("nricp_energy_gradient");
}
