// Hole filling: the minimum-area triangulation of many closed loops at once — gfx950.  Not in the reference.
//
// What it computes: the GPU work of recmv.holes.  A loop is n vertex ids l_0 .. l_{n-1} (3 <= n <= 4096) with the points
// p_i = verts[l_i]; all arithmetic is float64 on the f32 coordinates, un-contracted.  Interval dynamic programming
// (Barequet-Sharir, Liepa with the area weight):
//   W[i][i+1] = 0;   W[i][j] = min over i < k < j of  (W[i][k] + W[k][j]) + A(i,k,j)            for j - i >= 2
//   A(i,k,j)  = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz),   u = p_k - p_i,  v = p_j - p_i,
//               cx = u.y*v.z - u.z*v.y,  cy = u.z*v.x - u.x*v.z,  cz = u.x*v.y - u.y*v.x
// A candidate replaces the best so far only when it is smaller (<), scanning k upwards from +inf: ties go to the lowest k, a
// NaN never wins, and an entry none of whose candidates is below +inf is +inf with k = i + 1.  A vertex id outside [0, V)
// reads as a NaN point.  Per loop: the total W[0][n-1] and n - 2 faces in pre-order of the split tree — the triangle of
// (i, j) at position q, the subtree of (i, k) from q + 1, the subtree of (k, j) from q + 1 + (k - i - 1) — each written as
// (l_j, l_k, l_i), the reverse of the loop direction.  Only correctly rounded operations (+ - * sqrt) in a fixed order and an
// order-independent minimum: the same bits on both routes and in tests/hole_fill_reference.py.
//
// How:
//   * Both routes keep W twice, packed triangles: row-major (W[i][k] contiguous in k) and transposed (W[k][j] contiguous in
//     k), because the second operand walks a COLUMN of W: with one table a wave's 64 lanes would read 64 rows, with two both
//     reads are 64 consecutive doubles (in LDS: ds_read_b64 over consecutive addresses, conflict-free; in memory: 512
//     contiguous bytes).  The split table is u16.  Per loop n(n-1)/2 * 18 B and 12 n B of coordinates.
//   * lds route (n <= kHoleLdsMaxN; 'auto' takes it for n <= kHoleAutoMaxN): one workgroup of four or sixteen waves per loop, the tables in LDS; the diagonals d = j - i run in
//     order with a workgroup barrier between them, the entries of a diagonal go round the waves, a wave's lanes stride over k
//     and finish with a butterfly minimum on (value, k).  Lane 0 of wave 0 then walks the tree with an explicit stack laid
//     over the transposed table, which is no longer needed.
//   * global route: the tables in the caller's workspace, one launch per diagonal over the entries of all long loops
//     (a wave per entry): the launch boundary is the barrier, and a long loop has the whole device.  Then one lane per
//     loop walks the tree.  No grid synchronisation, no flags: plain launches in stream order.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

constexpr int kHoleBlock = 256;
constexpr int kHoleWaves = kHoleBlock / kWave;
constexpr int kHoleMaxN = 4096;                            // holes.MAX_LOOP_EDGES: k fits u16, n(n-1)/2 * 18 B = 151 MB a loop
// The lds threshold.  A loop costs n(n-1)/2 * 18 + 12 n bytes of LDS (W, its transpose, the split table; the coordinates).
// The budget is 64 KiB: what a workgroup gets without opting in to more, and with 160 KiB a CU it leaves two loops resident
// per CU, so that one loop's barrier waits hide behind the other's work.  85 * 84 / 2 * 18 + 12 * 85 = 65 280 <= 65 536;
// 86 gives 66 822.
constexpr int kHoleLdsMaxN = 85;
// Where route 'auto' changes over.  Measured on an MI355X (profiles/hole_fill_timing.json), one loop a call: n = 16 lds 54 us,
// global 80 us; n = 64 lds 219 us, global 235 us; n = 85 lds 363 us, global 315 us (a launch per diagonal, 3.8 us each, but
// the whole device on every diagonal).  The capacity bound is therefore not the crossover: auto switches at 64, the largest
// measured size at which one workgroup still wins; 'lds' can be forced up to kHoleLdsMaxN.
constexpr int kHoleAutoMaxN = 64;
// The lds route's workgroup: an entry is a chain of dependent steps (two LDS reads, a float64 sqrt, six shuffles), about a
// microsecond, so a diagonal costs its entries divided by the waves: 16 waves when a loop of the launch has more than 32
// vertices, 4 (and more loops resident per CU) when none has.
constexpr int kHoleLdsBlockMax = 1024, kHoleLdsSmallN = 32;
constexpr int kRouteAuto = 0, kRouteLds = 1, kRouteGlobal = 2;

__host__ __device__ __forceinline__ int64_t tri_count(int64_t n) { return n * (n - 1) / 2; }
// W[i][j], i < j, row-major packed; and the same entry in the transposed table (row j holds i = 0 .. j - 1)
__device__ __forceinline__ int tri_w(int i, int j, int n) { return i * (2 * n - i - 1) / 2 + (j - i - 1); }
__device__ __forceinline__ int tri_t(int j, int i) { return j * (j - 1) / 2 + i; }

__host__ __device__ __forceinline__ bool on_lds(int64_t n, int route) {
  return route == kRouteLds || (route == kRouteAuto && n <= kHoleAutoMaxN);
}
__host__ __device__ __forceinline__ int64_t align8(int64_t x) { return (x + 7) & ~(int64_t)7; }
// one long loop's segment of the workspace: W | transposed W | split (u16, padded) | coordinates (f32, padded)
__host__ __device__ __forceinline__ int64_t segment_bytes(int64_t n) {
  return 16 * tri_count(n) + align8(2 * tri_count(n)) + align8(12 * n);
}

__device__ __forceinline__ double tri_area(double ix, double iy, double iz, double kx, double ky, double kz, double jx,
                                           double jy, double jz) {
  const double ux = kx - ix, uy = ky - iy, uz = kz - iz;
  const double vx = jx - ix, vy = jy - iy, vz = jz - iz;
  const double cx = uy * vz - uz * vy;
  const double cy = uz * vx - ux * vz;
  const double cz = ux * vy - uy * vx;
  return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// Entry (i, j) by one wave: lanes stride over k.  Every lane returns the minimum and its k.
__device__ __forceinline__ void wave_entry(const double* W, const double* WT, const float* P, int n, int i, int j, int lane,
                                           double& best, int& bestk) {
  const double ix = (double)P[3 * i], iy = (double)P[3 * i + 1], iz = (double)P[3 * i + 2];
  const double jx = (double)P[3 * j], jy = (double)P[3 * j + 1], jz = (double)P[3 * j + 2];
  const int row_i = tri_w(i, i + 1, n) - (i + 1);          // W[row_i + k] = W[i][k]
  const int row_j = tri_t(j, 0);                           // WT[row_j + k] = W[k][j]
  best = __builtin_inf();
  bestk = 0x7fffffff;
  for (int k = i + 1 + lane; k < j; k += kWave) {
    const double a = tri_area(ix, iy, iz, (double)P[3 * k], (double)P[3 * k + 1], (double)P[3 * k + 2], jx, jy, jz);
    const double c = (W[row_i + k] + WT[row_j + k]) + a;
    if (c < best) {
      best = c;
      bestk = k;
    }
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double ob = __shfl_xor(best, off, kWave);
    const int ok = __shfl_xor(bestk, off, kWave);
    if (ob < best || (ob == best && ok < bestk)) {          // mesh_device.h's take_min, written out: the call moves this kernel's schedule
      best = ob;
      bestk = ok;
    }
  }
  if (bestk == 0x7fffffff) bestk = i + 1;
}

__device__ __forceinline__ void load_point(const float* verts, int64_t V, int64_t id, float* p) {
  const bool in = id >= 0 && id < V;
  const float nan = __builtin_nanf("");
  p[0] = in ? verts[3 * id] : nan;
  p[1] = in ? verts[3 * id + 1] : nan;
  p[2] = in ? verts[3 * id + 2] : nan;
}

// The n - 2 faces of one loop from its split table, by one lane; `stack` holds n - 2 entries.
__device__ void emit_faces(const uint16_t* S, int n, const int64_t* lv, int64_t* faces, unsigned long long* stack) {
  int top = 0;
  stack[top++] = ((unsigned long long)(n - 1) << 16) | 0ull;                 // pos << 32 | j << 16 | i
  while (top > 0) {
    const unsigned long long e = stack[--top];
    const int i = (int)(e & 0xffff), j = (int)((e >> 16) & 0xffff);
    const int64_t pos = (int64_t)(e >> 32);
    const int k = S[tri_w(i, j, n)];
    faces[3 * pos] = lv[j];
    faces[3 * pos + 1] = lv[k];
    faces[3 * pos + 2] = lv[i];
    if (j - k >= 2) stack[top++] = ((unsigned long long)(pos + 1 + (k - i - 1)) << 32) | ((unsigned long long)j << 16) | k;
    if (k - i >= 2) stack[top++] = ((unsigned long long)(pos + 1) << 32) | ((unsigned long long)k << 16) | i;
  }
}

__global__ __launch_bounds__(kHoleLdsBlockMax) void hole_fill_lds_kernel(const float* __restrict__ verts, int64_t V,
                                                                   const int64_t* __restrict__ loop_verts,
                                                                   const int64_t* __restrict__ offsets, int route,
                                                                   int64_t* __restrict__ out_faces,
                                                                   double* __restrict__ out_weight) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int l = blockIdx.x;
  const int64_t off = offsets[l];
  const int n = (int)(offsets[l + 1] - off);
  if (!on_lds(n, route) || n > kHoleLdsMaxN) return;       // (the whole workgroup)
  const int T = (int)tri_count(n);
  double* W = (double*)smem;
  double* WT = W + T;
  float* P = (float*)(WT + T);
  uint16_t* S = (uint16_t*)(P + 3 * n);
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave, waves = blockDim.x / kWave;
  for (int i = tid; i < n; i += blockDim.x) {
    load_point(verts, V, loop_verts[off + i], P + 3 * i);
    if (i + 1 < n) {
      W[tri_w(i, i + 1, n)] = 0.;
      WT[tri_t(i + 1, i)] = 0.;
    }
  }
  __syncthreads();
  for (int d = 2; d < n; ++d) {
    for (int i = wave; i + d < n; i += waves) {
      double best;
      int bestk;
      wave_entry(W, WT, P, n, i, i + d, lane, best, bestk);
      if (lane == 0) {
        W[tri_w(i, i + d, n)] = best;
        WT[tri_t(i + d, i)] = best;
        S[tri_w(i, i + d, n)] = (uint16_t)bestk;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    out_weight[l] = W[tri_w(0, n - 1, n)];
    emit_faces(S, n, loop_verts + off, out_faces + 3 * (off - 2 * (int64_t)l), (unsigned long long*)WT);
  }
}

struct LongLoop {
  int64_t loop, n, byte_off;                               // byte_off: of the loop's segment, from the workspace's start
};

struct Segment {
  double* W;
  double* WT;
  uint16_t* S;
  float* P;
};

__device__ __forceinline__ Segment segment_of(unsigned char* ws, const LongLoop& g) {
  const int64_t T = tri_count(g.n);
  Segment s;
  s.W = (double*)(ws + g.byte_off);
  s.WT = s.W + T;
  s.S = (uint16_t*)(s.WT + T);
  s.P = (float*)((unsigned char*)s.S + align8(2 * T));
  return s;
}

// The list of the long loops and where their segments lie, by one lane: L subtractions and a running sum.
__global__ void hole_fill_plan_kernel(const int64_t* __restrict__ offsets, int64_t L, int route, int64_t first_byte,
                                      LongLoop* __restrict__ plan) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t g = 0, at = first_byte;
  for (int64_t l = 0; l < L; ++l) {
    const int64_t n = offsets[l + 1] - offsets[l];
    if (on_lds(n, route)) continue;
    plan[g++] = LongLoop{l, n, at};
    at += segment_bytes(n);
  }
}

__global__ __launch_bounds__(kHoleBlock) void hole_fill_global_init_kernel(const float* __restrict__ verts, int64_t V,
                                                                           const int64_t* __restrict__ loop_verts,
                                                                           const int64_t* __restrict__ offsets,
                                                                           const LongLoop* __restrict__ plan, int64_t g0,
                                                                           unsigned char* __restrict__ ws) {
  const LongLoop g = plan[g0 + blockIdx.y];
  const int n = (int)g.n;
  const int i = blockIdx.x * kHoleBlock + threadIdx.x;
  if (i >= n) return;
  const Segment s = segment_of(ws, g);
  load_point(verts, V, loop_verts[offsets[g.loop] + i], s.P + 3 * i);
  if (i + 1 < n) {
    s.W[tri_w(i, i + 1, n)] = 0.;
    s.WT[tri_t(i + 1, i)] = 0.;
  }
}

__global__ __launch_bounds__(kHoleBlock) void hole_fill_global_diagonal_kernel(const LongLoop* __restrict__ plan, int64_t g0,
                                                                               int d, unsigned char* __restrict__ ws) {
  const LongLoop g = plan[g0 + blockIdx.y];
  const int n = (int)g.n;
  const int lane = threadIdx.x % kWave;
  const int i = blockIdx.x * kHoleWaves + threadIdx.x / kWave;
  if (i + d >= n) return;                                  // (the whole wave)
  const Segment s = segment_of(ws, g);
  double best;
  int bestk;
  wave_entry(s.W, s.WT, s.P, n, i, i + d, lane, best, bestk);
  if (lane == 0) {
    s.W[tri_w(i, i + d, n)] = best;
    s.WT[tri_t(i + d, i)] = best;
    s.S[tri_w(i, i + d, n)] = (uint16_t)bestk;
  }
}

__global__ void hole_fill_global_emit_kernel(const int64_t* __restrict__ loop_verts, const int64_t* __restrict__ offsets,
                                             const LongLoop* __restrict__ plan, int64_t G, unsigned char* __restrict__ ws,
                                             int64_t* __restrict__ out_faces, double* __restrict__ out_weight) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const LongLoop ll = plan[g];
  const int n = (int)ll.n;
  const Segment s = segment_of(ws, ll);
  const int64_t off = offsets[ll.loop];
  out_weight[ll.loop] = s.W[tri_w(0, n - 1, n)];
  emit_faces(s.S, n, loop_verts + off, out_faces + 3 * (off - 2 * ll.loop), (unsigned long long*)s.WT);
}

// What a call needs, from the offsets in HOST memory; false with a message when they are unusable.
struct HolePlan {
  int64_t total = 0, n_lds = 0, n_long = 0, max_lds = 0, max_long = 0, ws_bytes = 0;
};

bool plan_of(const char* who, const int64_t* offsets, int64_t L, int route, HolePlan& p) {
  if (L < 0) {
    set_error("%s: L=%lld must not be negative", who, (long long)L);
    return false;
  }
  if (route != kRouteAuto && route != kRouteLds && route != kRouteGlobal) {
    set_error("%s: route=%d must be 0 (auto), 1 (lds) or 2 (global)", who, route);
    return false;
  }
  if (L == 0) return true;
  if (L >= (1ll << 31)) {
    set_error("%s: at most 2^31 - 1 loops", who);
    return false;
  }
  if (!offsets) {
    set_error("%s: NULL loop_offsets", who);
    return false;
  }
  if (offsets[0] != 0) {
    set_error("%s: loop_offsets[0]=%lld must be 0", who, (long long)offsets[0]);
    return false;
  }
  int64_t bytes = 0;
  for (int64_t l = 0; l < L; ++l) {
    const int64_t n = offsets[l + 1] - offsets[l];
    if (n < 3) {
      set_error("%s: loop %lld has %lld vertices, a loop has at least 3", who, (long long)l, (long long)n);
      return false;
    }
    if (n > kHoleMaxN) {
      set_error("%s: loop %lld has %lld vertices, more than the hard cap of %d", who, (long long)l, (long long)n, kHoleMaxN);
      return false;
    }
    if (route == kRouteLds && n > kHoleLdsMaxN) {
      set_error("%s: loop %lld has %lld vertices, the lds route takes at most %d", who, (long long)l, (long long)n,
                kHoleLdsMaxN);
      return false;
    }
    if (on_lds(n, route)) {
      ++p.n_lds;
      if (n > p.max_lds) p.max_lds = n;
    } else {
      ++p.n_long;
      if (n > p.max_long) p.max_long = n;
      bytes += segment_bytes(n);
      if (bytes > (1ll << 46)) {
        set_error("%s: the workspace of the long loops passes 2^46 bytes", who);
        return false;
      }
    }
  }
  p.total = offsets[L];
  p.ws_bytes = p.n_long ? p.n_long * (int64_t)sizeof(LongLoop) + bytes : 0;
  return true;
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_hole_fill_lds_max_edges(void) { return kHoleLdsMaxN; }
extern "C" int64_t recmv_hole_fill_auto_max_edges(void) { return kHoleAutoMaxN; }
extern "C" int64_t recmv_hole_fill_max_edges(void) { return kHoleMaxN; }

extern "C" int64_t recmv_hole_triangulate_workspace_bytes(const int64_t* loop_offsets, int64_t L, int route) {
  HolePlan p;
  return plan_of("hole_triangulate_workspace_bytes", loop_offsets, L, route, p) ? p.ws_bytes : -1;
}

extern "C" int recmv_hole_triangulate(const float* verts, int64_t V, const int64_t* loop_verts, const int64_t* loop_offsets,
                                      const int64_t* loop_offsets_device, int64_t L, int64_t* out_faces, double* out_weight,
                                      void* workspace, int64_t workspace_bytes, int route, void* stream) {
  HolePlan p;
  if (!plan_of("hole_triangulate", loop_offsets, L, route, p)) return RECMV_ERR_ARG;
  if (L == 0) return RECMV_OK;
  RECMV_REQUIRE(V >= 0, "hole_triangulate: V=%lld must not be negative", (long long)V);
  RECMV_REQUIRE(verts || V == 0, "hole_triangulate: NULL verts");
  RECMV_REQUIRE(loop_verts && loop_offsets_device, "hole_triangulate: NULL loop_verts or loop_offsets_device");
  RECMV_REQUIRE(out_faces && out_weight, "hole_triangulate: NULL output");
  RECMV_REQUIRE((const void*)out_faces != (const void*)loop_verts && (const void*)out_faces != (const void*)verts &&
                    (const void*)out_faces != (const void*)loop_offsets_device &&
                    (const void*)out_weight != (const void*)verts && (const void*)out_weight != (const void*)loop_verts &&
                    (const void*)out_weight != (const void*)loop_offsets_device &&
                    (const void*)out_weight != (const void*)out_faces,
                "hole_triangulate: an output must not alias an input or the other output");
  if (p.n_long) {
    RECMV_REQUIRE(workspace, "hole_triangulate: NULL workspace");
    RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "hole_triangulate: workspace must be 8-byte aligned");
    if (workspace_bytes < p.ws_bytes) {
      set_error("hole_triangulate: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)p.ws_bytes);
      return RECMV_ERR_WORKSPACE;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (p.n_lds) {
    const size_t lds = (size_t)(18 * tri_count(p.max_lds) + 12 * p.max_lds);     // <= 65 280
    const int block = p.max_lds > kHoleLdsSmallN ? kHoleLdsBlockMax : kHoleBlock;
    hole_fill_lds_kernel<<<(unsigned)L, block, lds, s>>>(verts, V, loop_verts, loop_offsets_device, route, out_faces,
                                                             out_weight);
    if ((rc = check_launch("hole_fill_lds")) != RECMV_OK) return rc;
  }
  if (p.n_long) {
    unsigned char* ws = (unsigned char*)workspace;
    LongLoop* plan = (LongLoop*)workspace;
    hole_fill_plan_kernel<<<1, kWave, 0, s>>>(loop_offsets_device, L, route, p.n_long * (int64_t)sizeof(LongLoop), plan);
    if ((rc = check_launch("hole_fill_plan")) != RECMV_OK) return rc;
    const int64_t kChunk = 32768;                          // loops per launch: the grid's y extent
    for (int64_t g0 = 0; g0 < p.n_long; g0 += kChunk) {
      const unsigned gy = (unsigned)(p.n_long - g0 < kChunk ? p.n_long - g0 : kChunk);
      hole_fill_global_init_kernel<<<dim3((unsigned)ceil_div(p.max_long, kHoleBlock), gy), kHoleBlock, 0, s>>>(
          verts, V, loop_verts, loop_offsets_device, plan, g0, ws);
      if ((rc = check_launch("hole_fill_global_init")) != RECMV_OK) return rc;
    }
    for (int d = 2; d < p.max_long; ++d)
      for (int64_t g0 = 0; g0 < p.n_long; g0 += kChunk) {
        const unsigned gy = (unsigned)(p.n_long - g0 < kChunk ? p.n_long - g0 : kChunk);
        hole_fill_global_diagonal_kernel<<<dim3((unsigned)ceil_div(p.max_long - d, kHoleWaves), gy), kHoleBlock, 0, s>>>(
            plan, g0, d, ws);
        if ((rc = check_launch("hole_fill_global_diagonal")) != RECMV_OK) return rc;
      }
    hole_fill_global_emit_kernel<<<(unsigned)ceil_div(p.n_long, kWave), kWave, 0, s>>>(loop_verts, loop_offsets_device, plan,
                                                                                      p.n_long, ws, out_faces, out_weight);
    if ((rc = check_launch("hole_fill_global_emit")) != RECMV_OK) return rc;
  }
  return RECMV_OK;
}
