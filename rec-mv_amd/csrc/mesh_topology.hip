// Connected components of a graph, per-face quality figures and reproducible per-segment sums (the kernels of
// recmv.topology) — gfx950.
//
// What it computes (not in the reference, which never asks what a mesh is made of):
//   * recmv_graph_components: label [n] int32 = the smallest node index of every node's connected component, for a graph of n
//     nodes given as links [M,K] int64, K = 2 or 3; a row joins its K nodes.  A row with an index outside [0, n) or with a
//     repeated index joins nothing and is counted.  The labels are the unique fixpoint "smallest member": they do not depend on
//     scheduling, on the launch shape or on the run, and neither does the number of rounds.
//   * recmv_mesh_face_stats: per face, in float64 from the f32 coordinates: the area 0.5 |(b - a) x (c - a)|, the smallest of
//     the three corner angles atan2(|u x w|, u . w), and the ratio of the longest to the shortest edge (inf when the shortest is
//     0).  An invalid face (an index outside [0, V) or repeated) gets area 0 and NaN for the other two; a valid face with a
//     corner that is not finite gets NaN throughout; both kinds are counted.
//   * recmv_segment_sums: for values [N,C] float64 sorted by segment and offsets [S + 1], the sum, minimum and maximum of every
//     column over every segment — the same bits on every run.
//
// How: integer atomics only, no float atomics.
//   * components: two arrays.  label[x] is the root of x's tree after the last compression (every tree a star); parent[r] is
//     written at roots only.  A ROUND is two launches.  Hook: one thread per row reads the labels of its nodes (nothing writes
//     label in this launch), takes the smallest root m and does atomicMin(parent + r, m) on the row's other roots r — only roots
//     are written, and each ends as the smallest root among itself and its neighbour trees, whatever the order.  Compress: one
//     thread per node walks from its old root along parent while parent[r] < r — ids strictly decrease, so the walk ends after
//     at most r steps on any contents of parent — and writes the new root into label; on the way it shortens the chain
//     (parent[r] = parent[parent[r]], an ancestor either way, so a racing reader still walks towards the same root).
//     Rounds needed (the host's cap, recmv/topology.py): call a tree ACTIVE while a row joins it to another tree.  After a
//     round the surviving active trees are the local minima among their neighbours; a survivor that absorbed nothing has all
//     its neighbours inside trees with smaller roots, so it is no local minimum in the next round and disappears.  Hence
//     active(t + 2) <= absorbed(t) <= active(t) - active(t + 1), so active(t + 2) <= active(t) / 2: no active tree is left after
//     2 ceil(log2 n) rounds, one more round finds nothing to hook, and 2 ceil(log2 n) + 2 <= 64 rounds always suffice.
//     state[0] holds the number of the last round that hooked anything: the host reads it back instead of a flag per round.
//   * face stats: one thread per face.
//   * segment sums: a segment is cut into chunks of kSegChunk values at fixed places.  First launch: one wave per chunk, lane l
//     adds the values l, l + 64, ... of the chunk in that order, then the xor shuffle tree 32, 16, ..., 1.  Second launch: one
//     wave per segment does the same over the segment's chunk results.  The caller passes the chunk table
//     (chunk_offsets[s] = the chunks of the segments before s); every range read from the tables is clamped to the arrays.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

constexpr int kTopoBlock = 256;
constexpr int kSegChunk = 4096;                            // values of a segment one wave reduces in the first launch
constexpr int kSegMaxCols = 8;

#include "mesh_device.h"                                   // index_in, clamp_i64, length3

// ---- connected components ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t parent_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void parent_store(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// K = 2 (a link) or 3 (a face) indices in [0, n), all distinct; for K = 3 mesh_device.h's tri_valid in another order of tests
template <int K>
__device__ __forceinline__ bool row_valid(const int64_t* row, int64_t n) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (!index_in(row[k], n)) return false;
  if (row[0] == row[1]) return false;
  if (K == 3 && (row[0] == row[2] || row[1] == row[2])) return false;
  return true;
}

__global__ void __launch_bounds__(kTopoBlock)
components_init_kernel(int64_t n, int32_t* __restrict__ label, int32_t* __restrict__ parent, int32_t* __restrict__ state) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n; i += stride) {
    label[i] = (int32_t)i;
    parent[i] = (int32_t)i;
  }
  if (first == 0) state[0] = state[1] = state[2] = state[3] = 0;
}

// round: this round's number (from 1); count_invalid: the first round of a run also counts the rows that join nothing
template <int K>
__global__ void __launch_bounds__(kTopoBlock)
components_hook_kernel(int64_t n, const int64_t* __restrict__ links, int64_t M, const int32_t* __restrict__ label,
                       int32_t* __restrict__ parent, int32_t* __restrict__ state, int32_t round, int32_t count_invalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
    const int64_t* row = links + K * i;
    if (!row_valid<K>(row, n)) {
      if (count_invalid) atomicAdd(state + 1, 1);
      continue;
    }
    int32_t r[K];
    int32_t m = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      r[k] = label[row[k]];
      m = r[k] < m ? r[k] : m;
    }
    if (m < 0) continue;                                   // (labels this library wrote are in [0, n))
    bool hooked = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (r[k] != m && (int64_t)r[k] < n) {
        atomicMin(parent + r[k], m);
        hooked = true;
      }
    }
    if (hooked) state[0] = round;                          // every writer of this launch stores the same number
  }
}

__global__ void __launch_bounds__(kTopoBlock)
components_compress_kernel(int64_t n, int32_t* __restrict__ label, int32_t* parent) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += stride) {
    int32_t r = label[x];
    while (index_in(r, n)) {                               // r strictly decreases: at most r steps
      const int32_t p = parent_load(parent + r);
      if (p >= r || p < 0) break;                          // a root
      const int32_t g = parent_load(parent + p);
      if (g < p && g >= 0) parent_store(parent + r, g);    // shorten the chain behind us (g is an ancestor of r)
      r = p;
    }
    label[x] = r;
  }
}

// ---- per-face figures --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double corner_angle(double ux, double uy, double uz, double wx, double wy, double wz) {
  const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
  return atan2(sqrt(cx * cx + cy * cy + cz * cz), ux * wx + uy * wy + uz * wz);
}

__global__ void __launch_bounds__(kTopoBlock)
face_stats_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F, double* __restrict__ area,
                  double* __restrict__ min_angle, double* __restrict__ ratio, int32_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double nan = __builtin_nan("");
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < F; k += stride) {
    if (!row_valid<3>(f + 3 * k, V)) {
      area[k] = 0.;
      min_angle[k] = ratio[k] = nan;
      atomicAdd(counts, 1);
      continue;
    }
    const int64_t ia = f[3 * k], ib = f[3 * k + 1], ic = f[3 * k + 2];
    const double ax = v[3 * ia], ay = v[3 * ia + 1], az = v[3 * ia + 2];
    const double bx = v[3 * ib], by = v[3 * ib + 1], bz = v[3 * ib + 2];
    const double cx = v[3 * ic], cy = v[3 * ic + 1], cz = v[3 * ic + 2];
    const double sum = ax + ay + az + bx + by + bz + cx + cy + cz;
    if (!(sum - sum == 0.)) {                              // a corner that is not finite (a finite sum cannot hide one)
      area[k] = min_angle[k] = ratio[k] = nan;
      atomicAdd(counts + 1, 1);
      continue;
    }
    const double ux = bx - ax, uy = by - ay, uz = bz - az;                         // b - a
    const double wx = cx - ax, wy = cy - ay, wz = cz - az;                         // c - a
    const double tx = cx - bx, ty = cy - by, tz = cz - bz;                         // c - b
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    area[k] = 0.5 * length3(nx, ny, nz);
    const double a0 = corner_angle(ux, uy, uz, wx, wy, wz);                        // at a: (b - a, c - a)
    const double a1 = corner_angle(tx, ty, tz, -ux, -uy, -uz);                     // at b: (c - b, a - b)
    const double a2 = corner_angle(-wx, -wy, -wz, -tx, -ty, -tz);                  // at c: (a - c, b - c)
    double lo = a0 < a1 ? a0 : a1;
    min_angle[k] = a2 < lo ? a2 : lo;
    const double e0 = length3(ux, uy, uz), e1 = length3(tx, ty, tz), e2 = length3(wx, wy, wz);
    double emin = e0 < e1 ? e0 : e1, emax = e0 > e1 ? e0 : e1;
    emin = e2 < emin ? e2 : emin;
    emax = e2 > emax ? e2 : emax;
    ratio[k] = emin == 0. ? __builtin_inf() : emax / emin;
  }
}

// ---- per-segment sums --------------------------------------------------------------------------------------------------------
struct SegRed { double sum, lo, hi; };

// rows first .. last - 1 of column `col` of x [*, C]: lane l takes the rows first + l, first + l + 64, ... in that order, then the
// shuffle tree
__device__ __forceinline__ SegRed wave_reduce(const double* __restrict__ x, int64_t C, int64_t first, int64_t last, int col,
                                              int lane) {
  SegRed r{0., __builtin_inf(), -__builtin_inf()};
  for (int64_t i = first + lane; i < last; i += kWave) {
    const double t = x[i * C + col];
    r.sum += t;
    r.lo = t < r.lo ? t : r.lo;                            // NaN never wins a minimum or a maximum; it does poison the sum
    r.hi = t > r.hi ? t : r.hi;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double s = __shfl_xor(r.sum, off, kWave), lo = __shfl_xor(r.lo, off, kWave), hi = __shfl_xor(r.hi, off, kWave);
    r.sum += s;
    r.lo = lo < r.lo ? lo : r.lo;
    r.hi = hi > r.hi ? hi : r.hi;
  }
  return r;
}

// one wave per chunk: partial [max_chunks, C, 3] = (sum, min, max) of chunk w's values of column c
__global__ void __launch_bounds__(kTopoBlock)
segment_chunks_kernel(const double* __restrict__ values, int64_t N, int32_t C, const int64_t* __restrict__ offsets, int64_t S,
                      const int64_t* __restrict__ chunk_offsets, int64_t max_chunks, double* __restrict__ partial) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x % kWave;
  if (w >= max_chunks || w >= chunk_offsets[S]) return;
  int64_t lo = 0, hi = S;                                  // the segment s with chunk_offsets[s] <= w < chunk_offsets[s + 1]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (chunk_offsets[mid] <= w) lo = mid; else hi = mid;
  }
  const int64_t s = lo;
  const int64_t c = w - chunk_offsets[s];
  if (c < 0 || w >= chunk_offsets[s + 1]) return;          // (a table that is not the one the header describes)
  const int64_t end = clamp_i64(offsets[s + 1], 0, N);
  const int64_t first = clamp_i64(offsets[s], 0, end);
  const int64_t b = c <= (end - first) / kSegChunk ? first + c * kSegChunk : end;
  const int64_t e = end - b > kSegChunk ? b + kSegChunk : end;
  for (int col = 0; col < C; ++col) {
    const SegRed r = wave_reduce(values, C, b, e, col, lane);
    if (lane == 0) {
      double* out = partial + (w * C + col) * 3;
      out[0] = r.sum; out[1] = r.lo; out[2] = r.hi;
    }
  }
}

// one wave per segment over its chunks' results
__global__ void __launch_bounds__(kTopoBlock)
segment_finish_kernel(const double* __restrict__ partial, int64_t max_chunks, int32_t C, int64_t S,
                      const int64_t* __restrict__ chunk_offsets, double* __restrict__ sum, double* __restrict__ vmin,
                      double* __restrict__ vmax) {
  const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x % kWave;
  if (s >= S) return;
  const int64_t e = clamp_i64(chunk_offsets[s + 1], 0, max_chunks);
  const int64_t b = clamp_i64(chunk_offsets[s], 0, e);
  for (int col = 0; col < C; ++col) {
    SegRed r{0., __builtin_inf(), -__builtin_inf()};
    for (int64_t i = b + lane; i < e; i += kWave) {
      const double* p = partial + (i * C + col) * 3;
      r.sum += p[0];
      r.lo = p[1] < r.lo ? p[1] : r.lo;
      r.hi = p[2] > r.hi ? p[2] : r.hi;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const double t = __shfl_xor(r.sum, off, kWave), lo = __shfl_xor(r.lo, off, kWave), hi = __shfl_xor(r.hi, off, kWave);
      r.sum += t;
      r.lo = lo < r.lo ? lo : r.lo;
      r.hi = hi > r.hi ? hi : r.hi;
    }
    if (lane == 0) {
      sum[s * C + col] = r.sum;
      vmin[s * C + col] = r.lo;
      vmax[s * C + col] = r.hi;
    }
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int recmv_graph_components(int64_t n, const int64_t* links, int64_t M, int32_t K, int32_t rounds_done,
                                      int32_t rounds, int32_t* label, int32_t* parent, int32_t* state, void* stream) {
  const char* what = "graph_components";
  RECMV_REQUIRE(n >= 0 && M >= 0, "%s: n=%lld, M=%lld must not be negative", what, (long long)n, (long long)M);
  RECMV_REQUIRE(n < (1ll << 31) && M < (1ll << 31), "%s: at most 2^31 - 1 nodes and rows", what);
  RECMV_REQUIRE(K == 2 || K == 3, "%s: K=%d must be 2 or 3", what, (int)K);
  RECMV_REQUIRE(rounds_done >= 0 && rounds >= 0 && rounds <= 64 && rounds_done <= (1 << 20),
                "%s: rounds_done=%d, rounds=%d", what, (int)rounds_done, (int)rounds);
  if (n == 0 || M == 0) return RECMV_OK;                   // nothing joins anything: the caller's labels are the node ids
  RECMV_REQUIRE(links && label && parent && state, "%s: NULL pointer", what);
  hipStream_t s = (hipStream_t)stream;
  const int gn = stream_grid(n, kTopoBlock), gm = stream_grid(M, kTopoBlock);
  int rc;
  if (rounds_done == 0) {
    components_init_kernel<<<gn, kTopoBlock, 0, s>>>(n, label, parent, state);
    rc = check_launch("graph_components_init");
    if (rc != RECMV_OK) return rc;
  }
  for (int32_t t = 0; t < rounds; ++t) {
    const int32_t round = rounds_done + t + 1;
    if (K == 2)
      components_hook_kernel<2><<<gm, kTopoBlock, 0, s>>>(n, links, M, label, parent, state, round, round == 1);
    else
      components_hook_kernel<3><<<gm, kTopoBlock, 0, s>>>(n, links, M, label, parent, state, round, round == 1);
    rc = check_launch("graph_components_hook");
    if (rc != RECMV_OK) return rc;
    components_compress_kernel<<<gn, kTopoBlock, 0, s>>>(n, label, parent);
    rc = check_launch("graph_components_compress");
    if (rc != RECMV_OK) return rc;
  }
  return RECMV_OK;
}

extern "C" int recmv_mesh_face_stats(const float* verts, int64_t V, const int64_t* faces, int64_t F, double* area,
                                     double* min_angle, double* edge_ratio, int32_t* counts, void* stream) {
  const char* what = "mesh_face_stats";
  RECMV_REQUIRE(V >= 0 && F >= 0, "%s: V=%lld, F=%lld must not be negative", what, (long long)V, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31), "%s: at most 2^31 - 1 faces", what);
  if (F == 0) return RECMV_OK;
  RECMV_REQUIRE(faces && (V == 0 || verts), "%s: NULL mesh pointer", what);
  RECMV_REQUIRE(area && min_angle && edge_ratio && counts, "%s: NULL output pointer", what);
  hipStream_t s = (hipStream_t)stream;
  RECMV_HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s));
  face_stats_kernel<<<stream_grid(F, kTopoBlock), kTopoBlock, 0, s>>>(verts, V, faces, F, area, min_angle, edge_ratio, counts);
  return check_launch(what);
}

extern "C" int64_t recmv_segment_sums_chunk(void) { return kSegChunk; }

static int64_t segment_max_chunks(int64_t N, int64_t S) { return S + N / kSegChunk; }

extern "C" int64_t recmv_segment_sums_workspace_bytes(int64_t N, int64_t S, int32_t C) {
  if (N < 0 || S <= 0 || C <= 0) return 0;
  return segment_max_chunks(N, S) * C * 3 * (int64_t)sizeof(double);
}

extern "C" int recmv_segment_sums(const double* values, int64_t N, int32_t C, const int64_t* offsets, int64_t S,
                                  const int64_t* chunk_offsets, double* sum, double* vmin, double* vmax, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  const char* what = "segment_sums";
  RECMV_REQUIRE(N >= 0 && S >= 0, "%s: N=%lld, S=%lld must not be negative", what, (long long)N, (long long)S);
  RECMV_REQUIRE(N < (1ll << 40) && S < (1ll << 31), "%s: at most 2^40 - 1 values in 2^31 - 1 segments", what);
  RECMV_REQUIRE(C >= 1 && C <= kSegMaxCols, "%s: C=%d must be in [1, %d]", what, (int)C, kSegMaxCols);
  if (S == 0) return RECMV_OK;
  RECMV_REQUIRE(offsets && chunk_offsets && sum && vmin && vmax && (N == 0 || values), "%s: NULL pointer", what);
  RECMV_REQUIRE(workspace && workspace_bytes >= recmv_segment_sums_workspace_bytes(N, S, C),
                "%s: workspace of %lld bytes, %lld needed", what, (long long)workspace_bytes,
                (long long)recmv_segment_sums_workspace_bytes(N, S, C));
  RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", what);
  const int64_t max_chunks = segment_max_chunks(N, S);
  const int64_t nb1 = ceil_div(max_chunks * kWave, kTopoBlock), nb2 = ceil_div(S * kWave, kTopoBlock);
  RECMV_REQUIRE(nb1 < (1ll << 31) && nb2 < (1ll << 31), "%s: too many segments", what);
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)workspace;
  segment_chunks_kernel<<<(unsigned)nb1, kTopoBlock, 0, s>>>(values, N, C, offsets, S, chunk_offsets, max_chunks, partial);
  int rc = check_launch("segment_sums_chunks");
  if (rc != RECMV_OK) return rc;
  segment_finish_kernel<<<(unsigned)nb2, kTopoBlock, 0, s>>>(partial, max_chunks, C, S, chunk_offsets, sum, vmin, vmax);
  return check_launch("segment_sums_finish");
}
