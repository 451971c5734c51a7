// Generalized winding numbers of points about a triangle mesh: w(q) = (sum over the faces of their signed solid angle seen
// from q) / 4 pi — gfx950.  Not in the reference.
//
// What it computes: the GPU work of recmv.winding.  The per-face term is solid_angle.h's in f32, the sum over the faces is
// accumulated in f64 and the result is f64.  A face with an index outside [0, V) contributes 0, a face without area
// contributes 0, a face with a corner that is not finite makes every w NaN, a query that is not finite gets NaN.
//   * recmv_winding_exact: every face for every query.
//   * recmv_winding_tree_cells / _build / _query: a dense pyramid of cells over a cube around the mesh; a node far from the
//     query (|q - centre| > beta r) contributes its first-order (dipole) term, the faces of a finest cell that is near are
//     evaluated exactly.
//
// How:
//   * exact: one thread per query, grid (query blocks, face chunks).  The faces are cut into chunks of kChunkFaces, a
//     LIBRARY CONSTANT, so the partition — and with it the order of every f64 addition — does not depend on P, on the launch
//     or on scheduling.  A workgroup stages kTile faces at a time in LDS as 9 floats each (the staging thread's stride of 9
//     words is odd: no bank conflict on the write; every lane then reads the same face: a broadcast).  Each thread adds its
//     terms in ascending face order into one f64 and writes partial[chunk][query]; a second kernel adds a query's partials in
//     ascending chunk order and divides by 4 pi.  No atomics.
//   * tree: level l of the pyramid has 2^l cells per axis, l = 0 .. levels; node (l, i, j, k) sits at
//     (8^l - 1) / 7 + (i * 2^l + j) * 2^l + k, x slowest.  A face belongs to the finest cell that holds its centroid.  The
//     finest level is filled by one thread per cell that adds the cell's faces in their sorted order (and writes their corners
//     to the sorted corner table), each coarser level by one thread per parent that adds its 8 children, x slowest.  The
//     query walks depth-first in that child order without a stack: the cell coordinates of the current node ARE the path
//     (the low bits of i, j, k at every level are the child cursors), so the state is four integers in registers.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

constexpr int kWindBlock = 256;
constexpr int kTile = 256;                                  // faces staged per pass: 9 KB of LDS
constexpr int64_t kChunkFaces = 4096;                       // the fixed partition of the faces (recmv_winding_chunk_faces)
constexpr int kMaxLevels = 7;
constexpr double kFourPi = 12.566370614359172953850573533118;

#include "solid_angle.h"
#include "mesh_device.h"                                   // finite3, index_in

// partial[chunk * P + p] = the sum of the solid angles of the faces [chunk * kChunkFaces, min(F, (chunk + 1) * kChunkFaces))
// seen from p, added in ascending face order in f64.
__global__ void __launch_bounds__(kWindBlock)
winding_exact_kernel(const float* __restrict__ p, int64_t P, const float* __restrict__ v, int64_t V,
                     const int64_t* __restrict__ f, int64_t F, double* __restrict__ partial) {
  __shared__ float tile[kTile * 9];
  const int64_t chunk = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = q < P;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    qx = p[3 * q]; qy = p[3 * q + 1]; qz = p[3 * q + 2];
    if (!finite3(qx, qy, qz)) qx = qy = qz = __builtin_nanf("");
  }
  const int64_t first = chunk * kChunkFaces;
  const int64_t last = first + kChunkFaces < F ? first + kChunkFaces : F;
  double sum = 0.;
  for (int64_t base = first; base < last; base += kTile) {
    const int n = (int)(last - base < kTile ? last - base : kTile);
    __syncthreads();                                        // the previous tile has been read
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) load_corners(v, f, V, base + i, tile + 9 * i);
    __syncthreads();
    if (live)
      for (int i = 0; i < n; ++i) sum += (double)solid_angle(qx, qy, qz, tile + 9 * i);
  }
  if (live) partial[chunk * P + q] = sum;
}

__global__ void __launch_bounds__(kWindBlock)
winding_reduce_kernel(const double* __restrict__ partial, int64_t chunks, int64_t P, double* __restrict__ w) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P) return;
  double sum = 0.;
  for (int64_t c = 0; c < chunks; ++c) sum += partial[c * P + q];
  w[q] = sum / kFourPi;
}

struct Cube {
  float ox, oy, oz, side;
  int32_t levels;
};

__device__ __forceinline__ int64_t level_offset(int l) { return ((1ll << (3 * l)) - 1) / 7; }

// The cell index along one axis of a coordinate at a level of n cells per axis, clamped to [0, n - 1].
__device__ __forceinline__ int32_t cell_of(float x, float origin, float side, int32_t n) {
  const float t = floorf((x - origin) / (side / (float)n));
  if (!(t > 0.f)) return 0;
  return t < (float)(n - 1) ? (int32_t)t : n - 1;
}

// cells[k] = the finest cell of face k's centroid ((A + B) + C) / 3, (i * n + j) * n + k with n = 2^levels; -1 for a face with
// an index outside [0, V), -2 for a face with a corner that is not finite.
__global__ void __launch_bounds__(kWindBlock)
winding_cells_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F, Cube c,
                     int64_t* __restrict__ cells) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int32_t n = 1 << c.levels;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < F; k += stride) {
    float t[9];
    int64_t cell;
    if (!load_corners(v, f, V, k, t)) {
      cell = -1;
    } else if (t[0] != t[0]) {
      cell = -2;
    } else {
      const int32_t i = cell_of(((t[0] + t[3]) + t[6]) / 3.f, c.ox, c.side, n);
      const int32_t j = cell_of(((t[1] + t[4]) + t[7]) / 3.f, c.oy, c.side, n);
      const int32_t kk = cell_of(((t[2] + t[5]) + t[8]) / 3.f, c.oz, c.side, n);
      cell = ((int64_t)i * n + j) * n + kk;
    }
    cells[k] = cell;
  }
}

// The finest level: thread = cell; its faces are order[cell_start[cell] .. cell_start[cell + 1]).
__global__ void __launch_bounds__(kWindBlock)
winding_leaves_kernel(const float* __restrict__ v, int64_t V, const int64_t* __restrict__ f, int64_t F,
                      const int64_t* __restrict__ order, int64_t n_faces, const int64_t* __restrict__ cell_start, int levels,
                      float* __restrict__ nodes, float* __restrict__ tris) {
  const int64_t cells = 1ll << (3 * levels);
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= cells) return;
  NodeSum s;
  node_clear(s);
  int64_t i0 = cell_start[cell], i1 = cell_start[cell + 1];   // clipped to the tables, whatever the caller wrote
  if (i0 < 0) i0 = 0;
  if (i1 > n_faces) i1 = n_faces;
  for (int64_t i = i0; i < i1; ++i) {
    float t[9];
    const int64_t k = order[i];
    if (!index_in(k, F)) continue;                           // no such face: its row of tris is left alone
    load_corners(v, f, V, k, t);
    for (int a = 0; a < 9; ++a) tris[9 * i + a] = t[a];
    node_add_face(s, t);
  }
  node_store(s, nodes + (level_offset(levels) + cell) * kNodeFloats);
}

// Level l from level l + 1: thread = parent; the children in the order x, y, z with z fastest.
__global__ void __launch_bounds__(kWindBlock)
winding_parents_kernel(int l, float* __restrict__ nodes) {
  const int64_t cells = 1ll << (3 * l);
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= cells) return;
  const int64_t n = 1ll << l, m = 2 * n;
  const int64_t i = cell / (n * n), j = (cell / n) % n, k = cell % n;
  const float* child = nodes + level_offset(l + 1) * kNodeFloats;
  NodeSum s;
  node_clear(s);
  for (int c = 0; c < 8; ++c) {
    const int64_t ci = 2 * i + (c >> 2), cj = 2 * j + ((c >> 1) & 1), ck = 2 * k + (c & 1);
    node_add_node(s, child + ((ci * m + cj) * m + ck) * kNodeFloats);
  }
  node_store(s, nodes + (level_offset(l) + cell) * kNodeFloats);
}

// Thread t answers query order[t] (t itself when order is NULL).
__global__ void __launch_bounds__(kWindBlock)
winding_tree_kernel(const float* __restrict__ p, int64_t P, const int64_t* __restrict__ order, int levels,
                    const float* __restrict__ nodes, const int64_t* __restrict__ cell_start, const float* __restrict__ tris,
                    int64_t n_faces, float beta2, double* __restrict__ w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P) return;
  const int64_t q = order ? order[t] : t;
  if (!index_in(q, P)) return;                               // an order that is no permutation writes nothing out of bounds
  const float qx = p[3 * q], qy = p[3 * q + 1], qz = p[3 * q + 2];
  if (!finite3(qx, qy, qz)) {
    w[q] = (double)__builtin_nanf("");
    return;
  }
  double sum = 0.;
  int l = 0;
  int32_t i = 0, j = 0, k = 0;
  for (;;) {
    const int64_t cell = (((((int64_t)i) << l) + j) << l) + k;
    const float* node = nodes + (level_offset(l) + cell) * kNodeFloats;
    bool descend = false;
    if (node_count(node) != 0) {
      float term;
      if (node_far(node, qx, qy, qz, beta2, term)) {
        sum += (double)term;
      } else if (l == levels) {
        int64_t a0 = cell_start[cell], a1 = cell_start[cell + 1];
        if (a0 < 0) a0 = 0;
        if (a1 > n_faces) a1 = n_faces;
        for (int64_t a = a0; a < a1; ++a) sum += (double)solid_angle(qx, qy, qz, tris + 9 * a);
      } else {
        descend = true;
      }
    }
    if (descend) {
      ++l; i <<= 1; j <<= 1; k <<= 1;                        // the first child
      continue;
    }
    while (l > 0 && (i & j & k & 1)) {                       // the last child: back to the parent
      --l; i >>= 1; j >>= 1; k >>= 1;
    }
    if (l == 0) break;
    const int c = (((i & 1) << 2) | ((j & 1) << 1) | (k & 1)) + 1;      // the next sibling
    i = (i & ~1) | (c >> 2);
    j = (j & ~1) | ((c >> 1) & 1);
    k = (k & ~1) | (c & 1);
  }
  w[q] = sum / kFourPi;
}

// The cube of a tree descriptor, or false with a message.
bool cube_of(const char* who, const recmv_winding_tree* t, Cube& c) {
  if (!t) {
    set_error("%s: NULL tree", who);
    return false;
  }
  if (t->levels < 1 || t->levels > kMaxLevels) {
    set_error("%s: levels=%d must be 1 .. %d", who, t->levels, kMaxLevels);
    return false;
  }
  if (!(t->side > 0.f) || !(t->side < __builtin_inff())) {
    set_error("%s: the cube's side %g must be positive and finite", who, (double)t->side);
    return false;
  }
  for (int a = 0; a < 3; ++a)
    if (!(t->origin[a] > -__builtin_inff() && t->origin[a] < __builtin_inff())) {
      set_error("%s: the cube's origin must be finite", who);
      return false;
    }
  c = Cube{t->origin[0], t->origin[1], t->origin[2], t->side, t->levels};
  return true;
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_winding_chunk_faces(void) { return kChunkFaces; }

extern "C" int64_t recmv_winding_exact_workspace_bytes(int64_t P, int64_t F) {
  if (P < 0 || F < 0) {
    set_error("winding_exact_workspace_bytes: P=%lld, F=%lld must not be negative", (long long)P, (long long)F);
    return -1;
  }
  const int64_t chunks = ceil_div(F, kChunkFaces);
  if (chunks > 65535 || P >= (1ll << 40)) {
    set_error("winding_exact_workspace_bytes: at most 65535 chunks of %lld faces and 2^40 points", (long long)kChunkFaces);
    return -1;
  }
  return chunks * P * (int64_t)sizeof(double);
}

extern "C" int recmv_winding_exact(const float* p, int64_t P, const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                   double* w, void* workspace, int64_t workspace_bytes, void* stream) {
  RECMV_REQUIRE(P >= 0 && V >= 0 && F >= 0, "winding_exact: P=%lld, V=%lld, F=%lld must not be negative", (long long)P,
                (long long)V, (long long)F);
  const int64_t need = recmv_winding_exact_workspace_bytes(P, F);
  if (need < 0) return RECMV_ERR_ARG;
  if (P == 0) return RECMV_OK;
  RECMV_REQUIRE(p && w, "winding_exact: NULL points or output");
  hipStream_t s = (hipStream_t)stream;
  if (F == 0) {
    RECMV_HIP_TRY(hipMemsetAsync(w, 0, (size_t)P * sizeof(double), s));
    return RECMV_OK;
  }
  RECMV_REQUIRE(faces && (verts || V == 0), "winding_exact: NULL pointer of the mesh");
  RECMV_REQUIRE(workspace, "winding_exact: NULL workspace");
  RECMV_REQUIRE(workspace_bytes >= need, "winding_exact: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)need);
  RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "winding_exact: workspace must be 8-byte aligned");
  const int64_t chunks = ceil_div(F, kChunkFaces), blocks = ceil_div(P, kWindBlock);
  RECMV_REQUIRE(blocks < (1ll << 31), "winding_exact: too many points for one call");
  double* partial = (double*)workspace;
  winding_exact_kernel<<<dim3((unsigned)blocks, (unsigned)chunks), kWindBlock, 0, s>>>(p, P, verts, V, faces, F, partial);
  int rc = check_launch("winding_exact");
  if (rc != RECMV_OK) return rc;
  winding_reduce_kernel<<<(unsigned)blocks, kWindBlock, 0, s>>>(partial, chunks, P, w);
  return check_launch("winding_reduce");
}

extern "C" int64_t recmv_winding_tree_nodes(int levels) {
  if (levels < 1 || levels > kMaxLevels) {
    set_error("winding_tree_nodes: levels=%d must be 1 .. %d", levels, kMaxLevels);
    return -1;
  }
  return ((1ll << (3 * (levels + 1))) - 1) / 7;
}

extern "C" int recmv_winding_tree_cells(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                        const recmv_winding_tree* tree, int64_t* cells, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "winding_tree_cells: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  Cube c;
  if (!cube_of("winding_tree_cells", tree, c)) return RECMV_ERR_ARG;
  if (F == 0) return RECMV_OK;
  RECMV_REQUIRE(faces && cells && (verts || V == 0), "winding_tree_cells: NULL pointer");
  winding_cells_kernel<<<stream_grid(F, kWindBlock), kWindBlock, 0, (hipStream_t)stream>>>(verts, V, faces, F, c, cells);
  return check_launch("winding_tree_cells");
}

extern "C" int recmv_winding_tree_build(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* order,
                                        const recmv_winding_tree* tree, void* stream) {
  RECMV_REQUIRE(V >= 0 && F >= 0, "winding_tree_build: V=%lld, F=%lld must not be negative", (long long)V, (long long)F);
  Cube c;
  if (!cube_of("winding_tree_build", tree, c)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(tree->n_faces >= 0 && tree->n_faces <= F, "winding_tree_build: n_faces=%lld must be 0 .. F=%lld",
                (long long)tree->n_faces, (long long)F);
  RECMV_REQUIRE(tree->nodes && tree->cell_start, "winding_tree_build: NULL table");
  RECMV_REQUIRE(tree->n_faces == 0 || (tree->tris && order && faces && verts), "winding_tree_build: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t cells = 1ll << (3 * c.levels);
  winding_leaves_kernel<<<(unsigned)ceil_div(cells, kWindBlock), kWindBlock, 0, s>>>(
      verts, V, faces, F, order, tree->n_faces, tree->cell_start, c.levels, tree->nodes, tree->tris);
  int rc = check_launch("winding_tree_leaves");
  for (int l = c.levels - 1; l >= 0 && rc == RECMV_OK; --l) {
    winding_parents_kernel<<<(unsigned)ceil_div(1ll << (3 * l), kWindBlock), kWindBlock, 0, s>>>(l, tree->nodes);
    rc = check_launch("winding_tree_parents");
  }
  return rc;
}

extern "C" int recmv_winding_tree_query(const float* p, int64_t P, const int64_t* order, const recmv_winding_tree* tree,
                                        float beta, double* w, void* stream) {
  RECMV_REQUIRE(P >= 0, "winding_tree_query: P=%lld must not be negative", (long long)P);
  RECMV_REQUIRE(beta >= 1.f && beta < __builtin_inff(), "winding_tree_query: beta=%g must be finite and at least 1", (double)beta);
  Cube c;
  if (!cube_of("winding_tree_query", tree, c)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(tree->n_faces >= 0, "winding_tree_query: n_faces=%lld must not be negative", (long long)tree->n_faces);
  RECMV_REQUIRE(tree->nodes && tree->cell_start && (tree->tris || tree->n_faces == 0), "winding_tree_query: NULL table");
  if (P == 0) return RECMV_OK;
  RECMV_REQUIRE(p && w, "winding_tree_query: NULL points or output");
  const int64_t blocks = ceil_div(P, kWindBlock);
  RECMV_REQUIRE(blocks < (1ll << 31), "winding_tree_query: too many points for one call");
  winding_tree_kernel<<<(unsigned)blocks, kWindBlock, 0, (hipStream_t)stream>>>(p, P, order, c.levels, tree->nodes,
                                                                              tree->cell_start, tree->tris, tree->n_faces,
                                                                              beta * beta, w);
  return check_launch("winding_tree_query");
}
