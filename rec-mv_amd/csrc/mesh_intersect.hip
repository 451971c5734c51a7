// Which faces of two triangle meshes cross — the second query on mesh_grid.hip's uniform grid, and its brute force — gfx950.
//
// What it computes (not in the reference, whose engineer/optimizer/surface_intesection.py stops at a breakpoint after a ray
// cast): the pairs (i, j) of a face i of mesh A and a face j of mesh B whose closed boxes meet and that cross properly in
// the sense of tri_tri.h (strict: touching, coplanar overlap, faces without area and anything with a NaN are no crossing; a
// face with an index outside its mesh crosses nothing).  self_mode: A is B, only i < j; skip_shared: a pair of faces that
// share a vertex INDEX is skipped.
//   * recmv_mesh_intersect_brute: every pair (i, j) — the judge of the grid query and the method for small meshes.
//   * recmv_mesh_intersect_grid_count / _fill: against a grid built over B (recmv_mesh_grid_count / _fill).  Face i of A
//     takes its cell range in B's grid from face_range() — the arithmetic B's faces were binned with, on A's corners, clamped
//     into the grid — and walks those cells' entries.  A pair whose boxes share several cells is tested in exactly one of
//     them: the cell whose index is, per axis, the larger of the two faces' lower cell indices (it lies in both ranges when
//     they overlap, and they do in the cell being walked).  No memory is needed for that.
//     Closed boxes that meet have cell ranges that meet (the cell of a coordinate is monotone in it), so the grid reaches
//     every pair the brute force accepts: both apply tri_boxes_meet and then the one predicate, the same bits.
//
// How: two passes, integer atomics only.  The count pass writes per-face counts and their total; the caller scans the
// counts; the fill pass finds the same pairs again and writes them at the face's offset through an integer cursor, every
// slot clamped against the face's end and the capacity (a pair that does not fit is counted in `dropped`, never written).
// The order of one face's pairs follows the cursor: unspecified.
//   * grid kernels: a group of G lanes (1, 8 or 64: `lanes`) per face of A strides over the cells of its range, so that a
//     face with a large range is spread over its group; the group's count meets in a shuffle sum.  Loops: the cells of a
//     range (at most the grid's cell count) and a cell's entries (clamped into [0, n_entries]).
//   * brute force: one workgroup per face of A strides over the faces of B; the count meets in LDS.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "grid_query.h"                                    // Grid, Range, face_range, range_cell; GridView, for_each_entry
#include "tri_tri.h"                                       // Pts, load_pts, tri_boxes_meet, tri_tri_cross
#include "mesh_device.h"                                   // group_sum

constexpr int kBlock = 256;

// what both kernels do with a pair whose face i (corners ta, indices a0..a2) is loaded: true when (i, j) is a result
__device__ __forceinline__ bool pair_crosses(const Pts& ta, int64_t a0, int64_t a1, int64_t a2, int64_t i,
                                             const float* __restrict__ vb, const int64_t* __restrict__ fb, int64_t VB,
                                             int64_t j, bool self_mode, bool skip_shared) {
  if (self_mode && j <= i) return false;
  Pts tb;
  int64_t b0, b1, b2;
  if (!load_pts(vb, fb, VB, j, tb, b0, b1, b2)) return false;
  if (skip_shared && (a0 == b0 || a0 == b1 || a0 == b2 || a1 == b0 || a1 == b1 || a1 == b2 || a2 == b0 || a2 == b1 ||
                      a2 == b2))
    return false;
  return tri_boxes_meet(ta, tb) && tri_tri_cross(ta, tb);
}

// a found pair: into its slot when `pairs` is given (fill pass), counted either way
struct Sink {
  const int32_t* offsets;                                  // [FA + 1], NULL in the count pass
  int32_t* cursor;                                         // [FA]
  int32_t* pairs;                                          // [capacity, 2]
  int64_t capacity;
  unsigned long long* dropped;
};

__device__ __forceinline__ void emit(const Sink& s, int64_t i, int64_t j) {
  if (!s.offsets) return;
  const int slot = atomicAdd(s.cursor + i, 1);
  // the face's own end (the count pass found the same pairs, so this holds) and the capacity the caller allocated
  if (slot >= 0 && slot < s.offsets[i + 1] && (int64_t)slot < s.capacity) {
    s.pairs[2 * (int64_t)slot] = (int32_t)i;
    s.pairs[2 * (int64_t)slot + 1] = (int32_t)j;
  } else {
    atomicAdd(s.dropped, 1ull);
  }
}

__global__ void __launch_bounds__(kBlock)
intersect_brute_kernel(const float* __restrict__ va, int64_t VA, const int64_t* __restrict__ fa, int64_t FA,
                       const float* __restrict__ vb, int64_t VB, const int64_t* __restrict__ fb, int64_t FB,
                       int self_mode, int skip_shared, int32_t* __restrict__ counts, unsigned long long* __restrict__ total,
                       Sink sink) {
  __shared__ int32_t s[kBlock];
  for (int64_t i = blockIdx.x; i < FA; i += gridDim.x) {   // (uniform over the workgroup)
    Pts ta;
    int64_t a0, a1, a2;
    int32_t mine = 0;
    if (load_pts(va, fa, VA, i, ta, a0, a1, a2)) {
      for (int64_t j = threadIdx.x; j < FB; j += kBlock) {
        if (pair_crosses(ta, a0, a1, a2, i, vb, fb, VB, j, self_mode != 0, skip_shared != 0)) {
          ++mine;
          emit(sink, i, j);
        }
      }
    }
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0 && counts) {
      counts[i] = s[0];
      if (s[0]) atomicAdd(total, (unsigned long long)s[0]);
    }
    __syncthreads();                                       // s is rewritten by the next face
  }
}

template <int G>
__global__ void __launch_bounds__(kBlock)
intersect_grid_kernel(const float* __restrict__ va, int64_t VA, const int64_t* __restrict__ fa, int64_t FA,
                      const float* __restrict__ vb, int64_t VB, const int64_t* __restrict__ fb, int64_t FB,
                      GridView view, int self_mode, int skip_shared, int32_t* __restrict__ counts,
                      unsigned long long* __restrict__ total, Sink sink) {
  const Grid& g = view.g;
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  const int sub = threadIdx.x % G;
  if (i >= FA) return;                                     // (a whole group at once: i is the same in its lanes)
  Pts ta;
  int64_t a0, a1, a2;
  Range r{0, 0, 0, 0, 0, 0};
  int32_t mine = 0;
  if (load_pts(va, fa, VA, i, ta, a0, a1, a2) && face_range(va, fa, VA, i, g, r)) {
    const int64_t n = range_cells(r);                      // at most the grid's cell count: the range is clamped into it
    for (int64_t c = sub; c < n; c += G) {
      int x, y, z;
      range_cell(r, c, x, y, z);
      for_each_entry(view, cell_id(g, x, y, z), FB, [&](int64_t j) {
        if (self_mode && j <= i) return;
        Range rj;
        if (!face_range(vb, fb, VB, j, g, rj)) return;
        // the one cell of the pair: per axis the larger of the two lower cell indices
        if (x != max(r.x0, rj.x0) || y != max(r.y0, rj.y0) || z != max(r.z0, rj.z0)) return;
        if (pair_crosses(ta, a0, a1, a2, i, vb, fb, VB, j, self_mode != 0, skip_shared != 0)) {
          ++mine;
          emit(sink, i, j);
        }
      });
    }
  }
  mine = group_sum<G>(mine);
  if (sub == 0 && counts) {
    counts[i] = mine;
    if (mine) atomicAdd(total, (unsigned long long)mine);
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

#include "mesh_grid_host.h"                                // grid_view_args, lanes_ok, with_lanes

namespace {

// the two meshes and the flags, checked before any HIP call (0: fine)
int mesh_args(const char* what, const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA, const float* b_verts,
              int64_t VB, const int64_t* b_faces, int64_t FB, int32_t self_mode, int32_t skip_shared) {
  RECMV_REQUIRE(VA >= 0 && FA >= 0 && VB >= 0 && FB >= 0, "%s: VA=%lld, FA=%lld, VB=%lld, FB=%lld must not be negative", what,
                (long long)VA, (long long)FA, (long long)VB, (long long)FB);
  RECMV_REQUIRE(FA < (1ll << 31) && FB < (1ll << 31), "%s: at most 2^31 - 1 faces", what);
  RECMV_REQUIRE((self_mode == 0 || self_mode == 1) && (skip_shared == 0 || skip_shared == 1),
                "%s: self_mode=%d and skip_shared=%d must be 0 or 1", what, (int)self_mode, (int)skip_shared);
  RECMV_REQUIRE(self_mode || !skip_shared, "%s: skip_shared needs self_mode (vertex indices of two meshes do not compare)",
                what);
  RECMV_REQUIRE(!self_mode || (a_verts == b_verts && a_faces == b_faces && VA == VB && FA == FB),
                "%s: self_mode needs the same mesh as A and B", what);
  RECMV_REQUIRE(FA == 0 || (a_faces && (VA == 0 || a_verts)), "%s: NULL pointer of mesh A", what);
  RECMV_REQUIRE(FB == 0 || (b_faces && (VB == 0 || b_verts)), "%s: NULL pointer of mesh B", what);
  return RECMV_OK;
}

// the fill pass's arguments (offsets NULL: a count pass, nothing else is looked at)
int sink_args(const char* what, const int32_t* offsets, int32_t* pairs, int64_t capacity, int32_t* cursor, int64_t* dropped,
              Sink& s) {
  s = Sink{nullptr, nullptr, nullptr, 0, nullptr};
  if (!offsets) return RECMV_OK;
  RECMV_REQUIRE(capacity >= 0 && capacity < (1ll << 30), "%s: capacity=%lld must be in [0, 2^30)", what, (long long)capacity);
  RECMV_REQUIRE(cursor && dropped && (capacity == 0 || pairs), "%s: NULL pointer of the fill pass", what);
  RECMV_REQUIRE(((uintptr_t)dropped & 7) == 0, "%s: dropped must be 8-byte aligned", what);
  s = Sink{offsets, cursor, pairs, capacity, (unsigned long long*)dropped};
  return RECMV_OK;
}

// zero the outputs of a pass and set the cursor to the offsets
int prepare(const Sink& s, int64_t FA, int32_t* counts, int64_t* total, hipStream_t st) {
  if (total) {
    if (FA) RECMV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)FA * sizeof(int32_t), st));
    RECMV_HIP_TRY(hipMemsetAsync(total, 0, sizeof(int64_t), st));
  }
  if (s.offsets) {
    RECMV_HIP_TRY(hipMemsetAsync(s.dropped, 0, sizeof(int64_t), st));
    if (FA) RECMV_HIP_TRY(hipMemcpyAsync(s.cursor, s.offsets, (size_t)FA * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  }
  return RECMV_OK;
}

int grid_pass(const char* what, const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA, const float* b_verts,
              int64_t VB, const int64_t* b_faces, int64_t FB, const recmv_mesh_grid* grid, int32_t lanes, int32_t self_mode,
              int32_t skip_shared, int32_t* counts, int64_t* total, const int32_t* offsets, int32_t* pairs, int64_t capacity,
              int32_t* cursor, int64_t* dropped, void* stream) {
  int rc = mesh_args(what, a_verts, VA, a_faces, FA, b_verts, VB, b_faces, FB, self_mode, skip_shared);
  if (rc != RECMV_OK) return rc;
  rc = lanes_ok(what, lanes);
  if (rc != RECMV_OK) return rc;
  GridView view;
  rc = grid_view_args(what, grid, FA && FB ? kGridTables : kGridGeometry, view);
  if (rc != RECMV_OK) return rc;
  Sink s;
  rc = sink_args(what, offsets, pairs, capacity, cursor, dropped, s);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(s.offsets || (total && (counts || FA == 0)), "%s: NULL output pointer", what);
  RECMV_REQUIRE(!s.offsets || (!counts && !total), "%s: the fill pass writes no counts", what);
  RECMV_REQUIRE(!total || ((uintptr_t)total & 7) == 0, "%s: total must be 8-byte aligned", what);
  const int64_t nb = ceil_div(FA * lanes, kBlock);
  RECMV_REQUIRE(nb < (1ll << 31), "%s: too many faces", what);
  hipStream_t st = (hipStream_t)stream;
  rc = prepare(s, FA, counts, total, st);
  if (rc != RECMV_OK || FA == 0 || FB == 0) return rc;     // an empty mesh crosses nothing
  with_lanes(lanes, [&](auto G) {
    intersect_grid_kernel<decltype(G)::value><<<(unsigned)nb, kBlock, 0, st>>>(
        a_verts, VA, a_faces, FA, b_verts, VB, b_faces, FB, view, self_mode, skip_shared, counts, (unsigned long long*)total, s);
  });
  return check_launch(what);
}

}  // namespace

extern "C" int recmv_mesh_intersect_brute(const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA,
                                          const float* b_verts, int64_t VB, const int64_t* b_faces, int64_t FB,
                                          int32_t self_mode, int32_t skip_shared, int32_t* counts, int64_t* total,
                                          const int32_t* offsets, int32_t* pairs, int64_t capacity, int32_t* cursor,
                                          int64_t* dropped, void* stream) {
  const char* what = "mesh_intersect_brute";
  int rc = mesh_args(what, a_verts, VA, a_faces, FA, b_verts, VB, b_faces, FB, self_mode, skip_shared);
  if (rc != RECMV_OK) return rc;
  Sink s;
  rc = sink_args(what, offsets, pairs, capacity, cursor, dropped, s);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(s.offsets || (total && (counts || FA == 0)), "%s: NULL output pointer", what);
  RECMV_REQUIRE(!s.offsets || (!counts && !total), "%s: the fill pass writes no counts", what);
  RECMV_REQUIRE(!total || ((uintptr_t)total & 7) == 0, "%s: total must be 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  rc = prepare(s, FA, counts, total, st);
  if (rc != RECMV_OK || FA == 0 || FB == 0) return rc;
  const int64_t nb = FA < (int64_t)kNumCU * 8 ? FA : (int64_t)kNumCU * 8;
  intersect_brute_kernel<<<(unsigned)nb, kBlock, 0, st>>>(a_verts, VA, a_faces, FA, b_verts, VB, b_faces, FB, self_mode,
                                                          skip_shared, counts, (unsigned long long*)total, s);
  return check_launch(what);
}

extern "C" int recmv_mesh_intersect_grid_count(const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA,
                                               const float* b_verts, int64_t VB, const int64_t* b_faces, int64_t FB,
                                               const recmv_mesh_grid* grid, int32_t lanes, int32_t self_mode,
                                               int32_t skip_shared, int32_t* counts, int64_t* total, void* stream) {
  RECMV_REQUIRE(total && (counts || FA == 0), "mesh_intersect_grid_count: NULL output pointer");
  return grid_pass("mesh_intersect_grid_count", a_verts, VA, a_faces, FA, b_verts, VB, b_faces, FB, grid, lanes, self_mode,
                   skip_shared, counts, total, nullptr, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int recmv_mesh_intersect_grid_fill(const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA,
                                              const float* b_verts, int64_t VB, const int64_t* b_faces, int64_t FB,
                                              const recmv_mesh_grid* grid, int32_t lanes, int32_t self_mode,
                                              int32_t skip_shared, const int32_t* offsets, int32_t* pairs, int64_t capacity,
                                              int32_t* cursor, int64_t* dropped, void* stream) {
  RECMV_REQUIRE(offsets, "mesh_intersect_grid_fill: NULL offsets");
  return grid_pass("mesh_intersect_grid_fill", a_verts, VA, a_faces, FA, b_verts, VB, b_faces, FB, grid, lanes, self_mode,
                   skip_shared, nullptr, nullptr, offsets, pairs, capacity, cursor, dropped, stream);
}
