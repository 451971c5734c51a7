// Segments against a triangle mesh: first hit and number of faces hit — the third query on mesh_grid.hip's uniform grid, and
// its brute force — gfx950.
//
// What it computes (the reference's engineer/optimizer/surface_intesection.py casts rays with pyembree and stops at a
// breakpoint): for every segment p -> q the faces it HITS in the sense of seg_tri.h (strict: touching, a segment in a face's
// plane, faces without area, a segment without length and anything not finite are no hit; a face with an index outside its
// mesh is hit by nothing), behind seg_tri.h's box gate.  Outputs per segment: face (the hit with the smallest parameter t,
// ties to the lowest face id; -1: none), t (NaN: none), count (the number of faces hit).
//   * recmv_segment_mesh_brute: every face — the judge of the grid query and the method for small inputs.
//   * recmv_segment_mesh_grid: through a grid built over the mesh (recmv_mesh_grid_count / _fill).  The same bits: both run
//     seg_face_hit on the same corners, the minimum over (t, face id) does not depend on the order the faces are met in, and
//     every face is evaluated exactly once (below).  want_count = 0: the walk may stop early and `count` is not written.
//
// The walk.  u = cell_coord(x) are cell units, the ONE expression of the binning; up, uq the endpoints.  The major axis M is
// the one with the largest |uq - up|; the walk visits the slabs k (cells whose M index is k) from the endpoint p's side to
// q's, ci(min(up_M, uq_M) - E) .. ci(max(up_M, uq_M) + E) with ci = cell_index (clamped into the grid: at most n_M slabs).
// In slab k the major coordinate is clipped to [A, B] = [k - E, k + 1 + E] ∩ [min, max] (open outwards in the grid's first
// and last slab, where the binning clamps), a minor coordinate is F(m) = up + (m - up_M) s, s = (uq - up) / (uq_M - up_M)
// (|s| <= 1; 0 for a segment that is a point in cell units: no division by 0, and a minor direction component of 0 gives
// s = 0), and the slab's cells are ci(min(F(A), F(B)) - E) .. ci(max(F(A), F(B)) + E) in both minor axes: at most the
// grid's cells.  F is monotone in m whatever the rounding does (every rounding is monotone), so it need only be evaluated
// at A and B.
//
// The margin E, W the largest |u| of the endpoints, S the largest |coordinate| of p and q, to first order in eps32:
//   * a pair that seg_tri.h accepts has the point X = p + t (q - p) of its reported t, a point of the exact segment, within
//     47 eps32 S of the face's box clipped to the segment's box (seg_tri.h: the gate alone gives some such point within
//     28 eps32 S, seg_clamp_t this one); X clamped into that box is a point Xc of the FACE's box, so ci(u(Xc)) lies in the
//     face's cell range in every axis (the cell of a coordinate is monotone in it), and |u(X) - u(Xc)| <= 47 eps32 S / h;
//   * u computed in f32 is within 2 eps32 W of the exact (x - o) / h (one difference, one product, inv_h itself rounded);
//   * F(m) against the exact minor coordinate of X: up's own 2 eps32 W, (m - up_M) 4 eps32 W, the slope's error
//     9 eps32 W / |uq_M - up_M| times |m - up_M| <= |uq_M - up_M|, three roundings of F, 3 eps32 W: 18 eps32 W;
//   * k -+ E and F -+ E are rounded themselves: eps32 W (k <= W + 1 inside the walk).
//   So with E >= (21 W + 47 S / h) eps32 the slab that holds clamp(u_M(X)) into the face's major range has A <= u_M(X) <= B
//   and minor extents that meet the face's [u(lo), u(hi)] in both minor axes: a visited cell of the face's range.
//   E = 64 eps32 (W + S / h + 1), above that with room to spare.  Where E is not below 1/4 (|u| beyond 2^15, or not finite)
//   the walk is `coarse`: every slab takes the cell range of the segment's box in the minor axes — boxes that meet have cell ranges that
//   meet, mesh_intersect.hip's argument — still at most the grid's cells.
//   A segment that starts, ends or lies outside the grid is clamped by ci like the faces that were binned there; a segment
//   in a cell-boundary plane is within E of both neighbouring cells and visits both.
//
// Once per face, without memory.  A face binned in several visited cells is evaluated in one: in the first slab of the walk
// whose cell rectangle meets the face's range — the slabs from the later of the face's first slab (in walk order) and the
// walk's first one up to the current one are tested again, the same function on the same values — and there in the cell
// whose index is, per minor axis, the larger of the two lower indices (it lies in both ranges).  So `count` needs no
// atomics and the minimum evaluates no face twice.
//
// Early stop (want_count = 0).  Let the best hit so far have the parameter t*, and let a face not yet evaluated be accepted
// with t <= t*.  By the first item above, with X the point of THAT t — seg_clamp_t keeps the reported t at the face even
// where sp and sq are rounding noise, a face nearly coplanar with the segment — the face is evaluated no later than the slab
// that holds u_M(X) + E, and u_M(X) = up_M + t (uq_M - up_M) does not lie behind u_M(t*) in walk order.  So the walk stops
// in front of the first slab that lies wholly behind u_M(t*) + E, as computed (2 eps32 W more, inside E's room), and one
// further slab is granted besides: no face met from there on can report a t <= t*, in f32 and not merely in exact
// arithmetic, and the first hit is the brute force's.  The group's best is made uniform by a shuffle minimum after every
// slab, so the stop is the same in its lanes.
//
// How: a group of G lanes (1, 8 or 64: `lanes`) per segment strides over a slab's cells and meets in a shuffle minimum on
// (t, face id) and a shuffle sum of the count.  The brute force: one workgroup per segment strides over the faces, the
// waves meet through LDS.  No float atomics, no atomics at all.  Loops: slabs <= n_M, cells of a slab <= the grid's, a
// cell's entries clamped into [0, n_entries], the slabs tested again <= the slabs walked.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "grid_query.h"                                    // Grid, Range, cell_coord, cell_index, face_range; GridView, for_each_entry
#include "tri_tri.h"                                       // Pts, load_pts, orient3, opposite, edge_inside
#include "seg_tri.h"                                       // Seg, seg_make, seg_face_hit, seg_take_min

constexpr int kBlock = 256;
constexpr float kWalkMargin = 64.f;                        // E = kWalkMargin eps32 (W + S / h + 1)

__device__ __forceinline__ float pick(int axis, float x, float y, float z) { return axis == 0 ? x : (axis == 1 ? y : z); }
__device__ __forceinline__ int pick(int axis, int x, int y, int z) { return axis == 0 ? x : (axis == 1 ? y : z); }

struct Walk {
  int M, A, B;                                             // the major and the two minor axes (0: x, 1: y, 2: z)
  int nM, nA, nB;                                          // the grid's cells along them
  float pM, pA, pB;                                        // p in cell units
  float dM;                                                // uq_M - up_M
  float loM, hiM;                                          // min / max of the major coordinate
  float sA, sB;                                            // minor per major
  float E;
  bool coarse;
  int ca0, ca1, cb0, cb1;                                  // coarse: the cells of the segment's box in the minor axes
  int kstart, dir, slabs;                                  // first slab, +-1, number of slabs
};

__device__ __forceinline__ Walk walk_make(const Seg& s, const Grid& g) {
  Walk w;
  const float upx = cell_coord(s.px, g.ox, g.inv_h), upy = cell_coord(s.py, g.oy, g.inv_h), upz = cell_coord(s.pz, g.oz, g.inv_h);
  const float uqx = cell_coord(s.qx, g.ox, g.inv_h), uqy = cell_coord(s.qy, g.oy, g.inv_h), uqz = cell_coord(s.qz, g.oz, g.inv_h);
  const float dx = uqx - upx, dy = uqy - upy, dz = uqz - upz;
  const float adx = fabsf(dx), ady = fabsf(dy), adz = fabsf(dz);
  w.M = (adx >= ady && adx >= adz) ? 0 : (ady >= adz ? 1 : 2);
  w.A = w.M == 0 ? 1 : 0;
  w.B = w.M == 2 ? 1 : 2;
  w.nM = pick(w.M, g.nx, g.ny, g.nz); w.nA = pick(w.A, g.nx, g.ny, g.nz); w.nB = pick(w.B, g.nx, g.ny, g.nz);
  w.pM = pick(w.M, upx, upy, upz); w.pA = pick(w.A, upx, upy, upz); w.pB = pick(w.B, upx, upy, upz);
  const float qM = pick(w.M, uqx, uqy, uqz), qA = pick(w.A, uqx, uqy, uqz), qB = pick(w.B, uqx, uqy, uqz);
  w.dM = pick(w.M, dx, dy, dz);
  w.loM = fminf(w.pM, qM); w.hiM = fmaxf(w.pM, qM);
  const bool point = !(w.dM != 0.f);                       // (also a NaN: coarse below)
  w.sA = point ? 0.f : pick(w.A, dx, dy, dz) / w.dM;
  w.sB = point ? 0.f : pick(w.B, dx, dy, dz) / w.dM;
  const float W = fmaxf(fmaxf(fmaxf(fabsf(upx), fabsf(upy)), fabsf(upz)), fmaxf(fmaxf(fabsf(uqx), fabsf(uqy)), fabsf(uqz)));
  w.E = kWalkMargin * kSegEps32 * (W + s.s * g.inv_h + 1.f);
  w.coarse = !(w.E < 0.25f) || !(fabsf(w.sA) <= 2.f) || !(fabsf(w.sB) <= 2.f);
  if (w.coarse) w.E = 0.f;
  w.ca0 = cell_index(fminf(w.pA, qA), w.nA); w.ca1 = cell_index(fmaxf(w.pA, qA), w.nA);
  w.cb0 = cell_index(fminf(w.pB, qB), w.nB); w.cb1 = cell_index(fmaxf(w.pB, qB), w.nB);
  if (w.ca1 < w.ca0) w.ca1 = w.ca0;
  if (w.cb1 < w.cb0) w.cb1 = w.cb0;
  const int klo = cell_index(w.loM - w.E, w.nM);
  int khi = cell_index(w.hiM + w.E, w.nM);
  if (khi < klo) khi = klo;
  w.dir = qM >= w.pM ? 1 : -1;
  w.kstart = w.dir > 0 ? klo : khi;
  w.slabs = khi - klo + 1;                                 // at most n_M: both are clamped into [0, n_M)
  return w;
}

// the cells [a0, a1] x [b0, b1] of slab k in the minor axes, clamped into the grid
__device__ __forceinline__ void slab_rect(const Walk& w, int k, int& a0, int& a1, int& b0, int& b1) {
  if (w.coarse) { a0 = w.ca0; a1 = w.ca1; b0 = w.cb0; b1 = w.cb1; return; }
  const float inf = __builtin_inff();
  const float lo = k <= 0 ? -inf : (float)k - w.E, hi = k >= w.nM - 1 ? inf : (float)(k + 1) + w.E;
  const float mA = fminf(fmaxf(lo, w.loM), w.hiM) - w.pM, mB = fmaxf(fminf(hi, w.hiM), w.loM) - w.pM;
  const float xa = w.pA + mA * w.sA, xb = w.pA + mB * w.sA;
  const float ya = w.pB + mA * w.sB, yb = w.pB + mB * w.sB;
  a0 = cell_index(fminf(xa, xb) - w.E, w.nA); a1 = cell_index(fmaxf(xa, xb) + w.E, w.nA);
  b0 = cell_index(fminf(ya, yb) - w.E, w.nB); b1 = cell_index(fmaxf(ya, yb) + w.E, w.nB);
  if (a1 < a0) a1 = a0;
  if (b1 < b0) b1 = b0;
}

// (k, a, b) is the one cell face j is evaluated in; (a0, a1, b0, b1) = slab_rect(k), r the face's range
__device__ __forceinline__ bool first_meeting(const Walk& w, int k, int a, int b, int a0, int b0, const Range& r) {
  const int fm0 = pick(w.M, r.x0, r.y0, r.z0), fm1 = pick(w.M, r.x1, r.y1, r.z1);
  const int fa0 = pick(w.A, r.x0, r.y0, r.z0), fa1 = pick(w.A, r.x1, r.y1, r.z1);
  const int fb0 = pick(w.B, r.x0, r.y0, r.z0), fb1 = pick(w.B, r.x1, r.y1, r.z1);
  if (a != max(a0, fa0) || b != max(b0, fb0)) return false;
  int kk = w.dir > 0 ? max(fm0, w.kstart) : min(fm1, w.kstart);
  const int steps = w.dir > 0 ? k - kk : kk - k;           // at most the slabs walked so far
  for (int n = 0; n < steps; ++n, kk += w.dir) {
    int p0, p1, q0, q1;
    slab_rect(w, kk, p0, p1, q0, q1);
    if (p0 <= fa1 && fa0 <= p1 && q0 <= fb1 && fb0 <= q1) return false;          // met in an earlier slab
  }
  return true;
}

// slab k lies wholly behind the best hit (walk order), with the margin of the file header
__device__ __forceinline__ bool slab_behind(const Walk& w, int k, float best) {
  const float uh = w.pM + best * w.dM;
  return w.dir > 0 ? (float)k > uh + w.E + 1.f : (float)(k + 1) < uh - w.E - 1.f;
}

template <int G>
__global__ void __launch_bounds__(kBlock)
segment_grid_kernel(const float* __restrict__ p, const float* __restrict__ q, int64_t S, const float* __restrict__ verts,
                    int64_t V, const int64_t* __restrict__ faces, int64_t F, GridView view, int want_count,
                    int64_t* __restrict__ face_out, float* __restrict__ t_out, int32_t* __restrict__ count_out) {
  const Grid& g = view.g;
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  const int sub = threadIdx.x % G;
  if (i >= S) return;                                      // (a whole group at once: i is the same in its lanes)
  const Seg s = seg_make(p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
  float best = __builtin_inff();
  int bidx = -1;
  int32_t mine = 0;
  if (s.ok) {
    const Walk w = walk_make(s, g);
    for (int n = 0; n < w.slabs; ++n) {
      const int k = w.kstart + w.dir * n;
      if (!want_count && !w.coarse && bidx >= 0 && slab_behind(w, k, best)) break;     // (uniform over the group)
      int a0, a1, b0, b1;
      slab_rect(w, k, a0, a1, b0, b1);
      const int wa = a1 - a0 + 1;
      const int64_t cells = (int64_t)wa * (b1 - b0 + 1);   // at most the grid's: the rectangle is clamped into it
      for (int64_t c = sub; c < cells; c += G) {
        const int a = a0 + (int)(c % wa), b = b0 + (int)(c / wa);
        const int x = w.M == 0 ? k : a, z = w.M == 2 ? k : b, y = w.M == 0 ? a : (w.M == 1 ? k : b);
        for_each_entry(view, cell_id(g, x, y, z), F, [&](int64_t j) {
          Range r;
          if (!face_range(verts, faces, V, j, g, r)) return;
          if (!first_meeting(w, k, a, b, a0, b0, r)) return;
          float tt;
          if (seg_face_hit(s, verts, faces, V, j, tt)) {
            ++mine;
            seg_take_min(tt, (int)j, best, bidx);
          }
        });
      }
      if (!want_count) {
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {        // the group's best, in every lane of it
          const float ob = __shfl_xor(best, off, G);
          const int oi = __shfl_xor(bidx, off, G);
          if (oi >= 0) seg_take_min(ob, oi, best, bidx);
        }
      }
    }
  }
  // (the minimum skips an empty lane's index -1, so it is not mesh_device.h's take_min; the count's group_sum stays in its loop)
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, G);
    const int oi = __shfl_xor(bidx, off, G);
    if (oi >= 0) seg_take_min(ob, oi, best, bidx);
    mine += __shfl_xor(mine, off, G);
  }
  if (sub != 0) return;
  face_out[i] = bidx;
  t_out[i] = bidx >= 0 ? best : __builtin_nanf("");
  if (want_count) count_out[i] = mine;
}

__global__ void __launch_bounds__(kBlock)
segment_brute_kernel(const float* __restrict__ p, const float* __restrict__ q, int64_t S, const float* __restrict__ verts,
                     int64_t V, const int64_t* __restrict__ faces, int64_t F, int64_t* __restrict__ face_out,
                     float* __restrict__ t_out, int32_t* __restrict__ count_out) {
  constexpr int kWaves = kBlock / kWave;
  __shared__ float sb[kWaves];
  __shared__ int si[kWaves];
  __shared__ int32_t sc[kWaves];
  for (int64_t i = blockIdx.x; i < S; i += gridDim.x) {    // (uniform over the workgroup)
    const Seg s = seg_make(p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
    float best = __builtin_inff();
    int bidx = -1;
    int32_t mine = 0;
    if (s.ok) {
      for (int64_t j = threadIdx.x; j < F; j += kBlock) {
        float tt;
        if (seg_face_hit(s, verts, faces, V, j, tt)) {
          ++mine;
          seg_take_min(tt, (int)j, best, bidx);
        }
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, kWave);
      const int oi = __shfl_xor(bidx, off, kWave);
      if (oi >= 0) seg_take_min(ob, oi, best, bidx);
      mine += __shfl_xor(mine, off, kWave);
    }
    if (threadIdx.x % kWave == 0) {
      sb[threadIdx.x / kWave] = best; si[threadIdx.x / kWave] = bidx; sc[threadIdx.x / kWave] = mine;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < kWaves; ++k) {
        if (si[k] >= 0) seg_take_min(sb[k], si[k], best, bidx);
        mine += sc[k];
      }
      face_out[i] = bidx;
      t_out[i] = bidx >= 0 ? best : __builtin_nanf("");
      if (count_out) count_out[i] = mine;
    }
    __syncthreads();                                       // the LDS words are rewritten by the next segment
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

#include "mesh_grid_host.h"                                // grid_view_args, lanes_ok, with_lanes

namespace {

// the segments, the mesh and the outputs, checked before any HIP call (0: fine)
int common_args(const char* what, const float* p, const float* q, int64_t S, const float* verts, int64_t V,
                const int64_t* faces, int64_t F, int64_t* face, float* t) {
  RECMV_REQUIRE(S >= 0 && V >= 0 && F >= 0, "%s: S=%lld, V=%lld, F=%lld must not be negative", what, (long long)S,
                (long long)V, (long long)F);
  RECMV_REQUIRE(F < (1ll << 31), "%s: at most 2^31 - 1 faces", what);
  RECMV_REQUIRE(S == 0 || (p && q), "%s: NULL segment pointer", what);
  RECMV_REQUIRE(S == 0 || (face && t), "%s: NULL output pointer", what);
  RECMV_REQUIRE(F == 0 || (faces && (V == 0 || verts)), "%s: NULL pointer of the mesh", what);
  return RECMV_OK;
}

int launch_brute(const char* what, const float* p, const float* q, int64_t S, const float* verts, int64_t V,
                 const int64_t* faces, int64_t F, int64_t* face, float* t, int32_t* count, hipStream_t st) {
  const int64_t nb = S < (int64_t)kNumCU * 8 ? S : (int64_t)kNumCU * 8;
  segment_brute_kernel<<<(unsigned)nb, kBlock, 0, st>>>(p, q, S, verts, V, faces, F, face, t, count);
  return check_launch(what);
}

}  // namespace

extern "C" int recmv_segment_mesh_brute(const float* p, const float* q, int64_t S, const float* verts, int64_t V,
                                        const int64_t* faces, int64_t F, int64_t* face, float* t, int32_t* count,
                                        void* stream) {
  const char* what = "segment_mesh_brute";
  int rc = common_args(what, p, q, S, verts, V, faces, F, face, t);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(S == 0 || count, "%s: NULL count", what);
  if (S == 0) return RECMV_OK;
  return launch_brute(what, p, q, S, verts, V, faces, F, face, t, count, (hipStream_t)stream);
}

extern "C" int recmv_segment_mesh_grid(const float* p, const float* q, int64_t S, const float* verts, int64_t V,
                                       const int64_t* faces, int64_t F, const recmv_mesh_grid* grid, int32_t lanes,
                                       int32_t want_count, int64_t* face, float* t, int32_t* count, void* stream) {
  const char* what = "segment_mesh_grid";
  int rc = common_args(what, p, q, S, verts, V, faces, F, face, t);
  if (rc != RECMV_OK) return rc;
  RECMV_REQUIRE(want_count == 0 || want_count == 1, "%s: want_count=%d must be 0 or 1", what, (int)want_count);
  RECMV_REQUIRE(!want_count || S == 0 || count, "%s: want_count=1 needs count (NULL)", what);
  rc = lanes_ok(what, lanes);
  if (rc != RECMV_OK) return rc;
  GridView view;
  rc = grid_view_args(what, grid, S && F ? kGridTables : kGridGeometry, view);
  if (rc != RECMV_OK) return rc;
  const int64_t nb = ceil_div(S * lanes, kBlock);
  RECMV_REQUIRE(nb < (1ll << 31), "%s: too many segments", what);
  if (S == 0) return RECMV_OK;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) return launch_brute(what, p, q, S, verts, V, faces, F, face, t, want_count ? count : nullptr, st);   // hits nothing
  with_lanes(lanes, [&](auto G) {
    segment_grid_kernel<decltype(G)::value><<<(unsigned)nb, kBlock, 0, st>>>(p, q, S, verts, V, faces, F, view, want_count, face,
                                                                            t, count);
  });
  return check_launch(what);
}
