// Proper intersection of two triangles in f32, shared by the brute-force and the grid kernel of mesh_intersect.hip so that
// both give the same answer for the same pair.  Include it inside namespace recmv.  Every product, difference and fused
// multiply-add is written out (fmaf / __fmul_rn / __fsub_rn) in one fixed order: the compiler's contraction has no freedom,
// whatever -ffp-contract the file is built with, so the predicate's bits cannot differ between the kernels that inline it.
//
// Definition.  orient(a, b, c, d) is the determinant of the rows (b - a, c - a, d - a).  Edge pq pierces triangle abc iff
//   (1) orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs, and
//   (2) orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) have strictly the same sign.
// Two triangles cross iff one of the six edge-against-triangle tests holds.  Every inequality is strict, so touching (a
// shared vertex or edge, a vertex exactly in the other's plane), coplanar overlap and a triangle without area are no
// crossing, and neither is anything with a NaN.  Two guards in tri_tri_cross make the last two hold for every edge.
//
// Exact zeros.  A row of zeros (d, b or c bit-identical to a) gives 0 through the arithmetic itself.  Two identical rows
// do not: x (y w - z v) + y (z u - x w) + z (x v - y u) leaves rounding residue.  det3 therefore returns 0 when two of its
// rows are bit-identical, so that ANY repeated position among orient's four arguments gives an exact 0 and an unwelded mesh
// (every face with its own copies of its corners) reports nothing along its seams.
//
// f32 error.  Let L bound every coordinate difference among the points involved, u = 2^-24 = eps32 / 2, to first order in u:
//   * a row element is one rounded difference: relative error u, magnitude <= L;
//   * a cofactor m = fmaf(r1y, r2z, -fl(r1z r2y)): the rounded product errs by u L^2, the fused result by u |m| <= 2 u L^2,
//     and the two row elements in each of its products carry 2 u each: (|r1y r2z| + |r1z r2y|) 2 u <= 4 u L^2.  Together
//     7 u L^2 per cofactor, and |m| <= 2 L^2;
//   * the expansion fmaf(r0x, m0, fmaf(r0y, m1, fl(r0z m2))): three roundings of partial sums of at most 2, 4 and 6 L^3:
//     12 u L^3; the cofactors' errors times |r0| <= L: 21 u L^3; r0's own rounding on |r0 . m| <= 6 L^3: 6 u L^3.
//   |det_f32 - det| <= 39 u L^3 = 19.5 eps32 L^3; with the second-order terms below 20 eps32 L^3.
//   * two rows that round to the same bits differ by at most 2 u L per element before rounding, so the determinant that is
//     replaced by 0 was at most 6 L L (2 u L) = 12 u L^3: inside the same bound.
// A pair all of whose deciding determinants exceed 20 eps32 L^3 in magnitude is therefore decided as in exact arithmetic.
#pragma once

struct Pts {
  float ax, ay, az, bx, by, bz, cx, cy, cz;                // the three corners as they are stored (no differences)
};

// The face's corners (false when an index lies outside [0, V): load_tri's skip, such a face crosses nothing).
__device__ __forceinline__ bool load_pts(const float* __restrict__ v, const int64_t* __restrict__ f, int64_t V, int64_t k,
                                         Pts& t, int64_t& i0, int64_t& i1, int64_t& i2) {
  i0 = f[3 * k]; i1 = f[3 * k + 1]; i2 = f[3 * k + 2];
  if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) return false;
  t.ax = v[3 * i0]; t.ay = v[3 * i0 + 1]; t.az = v[3 * i0 + 2];
  t.bx = v[3 * i1]; t.by = v[3 * i1 + 1]; t.bz = v[3 * i1 + 2];
  t.cx = v[3 * i2]; t.cy = v[3 * i2 + 1]; t.cz = v[3 * i2 + 2];
  return true;
}

__device__ __forceinline__ float det3(float r0x, float r0y, float r0z, float r1x, float r1y, float r1z, float r2x, float r2y,
                                      float r2z) {
  const bool e01 = r0x == r1x && r0y == r1y && r0z == r1z;
  const bool e02 = r0x == r2x && r0y == r2y && r0z == r2z;
  const bool e12 = r1x == r2x && r1y == r2y && r1z == r2z;
  const float m0 = fmaf(r1y, r2z, -__fmul_rn(r1z, r2y));
  const float m1 = fmaf(r1z, r2x, -__fmul_rn(r1x, r2z));
  const float m2 = fmaf(r1x, r2y, -__fmul_rn(r1y, r2x));
  const float d = fmaf(r0x, m0, fmaf(r0y, m1, __fmul_rn(r0z, m2)));
  return (e01 || e02 || e12) ? 0.f : d;
}

// orient(a, b, c, d): rows of differences taken from the first argument
__device__ __forceinline__ float orient3(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                         float cz, float dx, float dy, float dz) {
  return det3(__fsub_rn(bx, ax), __fsub_rn(by, ay), __fsub_rn(bz, az), __fsub_rn(cx, ax), __fsub_rn(cy, ay),
              __fsub_rn(cz, az), __fsub_rn(dx, ax), __fsub_rn(dy, ay), __fsub_rn(dz, az));
}

// condition (2) for the edge pq against the triangle t
__device__ __forceinline__ bool edge_inside(float px, float py, float pz, float qx, float qy, float qz, const Pts& t) {
  const float s0 = orient3(px, py, pz, qx, qy, qz, t.ax, t.ay, t.az, t.bx, t.by, t.bz);
  const float s1 = orient3(px, py, pz, qx, qy, qz, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
  const float s2 = orient3(px, py, pz, qx, qy, qz, t.cx, t.cy, t.cz, t.ax, t.ay, t.az);
  return (s0 > 0.f && s1 > 0.f && s2 > 0.f) || (s0 < 0.f && s1 < 0.f && s2 < 0.f);
}

__device__ __forceinline__ bool opposite(float a, float b) { return (a > 0.f && b < 0.f) || (a < 0.f && b > 0.f); }

// the sides of t's plane the three corners of e lie on
__device__ __forceinline__ void plane_sides(const Pts& t, const Pts& e, float& da, float& db, float& dc) {
  da = orient3(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, e.ax, e.ay, e.az);
  db = orient3(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, e.bx, e.by, e.bz);
  dc = orient3(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, e.cx, e.cy, e.cz);
}

// one of the three edges of e pierces the triangle t, (da, db, dc) = plane_sides(t, e).  The determinants of condition (2)
// are only evaluated for an edge that passed (1): the value is that of the definition.
__device__ __forceinline__ bool edges_pierce(const Pts& t, const Pts& e, float da, float db, float dc) {
  bool hit = false;
  if (opposite(da, db)) hit = edge_inside(e.ax, e.ay, e.az, e.bx, e.by, e.bz, t);
  if (!hit && opposite(db, dc)) hit = edge_inside(e.bx, e.by, e.bz, e.cx, e.cy, e.cz, t);
  if (!hit && opposite(dc, da)) hit = edge_inside(e.cx, e.cy, e.cz, e.ax, e.ay, e.az, t);
  return hit;
}

// The predicate: symmetric under swapping the triangles (one function called both ways, OR-ed, behind two guards that are
// symmetric themselves).
//   * NaN: each triple of plane sides holds every corner of one triangle and all of the other's: a NaN anywhere in the pair
//     is in both triples, and the pair is no crossing whatever its remaining edges do.
//   * A plane none of the other triangle's corners leaves (three exact zeros): the triangles are coplanar, or the plane's
//     triangle has a repeated corner (every row pair of its determinants repeats) — a triangle without area.  No crossing,
//     also through the edges of the flat triangle, which the six tests alone would still let pierce the other.
__device__ __forceinline__ bool tri_tri_cross(const Pts& a, const Pts& b) {
  float a0, a1, a2, b0, b1, b2;
  plane_sides(b, a, a0, a1, a2);                           // a's corners against b's plane
  plane_sides(a, b, b0, b1, b2);
  if (!(a0 == a0 && a1 == a1 && a2 == a2 && b0 == b0 && b1 == b1 && b2 == b2)) return false;
  if ((a0 == 0.f && a1 == 0.f && a2 == 0.f) || (b0 == 0.f && b1 == 0.f && b2 == 0.f)) return false;
  return edges_pierce(b, a, a0, a1, a2) || edges_pierce(a, b, b0, b1, b2);
}

// The closed axis-aligned boxes of the two triangles meet (fminf / fmaxf pass over a NaN, as face_range does).  Triangles
// that cross have boxes that meet, so this is no part of the definition; both kernels apply it in front of the predicate because the grid can only bring
// together faces whose boxes share a cell, and the brute force must not answer differently for a pair the grid never sees.
__device__ __forceinline__ bool tri_boxes_meet(const Pts& a, const Pts& b) {
  return fminf(fminf(a.ax, a.bx), a.cx) <= fmaxf(fmaxf(b.ax, b.bx), b.cx) &&
         fminf(fminf(b.ax, b.bx), b.cx) <= fmaxf(fmaxf(a.ax, a.bx), a.cx) &&
         fminf(fminf(a.ay, a.by), a.cy) <= fmaxf(fmaxf(b.ay, b.by), b.cy) &&
         fminf(fminf(b.ay, b.by), b.cy) <= fmaxf(fmaxf(a.ay, a.by), a.cy) &&
         fminf(fminf(a.az, a.bz), a.cz) <= fmaxf(fmaxf(b.az, b.bz), b.cz) &&
         fminf(fminf(b.az, b.bz), b.cz) <= fmaxf(fmaxf(a.az, a.bz), a.cz);
}
