// A segment against a triangle in f32, shared by the brute-force and the grid kernel of segment_mesh.hip so that both give
// the same answer and the same hit parameter for the same pair.  Include it inside namespace recmv, after tri_tri.h and under
// `#pragma clang fp contract(off)`; every product, sum and difference that decides something is written out besides.
//
// Definition.  The segment pq HITS the triangle abc iff tri_tri.h's edge-against-triangle test holds (its functions, not a
// restatement):
//   (1) opposite(orient3(a,b,c,p), orient3(a,b,c,q)): the endpoints lie strictly on opposite sides of the plane, and
//   (2) edge_inside(p, q, abc): orient3(p,q,a,b), orient3(p,q,b,c), orient3(p,q,c,a) have strictly the same sign.
// Every inequality is strict, so none of these is a hit: touching (an endpoint exactly in the plane, a segment through a
// vertex or along an edge), a segment in the triangle's plane, a triangle with a repeated corner, a segment whose endpoints
// are the same bits (orient3 returns an exact 0 for a repeated position), anything with a NaN or an infinity.
// The hit parameter is t = sp / (sp - sq), sp = orient3(a,b,c,p), sq = orient3(a,b,c,q), one rounded difference and one
// rounded quotient, kept at the face by seg_clamp_t (below); in exact arithmetic it lies strictly inside (0, 1) by (1).  The corners are read through the face table
// (load_pts): the exact zeros need every corner's own bits.
//
// The box gate.  In exact arithmetic a hit point lies on the segment and in the triangle, hence in the closed box of the
// endpoints and in the closed box of the corners.  Both kernels therefore put seg_box_gate in front of the predicate, as
// mesh_intersect.hip puts tri_boxes_meet: the grid can only bring a segment together with faces binned near it, and the brute
// force must not answer differently for a pair whose f32 determinants are noise (a segment far shorter than its distance to a
// large face).  The gate: the face's box clipped to the segment's box is not empty (exact comparisons), and the segment
// passes the separating-axis test against that clipped box on the three axes d x e_i (the three box axes hold by the
// clipping), with the box inflated by delta = 16 eps32 S, S the largest |coordinate| of p and q.
//   f32 error of the gate, to first order in eps32, every value at most 2 S after the clipping: twice the box centre relative
//   to the segment's midpoint, C = (lo + hi) - (2 p + d), errs by 4.5 eps32 S; the two products of an axis and their
//   difference by 16 eps32 S (|d_i| + |d_j|) together; the right-hand side E_i |d_j| + E_j |d_i| by 6 eps32 S (|d_i| + |d_j|);
//   d = fl(q - p) stands for q - p at the price of moving q by eps32 S.  The test compares with the margin
//   2 delta (|d_i| + |d_j|) = 32 eps32 S (|d_i| + |d_j|), which is the exact test of the box inflated by delta.  So
//     * a pair that hits in exact arithmetic passes the gate (22 + 2 < 32), and
//     * a pair that passes it has a point of the exact segment within 28 eps32 S of the clipped box in every axis
//       ((32 + 22) / 2 + 1): what segment_mesh.hip's walk is built to reach.
//
// The parameter stays at the face.  In exact arithmetic the hit point lies in the clipped box, so the exact t lies in
// [t0, t1], the parameters at which the segment is within kappa = 40 eps32 S of the clipped box in every axis with a
// direction component other than 0.  A face nearly coplanar with the segment has sp and sq that are rounding noise, and
// sp / (sp - sq) can then land anywhere in (0, 1), far from the face: seg_clamp_t puts the quotient back into [t0, t1]
// (and calls the pair no hit where that interval is empty, which no exact hit's is).  Both kernels run it, so it cannot
// make them differ; it is what lets the grid's first-hit walk stop at the best hit, because the point p + t (q - p) of
// every reported t is now near the face's box and not merely some point of the segment.
//   f32 error of a bound (lo - kappa - p_i) / d_i as a position on axis i, every value at most 2 S: the two differences
//   3 eps32 S, the quotient and d_i = fl(q_i - p_i) 2 eps32 S each: 7 eps32 S.  So
//     * [t0, t1] as computed holds every t whose point is within (40 - 7) eps32 S of the clipped box: the gate's point
//       (28) and the exact t of an exact hit, so the interval is not empty for a pair that passed the gate, the clamp never
//       moves t away from the exact t, and csrc/tri_tri.h's bound on |t - t_exact| holds for the clamped t as well;
//     * the point of every reported t is within (40 + 7) eps32 S of the clipped box in every axis.
#pragma once

constexpr float kSegEps32 = 1.1920929e-7f;                 // 2^-23

struct Seg {
  float px, py, pz, qx, qy, qz;                            // the endpoints as they are stored
  float dx, dy, dz;                                        // fl(q - p)
  float lox, loy, loz, hix, hiy, hiz;                      // the closed box of the endpoints
  float s;                                                 // the largest |coordinate| of p and q
  float m;                                                 // 2 delta = 32 eps32 s
  float kappa;                                             // 40 eps32 s
  bool ok;                                                 // every coordinate finite (else the segment hits nothing)
};

__device__ __forceinline__ Seg seg_make(float px, float py, float pz, float qx, float qy, float qz) {
  Seg g;
  g.px = px; g.py = py; g.pz = pz; g.qx = qx; g.qy = qy; g.qz = qz;
  g.dx = __fsub_rn(qx, px); g.dy = __fsub_rn(qy, py); g.dz = __fsub_rn(qz, pz);
  g.lox = fminf(px, qx); g.hix = fmaxf(px, qx);
  g.loy = fminf(py, qy); g.hiy = fmaxf(py, qy);
  g.loz = fminf(pz, qz); g.hiz = fmaxf(pz, qz);
  g.s = fmaxf(fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)), fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)));
  g.m = __fmul_rn(32.f * kSegEps32, g.s);
  g.kappa = __fmul_rn(40.f * kSegEps32, g.s);
  const float inf = __builtin_inff();
  g.ok = fabsf(px) < inf && fabsf(py) < inf && fabsf(pz) < inf && fabsf(qx) < inf && fabsf(qy) < inf && fabsf(qz) < inf;
  return g;
}

// one axis d x e_i of the separating-axis test: (ci, cj) twice the centre, (ei, ej) twice the half extents, in the two other axes
__device__ __forceinline__ bool seg_axis_separates(float ci, float cj, float di, float dj, float ei, float ej, float m) {
  const float adi = fabsf(di), adj = fabsf(dj);
  const float lhs = fabsf(__fsub_rn(__fmul_rn(ci, dj), __fmul_rn(cj, di)));
  const float rhs = __fadd_rn(__fadd_rn(__fmul_rn(ei, adj), __fmul_rn(ej, adi)), __fmul_rn(m, __fadd_rn(adi, adj)));
  return lhs > rhs;                                        // (a NaN separates nothing: the predicate refuses it)
}

__device__ __forceinline__ bool seg_box_gate(const Seg& g, const Pts& t) {
  const float lox = fmaxf(fminf(fminf(t.ax, t.bx), t.cx), g.lox), hix = fminf(fmaxf(fmaxf(t.ax, t.bx), t.cx), g.hix);
  const float loy = fmaxf(fminf(fminf(t.ay, t.by), t.cy), g.loy), hiy = fminf(fmaxf(fmaxf(t.ay, t.by), t.cy), g.hiy);
  const float loz = fmaxf(fminf(fminf(t.az, t.bz), t.cz), g.loz), hiz = fminf(fmaxf(fmaxf(t.az, t.bz), t.cz), g.hiz);
  if (!(lox <= hix && loy <= hiy && loz <= hiz)) return false;
  const float cx = __fsub_rn(__fadd_rn(lox, hix), __fadd_rn(__fmul_rn(2.f, g.px), g.dx));
  const float cy = __fsub_rn(__fadd_rn(loy, hiy), __fadd_rn(__fmul_rn(2.f, g.py), g.dy));
  const float cz = __fsub_rn(__fadd_rn(loz, hiz), __fadd_rn(__fmul_rn(2.f, g.pz), g.dz));
  const float ex = __fsub_rn(hix, lox), ey = __fsub_rn(hiy, loy), ez = __fsub_rn(hiz, loz);
  return !seg_axis_separates(cy, cz, g.dy, g.dz, ey, ez, g.m) && !seg_axis_separates(cz, cx, g.dz, g.dx, ez, ex, g.m) &&
         !seg_axis_separates(cx, cy, g.dx, g.dy, ex, ey, g.m);
}

// one axis of seg_clamp_t: the parameters at which p + t d is in [lo - kappa, hi + kappa]
__device__ __forceinline__ void seg_axis_interval(float p, float d, float lo, float hi, float kappa, float& t0, float& t1) {
  if (d == 0.f) return;                                    // (the clipped box holds p on this axis)
  const float a = __fdiv_rn(__fsub_rn(__fsub_rn(lo, kappa), p), d), b = __fdiv_rn(__fsub_rn(__fadd_rn(hi, kappa), p), d);
  t0 = fmaxf(t0, fminf(a, b));
  t1 = fminf(t1, fmaxf(a, b));
}

// tt into the parameters at which the segment is within kappa of the face's box clipped to the segment's; false: there are none
__device__ __forceinline__ bool seg_clamp_t(const Seg& g, const Pts& t, float& tt) {
  const float lox = fmaxf(fminf(fminf(t.ax, t.bx), t.cx), g.lox), hix = fminf(fmaxf(fmaxf(t.ax, t.bx), t.cx), g.hix);
  const float loy = fmaxf(fminf(fminf(t.ay, t.by), t.cy), g.loy), hiy = fminf(fmaxf(fmaxf(t.ay, t.by), t.cy), g.hiy);
  const float loz = fmaxf(fminf(fminf(t.az, t.bz), t.cz), g.loz), hiz = fminf(fmaxf(fmaxf(t.az, t.bz), t.cz), g.hiz);
  float t0 = -__builtin_inff(), t1 = __builtin_inff();
  seg_axis_interval(g.px, g.dx, lox, hix, g.kappa, t0, t1);
  seg_axis_interval(g.py, g.dy, loy, hiy, g.kappa, t0, t1);
  seg_axis_interval(g.pz, g.dz, loz, hiz, g.kappa, t0, t1);
  if (!(t0 <= t1)) return false;
  tt = fminf(fmaxf(tt, t0), t1);
  return true;
}

// the predicate and the hit parameter
__device__ __forceinline__ bool seg_tri_hit(const Seg& g, const Pts& t, float& tt) {
  const float sp = orient3(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, g.px, g.py, g.pz);
  const float sq = orient3(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, g.qx, g.qy, g.qz);
  if (!opposite(sp, sq)) return false;
  if (!edge_inside(g.px, g.py, g.pz, g.qx, g.qy, g.qz, t)) return false;
  tt = __fdiv_rn(sp, __fsub_rn(sp, sq));
  if (!(tt == tt)) return false;                           // (determinants that overflowed: inf / inf)
  return seg_clamp_t(g, t, tt);
}

// what both kernels do with the segment and face j: true when the face is hit, tt its parameter
__device__ __forceinline__ bool seg_face_hit(const Seg& g, const float* __restrict__ v, const int64_t* __restrict__ f,
                                             int64_t V, int64_t j, float& tt) {
  Pts t;
  int64_t i0, i1, i2;
  if (!load_pts(v, f, V, j, t, i0, i1, i2)) return false;
  return seg_box_gate(g, t) && seg_tri_hit(g, t, tt);
}

// the first hit: the smaller t, ties to the lower face id
__device__ __forceinline__ void seg_take_min(float t, int j, float& best, int& bidx) {
  if (t < best || (t == best && j < bidx)) { best = t; bidx = j; }
}
