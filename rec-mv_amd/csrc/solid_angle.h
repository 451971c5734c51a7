// The signed solid angle of a triangle seen from a point (Van Oosterom & Strackee 1983) in f32 and the first-order (dipole)
// far-field term of a cluster of faces, shared by the exact and the tree kernels of winding.hip so that a face gives the same
// bits on either route.  Plain C++ that also compiles for the host.  Include it inside namespace recmv after
// `#pragma clang fp contract(off)`: the arithmetic must stay un-contracted.
#pragma once

// Omega = 2 atan2( a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b| ) with a = A - q, b = B - q, c = C - q: positive
// when the face's corners run counter-clockwise seen from the far side of q (q behind an outward-oriented face).
//   * a face without area has a zero numerator over a denominator that is not negative: 0;
//   * a corner or a query that is NaN gives NaN (the callers turn every non-finite corner and query into NaN first, so
//     that inf - inf and atan2(inf, inf) never decide);
//   * a query exactly on the face gets 2 atan2(+-0, negative) = +-2 pi: a winding term of +-1/2.
// `t` points at the face's 9 floats: A, B, C.
__device__ __forceinline__ float solid_angle(float qx, float qy, float qz, const float* t) {
  const float ax = t[0] - qx, ay = t[1] - qy, az = t[2] - qz;
  const float bx = t[3] - qx, by = t[4] - qy, bz = t[5] - qz;
  const float cx = t[6] - qx, cy = t[7] - qy, cz = t[8] - qz;
  const float la = sqrtf(ax * ax + ay * ay + az * az);
  const float lb = sqrtf(bx * bx + by * by + bz * bz);
  const float lc = sqrtf(cx * cx + cy * cy + cz * cz);
  const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  const float ab = ax * bx + ay * by + az * bz;
  const float bc = bx * cx + by * cy + bz * cz;
  const float ca = cx * ax + cy * ay + cz * az;
  const float den = la * lb * lc + ab * lc + bc * la + ca * lb;
  return 2.f * atan2f(det, den);
}

// The corners of face k as 9 floats A, B, C.  A face with an index outside [0, V) becomes nine zeros: every term of it is 0
// (a zero numerator over 4 |q|^3).  A face with a corner that is not finite becomes nine NaN.  false for the first kind.
__device__ __forceinline__ bool load_corners(const float* __restrict__ v, const int64_t* __restrict__ f, int64_t V, int64_t k,
                                             float* t) {
  const int64_t i0 = f[3 * k], i1 = f[3 * k + 1], i2 = f[3 * k + 2];
  if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) {
    for (int a = 0; a < 9; ++a) t[a] = 0.f;
    return false;
  }
  float z = 0.f;                                            // 0 * x: NaN exactly when x is not finite
  for (int a = 0; a < 3; ++a) {
    t[a] = v[3 * i0 + a];
    t[3 + a] = v[3 * i1 + a];
    t[6 + a] = v[3 * i2 + a];
    z += 0.f * t[a] + 0.f * t[3 + a] + 0.f * t[6 + a];
  }
  if (z != z)
    for (int a = 0; a < 9; ++a) t[a] = __builtin_nanf("");
  return true;
}

// One node of the pyramid, 16 floats: [0] the area sum, [1..3] the area-weighted centroid sum, [4..6] the area-vector sum
// N = sum of (B - A) x (C - A) / 2, [7] the number of faces (the bits of an int32), [8..10] and [12..14] the low and the high
// corner of the box of the faces' corners; [11] and [15] are 0.
constexpr int kNodeFloats = 16;

struct NodeSum {
  float area, sx, sy, sz, nx, ny, nz;
  int32_t count;
  float lox, loy, loz, hix, hiy, hiz;
};

__device__ __forceinline__ void node_clear(NodeSum& s) {
  s.area = s.sx = s.sy = s.sz = s.nx = s.ny = s.nz = 0.f;
  s.count = 0;
  s.lox = s.loy = s.loz = __builtin_inff();
  s.hix = s.hiy = s.hiz = -__builtin_inff();
}

// Adds one face (9 finite floats) to a node.
__device__ __forceinline__ void node_add_face(NodeSum& s, const float* t) {
  const float ux = t[3] - t[0], uy = t[4] - t[1], uz = t[5] - t[2];
  const float vx = t[6] - t[0], vy = t[7] - t[1], vz = t[8] - t[2];
  const float nx = 0.5f * (uy * vz - uz * vy), ny = 0.5f * (uz * vx - ux * vz), nz = 0.5f * (ux * vy - uy * vx);
  const float area = sqrtf(nx * nx + ny * ny + nz * nz);
  s.area += area;
  s.sx += area * (((t[0] + t[3]) + t[6]) / 3.f);
  s.sy += area * (((t[1] + t[4]) + t[7]) / 3.f);
  s.sz += area * (((t[2] + t[5]) + t[8]) / 3.f);
  s.nx += nx;
  s.ny += ny;
  s.nz += nz;
  s.count += 1;
  s.lox = fminf(s.lox, fminf(t[0], fminf(t[3], t[6])));
  s.loy = fminf(s.loy, fminf(t[1], fminf(t[4], t[7])));
  s.loz = fminf(s.loz, fminf(t[2], fminf(t[5], t[8])));
  s.hix = fmaxf(s.hix, fmaxf(t[0], fmaxf(t[3], t[6])));
  s.hiy = fmaxf(s.hiy, fmaxf(t[1], fmaxf(t[4], t[7])));
  s.hiz = fmaxf(s.hiz, fmaxf(t[2], fmaxf(t[5], t[8])));
}

__device__ __forceinline__ int32_t node_count(const float* n) {
  int32_t c;
  memcpy(&c, n + 7, 4);
  return c;
}

// Adds a child node (its 16 floats) to a parent's sums.
__device__ __forceinline__ void node_add_node(NodeSum& s, const float* n) {
  const int32_t c = node_count(n);
  if (c == 0) return;
  s.area += n[0];
  s.sx += n[1];
  s.sy += n[2];
  s.sz += n[3];
  s.nx += n[4];
  s.ny += n[5];
  s.nz += n[6];
  s.count = (int32_t)((uint32_t)s.count + (uint32_t)c);
  s.lox = fminf(s.lox, n[8]);
  s.loy = fminf(s.loy, n[9]);
  s.loz = fminf(s.loz, n[10]);
  s.hix = fmaxf(s.hix, n[12]);
  s.hiy = fmaxf(s.hiy, n[13]);
  s.hiz = fmaxf(s.hiz, n[14]);
}

__device__ __forceinline__ void node_store(const NodeSum& s, float* n) {
  n[0] = s.area; n[1] = s.sx; n[2] = s.sy; n[3] = s.sz;
  n[4] = s.nx; n[5] = s.ny; n[6] = s.nz;
  memcpy(n + 7, &s.count, 4);
  const bool any = s.count != 0;                             // an empty node stores a box of zeros, never +-inf
  n[8] = any ? s.lox : 0.f; n[9] = any ? s.loy : 0.f; n[10] = any ? s.loz : 0.f; n[11] = 0.f;
  n[12] = any ? s.hix : 0.f; n[13] = any ? s.hiy : 0.f; n[14] = any ? s.hiz : 0.f; n[15] = 0.f;
}

// The far-field test and term of a node that holds faces.  The centre is the centroid sum over the area sum, or the
// box's centre when the area sum is 0; r is the largest distance from it to a corner of the box.  true when
// |q - centre|^2 > beta2 * r^2 (beta2 = beta * beta, formed once in f32; NaN refuses), and then `term` is the node's
// solid angle to first order, N . (centre - q) / |centre - q|^3.
__device__ __forceinline__ bool node_far(const float* n, float qx, float qy, float qz, float beta2, float& term) {
  float px, py, pz;
  if (n[0] > 0.f) {
    px = n[1] / n[0]; py = n[2] / n[0]; pz = n[3] / n[0];
  } else {
    px = 0.5f * (n[8] + n[12]); py = 0.5f * (n[9] + n[13]); pz = 0.5f * (n[10] + n[14]);
  }
  const float ex = fmaxf(px - n[8], n[12] - px), ey = fmaxf(py - n[9], n[13] - py), ez = fmaxf(pz - n[10], n[14] - pz);
  const float r2 = ex * ex + ey * ey + ez * ez;
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  const float d2 = dx * dx + dy * dy + dz * dz;
  if (!(d2 > beta2 * r2)) return false;
  term = (n[4] * dx + n[5] * dy + n[6] * dz) / (d2 * sqrtf(d2));
  return true;
}
