// Exact closest point of a triangle to a point (Ericson, Real-Time Collision Detection, §5.1.5) in f32, shared by
// iso_remesh.hip (recmv_closest_point) and mesh_collide.hip (recmv_point_mesh_nearest, recmv_collision_push) so that both
// give the same bits for the same point and face.  Include it inside namespace recmv after `#pragma clang fp contract(off)`:
// the arithmetic must stay un-contracted.
#pragma once

struct Tri {
  float ax, ay, az, bx, by, bz, cx, cy, cz;                // a, ab = b - a, ac = c - a
};

// Which of Ericson's tests held: the part of the triangle the closest point lies on.  The numbers are the bit positions of
// recmv_icp_accumulate's border flags (include/recmv_hip.h); the face's inside has none.
enum Region : int { kEdgeAB = 0, kEdgeAC = 1, kEdgeBC = 2, kVertexA = 3, kVertexB = 4, kVertexC = 5, kInside = 6 };

// Ericson's ClosestPtPointTriangle with the point relative to a: (s, t) such that the closest point is a + s ab + t ac,
// the squared distance |ap - s ab - t ac|^2, and the region whose test held.
__device__ __forceinline__ float closest_st_region(float px, float py, float pz, const Tri& q, float& s, float& t,
                                                   int& region) {
  const float apx = px - q.ax, apy = py - q.ay, apz = pz - q.az;
  const float d1 = q.bx * apx + q.by * apy + q.bz * apz;
  const float d2 = q.cx * apx + q.cy * apy + q.cz * apz;
  const float bpx = apx - q.bx, bpy = apy - q.by, bpz = apz - q.bz;
  const float d3 = q.bx * bpx + q.by * bpy + q.bz * bpz;
  const float d4 = q.cx * bpx + q.cy * bpy + q.cz * bpz;
  const float cpx = apx - q.cx, cpy = apy - q.cy, cpz = apz - q.cz;
  const float d5 = q.bx * cpx + q.by * cpy + q.bz * cpz;
  const float d6 = q.cx * cpx + q.cy * cpy + q.cz * cpz;
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  if (d1 <= 0.f && d2 <= 0.f) {                            // vertex region a
    s = 0.f; t = 0.f; region = kVertexA;
  } else if (d3 >= 0.f && d4 <= d3) {                      // vertex region b
    s = 1.f; t = 0.f; region = kVertexB;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {        // edge ab
    s = d1 / (d1 - d3); t = 0.f; region = kEdgeAB;
  } else if (d6 >= 0.f && d5 <= d6) {                      // vertex region c
    s = 0.f; t = 1.f; region = kVertexC;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {        // edge ac
    s = 0.f; t = d2 / (d2 - d6); region = kEdgeAC;
  } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {   // edge bc
    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    s = 1.f - w; t = w; region = kEdgeBC;
  } else {                                                 // inside the face
    const float den = 1.f / (va + vb + vc);
    s = vb * den; t = vc * den; region = kInside;
  }
  const float dx = apx - s * q.bx - t * q.cx;
  const float dy = apy - s * q.by - t * q.cy;
  const float dz = apz - s * q.bz - t * q.cz;
  return dx * dx + dy * dy + dz * dz;
}

// The same without the region: the one body above, so both give the same bits.
__device__ __forceinline__ float closest_st(float px, float py, float pz, const Tri& q, float& s, float& t) {
  int region;
  return closest_st_region(px, py, pz, q, s, t, region);
}

// The face's vertices (false when an index lies outside [0, V): such a face is skipped).
__device__ __forceinline__ bool load_tri(const float* __restrict__ v, const int64_t* __restrict__ f, int64_t V, int64_t k,
                                         Tri& q) {
  const int64_t i0 = f[3 * k], i1 = f[3 * k + 1], i2 = f[3 * k + 2];
  if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) return false;
  q.ax = v[3 * i0]; q.ay = v[3 * i0 + 1]; q.az = v[3 * i0 + 2];
  q.bx = v[3 * i1] - q.ax; q.by = v[3 * i1 + 1] - q.ay; q.bz = v[3 * i1 + 2] - q.az;
  q.cx = v[3 * i2] - q.ax; q.cy = v[3 * i2 + 1] - q.ay; q.cz = v[3 * i2 + 2] - q.az;
  return true;
}
