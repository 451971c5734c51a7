// One 3x3 inverse by cofactor expansion with the reference's singularity test (FastMinv/Matrix3x3InvKernels.cu:22-104),
// shared by inv3x3.hip and nricp.hip so the NR-ICP validity mask is the one Fast3x3Minv returns.  Include it inside
// namespace recmv after `#pragma clang fp contract(off)`: the arithmetic must stay un-contracted.
#pragma once

template <typename T>
__device__ __forceinline__ bool inv_one(const T* m, T* inv) {
  T cof00 = m[4] * m[8] - m[5] * m[7];
  T cof01 = -m[3] * m[8] + m[5] * m[6];
  T cof02 = m[3] * m[7] - m[4] * m[6];
  T cof10 = -m[1] * m[8] + m[2] * m[7];
  T cof11 = m[0] * m[8] - m[2] * m[6];
  T cof12 = -m[0] * m[7] + m[1] * m[6];
  T cof20 = m[1] * m[5] - m[2] * m[4];
  T cof21 = -m[0] * m[5] + m[2] * m[3];
  T cof22 = m[0] * m[4] - m[1] * m[3];
  T det = m[0] * cof00 + m[1] * cof01 + m[2] * cof02;
  // reference: fabs(det) < 0.0001 with a double literal -> the comparison is done in double
  if (fabs((double)det) < 0.0001) {
#pragma unroll
    for (int i = 0; i < 9; ++i) inv[i] = (T)0;
    return false;
  }
  inv[0] = cof00 / det;
  inv[1] = cof10 / det;
  inv[2] = cof20 / det;
  inv[3] = cof01 / det;
  inv[4] = cof11 / det;
  inv[5] = cof21 / det;
  inv[6] = cof02 / det;
  inv[7] = cof12 / det;
  inv[8] = cof22 / det;
  return true;
}
