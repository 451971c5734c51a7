// Texture baking: a rasteriser in the UV plane (owner, count, barycentrics per texel), edge padding as an index map, per-texel
// interpolation of vertex attributes, detail transfer from a source mesh's hits, per-vertex tangent frames and the tangent-space
// normal-map encoding — gfx950.  Not in the reference.
//
// What it computes: the GPU work of recmv.bake; include/recmv_hip.h has the definitions (the coverage rule, the texel box, the
// gutter order, the transfer formula, the tangent convention) down to the order of the operations.  Coverage and barycentrics
// are float64, un-contracted; attributes are mixed in float32 in a fixed order; the only atomics are integer (atomicMin on the
// owner image, atomicAdd on the count image), so no result depends on the order in which faces arrive.
//
// How:
//   * Work: a chart of F faces on an H x W image covers at most H W texels once, so the scatter evaluates about (box area /
//     face area) ~ 2 - 3 edge-function triples per covered texel: at 2048^2 that is ~10^7 triples of a dozen f64 flops, tens of
//     microseconds of arithmetic; the kernel is bound by the atomics' traffic (two per covered texel and face) and by how evenly
//     the boxes spread over the lanes.  Everything else is one thread per texel or vertex, a few loads and stores each.
//   * scatter: `lanes` threads per face (8 or 64) stride over the face's texel box; a box larger than one pass of its lanes
//     loops.  Few large faces want 64 lanes, many small ones 8; the launch shape changes no bit, because an owner is a minimum
//     and a count a sum of integers.
//   * resolve recomputes the owner's three edge functions at the texel centre (the same expressions, so the same bits as the
//     scatter saw) instead of storing them: 24 bytes per texel and face would be written for every candidate.
//   * gutter: ping-pong over two int32 images, one launch per pass; a texel reads its eight neighbours of the previous pass.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)
#include "mesh_device.h"

constexpr int kBakeBlock = 256;
constexpr int kBakeMaxChannels = 16;
constexpr int32_t kBakeNoOwner = 2147483647;

// E of the directed edge a -> b at (px, py), evaluated from the lower-indexed endpoint: the two faces of an edge see the same
// bits with opposite signs
__device__ __forceinline__ double bake_edge(const double* __restrict__ uv, int64_t a, int64_t b, double px, double py) {
  const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
  const double ul = uv[2 * lo], vl = uv[2 * lo + 1];
  const double e = (uv[2 * hi] - ul) * (py - vl) - (uv[2 * hi + 1] - vl) * (px - ul);
  return a > b ? -e : e;
}

// A of a face row: the edge function of i0 -> i1 at vertex i2; false when the face covers nothing
__device__ __forceinline__ bool bake_area(const double* __restrict__ uv, int64_t V, const int64_t* row, double& A) {
  A = 0.;
  if (!tri_valid(row, V)) return false;
  A = bake_edge(uv, row[0], row[1], uv[2 * row[2]], uv[2 * row[2] + 1]);
  return finite(A) && A != 0.;
}

// (E12, E20, E01) at (px, py), negated for a flipped face; whether the face covers the point
__device__ __forceinline__ bool bake_cover(const double* __restrict__ uv, const int64_t* row, bool flipped, double px, double py,
                                           double* e) {
  e[0] = bake_edge(uv, row[1], row[2], px, py);
  e[1] = bake_edge(uv, row[2], row[0], px, py);
  e[2] = bake_edge(uv, row[0], row[1], px, py);
  if (flipped) {
    e[0] = -e[0];
    e[1] = -e[1];
    e[2] = -e[2];
  }
  return e[0] >= 0. && e[1] >= 0. && e[2] >= 0.;
}

__device__ __forceinline__ void bake_centre(int64_t x, int64_t y, int64_t H, int64_t W, double& px, double& py) {
  px = ((double)x + 0.5) / (double)W;
  py = ((double)(H - y) - 0.5) / (double)H;
}

// the texel box [x0, x1] x [y0, y1] of a face with finite corners, clipped to the image; false when it is empty
__device__ __forceinline__ bool bake_box(const double* __restrict__ uv, const int64_t* row, int64_t H, int64_t W, int64_t& x0,
                                         int64_t& x1, int64_t& y0, int64_t& y1) {
  double umin = uv[2 * row[0]], umax = umin, vmin = uv[2 * row[0] + 1], vmax = vmin;
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    const double u = uv[2 * row[k]], v = uv[2 * row[k] + 1];
    if (u < umin) umin = u;
    if (u > umax) umax = u;
    if (v < vmin) vmin = v;
    if (v > vmax) vmax = v;
  }
  const double w = (double)W, h = (double)H;
  double a0 = floor(umin * w - 0.5), a1 = ceil(umax * w - 0.5);
  double b0 = floor(h - 0.5 - vmax * h), b1 = ceil(h - 0.5 - vmin * h);
  if (a0 < 0.) a0 = 0.;
  if (b0 < 0.) b0 = 0.;
  if (a1 > w - 1.) a1 = w - 1.;
  if (b1 > h - 1.) b1 = h - 1.;
  if (!(a0 <= a1 && b0 <= b1)) return false;
  x0 = (int64_t)a0;
  x1 = (int64_t)a1;
  y0 = (int64_t)b0;
  y1 = (int64_t)b1;
  return true;
}

__global__ void __launch_bounds__(kBakeBlock)
bake_clear_kernel(int64_t T, int32_t* __restrict__ owner, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  owner[i] = kBakeNoOwner;
  count[i] = 0;
}

// `lanes` consecutive threads per face stride over the face's box
__global__ void __launch_bounds__(kBakeBlock)
bake_scatter_kernel(const double* __restrict__ uv, int64_t V, const int64_t* __restrict__ faces, int64_t F, int64_t H, int64_t W,
                    int lanes, int32_t* owner, int32_t* count) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t t = tid / lanes;
  const int64_t lane = tid % lanes;
  if (t >= F) return;
  const int64_t* row = faces + 3 * t;
  double A;
  if (!bake_area(uv, V, row, A)) return;
  int64_t x0, x1, y0, y1;
  if (!bake_box(uv, row, H, W, x0, x1, y0, y1)) return;
  const int64_t bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
  for (int64_t k = lane; k < n; k += lanes) {
    const int64_t x = x0 + k % bw, y = y0 + k / bw;
    double px, py, e[3];
    bake_centre(x, y, H, W, px, py);
    if (bake_cover(uv, row, A < 0., px, py, e)) {
      atomicMin(&owner[y * W + x], (int)t);
      atomicAdd(&count[y * W + x], 1);
    }
  }
}

// owner -> face id (in place; -1: none) and the barycentrics
__global__ void __launch_bounds__(kBakeBlock)
bake_resolve_kernel(const double* __restrict__ uv, int64_t V, const int64_t* __restrict__ faces, int64_t F, int64_t H, int64_t W,
                    int32_t* __restrict__ face, float* __restrict__ bary) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * W) return;
  const int64_t t = face[i];
  float b[3] = {0.f, 0.f, 0.f};
  double A;
  int32_t out = -1;
  if (index_in(t, F) && bake_area(uv, V, faces + 3 * t, A)) {
    double px, py, e[3];
    bake_centre(i % W, i / W, H, W, px, py);
    bake_cover(uv, faces + 3 * t, A < 0., px, py, e);
    const double S = e[0] + e[1] + e[2];
    b[0] = (float)(e[0] / S);
    b[1] = (float)(e[1] / S);
    b[2] = (float)(e[2] / S);
    out = (int32_t)t;
  }
  face[i] = out;
  bary[3 * i] = b[0];
  bary[3 * i + 1] = b[1];
  bary[3 * i + 2] = b[2];
}

// ---- gutter
__global__ void __launch_bounds__(kBakeBlock)
bake_gutter_init_kernel(const int32_t* __restrict__ face, int64_t T, int32_t* __restrict__ src) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  src[i] = face[i] >= 0 ? (int32_t)i : -1;
}

// a texel still empty takes the src of its first filled neighbour in the order W, E, N, S, NW, NE, SW, SE (N is row y - 1)
__global__ void __launch_bounds__(kBakeBlock)
bake_gutter_pass_kernel(const int32_t* __restrict__ prev, int64_t H, int64_t W, int32_t* __restrict__ next) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * W) return;
  int32_t s = prev[i];
  if (s < 0) {
    const int64_t x = i % W, y = i / W;
    const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t nx = x + dx[k], ny = y + dy[k];
      if (s < 0 && index_in(nx, W) && index_in(ny, H)) {
        const int32_t c = prev[ny * W + nx];
        if (c >= 0) s = c;
      }
    }
  }
  next[i] = s;
}

__global__ void __launch_bounds__(kBakeBlock)
bake_pad_kernel(const float* __restrict__ image, const int32_t* __restrict__ src, int64_t T, int C, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  const int64_t s = src[i];
  const bool ok = index_in(s, T);
  for (int c = 0; c < C; ++c) out[i * C + c] = ok ? image[s * C + c] : 0.f;
}

// ---- attributes
// out[c] = (b0 a0[c] + b1 a1[c]) + b2 a2[c] in float32; normalise: the first three channels over their f64 length, a vector
// without a finite positive length stays
__device__ __forceinline__ void bake_mix(const float* __restrict__ attr, const int64_t* row, const float* b, int C, bool normalise,
                                         float* __restrict__ out) {
  float v[kBakeMaxChannels];
#pragma unroll
  for (int c = 0; c < kBakeMaxChannels; ++c)
    v[c] = c < C ? b[0] * attr[row[0] * C + c] + b[1] * attr[row[1] * C + c] + b[2] * attr[row[2] * C + c] : 0.f;
  if (normalise) {
    const double x = v[0], y = v[1], z = v[2];
    const double len = length3(x, y, z);
    if (finite_positive(len)) {
      v[0] = (float)(x / len);
      v[1] = (float)(y / len);
      v[2] = (float)(z / len);
    }
  }
#pragma unroll
  for (int c = 0; c < kBakeMaxChannels; ++c)
    if (c < C) out[c] = v[c];
}

__global__ void __launch_bounds__(kBakeBlock)
bake_interpolate_kernel(const int32_t* __restrict__ face, const float* __restrict__ bary, int64_t T,
                        const int64_t* __restrict__ faces, int64_t F, const float* __restrict__ attr, int64_t V, int C,
                        int normalise, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  const int64_t t = face[i];
  if (index_in(t, F) && tri_valid(faces + 3 * t, V)) {
    const float b[3] = {bary[3 * i], bary[3 * i + 1], bary[3 * i + 2]};
    bake_mix(attr, faces + 3 * t, b, C, normalise != 0, out + i * C);
  } else {
    for (int c = 0; c < C; ++c) out[i * C + c] = 0.f;
  }
}

// the barycentrics of p in the source face (f64 from the f32 corners), then the mix
__global__ void __launch_bounds__(kBakeBlock)
bake_transfer_kernel(const int64_t* __restrict__ src_face, const float* __restrict__ src_point, int64_t T,
                     const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                     const float* __restrict__ attr, int C, int normalise, float* __restrict__ bary, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  const int64_t t = src_face[i];
  float b[3] = {0.f, 0.f, 0.f};
  const bool hit = index_in(t, F) && tri_valid(faces + 3 * t, V);
  if (hit) {
    const int64_t* row = faces + 3 * t;
    double p0[3], p1[3], p2[3], p[3];
    load3(verts, row[0], p0);
    load3(verts, row[1], p1);
    load3(verts, row[2], p2);
    load3(src_point, i, p);
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double d[3] = {p[0] - p0[0], p[1] - p0[1], p[2] - p0[2]};
    const double d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), r1 = dot3(d, e1), r2 = dot3(d, e2);
    const double det = d11 * d22 - d12 * d12;
    double b1 = 0., b2 = 0.;
    if (finite_positive(det)) {
      b1 = (d22 * r1 - d12 * r2) / det;
      b2 = (d11 * r2 - d12 * r1) / det;
    }
    b[0] = (float)(1. - b1 - b2);
    b[1] = (float)b1;
    b[2] = (float)b2;
    bake_mix(attr, row, b, C, normalise != 0, out + i * C);
  } else {
    for (int c = 0; c < C; ++c) out[i * C + c] = 0.f;
  }
  bary[3 * i] = b[0];
  bary[3 * i + 1] = b[1];
  bary[3 * i + 2] = b[2];
}

// ---- tangent frames: one thread per vertex over its faces in the adjacency's order
__global__ void __launch_bounds__(kBakeBlock)
bake_vertex_tangents_kernel(const float* __restrict__ verts, const double* __restrict__ uv, const float* __restrict__ normals,
                            int64_t V, const int64_t* __restrict__ faces, int64_t F, const int32_t* __restrict__ adj_off,
                            const int32_t* __restrict__ adj_codes, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  double T[3] = {0., 0., 0.}, B[3] = {0., 0., 0.};
  const CsrRow fan = csr_range_ordered(adj_off, i, 3 * F);
  for (int64_t s = fan.k0; s < fan.k1; ++s) {
    const int64_t code = adj_codes[s];
    if (!index_in(code, 3 * F)) continue;
    const int64_t* row = faces + 3 * (code / 3);
    double A;
    if (!bake_area(uv, V, row, A)) continue;
    double p0[3], p1[3], p2[3], n[3];
    load3(verts, row[0], p0);
    load3(verts, row[1], p1);
    load3(verts, row[2], p2);
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    cross3(e1, e2, n);
    const double area = 0.5 * sqrt(dot3(n, n));
    if (!finite_positive(area)) continue;
    const double du1 = uv[2 * row[1]] - uv[2 * row[0]], dv1 = uv[2 * row[1] + 1] - uv[2 * row[0] + 1];
    const double du2 = uv[2 * row[2]] - uv[2 * row[0]], dv2 = uv[2 * row[2] + 1] - uv[2 * row[0] + 1];
    const double w = area / A;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T[c] += w * (e1[c] * dv2 - e2[c] * dv1);
      B[c] += w * (e2[c] * du1 - e1[c] * du2);
    }
  }
  double n[3];
  load3(normals, i, n);
  const double nt = dot3(n, T);
  double t[3] = {T[0] - n[0] * nt, T[1] - n[1] * nt, T[2] - n[2] * nt};
  const double len = sqrt(dot3(t, t));
  float r[4] = {0.f, 0.f, 0.f, 1.f};
  if (finite_positive(len)) {
    t[0] = t[0] / len;
    t[1] = t[1] / len;
    t[2] = t[2] / len;
    double c[3];
    cross3(n, t, c);
    r[0] = (float)t[0];
    r[1] = (float)t[1];
    r[2] = (float)t[2];
    r[3] = dot3(c, B) < 0. ? -1.f : 1.f;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) out[4 * i + c] = r[c];
}

// the normal N in the frame (t', cross(n, t') w, n), t' = t made orthogonal to n, as 0.5 + 0.5 c; zeros where the texel has no owner
__global__ void __launch_bounds__(kBakeBlock)
bake_encode_normal_kernel(const int32_t* __restrict__ face, const float* __restrict__ normal, const float* __restrict__ frame_n,
                          const float* __restrict__ frame_t, int64_t T, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  float r[3] = {0.f, 0.f, 0.f};
  if (face[i] >= 0) {
    double N[3], n[3], t[3], b[3];
    load3(normal, i, N);
    load3(frame_n, i, n);
    t[0] = frame_t[4 * i];
    t[1] = frame_t[4 * i + 1];
    t[2] = frame_t[4 * i + 2];
    const double w = frame_t[4 * i + 3] < 0.f ? -1. : 1.;
    const double nt = dot3(n, t);                          // the interpolated tangent, made orthogonal to the interpolated normal again
    const double o[3] = {t[0] - n[0] * nt, t[1] - n[1] * nt, t[2] - n[2] * nt};
    const double len = sqrt(dot3(o, o));
    if (finite_positive(len)) {
      t[0] = o[0] / len;
      t[1] = o[1] / len;
      t[2] = o[2] / len;
    }
    cross3(n, t, b);
    r[0] = (float)(0.5 + 0.5 * dot3(N, t));
    r[1] = (float)(0.5 + 0.5 * (w * dot3(N, b)));
    r[2] = (float)(0.5 + 0.5 * dot3(N, n));
  }
  out[3 * i] = r[0];
  out[3 * i + 1] = r[1];
  out[3 * i + 2] = r[2];
}

inline unsigned bake_grid(int64_t n) { return (unsigned)((n + kBakeBlock - 1) / kBakeBlock); }

// sizes every entry point shares; false with a message
bool bake_sizes(const char* who, const char* a_name, int64_t a, const char* b_name, int64_t b) {
  if (a < 0 || b < 0) {
    set_error("%s: %s=%lld, %s=%lld must not be negative", who, a_name, (long long)a, b_name, (long long)b);
    return false;
  }
  if (a >= (1ll << 31) || b >= (1ll << 31)) {
    set_error("%s: %s and %s must be below 2^31", who, a_name, b_name);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int recmv_bake_raster(const double* uv, int64_t V, const int64_t* faces, int64_t F, int64_t H, int64_t W, int32_t lanes,
                                 int32_t* face, float* bary, int32_t* count, void* stream) {
  if (!bake_sizes("bake_raster", "V", V, "F", F)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(H >= 0 && W >= 0, "bake_raster: H=%lld, W=%lld must not be negative", (long long)H, (long long)W);
  RECMV_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && (H == 0 || W < (1ll << 31) / H),
                "bake_raster: H=%lld x W=%lld texels, at most 2^31 - 1", (long long)H, (long long)W);
  RECMV_REQUIRE(lanes == 8 || lanes == 64, "bake_raster: lanes=%d must be 8 or 64", (int)lanes);
  const int64_t T = H * W;
  if (T == 0) return RECMV_OK;
  RECMV_REQUIRE(face && bary && count, "bake_raster: NULL image");
  RECMV_REQUIRE(F == 0 || (faces && uv), "bake_raster: NULL pointer of the mesh");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  bake_clear_kernel<<<bake_grid(T), kBakeBlock, 0, s>>>(T, face, count);
  if ((rc = check_launch("bake_clear")) != RECMV_OK) return rc;
  if (F > 0) {
    bake_scatter_kernel<<<bake_grid(F * lanes), kBakeBlock, 0, s>>>(uv, V, faces, F, H, W, (int)lanes, face, count);
    if ((rc = check_launch("bake_scatter")) != RECMV_OK) return rc;
  }
  bake_resolve_kernel<<<bake_grid(T), kBakeBlock, 0, s>>>(uv, V, faces, F, H, W, face, bary);
  return check_launch("bake_resolve");
}

extern "C" int recmv_bake_gutter(const int32_t* face, int64_t H, int64_t W, int32_t passes, int32_t* src, int32_t* scratch,
                                 void* stream) {
  RECMV_REQUIRE(H >= 0 && W >= 0, "bake_gutter: H=%lld, W=%lld must not be negative", (long long)H, (long long)W);
  RECMV_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && (H == 0 || W < (1ll << 31) / H),
                "bake_gutter: H=%lld x W=%lld texels, at most 2^31 - 1", (long long)H, (long long)W);
  RECMV_REQUIRE(passes >= 0, "bake_gutter: passes=%d must not be negative", (int)passes);
  const int64_t T = H * W;
  if (T == 0) return RECMV_OK;
  RECMV_REQUIRE(face && src, "bake_gutter: NULL image");
  RECMV_REQUIRE(passes == 0 || scratch, "bake_gutter: NULL scratch image");
  hipStream_t s = (hipStream_t)stream;
  int32_t* buf[2] = {src, scratch};
  int cur = passes % 2;                                    // an even number of swaps ends in src
  int rc;
  bake_gutter_init_kernel<<<bake_grid(T), kBakeBlock, 0, s>>>(face, T, buf[cur]);
  if ((rc = check_launch("bake_gutter_init")) != RECMV_OK) return rc;
  for (int k = 0; k < passes; ++k, cur ^= 1) {
    bake_gutter_pass_kernel<<<bake_grid(T), kBakeBlock, 0, s>>>(buf[cur], H, W, buf[cur ^ 1]);
    if ((rc = check_launch("bake_gutter_pass")) != RECMV_OK) return rc;
  }
  return RECMV_OK;
}

extern "C" int recmv_bake_pad(const float* image, const int32_t* src, int64_t T, int32_t C, float* out, void* stream) {
  if (!bake_sizes("bake_pad", "T", T, "C", C)) return RECMV_ERR_ARG;
  if (T == 0 || C == 0) return RECMV_OK;
  RECMV_REQUIRE(image && src && out, "bake_pad: NULL pointer");
  RECMV_REQUIRE(image != out, "bake_pad: out must not be the image");
  bake_pad_kernel<<<bake_grid(T), kBakeBlock, 0, (hipStream_t)stream>>>(image, src, T, (int)C, out);
  return check_launch("bake_pad");
}

extern "C" int recmv_bake_interpolate(const int32_t* face, const float* bary, int64_t T, const int64_t* faces, int64_t F,
                                      const float* attr, int64_t V, int32_t C, int32_t normalise, float* out, void* stream) {
  if (!bake_sizes("bake_interpolate", "T", T, "F", F)) return RECMV_ERR_ARG;
  if (!bake_sizes("bake_interpolate", "V", V, "C", C)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(C >= 1 && C <= kBakeMaxChannels, "bake_interpolate: C=%d must be 1 .. %d", (int)C, kBakeMaxChannels);
  RECMV_REQUIRE(!normalise || C >= 3, "bake_interpolate: normalise needs C >= 3 (C=%d)", (int)C);
  if (T == 0) return RECMV_OK;
  RECMV_REQUIRE(face && bary && out, "bake_interpolate: NULL image");
  RECMV_REQUIRE(F == 0 || V == 0 || (faces && attr), "bake_interpolate: NULL pointer of the mesh");
  bake_interpolate_kernel<<<bake_grid(T), kBakeBlock, 0, (hipStream_t)stream>>>(face, bary, T, faces, F, attr, V, (int)C,
                                                                                 (int)normalise, out);
  return check_launch("bake_interpolate");
}

extern "C" int recmv_bake_transfer(const int64_t* src_face, const float* src_point, int64_t T, const float* src_verts, int64_t V,
                                   const int64_t* src_faces, int64_t F, const float* attr, int32_t C, int32_t normalise,
                                   float* bary, float* out, void* stream) {
  if (!bake_sizes("bake_transfer", "T", T, "F", F)) return RECMV_ERR_ARG;
  if (!bake_sizes("bake_transfer", "V", V, "C", C)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(C >= 1 && C <= kBakeMaxChannels, "bake_transfer: C=%d must be 1 .. %d", (int)C, kBakeMaxChannels);
  RECMV_REQUIRE(!normalise || C >= 3, "bake_transfer: normalise needs C >= 3 (C=%d)", (int)C);
  if (T == 0) return RECMV_OK;
  RECMV_REQUIRE(src_face && src_point && bary && out, "bake_transfer: NULL pointer of the hits");
  RECMV_REQUIRE(F == 0 || V == 0 || (src_verts && src_faces && attr), "bake_transfer: NULL pointer of the source");
  bake_transfer_kernel<<<bake_grid(T), kBakeBlock, 0, (hipStream_t)stream>>>(src_face, src_point, T, src_verts, V, src_faces, F,
                                                                              attr, (int)C, (int)normalise, bary, out);
  return check_launch("bake_transfer");
}

extern "C" int recmv_bake_vertex_tangents(const float* verts, const double* uv, const float* normals, int64_t V,
                                          const int64_t* faces, int64_t F, const int32_t* adj_offsets, const int32_t* adj_codes,
                                          float* out, void* stream) {
  if (!bake_sizes("bake_vertex_tangents", "V", V, "F", F)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(3 * F < (1ll << 31), "bake_vertex_tangents: F=%lld, at most (2^31 - 1) / 3 faces", (long long)F);
  if (V == 0) return RECMV_OK;
  RECMV_REQUIRE(verts && uv && normals && adj_offsets && out, "bake_vertex_tangents: NULL pointer of the vertices");
  RECMV_REQUIRE(F == 0 || (faces && adj_codes), "bake_vertex_tangents: NULL pointer of the faces");
  bake_vertex_tangents_kernel<<<bake_grid(V), kBakeBlock, 0, (hipStream_t)stream>>>(verts, uv, normals, V, faces, F, adj_offsets,
                                                                                     adj_codes, out);
  return check_launch("bake_vertex_tangents");
}

extern "C" int recmv_bake_encode_normal(const int32_t* face, const float* normal, const float* frame_n, const float* frame_t,
                                        int64_t T, float* out, void* stream) {
  if (!bake_sizes("bake_encode_normal", "T", T, "T", T)) return RECMV_ERR_ARG;
  if (T == 0) return RECMV_OK;
  RECMV_REQUIRE(face && normal && frame_n && frame_t && out, "bake_encode_normal: NULL pointer");
  bake_encode_normal_kernel<<<bake_grid(T), kBakeBlock, 0, (hipStream_t)stream>>>(face, normal, frame_n, frame_t, T, out);
  return check_launch("bake_encode_normal");
}
