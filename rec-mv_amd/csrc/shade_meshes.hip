// Vertex normals and hard Phong shading of rasterised meshes — gfx950.
//
// What it computes: the images the reference's inference renders with pytorch3d 0.4.0's
// `MeshRendererWithFragments(MeshRasterizer, HardPhongShader)` and white `TexturesVertex`
// (engineer/networks/OptimGarmentNetwork.py:3216-3306 `infer`; the shader is set by infer_fl.py).  pytorch3d is a
// third-party dependency that is not vendored in the reference tree, so its published arithmetic is restated here:
//   * Meshes._compute_vertex_normals: for every face the three corner cross products, added per vertex in the order
//     corner 1 (v2-v1)x(v0-v1), corner 2 (v0-v2)x(v1-v2), corner 0 (v1-v0)x(v2-v0), each pass in face order
//     (three `index_add`s), then F.normalize(eps=1e-6);
//   * shading.phong_shading + lighting.PointLights / _apply_lighting + blending.hard_rgb_blend: interpolate the
//     corner positions, normals and vertex colours with the fragment's barycentrics, diffuse = relu(n.l),
//     specular = [n.l > 0] relu(v.(2(n.l)n - l))^shininess, colour = (ambient + diffuse) * texel + specular,
//     background colour where no face covers the pixel, alpha 1.
//
// How: no float atomics anywhere.  The normals are a gather per (mesh, vertex) over a vertex -> (face, corner) list
// built once per face table (recmv/shading.py: a stable sort of the corner-1, corner-2, corner-0 lists), so every
// vertex sums its contributions in pytorch3d's order and the result does not depend on scheduling or on the number of
// meshes.  The shader is one thread per pixel; its optional silhouette counts (|M n G|, |M u G| per frame) are integer:
// reduced per workgroup, one 64-bit atomic add per workgroup, exact whatever the order.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "mesh_device.h"                                   // wave_sum, index_in

constexpr float kNormEps = 1e-6f;      // F.normalize(eps=1e-6) of pytorch3d's normals and lighting directions
constexpr int kShadeBlock = 256;

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 normalize(V3 a) {
  const float n = fmaxf(sqrtf(a.x * a.x + a.y * a.y + a.z * a.z), kNormEps);
  return {a.x / n, a.y / n, a.z / n};
}
__device__ __forceinline__ V3 load3(const float* p, int64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
// w0 a0 + w1 a1 + w2 a2, left to right (pytorch3d's interpolate_face_attributes)
__device__ __forceinline__ V3 interp(float w0, float w1, float w2, V3 a, V3 b, V3 c) {
  return {w0 * a.x + w1 * b.x + w2 * c.x, w0 * a.y + w1 * b.y + w2 * c.y, w0 * a.z + w1 * b.z + w2 * c.z};
}

// One thread per (mesh, vertex).  adj_offsets [V+1], adj_codes [3F] (face * 3 + corner) in pytorch3d's summation order.
__global__ void __launch_bounds__(256)
verts_normals_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                     const int32_t* __restrict__ adj_offsets, const int32_t* __restrict__ adj_codes, int64_t N,
                     int64_t V, int64_t F, float* __restrict__ normals) {
  const int64_t total = N * V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t n = i / V, v = i - n * V;
    const float* vb = verts + n * V * 3;
    V3 acc = {0.f, 0.f, 0.f};
    const int32_t e0 = adj_offsets[v], e1 = adj_offsets[v + 1];
    for (int32_t e = e0; e < e1; ++e) {
      const int64_t code = adj_codes[e];
      const int64_t f = code / 3;
      const int corner = (int)(code - 3 * f);
      if (f < 0 || f >= F) continue;
      const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if ((uint64_t)i0 >= (uint64_t)V || (uint64_t)i1 >= (uint64_t)V || (uint64_t)i2 >= (uint64_t)V) continue;
      const V3 p0 = load3(vb, i0), p1 = load3(vb, i1), p2 = load3(vb, i2);
      V3 c;
      if (corner == 1)
        c = cross(sub(p2, p1), sub(p0, p1));
      else if (corner == 2)
        c = cross(sub(p0, p2), sub(p1, p2));
      else
        c = cross(sub(p1, p0), sub(p2, p0));
      acc = {acc.x + c.x, acc.y + c.y, acc.z + c.z};
    }
    const V3 r = normalize(acc);
    normals[3 * i + 0] = r.x;
    normals[3 * i + 1] = r.y;
    normals[3 * i + 2] = r.z;
  }
}

struct ShadeParams {
  float light_loc[3], light_amb[3], light_diff[3], light_spec[3];
  float mat_amb[3], mat_diff[3], mat_spec[3];
  float shininess;
  float background[3];
};

// grid (x: pixel blocks of one frame, y: frame n).  pix_to_face [N,H,W] packed (mesh * F + face), bary [N,H,W,3].
__global__ void __launch_bounds__(kShadeBlock)
hard_phong_kernel(const int64_t* __restrict__ pix_to_face, const float* __restrict__ bary,
                  const float* __restrict__ verts, const float* __restrict__ normals,
                  const float* __restrict__ colors, int64_t colors_batch, const int64_t* __restrict__ faces,
                  const float* __restrict__ cam_centers, int64_t N, int64_t V, int64_t F, int64_t HW, ShadeParams prm,
                  float* __restrict__ out, const float* __restrict__ gt_mask, unsigned long long* __restrict__ counts) {
  const int64_t n = blockIdx.y;
  const V3 cam = load3(cam_centers, n);
  const V3 lloc = {prm.light_loc[0], prm.light_loc[1], prm.light_loc[2]};
  int inter = 0, uni = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += stride) {
    const int64_t i = n * HW + p;
    const int64_t face = pix_to_face[i];
    float rgb[3] = {prm.background[0], prm.background[1], prm.background[2]};
    const bool fg = face >= 0 && face < N * F;
    if (fg) {
      const int64_t m = face / F, f = face - m * F;
      const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if (index_in(i0, V) && index_in(i1, V) && index_in(i2, V)) {
        const float w0 = bary[3 * i], w1 = bary[3 * i + 1], w2 = bary[3 * i + 2];
        const float* vb = verts + m * V * 3;
        const float* nb = normals + m * V * 3;
        const float* cb = colors + (colors_batch == 1 ? 0 : m) * V * 3;
        const V3 pt = interp(w0, w1, w2, load3(vb, i0), load3(vb, i1), load3(vb, i2));
        const V3 nrm = normalize(interp(w0, w1, w2, load3(nb, i0), load3(nb, i1), load3(nb, i2)));
        const V3 tex = interp(w0, w1, w2, load3(cb, i0), load3(cb, i1), load3(cb, i2));
        const V3 ldir = normalize(sub(lloc, pt));
        const float cosang = dot(nrm, ldir);
        const float angle = fmaxf(cosang, 0.f);                                   // relu(n.l)
        const float mask = cosang > 0.f ? 1.f : 0.f;
        const V3 view = normalize(sub(cam, pt));
        const V3 refl = {-ldir.x + 2.f * (cosang * nrm.x), -ldir.y + 2.f * (cosang * nrm.y),
                         -ldir.z + 2.f * (cosang * nrm.z)};
        const float alpha = fmaxf(dot(view, refl), 0.f) * mask;
        const float spec = powf(alpha, prm.shininess);
        const float texc[3] = {tex.x, tex.y, tex.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float amb = prm.mat_amb[k] * prm.light_amb[k];
          const float dif = prm.mat_diff[k] * (prm.light_diff[k] * angle);
          const float spc = prm.mat_spec[k] * (prm.light_spec[k] * spec);
          rgb[k] = (amb + dif) * texc[k] + spc;
        }
      }
    }
    float4 o;
    o.x = rgb[0];
    o.y = rgb[1];
    o.z = rgb[2];
    o.w = 1.f;
    *reinterpret_cast<float4*>(out + 4 * i) = o;
    if (gt_mask != nullptr) {
      const bool g = gt_mask[i] != 0.f;
      inter += (fg && g) ? 1 : 0;
      uni += (fg || g) ? 1 : 0;
    }
  }
  if (counts == nullptr) return;
  __shared__ int s_i[kShadeBlock / kWave], s_u[kShadeBlock / kWave];
  inter = wave_sum(inter);
  uni = wave_sum(uni);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_i[wave] = inter;
    s_u[wave] = uni;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int ti = 0, tu = 0;
    for (int w = 0; w < kShadeBlock / kWave; ++w) {
      ti += s_i[w];
      tu += s_u[w];
    }
    if (ti) atomicAdd(counts + 2 * n, (unsigned long long)ti);
    if (tu) atomicAdd(counts + 2 * n + 1, (unsigned long long)tu);
  }
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int recmv_verts_normals(const float* verts, const int64_t* faces, const int32_t* adj_offsets,
                                   const int32_t* adj_codes, int64_t N, int64_t V, int64_t F, float* normals,
                                   void* stream) {
  RECMV_REQUIRE(N >= 0 && V >= 0 && F >= 0, "verts_normals: bad sizes N=%lld V=%lld F=%lld", (long long)N,
                (long long)V, (long long)F);
  RECMV_REQUIRE(3 * F < (1ll << 31) && V < (1ll << 31), "verts_normals: at most 2^31 / 3 faces and 2^31 vertices");
  if (N == 0 || V == 0) return RECMV_OK;
  RECMV_REQUIRE(verts && faces && adj_offsets && adj_codes && normals, "verts_normals: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  verts_normals_kernel<<<stream_grid(N * V, 256), 256, 0, s>>>(verts, faces, adj_offsets, adj_codes, N, V, F, normals);
  return check_launch("verts_normals");
}

extern "C" int recmv_hard_phong_shade(const int64_t* pix_to_face, const float* bary_coords, const float* verts,
                                      const float* normals, const float* colors, int64_t colors_batch,
                                      const int64_t* faces, const float* cam_centers, int64_t N, int64_t V, int64_t F,
                                      int64_t H, int64_t W, const float* params_host, float* images,
                                      const float* gt_mask, int64_t* counts, void* stream) {
  RECMV_REQUIRE(N >= 0 && V >= 0 && F >= 0 && H > 0 && W > 0, "hard_phong_shade: bad sizes N=%lld V=%lld F=%lld H=%lld W=%lld",
                (long long)N, (long long)V, (long long)F, (long long)H, (long long)W);
  RECMV_REQUIRE(colors_batch == 1 || colors_batch == N, "hard_phong_shade: colors_batch must be 1 or N (got %lld)",
                (long long)colors_batch);
  RECMV_REQUIRE(N < 65536, "hard_phong_shade: at most 65535 images per call");
  RECMV_REQUIRE(H * W < (1ll << 40), "hard_phong_shade: image too large");
  RECMV_REQUIRE(params_host != nullptr, "hard_phong_shade: NULL params_host");
  RECMV_REQUIRE((gt_mask == nullptr) == (counts == nullptr), "hard_phong_shade: gt_mask and counts go together");
  if (N == 0) return RECMV_OK;
  RECMV_REQUIRE(pix_to_face && bary_coords && verts && normals && colors && faces && cam_centers && images,
                "hard_phong_shade: NULL pointer");
  RECMV_REQUIRE(((uintptr_t)images & 15) == 0, "hard_phong_shade: images must be 16-byte aligned");
  ShadeParams prm;
  memcpy(&prm, params_host, sizeof(ShadeParams));
  hipStream_t s = (hipStream_t)stream;
  if (counts != nullptr) RECMV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)N * 2 * sizeof(int64_t), s));
  const int64_t HW = H * W;
  int gx = (int)ceil_div(HW, kShadeBlock);
  const int cap = (int)ceil_div((int64_t)kNumCU * 8, N);
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  dim3 grid((unsigned)gx, (unsigned)N);
  hard_phong_kernel<<<grid, kShadeBlock, 0, s>>>(pix_to_face, bary_coords, verts, normals, colors, colors_batch, faces,
                                                 cam_centers, N, V, F, HW, prm, images, gt_mask,
                                                 (unsigned long long*)counts);
  return check_launch("hard_phong_shade");
}

// Size of the parameter block recmv_hard_phong_shade reads from host memory, in floats.
extern "C" int64_t recmv_hard_phong_params_floats(void) { return (int64_t)(sizeof(ShadeParams) / sizeof(float)); }
