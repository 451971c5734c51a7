// Feature-curve tubes (`Intersect_Free_Curve.curve_to_mesh`, engineer/utils/garment_structure.py:176-274) — gfx950.
//
//   * recmv_curve_tubes: sweeps a ring of J vertices along every closed curve (:214-274), all curves in one launch.
//       tangent       d_i = (c_i - c_{i+1}) / (|.| + 1e-6), the last one c_{S-1} - c_0
//       ring vertex   c_i + radius (n cos t_j + (d x n) sin t_j + d * (d * n) (1 - cos t_j)),  t_j = radians(j (360 / J))
//     The last term is the reference's ELEMENTWISE product d * (d * n), not Rodrigues' d (d . n): kept, the fixtures pin it.
//     Vertices ring-major [S,J]; faces ring by ring, joint by joint: (a_v, b_v, b_v+1), (a_v, b_v+1, a_v+1) with a the ring, b
//     its successor (i+1) % S, indices local to the curve.  One thread per ring vertex writes it and its two faces.
//   * recmv_curve_fit_step: value and gradient of the fit of the curves to ground-truth polylines (:179-212): for every pair
//     (polyline p, curve target_idx[p])
//       w_cham (mean_i min_j |x_i - y_j|^2 + mean_j min_i |x_i - y_j|^2) + w_smooth sum_{k < S-1} (1 - cos(u_k, u_{k+1}))
//     with x = center + dirs init_scale relu(scale) + nx_scale nx and u_k = (x_k - x_{k+1}) / (|.| + 1e-6) (u_{S-1} closes
//     the curve), differentiated by hand with respect to scale and nx_scale.
//     One workgroup per curve: it loops over the pairs that target its curve, in pair order, with the curve and the
//     polyline in LDS (structure of arrays: every lane reads the same candidate, a broadcast).  No float atomics: the
//     polyline -> curve direction stores each polyline point's nearest sample, and every sample then gathers its polyline
//     points in index order; sums run in a fixed order, so the results are bitwise reproducible.  A tie goes to the lowest
//     index (torch.min).  A curve no pair targets gets zero gradients.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)

#include "mesh_device.h"                                   // wave_sum

constexpr int kTubeBlock = 256;
constexpr int kFitBlock = 256;
constexpr int64_t kFitLdsBytes = 64 * 1024 - 64;      // dynamic part: a workgroup's 64 KiB less the static reduction slots

__global__ void __launch_bounds__(kTubeBlock)
curve_tubes_kernel(const float* __restrict__ curves, const float* __restrict__ nx, float radius, int64_t L, int64_t S,
                   int64_t J, float* __restrict__ verts, int64_t* __restrict__ faces) {
  const int64_t total = L * S * J;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t step = 360 / J;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t j = t % J;
    const int64_t i = (t / J) % S;
    const int64_t l = t / (J * S);
    const int64_t i2 = i + 1 < S ? i + 1 : 0;
    const float* c = curves + (l * S + i) * 3;
    const float* c2 = curves + (l * S + i2) * 3;
    const float ex = c[0] - c2[0], ey = c[1] - c2[1], ez = c[2] - c2[2];
    const float inv = sqrtf(ex * ex + ey * ey + ez * ez) + 1e-6f;
    const float dx = ex / inv, dy = ey / inv, dz = ez / inv;
    const float nxx = nx[l * 3 + 0], nxy = nx[l * 3 + 1], nxz = nx[l * 3 + 2];
    const float crx = dy * nxz - dz * nxy, cry = dz * nxx - dx * nxz, crz = dx * nxy - dy * nxx;
    const float dtx = dx * (dx * nxx), dty = dy * (dy * nxy), dtz = dz * (dz * nxz);
    const float ang = (float)((double)(j * step) * (3.14159265358979323846 / 180.0));
    const float ca = cosf(ang), sa = sinf(ang), om = 1.f - ca;
    float* o = verts + t * 3;
    o[0] = c[0] + radius * ((nxx * ca + crx * sa) + dtx * om);
    o[1] = c[1] + radius * ((nxy * ca + cry * sa) + dty * om);
    o[2] = c[2] + radius * ((nxz * ca + crz * sa) + dtz * om);
    const int64_t j2 = j + 1 < J ? j + 1 : 0;
    const int64_t a0 = i * J + j, a1 = i * J + j2, b0 = i2 * J + j, b1 = i2 * J + j2;
    int64_t* f = faces + t * 6;
    f[0] = a0; f[1] = b0; f[2] = b1;
    f[3] = a0; f[4] = b1; f[5] = a1;
  }
}

__device__ __forceinline__ double fit_block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  __syncthreads();                                     // red may still be read from the previous sum
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double t = 0.;
  for (int w = 0; w < kFitBlock / kWave; ++w) t += red[w];
  return t;
}

// gradient of cos(a, b) = a.b / (max(|a|, eps) max(|b|, eps)) with respect to a (F.cosine_similarity, eps = 1e-8)
__device__ __forceinline__ void cos_grad(const float a[3], const float b[3], float g[3]) {
  const float eps = 1e-8f;
  const float la = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const float lb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  const float na = fmaxf(la, eps), nb = fmaxf(lb, eps);
  const float c = (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) / (na * nb);
  const float k = la > eps ? c / (na * na) : 0.f;
#pragma unroll
  for (int q = 0; q < 3; ++q) g[q] = b[q] / (na * nb) - k * a[q];
}

struct FitArgs {
  const float *center, *dirs, *init_scale, *nx, *scale, *nx_scale, *targets;
  const int32_t* target_idx;
  int64_t L, S, P, M;
  float w_cham, w_smooth;
  float *loss, *g_scale, *g_nx_scale;
};

__global__ void __launch_bounds__(kFitBlock) curve_fit_step_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double red[kFitBlock / kWave];
  const int S = (int)a.S, M = (int)a.M;
  const int64_t l = blockIdx.x;
  float* cx = smem;                   // the curve [3,S]
  float* ga = cx + 3 * S;             // dLoss/dx [3,S], every sample owned by the thread i % blockDim
  float* ux = ga + 3 * S;             // unit tangents [3,S]
  float* ge = ux + 3 * S;             // dLoss/d(edge) [3,S]
  float* ty = ge + 3 * S;             // the polyline [3,M]
  int* nn = (int*)(ty + 3 * M);       // nearest sample of every polyline point [M]
  const int tid = threadIdx.x;
  const float n0 = a.nx[l * 3 + 0], n1 = a.nx[l * 3 + 1], n2 = a.nx[l * 3 + 2];
  for (int i = tid; i < S; i += kFitBlock) {
    const int64_t k = l * S + i;
    const float r = a.init_scale[k] * fmaxf(a.scale[k], 0.f), s = a.nx_scale[k];
    cx[i] = (a.center[l * 3 + 0] + a.dirs[k * 3 + 0] * r) + s * n0;
    cx[S + i] = (a.center[l * 3 + 1] + a.dirs[k * 3 + 1] * r) + s * n1;
    cx[2 * S + i] = (a.center[l * 3 + 2] + a.dirs[k * 3 + 2] * r) + s * n2;
    ga[i] = ga[S + i] = ga[2 * S + i] = 0.f;
  }
  for (int64_t p = 0; p < a.P; ++p) {
    const int64_t tgt = a.target_idx[p];
    if (tgt != l) {
      if (l == 0 && tid == 0 && (tgt < 0 || tgt >= a.L)) a.loss[p] = 0.f;       // no curve: nothing to fit
      continue;
    }
    __syncthreads();
    const float* y = a.targets + p * (int64_t)M * 3;
    for (int j = tid; j < M; j += kFitBlock) {
      ty[j] = y[j * 3 + 0];
      ty[M + j] = y[j * 3 + 1];
      ty[2 * M + j] = y[j * 3 + 2];
    }
    __syncthreads();
    double lossA = 0., lossB = 0., lossS = 0.;
    // curve -> polyline
    const float wa = a.w_cham * 2.f / (float)S, wb = a.w_cham * 2.f / (float)M;
    for (int i = tid; i < S; i += kFitBlock) {
      const float x0 = cx[i], x1 = cx[S + i], x2 = cx[2 * S + i];
      float best = __builtin_inff();
      int bj = 0;
      for (int j = 0; j < M; ++j) {
        const float d0 = x0 - ty[j], d1 = x1 - ty[M + j], d2 = x2 - ty[2 * M + j];
        const float d = (d0 * d0 + d1 * d1) + d2 * d2;
        if (d < best) { best = d; bj = j; }
      }
      lossA += (double)best;
      ga[i] += wa * (x0 - ty[bj]);
      ga[S + i] += wa * (x1 - ty[M + bj]);
      ga[2 * S + i] += wa * (x2 - ty[2 * M + bj]);
    }
    // polyline -> curve: nearest sample of every polyline point ...
    for (int j = tid; j < M; j += kFitBlock) {
      const float y0 = ty[j], y1 = ty[M + j], y2 = ty[2 * M + j];
      float best = __builtin_inff();
      int bi = 0;
      for (int i = 0; i < S; ++i) {
        const float d0 = cx[i] - y0, d1 = cx[S + i] - y1, d2 = cx[2 * S + i] - y2;
        const float d = (d0 * d0 + d1 * d1) + d2 * d2;
        if (d < best) { best = d; bi = i; }
      }
      lossB += (double)best;
      nn[j] = bi;
    }
    // ... the unit tangents of the closed curve ...
    for (int i = tid; i < S; i += kFitBlock) {
      const int i2 = i + 1 < S ? i + 1 : 0;
      const float e0 = cx[i] - cx[i2], e1 = cx[S + i] - cx[S + i2], e2 = cx[2 * S + i] - cx[2 * S + i2];
      const float inv = sqrtf((e0 * e0 + e1 * e1) + e2 * e2) + 1e-6f;
      ux[i] = e0 / inv;
      ux[S + i] = e1 / inv;
      ux[2 * S + i] = e2 / inv;
    }
    __syncthreads();
    // ... then every sample gathers the polyline points it is nearest to, in index order
    for (int i = tid; i < S; i += kFitBlock) {
      const float x0 = cx[i], x1 = cx[S + i], x2 = cx[2 * S + i];
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int j = 0; j < M; ++j) {
        if (nn[j] == i) {
          s0 += x0 - ty[j];
          s1 += x1 - ty[M + j];
          s2 += x2 - ty[2 * M + j];
        }
      }
      ga[i] += wb * s0;
      ga[S + i] += wb * s1;
      ga[2 * S + i] += wb * s2;
      // smoothness: term k = i pairs (u_i, u_{i+1}) for i < S-1; u_i also is the second vector of term i-1
      const float u[3] = {ux[i], ux[S + i], ux[2 * S + i]};
      float gu[3] = {0.f, 0.f, 0.f}, g[3];
      if (i + 1 < S) {
        const float v[3] = {ux[i + 1], ux[S + i + 1], ux[2 * S + i + 1]};
        const float lu = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-8f);
        const float lv = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-8f);
        lossS += 1. - (double)((u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) / (lu * lv));
        cos_grad(u, v, g);
#pragma unroll
        for (int q = 0; q < 3; ++q) gu[q] -= g[q];
      }
      if (i >= 1) {
        const float v[3] = {ux[i - 1], ux[S + i - 1], ux[2 * S + i - 1]};
        cos_grad(u, v, g);
#pragma unroll
        for (int q = 0; q < 3; ++q) gu[q] -= g[q];
      }
      // through u = e / (|e| + 1e-6): ge = gu / (r + eps) - e (e . gu) / (r (r + eps)^2)
      const int i2 = i + 1 < S ? i + 1 : 0;
      const float e[3] = {x0 - cx[i2], x1 - cx[S + i2], x2 - cx[2 * S + i2]};
      const float r = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]), re = r + 1e-6f;
      const float dot = e[0] * gu[0] + e[1] * gu[1] + e[2] * gu[2];
      const float k = r > 0.f ? dot / (r * re * re) : 0.f;
#pragma unroll
      for (int q = 0; q < 3; ++q) ge[q * S + i] = a.w_smooth * (gu[q] / re - k * e[q]);
    }
    __syncthreads();
    for (int i = tid; i < S; i += kFitBlock) {
      const int im = i >= 1 ? i - 1 : S - 1;            // edge i leaves x_i, edge i-1 arrives at it
#pragma unroll
      for (int q = 0; q < 3; ++q) ga[q * S + i] += ge[q * S + i] - ge[q * S + im];
    }
    const double tot = fit_block_sum((double)a.w_cham * (lossA / (double)S + lossB / (double)M) + (double)a.w_smooth * lossS, red);
    if (tid == 0) a.loss[p] = (float)tot;
  }
  __syncthreads();
  for (int i = tid; i < S; i += kFitBlock) {
    const int64_t k = l * S + i;
    const float g0 = ga[i], g1 = ga[S + i], g2 = ga[2 * S + i];
    const float gd = (g0 * a.dirs[k * 3 + 0] + g1 * a.dirs[k * 3 + 1]) + g2 * a.dirs[k * 3 + 2];
    a.g_scale[k] = a.scale[k] > 0.f ? gd * a.init_scale[k] : 0.f;
    a.g_nx_scale[k] = (g0 * n0 + g1 * n1) + g2 * n2;
  }
}

inline int64_t fit_lds_bytes(int64_t S, int64_t M) { return (12 * S + 4 * M) * 4; }

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int recmv_curve_tubes(const float* curves, const float* nx, float radius, int64_t L, int64_t S, int64_t J,
                                 float* verts, int64_t* faces, void* stream) {
  RECMV_REQUIRE(L >= 1 && S >= 1 && J >= 1, "curve_tubes: L=%lld, S=%lld, num_joints=%lld must be at least 1", (long long)L,
                (long long)S, (long long)J);
  RECMV_REQUIRE(J <= 360 && 360 % J == 0, "curve_tubes: num_joints=%lld must divide 360", (long long)J);
  RECMV_REQUIRE(L < (1ll << 20) && S < (1ll << 20) && L * S * J < (1ll << 31) / 6,
                "curve_tubes: L=%lld curves of S=%lld samples and %lld joints are too many", (long long)L, (long long)S,
                (long long)J);
  RECMV_REQUIRE(radius == radius, "curve_tubes: radius is NaN");
  RECMV_REQUIRE(curves && nx && verts && faces, "curve_tubes: NULL pointer");
  curve_tubes_kernel<<<stream_grid(L * S * J, kTubeBlock), kTubeBlock, 0, (hipStream_t)stream>>>(curves, nx, radius, L, S, J,
                                                                                               verts, faces);
  return check_launch("curve_tubes");
}

extern "C" int recmv_curve_fit_step(const float* center, const float* dirs, const float* init_scale, const float* nx,
                                    const float* scale, const float* nx_scale, const float* targets,
                                    const int32_t* target_idx, int64_t L, int64_t S, int64_t P, int64_t M, float w_cham,
                                    float w_smooth, float* loss, float* g_scale, float* g_nx_scale, void* stream) {
  RECMV_REQUIRE(L >= 1 && S >= 1 && P >= 1 && M >= 1,
                "curve_fit_step: L=%lld, S=%lld, pairs=%lld, M=%lld must be at least 1", (long long)L, (long long)S,
                (long long)P, (long long)M);
  RECMV_REQUIRE(L <= 65535 && P < (1ll << 20) && S < (1ll << 20) && M < (1ll << 20) && fit_lds_bytes(S, M) <= kFitLdsBytes,
                "curve_fit_step: a curve of S=%lld samples and a polyline of M=%lld points need %lld bytes of LDS, %lld "
                "available (L=%lld, pairs=%lld)", (long long)S, (long long)M, (long long)fit_lds_bytes(S, M),
                (long long)kFitLdsBytes, (long long)L, (long long)P);
  RECMV_REQUIRE(w_cham == w_cham && w_smooth == w_smooth, "curve_fit_step: a weight is NaN");
  RECMV_REQUIRE(center && dirs && init_scale && nx && scale && nx_scale && targets && target_idx && loss && g_scale &&
                    g_nx_scale, "curve_fit_step: NULL pointer");
  FitArgs a{center, dirs, init_scale, nx, scale, nx_scale, targets, target_idx, L, S, P, M, w_cham, w_smooth, loss, g_scale,
            g_nx_scale};
  curve_fit_step_kernel<<<(int)L, kFitBlock, (size_t)fit_lds_bytes(S, M), (hipStream_t)stream>>>(a);
  return check_launch("curve_fit_step");
}
