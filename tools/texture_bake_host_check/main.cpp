// csrc/texture_bake.hip's kernels compiled for the CPU (one lane per wave, one thread per workgroup, one workgroup beyond the
// end) and run under the address and undefined-behaviour sanitizers against plain loops, bit for bit: owner, count and
// barycentrics of the UV rasteriser with 8 and 64 lanes per face, the gutter's index map after 0, 1 and 3 passes and the padded
// image, the interpolation with and without normalisation (C = 1, 3, 4, 16), the transfer from hits on a source mesh, the vertex
// tangents and the normal-map encoding.  The plain rasteriser visits every texel of every face, lowest face first, and applies
// the header's rule with the box as one of its conditions.
// Inputs: a jittered 7 x 9 grid on a 37 x 29 image with a flipped face, a face without area, rows with indices outside [0, V)
// or repeated, a NaN and an infinite coordinate; the same chart partly outside [0,1]^2; one triangle over a 96 x 80 image; a
// 1 x 1 image; and a mesh without faces.
#include "common.h"
#include "recmv_hip.h"
#include <stdlib.h>
#include <utility>
#include <vector>

#include "bake.inc"                                        // csrc/texture_bake.hip up to its entry points
using namespace recmv;

static uint32_t rng_state = 7u;
static double rnd() {                                      // [0, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) * (1. / 16777216.);
}

struct Chart {
  std::vector<float> v, nrm;                               // [V,3]
  std::vector<double> uv;                                  // [V,2]
  std::vector<int64_t> f;                                  // [F,3]
  int64_t V() const { return (int64_t)uv.size() / 2; }
  int64_t F() const { return (int64_t)f.size() / 3; }
};

static Chart grid(int n, int m, double jitter, double lo, double hi) {
  Chart g;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < m; ++j) {
      const bool inner = i > 0 && j > 0 && i < n - 1 && j < m - 1;
      const double x = i + (inner ? jitter * (rnd() - 0.5) : 0.), y = j + (inner ? jitter * (rnd() - 0.5) : 0.);
      g.uv.push_back(lo + (hi - lo) * x / (n - 1));
      g.uv.push_back(lo + (hi - lo) * y / (m - 1));
      const double z = 0.3 * sin(0.9 * x) * cos(0.7 * y);
      g.v.push_back((float)x);
      g.v.push_back((float)y);
      g.v.push_back((float)z);
      const double nx = -0.27 * cos(0.9 * x) * cos(0.7 * y), ny = 0.21 * sin(0.9 * x) * sin(0.7 * y);
      const double len = sqrt(nx * nx + ny * ny + 1.);
      g.nrm.push_back((float)(nx / len));
      g.nrm.push_back((float)(ny / len));
      g.nrm.push_back((float)(1. / len));
    }
  for (int i = 0; i + 1 < n; ++i)
    for (int j = 0; j + 1 < m; ++j) {
      const int64_t a = i * m + j, b = (i + 1) * m + j, c = (i + 1) * m + j + 1, d = i * m + j + 1;
      const int64_t even[6] = {a, b, c, a, c, d}, odd[6] = {a, b, d, b, c, d};
      g.f.insert(g.f.end(), (i + j) % 2 ? odd : even, ((i + j) % 2 ? odd : even) + 6);
    }
  return g;
}

static void flaw(Chart& g) {
  const int64_t V = g.V();
  std::swap(g.f[3 * 4 + 1], g.f[3 * 4 + 2]);               // flipped
  g.f[3 * 7 + 1] = V;                                      // outside [0, V)
  g.f[3 * 9 + 2] = -1;
  g.f[3 * 11 + 1] = g.f[3 * 11];                           // repeated
  const int64_t line[3] = {0, 1, 2};                       // three vertices of one grid line: no area
  g.f.insert(g.f.end(), line, line + 3);
  g.uv[2 * 30] = __builtin_nan("");
  g.uv[2 * 40 + 1] = __builtin_inf();
}

template <class T>
static int64_t differ(const std::vector<T>& a, const std::vector<T>& b) {
  int64_t bad = a.size() != b.size();
  for (size_t k = 0; k < a.size() && k < b.size(); ++k) bad += memcmp(&a[k], &b[k], sizeof(T)) != 0;
  return bad;
}

template <class K, class... A>
static void launch(int64_t n, K kernel, A... args) {       // one thread per workgroup, one workgroup beyond the end
  blockDim.x = 1;
  threadIdx.x = 0;
  gridDim.x = (unsigned)n + 1;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) kernel(args...);
}

// ---- the plain loops
static bool fin(double x) { return x - x == 0.; }

static bool row_ok(const Chart& g, int64_t t) {
  if (t < 0 || t >= g.F()) return false;
  const int64_t* r = &g.f[3 * t];
  for (int k = 0; k < 3; ++k)
    if (r[k] < 0 || r[k] >= g.V()) return false;
  return r[0] != r[1] && r[0] != r[2] && r[1] != r[2];
}

static double p_edge(const Chart& g, int64_t a, int64_t b, double px, double py) {
  const bool turned = a > b;
  if (turned) std::swap(a, b);
  const double e = (g.uv[2 * b] - g.uv[2 * a]) * (py - g.uv[2 * a + 1]) - (g.uv[2 * b + 1] - g.uv[2 * a + 1]) * (px - g.uv[2 * a]);
  return turned ? -e : e;
}

static bool p_area(const Chart& g, int64_t t, double& A) {
  if (!row_ok(g, t)) return false;
  const int64_t* r = &g.f[3 * t];
  A = p_edge(g, r[0], r[1], g.uv[2 * r[2]], g.uv[2 * r[2] + 1]);
  return fin(A) && A != 0.;
}

static bool p_covers(const Chart& g, int64_t t, double A, int64_t x, int64_t y, int64_t H, int64_t W, double* e) {
  const int64_t* r = &g.f[3 * t];
  const double w = (double)W, h = (double)H;
  const double us[3] = {g.uv[2 * r[0]], g.uv[2 * r[1]], g.uv[2 * r[2]]};
  const double vs[3] = {g.uv[2 * r[0] + 1], g.uv[2 * r[1] + 1], g.uv[2 * r[2] + 1]};
  const double umin = std::min(us[0], std::min(us[1], us[2])), umax = std::max(us[0], std::max(us[1], us[2]));
  const double vmin = std::min(vs[0], std::min(vs[1], vs[2])), vmax = std::max(vs[0], std::max(vs[1], vs[2]));
  const bool in_box = (double)x >= floor(umin * w - 0.5) && (double)x <= ceil(umax * w - 0.5) &&
                      (double)y >= floor(h - 0.5 - vmax * h) && (double)y <= ceil(h - 0.5 - vmin * h);
  const double px = ((double)x + 0.5) / w, py = ((double)(H - y) - 0.5) / h;
  const double s = A < 0. ? -1. : 1.;
  e[0] = s * p_edge(g, r[1], r[2], px, py);
  e[1] = s * p_edge(g, r[2], r[0], px, py);
  e[2] = s * p_edge(g, r[0], r[1], px, py);
  return in_box && e[0] >= 0. && e[1] >= 0. && e[2] >= 0.;
}

static void p_raster(const Chart& g, int64_t H, int64_t W, std::vector<int32_t>& face, std::vector<float>& bary,
                     std::vector<int32_t>& count) {
  face.assign(H * W, -1);
  count.assign(H * W, 0);
  bary.assign(3 * H * W, 0.f);
  for (int64_t t = 0; t < g.F(); ++t) {
    double A, e[3];
    if (!p_area(g, t, A)) continue;
    for (int64_t y = 0; y < H; ++y)
      for (int64_t x = 0; x < W; ++x)
        if (p_covers(g, t, A, x, y, H, W, e)) {
          ++count[y * W + x];
          if (face[y * W + x] < 0) {
            face[y * W + x] = (int32_t)t;
            const double S = e[0] + e[1] + e[2];
            for (int k = 0; k < 3; ++k) bary[3 * (y * W + x) + k] = (float)(e[k] / S);
          }
        }
  }
}

static std::vector<int32_t> p_gutter(const std::vector<int32_t>& face, int64_t H, int64_t W, int passes) {
  std::vector<int32_t> src(H * W);
  for (int64_t i = 0; i < H * W; ++i) src[i] = face[i] >= 0 ? (int32_t)i : -1;
  static const int order[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}};      // (dx, dy)
  for (int p = 0; p < passes; ++p) {
    const std::vector<int32_t> prev = src;
    for (int64_t y = 0; y < H; ++y)
      for (int64_t x = 0; x < W; ++x) {
        if (prev[y * W + x] >= 0) continue;
        for (const auto& d : order) {
          const int64_t nx = x + d[0], ny = y + d[1];
          if (nx < 0 || ny < 0 || nx >= W || ny >= H || prev[ny * W + nx] < 0) continue;
          src[y * W + x] = prev[ny * W + nx];
          break;
        }
      }
  }
  return src;
}

static void p_mix(const std::vector<float>& attr, int C, const int64_t* r, const float* b, bool normalise, float* out) {
  for (int c = 0; c < C; ++c) out[c] = b[0] * attr[r[0] * C + c] + b[1] * attr[r[1] * C + c] + b[2] * attr[r[2] * C + c];
  if (!normalise) return;
  const double x = out[0], y = out[1], z = out[2], len = sqrt(x * x + y * y + z * z);
  if (!(len > 0. && fin(len))) return;
  out[0] = (float)(x / len);
  out[1] = (float)(y / len);
  out[2] = (float)(z / len);
}

static double p_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

static void p_cross(const double* u, const double* w, double* n) {
  n[0] = u[1] * w[2] - u[2] * w[1];
  n[1] = u[2] * w[0] - u[0] * w[2];
  n[2] = u[0] * w[1] - u[1] * w[0];
}

static void p_tangents(const Chart& g, const std::vector<std::vector<int64_t>>& fans, std::vector<float>& out) {
  out.assign(4 * g.V(), 0.f);
  for (int64_t i = 0; i < g.V(); ++i) {
    double T[3] = {0., 0., 0.}, B[3] = {0., 0., 0.};
    for (int64_t t : fans[i]) {
      double A;
      if (!p_area(g, t, A)) continue;
      const int64_t* r = &g.f[3 * t];
      double e1[3], e2[3], n[3];
      for (int c = 0; c < 3; ++c) {
        e1[c] = (double)g.v[3 * r[1] + c] - (double)g.v[3 * r[0] + c];
        e2[c] = (double)g.v[3 * r[2] + c] - (double)g.v[3 * r[0] + c];
      }
      p_cross(e1, e2, n);
      const double area = 0.5 * sqrt(p_dot(n, n));
      if (!(area > 0. && fin(area))) continue;
      const double du1 = g.uv[2 * r[1]] - g.uv[2 * r[0]], dv1 = g.uv[2 * r[1] + 1] - g.uv[2 * r[0] + 1];
      const double du2 = g.uv[2 * r[2]] - g.uv[2 * r[0]], dv2 = g.uv[2 * r[2] + 1] - g.uv[2 * r[0] + 1];
      const double w = area / A;
      for (int c = 0; c < 3; ++c) {
        T[c] += w * (e1[c] * dv2 - e2[c] * dv1);
        B[c] += w * (e2[c] * du1 - e1[c] * du2);
      }
    }
    const double n[3] = {g.nrm[3 * i], g.nrm[3 * i + 1], g.nrm[3 * i + 2]};
    const double nt = p_dot(n, T);
    double t[3] = {T[0] - n[0] * nt, T[1] - n[1] * nt, T[2] - n[2] * nt}, c[3];
    const double len = sqrt(p_dot(t, t));
    out[4 * i + 3] = 1.f;
    if (!(len > 0. && fin(len))) continue;
    for (int k = 0; k < 3; ++k) t[k] = t[k] / len;
    p_cross(n, t, c);
    for (int k = 0; k < 3; ++k) out[4 * i + k] = (float)t[k];
    out[4 * i + 3] = p_dot(c, B) < 0. ? -1.f : 1.f;
  }
}

// ---- one chart on one image
static int64_t check(const char* what, Chart g, int64_t H, int64_t W) {
  const int64_t V = g.V(), F = g.F(), T = H * W;
  std::vector<int32_t> want_face, want_count;
  std::vector<float> want_bary;
  p_raster(g, H, W, want_face, want_bary, want_count);
  int64_t bad_raster = 0, covered = 0, shared = 0;
  std::vector<int32_t> face, count;
  std::vector<float> bary;
  for (int lanes : {8, 64}) {
    face.assign(T, 123);
    count.assign(T, 123);
    bary.assign(3 * T, -1.f);
    launch(T, bake_clear_kernel, T, face.data(), count.data());
    launch(F * lanes, bake_scatter_kernel, g.uv.data(), V, g.f.data(), F, H, W, lanes, face.data(), count.data());
    launch(T, bake_resolve_kernel, g.uv.data(), V, g.f.data(), F, H, W, face.data(), bary.data());
    bad_raster += differ(face, want_face) + differ(count, want_count) + differ(bary, want_bary);
  }
  for (int64_t i = 0; i < T; ++i) {
    covered += face[i] >= 0;
    shared += count[i] > 1;
  }

  int64_t bad_gutter = 0;
  std::vector<int32_t> src;
  for (int passes : {0, 1, 3}) {
    std::vector<int32_t> buf[2] = {std::vector<int32_t>(T, 77), std::vector<int32_t>(T, 77)};
    int cur = passes % 2;
    launch(T, bake_gutter_init_kernel, face.data(), T, buf[cur].data());
    for (int k = 0; k < passes; ++k, cur ^= 1) launch(T, bake_gutter_pass_kernel, buf[cur].data(), H, W, buf[cur ^ 1].data());
    bad_gutter += cur != 0;
    bad_gutter += differ(buf[0], p_gutter(face, H, W, passes));
    src = buf[0];
  }

  // attributes: the mesh's own, C = 1, 3, 4, 16
  int64_t bad_mix = 0;
  for (int C : {1, 3, 4, 16})
    for (int normalise = 0; normalise < (C >= 3 ? 2 : 1); ++normalise) {
      std::vector<float> attr(V * C), out(T * C, -1.f), want(T * C, 0.f), padded(T * C, -1.f), want_pad(T * C, 0.f);
      for (auto& a : attr) a = (float)(2. * rnd() - 1.);
      if (V > 3 && C >= 3) attr[3 * C] = attr[3 * C + 1] = attr[3 * C + 2] = 0.f;
      launch(T, bake_interpolate_kernel, face.data(), bary.data(), T, g.f.data(), F, attr.data(), V, C, normalise, out.data());
      for (int64_t i = 0; i < T; ++i)
        if (row_ok(g, want_face[i])) p_mix(attr, C, &g.f[3 * want_face[i]], &want_bary[3 * i], normalise != 0, &want[i * C]);
      launch(T, bake_pad_kernel, out.data(), src.data(), T, C, padded.data());
      for (int64_t i = 0; i < T; ++i)
        for (int c = 0; c < C; ++c) want_pad[i * C + c] = src[i] >= 0 ? want[(int64_t)src[i] * C + c] : 0.f;
      bad_mix += differ(out, want) + differ(padded, want_pad);
    }

  // transfer: hits on the chart's own mesh, with ids that are no face and a face without area among them
  int64_t bad_transfer = 0;
  {
    const int64_t P = 300, C = 3;
    std::vector<int64_t> hit(P);
    std::vector<float> point(3 * P), attr(V * C), tb(3 * P, -1.f), out(P * C, -1.f), want_b(3 * P, 0.f), want(P * C, 0.f);
    for (auto& a : attr) a = (float)(2. * rnd() - 1.);
    for (int64_t i = 0; i < P; ++i) {
      hit[i] = i % 17 == 0 ? -1 : (i % 19 == 0 ? F : (i % 23 == 0 ? F - 1 : (int64_t)(rnd() * F)));
      for (int c = 0; c < 3; ++c) point[3 * i + c] = (float)(8. * rnd());
    }
    launch(P, bake_transfer_kernel, hit.data(), point.data(), P, g.v.data(), V, g.f.data(), F, attr.data(), (int)C, 1, tb.data(),
           out.data());
    for (int64_t i = 0; i < P; ++i) {
      if (!row_ok(g, hit[i])) continue;
      const int64_t* r = &g.f[3 * hit[i]];
      double e1[3], e2[3], d[3];
      for (int c = 0; c < 3; ++c) {
        e1[c] = (double)g.v[3 * r[1] + c] - (double)g.v[3 * r[0] + c];
        e2[c] = (double)g.v[3 * r[2] + c] - (double)g.v[3 * r[0] + c];
        d[c] = (double)point[3 * i + c] - (double)g.v[3 * r[0] + c];
      }
      const double d11 = p_dot(e1, e1), d12 = p_dot(e1, e2), d22 = p_dot(e2, e2), r1 = p_dot(d, e1), r2 = p_dot(d, e2);
      const double det = d11 * d22 - d12 * d12;
      double b1 = 0., b2 = 0.;
      if (det > 0. && fin(det)) {
        b1 = (d22 * r1 - d12 * r2) / det;
        b2 = (d11 * r2 - d12 * r1) / det;
      }
      want_b[3 * i] = (float)(1. - b1 - b2);
      want_b[3 * i + 1] = (float)b1;
      want_b[3 * i + 2] = (float)b2;
      p_mix(attr, (int)C, r, &want_b[3 * i], true, &want[i * C]);
    }
    bad_transfer += differ(tb, want_b) + differ(out, want);
  }

  // tangents over the adjacency (corner 1, 2, 0, stable by vertex), one row with codes that must not count; then the encoding
  int64_t bad_tangent = 0;
  {
    std::vector<std::vector<int64_t>> fans(V);
    std::vector<std::vector<int32_t>> rows(V);
    const int corner[3] = {1, 2, 0};
    for (int c : corner)
      for (int64_t t = 0; t < F; ++t) {
        const int64_t i = g.f[3 * t + c];
        if (i < 0 || i >= V) continue;
        fans[i].push_back(t);
        rows[i].push_back((int32_t)(3 * t + c));
      }
    int64_t total = 0;
    for (const auto& r : rows) total += (int64_t)r.size();
    if (V > 5 && total + 2 <= 3 * F) {                     // (the flawed chart dropped two corners: the table stays at 3 F codes)
      rows[5].push_back(-4);
      rows[5].push_back((int32_t)(3 * F));
    }
    std::vector<int32_t> off(V + 1, 0), codes;
    for (int64_t i = 0; i < V; ++i) {
      codes.insert(codes.end(), rows[i].begin(), rows[i].end());
      off[i + 1] = (int32_t)codes.size();
    }
    codes.resize(3 * F + 2, -9);                           // never read: the rows end at 3 F codes
    std::vector<float> tan(4 * V, -7.f), want;
    p_tangents(g, fans, want);
    launch(V, bake_vertex_tangents_kernel, g.v.data(), g.uv.data(), g.nrm.data(), V, g.f.data(), F, off.data(), codes.data(),
           tan.data());
    bad_tangent += differ(tan, want);
    std::vector<float> fn(3 * T), ft(4 * T), N(3 * T), enc(3 * T, -1.f), want_enc(3 * T, 0.f);
    for (auto& a : fn) a = (float)(2. * rnd() - 1.);
    for (auto& a : ft) a = (float)(2. * rnd() - 1.);
    for (auto& a : N) a = (float)(2. * rnd() - 1.);
    launch(T, bake_encode_normal_kernel, face.data(), N.data(), fn.data(), ft.data(), T, enc.data());
    for (int64_t i = 0; i < T; ++i) {
      if (want_face[i] < 0) continue;
      const double n[3] = {fn[3 * i], fn[3 * i + 1], fn[3 * i + 2]};
      const double NN[3] = {N[3 * i], N[3 * i + 1], N[3 * i + 2]}, w = ft[4 * i + 3] < 0.f ? -1. : 1.;
      double t[3] = {ft[4 * i], ft[4 * i + 1], ft[4 * i + 2]}, b[3];
      const double nt = p_dot(n, t);
      const double o[3] = {t[0] - n[0] * nt, t[1] - n[1] * nt, t[2] - n[2] * nt};
      const double len = sqrt(p_dot(o, o));
      if (len > 0. && fin(len))
        for (int k = 0; k < 3; ++k) t[k] = o[k] / len;
      p_cross(n, t, b);
      want_enc[3 * i] = (float)(0.5 + 0.5 * p_dot(NN, t));
      want_enc[3 * i + 1] = (float)(0.5 + 0.5 * (w * p_dot(NN, b)));
      want_enc[3 * i + 2] = (float)(0.5 + 0.5 * p_dot(NN, n));
    }
    bad_tangent += differ(enc, want_enc);
  }

  const int64_t bad = bad_raster + bad_gutter + bad_mix + bad_transfer + bad_tangent;
  printf("%s: %lld vertices, %lld faces, %lld x %lld texels, %lld covered, %lld shared; raster %lld, gutter %lld, attributes %lld, "
         "transfer %lld, tangents %lld -> %lld mismatches\n", what, (long long)V, (long long)F, (long long)H, (long long)W,
         (long long)covered, (long long)shared, (long long)bad_raster, (long long)bad_gutter, (long long)bad_mix,
         (long long)bad_transfer, (long long)bad_tangent, (long long)bad);
  return bad;
}

int main() {
  int64_t bad = 0;
  Chart a = grid(7, 9, 0.6, 0.06, 0.94);
  flaw(a);
  bad += check("a jittered 7 x 9 grid with flawed faces and coordinates", a, 37, 29);
  Chart b = grid(7, 9, 0.6, -0.2, 1.15);
  bad += check("the grid partly outside the unit square", b, 16, 24);
  Chart c = grid(2, 2, 0., 0.02, 0.97);
  c.f.resize(3);
  bad += check("one triangle over 96 x 80 texels", c, 96, 80);
  bad += check("a 1 x 1 image", grid(3, 3, 0., 0., 1.), 1, 1);
  Chart e = grid(3, 3, 0., 0., 1.);
  e.f.clear();
  bad += check("a mesh without faces", e, 5, 4);
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad ? 1 : 0;
}
