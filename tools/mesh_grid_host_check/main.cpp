// Host check of csrc/mesh_grid.hip: the count, fill and one-lane query kernels compiled for the CPU (tools/host_check/common.h stands in for
// csrc/common.h: one lane per wave, kernels called as functions) and compared bit for bit with a brute force over the faces,
// on meshes and grids chosen to reach every branch.  kernels.inc is csrc/mesh_grid.hip up to its `using namespace recmv;` line
// (tests/host_check.py builds it; tests/test_mesh_metrics_cpu.py runs it).
#include "kernels.inc"
#include <vector>
#include <random>
using namespace recmv;
static std::mt19937 rng(7);
static float U(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }
struct Mesh { std::vector<float> v; std::vector<int64_t> f; };
static void brute(const Mesh& m, const float* p, int64_t& face, float& d2, float pt[3]) {
  int64_t V = m.v.size() / 3, F = m.f.size() / 3; float best = __builtin_inff(); int64_t bi = -1;
  for (int64_t k = 0; k < F; ++k) { Tri q; if (!load_tri(m.v.data(), m.f.data(), V, k, q)) continue; float s, t;
    float d = closest_st(p[0], p[1], p[2], q, s, t); if (d < best) { best = d; bi = k; } }
  face = bi; d2 = best;
  if (bi >= 0) { Tri q; load_tri(m.v.data(), m.f.data(), V, bi, q); float s, t; closest_st(p[0], p[1], p[2], q, s, t);
    pt[0] = q.ax + s * q.bx + t * q.cx; pt[1] = q.ay + s * q.by + t * q.cy; pt[2] = q.az + s * q.bz + t * q.cz; }
}
static int run(const char* name, const Mesh& m, std::vector<float> p, int nx, int ny, int nz, float h_force) {
  int64_t V = m.v.size() / 3, F = m.f.size() / 3, P = p.size() / 3;
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (int64_t i = 0; i < V; ++i) for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], m.v[3 * i + c]); hi[c] = fmaxf(hi[c], m.v[3 * i + c]); }
  float h = h_force;
  if (h <= 0) { h = 1e-30f; int n[3] = {nx, ny, nz}; for (int c = 0; c < 3; ++c) h = fmaxf(h, (hi[c] - lo[c]) / n[c] * 1.000001f); }
  Grid g{lo[0], lo[1], lo[2], h, 1.f / h, nx, ny, nz};
  // lattice / corner queries
  for (int i = 0; i < 60; ++i) { int a = rng() % (nx + 1), b = rng() % (ny + 1), c = rng() % (nz + 1);
    p.push_back(lo[0] + a * h); p.push_back(lo[1] + b * h); p.push_back(lo[2] + c * h); }
  P = p.size() / 3;
  int64_t cells = (int64_t)nx * ny * nz;
  std::vector<int32_t> counts(cells, 0), offsets(cells + 1, 0), cursor(cells, 0);
  unsigned long long total = 0;
  blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0};
  grid_count_kernel(m.v.data(), V, m.f.data(), F, g, counts.data(), &total);
  int64_t sum = 0; for (int64_t c = 0; c < cells; ++c) { offsets[c] = (int32_t)sum; cursor[c] = (int32_t)sum; sum += counts[c]; }
  offsets[cells] = (int32_t)sum;
  if ((unsigned long long)sum != total) { printf("%s: total %llu != sum %lld\n", name, total, (long long)sum); return 1; }
  std::vector<int32_t> entries(std::max<int64_t>(sum, 1), -7);
  std::vector<float4> tris(3 * F);
  grid_fill_kernel(m.v.data(), V, m.f.data(), F, g, offsets.data(), cursor.data(), entries.data(), sum, tris.data());
  for (int64_t c = 0; c < cells; ++c) if (cursor[c] != offsets[c + 1]) { printf("%s: cursor mismatch\n", name); return 1; }
  for (int64_t e = 0; e < sum; ++e) if (entries[e] < 0 || entries[e] >= F) { printf("%s: bad entry\n", name); return 1; }
  std::vector<int64_t> face(P); std::vector<float> point(3 * P), dist2(P);
  int bad = 0;
  for (int64_t s = 0; s < P; ++s) {
    blockIdx.x = (unsigned)(s / 256); threadIdx.x = (unsigned)(s % 256);
    closest_point_grid_kernel<1>(p.data(), P, nullptr, tris.data(), F, GridView{g, offsets.data(), entries.data(), sum}, face.data(), point.data(), dist2.data());
    int64_t bf; float bd; float bp[3] = {0, 0, 0};
    brute(m, &p[3 * s], bf, bd, bp);
    bool ok = bf == face[s] && memcmp(&bd, &dist2[s], 4) == 0 && (bf < 0 || memcmp(bp, &point[3 * s], 12) == 0);
    if (!ok && bad++ < 5) printf("%s: query %lld (%g %g %g): grid face %lld d2 %.9g, brute face %lld d2 %.9g\n", name, (long long)s,
                                 p[3 * s], p[3 * s + 1], p[3 * s + 2], (long long)face[s], dist2[s], (long long)bf, bd);
  }
  printf("%s: dims %dx%dx%d h %g, %lld faces, %lld entries, %lld queries, %d mismatches\n", name, nx, ny, nz, h, (long long)F,
         (long long)sum, (long long)P, bad);
  return bad != 0;
}
int main() {
  int rc = 0;
  // a bumpy sphere of random small triangles, duplicates, degenerate and invalid faces, one huge triangle
  Mesh m;
  int nv = 400;
  for (int i = 0; i < nv; ++i) { float x = U(-1, 1), y = U(-1, 1), z = U(-1, 1), r = sqrtf(x * x + y * y + z * z) + 1e-3f, s = 0.5f * (1 + 0.05f * sinf(5 * x));
    m.v.insert(m.v.end(), {s * x / r, s * y / r, s * z / r}); }
  for (int i = 0; i < 900; ++i) {   // faces between near vertices
    int a = rng() % nv, b = a, c = a; float bb = 1e9f, cc = 1e9f;
    for (int j = 0; j < nv; ++j) if (j != a) { float d = 0; for (int k = 0; k < 3; ++k) d += (m.v[3 * a + k] - m.v[3 * j + k]) * (m.v[3 * a + k] - m.v[3 * j + k]);
      d *= U(0.5f, 2.f); if (d < bb) { cc = bb; c = b; bb = d; b = j; } else if (d < cc) { cc = d; c = j; } }
    m.f.insert(m.f.end(), {a, b, c}); }
  for (int i = 0; i < 10; ++i) for (int k = 0; k < 3; ++k) m.f.push_back(m.f[3 * (i * 7) + k]);           // duplicates
  m.f.insert(m.f.end(), {5, 5, 9, 7, 11, 11, 4, 4, 4, nv, 1, 2, -1, 2, 3, 0, 1, (int64_t)nv + 5});       // degenerate, invalid
  std::vector<float> p;
  for (int i = 0; i < 1500; ++i) { p.insert(p.end(), {U(-0.7f, 0.7f), U(-0.7f, 0.7f), U(-0.7f, 0.7f)}); }
  for (int i = 0; i < nv; ++i) for (int k = 0; k < 3; ++k) p.push_back(m.v[3 * i + k]);                    // on vertices
  for (int i = 0; i < 200; ++i) { int64_t a = m.f[3 * i], b = m.f[3 * i + 1]; for (int k = 0; k < 3; ++k) p.push_back(0.5f * (m.v[3 * a + k] + m.v[3 * b + k])); }
  for (int i = 0; i < 14; ++i) { float d[3] = {0, 0, 0}; if (i < 6) d[i % 3] = i < 3 ? 1 : -1; else { d[0] = (i & 1) ? 1 : -1; d[1] = (i & 2) ? 1 : -1; d[2] = (i & 4) ? 1 : -1; }
    for (int k = 0; k < 3; ++k) p.push_back(17.f * d[k]); }
  rc |= run("sphere 9^3", m, p, 9, 9, 9, 0);
  rc |= run("sphere 1^3", m, p, 1, 1, 1, 0);
  rc |= run("sphere 31x2x7", m, p, 31, 2, 7, 0);
  rc |= run("sphere 40^3 small h (grid does not cover)", m, p, 40, 40, 40, 0.01f);
  Mesh two; two.v = m.v; two.f.assign(m.f.begin(), m.f.begin() + 6);
  std::vector<float> pf(p.begin(), p.begin() + 900);
  rc |= run("two faces 40^3", two, pf, 40, 40, 40, 0);
  Mesh huge = m; huge.v.insert(huge.v.end(), {-1, -1, -1, 1, -1, 1, -1, 1, 1}); huge.f.insert(huge.f.begin(), {nv, nv + 1, nv + 2}); huge.f.insert(huge.f.end(), {nv, nv + 1, nv + 2});
  rc |= run("huge 12^3", huge, p, 12, 12, 12, 0);
  Mesh flat; for (int i = 0; i <= 8; ++i) for (int j = 0; j <= 8; ++j) flat.v.insert(flat.v.end(), {j / 8.f + U(-.01f, .01f), i / 8.f + U(-.01f, .01f), 0.25f});
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { int64_t a = i * 9 + j; flat.f.insert(flat.f.end(), {a, a + 1, a + 9, a + 1, a + 10, a + 9}); }
  rc |= run("planar 7x7x1", flat, p, 7, 7, 1, 0);
  printf(rc ? "FAILED\n" : "all ok\n");
  return rc;
}
