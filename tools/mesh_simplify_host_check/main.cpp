// Host check of csrc/mesh_simplify.hip: its three kernels compiled for the CPU (the stand-in common.h of
// tools/host_check: kernels called as functions, one thread after the other) under the host's sanitizers.
// simplify.inc is csrc/mesh_simplify.hip up to its `using namespace recmv;` line (tests/host_check.py builds it;
// tests/test_mesh_simplify_cpu.py runs it).
//   * quadrics against a plain long-double loop: fans of 0, 1, 63, 64, 65 and 257 faces at one vertex, a bumpy grid with its
//     border, invalid faces and a NaN corner.
//   * placement and cost on quadrics of rank 0, 1 (a flat patch), 2 (a straight crease) and 3 built by hand, on E = 0, 1, 255,
//     256, 257 edges of the bumpy grid, on invalid edges: finite outputs, the cost no larger than at a, b and the midpoint,
//     the codes obeyed.
//   * the flip test against a plain long-double loop on random collapses and on hand cases with integer coordinates.
//   * tables filled with random numbers must stay inside the arrays (the sanitizers watch).
#include "common.h"
#include "simplify.inc"
#include <array>
#include <cmath>
#include <random>
#include <vector>
using namespace recmv;
typedef long double ld;
static std::mt19937 rng(41);

static void launch_shape() { blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0}; }

struct Mesh {
  std::vector<float> v;
  std::vector<int64_t> f;
  int64_t V() const { return (int64_t)v.size() / 3; }
  int64_t F() const { return (int64_t)f.size() / 3; }
};

static bool valid(const Mesh& m, int64_t k) {
  const int64_t* r = &m.f[3 * k];
  for (int t = 0; t < 3; ++t) if (r[t] < 0 || r[t] >= m.V()) return false;
  return r[0] != r[1] && r[0] != r[2] && r[1] != r[2];
}

struct Tables {
  std::vector<int64_t> vf_off, vf_idx, border, vb_off, vb_idx;
};

// vertex -> faces ascending; the border (a < b, face) in edge order; vertex -> border rows ascending
static Tables tables(const Mesh& m) {
  Tables t;
  const int64_t V = m.V(), F = m.F();
  std::vector<std::vector<int64_t>> vf(V), vb(V);
  std::vector<std::array<int64_t, 3>> half;                // (lo, hi, face)
  for (int64_t k = 0; k < F; ++k) {
    if (!valid(m, k)) continue;
    for (int c = 0; c < 3; ++c) {
      vf[m.f[3 * k + c]].push_back(k);
      const int64_t a = m.f[3 * k + c], b = m.f[3 * k + (c + 1) % 3];
      half.push_back({std::min(a, b), std::max(a, b), k});
    }
  }
  std::sort(half.begin(), half.end());
  for (size_t i = 0; i < half.size();) {
    size_t j = i;
    while (j < half.size() && half[j][0] == half[i][0] && half[j][1] == half[i][1]) ++j;
    if (j - i == 1) {
      const int64_t r = (int64_t)t.border.size() / 3;
      t.border.insert(t.border.end(), {half[i][0], half[i][1], half[i][2]});
      vb[half[i][0]].push_back(r);
      vb[half[i][1]].push_back(r);
    }
    i = j;
  }
  t.vf_off.assign(V + 1, 0);
  t.vb_off.assign(V + 1, 0);
  for (int64_t i = 0; i < V; ++i) {
    t.vf_idx.insert(t.vf_idx.end(), vf[i].begin(), vf[i].end());
    t.vb_idx.insert(t.vb_idx.end(), vb[i].begin(), vb[i].end());
    t.vf_off[i + 1] = (int64_t)t.vf_idx.size();
    t.vb_off[i + 1] = (int64_t)t.vb_idx.size();
  }
  return t;
}

static const int64_t* data_or_null(const std::vector<int64_t>& x) { return x.empty() ? nullptr : x.data(); }

static std::vector<double> run_quadrics(const Mesh& m, const Tables& t, double bw, int32_t* invalid) {
  std::vector<double> Q(std::max<int64_t>(m.V(), 1) * 11, -7.);
  int32_t counts = 0;
  launch_shape();
  vertex_quadrics_kernel(m.v.data(), m.V(), m.f.data(), m.F(), t.vf_off.data(), data_or_null(t.vf_idx), (int64_t)t.vf_idx.size(),
                         data_or_null(t.border), (int64_t)t.border.size() / 3, t.vb_off.data(), data_or_null(t.vb_idx),
                         (int64_t)t.vb_idx.size(), bw, Q.data(), &counts);
  *invalid = counts;
  return Q;
}

// the plain loop in long double; A gets the sums of the absolute terms
static void plain_quadrics(const Mesh& m, const Tables& t, double bw, std::vector<ld>& Q, std::vector<ld>& A) {
  const int64_t V = m.V();
  Q.assign(V * 11, 0);
  A.assign(V * 11, 0);
  auto P = [&](int64_t i, int c) { return (ld)m.v[3 * i + c]; };
  // pb: the plane with every entry's magnitude and its offset replaced by sum |n_i a_i| (what the offset's rounding scales with)
  auto add = [&](int64_t i, ld w, const ld* p, const ld* pb, bool weight) {
    int k = 0;
    for (int r = 0; r < 4; ++r)
      for (int c = r; c < 4; ++c, ++k) { Q[i * 11 + k] += w * p[r] * p[c]; A[i * 11 + k] += w * pb[r] * pb[c]; }
    if (weight) { Q[i * 11 + 10] += w; A[i * 11 + 10] += w; }
  };
  auto normal = [&](int64_t k, ld* n) {
    const int64_t a = m.f[3 * k], b = m.f[3 * k + 1], c = m.f[3 * k + 2];
    const ld u[3] = {P(b, 0) - P(a, 0), P(b, 1) - P(a, 1), P(b, 2) - P(a, 2)}, w[3] = {P(c, 0) - P(a, 0), P(c, 1) - P(a, 1), P(c, 2) - P(a, 2)};
    n[0] = u[1] * w[2] - u[2] * w[1]; n[1] = u[2] * w[0] - u[0] * w[2]; n[2] = u[0] * w[1] - u[1] * w[0];
  };
  for (int64_t i = 0; i < V; ++i) {
    for (int64_t j = t.vf_off[i]; j < t.vf_off[i + 1]; ++j) {
      const int64_t k = t.vf_idx[j];
      ld n[3];
      normal(k, n);
      const ld len = sqrtl(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      if (!(len > 0 && std::isfinite((double)len))) continue;
      const int64_t a = m.f[3 * k];
      const ld p[4] = {n[0] / len, n[1] / len, n[2] / len, -(n[0] * P(a, 0) + n[1] * P(a, 1) + n[2] * P(a, 2)) / len};
      const ld pb[4] = {fabsl(p[0]), fabsl(p[1]), fabsl(p[2]), (fabsl(n[0] * P(a, 0)) + fabsl(n[1] * P(a, 1)) + fabsl(n[2] * P(a, 2))) / len};
      add(i, len / 2, p, pb, true);
    }
    for (int64_t j = t.vb_off[i]; j < t.vb_off[i + 1]; ++j) {
      const int64_t* be = &t.border[3 * t.vb_idx[j]];
      ld n[3];
      normal(be[2], n);
      const ld e[3] = {P(be[1], 0) - P(be[0], 0), P(be[1], 1) - P(be[0], 1), P(be[1], 2) - P(be[0], 2)};
      const ld mm[3] = {n[1] * e[2] - n[2] * e[1], n[2] * e[0] - n[0] * e[2], n[0] * e[1] - n[1] * e[0]};
      const ld len = sqrtl(mm[0] * mm[0] + mm[1] * mm[1] + mm[2] * mm[2]);
      if (!(len > 0 && std::isfinite((double)len))) continue;
      const ld p[4] = {mm[0] / len, mm[1] / len, mm[2] / len, -(mm[0] * P(be[0], 0) + mm[1] * P(be[0], 1) + mm[2] * P(be[0], 2)) / len};
      const ld pb[4] = {fabsl(p[0]), fabsl(p[1]), fabsl(p[2]),
                        (fabsl(mm[0] * P(be[0], 0)) + fabsl(mm[1] * P(be[0], 1)) + fabsl(mm[2] * P(be[0], 2))) / len};
      add(i, (ld)bw * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), p, pb, false);
    }
  }
}

static int check_quadrics(const char* name, const Mesh& m, double bw, int64_t want_invalid, int64_t longest_row) {
  const Tables t = tables(m);
  int32_t invalid = -1;
  const std::vector<double> Q = run_quadrics(m, t, bw, &invalid);
  std::vector<ld> P, A;
  plain_quadrics(m, t, bw, P, A);
  int64_t bad = 0, nonfinite = 0, row = 0;
  for (int64_t i = 0; i < m.V(); ++i) {
    row = std::max(row, t.vf_off[i + 1] - t.vf_off[i]);
    const ld n = (ld)(t.vf_off[i + 1] - t.vf_off[i] + t.vb_off[i + 1] - t.vb_off[i] + 40);
    for (int k = 0; k < 11; ++k) {
      const double q = Q[i * 11 + k];
      if (!std::isfinite(q)) { ++nonfinite; continue; }
      if (fabsl((ld)q - P[i * 11 + k]) > n * 1.2e-16L * A[i * 11 + k]) ++bad;      // gamma_n on the absolute terms
    }
  }
  const bool ok = bad == 0 && nonfinite == 0 && invalid == want_invalid && row == longest_row;
  printf("quadrics %s: %lld vertices, %lld faces, %lld border edges, longest row %lld, %d invalid, %lld not finite, %lld mismatches%s\n",
         name, (long long)m.V(), (long long)m.F(), (long long)t.border.size() / 3, (long long)row, invalid, (long long)nonfinite,
         (long long)bad, ok ? "" : "  <-- WRONG");
  return ok ? 0 : 1;
}

// n triangles round vertex 0 (an open fan for n < 3), the rim on a bumpy circle
static Mesh fan(int64_t n) {
  Mesh m;
  std::uniform_real_distribution<float> U(-0.1f, 0.1f);
  m.v = {0.f, 0.f, 0.3f};
  for (int64_t i = 0; i <= n; ++i) {
    const double a = 2 * M_PI * (double)i / (double)(n + 1);
    m.v.insert(m.v.end(), {(float)cos(a), (float)sin(a), U(rng)});
  }
  for (int64_t i = 0; i < n; ++i) m.f.insert(m.f.end(), {0, 1 + i, 2 + i});
  return m;
}

static Mesh bumpy_grid(int n) {
  Mesh m;
  std::uniform_real_distribution<float> U(-0.2f, 0.2f);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) m.v.insert(m.v.end(), {(float)i + U(rng), (float)j + U(rng), U(rng)});
  for (int j = 0; j + 1 < n; ++j)
    for (int i = 0; i + 1 < n; ++i) {
      const int64_t a = j * n + i;
      m.f.insert(m.f.end(), {a, a + 1, a + n + 1, a, a + n + 1, a + n});
    }
  return m;
}

static std::vector<int64_t> edges_of(const Mesh& m) {
  std::vector<std::pair<int64_t, int64_t>> e;
  for (int64_t k = 0; k < m.F(); ++k)
    if (valid(m, k))
      for (int c = 0; c < 3; ++c) {
        const int64_t a = m.f[3 * k + c], b = m.f[3 * k + (c + 1) % 3];
        e.push_back({std::min(a, b), std::max(a, b)});
      }
  std::sort(e.begin(), e.end());
  e.erase(std::unique(e.begin(), e.end()), e.end());
  std::vector<int64_t> out;
  for (auto& p : e) out.insert(out.end(), {p.first, p.second});
  return out;
}

static ld plain_cost(const double* q, const float* p) {
  const ld x = p[0], y = p[1], z = p[2];
  const ld c = q[0] * x * x + 2 * q[1] * x * y + 2 * q[2] * x * z + 2 * q[3] * x + q[4] * y * y + 2 * q[5] * y * z + 2 * q[6] * y + q[7] * z * z +
               2 * q[8] * z + q[9];
  return c > 0 ? c : 0;
}

static ld abs_cost(const double* q, const float* p) {
  const ld x = fabsl(p[0]), y = fabsl(p[1]), z = fabsl(p[2]);
  return fabs(q[0]) * x * x + 2 * fabs(q[1]) * x * y + 2 * fabs(q[2]) * x * z + 2 * fabs(q[3]) * x + fabs(q[4]) * y * y + 2 * fabs(q[5]) * y * z +
         2 * fabs(q[6]) * y + fabs(q[7]) * z * z + 2 * fabs(q[8]) * z + fabs(q[9]);
}

// the cost kernel on the first E edges: every output finite, the codes obeyed, the cost the plain one at pos and no larger than
// at a, b and the midpoint
static int check_cost(const char* name, const std::vector<double>& Q, const std::vector<float>& v, const std::vector<int64_t>& edges,
                      int64_t E, double reach, int64_t want_invalid) {
  const int64_t V = (int64_t)v.size() / 3;
  std::vector<uint8_t> code(std::max<int64_t>(E, 1));
  for (int64_t i = 0; i < E; ++i) code[i] = (uint8_t)(i % 4 == 3 ? 7 : i % 4);      // 0, 1, 2, and a code that means free
  std::vector<float> pos(std::max<int64_t>(E, 1) * 3, NAN);
  std::vector<double> cost(std::max<int64_t>(E, 1), NAN), weight(std::max<int64_t>(E, 1), NAN);
  int32_t invalid = 0;
  launch_shape();
  edge_collapse_cost_kernel(Q.data(), v.data(), V, edges.data(), E, code.data(), reach * reach, pos.data(), cost.data(), weight.data(),
                            &invalid);
  int64_t bad = 0;
  for (int64_t i = 0; i < E; ++i) {
    const int64_t a = edges[2 * i], b = edges[2 * i + 1];
    const float* p = &pos[3 * i];
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(cost[i]) && std::isfinite(weight[i]))) { ++bad; continue; }
    if (a < 0 || a >= V || b < 0 || b >= V || a == b) { bad += !(cost[i] == kInvalidCost && weight[i] == 0 && p[0] == 0); continue; }
    double q[11];
    for (int t = 0; t < 11; ++t) q[t] = Q[a * 11 + t] + Q[b * 11 + t];
    const float* pa = &v[3 * a];
    const float* pb = &v[3 * b];
    const float mid[3] = {(float)(0.5 * ((double)pa[0] + pb[0])), (float)(0.5 * ((double)pa[1] + pb[1])), (float)(0.5 * ((double)pa[2] + pb[2]))};
    const ld tol = 32 * 1.1102230246251565e-16L * abs_cost(q, p);
    if (fabsl(plain_cost(q, p) - cost[i]) > tol || weight[i] != q[10] || cost[i] < 0) ++bad;
    if (code[i] == 1) bad += memcmp(p, pa, 12) != 0;
    else if (code[i] == 2) bad += memcmp(p, pb, 12) != 0;
    else {
      for (const float* c : {pa, pb, (const float*)mid}) bad += cost[i] > plain_cost(q, c) + 32 * 1.1102230246251565e-16L * abs_cost(q, c);
      const ld dx = p[0] - 0.5L * (pa[0] + (ld)pb[0]), dy = p[1] - 0.5L * (pa[1] + (ld)pb[1]), dz = p[2] - 0.5L * (pa[2] + (ld)pb[2]);
      const ld ex = (ld)pb[0] - pa[0], ey = (ld)pb[1] - pa[1], ez = (ld)pb[2] - pa[2];
      bad += dx * dx + dy * dy + dz * dz > (reach * reach) * (ex * ex + ey * ey + ez * ez) * (1 + 1e-12L) && memcmp(p, pa, 12) && memcmp(p, pb, 12);
    }
  }
  const bool ok = bad == 0 && invalid == want_invalid;
  printf("cost %s: %lld edges, %d invalid, %lld mismatches%s\n", name, (long long)E, invalid, (long long)bad, ok ? "" : "  <-- WRONG");
  return ok ? 0 : 1;
}

static void add_plane_host(double* q, double w, double nx, double ny, double nz, double d) {
  const double p[4] = {nx, ny, nz, d};
  int k = 0;
  for (int r = 0; r < 4; ++r)
    for (int c = r; c < 4; ++c, ++k) q[k] += w * p[r] * p[c];
  q[10] += w;
}

// two vertices with hand-made quadrics of rank 0 .. 3; returns the point and cost of the free edge (0, 1)
static int check_ranks() {
  int bad = 0;
  const std::vector<float> v = {1.f, 2.f, 0.f, 3.f, 2.f, 0.f};
  const std::vector<int64_t> e = {0, 1};
  const uint8_t code = 0;
  for (int rank = 0; rank <= 3; ++rank) {
    std::vector<double> Q(22, 0.);
    if (rank >= 1) { add_plane_host(&Q[0], 0.5, 0, 0, 1, 0); add_plane_host(&Q[11], 0.7, 0, 0, 1, 0); }      // z = 0
    if (rank >= 2) { add_plane_host(&Q[0], 0.3, 0, 1, 0, -2); add_plane_host(&Q[11], 0.3, 0, 1, 0, -2); }    // y = 2: a crease along x
    if (rank >= 3) add_plane_host(&Q[11], 0.2, 1, 0, 0, -2.5);                                              // x = 2.5
    float pos[3] = {NAN, NAN, NAN};
    double cost = NAN, weight = NAN;
    int32_t invalid = 0;
    launch_shape();
    edge_collapse_cost_kernel(Q.data(), v.data(), 2, e.data(), 1, &code, 4., pos, &cost, &weight, &invalid);
    // (rank 3: the ten terms of x, y and z planes mix, so the sum at the optimum is rounding noise, within 32 u sum |terms|)
    bool ok = std::isfinite(pos[0]) && std::isfinite(pos[1]) && std::isfinite(pos[2]) && invalid == 0 && (rank < 3 ? cost == 0. : cost >= 0. && cost <= 1e-13);
    if (rank < 3) ok = ok && pos[0] == 1.f && pos[1] == 2.f && pos[2] == 0.f;       // singular: a, b and the midpoint all cost 0, a is first
    else ok = ok && pos[0] == 2.5f && pos[1] == 2.f && pos[2] == 0.f;               // the one point on all three planes
    printf("cost rank %d: pos (%g, %g, %g), cost %g%s\n", rank, pos[0], pos[1], pos[2], cost, ok ? ", 0 mismatches" : "  <-- WRONG");
    bad += !ok;
  }
  {                                                        // the optimum 24 edge lengths from the midpoint: beyond a reach of 4 it takes no part and the cheaper end wins
    std::vector<double> Q(22, 0.);
    add_plane_host(&Q[0], 1, 0, 0, 1, 0); add_plane_host(&Q[0], 1, 0, 1, 0, -2); add_plane_host(&Q[11], 1, 1, 0, 0, -50);   // x = 50
    float pos[3];
    double cost, weight;
    int32_t invalid = 0;
    edge_collapse_cost_kernel(Q.data(), v.data(), 2, e.data(), 1, &code, 4. * 4., pos, &cost, &weight, &invalid);
    const bool ok = pos[0] == 3.f && pos[1] == 2.f && pos[2] == 0.f && cost == 47. * 47.;
    printf("cost beyond the reach: pos (%g, %g, %g), cost %g%s\n", pos[0], pos[1], pos[2], cost, ok ? ", 0 mismatches" : "  <-- WRONG");
    bad += !ok;
    edge_collapse_cost_kernel(Q.data(), v.data(), 2, e.data(), 1, &code, 40. * 40., pos, &cost, &weight, &invalid);
    const bool ok2 = pos[0] == 50.f && pos[1] == 2.f && pos[2] == 0.f && cost == 0.;
    printf("cost within a longer reach: pos (%g, %g, %g), cost %g%s\n", pos[0], pos[1], pos[2], cost, ok2 ? ", 0 mismatches" : "  <-- WRONG");
    bad += !ok2;
  }
  return bad;
}

static bool plain_flip(const Mesh& m, const Tables& t, int64_t a, int64_t b, const float* p, ld* closest) {
  bool good = true;
  for (int64_t end : {a, b})
    for (int64_t j = t.vf_off[end]; j < t.vf_off[end + 1]; ++j) {
      const int64_t* r = &m.f[3 * t.vf_idx[j]];
      const bool ha = r[0] == a || r[1] == a || r[2] == a, hb = r[0] == b || r[1] == b || r[2] == b;
      if (ha && hb) continue;
      ld c[3][3], d[3][3];
      for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y) { c[x][y] = m.v[3 * r[x] + y]; d[x][y] = r[x] == end ? (ld)p[y] : c[x][y]; }
      auto cross = [](ld q[3][3], ld* n) {
        const ld u[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]}, w[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
        n[0] = u[1] * w[2] - u[2] * w[1]; n[1] = u[2] * w[0] - u[0] * w[2]; n[2] = u[0] * w[1] - u[1] * w[0];
      };
      ld n0[3], n1[3];
      cross(c, n0); cross(d, n1);
      const ld dot = n0[0] * n1[0] + n0[1] * n1[1] + n0[2] * n1[2];
      const ld scale = sqrtl(n0[0] * n0[0] + n0[1] * n0[1] + n0[2] * n0[2]) * sqrtl(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2]) + 1e-300L;
      *closest = std::min(*closest, fabsl(dot) / scale);
      if (!(dot > 0)) good = false;
    }
  return good;
}

static int check_flip(const char* name, const Mesh& m, const std::vector<int64_t>& edges, int64_t E) {
  const Tables t = tables(m);
  std::vector<float> pos(std::max<int64_t>(E, 1) * 3);
  std::uniform_real_distribution<float> U(-0.8f, 0.8f);
  for (int64_t i = 0; i < E; ++i)
    for (int c = 0; c < 3; ++c) pos[3 * i + c] = 0.5f * (m.v[3 * edges[2 * i] + c] + m.v[3 * edges[2 * i + 1] + c]) + (i % 3 ? U(rng) : 0.f);
  std::vector<uint8_t> ok(std::max<int64_t>(E, 1), 9);
  launch_shape();
  collapse_flip_check_kernel(m.v.data(), m.V(), m.f.data(), m.F(), t.vf_off.data(), data_or_null(t.vf_idx), (int64_t)t.vf_idx.size(),
                             edges.data(), E, pos.data(), ok.data());
  int64_t bad = 0, refused = 0;
  for (int64_t i = 0; i < E; ++i) {
    ld closest = 1;
    const bool want = plain_flip(m, t, edges[2 * i], edges[2 * i + 1], &pos[3 * i], &closest);
    refused += !ok[i];
    if (ok[i] > 1 || ((ok[i] != 0) != want && closest > 1e-12L)) ++bad;
  }
  printf("flip %s: %lld edges, %lld refused, %lld mismatches%s\n", name, (long long)E, (long long)refused, (long long)bad, bad ? "  <-- WRONG" : "");
  return bad != 0;
}

// integer coordinates: the moved corner lands exactly in its opposite edge's line (the face degenerates: refused), exactly
// across it (n_old . n_new < 0), exactly where the new normal is perpendicular to the old (dot 0: refused), and on the good side
static int check_flip_by_hand() {
  Mesh m;
  m.v = {0, 0, 0, 4, 0, 0, 0, 4, 0, -4, 0, 0, 0, -4, 0};                           // a square fan round vertex 0 ...
  m.f = {0, 1, 2, 0, 2, 3, 0, 3, 4, 0, 4, 1};
  const Tables t = tables(m);
  const std::vector<int64_t> e = {0, 1, 0, 1, 0, 1, 0, 1, 0, 1};
  // the collapse of (0, 1) to p: faces (0,1,2) and (0,4,1) vanish; (0,2,3) and (0,3,4) move their corner 0 to p
  const std::vector<float> pos = {1, 0, 0,        // inside: fine
                                  -2, 2, 0,       // on the line through 2 and 3: face (p, 2, 3) has no area
                                  -4, 4, 0,       // beyond it: (p, 2, 3) turns over
                                  0, 0, 5,        // straight up from 0: normals (0,0,16) and (20,-20,16)-like, positive
                                  -2, 2, 7};      // above the line through 2 and 3: the new normal of (p, 2, 3) is horizontal: dot 0
  std::vector<uint8_t> ok(5, 9);
  launch_shape();
  collapse_flip_check_kernel(m.v.data(), m.V(), m.f.data(), m.F(), t.vf_off.data(), t.vf_idx.data(), (int64_t)t.vf_idx.size(), e.data(), 5,
                             pos.data(), ok.data());
  const uint8_t want[5] = {1, 0, 0, 1, 0};
  int bad = 0;
  for (int i = 0; i < 5; ++i) bad += ok[i] != want[i];
  printf("flip by hand: flags %d %d %d %d %d, %d mismatches%s\n", ok[0], ok[1], ok[2], ok[3], ok[4], bad, bad ? "  <-- WRONG" : "");
  return bad != 0;
}

// tables that are not what the header describes: every index must be checked before it is followed (the sanitizers watch)
static int wild_tables() {
  Mesh m = bumpy_grid(9);
  Tables t = tables(m);
  const int64_t V = m.V(), F = m.F(), B = (int64_t)t.border.size() / 3;
  auto wild = [&](std::vector<int64_t>& x, int64_t span) { for (auto& y : x) y = (int64_t)(rng() % (uint64_t)(4 * std::max<int64_t>(span, 1))) - span; };
  for (int round = 0; round < 4; ++round) {
    Tables w = t;
    Mesh mw = m;
    if (round != 1) { wild(w.vf_off, (int64_t)w.vf_idx.size()); wild(w.vb_off, (int64_t)w.vb_idx.size()); }
    if (round != 2) { wild(w.vf_idx, F); wild(w.vb_idx, B); wild(w.border, std::max(V, F)); }
    if (round == 3) wild(mw.f, V);
    std::vector<double> Q(V * 11);
    int32_t counts = 0;
    launch_shape();
    vertex_quadrics_kernel(mw.v.data(), V, mw.f.data(), F, w.vf_off.data(), w.vf_idx.data(), (int64_t)w.vf_idx.size(), w.border.data(), B,
                           w.vb_off.data(), w.vb_idx.data(), (int64_t)w.vb_idx.size(), 10., Q.data(), &counts);
    std::vector<int64_t> edges = edges_of(m);
    const int64_t E = (int64_t)edges.size() / 2;
    wild(edges, V);
    std::vector<uint8_t> code(E, (uint8_t)round), ok(E);
    std::vector<float> pos(3 * E);
    std::vector<double> cost(E), weight(E);
    edge_collapse_cost_kernel(Q.data(), mw.v.data(), V, edges.data(), E, code.data(), 4., pos.data(), cost.data(), weight.data(), &counts);
    collapse_flip_check_kernel(mw.v.data(), V, mw.f.data(), F, w.vf_off.data(), w.vf_idx.data(), (int64_t)w.vf_idx.size(), edges.data(), E,
                               pos.data(), ok.data());
  }
  printf("random tables: stayed inside the arrays, 0 mismatches\n");
  return 0;
}

int main() {
  int rc = 0;
  rc |= check_quadrics("fan of 0 (a lone vertex)", fan(0), 10., 0, 0);
  for (int64_t n : {1, 63, 64, 65, 257}) {
    char name[64];
    snprintf(name, sizeof name, "fan of %lld", (long long)n);
    rc |= check_quadrics(name, fan(n), 10., 0, n);
  }
  Mesh grid = bumpy_grid(12);                               // 242 faces, 385 edges
  rc |= check_quadrics("bumpy grid", grid, 10., 0, 6);
  rc |= check_quadrics("bumpy grid, boundary weight 0", grid, 0., 0, 6);
  {
    Mesh bad = grid;
    bad.f[3 * 5] = -1; bad.f[3 * 17 + 2] = bad.V(); bad.f[3 * 40 + 1] = bad.f[3 * 40];      // three invalid faces
    bad.v[3 * 50 + 1] = NAN;                                                                // and a corner that is not a number
    const Tables t = tables(bad);
    int32_t invalid = 0;
    const std::vector<double> Q = run_quadrics(bad, t, 10., &invalid);
    int64_t nonfinite = 0;
    for (double q : Q) nonfinite += !std::isfinite(q);
    const bool ok = invalid == 3 && nonfinite == 0;        // the faces at the NaN corner add nothing, to any vertex
    printf("quadrics with invalid faces and a NaN corner: %d invalid, %lld not finite%s\n", invalid, (long long)nonfinite,
           ok ? ", 0 mismatches" : "  <-- WRONG");
    rc |= !ok;
  }
  {
    const Tables t = tables(grid);
    int32_t invalid = 0;
    const std::vector<double> Q = run_quadrics(grid, t, 10., &invalid);
    const std::vector<int64_t> edges = edges_of(grid);
    for (int64_t E : {0, 1, 255, 256, 257}) {
      rc |= check_cost("bumpy grid", Q, grid.v, edges, E, 2., 0);
      rc |= check_flip("bumpy grid", grid, edges, E);
    }
    rc |= check_cost("bumpy grid, every edge", Q, grid.v, edges, (int64_t)edges.size() / 2, 2., 0);
    std::vector<int64_t> spoilt(edges.begin(), edges.begin() + 2 * 64);
    spoilt[0] = -1; spoilt[2 * 9 + 1] = grid.V(); spoilt[2 * 30] = spoilt[2 * 30 + 1];
    rc |= check_cost("with invalid edges", Q, grid.v, spoilt, 64, 2., 3);
    std::vector<double> zero(Q.size(), 0.);
    rc |= check_cost("rank 0 everywhere", zero, grid.v, edges, 64, 2., 0);
  }
  rc |= check_ranks() != 0;
  rc |= check_flip_by_hand();
  rc |= wild_tables();
  printf(rc ? "FAILED\n" : "all ok\n");
  return rc;
}
