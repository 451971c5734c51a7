// Host check of csrc/point_grid.hip: its kernels compiled for the CPU (the stand-in common.h of tools/host_check:
// kernels called as functions, one thread after the other) under the host's sanitizers.  point_grid.inc is
// csrc/point_grid.hip up to its `using namespace recmv;` line (tests/host_check.py builds it; tests/test_mesh_repair_cpu.py runs
// it).
//   * the pair set against the plain O(V^2) loop with the same float64 expression, and the same array from a second run, on
//     the shapes of tests/test_gpu_mesh_repair.py: V = 0, 1, 2; 255, 256, 257 random points; 300 coincident points; a 6 x 6 x 6
//     integer lattice with eps = 1, shifted to negative coordinates and to straddle 0; eps = 0 with signed zeros; NaN and inf;
//     two clusters 1e6 apart with eps = 1e-6 (the cell cap); eps beyond the bounding box.
//   * every table (cell starts, sorted ids, row offsets) filled with random numbers in turn: the kernels must stay inside
//     their arrays (the sanitizers watch).
#include "common.h"
#include "point_grid.inc"
#include <cmath>
#include <random>
#include <utility>
#include <vector>
using namespace recmv;
static std::mt19937 rng(29);

static void launch_shape() { blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0}; }

static bool finite_row(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// recmv/repair.py: grid_layout
static PointGrid layout(const std::vector<float>& v, double eps, int64_t* n_finite) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int64_t n = 0;
  for (size_t i = 0; i < v.size() / 3; ++i) {
    if (!finite_row(&v[3 * i])) continue;
    ++n;
    for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], (double)v[3 * i + c]); hi[c] = std::max(hi[c], (double)v[3 * i + c]); }
  }
  *n_finite = n;
  if (n == 0) return PointGrid{0., 0., 0., 1., 1, 1, 1};
  const int64_t cap = std::min<int64_t>(kPointMaxCells, std::max<int64_t>(4 * n, 64));
  const double ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
  double cell = std::max(eps * (1. + std::ldexp(1., -20)), std::max(ext[0], std::max(ext[1], ext[2])) / (double)(kPointMaxAxis - 2));
  if (!(cell > 0.)) cell = 1.;
  for (;;) {
    int64_t d[3];
    for (int c = 0; c < 3; ++c) d[c] = std::min<int64_t>((int64_t)(ext[c] / cell) + 1, kPointMaxAxis);
    if (d[0] * d[1] * d[2] <= cap) return PointGrid{lo[0], lo[1], lo[2], cell, (int32_t)d[0], (int32_t)d[1], (int32_t)d[2]};
    cell *= 2.;
  }
}

struct Search {
  PointGrid g;
  std::vector<float> pts;
  std::vector<int64_t> ids, counts, offsets, pairs;
  std::vector<int32_t> cell_start;
  int64_t n = 0, V = 0, nonfinite = 0, total = 0;
};

template <class T> static T* data_or_null(std::vector<T>& x) { return x.empty() ? nullptr : x.data(); }

static void sort_by_cell(Search& s, const std::vector<float>& v) {
  std::vector<int32_t> cell(std::max<int64_t>(s.V, 1), -7);
  launch_shape();
  points_cells_kernel(v.data(), s.V, s.g, cell.data());
  const int64_t cells = (int64_t)s.g.nx * s.g.ny * s.g.nz;
  std::vector<std::pair<int32_t, int64_t>> key;
  for (int64_t i = 0; i < s.V; ++i) {
    if (cell[i] >= 0) key.push_back({cell[i], i});
    else ++s.nonfinite;
  }
  std::sort(key.begin(), key.end());
  s.n = (int64_t)key.size();
  s.cell_start.assign(cells + 1, 0);
  for (auto& k : key) {
    s.ids.push_back(k.second);
    s.pts.insert(s.pts.end(), {v[3 * k.second], v[3 * k.second + 1], v[3 * k.second + 2]});
    ++s.cell_start[k.first + 1];
  }
  for (int64_t c = 0; c < cells; ++c) s.cell_start[c + 1] += s.cell_start[c];
}

static Search search(const std::vector<float>& v, double eps) {
  Search s;
  s.V = (int64_t)v.size() / 3;
  int64_t n_finite = 0;
  s.g = layout(v, eps, &n_finite);
  sort_by_cell(s, v);
  s.counts.assign(std::max<int64_t>(s.V, 1), 0);
  launch_shape();
  points_within_kernel<false>(data_or_null(s.pts), data_or_null(s.ids), s.n, s.V, eps * eps, s.g, s.cell_start.data(), nullptr,
                              s.counts.data(), 0);
  s.offsets.assign(std::max<int64_t>(s.V, 1), 0);
  for (int64_t i = 0; i < s.V; ++i) { s.offsets[i] = s.total; s.total += s.counts[i]; }
  s.pairs.assign(2 * std::max<int64_t>(s.total, 1), -1);
  points_within_kernel<true>(data_or_null(s.pts), data_or_null(s.ids), s.n, s.V, eps * eps, s.g, s.cell_start.data(), s.offsets.data(),
                             s.pairs.data(), s.total);
  s.pairs.resize(2 * s.total);
  return s;
}

static std::vector<std::pair<int64_t, int64_t>> plain(const std::vector<float>& v, double eps) {
  std::vector<std::pair<int64_t, int64_t>> out;
  const int64_t V = (int64_t)v.size() / 3;
  const double eps2 = eps * eps;
  for (int64_t i = 0; i < V; ++i)
    for (int64_t j = i + 1; j < V; ++j) {
      if (!finite_row(&v[3 * i]) || !finite_row(&v[3 * j])) continue;
      const double dx = (double)v[3 * j] - (double)v[3 * i], dy = (double)v[3 * j + 1] - (double)v[3 * i + 1],
                   dz = (double)v[3 * j + 2] - (double)v[3 * i + 2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      if (d2 <= eps2) out.push_back({i, j});
    }
  return out;
}

static int check(const char* name, const std::vector<float>& v, double eps, int64_t want_pairs, int64_t want_nonfinite) {
  const Search a = search(v, eps), b = search(v, eps);
  std::vector<std::pair<int64_t, int64_t>> got;
  for (int64_t k = 0; k < a.total; ++k) got.push_back({a.pairs[2 * k], a.pairs[2 * k + 1]});
  std::sort(got.begin(), got.end());
  const bool ok = got == plain(v, eps) && a.pairs == b.pairs && (want_pairs < 0 || a.total == want_pairs) && a.nonfinite == want_nonfinite &&
                  (int64_t)a.g.nx * a.g.ny * a.g.nz <= std::max<int64_t>(4 * a.n, 64) && a.g.h >= eps;
  printf("pairs %s: %lld vertices, %lld not finite, %d x %d x %d cells of %g, %lld pairs%s\n", name, (long long)a.V, (long long)a.nonfinite,
         a.g.nx, a.g.ny, a.g.nz, a.g.h, (long long)a.total, ok ? ", 0 mismatches" : "  <-- WRONG");
  return ok ? 0 : 1;
}

static std::vector<float> random_cloud(int64_t V, double scale = 1., double shift = 0.) {
  std::uniform_real_distribution<double> U(0., 1.);
  std::vector<float> v(3 * V);
  for (auto& x : v) x = (float)(U(rng) * scale + shift);
  return v;
}

static std::vector<float> lattice(int n, float shift) {
  std::vector<float> v;
  for (int x = 0; x < n; ++x)
    for (int y = 0; y < n; ++y)
      for (int z = 0; z < n; ++z) v.insert(v.end(), {(float)x + shift, (float)y + shift, (float)z + shift});
  return v;
}

// tables that are not what the header describes: every value must be checked before it is followed
static int wild_tables() {
  const std::vector<float> v = random_cloud(300);
  const double eps = 0.15;
  const Search good = search(v, eps);
  const int64_t cells = (int64_t)good.g.nx * good.g.ny * good.g.nz;
  for (int round = 0; round < 6; ++round) {
    Search s = good;
    if (round == 0 || round == 3) for (auto& x : s.cell_start) x = (int32_t)(rng() % 2000) - 1000;
    if (round == 1 || round == 3) for (auto& x : s.ids) x = (int64_t)(rng() % 1200) - 600;
    if (round == 2 || round == 3) for (auto& x : s.offsets) x = (int64_t)(rng() % (uint64_t)(4 * good.total + 4)) - 2 * good.total;
    if (round == 4) for (auto& x : s.cell_start) x = x % 2 ? INT32_MAX : INT32_MIN;
    if (round == 5) for (auto& x : s.offsets) x = x % 2 ? INT64_MAX : INT64_MIN;
    std::vector<int64_t> counts(s.V, 0), pairs(2 * good.total, -1);
    launch_shape();
    points_within_kernel<false>(s.pts.data(), s.ids.data(), s.n, s.V, eps * eps, s.g, s.cell_start.data(), nullptr, counts.data(), 0);
    points_within_kernel<true>(s.pts.data(), s.ids.data(), s.n, s.V, eps * eps, s.g, s.cell_start.data(), s.offsets.data(), pairs.data(),
                               good.total);
  }
  printf("random tables: %lld cells, stayed inside the arrays, 0 mismatches\n", (long long)cells);
  return 0;
}

int main() {
  int rc = 0;
  rc |= check("V=0", {}, 0.5, 0, 0);
  rc |= check("V=1", {1.f, 1.f, 1.f}, 0.5, 0, 0);
  rc |= check("V=2", {0.f, 0.f, 0.f, 0.25f, 0.f, 0.f}, 0.5, 1, 0);
  for (int64_t V : {255, 256, 257}) {
    char name[64];
    snprintf(name, sizeof name, "random V=%lld", (long long)V);
    rc |= check(name, random_cloud(V), 0.12, -1, 0);
  }
  {
    std::vector<float> v;
    for (int i = 0; i < 300; ++i) v.insert(v.end(), {0.5f, -2.f, 3.f});
    rc |= check("300 coincident", v, 0., 44850, 0);
  }
  rc |= check("lattice", lattice(6, 0.f), 1., 3 * 6 * 6 * 5, 0);                   // the axis neighbours at exactly d2 == eps^2
  rc |= check("lattice negative", lattice(6, -40.f), 1., 3 * 6 * 6 * 5, 0);
  rc |= check("lattice straddling 0", lattice(6, -3.f), 1., 3 * 6 * 6 * 5, 0);
  rc |= check("signed zeros", {0.f, 0.f, 0.f, -0.f, 0.f, -0.f, 0.f, -0.f, 0.f, 1.f, 0.f, 0.f, 1.f, -0.f, 0.f, 1.f, 0.f, 1e-30f}, 0., 4, 0);
  {
    std::vector<float> v = random_cloud(40);
    v[3 * 3] = NAN; v[3 * 9 + 2] = INFINITY; v[3 * 17 + 1] = -INFINITY; v[3 * 30] = v[3 * 30 + 1] = v[3 * 30 + 2] = NAN;
    for (int c = 0; c < 3; ++c) { v[3 * 4 + c] = v[3 * 5 + c]; v[3 * 10 + c] = v[3 * 11 + c]; v[3 * 31 + c] = v[3 * 32 + c]; }
    rc |= check("nan and inf", v, 0.2, -1, 4);
  }
  {
    std::vector<float> v = random_cloud(30, 2e-6), w = random_cloud(30, 2e-6, 1e6);
    v.insert(v.end(), w.begin(), w.end());
    rc |= check("two clusters 1e6 apart", v, 1e-6, -1, 0);
  }
  rc |= check("eps beyond the box", random_cloud(64), 10., 64 * 63 / 2, 0);
  rc |= wild_tables();
  printf(rc ? "FAILED\n" : "all ok\n");
  return rc;
}
