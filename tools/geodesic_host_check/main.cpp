// csrc/geodesic.hip's kernels compiled for the CPU (one lane per workgroup on the lds route, a few lanes per workgroup on the
// sweeps route) and run under the address and undefined-behaviour sanitizers: both routes against plain loops that evaluate
// every face of every vertex in every sweep — D bit for bit and the sweep count K — and the not-converged report of the lds
// route.  Inputs: a jittered grid, a single vertex, a mesh with invalid faces and a NaN vertex, two pieces with the source in
// one, a fan of valence 70, sources with values and a duplicate, and B = 3 fields at once.
#include "common.h"
#include "recmv_hip.h"
#include <stdarg.h>
#include <stdlib.h>
#include <vector>

#include "geodesic.inc"                                    // csrc/geodesic.hip up to its entry points
using namespace recmv;

static uint32_t rng_state = 77u;
static float rnd() {                                       // [0, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (float)(rng_state >> 8) * (1.f / 16777216.f);
}

struct Mesh {
  std::vector<float> v;
  std::vector<int64_t> f;
  int64_t V() const { return (int64_t)v.size() / 3; }
  int64_t F() const { return (int64_t)f.size() / 3; }
};

static Mesh grid(int n, float jitter, float ox) {
  Mesh m;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const bool inner = i > 0 && j > 0 && i < n - 1 && j < n - 1;
      m.v.push_back(ox + i + (inner ? jitter * (rnd() - 0.5f) : 0.f));
      m.v.push_back(j + (inner ? jitter * (rnd() - 0.5f) : 0.f));
      m.v.push_back(0.1f * jitter * rnd());
    }
  for (int i = 0; i + 1 < n; ++i)
    for (int j = 0; j + 1 < n; ++j) {
      const int64_t a = i * n + j, b = (i + 1) * n + j, c = (i + 1) * n + j + 1, d = i * n + j + 1;
      const int64_t even[6] = {a, b, c, a, c, d}, odd[6] = {a, b, d, b, c, d};
      m.f.insert(m.f.end(), (i + j) % 2 ? odd : even, ((i + j) % 2 ? odd : even) + 6);
    }
  return m;
}

static void append(Mesh& m, const Mesh& o) {
  const int64_t base = m.V();
  m.v.insert(m.v.end(), o.v.begin(), o.v.end());
  for (int64_t x : o.f) m.f.push_back(x + base);
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// ---- the plain loops: the header's definition written out once more
static double len3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

static double candidate(const float* verts, int64_t v, int64_t a, int64_t b, double Da, double Db) {
  double pv[3], pa[3], pb[3], w[3], u[3], e[3];
  for (int k = 0; k < 3; ++k) {
    pv[k] = verts[3 * v + k]; pa[k] = verts[3 * a + k]; pb[k] = verts[3 * b + k];
    w[k] = pv[k] - pa[k]; u[k] = pv[k] - pb[k]; e[k] = pb[k] - pa[k];
  }
  const double ca = Da + len3(w[0], w[1], w[2]), cb = Db + len3(u[0], u[1], u[2]);
  double U = cb < ca ? cb : ca;
  if (!(Da < INFINITY && Db < INFINITY)) return U;
  const double L2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], L = sqrt(L2), delta = Db - Da;
  if (!(L > 0. && fabs(delta) < L)) return U;
  const double h = len3(w[1] * e[2] - w[2] * e[1], w[2] * e[0] - w[0] * e[2], w[0] * e[1] - w[1] * e[0]) / L;
  if (!(h > 0.)) return U;
  const double t0 = ((w[0] * e[0] + w[1] * e[1]) + w[2] * e[2]) / L2;
  const double ts = t0 - (delta * h) / (L * sqrt(L2 - delta * delta));
  if (!(ts > 0. && ts < 1.)) return U;
  const double r = ts - t0;
  const double ci = (Da + ts * delta) + sqrt(h * h + L2 * (r * r));
  return ci < U ? ci : U;
}

static bool usable(const Mesh& m, int64_t f) {
  const int64_t* r = &m.f[3 * f];
  for (int k = 0; k < 3; ++k)
    if (r[k] < 0 || r[k] >= m.V()) return false;
  if (r[0] == r[1] || r[0] == r[2] || r[1] == r[2]) return false;
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(m.v[3 * r[k] + a])) return false;
  return true;
}

// D^K and K of one field
static int plain(const Mesh& m, std::vector<double>& D) {
  for (int K = 0;; ++K) {
    std::vector<double> next = D;
    for (int64_t f = 0; f < m.F(); ++f) {
      if (!usable(m, f)) continue;
      const int64_t* r = &m.f[3 * f];
      for (int c = 0; c < 3; ++c) {
        const double U = candidate(m.v.data(), r[c], r[(c + 1) % 3], r[(c + 2) % 3], D[r[(c + 1) % 3]], D[r[(c + 2) % 3]]);
        if (U < next[r[c]]) next[r[c]] = U;
      }
    }
    if (memcmp(next.data(), D.data(), 8 * D.size()) == 0) return K;
    D = next;
  }
}

struct Source {
  int64_t field, vertex;
  double value;
};

static int check(const char* name, const Mesh& m, int B, const std::vector<Source>& sources) {
  const int64_t V = m.V(), F = m.F();
  // the slot table: a corner outside [0, V) is in no row
  std::vector<int64_t> off(V + 1, 0), slots;
  for (int64_t v = 0; v < V; ++v) {
    for (int64_t s = 0; s < 3 * F; ++s)
      if (m.f[s] == v) slots.push_back(s);
    off[v + 1] = (int64_t)slots.size();
  }
  slots.push_back(-3);                                     // never read: a row ends before it (and it would be skipped)
  std::vector<double> D0(B * V, INFINITY);
  for (const Source& s : sources)
    if (s.value < D0[s.field * V + s.vertex]) D0[s.field * V + s.vertex] = s.value;
  std::vector<double> want(D0);
  std::vector<int> wantK(B);
  for (int b = 0; b < B; ++b) {
    std::vector<double> D(want.begin() + b * V, want.begin() + (b + 1) * V);
    wantK[b] = plain(m, D);
    std::copy(D.begin(), D.end(), want.begin() + b * V);
  }
  int64_t bad_sweeps = 0, bad_lds = 0, bad_cap = 0;

  // ---- the sweeps route: the workspace's three parts as separate arrays, so that a write past one is caught
  const int64_t BV = B * V;
  std::vector<double> Da(D0), Db(BV, -1.);
  std::vector<uint8_t> ca(BV, 9), cb(BV, 9);
  std::vector<int32_t> last(B, -5);
  blockDim.x = 5;
  gridDim.x = (unsigned)((BV + 4) / 5 + 1);                // one workgroup beyond the end
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    for (threadIdx.x = 0; threadIdx.x < blockDim.x; ++threadIdx.x) geodesic_begin_kernel(BV, B, ca.data(), last.data());
  int done = 0, Kmax = 0;
  for (int b = 0; b < B; ++b) Kmax = std::max(Kmax, wantK[b]);
  for (int k = 1; k <= Kmax + 3; ++k, ++done) {
    double* src = (k - 1) & 1 ? Db.data() : Da.data();
    double* dst = k & 1 ? Db.data() : Da.data();
    uint8_t* csrc = (k - 1) & 1 ? cb.data() : ca.data();
    uint8_t* cdst = k & 1 ? cb.data() : ca.data();
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
      for (threadIdx.x = 0; threadIdx.x < blockDim.x; ++threadIdx.x)
        geodesic_sweep_kernel(m.v.data(), V, m.f.data(), F, off.data(), slots.data(), B, src, dst, csrc, cdst, last.data(), k);
  }
  const double* got = done & 1 ? Db.data() : Da.data();
  for (int64_t i = 0; i < BV; ++i) bad_sweeps += !same_bits(got[i], want[i]);
  for (int b = 0; b < B; ++b) bad_sweeps += last[b] != wantK[b];

  // ---- the lds route, and its report when the cap is one sweep short
  std::vector<double> out(BV, -1.);
  std::vector<int32_t> K(B, -7);
  blockDim.x = 1; threadIdx.x = 0; gridDim.x = (unsigned)B;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    geodesic_lds_kernel(m.v.data(), V, m.f.data(), F, off.data(), slots.data(), D0.data(), out.data(), K.data(), (int32_t)V + 1);
  for (int64_t i = 0; i < BV; ++i) bad_lds += !same_bits(out[i], want[i]);
  for (int b = 0; b < B; ++b) bad_lds += K[b] != wantK[b];
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) {
    const int b = (int)blockIdx.x;
    geodesic_lds_kernel(m.v.data(), V, m.f.data(), F, off.data(), slots.data(), D0.data(), out.data(), K.data(), wantK[b]);
    bad_cap += K[b] != wantK[b];                           // max_sweeps = K succeeds
    if (wantK[b] > 0) {
      geodesic_lds_kernel(m.v.data(), V, m.f.data(), F, off.data(), slots.data(), D0.data(), out.data(), K.data(), wantK[b] - 1);
      bad_cap += K[b] != -1;                               // max_sweeps = K - 1 does not
    }
  }
  int64_t reached = 0;
  for (int64_t i = 0; i < BV; ++i) reached += want[i] < INFINITY;
  const int64_t bad = bad_sweeps + bad_lds + bad_cap;
  printf("%s: %lld vertices, %lld faces, %d fields, K", name, (long long)V, (long long)F, B);
  for (int b = 0; b < B; ++b) printf(" %d", wantK[b]);
  printf(", %lld values finite: sweeps %lld, lds %lld, cap %lld -> %lld mismatches\n", (long long)reached, (long long)bad_sweeps,
         (long long)bad_lds, (long long)bad_cap, (long long)bad);
  return bad != 0;
}

int main() {
  int fails = 0;
  const Mesh jittered = grid(9, 0.9f, 0.f);
  Mesh one;
  one.v = {1.f, 2.f, 3.f};
  Mesh broken = grid(6, 0.5f, 0.f);
  {
    const int64_t V = broken.V();
    broken.v[3 * 14 + 1] = NAN;                            // an inner vertex
    broken.v.insert(broken.v.end(), broken.v.begin() + 3 * 8, broken.v.begin() + 3 * 9);   // vertex V: vertex 8's point again
    const int64_t rows[6][3] = {{0, 1, V + 1}, {-1, 2, 3}, {4, 4, 5}, {0, 6, 12}, {8, V, 9}, {7, 2, 1ll << 40}};
    for (auto& r : rows) broken.f.insert(broken.f.end(), r, r + 3);
  }
  Mesh pieces = grid(5, 0.3f, 0.f);
  append(pieces, grid(4, 0.3f, 10.f));
  Mesh fan;
  fan.v = {0.f, 0.f, 0.f};
  for (int i = 0; i < 70; ++i) {
    const double a = 2. * M_PI * i / 70.;
    fan.v.insert(fan.v.end(), {(float)cos(a), (float)sin(a), 0.1f * (float)sin(5. * a)});
    fan.f.insert(fan.f.end(), {0, 1 + i, 1 + (i + 1) % 70});
  }
  fails += check("a jittered 9 x 9 grid from a corner", jittered, 1, {{0, 0, 0.}});
  fails += check("a single vertex", one, 1, {{0, 0, 0.}});
  fails += check("invalid faces and a NaN vertex", broken, 1, {{0, 0, 0.}});
  fails += check("two pieces, the source in one", pieces, 1, {{0, 3, 0.}});
  fails += check("a fan of valence 70 from its rim", fan, 1, {{0, 5, 0.}});
  fails += check("sources with values and a duplicate", jittered, 1, {{0, 0, 0.5}, {0, 80, 0.}, {0, 0, 0.25}, {0, 40, 3.}});
  fails += check("three fields at once", jittered, 3, {{0, 0, 0.}, {1, 40, 0.}, {2, 8, 0.}, {2, 72, 0.}, {2, 0, 0.}, {2, 80, 0.}});
  printf(fails ? "FAILED\n" : "all ok\n");
  return fails != 0;
}
