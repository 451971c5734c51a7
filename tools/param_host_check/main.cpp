// csrc/mesh_param.hip's kernels compiled for the CPU (one lane per wave, one thread per workgroup) and run under the address
// and undefined-behaviour sanitizers against plain loops, bit for bit: the flat frames and corner weights, the ARAP local step
// with its energy and right-hand side, the distortion, and the whole lds-route solve (iteration count, residual sums, zero
// rows, u).  With one lane per wave the canonical summation order is: a slot is the sum of 256 consecutive terms from 0,
// accumulator t adds the slots t, t + 256, ..., the 256 accumulators are added from 0.  The launch route's kernels reduce K > 1
// sums through K threads of a workgroup, which one thread after the other cannot play; the GPU tests hold them to the same bits.
// Inputs: a jittered grid with two sides fixed, a grid of 600 vertices (three slots), a mesh with an isolated vertex, a face
// without area, faces with indices outside [0, V) and a NaN vertex, and a single triangle.
#include "common.h"
#include "recmv_hip.h"
#include <stdlib.h>
#include <vector>

#include "param.inc"                                       // csrc/mesh_param.hip up to its entry points
using namespace recmv;

static uint32_t rng_state = 2024u;
static double rnd() {                                      // [0, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) * (1. / 16777216.);
}

struct Mesh {
  std::vector<float> v;
  std::vector<int64_t> f;
  int64_t V() const { return (int64_t)v.size() / 3; }
  int64_t F() const { return (int64_t)f.size() / 3; }
};

static Mesh grid(int n, int m, double jitter) {
  Mesh g;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < m; ++j) {
      const bool inner = i > 0 && j > 0 && i < n - 1 && j < m - 1;
      g.v.push_back((float)(i + (inner ? jitter * (rnd() - 0.5) : 0.)));
      g.v.push_back((float)(j + (inner ? jitter * (rnd() - 0.5) : 0.)));
      g.v.push_back((float)(0.3 * jitter * rnd()));
    }
  for (int i = 0; i + 1 < n; ++i)
    for (int j = 0; j + 1 < m; ++j) {
      const int64_t a = i * m + j, b = (i + 1) * m + j, c = (i + 1) * m + j + 1, d = i * m + j + 1;
      const int64_t even[6] = {a, b, c, a, c, d}, odd[6] = {a, b, d, b, c, d};
      g.f.insert(g.f.end(), (i + j) % 2 ? odd : even, ((i + j) % 2 ? odd : even) + 6);
    }
  return g;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static int64_t differ(const std::vector<double>& a, const std::vector<double>& b) {
  int64_t bad = a.size() != b.size();
  for (size_t k = 0; k < a.size() && k < b.size(); ++k) bad += !same_bits(a[k], b[k]);
  return bad;
}

// ---- the plain loops
static bool fin(double x) { return x - x == 0.; }

static double canon(const std::vector<double>& terms) {
  const size_t nslots = (terms.size() + 255) / 256;
  std::vector<double> acc(256, 0.);
  for (size_t s = 0; s < nslots; ++s) {
    double slot = 0.;
    for (size_t k = 256 * s; k < 256 * s + 256; ++k) slot += k < terms.size() ? terms[k] : 0.;
    acc[s % 256] += slot;
  }
  double total = 0.;
  for (double a : acc) total += a;
  return total;
}

static bool valid_row(const Mesh& m, int64_t t) {
  const int64_t* r = &m.f[3 * t];
  for (int k = 0; k < 3; ++k)
    if (r[k] < 0 || r[k] >= m.V()) return false;
  return r[0] != r[1] && r[0] != r[2] && r[1] != r[2];
}

static double plain_half_cot(const double p[3][3], int c) {
  const int a = (c + 1) % 3, b = (c + 2) % 3;
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) { e1[k] = p[a][k] - p[c][k]; e2[k] = p[b][k] - p[c][k]; }
  const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (!(fin(len) && len > 0.)) return 0.;
  const double cot = (e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2]) / len;
  return cot > 0. ? 0.5 * cot : 0.;
}

static void plain_frames(const Mesh& m, std::vector<double>& frames, std::vector<double>& cots) {
  frames.assign(4 * m.F(), 0.);
  cots.assign(3 * m.F(), 0.);
  for (int64_t t = 0; t < m.F(); ++t) {
    if (!valid_row(m, t)) continue;
    double p[3][3];
    bool ok = true;
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 3; ++k) {
        p[c][k] = m.v[3 * m.f[3 * t + c] + k];
        ok = ok && fin(p[c][k]);
      }
    if (!ok) continue;
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) { e1[k] = p[1][k] - p[0][k]; e2[k] = p[2][k] - p[0][k]; }
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double x1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    if (!(fin(len) && len > 0. && fin(x1) && x1 > 0.)) continue;
    frames[4 * t] = x1;
    frames[4 * t + 1] = (e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2]) / x1;
    frames[4 * t + 2] = len / x1;
    frames[4 * t + 3] = 0.5 * len;
    for (int c = 0; c < 3; ++c) cots[3 * t + c] = plain_half_cot(p, c);
  }
}

static bool flat(const Mesh& m, const std::vector<double>& frames, int64_t t, double X[3][2]) {
  if (!valid_row(m, t) || !(frames[4 * t + 3] > 0.)) return false;
  X[0][0] = X[0][1] = X[1][1] = 0.;
  X[1][0] = frames[4 * t];
  X[2][0] = frames[4 * t + 1];
  X[2][1] = frames[4 * t + 2];
  return true;
}

static void plain_arap(const Mesh& m, const std::vector<double>& frames, const std::vector<double>& cots,
                       const std::vector<double>& uv, std::vector<double>& rot, std::vector<double>& rhs, double& energy) {
  const int64_t F = m.F(), V = m.V();
  rot.assign(2 * F, 0.);
  rhs.assign(2 * V, 0.);
  std::vector<double> e(F, 0.);
  for (int64_t t = 0; t < F; ++t) {
    double X[3][2], ra = 1., rb = 0.;
    if (flat(m, frames, t, X)) {
      double du[3][2], dx[3][2], S[4] = {0., 0., 0., 0.};
      for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        for (int c = 0; c < 2; ++c) {
          du[k][c] = uv[2 * m.f[3 * t + a] + c] - uv[2 * m.f[3 * t + b] + c];
          dx[k][c] = X[a][c] - X[b][c];
        }
        for (int r = 0; r < 2; ++r)
          for (int c = 0; c < 2; ++c) S[2 * r + c] += cots[3 * t + k] * (du[k][r] * dx[k][c]);
      }
      const double ca = S[0] + S[3], cb = S[2] - S[1], len = sqrt(ca * ca + cb * cb);
      if (fin(len) && len > 0.) { ra = ca / len; rb = cb / len; }
      for (int k = 0; k < 3; ++k) {
        const double d0 = du[k][0] - (ra * dx[k][0] - rb * dx[k][1]), d1 = du[k][1] - (rb * dx[k][0] + ra * dx[k][1]);
        e[t] += cots[3 * t + k] * (d0 * d0 + d1 * d1);
      }
    }
    rot[2 * t] = ra;
    rot[2 * t + 1] = rb;
  }
  energy = canon(e);
  for (int64_t i = 0; i < V; ++i)
    for (int64_t t = 0; t < F; ++t)                        // the slots of a vertex, ascending
      for (int k = 0; k < 3; ++k) {
        double X[3][2];
        if (m.f[3 * t + k] != i || !flat(m, frames, t, X)) continue;
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const double ra = rot[2 * t], rb = rot[2 * t + 1], c1 = cots[3 * t + k2], c2 = cots[3 * t + k1];
        const double a0 = X[k][0] - X[k1][0], a1 = X[k][1] - X[k1][1], b0 = X[k][0] - X[k2][0], b1 = X[k][1] - X[k2][1];
        rhs[2 * i] += c1 * (ra * a0 - rb * a1);
        rhs[2 * i + 1] += c1 * (rb * a0 + ra * a1);
        rhs[2 * i] += c2 * (ra * b0 - rb * b1);
        rhs[2 * i + 1] += c2 * (rb * b0 + ra * b1);
      }
}

static void plain_distortion(const Mesh& m, const std::vector<double>& frames, const std::vector<double>& uv,
                             std::vector<double>& out) {
  out.assign(3 * m.F(), 0.);
  for (int64_t t = 0; t < m.F(); ++t) {
    double X[3][2];
    out[3 * t] = out[3 * t + 1] = NAN;
    if (!flat(m, frames, t, X)) continue;
    const int64_t* r = &m.f[3 * t];
    const double a0 = uv[2 * r[1]] - uv[2 * r[0]], a1 = uv[2 * r[1] + 1] - uv[2 * r[0] + 1];
    const double b0 = uv[2 * r[2]] - uv[2 * r[0]], b1 = uv[2 * r[2] + 1] - uv[2 * r[0] + 1];
    const double J00 = a0 / X[1][0], J10 = a1 / X[1][0], J01 = (b0 - J00 * X[2][0]) / X[2][1], J11 = (b1 - J10 * X[2][0]) / X[2][1];
    const double E = (J00 + J11) * 0.5, Fh = (J00 - J11) * 0.5, G = (J10 + J01) * 0.5, H = (J10 - J01) * 0.5;
    const double Q = sqrt(E * E + H * H), R = sqrt(Fh * Fh + G * G);
    out[3 * t] = Q + R;
    out[3 * t + 1] = Q > R ? Q - R : R - Q;
    out[3 * t + 2] = J00 * J11 - J01 * J10;
  }
}

struct Csr {
  std::vector<int32_t> off, nbr;
  std::vector<double> w;
};

// the neighbour table of the valid faces with the summed corner weights, plus entries that must not count
static Csr neighbours(const Mesh& m, const std::vector<double>& cots) {
  const int64_t V = m.V();
  std::vector<std::vector<std::pair<int32_t, double>>> rows(V);
  auto add = [&](int64_t i, int64_t j, double w) {
    for (auto& e : rows[i])
      if (e.first == j) { e.second += w; return; }
    rows[i].push_back({(int32_t)j, w});
  };
  for (int64_t t = 0; t < m.F(); ++t) {
    if (!valid_row(m, t)) continue;
    for (int c = 0; c < 3; ++c) {
      const int64_t a = m.f[3 * t + (c + 1) % 3], b = m.f[3 * t + (c + 2) % 3];
      add(a, b, cots[3 * t + c]);
      add(b, a, cots[3 * t + c]);
    }
  }
  Csr out;
  out.off.push_back(0);
  for (int64_t i = 0; i < V; ++i) {
    std::sort(rows[i].begin(), rows[i].end());
    for (auto& e : rows[i]) { out.nbr.push_back(e.first); out.w.push_back(e.second); }
    if (i == 3) { out.nbr.push_back(3); out.w.push_back(7.); out.nbr.push_back(-4); out.w.push_back(1.);   // itself; outside
                  out.nbr.push_back((int32_t)V); out.w.push_back(1.); out.nbr.push_back(0); out.w.push_back(NAN); }
    out.off.push_back((int32_t)out.nbr.size());
  }
  return out;
}

struct Solved {
  std::vector<double> u;
  int iters, zero_rows;
  double rr[2], bb[2];
};

static Solved plain_solve(const Csr& g, int64_t V, const std::vector<uint8_t>& fixed, const std::vector<double>& rhs,
                          std::vector<double> u, double tol, int max_iter) {
  auto counts = [&](int64_t i, int64_t k) {
    const int64_t j = g.nbr[k];
    return j >= 0 && j < V && j != i && fin(g.w[k]) && g.w[k] > 0.;
  };
  std::vector<double> dinv(V, 0.), r(2 * V, 0.), p(2 * V, 0.), q(2 * V, 0.);
  std::vector<double> t[8];
  for (auto& x : t) x.assign(V, 0.);
  Solved out;
  for (int64_t i = 0; i < V; ++i) {
    double d = 0., au[2] = {0., 0.}, fx[2] = {0., 0.};
    for (int64_t k = g.off[i]; k < g.off[i + 1]; ++k) {
      if (!counts(i, k)) continue;
      const int64_t j = g.nbr[k];
      d += g.w[k];
      for (int c = 0; c < 2; ++c) {
        au[c] += g.w[k] * (u[2 * i + c] - u[2 * j + c]);
        if (fixed[j]) fx[c] += g.w[k] * u[2 * j + c];
      }
    }
    const bool act = !fixed[i] && d > 0.;
    t[6][i] = (!fixed[i] && !(d > 0.)) ? 1. : 0.;
    if (!act) continue;
    dinv[i] = 1. / d;
    for (int c = 0; c < 2; ++c) {
      r[2 * i + c] = rhs[2 * i + c] - au[c];
      const double b = rhs[2 * i + c] + fx[c];
      t[c][i] = b * b;
      t[2 + c][i] = r[2 * i + c] * (r[2 * i + c] * dinv[i]);
      t[4 + c][i] = r[2 * i + c] * r[2 * i + c];
    }
  }
  double rz[2], alpha[2] = {0., 0.}, beta[2] = {0., 0.};
  bool active[2];
  for (int c = 0; c < 2; ++c) {
    out.bb[c] = canon(t[c]);
    rz[c] = canon(t[2 + c]);
    out.rr[c] = canon(t[4 + c]);
    active[c] = out.rr[c] > tol * tol * out.bb[c];
  }
  out.zero_rows = (int)canon(t[6]);
  out.iters = 0;
  bool done = !(active[0] || active[1]) || max_iter <= 0;
  while (!done) {
    for (int64_t i = 0; i < V; ++i)
      if (dinv[i] > 0.)
        for (int c = 0; c < 2; ++c) p[2 * i + c] = r[2 * i + c] * dinv[i] + beta[c] * p[2 * i + c];
    for (int c = 0; c < 2; ++c) t[c].assign(V, 0.);
    for (int64_t i = 0; i < V; ++i) {
      double s[2] = {0., 0.};
      if (dinv[i] > 0.)
        for (int64_t k = g.off[i]; k < g.off[i + 1]; ++k)
          if (counts(i, k))
            for (int c = 0; c < 2; ++c) s[c] += g.w[k] * (p[2 * i + c] - p[2 * g.nbr[k] + c]);
      for (int c = 0; c < 2; ++c) { q[2 * i + c] = s[c]; t[c][i] = p[2 * i + c] * s[c]; }
    }
    for (int c = 0; c < 2; ++c) {
      const double pq = canon(t[c]), al = rz[c] / pq;
      const bool ok = active[c] && pq > 0. && fin(al);
      alpha[c] = ok ? al : 0.;
      active[c] = ok;
    }
    ++out.iters;
    for (auto& x : t) x.assign(V, 0.);
    for (int64_t i = 0; i < V; ++i)
      if (dinv[i] > 0.)
        for (int c = 0; c < 2; ++c) {
          u[2 * i + c] = u[2 * i + c] + alpha[c] * p[2 * i + c];
          const double rc = r[2 * i + c] - alpha[c] * q[2 * i + c];
          r[2 * i + c] = rc;
          t[c][i] = rc * (rc * dinv[i]);
          t[2 + c][i] = rc * rc;
        }
    for (int c = 0; c < 2; ++c) {
      if (active[c]) {
        const double nrz = canon(t[c]), nrr = canon(t[2 + c]), be = rz[c] != 0. ? nrz / rz[c] : 0.;
        beta[c] = be;
        rz[c] = nrz;
        out.rr[c] = nrr;
        if (!(nrr > tol * tol * out.bb[c]) || !fin(be)) active[c] = false;
      }
      if (!active[c]) beta[c] = 0.;
    }
    done = !(active[0] || active[1]) || out.iters >= max_iter;
  }
  out.u = u;
  return out;
}

// ---- one mesh through every kernel
static int check(const char* name, const Mesh& m, bool sides_fixed, int max_iter) {
  const int64_t V = m.V(), F = m.F();
  std::vector<double> uv(2 * V);
  for (auto& x : uv) x = 4. * rnd() - 2.;
  blockDim.x = 1; threadIdx.x = 0;

  std::vector<double> frames(4 * F, -1.), cots(3 * F, -1.), wf, wc;
  gridDim.x = (unsigned)F + 1;                             // one workgroup beyond the end
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    param_face_frames_kernel(m.v.data(), V, m.f.data(), F, frames.data(), cots.data());
  plain_frames(m, wf, wc);
  const int64_t bad_frames = differ(frames, wf) + differ(cots, wc);

  std::vector<int64_t> soff(V + 1, 0), slots;
  for (int64_t i = 0; i < V; ++i) {
    for (int64_t s = 0; s < 3 * F; ++s)
      if (m.f[s] == i) slots.push_back(s);
    soff[i + 1] = (int64_t)slots.size();
  }
  slots.push_back(-3);                                     // never read: a row ends before it (and it would be skipped)
  std::vector<double> rot(2 * F, -1.), rhs(2 * V, -1.), partials(F + 1, -1.), energy(1, -1.), wrot, wrhs;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    param_arap_faces_kernel(m.f.data(), F, frames.data(), cots.data(), uv.data(), V, rot.data(), partials.data());
  // one term per workgroup here, so the slots of 256 faces are added by hand, then the kernel adds the slots: 256 threads, the
  // last first, so that thread 0 finds every accumulator
  std::vector<double> slotsum((F + 255) / 256, 0.);
  for (int64_t t = 0; t < F; ++t) slotsum[t / 256] += partials[t];
  blockDim.x = 256; gridDim.x = 1; blockIdx.x = 0;
  for (int t = 255; t >= 0; --t) {
    threadIdx.x = (unsigned)t;
    param_energy_kernel(slotsum.data(), (int)slotsum.size(), energy.data());
  }
  blockDim.x = 1; threadIdx.x = 0;
  gridDim.x = (unsigned)V + 1;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    param_arap_rhs_kernel(m.f.data(), F, frames.data(), cots.data(), rot.data(), V, soff.data(), slots.data(), rhs.data());
  double wenergy;
  plain_arap(m, frames, cots, uv, wrot, wrhs, wenergy);
  const int64_t bad_arap = differ(rot, wrot) + differ(rhs, wrhs) + !same_bits(energy[0], wenergy);

  std::vector<double> dist(3 * F, -1.), wdist;
  gridDim.x = (unsigned)F + 1;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    param_distortion_kernel(m.f.data(), F, frames.data(), uv.data(), V, dist.data());
  plain_distortion(m, frames, uv, wdist);
  const int64_t bad_dist = differ(dist, wdist);

  // the solve: two sides and the last four vertices (or vertex 0 alone) fixed at its uv, the ARAP right-hand side, from the random uv
  const Csr g = neighbours(m, cots);
  std::vector<uint8_t> fixed(V, 0);
  fixed[0] = 1;
  if (sides_fixed)
    for (int64_t i = 0; i < V; ++i) fixed[i] = m.v[3 * i] == 0.f || m.v[3 * i + 1] == 0.f || i >= V - 4;
  const Solved want = plain_solve(g, V, fixed, wrhs, uv, 1e-12, max_iter);
  std::vector<double> u(uv);
  ParamCg report;
  memset(&report, 0xff, sizeof report);
  const ParamArgs a{g.off.data(), g.nbr.data(), g.w.data(), V, (int64_t)g.nbr.size()};
  gridDim.x = 1; blockIdx.x = 0;
  param_solve_lds_kernel(a, fixed.data(), wrhs.data(), u.data(), 1e-12, max_iter, &report);
  int64_t bad_solve = differ(u, want.u) + (report.iters != want.iters) + (report.zero_rows != want.zero_rows);
  for (int c = 0; c < 2; ++c) bad_solve += !same_bits(report.rr[c], want.rr[c]) + !same_bits(report.bb[c], want.bb[c]);
  const int64_t bad = bad_frames + bad_arap + bad_dist + bad_solve;
  printf("%s: %lld vertices, %lld faces, %d iterations, %d zero rows: frames %lld, arap %lld, distortion %lld, solve %lld -> %lld "
         "mismatches\n", name, (long long)V, (long long)F, want.iters, want.zero_rows, (long long)bad_frames, (long long)bad_arap,
         (long long)bad_dist, (long long)bad_solve, (long long)bad);
  return bad != 0;
}

int main() {
  int fails = 0;
  const Mesh jittered = grid(9, 9, 0.8);
  const Mesh wide = grid(20, 30, 0.5);                     // 600 vertices: three slots of 256, 1102 faces: five
  Mesh broken = grid(6, 6, 0.5);
  {
    const int64_t V = broken.V();
    broken.v[3 * 14 + 1] = NAN;                            // an inner vertex
    broken.v.insert(broken.v.end(), {9.f, 9.f, 9.f});      // vertex V: isolated
    const int64_t rows[5][3] = {{0, 6, 12}, {-1, 2, 3}, {4, 4, 5}, {7, 2, 1ll << 40}, {0, 1, V + 1}};   // no area; not valid
    for (auto& r : rows) broken.f.insert(broken.f.end(), r, r + 3);
  }
  Mesh one;
  one.v = {0.f, 0.f, 0.f, 2.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  one.f = {0, 1, 2};
  fails += check("a jittered 9 x 9 grid, two sides fixed", jittered, true, 500);
  fails += check("the same grid, one vertex fixed, stopped after 7 iterations", jittered, false, 7);
  fails += check("a 20 x 30 grid, two sides fixed", wide, true, 4000);
  fails += check("an isolated vertex, a face without area, invalid faces, a NaN vertex", broken, false, 500);
  fails += check("a single triangle", one, false, 50);
  printf(fails ? "FAILED\n" : "all ok\n");
  return fails != 0;
}
