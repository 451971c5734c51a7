// csrc/winding.hip's kernels and csrc/solid_angle.h compiled for the CPU (one lane per workgroup) and run under the address and
// undefined-behaviour sanitizers: the binning against its restatement, the pyramid's sums against a loop over every (node,
// face) pair, the stack-free traversal against a recursive walk of the same table (bit for bit) and — with a beta that
// accepts nothing — against the brute sum, and the chunked exact kernel against the reduction the header defines (bit for
// bit).  Inputs: a soup that fills the cube, levels = 1, a mesh inside one finest cell, faces with invalid indices, faces
// without area, queries outside the cube, a query on a vertex, a query that is NaN, and a mesh of more than two chunks.
#include "common.h"
#include "recmv_hip.h"
#include <stdarg.h>
#include <stdlib.h>
#include <vector>

#include "winding.inc"                                     // csrc/winding.hip up to its entry points
using namespace recmv;

static uint32_t rng_state = 2024u;
static float rnd() {                                       // [0, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (float)(rng_state >> 8) * (1.f / 16777216.f);
}

struct Mesh {
  std::vector<float> v;
  std::vector<int64_t> f;
};

// `n` triangles with centres in [lo, lo + ext)^3 and edges up to `size`, then (broken) rows with indices out of range and
// faces without area
static Mesh soup(int n, float lo, float ext, float size, bool broken) {
  Mesh m;
  for (int i = 0; i < n; ++i) {
    const float c[3] = {lo + ext * rnd(), lo + ext * rnd(), lo + ext * rnd()};
    for (int k = 0; k < 3; ++k) {
      for (int a = 0; a < 3; ++a) m.v.push_back(c[a] + size * (rnd() - 0.5f));
      m.f.push_back(3 * i + k);
    }
  }
  if (broken) {
    const int64_t V = (int64_t)m.v.size() / 3;
    const float extra[2][3] = {{0.25f, 0.25f, 0.25f}, {0.75f, 0.75f, 0.75f}};
    for (auto& e : extra) m.v.insert(m.v.end(), e, e + 3);
    // V + 2 and -1: no such vertex; (4, 4, 4) and (5, 5, V): a point and a segment; (V, V + 1, mid): collinear
    m.v.insert(m.v.end(), {0.5f, 0.5f, 0.5f});
    const int64_t rows[6][3] = {{0, 1, V + 3}, {-1, 2, 3}, {4, 4, 4}, {5, 5, V}, {V, V + 1, V + 2}, {7, 8, 1ll << 40}};
    for (auto& r : rows) m.f.insert(m.f.end(), r, r + 3);
  }
  return m;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

static int32_t axis_cell(float x, float origin, float side, int32_t n) {
  const float t = floorf((x - origin) / (side / (float)n));
  if (!(t > 0.f)) return 0;
  return t < (float)(n - 1) ? (int32_t)t : n - 1;
}

struct Walk {
  int levels;
  const float* nodes;
  const int64_t* cell_start;
  const float* tris;
  float qx, qy, qz, beta2;
  double sum;
  void visit(int l, int32_t i, int32_t j, int32_t k) {
    const int64_t cell = (((int64_t)i << l) + j) * (1ll << l) + k;
    const float* node = nodes + (level_offset(l) + cell) * kNodeFloats;
    if (node_count(node) == 0) return;
    float term;
    if (node_far(node, qx, qy, qz, beta2, term)) {
      sum += (double)term;
    } else if (l == levels) {
      for (int64_t a = cell_start[cell]; a < cell_start[cell + 1]; ++a) sum += (double)solid_angle(qx, qy, qz, tris + 9 * a);
    } else {
      for (int c = 0; c < 8; ++c) visit(l + 1, 2 * i + (c >> 2), 2 * j + ((c >> 1) & 1), 2 * k + (c & 1));
    }
  }
};

static int check(const char* name, const Mesh& m, int levels, float ox, float oy, float oz, float side) {
  const int64_t V = (int64_t)m.v.size() / 3, F = (int64_t)m.f.size() / 3;
  const Cube cube{ox, oy, oz, side, levels};
  const int32_t n = 1 << levels;
  const int64_t n_cells = 1ll << (3 * levels);
  int64_t bad_cells = 0, bad_nodes = 0, bad_walk = 0, bad_brute = 0, bad_exact = 0;

  // ---- binning
  std::vector<int64_t> cells(F, -7);
  gridDim.x = 3; blockDim.x = 5;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    for (threadIdx.x = 0; threadIdx.x < blockDim.x; ++threadIdx.x)
      winding_cells_kernel(m.v.data(), V, m.f.data(), F, cube, cells.data());
  std::vector<int64_t> order;
  for (int64_t k = 0; k < F; ++k) {
    int64_t want = -1;
    const int64_t* r = &m.f[3 * k];
    if (r[0] >= 0 && r[0] < V && r[1] >= 0 && r[1] < V && r[2] >= 0 && r[2] < V) {
      int32_t c[3];
      for (int a = 0; a < 3; ++a)
        c[a] = axis_cell(((m.v[3 * r[0] + a] + m.v[3 * r[1] + a]) + m.v[3 * r[2] + a]) / 3.f, a == 0 ? ox : a == 1 ? oy : oz, side, n);
      want = ((int64_t)c[0] * n + c[1]) * n + c[2];
    }
    bad_cells += cells[k] != want;
  }
  // the stable sort by cell of the faces that have one
  std::vector<int64_t> cell_start(n_cells + 1, 0);
  for (int64_t k = 0; k < F; ++k)
    if (cells[k] >= 0) ++cell_start[cells[k] + 1];
  for (int64_t c = 0; c < n_cells; ++c) cell_start[c + 1] += cell_start[c];
  const int64_t n_faces = cell_start[n_cells];
  order.assign(n_faces, 0);
  {
    std::vector<int64_t> at(cell_start.begin(), cell_start.end() - 1);
    for (int64_t k = 0; k < F; ++k)
      if (cells[k] >= 0) order[at[cells[k]]++] = k;
  }

  // ---- the pyramid
  const int64_t n_nodes = ((1ll << (3 * (levels + 1))) - 1) / 7;
  std::vector<float> nodes(n_nodes * kNodeFloats, -99.f), tris(n_faces * 9, -99.f);
  blockDim.x = 1; threadIdx.x = 0;
  for (blockIdx.x = 0; blockIdx.x < (unsigned)n_cells + 2; ++blockIdx.x)          // two threads beyond the last cell
    winding_leaves_kernel(m.v.data(), V, m.f.data(), F, order.data(), n_faces, cell_start.data(), levels, nodes.data(), tris.data());
  for (int l = levels - 1; l >= 0; --l)
    for (blockIdx.x = 0; blockIdx.x < (unsigned)(1ll << (3 * l)) + 2; ++blockIdx.x) winding_parents_kernel(l, nodes.data());
  for (int l = 0; l <= levels; ++l) {
    const int s = levels - l;
    const int64_t nl = 1ll << l;
    struct Sum { double area = 0, c[3] = {0, 0, 0}, N[3] = {0, 0, 0}; int32_t count = 0; float lo[3], hi[3]; };
    std::vector<Sum> want(nl * nl * nl);
    for (auto& w : want)
      for (int a = 0; a < 3; ++a) { w.lo[a] = INFINITY; w.hi[a] = -INFINITY; }
    double scale = 0;
    for (int64_t k = 0; k < F; ++k) {
      if (cells[k] < 0) continue;
      const int64_t i = cells[k] / ((int64_t)n * n) >> s, j = (cells[k] / n) % n >> s, kk = cells[k] % n >> s;
      Sum& w = want[(i * nl + j) * nl + kk];
      double p[3][3];
      for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) {
          const float x = m.v[3 * m.f[3 * k + c] + a];
          p[c][a] = x;
          w.lo[a] = fminf(w.lo[a], x);
          w.hi[a] = fmaxf(w.hi[a], x);
        }
      double u[3], v[3], nv[3];
      for (int a = 0; a < 3; ++a) { u[a] = p[1][a] - p[0][a]; v[a] = p[2][a] - p[0][a]; }
      nv[0] = 0.5 * (u[1] * v[2] - u[2] * v[1]); nv[1] = 0.5 * (u[2] * v[0] - u[0] * v[2]); nv[2] = 0.5 * (u[0] * v[1] - u[1] * v[0]);
      const double area = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
      w.area += area;
      for (int a = 0; a < 3; ++a) {
        w.c[a] += area * (p[0][a] + p[1][a] + p[2][a]) / 3.;
        w.N[a] += nv[a];
        scale = fmax(scale, fabs(p[0][a]));
      }
      ++w.count;
    }
    for (int64_t c = 0; c < nl * nl * nl; ++c) {
      const float* g = &nodes[(level_offset(l) + c) * kNodeFloats];
      const Sum& w = want[c];
      bool ok = node_count(g) == w.count && g[11] == 0.f && g[15] == 0.f;
      const double tol = 1e-5 * (w.area * (1. + scale) + 1e-30);
      ok = ok && fabs(g[0] - w.area) <= tol;
      for (int a = 0; a < 3; ++a) {
        ok = ok && fabs(g[1 + a] - w.c[a]) <= tol && fabs(g[4 + a] - w.N[a]) <= tol;
        ok = ok && g[8 + a] == (w.count ? w.lo[a] : 0.f) && g[12 + a] == (w.count ? w.hi[a] : 0.f);
      }
      bad_nodes += !ok;
    }
  }

  // ---- queries: inside the cube, far outside it, on a vertex, not finite
  std::vector<float> q;
  for (int t = 0; t < 40; ++t)
    for (int a = 0; a < 3; ++a) q.push_back((a == 0 ? ox : a == 1 ? oy : oz) + side * rnd());
  for (int t = 0; t < 12; ++t)
    for (int a = 0; a < 3; ++a) q.push_back((a == 0 ? ox : a == 1 ? oy : oz) + side * (rnd() * 9.f - 4.f));
  for (int a = 0; a < 3; ++a) q.push_back(m.v[3 * 2 + a]);
  q.insert(q.end(), {0.5f, NAN, 0.5f});
  q.insert(q.end(), {INFINITY, 0.f, 0.f});
  const int64_t P = (int64_t)q.size() / 3;
  std::vector<int64_t> perm(P);
  for (int64_t t = 0; t < P; ++t) perm[t] = (t * 7 + 3) % P;                       // 7 and P = 55 have no common factor
  std::vector<double> brute(P);
  for (int64_t t = 0; t < P; ++t) {
    double sum = 0.;
    float qx = q[3 * t], qy = q[3 * t + 1], qz = q[3 * t + 2];
    if (!finite3(qx, qy, qz)) qx = qy = qz = NAN;
    for (int64_t k = 0; k < F; ++k) {
      float c[9];
      load_corners(m.v.data(), m.f.data(), V, k, c);
      sum += (double)solid_angle(qx, qy, qz, c);
    }
    brute[t] = sum / kFourPi;
  }
  const float betas[3] = {2.f, 3.f, 1e30f};
  for (float beta : betas) {
    std::vector<double> w(P, -5.), w2(P, -5.);
    blockDim.x = 1; threadIdx.x = 0;
    for (blockIdx.x = 0; blockIdx.x < (unsigned)P + 2; ++blockIdx.x) {
      winding_tree_kernel(q.data(), P, nullptr, levels, nodes.data(), cell_start.data(), tris.data(), n_faces, beta * beta, w.data());
      winding_tree_kernel(q.data(), P, perm.data(), levels, nodes.data(), cell_start.data(), tris.data(), n_faces, beta * beta,
                          w2.data());
    }
    for (int64_t t = 0; t < P; ++t) {
      Walk walk{levels, nodes.data(), cell_start.data(), tris.data(), q[3 * t], q[3 * t + 1], q[3 * t + 2], beta * beta, 0.};
      double want = NAN;
      if (finite3(walk.qx, walk.qy, walk.qz)) {
        walk.visit(0, 0, 0, 0);
        want = walk.sum / kFourPi;
      }
      bad_walk += !same_bits(w[t], want) || !same_bits(w2[t], want);
      if (beta > 1e20f) bad_brute += !(fabs(w[t] - brute[t]) <= 1e-12 || (w[t] != w[t] && brute[t] != brute[t]));
      else bad_brute += !(fabs(w[t] - brute[t]) <= 0.2 || (w[t] != w[t] && brute[t] != brute[t]));   // a dipole sum is near, never wild
    }
  }

  // ---- the exact kernel: its partials and the reduction of the header
  const int64_t chunks = (F + kChunkFaces - 1) / kChunkFaces;
  std::vector<double> partial(chunks * P, -5.), w(P, -5.);
  blockDim.x = 1; threadIdx.x = 0;
  for (blockIdx.y = 0; blockIdx.y < (unsigned)chunks; ++blockIdx.y)
    for (blockIdx.x = 0; blockIdx.x < (unsigned)P + 2; ++blockIdx.x)
      winding_exact_kernel(q.data(), P, m.v.data(), V, m.f.data(), F, partial.data());
  blockIdx.y = 0;
  for (blockIdx.x = 0; blockIdx.x < (unsigned)P + 2; ++blockIdx.x) winding_reduce_kernel(partial.data(), chunks, P, w.data());
  for (int64_t t = 0; t < P; ++t) {
    float qx = q[3 * t], qy = q[3 * t + 1], qz = q[3 * t + 2];
    if (!finite3(qx, qy, qz)) qx = qy = qz = NAN;
    double total = 0.;
    for (int64_t c = 0; c < chunks; ++c) {
      double sum = 0.;
      for (int64_t k = c * kChunkFaces; k < F && k < (c + 1) * kChunkFaces; ++k) {
        float cc[9];
        load_corners(m.v.data(), m.f.data(), V, k, cc);
        sum += (double)solid_angle(qx, qy, qz, cc);
      }
      bad_exact += !same_bits(partial[c * P + t], sum);
      total += sum;
    }
    bad_exact += !same_bits(w[t], total / kFourPi);
    bad_exact += !(fabs(w[t] - brute[t]) <= 1e-12 || (w[t] != w[t] && brute[t] != brute[t]));
  }
  const int64_t bad = bad_cells + bad_nodes + bad_walk + bad_brute + bad_exact;
  printf("%s: %lld faces (%lld binned), levels %d, %lld queries, %lld chunks: cells %lld, nodes %lld, walk %lld, brute %lld, exact %lld "
         "-> %lld mismatches\n", name, (long long)F, (long long)n_faces, levels, (long long)P, (long long)chunks, (long long)bad_cells,
         (long long)bad_nodes, (long long)bad_walk, (long long)bad_brute, (long long)bad_exact, (long long)bad);
  return bad != 0;
}

int main() {
  int fails = 0;
  const Mesh fill = soup(400, 0.05f, 0.9f, 0.08f, false), tiny = soup(30, 0.501f, 0.004f, 0.002f, false),
             broken = soup(200, 0.1f, 0.8f, 0.1f, true), large = soup(9000, 0.1f, 0.8f, 0.03f, false);
  fails += check("fills the cube, levels 3", fill, 3, 0.f, 0.f, 0.f, 1.f);
  fails += check("levels 1", fill, 1, 0.f, 0.f, 0.f, 1.f);
  fails += check("levels 5", fill, 5, 0.f, 0.f, 0.f, 1.f);
  fails += check("inside one finest cell", tiny, 4, 0.f, 0.f, 0.f, 1.f);
  fails += check("invalid indices and faces without area", broken, 3, 0.f, 0.f, 0.f, 1.f);
  fails += check("a cube smaller than the mesh", fill, 2, 0.3f, 0.3f, 0.3f, 0.4f);
  fails += check("more than two chunks", large, 4, 0.f, 0.f, 0.f, 1.f);
  printf(fails ? "FAILED\n" : "all ok\n");
  return fails != 0;
}
