// Host check of csrc/segment_mesh.hip: the one-lane grid kernel compiled for the CPU (the stand-in common.h of
// tools/host_check: one lane per wave, kernels called as functions), in both modes, compared bit for bit (face, the
// bits of t, count) with a loop over seg_face_hit — what the brute-force kernel runs for every face — on nine meshes and
// grids, with segments chosen to reach every branch of the walk, and on two families of small scenes under random rigid
// motions that the f32 determinants cannot decide, under the host's sanitizers.  grid.inc / segment.inc are
// csrc/mesh_grid.hip and csrc/segment_mesh.hip up to their `using namespace recmv;` line (tests/host_check.py builds it).
#define __fmul_rn(a, b) ((float)(a) * (float)(b))
#define __fsub_rn(a, b) ((float)(a) - (float)(b))
#define __fadd_rn(a, b) ((float)(a) + (float)(b))
#define __fdiv_rn(a, b) ((float)(a) / (float)(b))
#include "common.h"
using std::min;
#include "grid.inc"
#include "segment.inc"
#include <map>
#include <random>
#include <vector>
using namespace recmv;
static std::mt19937 rng(13);
static float U(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }
struct Mesh { std::vector<float> v; std::vector<int64_t> f; };

static Mesh icosphere(int level, float radius) {
  const float t = (1.f + sqrtf(5.f)) / 2.f;
  Mesh m;
  const float v0[12][3] = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t}, {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
  const int f0[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                         {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  for (auto& p : v0) m.v.insert(m.v.end(), {p[0], p[1], p[2]});
  for (auto& f : f0) m.f.insert(m.f.end(), {f[0], f[1], f[2]});
  for (int l = 0; l < level; ++l) {
    std::map<std::pair<int64_t, int64_t>, int64_t> mid;
    auto midpoint = [&](int64_t a, int64_t b) {
      auto key = std::make_pair(std::min(a, b), std::max(a, b));
      auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      for (int c = 0; c < 3; ++c) m.v.push_back(0.5f * (m.v[3 * a + c] + m.v[3 * b + c]));
      return mid[key] = (int64_t)m.v.size() / 3 - 1;
    };
    std::vector<int64_t> nf;
    for (size_t k = 0; k < m.f.size(); k += 3) {
      int64_t a = m.f[k], b = m.f[k + 1], c = m.f[k + 2], ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
      nf.insert(nf.end(), {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca});
    }
    m.f = nf;
  }
  for (size_t i = 0; i < m.v.size(); i += 3) {
    float n = sqrtf(m.v[i] * m.v[i] + m.v[i + 1] * m.v[i + 1] + m.v[i + 2] * m.v[i + 2]);
    for (int c = 0; c < 3; ++c) m.v[i + c] *= radius / n;
  }
  return m;
}

// the segment set of every run: p and q interleaved
static std::vector<float> segments(const Mesh& m, const float lo[3], const float hi[3], float h, int nx, int ny, int nz) {
  std::vector<float> s;
  auto add = [&](float a, float b, float c, float d, float e, float f) { s.insert(s.end(), {a, b, c, d, e, f}); };
  float ext[3] = {hi[0] - lo[0] + 1e-3f, hi[1] - lo[1] + 1e-3f, hi[2] - lo[2] + 1e-3f};
  auto R = [&](int c, float a, float b) { return lo[c] + U(a, b) * ext[c]; };
  for (int i = 0; i < 700; ++i) add(R(0, -.3f, 1.3f), R(1, -.3f, 1.3f), R(2, -.3f, 1.3f), R(0, -.3f, 1.3f), R(1, -.3f, 1.3f), R(2, -.3f, 1.3f));
  for (int i = 0; i < 300; ++i) {                           // short ones
    float x = R(0, 0, 1), y = R(1, 0, 1), z = R(2, 0, 1), l = 0.08f;
    add(x, y, z, x + U(-l, l) * ext[0], y + U(-l, l) * ext[1], z + U(-l, l) * ext[2]);
  }
  for (int i = 0; i < 240; ++i) {                           // one or two direction components exactly 0
    float x = R(0, -.2f, 1.2f), y = R(1, -.2f, 1.2f), z = R(2, -.2f, 1.2f), q[3] = {x, y, z};
    q[i % 3] = R(i % 3, -.2f, 1.2f);
    if (i % 2) q[(i + 1) % 3] = R((i + 1) % 3, -.2f, 1.2f);
    add(x, y, z, q[0], q[1], q[2]);
  }
  for (int i = 0; i < 240; ++i) {                           // in a cell-boundary plane, along cell edges, through cell corners
    int n[3] = {nx, ny, nz};
    float a[3], b[3];
    for (int c = 0; c < 3; ++c) { a[c] = R(c, -.1f, 1.1f); b[c] = R(c, -.1f, 1.1f); }
    int c = i % 3;
    a[c] = b[c] = lo[c] + (float)(rng() % (n[c] + 1)) * h;
    if (i % 4 == 1) { int e = (c + 1) % 3; a[e] = b[e] = lo[e] + (float)(rng() % (n[e] + 1)) * h; }
    if (i % 4 == 2) for (int e = 0; e < 3; ++e) { a[e] = lo[e] + (float)(rng() % (n[e] + 1)) * h; b[e] = lo[e] + (float)(rng() % (n[e] + 1)) * h; }
    add(a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  for (int i = 0; i < 200; ++i) {                           // from outside in, from inside out, wholly outside, far away
    float a[3], b[3];
    for (int c = 0; c < 3; ++c) { a[c] = R(c, 0, 1); b[c] = R(c, 0, 1); }
    int c = i % 3;
    float far = i % 5 == 0 ? 1e4f : 3.f;
    if (i % 4 == 0) a[c] = lo[c] - far * ext[c];
    else if (i % 4 == 1) b[c] = hi[c] + far * ext[c];
    else if (i % 4 == 2) { a[c] = hi[c] + 0.5f * ext[c]; b[c] = hi[c] + far * ext[c]; }
    else { a[c] = lo[c] - far * ext[c]; b[c] = hi[c] + far * ext[c]; }
    add(a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  int64_t V = m.v.size() / 3, F = m.f.size() / 3;
  for (int i = 0; i < 300 && F; ++i) {                      // through faces, vertices and edges of the mesh; in a face's plane
    int64_t k = rng() % F, ia = m.f[3 * k], ib = m.f[3 * k + 1], ic = m.f[3 * k + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) continue;
    const float *a = &m.v[3 * ia], *b = &m.v[3 * ib], *c = &m.v[3 * ic];
    float wa = U(0, 1), wb = U(0, 1 - wa), wc = 1 - wa - wb;
    if (i % 6 == 1) { wa = 1; wb = wc = 0; }
    if (i % 6 == 2) { wc = 0; wb = 1 - wa; }
    float x[3], d[3];
    for (int e = 0; e < 3; ++e) { x[e] = wa * a[e] + wb * b[e] + wc * c[e]; d[e] = U(-.3f, .3f) * ext[e]; }
    if (i % 6 == 3) for (int e = 0; e < 3; ++e) d[e] = b[e] - a[e];              // in the plane
    if (i % 6 == 4) add(x[0], x[1], x[2], x[0] + d[0], x[1] + d[1], x[2] + d[2]);  // an endpoint in the plane
    else add(x[0] - d[0], x[1] - d[1], x[2] - d[2], x[0] + d[0], x[1] + d[1], x[2] + d[2]);
  }
  for (int i = 0; i < 40; ++i) { float x = R(0, -.2f, 1.2f), y = R(1, -.2f, 1.2f), z = R(2, -.2f, 1.2f); add(x, y, z, x, y, z); }   // no length
  for (int i = 0; i < 40; ++i) {                            // hardly any length
    float x = R(0, 0, 1), y = R(1, 0, 1), z = R(2, 0, 1);
    add(x, y, z, nextafterf(x, 9.f), i % 2 ? y : nextafterf(y, -9.f), z);
  }
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
  for (int i = 0; i < 36; ++i) {
    float a[6] = {R(0, 0, 1), R(1, 0, 1), R(2, 0, 1), R(0, 0, 1), R(1, 0, 1), R(2, 0, 1)};
    a[i % 6] = i < 12 ? nan : (i < 24 ? inf : (i < 30 ? -inf : 3e38f));
    if (i >= 30) a[(i + 3) % 6] = -3e38f;
    add(a[0], a[1], a[2], a[3], a[4], a[5]);
  }
  return s;
}

struct Tally { int64_t hits = 0, multi = 0, sum = 0, S = 0, ungated = 0, clamped = 0, late = 0; float h = 0; };

// the grid over m and `seg` (p and q interleaved) through it, both modes, against the brute loop: the number of mismatches
static int compare(const char* name, const Mesh& m, int nx, int ny, int nz, float h_force, bool shuffle, bool own_segments,
                   std::vector<float> seg, Tally& ty) {
  int64_t V = m.v.size() / 3, F = m.f.size() / 3;
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (int64_t i = 0; i < V; ++i) for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], m.v[3 * i + c]); hi[c] = fmaxf(hi[c], m.v[3 * i + c]); }
  float h = h_force;
  if (h <= 0) { h = 1e-30f; int n[3] = {nx, ny, nz}; for (int c = 0; c < 3; ++c) h = fmaxf(h, (hi[c] - lo[c]) / n[c] * 1.000001f); }
  Grid g{lo[0], lo[1], lo[2], h, 1.f / h, nx, ny, nz};
  int64_t cells = (int64_t)nx * ny * nz;
  std::vector<int32_t> counts(cells, 0), offsets(cells + 1, 0), cursor(cells, 0);
  unsigned long long total = 0;
  blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0};
  grid_count_kernel(m.v.data(), V, m.f.data(), F, g, counts.data(), &total);
  int64_t sum = 0; for (int64_t c = 0; c < cells; ++c) { offsets[c] = (int32_t)sum; cursor[c] = (int32_t)sum; sum += counts[c]; }
  offsets[cells] = (int32_t)sum;
  std::vector<int32_t> entries(std::max<int64_t>(sum, 1), -7);                     // exactly the capacity: ASan guards the ends
  std::vector<float4> tris(3 * F);
  grid_fill_kernel(m.v.data(), V, m.f.data(), F, g, offsets.data(), cursor.data(), entries.data(), sum, tris.data());
  if (shuffle) for (int64_t c = 0; c < cells; ++c) std::shuffle(entries.begin() + offsets[c], entries.begin() + offsets[c + 1], rng);
  float glo[3] = {lo[0], lo[1], lo[2]}, ghi[3] = {lo[0] + nx * h, lo[1] + ny * h, lo[2] + nz * h};
  if (!own_segments) seg = segments(m, glo, ghi, h, nx, ny, nz);
  int64_t S = seg.size() / 6;
  std::vector<float> p(3 * S), q(3 * S);
  for (int64_t i = 0; i < S; ++i) for (int c = 0; c < 3; ++c) { p[3 * i + c] = seg[6 * i + c]; q[3 * i + c] = seg[6 * i + 3 + c]; }
  int bad = 0;
  for (int mode = 0; mode < 2; ++mode) {
    std::vector<int64_t> face(S, -9);                       // exactly S: ASan guards the ends
    std::vector<float> t(S, -9.f);
    std::vector<int32_t> count(S, -9);
    for (int64_t i = 0; i < S; ++i) {
      blockIdx.x = (unsigned)(i / 256); threadIdx.x = (unsigned)(i % 256);
      segment_grid_kernel<1>(p.data(), q.data(), S, m.v.data(), V, m.f.data(), F, GridView{g, offsets.data(), entries.data(), sum},
                             mode, face.data(), t.data(), mode ? count.data() : nullptr);
      const Seg s = seg_make(p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
      float best = __builtin_inff(); int bidx = -1; int32_t n = 0;
      if (s.ok) for (int64_t j = 0; j < F; ++j) {
        float tt;
        if (seg_face_hit(s, m.v.data(), m.f.data(), V, j, tt)) { ++n; seg_take_min(tt, (int)j, best, bidx); }
        if (!mode) continue;
        Pts c; int64_t i0, i1, i2;                          // what the gate and the clamp did, for the summary lines
        if (!load_pts(m.v.data(), m.f.data(), V, j, c, i0, i1, i2)) continue;
        const float sp = orient3(c.ax, c.ay, c.az, c.bx, c.by, c.bz, c.cx, c.cy, c.cz, s.px, s.py, s.pz);
        const float sq = orient3(c.ax, c.ay, c.az, c.bx, c.by, c.bz, c.cx, c.cy, c.cz, s.qx, s.qy, s.qz);
        const bool raw = opposite(sp, sq) && edge_inside(s.px, s.py, s.pz, s.qx, s.qy, s.qz, c);
        if (!raw) continue;
        const float traw = sp / (sp - sq);
        if (!seg_box_gate(s, c)) ++ty.ungated;
        else if (seg_tri_hit(s, c, tt) && memcmp(&traw, &tt, 4) != 0) ++ty.clamped;
      }
      const float bt = bidx >= 0 ? best : __builtin_nanf("");
      if (mode) { ty.hits += n > 0; ty.multi += n > 1; ty.late += n > 1 && bidx != 2; }
      const bool ok = face[i] == bidx && memcmp(&bt, &t[i], 4) == 0 && (!mode || count[i] == n);
      if (!ok && bad++ < 5)
        printf("%s: mode %d segment %lld (%g %g %g)-(%g %g %g): grid face %lld t %.9g count %d, brute face %d t %.9g count %d\n", name, mode,
               (long long)i, p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2], (long long)face[i], t[i],
               mode ? count[i] : -1, bidx, bt, n);
    }
  }
  ty.sum += sum; ty.S += S; ty.h = h;
  return bad;
}

static int run(const char* name, const Mesh& m, int nx, int ny, int nz, float h_force, bool shuffle) {
  Tally ty;
  int bad = compare(name, m, nx, ny, nz, h_force, shuffle, false, {}, ty);
  printf("%s: dims %dx%dx%d h %g, %lld faces, %lld entries, %lld segments (%lld hit, %lld more than one face), %d mismatches\n", name,
         nx, ny, nz, ty.h, (long long)(m.f.size() / 3), (long long)ty.sum, (long long)ty.S, (long long)ty.hits, (long long)ty.multi, bad);
  return bad != 0;
}

// a random rigid motion (rotation about a random axis, then a shift) of the points of m, rounded to f32
static void move_rigidly(std::vector<float>& x, float shift) {
  double a[3] = {U(-1, 1), U(-1, 1), U(-1, 1)}, n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) + 1e-30, w = U(0, 6.2831853f);
  for (double& c : a) c /= n;
  double c = cos(w), s = sin(w), t[3] = {U(-shift, shift), U(-shift, shift), U(-shift, shift)};
  double R[3][3] = {{c + a[0] * a[0] * (1 - c), a[0] * a[1] * (1 - c) - a[2] * s, a[0] * a[2] * (1 - c) + a[1] * s},
                    {a[1] * a[0] * (1 - c) + a[2] * s, c + a[1] * a[1] * (1 - c), a[1] * a[2] * (1 - c) - a[0] * s},
                    {a[2] * a[0] * (1 - c) - a[1] * s, a[2] * a[1] * (1 - c) + a[0] * s, c + a[2] * a[2] * (1 - c)}};
  for (size_t i = 0; i < x.size(); i += 3) {
    double v[3] = {x[i], x[i + 1], x[i + 2]};
    for (int r = 0; r < 3; ++r) x[i + r] = (float)(R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] + t[r]);
  }
}

// A face that holds the segment's line, late in the walk, behind a clean hit: sp and sq of that face are rounding noise, so
// the quotient sp / (sp - sq) of a pair the predicate accepts says nothing about where the face is; seg_clamp_t keeps the
// reported t at the face, and the first-hit walk may stop at the clean hit.  Face 2 is the clean one, at t = 0.21; faces 0
// and 1 hold the line between 0.7 and 0.95 of its length.  Every coordinate stays below 1.2 in magnitude.
static int coplanar_scenes(int trials) {
  Tally ty;
  int bad = 0;
  for (int n = 0; n < trials; ++n) {
    float w = U(0, 6.2831853f), cy = cosf(w), cz = sinf(w);  // the direction across the line, in the coplanar faces' plane
    std::vector<float> x = {0.4f, -0.2f * cy, -0.2f * cz, 0.9f, -0.1f * cy, -0.1f * cz, 0.65f, 0.3f * cy, 0.3f * cz, 0.95f, 0.25f * cy, 0.25f * cz,
                            -0.58f, -0.3f, -0.3f, -0.58f, 0.4f, -0.2f, -0.58f, 0.f, 0.5f,
                            -1, 0, 0, 1, 0, 0, -0.8f, 0, 0, 0.97f, 0, 0, -1, 0, 0, 0.8f, 0, 0};
    move_rigidly(x, 0.15f);
    Mesh m;
    m.v.assign(x.begin(), x.begin() + 21);
    m.f = {0, 1, 2, 1, 3, 2, 4, 5, 6};
    std::vector<float> seg(x.begin() + 21, x.end());
    bad += compare("coplanar face behind a hit 24^3", m, 24, 24, 24, 0, false, true, seg, ty);
  }
  printf("coplanar face behind a hit 24^3: %d scenes, %lld segments (%lld hit, %lld hit a coplanar face besides the clean one, %lld of "
         "those in front of it by their t; %lld quotients clamped), %d mismatches\n", trials, (long long)ty.S, (long long)ty.hits,
         (long long)ty.multi, (long long)ty.late, (long long)ty.clamped, bad);
  if (ty.multi < 20) { printf("coplanar face behind a hit: too few undecidable pairs accepted to show anything\n"); return 1; }
  return bad != 0;
}

// Tiny segments in the plane of a huge face, far from it.  The plane is x = 3 y and every point has x = 3 y exactly (y a
// multiple of 2^-10 below 2^10), so all five determinants of a pair are 0 in exact arithmetic while their f32 products round
// differently: pure noise, and the bare predicate accepts many such pairs.  A grid has no reason to bring a segment
// together with a face whose box is far from it (a small second face far away makes the grid cover the segments), so
// seg_box_gate, in front of the predicate in both kernels, is what keeps them in agreement: the pairs the bare predicate
// accepts and the gate refuses are counted, and there must be some for the run to show it.
static int gate_scenes(int trials) {
  Tally ty;
  int bad = 0;
  auto Y = [](float a, float b) { return floorf(U(a, b) * 1024.f) / 1024.f; };
  for (int n = 0; n < trials; ++n) {
    Mesh m;
    for (int i = 0; i < 3; ++i) { float y = Y(-60, 60) + (i == 1 ? 40 : 0), z = U(-60, 60) + (i == 2 ? 40 : 0); m.v.insert(m.v.end(), {3 * y, y, z}); }
    for (int i = 0; i < 3; ++i) { float y = Y(600, 605), z = U(600, 605); m.v.insert(m.v.end(), {3 * y, y, z}); }
    m.f = {0, 1, 2, 3, 4, 5};
    std::vector<float> seg;
    for (int i = 0; i < 12; ++i) {                          // in and around the huge face's box, and up to 5 extents away
      float r = i % 2 ? 600.f : 150.f, y = Y(-r, r), z = U(-r, r), y2 = y + (float)((int)(rng() % 17) - 8) / 1024.f, z2 = z + U(-.01f, .01f);
      seg.insert(seg.end(), {3 * y, y, z, 3 * y2, y2, z2});
    }
    bad += compare("tiny segments far from a huge face 16^3", m, 16, 16, 16, 0, false, true, seg, ty);
  }
  printf("tiny segments far from a huge face 16^3: %d scenes, %lld segments (%lld hit; %lld pairs accepted by the bare predicate and "
         "refused by the gate), %d mismatches\n", trials, (long long)ty.S, (long long)ty.hits, (long long)ty.ungated, bad);
  if (ty.ungated < 20) { printf("tiny segments far from a huge face: the gate refused too few accepted pairs to show anything\n"); return 1; }
  return bad != 0;
}

int main() {
  int rc = 0;
  Mesh ico = icosphere(3, 0.5f);                            // 1280 faces
  for (size_t i = 0; i < ico.v.size(); ++i) ico.v[i] *= 1.f + 0.03f * sinf(7.f * ico.v[(i / 3) * 3]);
  int64_t nv = ico.v.size() / 3;
  Mesh messy = ico;                                         // duplicates, faces without area, invalid faces
  for (int i = 0; i < 10; ++i) for (int k = 0; k < 3; ++k) messy.f.push_back(messy.f[3 * (i * 7) + k]);
  messy.f.insert(messy.f.end(), {5, 5, 9, 7, 11, 11, 4, 4, 4, nv, 1, 2, -1, 2, 3, 0, 1, nv + 5});
  rc |= run("icosphere 11^3", messy, 11, 11, 11, 0, false);
  rc |= run("icosphere 11^3 shuffled entries", messy, 11, 11, 11, 0, true);
  rc |= run("single cell", messy, 1, 1, 1, 0, false);
  rc |= run("column 1x1x17", messy, 1, 1, 17, 0, false);
  rc |= run("31x2x7", messy, 31, 2, 7, 0, true);
  Mesh two; two.v = ico.v; two.f.assign(ico.f.begin(), ico.f.begin() + 6);
  rc |= run("two faces 40^3", two, 40, 40, 40, 0, false);
  rc |= run("grid does not cover 40^3", messy, 40, 40, 40, 0.01f, false);
  Mesh flat;
  for (int i = 0; i <= 8; ++i) for (int j = 0; j <= 8; ++j) flat.v.insert(flat.v.end(), {j / 8.f + U(-.01f, .01f), i / 8.f + U(-.01f, .01f), 0.25f});
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { int64_t a = i * 9 + j; flat.f.insert(flat.f.end(), {a, a + 1, a + 9, a + 1, a + 10, a + 9}); }
  rc |= run("planar 7x7x1", flat, 7, 7, 1, 0, false);
  Mesh huge = messy;
  huge.v.insert(huge.v.end(), {-1, -1, -1, 1, -1, 1, -1, 1, 1});
  huge.f.insert(huge.f.begin(), {nv, nv + 1, nv + 2}); huge.f.insert(huge.f.end(), {nv, nv + 1, nv + 2});
  rc |= run("a face in every cell 12^3", huge, 12, 12, 12, 0, true);
  rc |= coplanar_scenes(6000);
  rc |= gate_scenes(1500);
  printf(rc ? "FAILED\n" : "all ok\n");
  return rc;
}
