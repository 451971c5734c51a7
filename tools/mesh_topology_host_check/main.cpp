// Host check of csrc/mesh_topology.hip: its kernels compiled for the CPU (the stand-in common.h of tools/host_check: one lane
// per wave, kernels called as functions, one thread after the other; the integer minimum and the relaxed loads and stores of
// the compression are plain ones there) under the host's sanitizers.  topology.inc is csrc/mesh_topology.hip up to its
// `using namespace recmv;` line (tests/host_check.py builds it; tests/test_mesh_topology_cpu.py runs it).
//   * components: the rounds run serially until a round hooks nothing; the labels against a plain union-find (smallest member),
//     the number of rounds against a plain restatement of the synchronous algorithm (every root takes the smallest root among
//     its neighbour trees, then every node its tree's root) and against the cap 2 ceil(log2 n) + 2.
//   * face figures against plain loops; segment sums against plain loops.
#include "topology.inc"
#include <numeric>
#include <random>
#include <vector>
using namespace recmv;
typedef std::vector<int64_t> Links;
static std::mt19937 rng(29);

static int cap_of(int64_t n) { int l = 0; while ((1ll << l) < n) ++l; return 2 * l + 2; }

static bool row_ok(const int64_t* r, int K, int64_t n) {
  for (int k = 0; k < K; ++k) if (r[k] < 0 || r[k] >= n) return false;
  if (r[0] == r[1]) return false;
  return K == 2 || (r[0] != r[2] && r[1] != r[2]);
}

// smallest member of every component by union-find
static std::vector<int32_t> union_find(int64_t n, const Links& l, int K, int64_t& invalid) {
  std::vector<int32_t> p(n);
  std::iota(p.begin(), p.end(), 0);
  auto find = [&](int32_t x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; };
  invalid = 0;
  for (size_t i = 0; i + K <= l.size(); i += K) {
    if (!row_ok(&l[i], K, n)) { ++invalid; continue; }
    for (int k = 1; k < K; ++k) {
      int32_t a = find((int32_t)l[i]), b = find((int32_t)l[i + k]);
      if (a != b) p[std::max(a, b)] = std::min(a, b);      // the smaller id stays the root
    }
  }
  std::vector<int32_t> out(n);
  for (int64_t i = 0; i < n; ++i) out[i] = find((int32_t)i);
  return out;
}

// the synchronous algorithm restated: the number of rounds until one hooks nothing (that round included)
static int plain_rounds(int64_t n, const Links& l, int K) {
  std::vector<int32_t> label(n), parent(n);
  std::iota(label.begin(), label.end(), 0);
  for (int round = 1;; ++round) {
    std::iota(parent.begin(), parent.end(), 0);
    bool hooked = false;
    for (size_t i = 0; i + K <= l.size(); i += K) {
      if (!row_ok(&l[i], K, n)) continue;
      int32_t m = label[l[i]];
      for (int k = 1; k < K; ++k) m = std::min(m, label[l[i + k]]);
      for (int k = 0; k < K; ++k) { int32_t r = label[l[i + k]]; if (r != m) { parent[r] = std::min(parent[r], m); hooked = true; } }
    }
    if (!hooked) return round;
    for (int64_t r = 0; r < n; ++r) parent[r] = parent[parent[r]];                // parent[r] <= r: ascending, every chain is done
    for (int64_t x = 0; x < n; ++x) label[x] = parent[label[x]];
  }
}

static int components(const char* name, int64_t n, const Links& l, int K) {
  const int64_t M = (int64_t)l.size() / K;
  int64_t invalid = 0;
  const std::vector<int32_t> want = union_find(n, l, K, invalid);
  std::vector<int32_t> label(std::max<int64_t>(n, 1), -5), parent(std::max<int64_t>(n, 1), -5);
  int32_t state[4] = {-1, -1, -1, -1};
  blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0};
  const int cap = cap_of(n);
  int rounds = 0;
  if (n > 0 && M > 0) {                                    // (the entry point returns before any launch otherwise)
    components_init_kernel(n, label.data(), parent.data(), state);
    for (;;) {
      ++rounds;
      if (K == 2) components_hook_kernel<2>(n, l.data(), M, label.data(), parent.data(), state, rounds, rounds == 1);
      else components_hook_kernel<3>(n, l.data(), M, label.data(), parent.data(), state, rounds, rounds == 1);
      components_compress_kernel(n, label.data(), parent.data());
      if (state[0] < rounds) break;
      if (rounds > cap) { printf("%s: more than %d rounds\n", name, cap); return 1; }
    }
  } else {
    std::iota(label.begin(), label.begin() + n, 0);
    state[1] = 0;
    rounds = 1;
  }
  int64_t bad = 0;
  for (int64_t i = 0; i < n; ++i) bad += label[i] != want[i];
  const int plain = plain_rounds(n, l, K);
  const bool ok = bad == 0 && rounds == plain && rounds <= cap && (M == 0 || n == 0 || state[1] == invalid);
  printf("%s: n %lld, %lld rows of %d, %lld invalid, %d rounds (plain %d, cap %d), %lld mismatches%s\n", name, (long long)n,
         (long long)M, K, (long long)invalid, rounds, plain, cap, (long long)bad, ok ? "" : "  <-- WRONG");
  return ok ? 0 : 1;
}

static std::vector<int64_t> numbering(int64_t n, int kind) {                      // 0 ascending, 1 descending, 2 random
  std::vector<int64_t> p(n);
  std::iota(p.begin(), p.end(), 0);
  if (kind == 1) std::reverse(p.begin(), p.end());
  if (kind == 2) std::shuffle(p.begin(), p.end(), rng);
  return p;
}

// a strip of F triangles over F + 2 vertices: faces (i, i + 1, i + 2) under a numbering
static Links strip(int64_t F, int kind, int K) {
  const std::vector<int64_t> p = numbering(F + 2, kind);
  Links l;
  for (int64_t i = 0; i < F; ++i) {
    if (K == 3) l.insert(l.end(), {p[i], p[i + 1], p[i + 2]});
    else l.insert(l.end(), {p[i], p[i + 1], p[i + 1], p[i + 2], p[i + 2], p[i]});
  }
  return l;
}

static Links path(int64_t n, int kind) {
  const std::vector<int64_t> p = numbering(n, kind);
  Links l;
  for (int64_t i = 0; i + 1 < n; ++i) l.insert(l.end(), {p[i], p[i + 1]});
  return l;
}

static Links icosphere_faces(int level, int64_t& V) {
  const int f0[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                         {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  Links f;
  for (auto& t : f0) f.insert(f.end(), {t[0], t[1], t[2]});
  V = 12;
  for (int l = 0; l < level; ++l) {
    std::vector<std::pair<std::pair<int64_t, int64_t>, int64_t>> mids;
    auto mid = [&](int64_t a, int64_t b) {
      const auto key = std::make_pair(std::min(a, b), std::max(a, b));
      for (auto& m : mids) if (m.first == key) return m.second;
      mids.push_back({key, V});
      return V++;
    };
    Links nf;
    for (size_t k = 0; k < f.size(); k += 3) {
      const int64_t a = f[k], b = f[k + 1], c = f[k + 2], ab = mid(a, b), bc = mid(b, c), ca = mid(c, a);
      nf.insert(nf.end(), {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca});
    }
    f = nf;
  }
  return f;
}

static int face_stats() {
  // a right triangle, an equilateral one, a sliver, a repeated point, three corners in a line, invalid rows, a NaN and an inf
  // (point 9 is a second point at the origin: a valid face with an edge of length 0)
  std::vector<float> v = {0, 0, 0, 3, 0, 0, 0, 4, 0, 1, 0, 0, 0.5f, 0.8660254f, 0, 1e-3f, 1, 7, 2, 0, 0, NAN, 0, 0, INFINITY, 1, 1, 0, 0, 0};
  const int64_t V2 = (int64_t)v.size() / 3;
  Links f = {0, 1, 2, 0, 3, 4, 0, 1, 5, 0, 0, 1, 0, 3, 6, 0, 1, V2, -1, 1, 2, 0, 3, 7, 0, 8, 3, 0, 3, 6, 3, 0, 6, 0, 6, 3, 0, 9, 1};
  const int64_t F = (int64_t)f.size() / 3;
  std::vector<double> area(F, -1), ang(F, -1), ratio(F, -1);
  int32_t counts[2] = {0, 0};
  blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0};
  face_stats_kernel(v.data(), V2, f.data(), F, area.data(), ang.data(), ratio.data(), counts);
  int bad = 0;
  auto near = [](double a, double b) { return fabs(a - b) <= 1e-12 * (1 + fabs(b)); };
  bad += !(near(area[0], 6) && near(ang[0], atan2(3., 4.)) && near(ratio[0], 5. / 3.));
  bad += !(fabs(area[1] - 0.25 * sqrt(3.)) < 1e-7 && fabs(ang[1] - M_PI / 3) < 1e-7 && fabs(ratio[1] - 1) < 1e-7);
  bad += !(area[3] == 0 && std::isnan(ang[3]) && std::isnan(ratio[3]));          // (0, 0, 1): invalid
  bad += !(area[4] == 0 && ang[4] == 0 && near(ratio[4], 2));                     // three corners in a line
  bad += !(area[5] == 0 && std::isnan(ang[5]) && area[6] == 0 && std::isnan(ratio[6]));
  bad += !(std::isnan(area[7]) && std::isnan(ang[7]) && std::isnan(ratio[7]));    // NaN corner
  bad += !(std::isnan(area[8]) && std::isnan(ang[8]) && std::isnan(ratio[8]));    // inf corner
  bad += !(area[F - 1] == 0 && ang[F - 1] == 0 && std::isinf(ratio[F - 1]));      // an edge of length 0
  bad += !(counts[0] == 3 && counts[1] == 2);
  for (int64_t k = 0; k < F; ++k) {                         // the smallest of three angles that add up to pi
    if (!(area[k] > 0)) continue;
    if (!(ang[k] > 0 && ang[k] <= M_PI / 3 + 1e-12 && ratio[k] >= 1)) ++bad;
  }
  for (int64_t k = 0; k < F && bad; ++k) printf("  face %lld: area %.17g angle %.17g ratio %.17g\n", (long long)k, area[k], ang[k], ratio[k]);
  printf("face figures: %lld faces, %d invalid, %d not finite, %d mismatches\n", (long long)F, counts[0], counts[1], bad);
  return bad != 0;
}

static int segment_sums() {
  const int C = 3;
  const std::vector<int64_t> lens = {0, 1, 5, kSegChunk, kSegChunk + 1, 0, 3 * kSegChunk + 5, 63, 64, 65, 0};
  const int64_t S = (int64_t)lens.size();
  std::vector<int64_t> off(S + 1, 0), coff(S + 1, 0);
  for (int64_t s = 0; s < S; ++s) { off[s + 1] = off[s] + lens[s]; coff[s + 1] = coff[s] + (lens[s] + kSegChunk - 1) / kSegChunk; }
  const int64_t N = off[S], max_chunks = S + N / kSegChunk;
  std::vector<double> x(N * C);
  std::uniform_real_distribution<double> U(-1., 3.);
  for (auto& t : x) t = U(rng);
  std::vector<double> partial(max_chunks * C * 3, NAN), sum(S * C, NAN), lo(S * C, NAN), hi(S * C, NAN);
  blockDim = {1, 1, 1}; gridDim = {1, 1, 1};
  for (int64_t w = 0; w < max_chunks; ++w) {               // one-lane waves: thread w is wave w
    blockIdx.x = (unsigned)w; threadIdx.x = 0;
    segment_chunks_kernel(x.data(), N, C, off.data(), S, coff.data(), max_chunks, partial.data());
  }
  for (int64_t s = 0; s < S; ++s) {
    blockIdx.x = (unsigned)s; threadIdx.x = 0;
    segment_finish_kernel(partial.data(), max_chunks, C, S, coff.data(), sum.data(), lo.data(), hi.data());
  }
  int bad = 0;
  for (int64_t s = 0; s < S; ++s)
    for (int c = 0; c < C; ++c) {
      double t = 0, a = INFINITY, b = -INFINITY;
      for (int64_t i = off[s]; i < off[s + 1]; ++i) { t += x[i * C + c]; a = std::min(a, x[i * C + c]); b = std::max(b, x[i * C + c]); }
      if (!(fabs(sum[s * C + c] - t) <= 1e-12 * (1 + fabs(t)) && lo[s * C + c] == a && hi[s * C + c] == b)) ++bad;
    }
  // tables that are not what the header describes must stay inside the arrays (the sanitizers watch)
  std::vector<int64_t> wild_off(S + 1), wild_coff(S + 1);
  for (int64_t s = 0; s <= S; ++s) { wild_off[s] = (int64_t)(rng() % (4 * N)) - N; wild_coff[s] = (int64_t)(rng() % (4 * max_chunks)) - max_chunks; }
  for (int64_t w = 0; w < max_chunks; ++w) {
    blockIdx.x = (unsigned)w;
    segment_chunks_kernel(x.data(), N, C, wild_off.data(), S, wild_coff.data(), max_chunks, partial.data());
    segment_chunks_kernel(x.data(), N, C, wild_off.data(), S, coff.data(), max_chunks, partial.data());
  }
  for (int64_t s = 0; s < S; ++s) {
    blockIdx.x = (unsigned)s;
    segment_finish_kernel(partial.data(), max_chunks, C, S, wild_coff.data(), sum.data(), lo.data(), hi.data());
  }
  printf("segment sums: %lld segments of %lld rows in %lld chunks, %d mismatches\n", (long long)S, (long long)N, (long long)coff[S], bad);
  return bad != 0;
}

int main() {
  int rc = 0;
  for (int K = 3; K >= 2; --K) {
    rc |= components("strip 4097 ascending", 4099, strip(4097, 0, K), K);
    rc |= components("strip 4097 descending", 4099, strip(4097, 1, K), K);
    rc |= components("strip 4097 random", 4099, strip(4097, 2, K), K);
  }
  {                                                        // one hub vertex in 5 000 triangles: the last, the first, a middle id
    for (int64_t hub : {(int64_t)10000, (int64_t)0, (int64_t)5000}) {
      Links l;
      for (int64_t i = 0; i < 5000; ++i) { int64_t a = 2 * i, b = 2 * i + 1; if (a >= hub) ++a; if (b >= hub) ++b; l.insert(l.end(), {hub, a, b}); }
      rc |= components("hub of 5000 triangles", 10001, l, 3);
    }
  }
  {
    int64_t V = 0;
    Links l = icosphere_faces(3, V);                        // 1 280 faces
    for (int64_t i = 0; i < 3000; ++i) l.insert(l.end(), {V + 3 * i, V + 3 * i + 1, V + 3 * i + 2});
    rc |= components("body and 3000 isolated triangles", V + 9000 + 7, l, 3);
  }
  {
    const Links all = strip(4097, 2, 2);
    for (int64_t M : {0, 1, 63, 64, 65, 255, 257}) rc |= components("first rows of the strip", 4099, Links(all.begin(), all.begin() + 2 * M), 2);
    const Links all3 = strip(4097, 2, 3);
    for (int64_t M : {1, 65, 257}) rc |= components("first rows of the strip", 4099, Links(all3.begin(), all3.begin() + 3 * M), 3);
  }
  for (int K = 2; K <= 3; ++K) {                            // rows that join nothing
    Links l = strip(600, 2, K);
    const int64_t n = 602;
    const int64_t M = (int64_t)l.size() / K;
    for (int64_t i = 0; i < M; i += 7) {
      int64_t* r = &l[K * i];
      switch ((i / 7) % 4) { case 0: r[0] = -1; break; case 1: r[K - 1] = n; break; case 2: r[1] = r[0]; break; default: r[K - 1] = r[0]; }
    }
    rc |= components("strip with invalid rows", n, l, K);
  }
  for (int kind = 0; kind < 3; ++kind) rc |= components(kind == 0 ? "path 4098 ascending" : kind == 1 ? "path 4098 descending" : "path 4098 random",
                                                        4098, path(4098, kind), 2);
  for (int kind = 0; kind < 3; ++kind) rc |= components(kind == 0 ? "path 200000 ascending" : kind == 1 ? "path 200000 descending" : "path 200000 random",
                                                        200000, path(200000, kind), 2);
  rc |= components("empty", 0, Links(), 2);
  rc |= components("nodes without rows", 17, Links(), 3);
  rc |= components("one node", 1, Links{0, 0}, 2);
  rc |= face_stats();
  rc |= segment_sums();
  printf(rc ? "FAILED\n" : "all ok\n");
  return rc;
}
