// Host check of csrc/mesh_intersect.hip: the one-lane grid kernel compiled for the CPU (the stand-in
// common.h of tools/host_check: one lane per wave, kernels called as functions), count and fill pass, compared as
// integers with a double loop over the brute-force kernel's pair test on random triangle soups and grids, under the host's sanitizers.  grid.inc / intersect.inc are csrc/mesh_grid.hip
// and csrc/mesh_intersect.hip up to their `using namespace recmv;` line (tests/host_check.py builds it).
#define __fmul_rn(a, b) ((float)(a) * (float)(b))
#define __fsub_rn(a, b) ((float)(a) - (float)(b))
#include "grid.inc"
#include "intersect.inc"
#include <vector>
#include <random>
#include <algorithm>
using namespace recmv;
static std::mt19937 rng(11);
static float U(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }
struct Mesh { std::vector<float> v; std::vector<int64_t> f; };
typedef std::vector<std::pair<int, int>> Pairs;

static Mesh soup(int nv, int nf, float size, float ox) {
  Mesh m;
  for (int i = 0; i < nv; ++i) m.v.insert(m.v.end(), {ox + U(-1, 1), U(-1, 1), U(-1, 1)});
  for (int i = 0; i < nf; ++i) {                            // a face around a random vertex: two corners within `size`
    int a = rng() % nv;
    int b = nv + 2 * i, c = b + 1;
    m.f.insert(m.f.end(), {a, b, c});
  }
  for (int i = 0; i < nf; ++i) for (int k = 0; k < 2; ++k) {
    int a = (int)m.f[3 * i];
    m.v.insert(m.v.end(), {m.v[3 * a] + U(-size, size), m.v[3 * a + 1] + U(-size, size), m.v[3 * a + 2] + U(-size, size)});
  }
  int V = (int)m.v.size() / 3;
  m.f.insert(m.f.end(), {5, 5, 9, 7, 11, 11, 4, 4, 4, V, 1, 2, -1, 2, 3});          // without area, invalid
  m.f.insert(m.f.end(), {0, 1, 2});                                                  // one large face
  return m;
}

// both passes of a kernel call `pass(counts, total, sink)`; returns the sorted pairs
template <class Pass>
static int two_passes(const char* name, int64_t FA, Pass pass, Pairs& out) {
  std::vector<int32_t> counts(FA, -3), offsets(FA + 1, 0), cursor(FA, 0);
  unsigned long long total = 0, dropped = 0;
  std::fill(counts.begin(), counts.end(), 0);
  pass(counts.data(), &total, Sink{nullptr, nullptr, nullptr, 0, nullptr});
  int64_t sum = 0;
  for (int64_t i = 0; i < FA; ++i) { offsets[i] = (int32_t)sum; cursor[i] = (int32_t)sum; sum += counts[i]; }
  offsets[FA] = (int32_t)sum;
  if ((unsigned long long)sum != total) { printf("%s: total %llu != sum %lld\n", name, total, (long long)sum); return 1; }
  std::vector<int32_t> pairs(2 * std::max<int64_t>(sum, 1), -7);                    // exactly the capacity: ASan guards the ends
  pass(nullptr, nullptr, Sink{offsets.data(), cursor.data(), pairs.data(), sum, &dropped});
  if (dropped) { printf("%s: %llu dropped\n", name, dropped); return 1; }
  for (int64_t i = 0; i < FA; ++i) if (cursor[i] != offsets[i + 1]) { printf("%s: cursor mismatch\n", name); return 1; }
  out.clear();
  for (int64_t k = 0; k < sum; ++k) out.push_back({pairs[2 * k], pairs[2 * k + 1]});
  std::sort(out.begin(), out.end());
  // half the capacity: nothing beyond it is written (ASan), the rest is reported
  std::vector<int32_t> small(2 * std::max<int64_t>(sum / 2, 1), -7);
  for (int64_t i = 0; i < FA; ++i) cursor[i] = offsets[i];
  dropped = 0;
  pass(nullptr, nullptr, Sink{offsets.data(), cursor.data(), small.data(), sum / 2, &dropped});
  if ((int64_t)dropped != sum - sum / 2) { printf("%s: dropped %llu of %lld\n", name, dropped, (long long)sum); return 1; }
  return 0;
}

static int run(const char* name, const Mesh& a, const Mesh& b, bool self, int nx, int ny, int nz) {
  int64_t VA = a.v.size() / 3, FA = a.f.size() / 3, VB = b.v.size() / 3, FB = b.f.size() / 3;
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (int64_t i = 0; i < VB; ++i) for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], b.v[3 * i + c]); hi[c] = fmaxf(hi[c], b.v[3 * i + c]); }
  float h = 1e-30f; int n[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c) h = fmaxf(h, (hi[c] - lo[c]) / n[c] * 1.000001f);
  Grid g{lo[0], lo[1], lo[2], h, 1.f / h, nx, ny, nz};
  int64_t cells = (int64_t)nx * ny * nz;
  std::vector<int32_t> counts(cells, 0), offsets(cells + 1, 0), cursor(cells, 0);
  unsigned long long total = 0;
  blockDim = {1, 1, 1}; gridDim = {1, 1, 1}; blockIdx = {0, 0, 0}; threadIdx = {0, 0, 0};
  grid_count_kernel(b.v.data(), VB, b.f.data(), FB, g, counts.data(), &total);
  int64_t sum = 0; for (int64_t c = 0; c < cells; ++c) { offsets[c] = (int32_t)sum; cursor[c] = (int32_t)sum; sum += counts[c]; }
  offsets[cells] = (int32_t)sum;
  std::vector<int32_t> entries(std::max<int64_t>(sum, 1), -7);
  std::vector<float4> tris(3 * FB);
  grid_fill_kernel(b.v.data(), VB, b.f.data(), FB, g, offsets.data(), cursor.data(), entries.data(), sum, tris.data());
  Pairs pb, pg;
  // the judge: pair_crosses — what the brute-force kernel runs for every (i, j) — in a plain double loop
  for (int64_t i = 0; i < FA; ++i) {
    Pts ta; int64_t a0, a1, a2;
    if (!load_pts(a.v.data(), a.f.data(), VA, i, ta, a0, a1, a2)) continue;
    for (int64_t j = 0; j < FB; ++j)
      if (pair_crosses(ta, a0, a1, a2, i, b.v.data(), b.f.data(), VB, j, self, self)) pb.push_back({(int)i, (int)j});
  }
  int rc = 0;
  rc |= two_passes(name, FA, [&](int32_t* cnt, unsigned long long* tot, Sink s) {
    for (int64_t i = 0; i < FA; ++i) {
      blockIdx.x = (unsigned)(i / 256); threadIdx.x = (unsigned)(i % 256);
      intersect_grid_kernel<1>(a.v.data(), VA, a.f.data(), FA, b.v.data(), VB, b.f.data(), FB,
                               GridView{g, offsets.data(), entries.data(), sum}, self, self, cnt, tot, s);
    }
  }, pg);
  bool same = pb == pg;
  bool ordered = true;
  if (self) for (auto& p : pb) ordered &= p.first < p.second;
  printf("%s: dims %dx%dx%d, %lld x %lld faces, %lld entries, %zu pairs, %s\n", name, nx, ny, nz, (long long)FA, (long long)FB,
         (long long)sum, pb.size(), same && ordered && !rc ? "0 mismatches" : "MISMATCH");
  return !(same && ordered) || rc;
}

int main() {
  int rc = 0;
  Mesh a = soup(300, 700, 0.25f, 0.f), b = soup(280, 650, 0.3f, 0.2f);
  rc |= run("soups 9^3", a, b, false, 9, 9, 9);
  rc |= run("soups 1^3", a, b, false, 1, 1, 1);
  rc |= run("soups 31x2x7", a, b, false, 31, 2, 7);
  rc |= run("soups 40^3", b, a, false, 40, 40, 40);
  rc |= run("self 11^3", a, a, true, 11, 11, 11);
  rc |= run("self 1^3", b, b, true, 1, 1, 1);
  Mesh far = soup(50, 80, 0.2f, 5.f);                       // A outside B's grid: clamped into its edge cells
  rc |= run("disjoint 6^3", far, a, false, 6, 6, 6);
  Mesh nan = a;
  for (size_t i = 0; i < nan.v.size(); i += 17) nan.v[i] = __builtin_nanf("");
  rc |= run("NaN in A 9^3", nan, b, false, 9, 9, 9);
  printf(rc ? "FAILED\n" : "all ok\n");
  return rc;
}
