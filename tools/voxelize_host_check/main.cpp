// csrc/mesh_voxelize.hip's kernels compiled for the CPU (one lane per wave) and run under the address and undefined-behaviour
// sanitizers: the scatter over every face's dilated box against a loop over all (node, face) pairs, the same keys bit for
// bit, on lattices that cover the mesh, cover half of it, lie beside it, have single-node axes, and on faces with invalid
// indices, without area, with NaN and with infinite corners; and the column walk against its restatement.
#include "common.h"
#include "recmv_hip.h"
#include <stdarg.h>
#include <stdlib.h>
#include <vector>

static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
  auto o = *p;
  if (v < o) *p = v;
  return o;
}
#include "voxelize.inc"                                    // csrc/mesh_voxelize.hip up to its entry points
using namespace recmv;

static uint32_t rng_state = 12345u;
static float rnd() {                                       // [0, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (float)(rng_state >> 8) * (1.f / 16777216.f);
}

struct Mesh {
  std::vector<float> v;
  std::vector<int64_t> f;
};

// `n` triangles with corners in the unit cube, edges up to `size`, then the broken rows
static Mesh soup(int n, float size, bool broken) {
  Mesh m;
  for (int i = 0; i < n; ++i) {
    const float c[3] = {rnd(), rnd(), rnd()};
    for (int k = 0; k < 3; ++k) {
      for (int a = 0; a < 3; ++a) m.v.push_back(c[a] + size * (rnd() - 0.5f));
      m.f.push_back(3 * i + k);
    }
  }
  if (broken) {
    const int64_t V = (int64_t)m.v.size() / 3;
    const float extra[4][3] = {{NAN, 0.5f, 0.5f}, {INFINITY, 0.5f, 0.5f}, {0.5f, -INFINITY, 0.25f}, {0.3f, 0.3f, 0.3f}};
    for (auto& e : extra) m.v.insert(m.v.end(), e, e + 3);
    const int64_t rows[6][3] = {{0, 1, V + 9}, {-1, 2, 3}, {4, 4, 4}, {0, 1, V}, {2, V + 1, 5}, {V + 2, 7, 8}};
    for (auto& r : rows) m.f.insert(m.f.end(), r, r + 3);
    m.f.insert(m.f.end(), {5, 5, V + 3});
  }
  return m;
}

static int check(const char* name, const Mesh& m, recmv_lattice lat, float band) {
  const int64_t V = (int64_t)m.v.size() / 3, F = (int64_t)m.f.size() / 3;
  const int64_t N = (int64_t)lat.nx * lat.ny * lat.nz;
  std::vector<unsigned long long> keys(N, ~0ull), want(N, ~0ull);
  const Lat L = lat_of(&lat);
  gridDim.x = 3;
  for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
    for (threadIdx.x = 0; threadIdx.x < (unsigned)kVoxBlock; ++threadIdx.x)
      voxel_band_kernel(m.v.data(), V, m.f.data(), F, L, band, keys.data());
  const float band2 = band * band;
  int64_t in_band = 0;
  for (int32_t i = 0; i < lat.nx; ++i)
    for (int32_t j = 0; j < lat.ny; ++j)
      for (int32_t k = 0; k < lat.nz; ++k) {
        const float px = lat.origin[0] + (float)i * lat.step, py = lat.origin[1] + (float)j * lat.step,
                    pz = lat.origin[2] + (float)k * lat.step;
        unsigned long long best = ~0ull;
        for (int64_t t = 0; t < F; ++t) {
          Tri q;
          if (!load_tri(m.v.data(), m.f.data(), V, t, q)) continue;
          float s, u;
          const float d = closest_st(px, py, pz, q, s, u);
          if (d <= band2) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)t;
            if (key < best) best = key;
          }
        }
        want[((int64_t)i * lat.ny + j) * lat.nz + k] = best;
        in_band += best != ~0ull;
      }
  int64_t bad = 0;
  for (int64_t n = 0; n < N; ++n) bad += keys[n] != want[n];
  // the finish kernel and the column walk
  std::vector<float> d2(N), sdf(N);
  std::vector<int64_t> face(N);
  std::vector<uint8_t> flag(N), inside(N);
  gridDim.x = 1; blockDim.x = 1; blockIdx.x = 0; threadIdx.x = 0;
  if (N) voxel_band_finish_kernel(keys.data(), N, d2.data(), face.data());
  for (int64_t n = 0; n < N; ++n) flag[n] = (uint8_t)((n * 2654435761u >> 7) & 1);
  unsigned long long open = 0, open_want = 0;
  const int64_t columns = (int64_t)lat.ny * lat.nz;
  blockDim.x = 1;
  for (blockIdx.x = 0; blockIdx.x < (unsigned)columns + 2; ++blockIdx.x)        // two threads beyond the last column
    voxel_sign_fill_kernel(d2.data(), flag.data(), L, band, 1, sdf.data(), inside.data(), &open);
  for (int64_t c = 0; c < columns; ++c) {
    uint8_t st = 0;
    for (int32_t i = 0; i < lat.nx; ++i) {
      const int64_t n = (int64_t)i * columns + c;
      if (want[n] != ~0ull) st = flag[n];
      const float d = want[n] != ~0ull ? fminf(sqrtf(d2[n]), band) : band;
      bad += inside[n] != st || sdf[n] != (st ? -d : d) || (want[n] == ~0ull) != (face[n] == -1);
    }
    open_want += st;
  }
  bad += open != open_want;
  printf("%s: %lld nodes, %lld faces, %lld in the band, %lld mismatches\n", name, (long long)N, (long long)F,
         (long long)in_band, (long long)bad);
  return bad != 0;
}

int main() {
  int fails = 0;
  const Mesh small = soup(300, 0.08f, false), large = soup(12, 1.5f, false), broken = soup(200, 0.1f, true);
  fails += check("covers the mesh", small, recmv_lattice{{-0.2f, -0.2f, -0.2f}, 0.05f, 29, 30, 31}, 0.15f);
  fails += check("covers half of it", small, recmv_lattice{{0.45f, -0.3f, 0.5f}, 0.04f, 17, 33, 9}, 0.1f);
  fails += check("beside the mesh", small, recmv_lattice{{3.f, 3.f, -4.f}, 0.1f, 5, 5, 5}, 0.3f);
  fails += check("faces larger than the lattice", large, recmv_lattice{{0.2f, 0.2f, 0.2f}, 0.03f, 21, 19, 23}, 0.07f);
  fails += check("single-node axes 1x9x70", small, recmv_lattice{{0.5f, 0.1f, -0.4f}, 0.025f, 1, 9, 70}, 0.06f);
  fails += check("one node", small, recmv_lattice{{0.5f, 0.5f, 0.5f}, 0.1f, 1, 1, 1}, 0.5f);
  fails += check("band 0", small, recmv_lattice{{0.f, 0.f, 0.f}, 0.1f, 11, 11, 11}, 0.f);
  fails += check("broken faces", broken, recmv_lattice{{-0.1f, -0.1f, -0.1f}, 0.06f, 21, 21, 21}, 0.13f);
  fails += check("far origin", small, recmv_lattice{{-1000.f, 0.f, 0.f}, 10.f, 120, 3, 3}, 25.f);
  printf(fails ? "FAILED\n" : "all ok\n");
  return fails != 0;
}
