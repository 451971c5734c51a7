// Geodesic distance fields on a triangle mesh: Jacobi sweeps of the first-order Hopf-Lax update — gfx950.  Not in the reference.
//
// What it computes: the GPU work of recmv.geodesic.  B independent fields D [B, V] f64 over one mesh (verts [V,3] f32, faces
// [F,3] int64), each the fixed point of
//   D^{k+1}(v) = min(D^k(v), min over the usable faces (v, a, b) of v of U(v; a, b))            (every U reads D^k only)
// reached from above from D^0 (+inf except at the sources).  U is hopf_lax() below, which IS the definition of
// include/recmv_hip.h down to the order of the operations: float64 on the f32 coordinates, un-contracted, only correctly
// rounded operations (+ - * / sqrt) and an order-independent minimum, so both routes and tests/geodesic_reference.py give
// the same bits and the same sweep count K (the last sweep that lowered a value).
//
// How:
//   * Work per sweep: a vertex has about 6 faces, a face costs three dozen f64 operations, three square roots and two
//     divisions at the least, two more of each with an interior candidate.  A face both of whose other corners are at +inf
//     has no finite candidate and is skipped before its coordinates are loaded; a face neither of whose other corners was
//     lowered by the previous sweep gives the candidate it gave then, which D(v) already is at most, and is skipped too (a
//     "changed" byte per vertex, ping-pong like D).  Neither skip can change a bit: the tests compare with a restatement
//     that recomputes everything.
//   * sweeps route: one launch per sweep, one thread per (field, vertex), D and the changed bytes ping-pong in the caller's
//     workspace.  A thread that lowers its value stores the sweep's index into last_changed[b]: every writer of a sweep
//     stores the same number, a plain store.  The caller reads last_changed back every so often; the launches beyond K are
//     no-ops.  Plain launches in stream order: no grid synchronisation, no flag anybody waits on.
//   * lds route (V <= kGeoLdsMaxV): one workgroup per field, both D buffers and both changed-byte buffers in LDS, a
//     workgroup barrier between sweeps, until a sweep lowers nothing.
#include "common.h"

namespace recmv {
namespace {

#pragma clang fp contract(off)
#include "mesh_device.h"

constexpr int kGeoBlock = 256;
// The lds route's capacity.  The budget is 64 KiB: what a workgroup gets without opting in to more, and with 160 KiB a CU
// it leaves two fields resident per CU.  A vertex costs 2 * 8 bytes of D and 2 * 1 byte of "changed" (in LDS as well: a
// changed byte is read twelve times per vertex and sweep, as often as D); 16 bytes hold the three rotating "a value was
// lowered" words.  18 * 3640 + 16 = 65 536; 3641 does not fit.  (Two D buffers alone would give 4096.)
constexpr int kGeoLdsBytes = 65536;
constexpr int kGeoLdsMaxV = 3640;
constexpr int kGeoLdsBlockMax = 1024;
// Where route 'auto' changes over: the lds route for V <= kGeoAutoMaxV.  Measured on an MI355X
// (profiles/geodesic_timing.json, tools/geodesic_timing.py): square grids, a corner source per field, whole solves between
// device events (the sweeps route with its read-back every 32 sweeps), medians of 5, microseconds, lds / sweeps:
//   V =   64 (K 13):  B = 1   254 /  442,   B = 32   398 /  657
//   V =  256 (K 29):  B = 1   445 /  594,   B = 32   599 /  785
//   V =  529 (K 40):  B = 1   678 /  946,   B = 32   848 / 1233
//   V = 1024 (K 52):  B = 1  1085 / 1086,   B = 32  1236 / 1370
//   V = 2025 (K 71):  B = 1  2474 / 1617,   B = 32  2669 / 1824
//   V = 3600 (K 90):  B = 1  5136 / 1975,   B = 32  5330 / 2397
// One workgroup wins while a sweep is a chain of dependent loads (about 20 us either way, no launch between sweeps) and
// loses once its 1024 threads hold several vertices each: the capacity is not the crossover, for one field as for 32.  At
// 1024 vertices the two are level (and an earlier run had the sweeps route ahead by 1 - 4 %), so auto switches at 529, the
// largest measured size at which the lds route wins clearly; 'lds' can be forced up to kGeoLdsMaxV.
constexpr int kGeoAutoMaxV = 529;
constexpr int kGeoMaxSweeps = 1 << 30;

// U(v; a, b) of include/recmv_hip.h: the three points in f64, Da = D(a), Db = D(b) (never NaN; +inf allowed).
__device__ __forceinline__ double hopf_lax(const double* pv, const double* pa, const double* pb, double Da, double Db) {
  const double inf = __builtin_inf();
  const double w[3] = {pv[0] - pa[0], pv[1] - pa[1], pv[2] - pa[2]};
  const double u[3] = {pv[0] - pb[0], pv[1] - pb[1], pv[2] - pb[2]};
  const double la = length3(w[0], w[1], w[2]), lb = length3(u[0], u[1], u[2]);
  const double ca = Da + la, cb = Db + lb;
  double U = cb < ca ? cb : ca;
  if (Da < inf && Db < inf) {
    const double e[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
    const double L2 = dot3(e, e), L = sqrt(L2), delta = Db - Da;
    if (L > 0. && (delta < 0. ? -delta : delta) < L) {
      double n[3];
      cross3(w, e, n);
      const double h = length3(n[0], n[1], n[2]) / L;
      if (h > 0.) {
        const double t0 = dot3(w, e) / L2;
        const double ts = t0 - (delta * h) / (L * sqrt(L2 - delta * delta));
        if (ts > 0. && ts < 1.) {                          // (false for a NaN or an infinite ts)
          const double r = ts - t0;
          const double ci = (Da + ts * delta) + sqrt(h * h + L2 * (r * r));
          if (ci < U) U = ci;
        }
      }
    }
  }
  return U;
}

// min(best, the candidates of v's usable faces), reading D and the changed bytes of one field.  Every index is checked:
// a table that does not belong to the faces costs wrong values, never a read out of bounds.
__device__ __forceinline__ double relax_vertex(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces,
                                               int64_t F, const int64_t* __restrict__ off, const int64_t* __restrict__ slots,
                                               int64_t v, const double* D, const uint8_t* changed, double best) {
  const double inf = __builtin_inf();
  const CsrRow row = csr_range_ordered(off, v, 3 * F);
  for (int64_t s = row.k0; s < row.k1; ++s) {
    const int64_t slot = slots[s];
    if (!index_in(slot, 3 * F)) continue;
    const int64_t f = slot / 3;
    const int c = (int)(slot - 3 * f);
    const int64_t* tri = faces + 3 * f;
    if (!tri_valid(tri, V) || tri[c] != v) continue;
    const int64_t a = tri[(c + 1) % 3], b = tri[(c + 2) % 3];
    if (!(changed[a] | changed[b])) continue;
    const double Da = D[a], Db = D[b];
    if (!(Da < inf) && !(Db < inf)) continue;
    double pv[3], pa[3], pb[3];
    load3(verts, v, pv);
    load3(verts, a, pa);
    load3(verts, b, pb);
    if (!finite3(pv[0], pv[1], pv[2]) || !finite3(pa[0], pa[1], pa[2]) || !finite3(pb[0], pb[1], pb[2])) continue;
    const double U = hopf_lax(pv, pa, pb, Da, Db);
    if (U < best) best = U;
  }
  return best;
}

// Sweep k of every field: D^k from D^{k-1}.
__global__ __launch_bounds__(kGeoBlock) void geodesic_sweep_kernel(const float* __restrict__ verts, int64_t V,
                                                                   const int64_t* __restrict__ faces, int64_t F,
                                                                   const int64_t* __restrict__ off,
                                                                   const int64_t* __restrict__ slots, int64_t B,
                                                                   const double* __restrict__ Dsrc, double* __restrict__ Ddst,
                                                                   const uint8_t* __restrict__ csrc, uint8_t* __restrict__ cdst,
                                                                   int32_t* __restrict__ last_changed, int32_t k) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * V) return;
  const int64_t b = idx / V, v = idx - b * V;
  const double old = Dsrc[idx];
  const double now = relax_vertex(verts, V, faces, F, off, slots, v, Dsrc + b * V, csrc + b * V, old);
  const bool lowered = now < old;
  Ddst[idx] = now;
  cdst[idx] = lowered ? 1 : 0;
  if (lowered) last_changed[b] = k;
}

// D^0 is D[0] of the workspace, written by the caller; this marks every vertex as changed and clears last_changed.
__global__ __launch_bounds__(kGeoBlock) void geodesic_begin_kernel(int64_t BV, int64_t B, uint8_t* __restrict__ changed,
                                                                   int32_t* __restrict__ last_changed) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < BV) changed[idx] = 1;
  if (idx < B) last_changed[idx] = 0;
}

// One field per workgroup, the whole solve.
__global__ __launch_bounds__(kGeoLdsBlockMax) void geodesic_lds_kernel(const float* __restrict__ verts, int64_t V,
                                                                       const int64_t* __restrict__ faces, int64_t F,
                                                                       const int64_t* __restrict__ off,
                                                                       const int64_t* __restrict__ slots,
                                                                       const double* __restrict__ D0, double* __restrict__ Dout,
                                                                       int32_t* __restrict__ sweeps, int32_t max_sweeps) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kGeoLdsBytes];
  if (V > kGeoLdsMaxV) return;                             // (the whole workgroup; the entry point refuses it)
  const int64_t b = blockIdx.x;
  const int n = (int)V, tid = (int)threadIdx.x, step = (int)blockDim.x;
  double* Dl = (double*)smem;                              // [2][n]
  uint8_t* cl = smem + 16 * n;                             // [2][n]
  int32_t* any = (int32_t*)(smem + kGeoLdsBytes - 16);     // [3] used
  for (int i = tid; i < n; i += step) {
    Dl[i] = D0[b * V + i];
    cl[i] = 1;
  }
  if (tid < 4) any[tid] = 0;
  __syncthreads();
  int32_t K = -1, k = 1;
  for (;; ++k) {
    const double* src = Dl + ((k - 1) & 1) * n;
    double* dst = Dl + (k & 1) * n;
    const uint8_t* csrc = cl + ((k - 1) & 1) * n;
    uint8_t* cdst = cl + (k & 1) * n;
    for (int i = tid; i < n; i += step) {
      const double old = src[i];
      const double now = relax_vertex(verts, V, faces, F, off, slots, i, src, csrc, old);
      const bool lowered = now < old;
      dst[i] = now;
      cdst[i] = lowered ? 1 : 0;
      if (lowered) any[k % 3] = 1;
    }
    __syncthreads();
    const int32_t lowered_any = any[k % 3];
    if (tid == 0) any[(k + 2) % 3] = 0;                    // sweep k - 1's word, read by everybody before this sweep's barrier
    if (!lowered_any) {
      K = k - 1;
      break;
    }
    if (k > max_sweeps) break;                             // sweep max_sweeps + 1 still lowered a value: not converged
  }
  const double* res = Dl + (k & 1) * n;
  for (int i = tid; i < n; i += step) Dout[b * V + i] = res[i];
  if (tid == 0) sweeps[b] = K;
}

inline int64_t geo_align8(int64_t x) { return (x + 7) & ~(int64_t)7; }

// false with a message when the sizes cannot be used
bool geo_sizes(const char* who, int64_t V, int64_t F, int64_t B) {
  if (V < 0) {
    set_error("%s: V=%lld must not be negative", who, (long long)V);
    return false;
  }
  if (F < 0) {
    set_error("%s: F=%lld must not be negative", who, (long long)F);
    return false;
  }
  if (B < 0) {
    set_error("%s: B=%lld must not be negative", who, (long long)B);
    return false;
  }
  if (V >= (1ll << 31) || F >= (1ll << 31) || B >= (1ll << 31) || (V > 0 && B > (1ll << 38) / V)) {
    set_error("%s: V=%lld, F=%lld, B=%lld: at most 2^31 - 1 each and B * V at most 2^38", who, (long long)V, (long long)F,
              (long long)B);
    return false;
  }
  return true;
}

int64_t geo_workspace_bytes(int64_t V, int64_t B) { return 16 * B * V + 2 * geo_align8(B * V) + geo_align8(4 * B); }

bool geo_mesh(const char* who, const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* off,
              const int64_t* slots) {
  if (!verts || !off || (F > 0 && (!faces || !slots))) {
    set_error("%s: NULL pointer of the mesh or of its slot table", who);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace recmv

using namespace recmv;

extern "C" int64_t recmv_geodesic_lds_max_vertices(void) { return kGeoLdsMaxV; }
extern "C" int64_t recmv_geodesic_auto_max_vertices(void) { return kGeoAutoMaxV; }

extern "C" int64_t recmv_geodesic_workspace_bytes(int64_t V, int64_t F, int64_t B) {
  if (!geo_sizes("geodesic_workspace_bytes", V, F, B)) return -1;
  return geo_workspace_bytes(V, B);
}

extern "C" int recmv_geodesic_check_sources(const int64_t* sources, const double* values, int64_t S, int64_t V) {
  RECMV_REQUIRE(S >= 0, "geodesic_check_sources: S=%lld must not be negative", (long long)S);
  RECMV_REQUIRE(V >= 0, "geodesic_check_sources: V=%lld must not be negative", (long long)V);
  if (S == 0) return RECMV_OK;
  RECMV_REQUIRE(sources, "geodesic_check_sources: NULL sources");
  for (int64_t i = 0; i < S; ++i) {
    RECMV_REQUIRE(sources[i] >= 0 && sources[i] < V, "geodesic_check_sources: source %lld is vertex %lld, outside [0, %lld)",
                  (long long)i, (long long)sources[i], (long long)V);
    if (values)
      RECMV_REQUIRE(values[i] - values[i] == 0., "geodesic_check_sources: the value of source %lld is not finite", (long long)i);
  }
  return RECMV_OK;
}

extern "C" int recmv_geodesic_sweeps(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* slot_offsets,
                                     const int64_t* slots, int64_t B, void* workspace, int64_t workspace_bytes, int64_t k0,
                                     int64_t n, void* stream) {
  if (!geo_sizes("geodesic_sweeps", V, F, B)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(k0 >= 0 && n >= 0 && k0 <= kGeoMaxSweeps && n <= kGeoMaxSweeps,
                "geodesic_sweeps: k0=%lld and n=%lld must be 0 .. 2^30", (long long)k0, (long long)n);
  if (V == 0 || B == 0) return RECMV_OK;
  if (!geo_mesh("geodesic_sweeps", verts, V, faces, F, slot_offsets, slots)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(workspace, "geodesic_sweeps: NULL workspace");
  RECMV_REQUIRE(((uintptr_t)workspace & 7) == 0, "geodesic_sweeps: workspace must be 8-byte aligned");
  const int64_t need = geo_workspace_bytes(V, B);
  if (workspace_bytes < need) {
    set_error("geodesic_sweeps: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    return RECMV_ERR_ARG;
  }
  const int64_t BV = B * V;
  double* D = (double*)workspace;
  uint8_t* changed = (uint8_t*)(D + 2 * BV);
  int32_t* last_changed = (int32_t*)(changed + 2 * geo_align8(BV));
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)ceil_div(BV, kGeoBlock);
  int rc;
  if (k0 == 0) {
    geodesic_begin_kernel<<<grid, kGeoBlock, 0, s>>>(BV, B, changed, last_changed);
    if ((rc = check_launch("geodesic_begin")) != RECMV_OK) return rc;
  }
  for (int64_t k = k0 + 1; k <= k0 + n; ++k) {
    const int64_t from = (k - 1) & 1, to = k & 1;
    geodesic_sweep_kernel<<<grid, kGeoBlock, 0, s>>>(verts, V, faces, F, slot_offsets, slots, B, D + from * BV, D + to * BV,
                                                     changed + from * geo_align8(BV), changed + to * geo_align8(BV),
                                                     last_changed, (int32_t)k);
    if ((rc = check_launch("geodesic_sweep")) != RECMV_OK) return rc;
  }
  return RECMV_OK;
}

extern "C" int recmv_geodesic_lds(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* slot_offsets,
                                  const int64_t* slots, int64_t B, const double* D0, double* D, int32_t* sweeps,
                                  int64_t max_sweeps, void* stream) {
  if (!geo_sizes("geodesic_lds", V, F, B)) return RECMV_ERR_ARG;
  RECMV_REQUIRE(max_sweeps >= 0 && max_sweeps <= kGeoMaxSweeps, "geodesic_lds: max_sweeps=%lld must be 0 .. 2^30",
                (long long)max_sweeps);
  RECMV_REQUIRE(V <= kGeoLdsMaxV, "geodesic_lds: V=%lld, the lds route takes at most %d vertices", (long long)V, kGeoLdsMaxV);
  if (B == 0) return RECMV_OK;
  RECMV_REQUIRE(sweeps, "geodesic_lds: NULL sweeps");
  RECMV_REQUIRE(V == 0 || (D0 && D), "geodesic_lds: NULL field");
  if (V > 0 && !geo_mesh("geodesic_lds", verts, V, faces, F, slot_offsets, slots)) return RECMV_ERR_ARG;
  int block = (int)ceil_div(V > 0 ? V : 1, kWave) * kWave;
  if (block > kGeoLdsBlockMax) block = kGeoLdsBlockMax;
  geodesic_lds_kernel<<<(unsigned)B, block, 0, (hipStream_t)stream>>>(verts, V, faces, F, slot_offsets, slots, D0, D, sweeps,
                                                                      (int32_t)max_sweeps);
  return check_launch("geodesic_lds");
}
