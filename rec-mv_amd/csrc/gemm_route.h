// Which kernel a recmv_gemm_nt* / recmv_gemm_tn launch gets: the one place where the routes of gemm_f32.hip and gemm_tn.hip are decided.
//
// Pure host code over standard headers only (no HIP): tools/gemm_route_host_check compiles it with a plain C++ compiler
// (tests/host_check.py) and tests/test_gemm_route_cpu.py compares its plans with the census of tests/golden/gemm_routes.json.
//
// The invariant the planner keeps: a launch that one of the later kernels takes (the thin kernels for K <= 4 / N <= 4 / a TN output of
// <= 4 rows or columns, the SCAL kernels for unaligned operands) keeps the bits and the profile slot of the MFMA kernel that took it
// before.  That kernel is not re-derived anywhere: it is plan_nt on the same shape with `skinny` off (plan_tn: the `replaced` member).
#pragma once
#include <stdint.h>

namespace recmv {
namespace route {

// ---- tile sizes and thresholds the routes depend on (the kernels take them from here)
constexpr int BM = 128, BN = 128, BK = 32;     // large NT tile and the TN kernels' tile; BK: K-tile of the two-per-CU kernels
constexpr int kMidTile = 64;                   // 64 x 64 NT tile; the narrow kernel's is 64 x kNarrowN
constexpr int kNarrowN = 32;
constexpr int kOccBK = 16;                     // K-tile of the high-occupancy kernels (NT and TN)
constexpr int kCUs = 256;                      // MI355X (common.h: kNumCU)
constexpr int64_t kLargeTilesMin = 2 * kCUs;           // 128 x 128 tiles from two workgroups per CU on
constexpr int64_t kOcc128TilesMin = 3600;              // below: 64 x 128 tiles at five per CU (profiles/r03_gemm_occupancy_variants.txt)
constexpr int64_t kNarrowTilesBelow = (5 * kCUs) / 2;  // fewer 64 x 64 tiles than 2.5 per CU: 64 x 32 tiles
constexpr double kLogFloor = 1e8;              // RECMV_GEMM_SHAPES=1 prints products of at least this many multiply-adds

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the 14 profile slots (recmv_profile_end)
enum Slot {
  kSlotNt64 = 0, kSlotNt128, kSlotNt64Fast, kSlotNt128Fast,                      // gemm_nt_kernel<T, FAST, false>: (T-1) + 2 FAST
  kSlotNt64Amul, kSlotNt128Amul, kSlotNt64FastAmul, kSlotNt128FastAmul,          //   ... <T, FAST, true>: + 4
  kSlotTn,                                                                       // every TN product kernel
  kSlotOcc128, kSlotOcc64x128, kSlotOccAmul,                                     // gemm_nt_occ_kernel<false, ...> by tile, <true, ...>
  kSlotNarrowFast, kSlotNarrowOther,                                             // gemm_nt_narrow_kernel<true, false, .> / the others
  kNumSlots
};
inline int slot_nt(int T, bool fast, bool amul) { return (T - 1) + 2 * (fast ? 1 : 0) + 4 * (amul ? 1 : 0); }
// the slot of a caller with room for n_variants >= 9: the slots added later fold into those of the kernels they replaced
inline int fold_slot(int v, int n_variants) {
  if (v < n_variants) return v;
  return v == kSlotOccAmul ? kSlotNt128FastAmul : v == kSlotNarrowFast ? kSlotNt64Fast : v == kSlotNarrowOther ? kSlotNt64FastAmul : kSlotNt128Fast;
}

// ---- the switches
struct GemmSwitches {
  int mode;          // g_gemm_mode: 0 f32 MFMA, 1 bf16x6
  int b3_families;   // g_b3_families (mode 1): bit 0 the 128 x 128 NT kernels, bit 1 the 64 x 64 / 64 x 32 NT kernels, bit 2 the TN kernel
  bool occ;          // RECMV_GEMM_OCC != 0 (read once per process): the high-occupancy kernels
  bool skinny;       // RECMV_GEMM_SKINNY != 0 (read at every launch): the thin and the SCAL kernels; off without `occ` as well
};

// ---- NT
struct NtShape {
  int64_t M, N, K;
  bool a_vec, b_vec, c_vec;   // operand / result rows 16-byte aligned (base and leading dimension)
  bool amul, emul, seg;       // operand transform, output transform, second weight set
  bool lda_ge_k;              // rows of A do not overlap (recmv_gemm_nt_actgrad allows lda = 0)
};
enum class NtKernel { Tile128, Tile64, Narrow, Occ128, Occ64x128, Occ128Scal, Occ64x128Scal, B3, ThinK, ThinN };
struct NtPlan {
  NtKernel kernel;
  bool fast;            // every staging load one aligned 16-byte load
  bool bf3;             // Tile128 / Tile64 / Narrow: the BF3 instantiation
  bool a_vec, b_vec;    // what the kernel is told about its operands' rows (the aligned Occ kernels: true; SCAL: A's rows must not overlap)
  int slot;
  bool halves;          // ThinN: sum the two halves of every 32-wide K-tile on separate chains (the order of Narrow)
  const char* route;    // what RECMV_GEMM_SHAPES=1 prints; "" for a launch that is not printed
  const char* parent;
};

inline NtPlan plan_nt(const NtShape& s, const GemmSwitches& sw) {
  NtPlan p = {NtKernel::Tile64, false, false, s.a_vec, s.b_vec, 0, false, "", ""};
  p.fast = s.a_vec && s.b_vec && s.K % 4 == 0 && s.K > 0;
  const int64_t large_tiles = cdiv(s.M, BM) * cdiv(s.N, BN);
  const bool large = large_tiles >= kLargeTilesMin;
  const bool bf3_large = sw.mode == 1 && (sw.b3_families & 1), bf3_mid = sw.mode == 1 && (sw.b3_families & 2);
  const bool skinny = sw.occ && sw.skinny;
  p.parent = large ? (p.fast ? "nt_occ" : "nt_kernel<2,false>") : "below 512 large tiles";
  // f32 mode, skinny shapes (chosen by N and K alone): the rank-K update for K <= 4, the per-row chains for N <= 4
  const bool thin_k = s.K >= 1 && s.K <= 4, thin_n = !s.amul && s.N <= 4;
  if (sw.mode == 0 && skinny && (thin_k || thin_n)) {
    GemmSwitches mfma_sw = sw;
    mfma_sw.skinny = false;
    const NtPlan mfma = plan_nt(s, mfma_sw);
    p.kernel = thin_k ? NtKernel::ThinK : NtKernel::ThinN;
    p.slot = mfma.slot;
    p.halves = mfma.kernel == NtKernel::Narrow;
    p.route = thin_k ? "thin_k" : "thin_n";
    return p;
  }
  if (large) {
    const bool occ128 = large_tiles >= kOcc128TilesMin;
    if (bf3_large && p.fast) {
      p.kernel = NtKernel::B3;
      p.slot = slot_nt(2, true, s.amul);
    } else if (p.fast && !bf3_large && sw.occ) {
      p.kernel = occ128 ? NtKernel::Occ128 : NtKernel::Occ64x128;
      p.slot = s.amul ? kSlotOccAmul : (occ128 ? kSlotOcc128 : kSlotOcc64x128);
      p.a_vec = p.b_vec = true;
    } else if (!p.fast && !bf3_large && skinny && s.K > 0) {
      // unaligned operands or K % 4 != 0: the high-occupancy kernels with dword staging loads, under the slot of gemm_nt_kernel<2, false, .>
      p.kernel = occ128 ? NtKernel::Occ128Scal : NtKernel::Occ64x128Scal;
      p.slot = slot_nt(2, false, s.amul);
      p.a_vec = s.a_vec && s.lda_ge_k;
      p.route = "occ_scal";
    } else {
      p.kernel = NtKernel::Tile128;
      p.bf3 = bf3_large;
      p.slot = slot_nt(2, p.fast, s.amul);
      if (!p.fast) p.route = "nt_kernel<2,false>";
    }
    return p;
  }
  p.bf3 = bf3_mid;
  if (cdiv(s.M, kMidTile) * cdiv(s.N, kMidTile) < kNarrowTilesBelow) {
    p.kernel = NtKernel::Narrow;
    p.slot = p.fast && !s.amul ? kSlotNarrowFast : kSlotNarrowOther;
  } else {
    p.kernel = NtKernel::Tile64;
    p.slot = slot_nt(1, p.fast, s.amul);
  }
  return p;
}

// ---- TN
struct TnShape {
  int64_t M, N, K, lda, ldb;
  bool a_vec, b_vec;
};
enum class TnKernel { Thin, Occ, OccScal, Tile, TileB3 };
struct TnPlan {
  TnKernel kernel;
  TnKernel replaced;    // Thin: the MFMA kernel that took the launch before (Occ or Tile); otherwise == kernel
  bool swap;            // Thin: the thin operand is B
  int splits;
  int64_t kchunk;       // rows of K per split
  const char* route;
  const char* parent;
};

inline int tn_splits(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = cdiv(M, BM) * cdiv(N, BN);
  int64_t want = cdiv((int64_t)kCUs * 4, tiles);          // ~4 workgroups per CU overall
  const int64_t maxs = cdiv(K, (int64_t)BK * 4);          // at least 4 K-tiles per split
  if (want > maxs) want = maxs;
  if (want > 128) want = 128;
  if (want < 1) want = 1;
  return (int)want;
}

inline TnPlan plan_tn(const TnShape& s, const GemmSwitches& sw) {
  TnPlan p = {TnKernel::Tile, TnKernel::Tile, false, tn_splits(s.M, s.N, s.K), 0, "", ""};
  const bool bf3 = sw.mode == 1 && (sw.b3_families & 4);
  const bool skinny = sw.occ && sw.skinny;
  // the aligned high-occupancy kernel reads whole float4s of both operands' rows
  const bool occ_ok = s.a_vec && s.b_vec && s.lda >= ((s.M + 3) & ~3ll) && s.ldb >= ((s.N + 3) & ~3ll) && s.M >= 4 && s.N >= 4;
  if (bf3) {
    p.kernel = TnKernel::TileB3;
  } else if (skinny && (s.M <= 4 || s.N <= 4)) {
    // a skinny output (the weight gradient of a 1- or 3-output layer): weighted column sums on the VALU, with the partials and the
    // split lengths of the MFMA kernel that took the launch before
    p.kernel = TnKernel::Thin;
    p.replaced = occ_ok ? TnKernel::Occ : TnKernel::Tile;
    p.swap = s.M > 4;
    p.route = "tn_thin";
    p.parent = occ_ok ? "tn_occ" : "tn_kernel<false>";
  } else if (sw.occ && occ_ok) {
    p.kernel = TnKernel::Occ;
  } else if (skinny && s.M > 4 && s.N > 4) {
    // a leading dimension that is no multiple of 4 or an unaligned base: the high-occupancy kernel with dword staging loads, with the
    // split lengths of the kernel it replaces (the launch keeps its bits)
    p.kernel = TnKernel::OccScal;
    p.replaced = TnKernel::Tile;
    p.route = "tn_occ_scal";
    p.parent = "tn_kernel<false>";
  } else {
    p.route = p.parent = "tn_kernel<false>";
  }
  if (p.kernel != TnKernel::Thin && p.kernel != TnKernel::OccScal) p.replaced = p.kernel;
  // split lengths: the aligned high-occupancy kernel rounds them to its K-tile of 16 rows, the others to 32
  const int granule = p.replaced == TnKernel::Occ ? kOccBK : BK;
  p.kchunk = cdiv(cdiv(s.K, p.splits), granule) * granule;
  return p;
}

inline bool logged(int64_t M, int64_t N, int64_t K) { return (double)M * (double)N * (double)K >= kLogFloor; }

}  // namespace route
}  // namespace recmv
