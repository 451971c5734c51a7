// f32 MFMA weight-gradient products (the TN half of the layer products; see gemm_f32.hip for the tiling) — gfx950.
//
//   gemm_tn : C[M,N] = A[K,M]^T . B[K,N]      dW = dZ^T . X  (K = #points): split-K partials, then a deterministic reduction
//
// Which kernel a launch gets, its number of splits and their length are decided in gemm_route.h (plan_tn).
#include "gemm_common.h"
#include "gemm_host.h"

namespace recmv {
namespace {

constexpr int LDM = BM + 4;    // TN: padded m stride (floats) of an LDS k-row

// ------------------------------------------------------------------------------------------ TN
// partial[split][M][N] = sum over k in the split's range of A[k][m]*B[k][n]
template <bool BF3>
__global__ __launch_bounds__(kBlk) void gemm_tn_kernel(const float* __restrict__ A, int64_t lda,
                                                       const float* __restrict__ B, int64_t ldb,
                                                       float* __restrict__ P, int M, int N, int64_t K, int nbm,
                                                       int nbn, int64_t kchunk, bool a_vec, bool b_vec) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                       // [2][BK][LDM]
  float* Bs = smem + 2 * BK * LDM;        // [2][BK][LDM]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles = nbm * nbn;
  const int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int tile_m = tile / nbn, tile_n = tile % nbn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int64_t kbeg = (int64_t)split * kchunk;
  int64_t kend = kbeg + kchunk;
  if (kend > K) kend = K;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // staging: BK rows x 128 floats = 1024 float4 per operand; krow = idx/32, c4 = idx%32
  float4 ra[4], rb[4];
  // `fast` (uniform): 16-byte aligned operands whose widths are multiples of 4 — a float4 of a row is entirely inside or
  // outside the matrix, so every staging load is one unconditional 16-byte load (an outside one reads a clamped address and
  // is zeroed); whole tiles (the common case: M, N multiples of 128, K-tile inside the split) skip the zeroing too.
  // Otherwise the element-guarded loader, whose per-lane branches keep the eight loads of a K-tile from overlapping.
  const bool fast = a_vec && b_vec && (M & 3) == 0 && (N & 3) == 0 && M >= 4 && N >= 4;
  const bool whole_mn = m0 + BM <= M && n0 + BN <= N;
  auto gload = [&](int64_t k0) {
    if (fast) {
      const bool whole = whole_mn && k0 + BK <= kend;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int idx = tid + kBlk * r;
        const int krow = idx >> 5, c4 = idx & 31;
        const int64_t k = k0 + krow;
        const int cm = m0 + c4 * 4, cn = n0 + c4 * 4;
        if (whole) {
          ra[r] = *reinterpret_cast<const float4*>(A + k * lda + cm);
          rb[r] = *reinterpret_cast<const float4*>(B + k * ldb + cn);
        } else {
          const bool kin = k < kend, ain = kin && cm < M, bin = kin && cn < N;
          const int64_t kc = kin ? k : kend - 1;
          float4 a = *reinterpret_cast<const float4*>(A + kc * lda + (cm < M ? cm : M - 4));
          float4 b = *reinterpret_cast<const float4*>(B + kc * ldb + (cn < N ? cn : N - 4));
          ra[r] = make_float4(ain ? a.x : 0.f, ain ? a.y : 0.f, ain ? a.z : 0.f, ain ? a.w : 0.f);
          rb[r] = make_float4(bin ? b.x : 0.f, bin ? b.y : 0.f, bin ? b.z : 0.f, bin ? b.w : 0.f);
        }
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int idx = tid + kBlk * r;
      const int krow = idx >> 5, c4 = idx & 31;
      const int64_t k = k0 + krow;
      const int cm = m0 + c4 * 4, cn = n0 + c4 * 4;
      ra[r] = (k < kend) ? load4_guard(A + k * lda + cm, M - cm, a_vec) : make_float4(0, 0, 0, 0);
      rb[r] = (k < kend) ? load4_guard(B + k * ldb + cn, N - cn, b_vec) : make_float4(0, 0, 0, 0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int idx = tid + kBlk * r;
      const int krow = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<float4*>(As + (buf * BK + krow) * LDM + c4 * 4) = ra[r];
      *reinterpret_cast<float4*>(Bs + (buf * BK + krow) * LDM + c4 * 4) = rb[r];
    }
  };

  const int nk = (int)((kend - kbeg + BK - 1) / BK);
  if (nk > 0) {
    gload(kbeg);
    lstore(0);
  }
  __syncthreads();
  const int acol = wm * 64 + (lane & 31), bcol = wn * 64 + (lane & 31), kh = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kbeg + (int64_t)(kt + 1) * BK);
    if (BF3) {
      // bf16x6 (see split2): a lane's 8 consecutive k of column m are 8 rows of the k-major LDS tile
      const float* as = As + (buf * BK + 8 * kh) * LDM + acol;
      const float* bs = Bs + (buf * BK + 8 * kh) * LDM + bcol;
#pragma unroll
      for (int ks = 0; ks < BK / 16; ++ks) {
        Pieces pa[2], pb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float* ap = as + ks * 16 * LDM + 32 * i;
          const float* bp = bs + ks * 16 * LDM + 32 * i;
          pa[i] = split8(make_float4(ap[0], ap[LDM], ap[2 * LDM], ap[3 * LDM]),
                         make_float4(ap[4 * LDM], ap[5 * LDM], ap[6 * LDM], ap[7 * LDM]));
          pb[i] = split8(make_float4(bp[0], bp[LDM], bp[2 * LDM], bp[3 * LDM]),
                         make_float4(bp[4 * LDM], bp[5 * LDM], bp[6 * LDM], bp[7 * LDM]));
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].h, pb[ni].l, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].l, pb[ni].h, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].m, pb[ni].m, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].h, pb[ni].m, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].m, pb[ni].h, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].h, pb[ni].h, acc[mi][ni], 0, 0, 0);
          }
      }
    } else {
    const float* as = As + (buf * BK + kh) * LDM + acol;
    const float* bs = Bs + (buf * BK + kh) * LDM + bcol;
#pragma unroll
    for (int k2 = 0; k2 < BK / 2; ++k2) {
      const float a0 = as[k2 * 2 * LDM], a1 = as[k2 * 2 * LDM + 32];
      const float b0 = bs[k2 * 2 * LDM], b1 = bs[k2 * 2 * LDM + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  float* Ps = P + (int64_t)split * M * N;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int gn = n0 + wn * 64 + ni * 32 + (lane & 31);
    if (gn >= N) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm < M) Ps[(int64_t)gm * N + gn] = acc[mi][ni][r];
      }
    }
  }
}

// The same partial products with ONE 16-row K-tile in LDS (17 KB instead of 68 KB) and at most 128 registers: four workgroups
// per CU instead of two (the same step the NT kernel took: a workgroup's barriers, prologue and register -> HBM epilogue are
// covered by three neighbours instead of one).  f32 mode, aligned whole-float4 operands only; same summation order.
// SCAL: operands that miss the 16-byte conditions (a leading dimension that is no multiple of 4, an unaligned base) are staged with
// loads that need only dword alignment (load4_dword), the last group of a row element by element; same LDS image and MFMA order as the aligned loads on a zero-padded copy.
template <int BKT, bool SCAL = false>
__global__ __launch_bounds__(kBlk, 4) void gemm_tn_occ_kernel(const float* __restrict__ A, int64_t lda,
                                                              const float* __restrict__ B, int64_t ldb,
                                                              float* __restrict__ P, int M, int N, int64_t K, int nbm,
                                                              int nbn, int64_t kchunk) {
  constexpr int NLD = BKT * 32 / kBlk;    // float4 per thread per operand tile
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                       // [BKT][LDM]
  float* Bs = smem + BKT * LDM;           // [BKT][LDM]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles = nbm * nbn;
  // consecutive workgroup ids go round the 8 XCDs: keep ALL output tiles of a split (they read the same operand rows) on one XCD,
  // so that its L2 fetches those rows once — XCD x takes the splits x, x + 8, ...
  int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int splits = gridDim.x / tiles;
  if (splits % kNumXCD == 0) {
    const int x = blockIdx.x % kNumXCD, j = blockIdx.x / kNumXCD;
    split = x + kNumXCD * (j / tiles);
    tile = j % tiles;
  }
  const int tile_m = tile / nbn, tile_n = tile % nbn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int64_t kbeg = (int64_t)split * kchunk;
  int64_t kend = kbeg + kchunk;
  if (kend > K) kend = K;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  float4 ra[NLD], rb[NLD];
  const bool whole_mn = m0 + BM <= M && n0 + BN <= N;
  auto gload = [&](int64_t k0) {
    const bool whole = whole_mn && k0 + BKT <= kend;
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = tid + kBlk * r;
      const int krow = idx >> 5, c4 = idx & 31;
      const int64_t k = k0 + krow;
      const int cm = m0 + c4 * 4, cn = n0 + c4 * 4;
      if (SCAL) {
        ra[r] = k < kend ? load4_dword(A + k * lda + cm, M - cm) : make_float4(0, 0, 0, 0);
        rb[r] = k < kend ? load4_dword(B + k * ldb + cn, N - cn) : make_float4(0, 0, 0, 0);
      } else if (whole) {
        ra[r] = *reinterpret_cast<const float4*>(A + k * lda + cm);
        rb[r] = *reinterpret_cast<const float4*>(B + k * ldb + cn);
      } else {
        const bool kin = k < kend, ain = kin && cm < M, bin = kin && cn < N;
        const int64_t kc = kin ? k : kend - 1;
        // widths that are no multiple of 4 (the skip layer's 473 columns inside a 512-wide buffer): the launcher has checked that
        // the row strides cover the rounded-up widths, so the last float4 of a row reads up to 3 elements of padding — they only
        // reach output rows / columns >= M / N, which are never stored
        float4 a = *reinterpret_cast<const float4*>(A + kc * lda + (cm < M ? cm : (M - 1) & ~3));
        float4 b = *reinterpret_cast<const float4*>(B + kc * ldb + (cn < N ? cn : (N - 1) & ~3));
        ra[r] = make_float4(ain ? a.x : 0.f, ain ? a.y : 0.f, ain ? a.z : 0.f, ain ? a.w : 0.f);
        rb[r] = make_float4(bin ? b.x : 0.f, bin ? b.y : 0.f, bin ? b.z : 0.f, bin ? b.w : 0.f);
      }
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = tid + kBlk * r;
      const int krow = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<float4*>(As + krow * LDM + c4 * 4) = ra[r];
      *reinterpret_cast<float4*>(Bs + krow * LDM + c4 * 4) = rb[r];
    }
  };

  const int nk = (int)((kend - kbeg + BKT - 1) / BKT);
  if (nk > 0) {
    gload(kbeg);
    lstore();
  }
  __syncthreads();
  const int acol = wm * 64 + (lane & 31), bcol = wn * 64 + (lane & 31), kh = lane >> 5;
  const float* as = As + kh * LDM + acol;
  const float* bs = Bs + kh * LDM + bcol;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) gload(kbeg + (int64_t)(kt + 1) * BKT);
#pragma unroll
    for (int k2 = 0; k2 < BKT / 2; ++k2) {
      const float a0 = as[k2 * 2 * LDM], a1 = as[k2 * 2 * LDM + 32];
      const float b0 = bs[k2 * 2 * LDM], b1 = bs[k2 * 2 * LDM + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
    if (kt + 1 < nk) lstore();
    __syncthreads();
  }

  float* Ps = P + (int64_t)split * M * N;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int gn = n0 + wn * 64 + ni * 32 + (lane & 31);
    if (gn >= N) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm < M) Ps[(int64_t)gm * N + gn] = acc[mi][ni][r];
      }
    }
  }
}

// Skinny TN products (f32 mode): one operand has NT <= 4 columns — the weight gradient of a last layer is NT weighted column sums of
// X.  T [K, NT] is the thin operand, W [K, NW] the wide one; partial[split][t][w] (SWAP: [w][t], the thin operand is the product's
// B) = sum over the split's rows of T[k][t] W[k][w].  One wave takes 64 columns of one split, a lane one column: coalesced 256-byte
// row segments, 16 rows requested ahead of the chain that consumes them.
// Summation order: per split ONE k-ascending fmaf chain from 0 — the order of the MFMA kernels above (k0 = even k from lanes 0-31,
// k1 = odd k from lanes 32-63, rows past the split as exact zeros) with the same split lengths — then the splits in ascending order
// by the split-K reduction below: the results are those of the MFMA route, bit for bit.
template <int NT, bool SWAP>
__global__ __launch_bounds__(kWave) void gemm_tn_thin_kernel(const float* __restrict__ T, int64_t ldt,
                                                             const float* __restrict__ W, int64_t ldw,
                                                             float* __restrict__ P, int NW, int64_t K, int64_t kchunk,
                                                             int ntile) {
  const int tile = blockIdx.x % ntile, split = blockIdx.x / ntile;
  const int c = tile * kWave + threadIdx.x;
  if (c >= NW) return;
  const int64_t kbeg = (int64_t)split * kchunk;
  int64_t kend = kbeg + kchunk;
  if (kend > K) kend = K;
  float acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = 0.f;
  const float* w = W + c;
#pragma unroll 16
  for (int64_t k = kbeg; k < kend; ++k) {
    const float wv = w[k * ldw];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = fmaf(T[k * ldt + t], wv, acc[t]);
  }
  float* Ps = P + (int64_t)split * NT * NW;
#pragma unroll
  for (int t = 0; t < NT; ++t) Ps[SWAP ? (int64_t)c * NT + t : (int64_t)t * NW + c] = acc[t];
}

// C[m][n] = sum_s P[s][m][n]   (fixed order -> deterministic)
__global__ __launch_bounds__(kBlk) void splitk_reduce_kernel(const float* __restrict__ P, float* __restrict__ C,
                                                             int64_t ldc, int M, int N, int splits) {
  const int64_t total = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlk) {
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += P[(int64_t)sp * total + i];
    C[(i / N) * ldc + (i % N)] = s;
  }
}

// The same sums in the same order, four columns per lane and eight partial tiles requested before the first is added: the
// scalar loop above asks for one 4-byte value per split and lane at a time (64 dependent round trips for 64 splits).
__global__ __launch_bounds__(kBlk) void splitk_reduce4_kernel(const float4* __restrict__ P, float* __restrict__ C,
                                                              int64_t ldc, int M, int N, int splits) {
  const int64_t total4 = (int64_t)M * N / 4;
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < total4; i += (int64_t)gridDim.x * kBlk) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int sp = 0;
    for (; sp + 8 <= splits; sp += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = P[(int64_t)(sp + u) * total4 + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s.x += v[u].x;
        s.y += v[u].y;
        s.z += v[u].z;
        s.w += v[u].w;
      }
    }
    for (; sp < splits; ++sp) {
      const float4 v = P[(int64_t)sp * total4 + i];
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
    const int64_t e = i * 4;
    *reinterpret_cast<float4*>(C + (e / N) * ldc + (e % N)) = s;
  }
}

constexpr int kTnLds = (4 * BK * LDM) * 4;                       // 67584 B
constexpr int kTnOccLds = 2 * route::kOccBK * LDM * 4;

}  // namespace
}  // namespace recmv

using namespace recmv;
using route::TnKernel;

extern "C" int64_t recmv_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return (int64_t)route::tn_splits(M, N, K) * M * N * 4;
}

// The skinny route's kernel arguments: T is the thin operand (the product's B when the plan swaps), W the wide one.
struct TnThinArgs {
  const float* T;
  int64_t ldt;
  const float* W;
  int64_t ldw;
  float* P;
  int NW;
  int64_t K, kchunk;
  int ntile;
};
template <int NT>
static void launch_tn_thin(const TnThinArgs& a, bool swap, int splits, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.ntile * splits));
  if (swap)
    hipLaunchKernelGGL((gemm_tn_thin_kernel<NT, true>), grid, dim3(kWave), 0, s, a.T, a.ldt, a.W, a.ldw, a.P, a.NW, a.K, a.kchunk, a.ntile);
  else
    hipLaunchKernelGGL((gemm_tn_thin_kernel<NT, false>), grid, dim3(kWave), 0, s, a.T, a.ldt, a.W, a.ldw, a.P, a.NW, a.K, a.kchunk, a.ntile);
}

extern "C" int recmv_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  RECMV_REQUIRE(M >= 0 && N >= 0 && K >= 0, "gemm_tn: negative size");
  if (M == 0 || N == 0) return RECMV_OK;
  RECMV_REQUIRE(M < (1 << 20) && N < (1 << 20), "gemm_tn: output too large");
  hipStream_t s = (hipStream_t)stream;
  if (K == 0) {                // an empty reduction (its operands carry NULL data pointers): C = 0
    RECMV_REQUIRE(C && ldc >= N, "gemm_tn: bad output");
    for (int64_t m = 0; m < M; ++m) RECMV_HIP_TRY(hipMemsetAsync(C + m * ldc, 0, N * 4, s));
    return RECMV_OK;
  }
  RECMV_REQUIRE(A && B && C, "gemm_tn: NULL pointer");
  RECMV_REQUIRE(lda >= M && ldb >= N && ldc >= N, "gemm_tn: leading dimension too small");
  const route::TnShape sh = {M, N, K, lda, ldb, aligned16(A) && lda % 4 == 0, aligned16(B) && ldb % 4 == 0};
  const route::TnPlan p = route::plan_tn(sh, gemm_switches());
  const int splits = p.splits;
  const int64_t need = (int64_t)splits * M * N * 4;
  if (!workspace || workspace_bytes < need) {
    set_error("gemm_tn: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    return RECMV_ERR_WORKSPACE;
  }
  static bool attr_set = false;
  if (!attr_set) {
    RECMV_HIP_TRY(hipFuncSetAttribute((const void*)gemm_tn_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kTnLds));
    RECMV_HIP_TRY(hipFuncSetAttribute((const void*)gemm_tn_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kTnLds));
    attr_set = true;
  }
  const int nbm = (int)ceil_div(M, BM), nbn = (int)ceil_div(N, BN);
  const dim3 grid((unsigned)(nbm * nbn * splits));
  float* partial = (float*)workspace;
  if (p.route[0]) log_shape(p.route, p.parent, {M, N, K, lda, ldb, A, B, false, false, false});
  int rc;
  {                          // the events bracket the product kernel alone (one slot for every TN kernel); its reduction pass follows
    ScopedLaunchTimer timer(route::kSlotTn, (double)M, (double)N, (double)K, s);
    switch (p.kernel) {
      case TnKernel::Thin: {
        const int64_t NW = p.swap ? M : N;
        const TnThinArgs t = {p.swap ? B : A, p.swap ? ldb : lda, p.swap ? A : B, p.swap ? lda : ldb, partial, (int)NW, K, p.kchunk,
                              (int)ceil_div(NW, kWave)};
        switch (p.swap ? N : M) {
          case 1: launch_tn_thin<1>(t, p.swap, splits, s); break;
          case 2: launch_tn_thin<2>(t, p.swap, splits, s); break;
          case 3: launch_tn_thin<3>(t, p.swap, splits, s); break;
          default: launch_tn_thin<4>(t, p.swap, splits, s);
        }
        break;
      }
      case TnKernel::Occ:
        hipLaunchKernelGGL(gemm_tn_occ_kernel<16>, grid, dim3(kBlk), kTnOccLds, s, A, lda, B, ldb, partial, (int)M, (int)N, K, nbm, nbn,
                           p.kchunk);
        break;
      case TnKernel::OccScal:
        hipLaunchKernelGGL((gemm_tn_occ_kernel<16, true>), grid, dim3(kBlk), kTnOccLds, s, A, lda, B, ldb, partial, (int)M, (int)N, K, nbm,
                           nbn, p.kchunk);
        break;
      case TnKernel::TileB3:
        hipLaunchKernelGGL(gemm_tn_kernel<true>, grid, dim3(kBlk), kTnLds, s, A, lda, B, ldb, partial, (int)M, (int)N, K, nbm, nbn,
                           p.kchunk, sh.a_vec, sh.b_vec);
        break;
      case TnKernel::Tile:
        hipLaunchKernelGGL(gemm_tn_kernel<false>, grid, dim3(kBlk), kTnLds, s, A, lda, B, ldb, partial, (int)M, (int)N, K, nbm, nbn,
                           p.kchunk, sh.a_vec, sh.b_vec);
        break;
    }
    rc = check_launch("gemm_tn");
  }
  if (rc) return rc;
  if (N % 4 == 0 && ldc % 4 == 0 && aligned16(C) && aligned16(workspace))
    hipLaunchKernelGGL(splitk_reduce4_kernel, dim3(stream_grid(M * N / 4, kBlk)), dim3(kBlk), 0, s,
                       (const float4*)workspace, C, ldc, (int)M, (int)N, splits);
  else
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(stream_grid(M * N, kBlk)), dim3(kBlk), 0, s,
                       (const float*)workspace, C, ldc, (int)M, (int)N, splits);
  return check_launch("gemm_tn/reduce");
}
