// f32 MFMA contractions for the three MLPs of the hot path (SDF, deformer, colour) — gfx950.
//
// The reference runs these as torch.nn.Linear -> cuBLAS sgemm plus separate bias / activation kernels
// (model/network.py:98-111, model/Deformer.py:194-199, model/RenderNet.py:83-94).  Here each layer is ONE
// kernel: v_mfma_f32_32x32x2_f32 (exact f32 multiply-accumulate, 157 TFLOP/s dense peak on MI355X) over
// LDS-staged 128x128x32 tiles, with bias + activation (+ the 1/sqrt(2) skip scale) fused in the epilogue
// so activations make one HBM round trip per layer.
//
//   gemm_nt : C[M,N] = act(A[M,K] . B[N,K]^T + bias) * out_scale      forward  (A = activations, B = W)
//                                                                     and dX = dZ . W^T^T (B = W^T copy)
//   gemm_tn : C[M,N] = A[K,M]^T . B[K,N]                              dW = dZ^T . X  (K = #points), split-K   (gemm_tn.hip)
//
// Tiling (wave64): 256 threads = 4 waves in 2x2, each wave owns a 64x64 sub-tile = 2x2 MFMA tiles
// (64 accumulator VGPRs).  gemm_nt keeps both operands k-contiguous in LDS (row stride 36 floats: the
// 16-lane groups of ds_read_b128 hit 16 distinct 4-bank slots) and feeds 4 MFMAs per 16-byte read;
// gemm_tn keeps them k-major and reads one dword per MFMA operand (conflict-free, 2 x 32-lane groups).
// Global->LDS goes through registers one K-tile ahead (one barrier per K-tile, 2 LDS buffers).
// Workgroup ids are remapped so the column tiles that share an A row-panel run on the same XCD/L2.
//
// FLOPs: 2*M*N*K.  With K=N=512 the arithmetic intensity is 128 FLOP/B >> 157e12/8e12, so every layer
// is MFMA-bound, not HBM-bound.
//
// Which kernel a launch gets is decided in gemm_route.h (plan_nt), on the host and without HIP; this file launches what the plan names.
// The profiler that brackets the product launches of both files (recmv_profile_*) is here too.
#include <mutex>
#include <string>
#include <unordered_map>
#include <type_traits>
#include <vector>
#include <algorithm>
#include "gemm_common.h"
#include "gemm_host.h"

namespace recmv {
namespace {

constexpr int LDK = BK + 4;    // NT: padded k stride (floats) of an LDS row

// The activations of the fused epilogue (apply_act<ACT>) and act'(z) through y = act(z) on the staging and epilogue paths (dact_hw):
// activation.h.  elementwise.hip and mlp_chain.hip use another form of that derivative (dact_libm); the two agree to rounding.

// Optional transform of the A operand while it is staged: A_eff = A (.) act'(y_scale * Y) * a_scale — the
// dZ = dY (.) act'(Z) step of a layer's backward fused into the dX = dZ W product (no dZ round trip through HBM).
struct AMul {
  const float* Y;
  int64_t ldy;
  int act;
  float param, y_scale, a_scale;
  // row-segmented weights (recmv_gemm_nt_seg): tiles whose first row is >= split multiply by B2 (+ bias2) instead of B (+ bias) —
  // two nets of one shape over one concatenated row block in one launch; split is a multiple of every tile height (128)
  const float* B2;
  const float* bias2;
  int split;
};

__device__ __forceinline__ float4 amul4(float4 a, float4 y, const AMul& m) {
  a.x *= dact_hw(y.x * m.y_scale, m.act, m.param) * m.a_scale;
  a.y *= dact_hw(y.y * m.y_scale, m.act, m.param) * m.a_scale;
  a.z *= dact_hw(y.z * m.y_scale, m.act, m.param) * m.a_scale;
  a.w *= dact_hw(y.w * m.y_scale, m.act, m.param) * m.a_scale;
  return a;
}

// ------------------------------------------------------------------------------------------ NT
// T = MFMA tiles per wave along each dimension: T=2 -> 128x128 workgroup tile (large M), T=1 -> 64x64
// (small M: the ray path launches 3k-6k rows, 128-tiles would leave most of the 256 CUs idle).
// FAST: both operands 16-byte aligned with row strides and K multiples of 4 -> every staging load is one
// unconditional-address global_load_dwordx4 (rows clamped to the last valid row, k tail zero-filled per
// float4); otherwise the element-guarded loader.
//
// Epilogue: the accumulators go through LDS (the operand buffers are dead by then) and are written out by a
// compact loop — each thread owns a fixed 4-column strip, adds its bias float4, applies the activation and
// issues 16-byte row-contiguous stores.  (A fully unrolled per-accumulator-register epilogue costs 64 copies
// of the activation per thread: more instruction bytes than the instruction cache holds, and 4-byte stores.)
// Optional OUTPUT transform of the kernels without the operand transform: C (.)= act'(y_scale * Y[row, col]) * a_scale —
// the dZ = dY (.) act'(Z) step of the NEXT layer of a backward chain applied where dY is produced (each element once;
// the operand transform above recomputes it in every column tile that reads the element).
__device__ __forceinline__ float4 emul4(float4 v, const AMul& m, int gm, int gn, int N) {
  const float* y = m.Y + (int64_t)gm * m.ldy + gn;
  float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gn + 4 <= N && (m.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(m.Y) & 15) == 0) {
    yv = *reinterpret_cast<const float4*>(y);
  } else {
    yv.x = y[0];
    if (gn + 1 < N) yv.y = y[1];
    if (gn + 2 < N) yv.z = y[2];
    if (gn + 3 < N) yv.w = y[3];
  }
  v.x *= dact_hw(yv.x * m.y_scale, m.act, m.param) * m.a_scale;
  v.y *= dact_hw(yv.y * m.y_scale, m.act, m.param) * m.a_scale;
  v.z *= dact_hw(yv.z * m.y_scale, m.act, m.param) * m.a_scale;
  v.w *= dact_hw(yv.w * m.y_scale, m.act, m.param) * m.a_scale;
  return v;
}

// Row-segmented weights (see AMul): the tiles whose first row m0 is >= split take the second weight set.  split is a multiple of every
// tile height (128) or M, so the choice is uniform over a workgroup.
__device__ __forceinline__ void seg_operands(const AMul& am, int m0, const float* __restrict__& B, const float* __restrict__& bias) {
  if (am.B2 && m0 >= am.split) {
    B = am.B2;
    bias = am.bias2;
  }
}

template <int TBM, int TBN, int ACT>
__device__ __forceinline__ void nt_epilogue_rows(const float* __restrict__ Cs, const float* __restrict__ bias,
                                                 float* __restrict__ C, int64_t ldc, int M, int N, int m0, int n0,
                                                 float act_param, float out_scale, bool c_vec, const AMul& em) {
  constexpr int LDC = TBN + 4;
  constexpr int C4 = TBN / 4;                 // float4 strips per tile row (32 or 16): divides kBlk
  constexpr int ROWS_PER_PASS = kBlk / C4;    // 8 or 16
  const int tid = threadIdx.x;
  const int c4 = tid % C4, r0 = tid / C4;
  const int gn = n0 + c4 * 4;
  if (gn >= N) return;
  const float inv_p = act_param != 0.f ? 1.f / act_param : 0.f;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    bv.x = bias[gn];
    if (gn + 1 < N) bv.y = bias[gn + 1];
    if (gn + 2 < N) bv.z = bias[gn + 2];
    if (gn + 3 < N) bv.w = bias[gn + 3];
  }
  const bool full4 = c_vec && gn + 4 <= N;
#pragma unroll 2
  for (int row = r0; row < TBM; row += ROWS_PER_PASS) {
    const int gm = m0 + row;
    if (gm >= M) break;
    float4 v = *reinterpret_cast<const float4*>(Cs + row * LDC + c4 * 4);
    v.x = apply_act<ACT>(v.x + bv.x, act_param, inv_p) * out_scale;
    v.y = apply_act<ACT>(v.y + bv.y, act_param, inv_p) * out_scale;
    v.z = apply_act<ACT>(v.z + bv.z, act_param, inv_p) * out_scale;
    v.w = apply_act<ACT>(v.w + bv.w, act_param, inv_p) * out_scale;
    if (em.Y) v = emul4(v, em, gm, gn, N);
    float* dst = C + (int64_t)gm * ldc + gn;
    if (full4) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      if (gn + 1 < N) dst[1] = v.y;
      if (gn + 2 < N) dst[2] = v.z;
      if (gn + 3 < N) dst[3] = v.w;
    }
  }
}

template <int T, int ACT>
__device__ __forceinline__ void nt_epilogue(const float* __restrict__ Cs, const float* __restrict__ bias,
                                            float* __restrict__ C, int64_t ldc, int M, int N, int m0, int n0,
                                            float act_param, float out_scale, bool c_vec, const AMul& em) {
  nt_epilogue_rows<64 * T, 64 * T, ACT>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, em);
}

template <int T, bool FAST, bool AMUL, bool BF3>
__global__ __launch_bounds__(kBlk) void gemm_nt_kernel(const float* __restrict__ A, int64_t lda,
                                                       const float* __restrict__ B, int64_t ldb,
                                                       const float* __restrict__ bias, float* __restrict__ C,
                                                       int64_t ldc, int M, int N, int K, int act,
                                                       float act_param, float out_scale, int nbm, int nbn,
                                                       bool a_vec, bool b_vec, bool c_vec, AMul am) {
  constexpr int TBM = 64 * T, TBN = 64 * T;     // workgroup tile
  constexpr int WT = 32 * T;                    // wave tile edge
  constexpr int NLD = TBM * 8 / kBlk;           // float4 per thread per operand tile (4 or 2)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                        // [2][TBM][LDK]
  float* Bs = smem + 2 * TBM * LDK;        // [2][TBN][LDK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;      // 2x2 waves
  const int64_t logical = xcd_remap(blockIdx.x, (int64_t)nbm * nbn);
  const int tile_m = (int)(logical / nbn), tile_n = (int)(logical % nbn);
  const int m0 = tile_m * TBM, n0 = tile_n * TBN;
  seg_operands(am, m0, B, bias);

  f32x16 acc[T][T];
#pragma unroll
  for (int a = 0; a < T; ++a)
#pragma unroll
    for (int b = 0; b < T; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // staging map: TBM*8 float4 per operand tile; row = idx/8, c4 = idx%8
  float4 ra[NLD], rb[NLD];
  const float* pa[NLD];
  const float* pb[NLD];
  const float* py[NLD];
  if (FAST) {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = tid + kBlk * r;
      const int row = idx >> 3, c4 = idx & 7;
      int gm = m0 + row, gn = n0 + row;
      gm = gm < M ? gm : M - 1;                 // clamped rows are computed and never stored
      gn = gn < N ? gn : N - 1;
      pa[r] = A + (int64_t)gm * lda + c4 * 4;
      pb[r] = B + (int64_t)gn * ldb + c4 * 4;
      if (AMUL) py[r] = am.Y + (int64_t)gm * am.ldy + c4 * 4;
    }
  }
  auto gload = [&](int k0) {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = tid + kBlk * r;
      const int row = idx >> 3, c4 = idx & 7;
      const int k = k0 + c4 * 4;
      if (FAST) {
        const bool in = k < K;                  // K % 4 == 0: a float4 is entirely inside or outside
        ra[r] = in ? *reinterpret_cast<const float4*>(pa[r] + k0) : make_float4(0, 0, 0, 0);
        rb[r] = in ? *reinterpret_cast<const float4*>(pb[r] + k0) : make_float4(0, 0, 0, 0);
        if (AMUL && in) ra[r] = amul4(ra[r], *reinterpret_cast<const float4*>(py[r] + k0), am);
      } else {
        const int gm = m0 + row, gn = n0 + row;
        ra[r] = (gm < M) ? load4_guard(A + (int64_t)gm * lda + k, K - k, a_vec) : make_float4(0, 0, 0, 0);
        rb[r] = (gn < N) ? load4_guard(B + (int64_t)gn * ldb + k, K - k, b_vec) : make_float4(0, 0, 0, 0);
        if (AMUL && gm < M) ra[r] = amul4(ra[r], load4_guard(am.Y + (int64_t)gm * am.ldy + k, K - k, false), am);
      }
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = tid + kBlk * r;
      const int row = idx >> 3, c4 = idx & 7;
      *reinterpret_cast<float4*>(As + (buf * TBM + row) * LDK + c4 * 4) = ra[r];
      *reinterpret_cast<float4*>(Bs + (buf * TBN + row) * LDK + c4 * 4) = rb[r];
    }
  };

  const int nk = (K + BK - 1) / BK;
  gload(0);
  lstore(0);
  __syncthreads();
  const int arow = wm * WT + (lane & 31), brow = wn * WT + (lane & 31), khalf = (lane >> 5) * 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * BK);
    if (BF3) {
      // bf16x6: per 16-column step every lane converts its 8 consecutive k of each operand row into three bf16
      // pieces (registers only; LDS still holds f32) and issues six bf16 MFMAs per 32x32 tile, small terms first
      const float* as = As + (buf * TBM + arow) * LDK + 2 * khalf;
      const float* bs = Bs + (buf * TBN + brow) * LDK + 2 * khalf;
#pragma unroll
      for (int ks = 0; ks < BK / 16; ++ks) {
        Pieces pa[T], pb[T];
#pragma unroll
        for (int i = 0; i < T; ++i) {
          const float* ap = as + i * 32 * LDK + ks * 16;
          const float* bp = bs + i * 32 * LDK + ks * 16;
          pa[i] = split8(*reinterpret_cast<const float4*>(ap), *reinterpret_cast<const float4*>(ap + 4));
          pb[i] = split8(*reinterpret_cast<const float4*>(bp), *reinterpret_cast<const float4*>(bp + 4));
        }
#pragma unroll
        for (int mi = 0; mi < T; ++mi)
#pragma unroll
          for (int ni = 0; ni < T; ++ni) {
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].h, pb[ni].l, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].l, pb[ni].h, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].m, pb[ni].m, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].h, pb[ni].m, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].m, pb[ni].h, acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mi].h, pb[ni].h, acc[mi][ni], 0, 0, 0);
          }
      }
    } else {
    const float* as = As + (buf * TBM + arow) * LDK + khalf;
    const float* bs = Bs + (buf * TBN + brow) * LDK + khalf;
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 a[T], b[T];
#pragma unroll
      for (int i = 0; i < T; ++i) {
        a[i] = *reinterpret_cast<const float4*>(as + i * 32 * LDK + kk * 8);
        b[i] = *reinterpret_cast<const float4*>(bs + i * 32 * LDK + kk * 8);
      }
#pragma unroll
      for (int mi = 0; mi < T; ++mi)
#pragma unroll
        for (int ni = 0; ni < T; ++ni) {
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].x, b[ni].x, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].y, b[ni].y, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].z, b[ni].z, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].w, b[ni].w, acc[mi][ni], 0, 0, 0);
        }
    }
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  // accumulators -> LDS: D[row][col], col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  constexpr int LDC = TBN + 4;
  float* Cs = smem;                        // [TBM][LDC] <= the operand buffers
#pragma unroll
  for (int mi = 0; mi < T; ++mi)
#pragma unroll
    for (int ni = 0; ni < T; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * WT + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = wn * WT + ni * 32 + (lane & 31);
        Cs[row * LDC + col] = acc[mi][ni][r];
      }
  __syncthreads();
  switch (act) {
    case RECMV_ACT_RELU:
      nt_epilogue<T, RECMV_ACT_RELU>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
      break;
    case RECMV_ACT_SOFTPLUS:
      nt_epilogue<T, RECMV_ACT_SOFTPLUS>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
      break;
    case RECMV_ACT_TANH:
      nt_epilogue<T, RECMV_ACT_TANH>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
      break;
    default:
      nt_epilogue<T, RECMV_ACT_NONE>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
  }
}

// ------------------------------------------------------------------------------------------ NT 128x128, three workgroups per CU
// The 128x128 f32 kernel above keeps two K-tiles of both operands in LDS (72 KB): two workgroups per CU, i.e. two waves per SIMD, and
// with K = 512 a workgroup lives for only 16 K-tiles — its prologue (first operand tile from HBM) and its epilogue (accumulators ->
// LDS -> activation -> HBM) leave its SIMD partner alone with the matrix pipe for ~15 % of its life, and one wave alone does not
// keep the pipe busy across its own barriers.  This variant holds LESS in LDS so that THREE workgroups fit a CU (registers allow
// exactly three: 94 + 64 accumulators): either one K-tile of 32 columns (SINGLE: the next tile waits in registers, two barriers per
// tile) or two K-tiles of 16 columns; the epilogue goes through LDS in two halves of 64 rows.  Same products in the same order
// as gemm_nt_kernel<2, true, ...>: bit-identical results.

// SCAL: operands that miss the 16-byte conditions (a leading dimension or K that is no multiple of 4, an unaligned base) are staged with
// loads that need only dword alignment (load4_dword), the last group of a row's K range element by element — the LDS image is that of the aligned kernel on a
// zero-padded copy and the MFMA order is the same, so the results are bit-identical to it.
template <bool AMUL, int BKT, bool SINGLE, int MI, int NI, bool SCAL = false>
__global__ __launch_bounds__(kBlk, (MI * NI == 4 ? (BKT <= 16 ? 4 : 3) : 5))
void gemm_nt_occ_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                        const float* __restrict__ bias, float* __restrict__ C, int64_t ldc, int M, int N, int K, int act,
                        float act_param, float out_scale, int nbm, int nbn, bool c_vec, AMul am, bool a_vec, bool b_vec) {
  constexpr int TBM = 64 * MI, TBN = 64 * NI;   // workgroup tile; 2 x 2 waves of (32 MI) x (32 NI)
  constexpr int LDKT = BKT + 4;                 // padded k stride (floats) of an LDS row
  constexpr int C4R = BKT / 4;                  // float4 per operand row and K-tile
  constexpr int NLA = TBM * C4R / kBlk, NLB = TBN * C4R / kBlk;   // float4 per thread per operand tile
  constexpr int NBUF = SINGLE ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                             // [NBUF][TBM][LDKT]
  float* Bs = smem + NBUF * TBM * LDKT;         // [NBUF][TBN][LDKT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t logical = xcd_remap(blockIdx.x, (int64_t)nbm * nbn);
  const int tile_m = (int)(logical / nbn), tile_n = (int)(logical % nbn);
  const int m0 = tile_m * TBM, n0 = tile_n * TBN;
  seg_operands(am, m0, B, bias);
  f32x16 acc[MI][NI];
#pragma unroll
  for (int a = 0; a < MI; ++a)
#pragma unroll
    for (int b = 0; b < NI; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  float4 ra[NLA], rb[NLB];
  const float* pa[NLA];
  const float* pb[NLB];
  const float* py[NLA];
  bool va[NLA], vb[NLB];
#pragma unroll
  for (int r = 0; r < NLA; ++r) {
    const int idx = tid + kBlk * r;
    int gm = m0 + idx / C4R;
    gm = gm < M ? gm : M - 1;                   // clamped rows are computed and never stored
    pa[r] = A + (int64_t)gm * lda + (idx % C4R) * 4;
    if (AMUL) py[r] = am.Y + (int64_t)gm * am.ldy + (idx % C4R) * 4;
    va[r] = a_vec && gm < M - 1;                // SCAL: the last row's padding need not exist
  }
#pragma unroll
  for (int r = 0; r < NLB; ++r) {
    const int idx = tid + kBlk * r;
    int gn = n0 + idx / C4R;
    gn = gn < N ? gn : N - 1;
    pb[r] = B + (int64_t)gn * ldb + (idx % C4R) * 4;
    vb[r] = b_vec && gn < N - 1;
  }
  auto gload = [&](int k0) {
#pragma unroll
    for (int r = 0; r < NLA; ++r) {
      const int k = k0 + ((tid + kBlk * r) % C4R) * 4;
      if (SCAL) {
        // 16-byte aligned rows (lda % 4 == 0, so the next row starts past K rounded up to 4): one 16-byte load, the elements past K dropped
        ra[r] = va[r] ? keep4(k < K ? *reinterpret_cast<const float4*>(pa[r] + k0) : make_float4(0, 0, 0, 0), K - k)
                      : load4_dword(pa[r] + k0, K - k);
        if (AMUL && k < K)
          ra[r] = amul4(ra[r], va[r] ? keep4(*reinterpret_cast<const float4*>(py[r] + k0), K - k)
                                     : load4_dword(py[r] + k0, K - k), am);
        continue;
      }
      const bool in = k < K;       // K % 4 == 0: a float4 is entirely inside or outside
      ra[r] = in ? *reinterpret_cast<const float4*>(pa[r] + k0) : make_float4(0, 0, 0, 0);
      if (AMUL && in) ra[r] = amul4(ra[r], *reinterpret_cast<const float4*>(py[r] + k0), am);
    }
#pragma unroll
    for (int r = 0; r < NLB; ++r) {
      const int k = k0 + ((tid + kBlk * r) % C4R) * 4;
      if (SCAL) {
        rb[r] = vb[r] ? keep4(k < K ? *reinterpret_cast<const float4*>(pb[r] + k0) : make_float4(0, 0, 0, 0), K - k)
                      : load4_dword(pb[r] + k0, K - k);
        continue;
      }
      const bool in = k < K;
      rb[r] = in ? *reinterpret_cast<const float4*>(pb[r] + k0) : make_float4(0, 0, 0, 0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < NLA; ++r) {
      const int idx = tid + kBlk * r;
      *reinterpret_cast<float4*>(As + (buf * TBM + idx / C4R) * LDKT + (idx % C4R) * 4) = ra[r];
    }
#pragma unroll
    for (int r = 0; r < NLB; ++r) {
      const int idx = tid + kBlk * r;
      *reinterpret_cast<float4*>(Bs + (buf * TBN + idx / C4R) * LDKT + (idx % C4R) * 4) = rb[r];
    }
  };

  const int nk = (K + BKT - 1) / BKT;
  gload(0);
  lstore(0);
  __syncthreads();
  const int arow = wm * 32 * MI + (lane & 31), brow = wn * 32 * NI + (lane & 31), khalf = (lane >> 5) * 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = SINGLE ? 0 : (kt & 1);
    if (kt + 1 < nk) gload((kt + 1) * BKT);
    const float* as = As + (buf * TBM + arow) * LDKT + khalf;
    const float* bs = Bs + (buf * TBN + brow) * LDKT + khalf;
#pragma unroll
    for (int kk = 0; kk < BKT / 8; ++kk) {
      float4 a[MI], b[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const float4*>(as + i * 32 * LDKT + kk * 8);
#pragma unroll
      for (int i = 0; i < NI; ++i) b[i] = *reinterpret_cast<const float4*>(bs + i * 32 * LDKT + kk * 8);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].x, b[ni].x, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].y, b[ni].y, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].z, b[ni].z, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].w, b[ni].w, acc[mi][ni], 0, 0, 0);
        }
    }
    if (SINGLE) __syncthreads();                 // every wave has read the tile: the buffer may be overwritten
    if (kt + 1 < nk) lstore(SINGLE ? 0 : (buf ^ 1));
    __syncthreads();
  }

  // accumulators -> LDS -> HBM in two passes: pass h takes the rows of the waves with wm == h (the half-tile fits the LDS the
  // occupancy allows)
  constexpr int HR = 32 * MI, LDC = TBN + 4;
  float* Cs = smem;                              // [HR][LDC]
  const AMul em = AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();
    if (wm == h) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int col = wn * 32 * NI + ni * 32 + (lane & 31);
            Cs[row * LDC + col] = acc[mi][ni][r];
          }
    }
    __syncthreads();
    const int mh = m0 + HR * h;
    switch (act) {
      case RECMV_ACT_RELU:
        nt_epilogue_rows<HR, TBN, RECMV_ACT_RELU>(Cs, bias, C, ldc, M, N, mh, n0, act_param, out_scale, c_vec, em);
        break;
      case RECMV_ACT_SOFTPLUS:
        nt_epilogue_rows<HR, TBN, RECMV_ACT_SOFTPLUS>(Cs, bias, C, ldc, M, N, mh, n0, act_param, out_scale, c_vec, em);
        break;
      case RECMV_ACT_TANH:
        nt_epilogue_rows<HR, TBN, RECMV_ACT_TANH>(Cs, bias, C, ldc, M, N, mh, n0, act_param, out_scale, c_vec, em);
        break;
      default:
        nt_epilogue_rows<HR, TBN, RECMV_ACT_NONE>(Cs, bias, C, ldc, M, N, mh, n0, act_param, out_scale, c_vec, em);
    }
  }
}

// ------------------------------------------------------------------------------------------ NT, skinny shapes (f32 mode)
// The networks end in layers of 1 or 3 outputs (SDF value, offset MLP).  On the MFMA kernels their forward is a 128-column tile of
// which 1-3 columns are real, and their input gradient (K = 1 or 3) is a 32-deep K-tile of which 1-3 steps are real.  Both are
// bounded by ONE pass over the [M, 512] side of the product, and both are done here on the VALU with the summation order of the
// MFMA kernels, so every launch keeps the bits it had on them (the route depends on N and K only).
//
// Order of the MFMA kernels above: a v_mfma_f32_32x32x2_f32 is acc = fma(a[k1], b[k1], fma(a[k0], b[k0], acc)) with k0 from lanes
// 0-31 and k1 from lanes 32-63, and the lanes 32-63 read their operands 4 columns further (khalf) — so within every group of 8
// consecutive k the chain runs k = 0, 4, 1, 5, 2, 6, 3, 7, the groups in ascending order, columns past K as exact zeros.  The 64 x 32
// kernel of the small launches keeps columns 0-15 and 16-31 of every K-tile on two chains and adds them before the bias; for K <= 4 that
// makes no difference, for N <= 4 the thin kernel does the same (`halves`) at the row counts where that kernel had the launch.
__device__ __forceinline__ float apply_act_rt(float z, int act, float p, float inv_p) {
  switch (act) {
    case RECMV_ACT_RELU: return apply_act<RECMV_ACT_RELU>(z, p, inv_p);
    case RECMV_ACT_SOFTPLUS: return apply_act<RECMV_ACT_SOFTPLUS>(z, p, inv_p);
    case RECMV_ACT_TANH: return apply_act<RECMV_ACT_TANH>(z, p, inv_p);
    default: return z;
  }
}

// N = NN <= 4 outputs, any K.  128 rows per workgroup, one thread per row: the [128][32] activation tile goes through LDS (coalesced
// 128-byte row segments from HBM, 16-byte conflict-free reads: row stride 36 floats), the NN weight rows ride along as a [4][32]
// tile that every lane reads at the same address.  VEC: 16-byte staging loads (aligned A, lda and K multiples of 4).
constexpr int kThinRows = 128;
template <int NN, bool VEC>
__global__ __launch_bounds__(kThinRows) void gemm_nt_thin_n_kernel(const float* __restrict__ A, int64_t lda,
                                                                   const float* __restrict__ B, int64_t ldb,
                                                                   const float* __restrict__ bias, float* __restrict__ C,
                                                                   int64_t ldc, int M, int K, int act, float act_param,
                                                                   float out_scale, bool halves, AMul am) {
  __shared__ __attribute__((aligned(16))) float As[kThinRows * LDK];
  __shared__ __attribute__((aligned(16))) float Bs[4 * LDK];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * kThinRows;
  seg_operands(am, m0, B, bias);
  constexpr int NLD = kThinRows * 8 / kThinRows;   // float4 per thread and K-tile
  float4 ra[NLD];
  float rb;
  const float* pa[NLD];
#pragma unroll
  for (int r = 0; r < NLD; ++r) {
    const int idx = tid + kThinRows * r;
    int gm = m0 + (idx >> 3);
    gm = gm < M ? gm : M - 1;                   // clamped rows are computed and never stored
    pa[r] = A + (int64_t)gm * lda + (idx & 7) * 4;
  }
  const int bn = tid >> 5, bk = tid & 31;
  auto gload = [&](int k0) {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int k = k0 + ((tid + kThinRows * r) & 7) * 4;
      if (VEC)
        ra[r] = k < K ? *reinterpret_cast<const float4*>(pa[r] + k0) : make_float4(0, 0, 0, 0);
      else
        ra[r] = load4_dword(pa[r] + k0, K - k);
    }
    rb = (bn < NN && k0 + bk < K) ? B[(int64_t)bn * ldb + k0 + bk] : 0.f;
  };
  auto lstore = [&]() {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = tid + kThinRows * r;
      *reinterpret_cast<float4*>(As + (idx >> 3) * LDK + (idx & 7) * 4) = ra[r];
    }
    Bs[bn * LDK + bk] = rb;
  };
  float acc[2][NN];
#pragma unroll
  for (int n = 0; n < NN; ++n) acc[0][n] = acc[1][n] = 0.f;
  const int nk = (K + BK - 1) / BK;
  gload(0);
  lstore();
  __syncthreads();
  const float* as = As + tid * LDK;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) gload((kt + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      const float4 a0 = *reinterpret_cast<const float4*>(as + kk * 8);
      const float4 a1 = *reinterpret_cast<const float4*>(as + kk * 8 + 4);
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        const float4 b0 = *reinterpret_cast<const float4*>(Bs + n * LDK + kk * 8);
        const float4 b1 = *reinterpret_cast<const float4*>(Bs + n * LDK + kk * 8 + 4);
        const int h = (halves && kk >= BK / 16) ? 1 : 0;      // `halves`: columns 16-31 of every K-tile on a chain of their own
        float s = acc[h][n];
        s = fmaf(a0.x, b0.x, s);
        s = fmaf(a1.x, b1.x, s);
        s = fmaf(a0.y, b0.y, s);
        s = fmaf(a1.y, b1.y, s);
        s = fmaf(a0.z, b0.z, s);
        s = fmaf(a1.z, b1.z, s);
        s = fmaf(a0.w, b0.w, s);
        s = fmaf(a1.w, b1.w, s);
        acc[h][n] = s;
      }
    }
    __syncthreads();                             // every thread has read the tile: the buffer may be overwritten
    if (kt + 1 < nk) lstore();
    __syncthreads();
  }
  const int gm = m0 + tid;
  if (gm >= M) return;
  const float inv_p = act_param != 0.f ? 1.f / act_param : 0.f;
#pragma unroll
  for (int n = 0; n < NN; ++n) {
    const float z = halves ? acc[0][n] + acc[1][n] : acc[0][n];
    float v = apply_act_rt(z + (bias ? bias[n] : 0.f), act, act_param, inv_p) * out_scale;
    if (am.Y) v *= dact_hw(am.Y[(int64_t)gm * am.ldy + n] * am.y_scale, am.act, am.param) * am.a_scale;
    C[(int64_t)gm * ldc + n] = v;
  }
}

// K = KK <= 4, any N: C = act(A' . B^T + bias) * out_scale as one element-wise pass, A' = A or (AMUL) A (.) act'(y_scale Y) a_scale.
// 32 rows per workgroup; `cw` = 2^cw_log2 threads span the float4 column strips of a row (a wave writes 1 KB of a row at N = 512),
// the other 256 / cw take turns over the rows; a thread keeps its 4 x KK weights in registers across its rows.
constexpr int kThinKRows = 32;
template <int KK, bool AMUL>
__global__ __launch_bounds__(kBlk) void gemm_nt_thin_k_kernel(const float* __restrict__ A, int64_t lda,
                                                              const float* __restrict__ B, int64_t ldb,
                                                              const float* __restrict__ bias, float* __restrict__ C,
                                                              int64_t ldc, int M, int N, int act, float act_param,
                                                              float out_scale, int cw_log2, bool c_vec, AMul am) {
  const int tid = threadIdx.x;
  const int cw = 1 << cw_log2, cl = tid & (cw - 1), rsub = tid >> cw_log2, rstep = kBlk >> cw_log2;
  const int m0 = blockIdx.x * kThinKRows;
  const int mend = m0 + kThinKRows < M ? m0 + kThinKRows : M;
  if (am.B2 && m0 >= am.split) {              // (written out: through seg_operands this kernel's instructions come out differently)
    B = am.B2;
    bias = am.bias2;
  }
  const float inv_p = act_param != 0.f ? 1.f / act_param : 0.f;
  for (int gn = cl * 4; gn < N; gn += cw * 4) {
    float b[4][KK], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bv[j] = (bias && gn + j < N) ? bias[gn + j] : 0.f;
#pragma unroll
      for (int k = 0; k < KK; ++k) b[j][k] = gn + j < N ? B[(int64_t)(gn + j) * ldb + k] : 0.f;
    }
    const bool full4 = c_vec && gn + 4 <= N;
    for (int gm = m0 + rsub; gm < mend; gm += rstep) {
      float a[KK];
#pragma unroll
      for (int k = 0; k < KK; ++k) {
        a[k] = A[(int64_t)gm * lda + k];
        if (AMUL) a[k] *= dact_hw(am.Y[(int64_t)gm * am.ldy + k] * am.y_scale, am.act, am.param) * am.a_scale;
      }
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k) s = fmaf(a[k], b[j][k], s);
        o[j] = apply_act_rt(s + bv[j], act, act_param, inv_p) * out_scale;
      }
      float4 v = make_float4(o[0], o[1], o[2], o[3]);
      if (!AMUL && am.Y) v = emul4(v, am, gm, gn, N);
      float* dst = C + (int64_t)gm * ldc + gn;
      if (full4) {
        *reinterpret_cast<float4*>(dst) = v;
      } else {
        dst[0] = v.x;
        if (gn + 1 < N) dst[1] = v.y;
        if (gn + 2 < N) dst[2] = v.z;
        if (gn + 3 < N) dst[3] = v.w;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ NT, bf16x6 staged
// The bf16x6 mode with the 3-way split done ONCE per operand element, on the global -> LDS staging path (8 elements
// per thread and item: two 16-byte loads, 44 VALU, three 16-byte LDS stores), instead of once per wave that reads the
// element as an MFMA fragment: the main loop is then 16-byte fragment reads + bf16 MFMAs, with the split's VALU issued
// in the shadow of the MFMAs (about four per MFMA).
// LDS image of an operand tile: three planes (h, m, l) of [rows][32 k] bf16, row = 64 bytes = four 16-byte chunks,
// chunk c of row r stored at chunk position c ^ ((r >> 2) & 3): the four 16-lane groups of a ds_read_b128 fragment
// read (rows {0-3,12-15,20-27}+.. at one chunk) and the 8-lane groups of the ds_write_b128 stores (two rows x four
// chunks) each cover distinct 16-byte bank slots, without padding.  One LDS buffer (48 KB of operands for 128x128; two
// workgroups per CU, each covering the other's barriers and epilogue).
// Pipeline per K-tile kt (raw = f32 as loaded, pieces = packed bf16 planes, both in registers): the raw registers hold
// tile kt+1 (requested during the previous iteration); it is split while the first 16 columns of tile kt are multiplied
// (each MFMA followed by its share of the split's VALU), tile kt+2 is requested as soon as the raw registers are free,
// the second 16 columns are multiplied, then barrier, pieces -> LDS, barrier.
// Measured alternatives that were slower (profiles/r02_gemm_staged_split.txt): two raw A sets with the A request a whole
// K-tile ahead (-6 %), accumulators taking turns between consecutive MFMAs (-5 %): the loop is bound by the SIMD's issue
// slots (about 6 non-MFMA instructions per MFMA across the two co-resident waves), not by latency.
__device__ __forceinline__ int b3_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// PRE: the B operand (a weight matrix, re-read by every row tile of every launch of an optimiser step) arrives already split —
// three bf16 planes [3][rows][Kp] (Kp = K rounded up to a K-tile, zero-padded) written once per weight version by
// recmv_b3_split with the SAME split8 as the staging path, so the pieces, the products and their order are those of the in-loop
// split (bit-identical results).  The B half of the split's VALU (44 per 8 elements) leaves the loop, which is bound by its issue
// slots; a thread's three 16-byte plane chunks of K-tile kt + 2 are requested behind the LDS stores of tile kt + 1 and stored one
// K-tile later.
struct B3Pre {
  const char* planes;        // first weight set
  const char* planes2;       // second weight set (row-segmented launches), or NULL
  int64_t plane_bytes, plane_bytes2;
  int Kp;
};

template <int T, bool AMUL, bool PRE>
__global__ __launch_bounds__(kBlk, 2) void gemm_nt_b3_kernel(const float* __restrict__ A, int64_t lda,
                                                             const float* __restrict__ B, int64_t ldb,
                                                             const float* __restrict__ bias, float* __restrict__ C,
                                                             int64_t ldc, int M, int N, int K, int act,
                                                             float act_param, float out_scale, int nbm, int nbn,
                                                             bool c_vec, AMul am, B3Pre pre) {
  constexpr int TBM = 64 * T, TBN = 64 * T, WT = 32 * T;
  constexpr int NI = TBM * 4 / kBlk;            // (row, 8-k chunk) items per thread and operand: 2 or 1
  constexpr int PLANE = TBM * 64;               // bytes of one plane of one operand tile
  constexpr int NSET = 1;                       // raw A register sets
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* As = reinterpret_cast<char*>(smem);     // [3][TBM][64 B]
  char* Bs = As + 3 * PLANE;                    // [3][TBN][64 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t logical = xcd_remap(blockIdx.x, (int64_t)nbm * nbn);
  const int tile_m = (int)(logical / nbn), tile_n = (int)(logical % nbn);
  const int m0 = tile_m * TBM, n0 = tile_n * TBN;
  const char* planes = pre.planes;
  int64_t plane_bytes = pre.plane_bytes;
  if (am.B2 && m0 >= am.split) {              // second weight set for the rows of the second net (see AMul)
    B = am.B2;
    bias = am.bias2;
    planes = pre.planes2;
    plane_bytes = pre.plane_bytes2;
  }

  f32x16 acc[T][T];
#pragma unroll
  for (int a = 0; a < T; ++a)
#pragma unroll
    for (int b = 0; b < T; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  float4 ra[NSET][NI][2], rb[NI][2], ry[AMUL ? NI : 1][2];
  u32x4 sa[NI][3], sb[NI][3];
  const float* pa[NI];
  const float* pb[NI];
  const char* pq[NI];
  const float* py[NI];
  int soff[NI];
#pragma unroll
  for (int r = 0; r < NI; ++r) {
    const int item = tid + kBlk * r;
    const int row = item >> 2, ch = item & 3;
    int gm = m0 + row, gn = n0 + row;
    gm = gm < M ? gm : M - 1;                   // clamped rows are computed and never stored
    gn = gn < N ? gn : N - 1;
    pa[r] = A + (int64_t)gm * lda + ch * 8;
    pb[r] = B + (int64_t)gn * ldb + ch * 8;
    if (PRE) pq[r] = planes + ((int64_t)gn * pre.Kp + ch * 8) * 2;
    if (AMUL) py[r] = am.Y + (int64_t)gm * am.ldy + ch * 8;
    soff[r] = b3_off(row, ch);
  }
  const int kch = (tid & 3) * 8;
  const int nk = (K + BK - 1) / BK;
  // Offsets of a thread's two float4 of K-tile t, and whether they are inside K (K % 4 == 0: a float4 is entirely
  // inside or outside; an outside one reads the row's last float4 and is zeroed).  Whole tiles take the plain path.
#define RECMV_KEEP4(v, c) v = make_float4((c) ? v.x : 0.f, (c) ? v.y : 0.f, (c) ? v.z : 0.f, (c) ? v.w : 0.f)
  auto load_a = [&](auto set_c, auto whole_c, int t) __attribute__((always_inline)) {
    constexpr int S = decltype(set_c)::value;
    const int k0 = t * BK, k = k0 + kch;
    const bool in0 = decltype(whole_c)::value || k < K, in1 = decltype(whole_c)::value || k + 4 < K;
    const int o0 = in0 ? k0 : K - 4 - kch, o1 = in1 ? k0 + 4 : K - 4 - kch;
#pragma unroll
    for (int r = 0; r < NI; ++r) {
      ra[S][r][0] = *reinterpret_cast<const float4*>(pa[r] + o0);
      ra[S][r][1] = *reinterpret_cast<const float4*>(pa[r] + o1);
      if (AMUL) {
        ry[r][0] = *reinterpret_cast<const float4*>(py[r] + o0);
        ry[r][1] = *reinterpret_cast<const float4*>(py[r] + o1);
      }
      if (!decltype(whole_c)::value) {
        RECMV_KEEP4(ra[S][r][0], in0);
        RECMV_KEEP4(ra[S][r][1], in1);
      }
    }
  };
  auto load_b = [&](auto whole_c, int t) __attribute__((always_inline)) {
    const int k0 = t * BK, k = k0 + kch;
    const bool in0 = decltype(whole_c)::value || k < K, in1 = decltype(whole_c)::value || k + 4 < K;
    const int o0 = in0 ? k0 : K - 4 - kch, o1 = in1 ? k0 + 4 : K - 4 - kch;
#pragma unroll
    for (int r = 0; r < NI; ++r) {
      rb[r][0] = *reinterpret_cast<const float4*>(pb[r] + o0);
      rb[r][1] = *reinterpret_cast<const float4*>(pb[r] + o1);
      if (!decltype(whole_c)::value) {
        RECMV_KEEP4(rb[r][0], in0);
        RECMV_KEEP4(rb[r][1], in1);
      }
    }
  };
#undef RECMV_KEEP4
  auto load_b_pre = [&](int t) __attribute__((always_inline)) {      // pieces of K-tile t straight into the store registers
#pragma unroll
    for (int r = 0; r < NI; ++r)
#pragma unroll
      for (int p = 0; p < 3; ++p) sb[r][p] = *reinterpret_cast<const u32x4*>(pq[r] + p * plane_bytes + (int64_t)t * (BK * 2));
  };
  auto split_a = [&](auto set_c) __attribute__((always_inline)) {
    constexpr int S = decltype(set_c)::value;
#pragma unroll
    for (int r = 0; r < NI; ++r) {
      if (AMUL) {
        ra[S][r][0] = amul4(ra[S][r][0], ry[r][0], am);
        ra[S][r][1] = amul4(ra[S][r][1], ry[r][1], am);
      }
      const Pieces a = split8(ra[S][r][0], ra[S][r][1]);
      sa[r][0] = __builtin_bit_cast(u32x4, a.h);
      sa[r][1] = __builtin_bit_cast(u32x4, a.m);
      sa[r][2] = __builtin_bit_cast(u32x4, a.l);
    }
  };
  // keeps everything computed from `v` behind this point of the instruction stream (the split is pure arithmetic: without
  // it the compiler may start it ahead of the scheduling barrier, right behind the loads it waits for)
  auto pin4 = [&](float4& v) __attribute__((always_inline)) {
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
  };
  auto split_b = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < NI; ++r) {
      pin4(rb[r][0]);
      pin4(rb[r][1]);
      const Pieces b = split8(rb[r][0], rb[r][1]);
      sb[r][0] = __builtin_bit_cast(u32x4, b.h);
      sb[r][1] = __builtin_bit_cast(u32x4, b.m);
      sb[r][2] = __builtin_bit_cast(u32x4, b.l);
    }
  };
  auto lstore = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < NI; ++r)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        *reinterpret_cast<u32x4*>(As + p * PLANE + soff[r]) = sa[r][p];
        *reinterpret_cast<u32x4*>(Bs + p * PLANE + soff[r]) = sb[r][p];
      }
  };
  const int arow = wm * WT + (lane & 31), brow = wn * WT + (lane & 31), kh = lane >> 5;
  const int aswz = (arow >> 2) & 3, bswz = (brow >> 2) & 3;   // (+32 rows leaves the swizzle unchanged)
  bf16x8 fa[T][3], fb[T][3];
  auto reads = [&](int ks) __attribute__((always_inline)) {
    const char* ap = As + arow * 64 + (((ks * 2 + kh) ^ aswz) << 4);
    const char* bp = Bs + brow * 64 + (((ks * 2 + kh) ^ bswz) << 4);
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[i][p] = *reinterpret_cast<const bf16x8*>(ap + p * PLANE + i * 32 * 64);
        fb[i][p] = *reinterpret_cast<const bf16x8*>(bp + p * PLANE + i * 32 * 64);
      }
  };
  auto mfmas = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int mi = 0; mi < T; ++mi)
#pragma unroll
      for (int ni = 0; ni < T; ++ni) {     // piece products hl, lh, mm, hm, mh, hh: small terms first
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][0], fb[ni][2], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][2], fb[ni][0], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][1], fb[ni][1], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][0], fb[ni][1], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][1], fb[ni][0], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi][0], fb[ni][0], acc[mi][ni], 0, 0, 0);
      }
  };
  // the scheduling pattern of half a K-tile: its fragment reads, then every MFMA followed by VALU of the split
  auto pattern = [&](auto valu_c) __attribute__((always_inline)) {
    constexpr int valu_per_mfma = decltype(valu_c)::value;
    __builtin_amdgcn_sched_group_barrier(0x100, 6 * T, 0);
#pragma unroll
    for (int i = 0; i < 6 * T * T; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, valu_per_mfma, 0);
    }
  };
  using Yes = std::integral_constant<bool, true>;
  using No = std::integral_constant<bool, false>;
  using S0 = std::integral_constant<int, 0>;

  {
    auto ktile = [&](auto whole_c, int kt) __attribute__((always_inline)) {
      __builtin_amdgcn_sched_barrier(0);
      reads(0);
      split_a(S0{});
      if (!PRE) split_b();
      if (decltype(whole_c)::value || kt + 2 < nk) {
        load_a(S0{}, whole_c, kt + 2);
        if (!PRE) load_b(whole_c, kt + 2);
      }
      mfmas();
      if (decltype(whole_c)::value) {
        pattern(std::integral_constant<int, PRE ? 4 : 8>{});
        __builtin_amdgcn_sched_group_barrier(0x020, ((AMUL ? 4 : 2) + (PRE ? 0 : 2)) * NI, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      reads(1);
      mfmas();
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      lstore();
      __syncthreads();
      if (PRE && (decltype(whole_c)::value || kt + 2 < nk)) load_b_pre(kt + 2);
    };
    load_a(S0{}, No{}, 0);
    if (PRE) load_b_pre(0);
    else load_b(No{}, 0);
    split_a(S0{});
    if (!PRE) split_b();
    lstore();
    if (nk > 1) {
      load_a(S0{}, No{}, 1);
      if (PRE) load_b_pre(1);
      else load_b(No{}, 1);
    }
    __syncthreads();
    int kt = 0;
    const int nwhole = K / BK;
    for (; kt + 2 < nwhole; ++kt) ktile(Yes{}, kt);
    for (; kt + 1 < nk; ++kt) ktile(No{}, kt);
  }
  reads(0);
  mfmas();
  reads(1);
  mfmas();
  __syncthreads();

  constexpr int LDC = TBN + 4;
  float* Cs = smem;                        // [TBM][LDC]
#pragma unroll
  for (int mi = 0; mi < T; ++mi)
#pragma unroll
    for (int ni = 0; ni < T; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * WT + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = wn * WT + ni * 32 + (lane & 31);
        Cs[row * LDC + col] = acc[mi][ni][r];
      }
  __syncthreads();
  switch (act) {
    case RECMV_ACT_RELU:
      nt_epilogue<T, RECMV_ACT_RELU>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
      break;
    case RECMV_ACT_SOFTPLUS:
      nt_epilogue<T, RECMV_ACT_SOFTPLUS>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
      break;
    case RECMV_ACT_TANH:
      nt_epilogue<T, RECMV_ACT_TANH>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
      break;
    default:
      nt_epilogue<T, RECMV_ACT_NONE>(Cs, bias, C, ldc, M, N, m0, n0, act_param, out_scale, c_vec, AMUL ? AMul{nullptr, 0, 0, 0.f, 1.f, 1.f} : am);
  }
}

// B [N][K] f32 (row stride ldb, K % 8 == 0) -> planes [3][N][Kp] bf16 (h, m, l of split8), zero beyond K.
__global__ __launch_bounds__(kBlk) void b3_split_kernel(const float* __restrict__ B, int64_t ldb, int64_t N, int K, int Kp,
                                                        char* __restrict__ planes) {
  const int c8 = Kp / 8;
  const int64_t items = N * c8, plane_bytes = N * (int64_t)Kp * 2;
  for (int64_t e = (int64_t)blockIdx.x * kBlk + threadIdx.x; e < items; e += (int64_t)gridDim.x * kBlk) {
    const int64_t row = e / c8;
    const int k = (int)(e - row * c8) * 8;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (k < K) {                                    // (K % 8 == 0: a chunk is entirely inside or outside)
      a = *reinterpret_cast<const float4*>(B + row * ldb + k);
      b = *reinterpret_cast<const float4*>(B + row * ldb + k + 4);
    }
    const Pieces p = split8(a, b);
    char* o = planes + (row * Kp + k) * 2;
    *reinterpret_cast<u32x4*>(o) = __builtin_bit_cast(u32x4, p.h);
    *reinterpret_cast<u32x4*>(o + plane_bytes) = __builtin_bit_cast(u32x4, p.m);
    *reinterpret_cast<u32x4*>(o + 2 * plane_bytes) = __builtin_bit_cast(u32x4, p.l);
  }
}

// ------------------------------------------------------------------------------------------ NT, narrow tile
// 64x32 workgroup tile for launches too small to give every CU three 64x64 workgroups (the ray path: M = 3072 rows
// against N = 512 is 384 tiles of 64x64 — 1.5 per CU, so half the CUs carry twice the work of the others — but 768
// tiles of 64x32 = 3 per CU).  The 4 waves are 2 (row halves) x 2 (halves of every K-tile): each wave owns one 32x32
// MFMA tile over half of K, the two K-halves are summed through LDS before the epilogue.
template <bool FAST, bool AMUL, bool BF3>
__global__ __launch_bounds__(kBlk) void gemm_nt_narrow_v1_kernel(const float* __restrict__ A, int64_t lda,
                                                                 const float* __restrict__ B, int64_t ldb,
                                                                 const float* __restrict__ bias, float* __restrict__ C,
                                                                 int64_t ldc, int M, int N, int K, int act,
                                                                 float act_param, float out_scale, int nbm, int nbn,
                                                                 bool a_vec, bool b_vec, bool c_vec, AMul am) {
  constexpr int TBM = 64, TBN = 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                        // [2][64][LDK]
  float* Bs = smem + 2 * TBM * LDK;        // [2][32][LDK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wk = wave >> 1;
  const int64_t logical = xcd_remap(blockIdx.x, (int64_t)nbm * nbn);
  const int tile_m = (int)(logical / nbn), tile_n = (int)(logical % nbn);
  const int m0 = tile_m * TBM, n0 = tile_n * TBN;
  seg_operands(am, m0, B, bias);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // staging: A 64 rows x 8 float4 (2 per thread), B 32 rows x 8 float4 (1 per thread)
  float4 ra[2], rb;
  const float* pa[2];
  const float* pb;
  const float* py[2];
  const int brow_s = tid >> 3, c4s = tid & 7;
  if (FAST) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      int gm = m0 + brow_s + 32 * r;
      gm = gm < M ? gm : M - 1;
      pa[r] = A + (int64_t)gm * lda + c4s * 4;
      if (AMUL) py[r] = am.Y + (int64_t)gm * am.ldy + c4s * 4;
    }
    int gn = n0 + brow_s;
    gn = gn < N ? gn : N - 1;
    pb = B + (int64_t)gn * ldb + c4s * 4;
  }
  auto gload = [&](int k0) {
    const int k = k0 + c4s * 4;
    if (FAST) {
      const bool in = k < K;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        ra[r] = in ? *reinterpret_cast<const float4*>(pa[r] + k0) : make_float4(0, 0, 0, 0);
        if (AMUL && in) ra[r] = amul4(ra[r], *reinterpret_cast<const float4*>(py[r] + k0), am);
      }
      rb = in ? *reinterpret_cast<const float4*>(pb + k0) : make_float4(0, 0, 0, 0);
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int gm = m0 + brow_s + 32 * r;
        ra[r] = (gm < M) ? load4_guard(A + (int64_t)gm * lda + k, K - k, a_vec) : make_float4(0, 0, 0, 0);
        if (AMUL && gm < M) ra[r] = amul4(ra[r], load4_guard(am.Y + (int64_t)gm * am.ldy + k, K - k, false), am);
      }
      const int gn = n0 + brow_s;
      rb = (gn < N) ? load4_guard(B + (int64_t)gn * ldb + k, K - k, b_vec) : make_float4(0, 0, 0, 0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
      *reinterpret_cast<float4*>(As + (buf * TBM + brow_s + 32 * r) * LDK + c4s * 4) = ra[r];
    *reinterpret_cast<float4*>(Bs + (buf * TBN + brow_s) * LDK + c4s * 4) = rb;
  };

  const int nk = (K + BK - 1) / BK;
  gload(0);
  lstore(0);
  __syncthreads();
  const int arow = wm * 32 + (lane & 31), brow = lane & 31, khalf = (lane >> 5) * 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * BK);
    if (BF3) {
      const float* ap = As + (buf * TBM + arow) * LDK + 2 * khalf + wk * 16;
      const float* bp = Bs + (buf * TBN + brow) * LDK + 2 * khalf + wk * 16;
      const Pieces a = split8(*reinterpret_cast<const float4*>(ap), *reinterpret_cast<const float4*>(ap + 4));
      const Pieces b = split8(*reinterpret_cast<const float4*>(bp), *reinterpret_cast<const float4*>(bp + 4));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, acc, 0, 0, 0);
    } else {
      const float* as = As + (buf * TBM + arow) * LDK + khalf + wk * 16;
      const float* bs = Bs + (buf * TBN + brow) * LDK + khalf + wk * 16;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const float4 a = *reinterpret_cast<const float4*>(as + kk * 8);
        const float4 b = *reinterpret_cast<const float4*>(bs + kk * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
      }
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  // the two K-halves -> two LDS planes [64][LDC]; the epilogue adds them
  constexpr int LDC = TBN + 4;
  float* Cs = smem;                        // [2][64][LDC] = 18.4 KB <= the operand buffers
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    Cs[(wk * TBM + row) * LDC + (lane & 31)] = acc[r];
  }
  __syncthreads();
  const int c4 = tid & 7, r0 = tid >> 3;   // 8 float4 strips per row, 32 rows per pass
  const int gn = n0 + c4 * 4;
  if (gn >= N) return;
  const float inv_p = act_param != 0.f ? 1.f / act_param : 0.f;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    bv.x = bias[gn];
    if (gn + 1 < N) bv.y = bias[gn + 1];
    if (gn + 2 < N) bv.z = bias[gn + 2];
    if (gn + 3 < N) bv.w = bias[gn + 3];
  }
  const bool full4 = c_vec && gn + 4 <= N;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int row = r0 + 32 * pass;
    const int gm = m0 + row;
    if (gm >= M) break;
    const float4 v0 = *reinterpret_cast<const float4*>(Cs + row * LDC + c4 * 4);
    const float4 v1 = *reinterpret_cast<const float4*>(Cs + (TBM + row) * LDC + c4 * 4);
    float4 v = make_float4(v0.x + v1.x + bv.x, v0.y + v1.y + bv.y, v0.z + v1.z + bv.z, v0.w + v1.w + bv.w);
    switch (act) {
      case RECMV_ACT_RELU:
        v.x = apply_act<RECMV_ACT_RELU>(v.x, act_param, inv_p);
        v.y = apply_act<RECMV_ACT_RELU>(v.y, act_param, inv_p);
        v.z = apply_act<RECMV_ACT_RELU>(v.z, act_param, inv_p);
        v.w = apply_act<RECMV_ACT_RELU>(v.w, act_param, inv_p);
        break;
      case RECMV_ACT_SOFTPLUS:
        v.x = apply_act<RECMV_ACT_SOFTPLUS>(v.x, act_param, inv_p);
        v.y = apply_act<RECMV_ACT_SOFTPLUS>(v.y, act_param, inv_p);
        v.z = apply_act<RECMV_ACT_SOFTPLUS>(v.z, act_param, inv_p);
        v.w = apply_act<RECMV_ACT_SOFTPLUS>(v.w, act_param, inv_p);
        break;
      case RECMV_ACT_TANH:
        v.x = apply_act<RECMV_ACT_TANH>(v.x, act_param, inv_p);
        v.y = apply_act<RECMV_ACT_TANH>(v.y, act_param, inv_p);
        v.z = apply_act<RECMV_ACT_TANH>(v.z, act_param, inv_p);
        v.w = apply_act<RECMV_ACT_TANH>(v.w, act_param, inv_p);
        break;
      default:
        break;
    }
    v.x *= out_scale;
    v.y *= out_scale;
    v.z *= out_scale;
    v.w *= out_scale;
    if (!AMUL && am.Y) v = emul4(v, am, gm, gn, N);
    float* dst = C + (int64_t)gm * ldc + gn;
    if (full4) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      if (gn + 1 < N) dst[1] = v.y;
      if (gn + 2 < N) dst[2] = v.z;
      if (gn + 3 < N) dst[3] = v.w;
    }
  }
}

// The kernel in use (RECMV_GEMM_NARROW=0 selects the one above): the same tile, wave layout, LDS image and epilogue, and for every output
// element the same sums in the same order — two chains over K (k mod 32 < 16 and the rest) in ascending tile order, within 8 consecutive k
// the order 0, 4, 1, 5, 2, 6, 3, 7, columns past K exact zeros, chain0 + chain1, then the bias — so its results are the bits of the kernel
// above.  What differs is the schedule of a K-tile:
//   - the barrier stands in the MIDDLE of a tile's 8 MFMAs and the fragments are double-buffered by half-tiles: after the barrier a wave
//     reads the first half-tile of tile kt+1 while the second half of tile kt (already in registers) feeds the pipe, so neither the LDS
//     read latency nor the other waves' skew at the barrier leaves the wave without an MFMA to issue;
//   - the staging registers of tile kt+1 go to LDS behind the first 4 MFMAs of tile kt, just in front of the barrier (they were loaded
//     at the same place of tile kt-1: 8 MFMAs and a barrier wait behind), so the wait for them and for the LDS stores runs under MFMAs
//     in flight, and the loads of tile kt+2 follow at once; the loads are unconditional at clamped addresses, the K tail is zeroed at
//     the LDS store and the operand transform is applied there, so nothing waits on a fresh load result;
//   - the unaligned instantiation loads whole groups of 4 as one dword-aligned access (load4_dword), like the SCAL kernels;
//   - without the operand transform the kernel is held to 64 registers (8 waves per SIMD), so that a workgroup fits beside resident
//     waves of the weight-gradient kernel.
// The bf16x6 mode (BF3) keeps the kernel above.
template <bool FAST, bool AMUL, bool BF3>
__global__ __launch_bounds__(kBlk) __attribute__((amdgpu_waves_per_eu(AMUL ? 4 : 8)))
void gemm_nt_narrow_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                           const float* __restrict__ bias, float* __restrict__ C, int64_t ldc, int M, int N, int K, int act,
                           float act_param, float out_scale, int nbm, int nbn, bool a_vec, bool b_vec, bool c_vec, AMul am) {
  static_assert(!BF3, "the bf16x6 mode runs gemm_nt_narrow_v1_kernel");
  constexpr int TBM = 64, TBN = 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                        // [2][64][LDK]
  float* Bs = smem + 2 * TBM * LDK;        // [2][32][LDK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wk = wave >> 1;
  const int64_t logical = xcd_remap(blockIdx.x, (int64_t)nbm * nbn);
  const int tile_m = (int)(logical / nbn), tile_n = (int)(logical % nbn);
  const int m0 = tile_m * TBM, n0 = tile_n * TBN;
  seg_operands(am, m0, B, bias);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // staging: A 64 rows x 8 float4 (2 per thread), B 32 rows x 8 float4 (1 per thread); rows past M / N are clamped to the last one (FAST)
  // or zero (otherwise): they reach no stored element
  float4 ra[2], ry[2], rb;
  const float* pa[2];
  const float* pb;
  const float* py[2];
  const int brow_s = tid >> 3, c4s = tid & 7;
  bool rowok[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    int gm = m0 + brow_s + 32 * r;
    rowok[r] = gm < M;
    gm = gm < M ? gm : M - 1;
    pa[r] = A + (int64_t)gm * lda + c4s * 4;
    if (AMUL) py[r] = am.Y + (int64_t)gm * am.ldy + c4s * 4;
  }
  int gnb = n0 + brow_s;
  const bool bok = gnb < N;
  gnb = bok ? gnb : N - 1;
  pb = B + (int64_t)gnb * ldb + c4s * 4;
  auto gload = [&](int k0) {
    const int k = k0 + c4s * 4;
    if (FAST) {
      const int ko = k < K ? k0 : K - 4 - c4s * 4;      // K % 4 == 0, K >= 4: the last float4 of the row instead of one past it
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        ra[r] = *reinterpret_cast<const float4*>(pa[r] + ko);
        if (AMUL) ry[r] = *reinterpret_cast<const float4*>(py[r] + ko);
      }
      rb = *reinterpret_cast<const float4*>(pb + ko);
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        ra[r] = rowok[r] ? load4_dword(pa[r] + k0, K - k) : make_float4(0, 0, 0, 0);
        if (AMUL) ry[r] = rowok[r] ? load4_dword(py[r] + k0, K - k) : make_float4(0, 0, 0, 0);
      }
      rb = bok ? load4_dword(pb + k0, K - k) : make_float4(0, 0, 0, 0);
    }
  };
  auto lstore = [&](int buf, int k0) {
    const int keep = (!FAST || k0 + c4s * 4 < K) ? 4 : 0;      // FAST: the staged float4 lies inside K or past it
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float4 v = ra[r];
      if (AMUL && (FAST || rowok[r])) v = amul4(v, ry[r], am);
      *reinterpret_cast<float4*>(As + (buf * TBM + brow_s + 32 * r) * LDK + c4s * 4) = keep4(v, keep);
    }
    *reinterpret_cast<float4*>(Bs + (buf * TBN + brow_s) * LDK + c4s * 4) = keep4(rb, keep);
  };

  const int nk = (K + BK - 1) / BK;
  gload(0);
  lstore(0, 0);
  if (nk > 1) gload(BK);
  __syncthreads();
  // fragments: lanes 0-31 hold k = 0..3 and lanes 32-63 k = 4..7 of each group of 8, so the MFMAs of a float4 take k in the order 0, 4, 1, 5, ...
  const float* as = As + (wm * 32 + (lane & 31)) * LDK + (lane >> 5) * 4 + wk * 16;
  const float* bs = Bs + (lane & 31) * LDK + (lane >> 5) * 4 + wk * 16;
  float4 a0 = *reinterpret_cast<const float4*>(as), b0 = *reinterpret_cast<const float4*>(bs);
  float4 a1 = *reinterpret_cast<const float4*>(as + 8), b1 = *reinterpret_cast<const float4*>(bs + 8);
  auto mfma4 = [&](const float4& a, const float4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  };
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    const int nb = (kt + 1) & 1;
    mfma4(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      lstore(nb, (kt + 1) * BK);           // buffer nb held tile kt-1: every wave finished reading it before the barrier of tile kt-1
      if (kt + 2 < nk) gload((kt + 2) * BK);
    }
    __syncthreads();
    if (more) {
      a0 = *reinterpret_cast<const float4*>(as + nb * TBM * LDK);
      b0 = *reinterpret_cast<const float4*>(bs + nb * TBN * LDK);
    }
    mfma4(a1, b1);
    if (more) {
      a1 = *reinterpret_cast<const float4*>(as + nb * TBM * LDK + 8);
      b1 = *reinterpret_cast<const float4*>(bs + nb * TBN * LDK + 8);
    }
  }

  // the two K-halves -> two LDS planes [64][LDC]; the epilogue adds them.  No wave reads an operand buffer after the last barrier above.
  constexpr int LDC = TBN + 4;
  float* Cs = smem;                        // [2][64][LDC] = 18.4 KB <= the operand buffers
  int te = tid;                            // the epilogue's indices are formed here, not kept in registers across the K loop
  asm volatile("" : "+v"(te));
  const int elane = te & 63, ewm = (te >> 6) & 1, ewk = te >> 7;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = ewm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (elane >> 5);
    Cs[(ewk * TBM + row) * LDC + (elane & 31)] = acc[r];
  }
  __syncthreads();
  const int c4 = te & 7, r0 = te >> 3;     // 8 float4 strips per row, 32 rows per pass
  const int gn = n0 + c4 * 4;
  if (gn >= N) return;
  const float inv_p = act_param != 0.f ? 1.f / act_param : 0.f;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    bv.x = bias[gn];
    if (gn + 1 < N) bv.y = bias[gn + 1];
    if (gn + 2 < N) bv.z = bias[gn + 2];
    if (gn + 3 < N) bv.w = bias[gn + 3];
  }
  const bool full4 = c_vec && gn + 4 <= N;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int row = r0 + 32 * pass;
    const int gm = m0 + row;
    if (gm >= M) break;
    const float4 v0 = *reinterpret_cast<const float4*>(Cs + row * LDC + c4 * 4);
    const float4 v1 = *reinterpret_cast<const float4*>(Cs + (TBM + row) * LDC + c4 * 4);
    float4 v = make_float4(v0.x + v1.x + bv.x, v0.y + v1.y + bv.y, v0.z + v1.z + bv.z, v0.w + v1.w + bv.w);
    switch (act) {
      case RECMV_ACT_RELU:
        v.x = apply_act<RECMV_ACT_RELU>(v.x, act_param, inv_p);
        v.y = apply_act<RECMV_ACT_RELU>(v.y, act_param, inv_p);
        v.z = apply_act<RECMV_ACT_RELU>(v.z, act_param, inv_p);
        v.w = apply_act<RECMV_ACT_RELU>(v.w, act_param, inv_p);
        break;
      case RECMV_ACT_SOFTPLUS:
        v.x = apply_act<RECMV_ACT_SOFTPLUS>(v.x, act_param, inv_p);
        v.y = apply_act<RECMV_ACT_SOFTPLUS>(v.y, act_param, inv_p);
        v.z = apply_act<RECMV_ACT_SOFTPLUS>(v.z, act_param, inv_p);
        v.w = apply_act<RECMV_ACT_SOFTPLUS>(v.w, act_param, inv_p);
        break;
      case RECMV_ACT_TANH:
        v.x = apply_act<RECMV_ACT_TANH>(v.x, act_param, inv_p);
        v.y = apply_act<RECMV_ACT_TANH>(v.y, act_param, inv_p);
        v.z = apply_act<RECMV_ACT_TANH>(v.z, act_param, inv_p);
        v.w = apply_act<RECMV_ACT_TANH>(v.w, act_param, inv_p);
        break;
      default:
        break;
    }
    v.x *= out_scale;
    v.y *= out_scale;
    v.z *= out_scale;
    v.w *= out_scale;
    if (!AMUL && am.Y) v = emul4(v, am, gm, gn, N);
    float* dst = C + (int64_t)gm * ldc + gn;
    if (full4) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      if (gn + 1 < N) dst[1] = v.y;
      if (gn + 2 < N) dst[2] = v.z;
      if (gn + 3 < N) dst[3] = v.w;
    }
  }
}

// ---- optional per-launch HIP-event timing of the MFMA kernels (bench.py's roofline object) ----------------------
// Events are recorded on the stream the kernel is launched on, immediately before and after the launch.
struct Profiler {
  bool on = false;
  double min_flops = 0.0;          // launches below this are counted but not bracketed by events
  double untimed[route::kNumSlots][2] = {};      // [variant][launches, flops]
  std::vector<LaunchRec> recs;
  std::vector<hipEvent_t> pool;
  double large[route::kNumSlots][3] = {};        // of the last recmv_profile_end: launches / seconds / FLOP of the bracketed launches of >= 4 GFLOP
  double timed_bytes[route::kNumSlots] = {};     // of the last recmv_profile_end: algorithmic bytes (4 (MK + NK + MN)) of the bracketed launches, per variant
  double busy_union_s = 0.0, busy_span_s = 0.0;   // of the last recmv_profile_end: union of the bracketed intervals, first start -> last end
  std::mutex mu;        // autograd's backward thread launches too
  hipEvent_t get() {
    std::lock_guard<std::mutex> lk(mu);
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
};
Profiler g_prof;

constexpr int kNtLds = (2 * BM * LDK + 2 * BN * LDK) * 4;   // 73728 B (T=2); half of it for T=1
constexpr int kNarrowLds = 2 * (64 + 32) * LDK * 4;         // 27648 B

// One NT product as the entry points hand it to dispatch_nt, which fills in the alignment flags.
struct NtCall {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  const float* bias;
  float* C;
  int64_t ldc, M, N, K;
  int act;
  float act_param, out_scale;
  AMul am;
  hipStream_t stream;
  bool a_vec, b_vec, c_vec;
};

}  // namespace

ScopedLaunchTimer::ScopedLaunchTimer(int variant, double M, double N, double K, hipStream_t stream) : s(stream), active(g_prof.on) {
  if (!active) return;
  const double flops = 2.0 * M * N * K;
  r.bytes = 4.0 * (M * K + N * K + M * N);
  if (flops < g_prof.min_flops) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.untimed[variant][0] += 1.0;
    g_prof.untimed[variant][1] += flops;
    active = false;
    return;
  }
  r.variant = variant;
  r.flops = flops;
  r.a = g_prof.get();
  r.b = g_prof.get();
  if (!r.a || !r.b) {
    active = false;
    return;
  }
  (void)hipEventRecord(r.a, s);
}
ScopedLaunchTimer::~ScopedLaunchTimer() {
  if (!active) return;
  (void)hipEventRecord(r.b, s);
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.recs.push_back(r);
}

void log_shape(const char* route, const char* parent, const LoggedShape& s) {
  static const bool on = [] { const char* e = getenv("RECMV_GEMM_SHAPES"); return e && e[0] == '1'; }();
  if (!on || !route::logged(s.M, s.N, s.K)) return;
  static std::mutex mu;
  static std::unordered_map<std::string, int> seen;
  char key[256];
  snprintf(key, sizeof key, "%s (before: %s) M=%lld N=%lld K=%lld lda=%lld ldb=%lld A%%16=%d B%%16=%d amul=%d emul=%d seg=%d", route, parent,
           (long long)s.M, (long long)s.N, (long long)s.K, (long long)s.lda, (long long)s.ldb, (int)(reinterpret_cast<uintptr_t>(s.A) & 15),
           (int)(reinterpret_cast<uintptr_t>(s.B) & 15), (int)s.amul, (int)s.emul, (int)s.seg);
  std::lock_guard<std::mutex> lk(mu);
  if (seen[key]++ == 0) fprintf(stderr, "[recmv shapes] %s\n", key);
}

}  // namespace recmv

using namespace recmv;
using route::NtKernel;
using route::NtPlan;

int g_b3_families = 7;   // mode 1 only: bit 0 the 128 x 128 NT kernels, bit 1 the 64 x 64 / 64 x 32 NT kernels, bit 2 the TN (dW) kernel
int g_gemm_mode = 0;     // 0: f32 MFMA (exact f32 products), 1: bf16x6 (3-way bf16 split, six bf16 MFMA products)

route::GemmSwitches recmv::gemm_switches() {
  static const bool occ = [] { const char* e = getenv("RECMV_GEMM_OCC"); return !(e && e[0] == '0'); }();   // =0: the two-per-CU kernels (A/B)
  const char* e = getenv("RECMV_GEMM_SKINNY");
  return {g_gemm_mode, g_b3_families, occ, !(e && e[0] == '0')};
}

// ---- launchers: one per kernel template.  The profile slot comes with the plan: a launch of a kernel added after the 14 slots were
// fixed is recorded under the slot of the kernel that took the launch before, so the per-step FLOP totals stay comparable.
template <int T, bool FAST, bool AMUL, bool BF3>
static int launch_nt(const NtCall& c, const NtPlan& p) {
  constexpr int lds = kNtLds / (T == 2 ? 1 : 2);
  static bool attr_set = false;
  if (!attr_set) {
    RECMV_HIP_TRY(hipFuncSetAttribute((const void*)gemm_nt_kernel<T, FAST, AMUL, BF3>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr_set = true;
  }
  const int nbm = (int)ceil_div(c.M, 64 * T), nbn = (int)ceil_div(c.N, 64 * T);
  ScopedLaunchTimer timer(p.slot, (double)c.M, (double)c.N, (double)c.K, c.stream);
  hipLaunchKernelGGL((gemm_nt_kernel<T, FAST, AMUL, BF3>), dim3((unsigned)((int64_t)nbm * nbn)), dim3(kBlk), lds, c.stream, c.A,
                     c.lda, c.B, c.ldb, c.bias, c.C, c.ldc, (int)c.M, (int)c.N, (int)c.K, c.act, c.act_param, c.out_scale, nbm, nbn,
                     p.a_vec, p.b_vec, c.c_vec, c.am);
  return check_launch("gemm_nt");
}

// V1: gemm_nt_narrow_v1_kernel (the bf16x6 mode, and every launch under RECMV_GEMM_NARROW=0); otherwise gemm_nt_narrow_kernel: same bits
template <bool FAST, bool AMUL, bool BF3, bool V1>
static int launch_nt_narrow(const NtCall& c, const NtPlan& p) {
  const int nbm = (int)ceil_div(c.M, 64), nbn = (int)ceil_div(c.N, 32);
  ScopedLaunchTimer timer(p.slot, (double)c.M, (double)c.N, (double)c.K, c.stream);
  if constexpr (V1 || BF3)
    hipLaunchKernelGGL((gemm_nt_narrow_v1_kernel<FAST, AMUL, BF3>), dim3((unsigned)((int64_t)nbm * nbn)), dim3(kBlk), kNarrowLds, c.stream,
                       c.A, c.lda, c.B, c.ldb, c.bias, c.C, c.ldc, (int)c.M, (int)c.N, (int)c.K, c.act, c.act_param, c.out_scale, nbm, nbn,
                       p.a_vec, p.b_vec, c.c_vec, c.am);
  else
    hipLaunchKernelGGL((gemm_nt_narrow_kernel<FAST, AMUL, BF3>), dim3((unsigned)((int64_t)nbm * nbn)), dim3(kBlk), kNarrowLds, c.stream,
                       c.A, c.lda, c.B, c.ldb, c.bias, c.C, c.ldc, (int)c.M, (int)c.N, (int)c.K, c.act, c.act_param, c.out_scale, nbm, nbn,
                       p.a_vec, p.b_vec, c.c_vec, c.am);
  return check_launch("gemm_nt(narrow)");
}

// MI x NI tiles of 64 x 64 per workgroup, K-tile 16; SCAL: staging loads that need only dword alignment
template <bool AMUL, int MI, int NI, bool SCAL>
static int launch_nt_occ(const NtCall& c, const NtPlan& p) {
  constexpr int lds_ops = 64 * (MI + NI) * (16 + 4) * 4, lds_c = 32 * MI * (64 * NI + 4) * 4;
  constexpr int lds = lds_ops > lds_c ? lds_ops : lds_c;
  const int nbm = (int)ceil_div(c.M, 64 * MI), nbn = (int)ceil_div(c.N, 64 * NI);
  ScopedLaunchTimer timer(p.slot, (double)c.M, (double)c.N, (double)c.K, c.stream);
  hipLaunchKernelGGL((gemm_nt_occ_kernel<AMUL, 16, true, MI, NI, SCAL>), dim3((unsigned)((int64_t)nbm * nbn)), dim3(kBlk), lds,
                     c.stream, c.A, c.lda, c.B, c.ldb, c.bias, c.C, c.ldc, (int)c.M, (int)c.N, (int)c.K, c.act, c.act_param,
                     c.out_scale, nbm, nbn, c.c_vec, c.am, p.a_vec, p.b_vec);
  return check_launch("gemm_nt(occ)");
}

template <int NN>
static int launch_nt_thin_n(const NtCall& c, const NtPlan& p) {
  ScopedLaunchTimer timer(p.slot, (double)c.M, (double)NN, (double)c.K, c.stream);
  const dim3 grid((unsigned)ceil_div(c.M, kThinRows));
  if (p.a_vec && c.K % 4 == 0)
    hipLaunchKernelGGL((gemm_nt_thin_n_kernel<NN, true>), grid, dim3(kThinRows), 0, c.stream, c.A, c.lda, c.B, c.ldb, c.bias, c.C,
                       c.ldc, (int)c.M, (int)c.K, c.act, c.act_param, c.out_scale, p.halves, c.am);
  else
    hipLaunchKernelGGL((gemm_nt_thin_n_kernel<NN, false>), grid, dim3(kThinRows), 0, c.stream, c.A, c.lda, c.B, c.ldb, c.bias, c.C,
                       c.ldc, (int)c.M, (int)c.K, c.act, c.act_param, c.out_scale, p.halves, c.am);
  return check_launch("gemm_nt(thin n)");
}

template <int KK, bool AMUL>
static int launch_nt_thin_k(const NtCall& c, const NtPlan& p) {
  ScopedLaunchTimer timer(p.slot, (double)c.M, (double)c.N, (double)KK, c.stream);
  int cw_log2 = 0;
  while (cw_log2 < 8 && (4ll << cw_log2) < c.N) ++cw_log2;      // threads across a row: the float4 strips of a row, at most 256
  hipLaunchKernelGGL((gemm_nt_thin_k_kernel<KK, AMUL>), dim3((unsigned)ceil_div(c.M, kThinKRows)), dim3(kBlk), 0, c.stream, c.A, c.lda,
                     c.B, c.ldb, c.bias, c.C, c.ldc, (int)c.M, (int)c.N, c.act, c.act_param, c.out_scale, cw_log2, c.c_vec, c.am);
  return check_launch("gemm_nt(thin k)");
}

// Weight matrices whose bf16 planes exist (recmv_b3_split), by the address the products get them under.
struct B3Entry {
  const char* planes;
  int64_t N, K, ldb, Kp;
};
static std::mutex g_b3_mu;
static std::unordered_map<const float*, B3Entry> g_b3;
static bool b3_lookup(const float* B, const NtCall& c, B3Entry* out) {
  std::lock_guard<std::mutex> lock(g_b3_mu);
  auto it = g_b3.find(B);
  if (it == g_b3.end() || it->second.K != c.K || it->second.ldb != c.ldb || it->second.N < c.N) return false;
  *out = it->second;
  return true;
}

template <int T, bool AMUL, bool PRE>
static int launch_nt_b3_as(const NtCall& c, const NtPlan& p, const B3Pre& pre) {
  constexpr int lds_ops = 6 * 64 * T * 64, lds_c = 64 * T * (64 * T + 4) * 4;
  constexpr int lds = lds_ops > lds_c ? lds_ops : lds_c;
  static bool attr_set = false;
  if (!attr_set) {
    RECMV_HIP_TRY(hipFuncSetAttribute((const void*)gemm_nt_b3_kernel<T, AMUL, PRE>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr_set = true;
  }
  const int nbm = (int)ceil_div(c.M, 64 * T), nbn = (int)ceil_div(c.N, 64 * T);
  ScopedLaunchTimer timer(p.slot, (double)c.M, (double)c.N, (double)c.K, c.stream);
  hipLaunchKernelGGL((gemm_nt_b3_kernel<T, AMUL, PRE>), dim3((unsigned)((int64_t)nbm * nbn)), dim3(kBlk), lds, c.stream, c.A, c.lda,
                     c.B, c.ldb, c.bias, c.C, c.ldc, (int)c.M, (int)c.N, (int)c.K, c.act, c.act_param, c.out_scale, nbm, nbn, c.c_vec,
                     c.am, pre);
  return check_launch("gemm_nt(b3)");
}

template <int T, bool AMUL>
static int launch_nt_b3(const NtCall& c, const NtPlan& p) {
  B3Entry e, e2;
  if (b3_lookup(c.B, c, &e) && (!c.am.B2 || (b3_lookup(c.am.B2, c, &e2) && e2.Kp == e.Kp))) {
    B3Pre pre = {e.planes, c.am.B2 ? e2.planes : nullptr, e.N * e.Kp * 2, c.am.B2 ? e2.N * e2.Kp * 2 : 0, (int)e.Kp};
    return launch_nt_b3_as<T, AMUL, true>(c, p, pre);
  }
  B3Pre none = {nullptr, nullptr, 0, 0, 0};
  return launch_nt_b3_as<T, AMUL, false>(c, p, none);
}

// the FAST / BF3 instantiation the plan names
template <int T, bool AMUL>
static int launch_nt_tile(const NtCall& c, const NtPlan& p) {
  if (p.fast) return p.bf3 ? launch_nt<T, true, AMUL, true>(c, p) : launch_nt<T, true, AMUL, false>(c, p);
  return p.bf3 ? launch_nt<T, false, AMUL, true>(c, p) : launch_nt<T, false, AMUL, false>(c, p);
}
template <bool AMUL>
static int launch_nt_narrow_tile(const NtCall& c, const NtPlan& p) {
  const char* e = getenv("RECMV_GEMM_NARROW");       // =0: the kernel before the half-tile schedule (A/B); read at every launch
  const bool v1 = e && e[0] == '0';
  if (p.bf3) return p.fast ? launch_nt_narrow<true, AMUL, true, true>(c, p) : launch_nt_narrow<false, AMUL, true, true>(c, p);
  if (p.fast) return v1 ? launch_nt_narrow<true, AMUL, false, true>(c, p) : launch_nt_narrow<true, AMUL, false, false>(c, p);
  return v1 ? launch_nt_narrow<false, AMUL, false, true>(c, p) : launch_nt_narrow<false, AMUL, false, false>(c, p);
}

// plan (gemm_route.h), log, launch
template <bool AMUL>
static int dispatch_nt(NtCall& c) {
  c.a_vec = aligned16(c.A) && c.lda % 4 == 0 && (!AMUL || (aligned16(c.am.Y) && c.am.ldy % 4 == 0));
  c.b_vec = aligned16(c.B) && c.ldb % 4 == 0 && (!c.am.B2 || aligned16(c.am.B2));
  c.c_vec = aligned16(c.C) && c.ldc % 4 == 0;
  const bool emul = !AMUL && c.am.Y, seg = c.am.B2 != nullptr;
  const NtPlan p = route::plan_nt({c.M, c.N, c.K, c.a_vec, c.b_vec, c.c_vec, AMUL, emul, seg, c.lda >= c.K}, gemm_switches());
  if (p.route[0]) log_shape(p.route, p.parent, {c.M, c.N, c.K, c.lda, c.ldb, c.A, c.B, AMUL, emul, seg});
  switch (p.kernel) {
    case NtKernel::ThinK:
      switch (c.K) {
        case 1: return launch_nt_thin_k<1, AMUL>(c, p);
        case 2: return launch_nt_thin_k<2, AMUL>(c, p);
        case 3: return launch_nt_thin_k<3, AMUL>(c, p);
        default: return launch_nt_thin_k<4, AMUL>(c, p);
      }
    case NtKernel::ThinN:
      switch (c.N) {
        case 1: return launch_nt_thin_n<1>(c, p);
        case 2: return launch_nt_thin_n<2>(c, p);
        case 3: return launch_nt_thin_n<3>(c, p);
        default: return launch_nt_thin_n<4>(c, p);
      }
    case NtKernel::B3: return launch_nt_b3<2, AMUL>(c, p);
    case NtKernel::Occ128: return launch_nt_occ<AMUL, 2, 2, false>(c, p);
    case NtKernel::Occ64x128: return launch_nt_occ<AMUL, 1, 2, false>(c, p);
    case NtKernel::Occ128Scal: return launch_nt_occ<AMUL, 2, 2, true>(c, p);
    case NtKernel::Occ64x128Scal: return launch_nt_occ<AMUL, 1, 2, true>(c, p);
    case NtKernel::Tile128: return launch_nt_tile<2, AMUL>(c, p);
    case NtKernel::Narrow: return launch_nt_narrow_tile<AMUL>(c, p);
    case NtKernel::Tile64: break;
  }
  return launch_nt_tile<1, AMUL>(c, p);
}

// Matrix mode of recmv_gemm_nt: 0 = f32-input MFMA (default; bit-for-bit an f32 fma chain), 1 = "bf16x6" (each f32
// operand split into three bf16 pieces in registers, six bf16 MFMA products per tile step, f32 accumulation: f32-level
// accuracy at up to 2.7x the f32 matrix rate).  Returns the previous mode.
extern "C" int recmv_set_gemm_mode(int mode) {
  const int prev = g_gemm_mode;
  if (mode == 0 || mode == 1) g_gemm_mode = mode;
  return prev;
}

extern "C" int recmv_get_gemm_mode(void) { return g_gemm_mode; }

// Mode 1 only — which kernel families compute in bf16x6 (the others stay on the exact-f32 kernels): bit 0 = 128 x 128 NT tiles, bit 1 =
// 64 x 64 and 64 x 32 NT tiles, bit 2 = TN (dW) tiles.  7 (default) = all.  A bisect / A-B switch (tools/erratum/loop_repro_inproc.py); returns
// the previous mask.
extern "C" int recmv_set_b3_families(int mask) {
  const int prev = g_b3_families;
  if (mask >= 0 && mask <= 7) g_b3_families = mask;
  return prev;
}

extern "C" int64_t recmv_b3_planes_bytes(int64_t N, int64_t K) {
  if (N <= 0 || K <= 0) return 0;
  return 3 * N * (ceil_div(K, (int64_t)BK) * BK) * 2;
}

extern "C" int recmv_b3_split(const float* B, int64_t ldb, int64_t N, int64_t K, void* planes, int64_t planes_bytes, void* stream) {
  RECMV_REQUIRE(B && planes, "b3_split: NULL pointer");
  RECMV_REQUIRE(N > 0 && K > 0 && K % 8 == 0 && ldb >= K && ldb % 4 == 0 && aligned16(B) && aligned16(planes),
                "b3_split: needs K %% 8 == 0 and 16-byte aligned rows (N=%lld K=%lld ldb=%lld)", (long long)N, (long long)K,
                (long long)ldb);
  RECMV_REQUIRE(K < (1ll << 30) && N < (1ll << 31), "b3_split: size overflow");
  const int64_t Kp = ceil_div(K, (int64_t)BK) * BK;
  RECMV_REQUIRE(planes_bytes >= 3 * N * Kp * 2, "b3_split: planes buffer %lld < %lld bytes", (long long)planes_bytes,
                (long long)(3 * N * Kp * 2));
  hipLaunchKernelGGL(b3_split_kernel, dim3(stream_grid(N * (Kp / 8), kBlk)), dim3(kBlk), 0, (hipStream_t)stream, B, ldb, N, (int)K,
                     (int)Kp, (char*)planes);
  {
    const int rc = check_launch("b3_split");
    if (rc) return rc;
  }
  std::lock_guard<std::mutex> lock(g_b3_mu);
  g_b3[B] = B3Entry{(const char*)planes, N, K, ldb, Kp};
  return RECMV_OK;
}

extern "C" int recmv_b3_forget(const float* B) {
  std::lock_guard<std::mutex> lock(g_b3_mu);
  g_b3.erase(B);
  return RECMV_OK;
}

// The checks the five NT entry points share, in their order, under the entry point's name.  *run: there is something to launch
// (an empty product passes with NULL operands).
static int check_nt_args(const char* name, const NtCall& c, bool pointers, bool leading_dims, bool* run) {
  *run = false;
  RECMV_REQUIRE(c.M >= 0 && c.N >= 0 && c.K >= 0, "%s: negative size", name);
  if (c.M == 0 || c.N == 0) return RECMV_OK;
  RECMV_REQUIRE(pointers, "%s: NULL pointer", name);
  RECMV_REQUIRE(leading_dims, "%s: leading dimension too small", name);
  RECMV_REQUIRE(c.M < (1ll << 31) - BM && c.N < (1ll << 31) - BN && c.K < (1ll << 31) - BK, "%s: size overflow", name);
  const int act = c.am.Y ? c.am.act : c.act;      // the caller's activation: the transform's where there is one, else the epilogue's
  RECMV_REQUIRE(act >= RECMV_ACT_NONE && act <= RECMV_ACT_TANH, "%s: unknown activation %d", name, act);
  *run = true;
  return RECMV_OK;
}

extern "C" int recmv_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias,
                             float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act,
                             float act_param, float out_scale, void* stream) {
  NtCall c = {A, lda, B, ldb, bias, C, ldc, M, N, K, act, act_param, out_scale, {nullptr, 0, RECMV_ACT_NONE, 0.f, 1.f, 1.f},
              (hipStream_t)stream};
  bool run;
  const int rc = check_nt_args("gemm_nt", c, A && B && C, lda >= K && ldb >= K && ldc >= N, &run);
  if (!run) return rc;
  return dispatch_nt<false>(c);
}

// C[M,N] = (G (.) act'(y_scale * Y) * g_scale) . B^T : the activation-gradient step fused into the product.
// G's row stride ldg may be 0 (one cotangent row for every point).
extern "C" int recmv_gemm_nt_actgrad(const float* G, int64_t ldg, const float* Y, int64_t ldy, const float* B,
                                     int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act,
                                     float act_param, float y_scale, float g_scale, void* stream) {
  NtCall c = {G, ldg, B, ldb, nullptr, C, ldc, M, N, K, RECMV_ACT_NONE, 0.f, 1.f, {Y, ldy, act, act_param, y_scale, g_scale},
              (hipStream_t)stream};
  bool run;
  const int rc = check_nt_args("gemm_nt_actgrad", c, G && Y && B && C, (ldg >= K || ldg == 0) && ldy >= K && ldb >= K && ldc >= N, &run);
  if (!run) return rc;
  return dispatch_nt<true>(c);
}

// C[M,N] = (A . B^T) (.) act'(y_scale * Y) * scale : the activation-gradient step of the NEXT backward layer fused into the
// epilogue of the product that creates its cotangent (Y [M,N], row stride ldy).
extern "C" int recmv_gemm_nt_mulgrad(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                                     int64_t M, int64_t N, int64_t K, const float* Y, int64_t ldy, int act,
                                     float act_param, float y_scale, float scale, void* stream) {
  NtCall c = {A, lda, B, ldb, nullptr, C, ldc, M, N, K, RECMV_ACT_NONE, 0.f, 1.f, {Y, ldy, act, act_param, y_scale, scale},
              (hipStream_t)stream};
  bool run;
  const int rc = check_nt_args("gemm_nt_mulgrad", c, A && B && C && Y, lda >= K && ldb >= K && ldc >= N && ldy >= N, &run);
  if (!run) return rc;
  return dispatch_nt<false>(c);
}

// The same products over a row block that holds the rows of TWO nets of one shape: rows [0, split_row) use B / bias, rows
// [split_row, M) use B2 / bias2 (split_row a multiple of 128, the largest tile height; B2 == NULL: the plain product).
extern "C" int recmv_gemm_nt_seg(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias,
                                 const float* B2, const float* bias2, int64_t split_row, float* C, int64_t ldc, int64_t M,
                                 int64_t N, int64_t K, int act, float act_param, float out_scale, void* stream) {
  NtCall c = {A, lda, B, ldb, bias, C, ldc, M, N, K, act, act_param, out_scale,
              {nullptr, 0, RECMV_ACT_NONE, 0.f, 1.f, 1.f, B2, bias2, (int)(split_row < M ? split_row : M)}, (hipStream_t)stream};
  bool run;
  const int rc = check_nt_args("gemm_nt_seg", c, A && B && C, lda >= K && ldb >= K && ldc >= N, &run);
  if (!run) return rc;
  RECMV_REQUIRE(!B2 || (split_row >= 0 && split_row % BM == 0), "gemm_nt_seg: split_row must be a multiple of %d", BM);
  RECMV_REQUIRE(!B2 || !bias == !bias2, "gemm_nt_seg: both nets with or both without a bias");
  return dispatch_nt<false>(c);
}

extern "C" int recmv_gemm_nt_mulgrad_seg(const float* A, int64_t lda, const float* B, const float* B2, int64_t split_row,
                                         int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const float* Y,
                                         int64_t ldy, int act, float act_param, float y_scale, float scale, void* stream) {
  NtCall c = {A, lda, B, ldb, nullptr, C, ldc, M, N, K, RECMV_ACT_NONE, 0.f, 1.f,
              {Y, ldy, act, act_param, y_scale, scale, B2, nullptr, (int)(split_row < M ? split_row : M)}, (hipStream_t)stream};
  bool run;
  const int rc = check_nt_args("gemm_nt_mulgrad_seg", c, A && B && C && Y, lda >= K && ldb >= K && ldc >= N && ldy >= N, &run);
  if (!run) return rc;
  RECMV_REQUIRE(!B2 || (split_row >= 0 && split_row % BM == 0), "gemm_nt_mulgrad_seg: split_row must be a multiple of %d", BM);
  return dispatch_nt<false>(c);
}

// Per-launch HIP-event timing of the MFMA kernels.  recmv_profile_begin() starts recording (events on the launch
// stream around every gemm_nt / gemm_tn launch); recmv_profile_end() waits for the recorded events and returns, per
// slot v (route::Slot of gemm_route.h — 0..7: gemm_nt_kernel<T, FAST, AMUL> with v = (T-1) + 2*FAST + 4*AMUL; 8: gemm_tn_occ_kernel / gemm_tn_kernel
// (the product alone, its split-K reduction pass is not bracketed); 9 / 10: gemm_nt_occ_kernel<false, ...> with 128x128 / 64x128 tiles, 11: gemm_nt_occ_kernel<true, ...>; 12 / 13: gemm_nt_narrow_kernel<true, false, .> / its other instantiations), out[5v] = timed launches, out[5v+1] = their summed duration in seconds, out[5v+2] = their
// summed algorithmic FLOP (2 M N K), out[5v+3] / out[5v+4] = launches / FLOP of the launches below `min_flops`, which
// are only counted (bracketing tens of thousands of ~20 us launches with events would perturb the run being timed).
// A caller with room for fewer than 14 slots (at least 9) gets the later slots folded into those of the kernels they replaced (route::fold_slot).
extern "C" int recmv_profile_begin(double min_flops) {
  g_prof.recs.clear();
  for (auto& u : g_prof.untimed) u[0] = u[1] = 0.0;
  g_prof.min_flops = min_flops;
  g_prof.on = true;
  return RECMV_OK;
}

// Algorithmic bytes (4 (M K + N K + M N): both operands read once, the result written once) of the launches the last
// recmv_profile_end bracketed, per variant with the same slot folding as its `out`.  (ABI v7)
extern "C" int recmv_profile_bytes(double* out, int n_variants) {
  RECMV_REQUIRE(out && n_variants >= 9, "profile_bytes: need room for 9 variants");
  for (int i = 0; i < n_variants; ++i) out[i] = 0.0;
  for (int v = 0; v < route::kNumSlots; ++v) out[route::fold_slot(v, n_variants)] += g_prof.timed_bytes[v];
  return RECMV_OK;
}

// The launches of >= 4 GFLOP among those the last recmv_profile_end bracketed (a pass that brackets EVERY launch still yields the
// large products' own rate): out[3v] = launches, out[3v+1] = seconds, out[3v+2] = FLOP, same slots as recmv_profile_end.  (ABI v7)
extern "C" int recmv_profile_large(double* out, int n_variants) {
  RECMV_REQUIRE(out && n_variants >= 9, "profile_large: need room for 9 variants");
  for (int i = 0; i < 3 * n_variants; ++i) out[i] = 0.0;
  for (int v = 0; v < route::kNumSlots; ++v)
    for (int q = 0; q < 3; ++q) out[3 * route::fold_slot(v, n_variants) + q] += g_prof.large[v][q];
  return RECMV_OK;
}

extern "C" int recmv_profile_busy(double* out2) {
  RECMV_REQUIRE(out2, "profile_busy: NULL");
  out2[0] = g_prof.busy_union_s;
  out2[1] = g_prof.busy_span_s;
  return RECMV_OK;
}

extern "C" int recmv_profile_end(double* out, int n_variants) {
  g_prof.on = false;
  RECMV_REQUIRE(out && n_variants >= 9, "profile_end: need room for 9 variants");
  for (int i = 0; i < 5 * n_variants; ++i) out[i] = 0.0;
  auto slot = [&](int v) { return route::fold_slot(v, n_variants); };
  for (int v = 0; v < route::kNumSlots; ++v) {
    out[5 * slot(v) + 3] += g_prof.untimed[v][0];
    out[5 * slot(v) + 4] += g_prof.untimed[v][1];
  }
  // every bracket also as an interval on one time axis (the first recorded event is the origin; events of different streams of a
  // device share a clock): the union of the intervals is the time in which at least one bracketed MFMA kernel was running
  std::vector<std::pair<double, double>> iv;
  iv.reserve(g_prof.recs.size());
  hipEvent_t origin = g_prof.recs.empty() ? nullptr : g_prof.recs.front().a;
  for (auto& b : g_prof.timed_bytes) b = 0.0;
  for (auto& l : g_prof.large) l[0] = l[1] = l[2] = 0.0;
  for (auto& r : g_prof.recs) {
    g_prof.timed_bytes[r.variant] += r.bytes;
    RECMV_HIP_TRY(hipEventSynchronize(r.b));
    float ms = 0.f;
    RECMV_HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
    if (r.flops >= 4.0e9) {
      g_prof.large[r.variant][0] += 1.0;
      g_prof.large[r.variant][1] += (double)ms * 1e-3;
      g_prof.large[r.variant][2] += r.flops;
    }
    out[5 * slot(r.variant) + 0] += 1.0;
    out[5 * slot(r.variant) + 1] += (double)ms * 1e-3;
    out[5 * slot(r.variant) + 2] += r.flops;
    float t0 = 0.f;
    if (r.a != origin && hipEventElapsedTime(&t0, origin, r.a) != hipSuccess) t0 = -1.f;
    if (t0 >= 0.f) iv.emplace_back((double)t0 * 1e-3, (double)(t0 + ms) * 1e-3);
  }
  for (auto& r : g_prof.recs) {
    g_prof.pool.push_back(r.a);
    g_prof.pool.push_back(r.b);
  }
  g_prof.recs.clear();
  g_prof.busy_union_s = g_prof.busy_span_s = 0.0;
  if (!iv.empty()) {
    std::sort(iv.begin(), iv.end());
    double lo = iv[0].first, hi = iv[0].second, first = iv[0].first, last = iv[0].second;
    for (size_t i = 1; i < iv.size(); ++i) {
      if (iv[i].first > hi) {
        g_prof.busy_union_s += hi - lo;
        lo = iv[i].first;
        hi = iv[i].second;
      } else if (iv[i].second > hi) {
        hi = iv[i].second;
      }
      if (iv[i].second > last) last = iv[i].second;
    }
    g_prof.busy_union_s += hi - lo;
    g_prof.busy_span_s = last - first;
  }
  return RECMV_OK;
}
