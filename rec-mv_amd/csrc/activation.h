// Every form in which the kernels of this library evaluate the MLP activations (RECMV_ACT_*) and their derivatives — ONE place,
// because the form a kernel uses decides which error bound its float64 test may claim.  softplus(beta) has torch's semantics
// (beta z > 20 ? z : log1p(exp(beta z)) / beta); p = beta, inv_p = 1 / beta.
//
//   form                        expression (softplus)                              used by                                     judged by
//   dact_libm / d2act_libm      -expm1(-p y);  p exp(-p y), libm                  elementwise, mlp_chain (act_grad_2d), linear_bwd  layer_backward_reference.py; mlp_reference.py act_grad_y('expm1')
//   dact_hw                     t = p y: series below 1/64, else 1 - exp2 unit     gemm_f32 (operand / output transform)       mlp_reference.py act_grad_y('hw'); layer_backward_reference.py (fused route)
//   softplus_grad, act_grad     the same values, both arms evaluated and selected  mlp_rows                                    mlp_reference.py act_grad_y('hw'), family rows
//   apply_act<ACT>              exp2 unit, series below 2^-6, else __logf(1 + t)   gemm_f32 epilogues                          mlp_reference.py _act_forward, family chain
//   softplus_fwd, act_fwd<ACT>  the same with the bare __log2f(1 + t) ln2, selected  mlp_rows                                  mlp_reference.py _act_forward, family rows
//   act_jet                     phi, phi', phi'' through expf / log1pf / tanhf     mlp_jet                                     mlp_reference.py act_jet
// tests/test_gpu_mlp_passes.py (test_activation_sweep: every switch point of each family's forms) and tests/test_gpu_layer_backward.py run them.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/recmv_hip.h"
// RECMV_LIBM_SOFTPLUS (an experiment build of tools/trajectory_seeds.py, never the product's): the hardware forms through the
// correctly-rounded-to-an-ulp library functions instead of the hardware exp2 / log2 units.
#ifdef RECMV_LIBM_SOFTPLUS
#define RECMV_EXPF(x) expf(x)
#define RECMV_LOG1PF(t) log1pf(t)
#else
#define RECMV_EXPF(x) __expf(x)
#define RECMV_LOG1PF(t) __logf(1.f + (t))
#endif

namespace recmv {
namespace {

// ---- act'(z) expressed through y = act(z), library functions: the memory-bound element-wise kernels
__device__ __forceinline__ float dact_libm(float y, int act, float p) {
  switch (act) {
    case RECMV_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case RECMV_ACT_SOFTPLUS: return -expm1f(-p * y);          // sigmoid(beta z) = 1 - exp(-beta y)
    case RECMV_ACT_TANH: return 1.f - y * y;
    default: return 1.f;
  }
}
// d/dy of the above (the double-backward term of the same step)
__device__ __forceinline__ float d2act_libm(float y, int act, float p) {
  switch (act) {
    case RECMV_ACT_SOFTPLUS: return p * expf(-p * y);
    case RECMV_ACT_TANH: return -2.f * y;
    default: return 0.f;
  }
}

// ---- the same derivative on the operand-staging and epilogue paths of the MFMA kernels: the hardware exp2 unit; below t = 1/64 the
// alternating series keeps the relative accuracy expm1 would give.  (Not the libm form: results differ from dact_libm by rounding.)
__device__ __forceinline__ float dact_hw(float y, int act, float p) {
  switch (act) {
    case RECMV_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case RECMV_ACT_SOFTPLUS: {
      const float t = p * y;
      const float series = t * (1.f - t * (0.5f - t * (0.16666667f - 0.041666668f * t)));
      return t < 0.015625f ? series : 1.f - RECMV_EXPF(-t);
    }
    case RECMV_ACT_TANH: return 1.f - y * y;
    default: return 1.f;
  }
}

// ---- the row-tile kernels' derivative: dact_hw's values as straight-line code, both arms of the small-t split evaluated and selected,
// so that the epilogue of a tile is one basic block.  Beside dact_hw because the instructions differ (a select against a branch: either
// function written through the other changes the kernels of gemm_f32.hip or mlp_rows.hip).
__device__ __forceinline__ float softplus_grad(float y, float p) {
  const float t = p * y;
  const float series = t * (1.f - t * (0.5f - t * (0.16666667f - 0.041666668f * t)));
  const float e = 1.f - RECMV_EXPF(-t);
  return t < 0.015625f ? series : e;
}
// ACT: a compile-time activation (RECMV_ACT_SOFTPLUS) or -1 = look at the run-time value.
template <int ACT>
__device__ __forceinline__ float act_grad(float y, int act, float p) {
  if (ACT == RECMV_ACT_SOFTPLUS) return softplus_grad(y, p);
  switch (act) {
    case RECMV_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case RECMV_ACT_SOFTPLUS: return softplus_grad(y, p);
    case RECMV_ACT_TANH: return 1.f - y * y;
    default: return 1.f;
  }
}

// ---- forward, the fused epilogue of the layer products.  ACT is a compile-time constant inside the epilogue loops.
//   softplus: (max(zb,0) + log1p(exp(-|zb|))) / beta with the hardware exp2/log2 units: exp(-|zb|) = t in (0,1]; log1p(t) by its alternating
//   series below 2^-6 (keeps the relative accuracy of tiny outputs, which the backward recovers sigmoid(zb) = 1 - exp(-beta*y) from) and
//   __logf(1+t) above.  |error| < 2e-7/beta.
template <int ACT>
__device__ __forceinline__ float apply_act(float z, float p, float inv_p) {
  if (ACT == RECMV_ACT_RELU) return z > 0.f ? z : 0.f;
  if (ACT == RECMV_ACT_SOFTPLUS) {
    const float zb = z * p;
    const float t = RECMV_EXPF(-fabsf(zb));
    const float series = t * (1.f - t * (0.5f - t * (0.33333334f - 0.25f * t)));
    const float l = t < 0.015625f ? series : RECMV_LOG1PF(t);
    const float y = (fmaxf(zb, 0.f) + l) * inv_p;
    return zb > 20.f ? z : y;
  }
  if (ACT == RECMV_ACT_TANH) return tanhf(z);
  return z;
}

// ---- forward, the row-tile kernels: apply_act's formula as straight-line code (both arms selected), and the logarithm as the bare
// v_log_f32 — 1 + t lies in [1, 2], which needs none of __logf's range fix-ups.  Beside apply_act because of those two differences;
// the values agree to rounding, not bitwise.
__device__ __forceinline__ float softplus_fwd(float z, float p, float inv_p) {
  const float zb = z * p;
  const float t = RECMV_EXPF(-fabsf(zb));
  const float series = t * (1.f - t * (0.5f - t * (0.33333334f - 0.25f * t)));
#ifdef RECMV_LIBM_SOFTPLUS
  const float lg = log1pf(t);
#else
  const float lg = __log2f(1.f + t) * 0.69314718f;
#endif
  const float l = t < 0.015625f ? series : lg;
  const float y = (fmaxf(zb, 0.f) + l) * inv_p;
  return zb > 20.f ? z : y;
}
template <int ACT>
__device__ __forceinline__ float act_fwd(float z, int act, float p, float inv_p) {
  if (ACT == RECMV_ACT_SOFTPLUS) return softplus_fwd(z, p, inv_p);
  if (act == RECMV_ACT_RELU) return z > 0.f ? z : 0.f;
  if (act == RECMV_ACT_SOFTPLUS) return softplus_fwd(z, p, inv_p);
  if (act == RECMV_ACT_TANH) return tanhf(z);
  return z;
}

// ---- the jet: phi, phi', phi'' at z through the library functions (an element-wise kernel between the products)
struct ActD { float f, d1, d2; };
__device__ __forceinline__ ActD act_jet(float z, int act, float p) {
  ActD r = {z, 1.f, 0.f};                                  // no activation; softplus beyond beta z = 20
  switch (act) {
    case RECMV_ACT_RELU:
      r.f = z > 0.f ? z : 0.f;
      r.d1 = z > 0.f ? 1.f : 0.f;
      break;
    case RECMV_ACT_SOFTPLUS: {
      const float zb = z * p;
      if (!(zb > 20.f)) {
        const float e = expf(-fabsf(zb));                  // in (0,1]
        const float sig = zb >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        r.f = (fmaxf(zb, 0.f) + log1pf(e)) / p;
        r.d1 = sig;
        r.d2 = p * sig * (1.f - sig);
      }
      break;
    }
    case RECMV_ACT_TANH: {
      const float t = tanhf(z);
      r.f = t;
      r.d1 = 1.f - t * t;
      r.d2 = -2.f * t * r.d1;
      break;
    }
  }
  return r;
}

}  // namespace
}  // namespace recmv
