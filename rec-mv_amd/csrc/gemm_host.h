// Host-side pieces that gemm_f32.hip defines and gemm_tn.hip uses as well: the per-launch timer of the profiler, the switches
// of the route planner (gemm_route.h) and the RECMV_GEMM_SHAPES log.
#pragma once
#include "common.h"
#include "gemm_route.h"

namespace recmv {

static_assert(route::kCUs == kNumCU, "gemm_route.h plans for the CU count of common.h");

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Brackets one kernel launch with two events on its stream while recmv_profile_begin / _end record (gemm_f32.hip).
struct LaunchRec {
  hipEvent_t a, b;
  int variant;
  double flops, bytes;
};
struct ScopedLaunchTimer {
  LaunchRec r;
  hipStream_t s;
  bool active;
  ScopedLaunchTimer(int slot, double M, double N, double K, hipStream_t stream);
  ~ScopedLaunchTimer();
};

// g_gemm_mode, g_b3_families, RECMV_GEMM_OCC (read once per process) and RECMV_GEMM_SKINNY (read at every launch, so one process
// can time both: the tool of profiles/r07_fallback_shapes_ab.txt)
route::GemmSwitches gemm_switches();

// RECMV_GEMM_SHAPES=1: every distinct (route, route before the skinny / SCAL kernels, shape, leading dimensions, alignment) of a product
// of more than 1e8 multiply-adds that has a route name (gemm_route.h) is printed once to stderr — how the table of
// profiles/r07_fallback_shapes.txt was taken.
struct LoggedShape {
  int64_t M, N, K, lda, ldb;
  const void* A;
  const void* B;
  bool amul, emul, seg;
};
void log_shape(const char* route, const char* parent, const LoggedShape& s);

}  // namespace recmv
