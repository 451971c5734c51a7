// The recmv_mlp descriptor's validation and the small host-side parts that mlp_chain.hip, mlp_rows.hip and mlp_jet.hip share (the workspace
// carving also serves linear_bwd.hip and marching_cubes.hip).  Pure host code over standard headers and the C ABI header (no HIP), like gemm_route.h.
#pragma once
#include <stdint.h>
#include "../../include/recmv_hip.h"

namespace recmv {

void set_error(const char* fmt, ...);      // api_common.hip

// a failing call returns its code to the caller's caller
#define RECMV_TRY(expr)                \
  do {                                 \
    int rc__ = (expr);                 \
    if (rc__ != RECMV_OK) return rc__; \
  } while (0)

constexpr float kInvSqrt2 = 0.70710678118654752440f;    // the skip concatenation [h | gamma] / sqrt2 and its reverse
constexpr float kSqrt2 = 1.41421356237309504880f;

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// Consecutive 256-byte aligned ranges of a workspace: take(bytes) is the offset of the next one, `o` the bytes handed out so far.
struct Carve {
  int64_t o = 0;
  int64_t take(int64_t bytes) { const int64_t r = o; o += align_up(bytes, 256); return r; }
};

inline int mlp_d_pe(const recmv_mlp* m) { return 3 + 6 * m->multires; }      // width of gamma(x)

// rows >= split_row belong to a second weight set (recmv_mlp_forward / _vjp_input only)
inline bool mlp_has_second(const recmv_mlp* m) { return m->split_row > 0 && m->W2[0]; }

// THE validation of a descriptor, for every entry point that takes one; `who` names the entry point in the message.  What is specific
// to a family (the row-tile width limits, one net only for the jet, n_out, transposed weights, the workspace size) stays with it.
inline int mlp_validate(const recmv_mlp* m, const char* who) {
#define MLP_REQUIRE(cond, ...) \
  do { if (!(cond)) { set_error(__VA_ARGS__); return RECMV_ERR_ARG; } } while (0)
  MLP_REQUIRE(m, "%s: NULL descriptor", who);
  MLP_REQUIRE(m->n_layers >= 1 && m->n_layers <= RECMV_MLP_MAX_LAYERS, "%s: bad layer count %d", who, m->n_layers);
  MLP_REQUIRE(m->multires >= 0 && m->multires <= 16 && m->cond_dim >= 0, "%s: bad encoding", who);
  MLP_REQUIRE(m->dims[0] == mlp_d_pe(m) + m->cond_dim, "%s: dims[0] != 3+6L+cond_dim", who);
  for (int l = 0; l < m->n_layers; ++l) {
    MLP_REQUIRE(m->W[l] && m->rows[l] > 0 && m->dims[l] > 0, "%s: layer %d incomplete", who, l);
    const int expect = (l + 1 == m->skip_layer) ? m->dims[l + 1] - mlp_d_pe(m) : m->dims[l + 1];
    MLP_REQUIRE(m->rows[l] == expect, "%s: layer %d has %d rows, expected %d", who, l, m->rows[l], expect);
  }
  MLP_REQUIRE(m->skip_layer < m->n_layers, "%s: bad skip layer", who);
  if (mlp_has_second(m)) {
    MLP_REQUIRE(m->split_row % 128 == 0, "%s: split_row %lld is not a multiple of 128", who, (long long)m->split_row);
    for (int l = 0; l < m->n_layers; ++l)
      MLP_REQUIRE(m->W2[l] && (!m->bias[l] == !m->bias2[l]), "%s: the second net's layer %d is incomplete", who, l);
  }
#undef MLP_REQUIRE
  return RECMV_OK;
}

}  // namespace recmv
