// Host-side pieces that mesh_grid.hip, mesh_intersect.hip and segment_mesh.hip share: the check of a recmv_mesh_grid
// descriptor and the choice of a query's launch shape.  Include it after grid_query.h, behind the file's
// `using namespace recmv;` (the host checks of tools/ cut the kernels off in front of that line).
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int64_t kMaxCells = 1ll << 26;

// what an entry point reads of the descriptor besides the geometry and n_entries
enum GridNeeds { kGridGeometry = 0, kGridTables = 1, kGridTris = 2 };

// the descriptor, checked before any HIP call (0: fine), and the view of it the kernels take
int grid_view_args(const char* what, const recmv_mesh_grid* d, int needs, GridView& v) {
  RECMV_REQUIRE(d, "%s: NULL grid descriptor", what);
  RECMV_REQUIRE(d->nx >= 1 && d->ny >= 1 && d->nz >= 1, "%s: dims=(%lld,%lld,%lld) must be at least 1", what,
                (long long)d->nx, (long long)d->ny, (long long)d->nz);
  const float h = d->cell_size;
  RECMV_REQUIRE(h > 0.f && h < __builtin_inff(), "%s: cell size %g must be positive and finite", what, (double)h);
  RECMV_REQUIRE(d->nx <= kMaxCells && d->ny <= kMaxCells && d->nz <= kMaxCells && d->nx * d->ny * d->nz <= kMaxCells,
                "%s: at most 2^26 cells", what);
  RECMV_REQUIRE(d->n_entries >= 0 && d->n_entries < (1ll << 31), "%s: entries=%lld must be in [0, 2^31)", what,
                (long long)d->n_entries);
  RECMV_REQUIRE(!(needs & kGridTables) || (d->offsets && (d->n_entries == 0 || d->entries)), "%s: NULL pointer of the grid",
                what);
  RECMV_REQUIRE(!(needs & kGridTris) || (d->tris && ((uintptr_t)d->tris & 15) == 0),
                "%s: the tris of the grid must be given and 16-byte aligned", what);
  v = GridView{Grid{d->origin[0], d->origin[1], d->origin[2], h, 1.f / h, (int)d->nx, (int)d->ny, (int)d->nz}, d->offsets,
               d->entries, d->n_entries};
  return RECMV_OK;
}

int lanes_ok(const char* what, int32_t lanes) {
  RECMV_REQUIRE(lanes == 1 || lanes == 8 || lanes == 64, "%s: lanes=%d must be 1, 8 or 64", what, (int)lanes);
  return RECMV_OK;
}

// launch(std::integral_constant<int, G>) for the G = lanes that lanes_ok accepted: the kernel's template argument
template <class Launch>
void with_lanes(int32_t lanes, Launch launch) {
  if (lanes == 1) launch(std::integral_constant<int, 1>{});
  else if (lanes == 8) launch(std::integral_constant<int, 8>{});
  else launch(std::integral_constant<int, 64>{});
}

}  // namespace
