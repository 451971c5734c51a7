// host stand-ins for csrc/mesh_topology.hip on top of tools/mesh_grid_host_check/common.h (copied beside this file as common.h):
// the integer minimum and the relaxed loads and stores of the compression, one thread at a time
#pragma once
#include "common.h"
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __hip_atomic_store(p, v, order, scope) (*(p) = (v))
static inline int atomicMin(int32_t* p, int v) { int o = *p; if (v < o) *p = v; return o; }
