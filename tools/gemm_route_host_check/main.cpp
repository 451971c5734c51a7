// The route planner of csrc/gemm_route.h on the host: reads one case per line from stdin, prints the plan as one tab-separated line.
//
//   nt NAME M N K a_vec b_vec c_vec amul emul seg lda_ge_k  mode families occ skinny
//     -> NAME kernel slot route parent halves kernel_with_skinny_off        (route / parent: as RECMV_GEMM_SHAPES=1 would print them,
//   tn NAME M N K lda ldb a_vec b_vec  mode families occ skinny                empty below the log's floor or for a launch without a name)
//     -> NAME kernel slot route parent swap splits kchunk
//
// tests/test_gemm_route_cpu.py builds this with the address and undefined-behaviour sanitizers and compares the plans with the census of
// tests/golden/gemm_routes.json.
#include <stdio.h>
#include <string.h>

#include "gemm_route.h"

using namespace recmv::route;

static const char* name_of(NtKernel k) {
  switch (k) {
    case NtKernel::Tile128: return "Tile128";
    case NtKernel::Tile64: return "Tile64";
    case NtKernel::Narrow: return "Narrow";
    case NtKernel::Occ128: return "Occ128";
    case NtKernel::Occ64x128: return "Occ64x128";
    case NtKernel::Occ128Scal: return "Occ128Scal";
    case NtKernel::Occ64x128Scal: return "Occ64x128Scal";
    case NtKernel::B3: return "B3";
    case NtKernel::ThinK: return "ThinK";
    case NtKernel::ThinN: return "ThinN";
  }
  return "?";
}

static const char* name_of(TnKernel k) {
  switch (k) {
    case TnKernel::Thin: return "Thin";
    case TnKernel::Occ: return "Occ";
    case TnKernel::OccScal: return "OccScal";
    case TnKernel::Tile: return "Tile";
    case TnKernel::TileB3: return "TileB3";
  }
  return "?";
}

int main() {
  char line[512], kind[8], name[128];
  int n_lines = 0;
  while (fgets(line, sizeof line, stdin)) {
    long long M, N, K, lda, ldb;
    int f[7], mode, fam, occ, skinny, used = 0;
    if (sscanf(line, "%7s %127s %lld %lld %lld%n", kind, name, &M, &N, &K, &used) != 5) {
      fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    const char* rest = line + used;
    if (!strcmp(kind, "nt")) {
      if (sscanf(rest, "%d %d %d %d %d %d %d %d %d %d %d", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &f[6], &mode, &fam, &occ, &skinny) != 11) return 2;
      const NtShape s = {M, N, K, f[0] != 0, f[1] != 0, f[2] != 0, f[3] != 0, f[4] != 0, f[5] != 0, f[6] != 0};
      const GemmSwitches sw = {mode, fam, occ != 0, skinny != 0};
      GemmSwitches off = sw;
      off.skinny = false;
      const NtPlan p = plan_nt(s, sw);
      const bool log = logged(M, N, K);
      printf("%s\t%s\t%d\t%s\t%s\t%d\t%s\n", name, name_of(p.kernel), p.slot, log ? p.route : "", log && p.route[0] ? p.parent : "",
             (int)p.halves, name_of(plan_nt(s, off).kernel));
    } else if (!strcmp(kind, "tn")) {
      if (sscanf(rest, "%lld %lld %d %d %d %d %d %d", &lda, &ldb, &f[0], &f[1], &mode, &fam, &occ, &skinny) != 8) return 2;
      const TnShape s = {M, N, K, lda, ldb, f[0] != 0, f[1] != 0};
      const TnPlan p = plan_tn(s, {mode, fam, occ != 0, skinny != 0});
      const bool log = logged(M, N, K);
      printf("%s\t%s\t%d\t%s\t%s\t%d\t%d\t%lld\n", name, name_of(p.kernel), (int)kSlotTn, log ? p.route : "", log && p.route[0] ? p.parent : "",
             (int)p.swap, p.splits, (long long)p.kchunk);
    } else {
      fprintf(stderr, "bad kind: %s\n", kind);
      return 2;
    }
    ++n_lines;
  }
  fprintf(stderr, "%d plans\n", n_lines);
  return 0;
}
