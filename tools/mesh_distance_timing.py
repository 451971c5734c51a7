"""Time of the exact closest-point query through the uniform grid (recmv.metrics.MeshGrid: build and query) against the brute
force recmv_closest_point on the same inputs, at three sizes: DESIGN.md's existing row (40 962 points onto 81 920 faces), a mid
size (1e5 surface samples onto a level-7 icosphere, 327 680 faces) and an evaluation-sized one (2e5 samples onto a level-8
icosphere, 1 310 720 faces).  The queries are surface samples of the mesh moved off it by up to 1 % of the radius, what a
prediction close to its ground truth gives.

Every launch shape of the query (1, 8 or 64 lanes per query; queries sorted by cell or not; the sort is inside the timed
call) is timed; grid and brute force alternate inside one process after a warm-up of each; every sample is a host clock
around work that ends in a device synchronise.  The results of every shape are compared bit for bit with the brute force's.
The crossover is the product P * F at which build + best query equals the brute force, interpolated between the measured
sizes on a log-log line (when the grid wins at every size: the smallest size measured, nothing is extrapolated below it).

    python tools/mesh_distance_timing.py [--reps 9] [--brute-reps 3] [--out profiles/mesh_distance_timing.json]
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(REPO / "tests"))

SHAPES = ((1, False), (1, True), (8, False), (8, True), (64, False), (64, True))


def _samples(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def _stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def _bits_equal(a, b):
    import torch
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--brute-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from recmv import metrics, nricp
    from recmv.iso_remesh import closest_point
    from test_nricp_cpu import icosphere
    assert torch.cuda.is_available(), "mesh_distance_timing.py measures on the GPU"
    dev = "cuda:0"
    v, f = icosphere(6)
    v, f = v.to(dev), f.to(dev)
    meshes = {6: (v, f)}
    for level in (7, 8):
        v, f = nricp.edge_subdivide(v, f)
        v = v / v.norm(dim=1, keepdim=True)
        meshes[level] = (v.contiguous(), f.contiguous())
    gen = torch.Generator(device=dev).manual_seed(0)
    cases = []
    for name, level, count in (("design_row", 6, 40962), ("mid", 7, 100000), ("evaluation", 8, 200000)):
        v, f = meshes[level]
        v = (0.5 * v).contiguous()
        p, _ = metrics.sample_surface(v, f, count, gen)
        p = (p * (1 + 0.01 * (2 * torch.rand(count, 1, device=dev, generator=gen) - 1))).contiguous()
        P, F = p.shape[0], f.shape[0]
        grid = metrics.MeshGrid(v, f)
        brute = closest_point(p, v, f)
        same = {}
        for lanes, sort in SHAPES:                                  # same results first, and the warm-up of every shape
            same["lanes%d_%s" % (lanes, "sorted" if sort else "unsorted")] = _bits_equal(
                grid.closest_point(p, lanes=lanes, sort=sort), brute)
        t_build, t_brute = [], []
        t_query = {k: [] for k in same}
        rounds = max(1, args.brute_reps)
        per = max(1, args.reps // rounds)
        for _ in range(rounds):                                      # alternate the paths
            t_build += _samples(lambda: metrics.MeshGrid(v, f), per)
            for lanes, sort in SHAPES:
                key = "lanes%d_%s" % (lanes, "sorted" if sort else "unsorted")
                t_query[key] += _samples(lambda: grid.closest_point(p, lanes=lanes, sort=sort), per)
            t_brute += _samples(lambda: closest_point(p, v, f), 1)
        med = statistics.median
        best = min(t_query, key=lambda k: med(t_query[k]))
        total = med(t_build) + med(t_query[best])
        cases.append({"case": name, "points": P, "faces": F, "point_triangle_tests": P * F,
                      "grid_dims": list(grid.dims), "grid_cell_size": grid.cell_size, "grid_entries": grid.n_entries,
                      "entries_per_face": grid.n_entries / F,
                      "grid_build_s": _stats(t_build), "grid_query_s": {k: _stats(x) for k, x in t_query.items()},
                      "best_query_shape": best, "grid_build_plus_best_query_s": total,
                      "brute_force_s": _stats(t_brute), "brute_force_tests_per_s": P * F / med(t_brute),
                      "brute_over_grid": med(t_brute) / total, "identical_bits_grid_vs_brute": same})
        print(json.dumps(cases[-1]))
    # the crossover on a log-log line between the measured sizes
    x = [math.log(c["point_triangle_tests"]) for c in cases]
    y = [math.log(c["brute_over_grid"]) for c in cases]
    if all(v >= 0 for v in y):
        cross, how = cases[0]["point_triangle_tests"], "the grid wins at every size measured: the smallest one"
    elif y[-1] < 0:
        cross, how = None, "the grid does not win at the largest size measured"
    else:
        k = max(i for i in range(len(y) - 1) if y[i] < 0)
        cross = math.exp(x[k] + (x[k + 1] - x[k]) * (0 - y[k]) / (y[k + 1] - y[k]))
        how = "interpolated between %s and %s" % (cases[k]["case"], cases[k + 1]["case"])
    res = {"cases": cases, "crossover_point_triangle_tests": cross, "crossover_how": how,
           "all_identical_bits": all(all(c["identical_bits_grid_vs_brute"].values()) for c in cases),
           "faces_per_cell_target": metrics.FACES_PER_CELL}
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    assert res["all_identical_bits"], "the grid query must return the brute force's bits"
    return res


if __name__ == "__main__":
    main()
