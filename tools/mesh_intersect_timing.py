"""Time of the crossing-faces query through the uniform grid (recmv.metrics.MeshGrid: build + count + fill) against the brute
force recmv_mesh_intersect_brute (count + fill) on two interpenetrating spheres: an icosphere of level 3 .. 7 (1 280 ..
327 680 faces) and a copy of it scaled 0.9 and shifted by 0.3 radius.  The brute force is timed up to --brute-max-faces.

Every launch shape of the grid query (1, 8 or 64 lanes per face) is timed; grid and brute force alternate inside one process
after a warm-up of each; every sample is a host clock around work that ends in a device synchronise (the query's own
read-back of the pair count is inside it).  The pairs of every shape are compared with the brute force's as integers.
`crossover_pairs` is the number of face pairs FA * FB at which build + best query equals the brute force, interpolated
between the measured sizes on a log-log line (when one side wins at every size: no crossover is extrapolated, the field
says which side); `best_lanes` is the shape with the lowest summed query time over the sizes.

    python tools/mesh_intersect_timing.py [--reps 7] [--brute-reps 3] [--out profiles/mesh_intersect_timing.json]
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

LANES = (1, 8, 64)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 4, 5, 6, 7])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--brute-reps", type=int, default=3)
    ap.add_argument("--brute-max-faces", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from recmv import metrics
    from test_nricp_cpu import icosphere
    dev = torch.device("cuda:0")
    rows = []
    for level in args.levels:
        v, f = icosphere(level)
        av, af = v.float().to(dev).contiguous(), f.to(dev).contiguous()
        bv, bf = (0.9 * v + torch.tensor([0.3, 0., 0.])).float().to(dev).contiguous(), af.clone()
        F = af.shape[0]
        row = {"level": level, "faces": F, "face_pairs": F * F}
        grid = metrics.MeshGrid(bv, bf)
        row["grid_dims"], row["grid_entries"] = list(grid.dims), grid.n_entries
        ref = grid.intersections(av, af)[0]
        row["crossing_pairs"] = int(ref.shape[0])
        with_brute = F <= args.brute_max_faces
        if with_brute:
            brute = metrics._brute_crossings(av, af, bv, bf, False)[0]                # (warm-up as well)
            row["grid_equals_brute"] = bool(torch.equal(brute, ref))
        for lanes in LANES:                                                            # warm-up, and the shapes agree
            assert torch.equal(grid.intersections(av, af, lanes=lanes)[0], ref)
        t_build, t_query, t_brute = [], {n: [] for n in LANES}, []
        for r in range(args.reps):                                                     # alternate: build, shapes, brute force
            t_build += _samples(lambda: metrics.MeshGrid(bv, bf), 1)
            for lanes in LANES:
                t_query[lanes] += _samples(lambda: grid.intersections(av, af, lanes=lanes), 1)
            if with_brute and r < args.brute_reps:
                t_brute += _samples(lambda: metrics._brute_crossings(av, af, bv, bf, False), 1)
        row["grid_build_s"] = _stats(t_build)
        row["grid_query_s"] = {str(n): _stats(t) for n, t in t_query.items()}
        best = min(LANES, key=lambda n: statistics.median(t_query[n]))
        row["best_lanes"] = best
        row["grid_total_s"] = row["grid_build_s"]["median"] + row["grid_query_s"][str(best)]["median"]
        row["brute_s"] = _stats(t_brute) if t_brute else None
        rows.append(row)
        print(json.dumps(row), flush=True)
    both = [r for r in rows if r["brute_s"]]
    ratio = [math.log(r["grid_total_s"] / r["brute_s"]["median"]) for r in both]
    crossover, note = None, "not measured"
    if both and all(x < 0 for x in ratio):
        note = "the grid is faster at every size measured"
    elif both and all(x > 0 for x in ratio):
        note = "the brute force is faster at every size measured"
    else:
        for (r0, x0), (r1, x1) in zip(zip(both, ratio), zip(both[1:], ratio[1:])):
            if x0 > 0 >= x1:
                t = x0 / (x0 - x1)
                crossover = int(round(math.exp(math.log(r0["face_pairs"]) * (1 - t) + math.log(r1["face_pairs"]) * t)))
                note = "interpolated between %d and %d faces" % (r0["faces"], r1["faces"])
    total = {n: sum(r["grid_query_s"][str(n)]["median"] for r in rows) for n in LANES}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "brute_reps": args.brute_reps, "rows": rows,
           "crossover_pairs": crossover, "crossover_note": note, "query_s_summed_over_sizes": {str(n): t for n, t in total.items()},
           "best_lanes": min(LANES, key=lambda n: total[n]),
           "constants": {"AUTO_GRID_MIN_PAIRS": metrics.AUTO_GRID_MIN_PAIRS, "INTERSECT_LANES": metrics.INTERSECT_LANES}}
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
