"""Time of the segment query through the uniform grid (recmv.metrics.MeshGrid: build + recmv_segment_mesh_grid) against the
brute force recmv_segment_mesh_brute, on icospheres of level 3 .. 7 (1 280 .. 327 680 faces) and 1e4 .. 1e6 seeded segments
with endpoints uniform in 1.5 times the bounding box.  The brute force is timed up to --brute-max-tests segment-face tests.

Every launch shape of the grid query (1, 8 or 64 lanes per segment) and both modes (first hit, counting) are timed; the shapes
and the brute force alternate inside one process, repeat by repeat, after a warm-up of each; every sample is a host clock
around work that ends in a device synchronise; the grid's samples include its build.  Every shape's face, t bits and count are
compared with the brute force's (`same_bits`).  Two constants of recmv.metrics are read off the result:
  best_lanes      the shape with the lowest time summed over the cases and both modes            -> SEGMENT_LANES
  auto_min_tests  the smallest S * F from which on — at that case and every larger one — the grid with `best_lanes` was
                  faster than the brute force in EVERY repeat (the grid's slowest sample below the brute force's fastest),
                  in both modes; null when there is no such case                                 -> AUTO_GRID_MIN_SEGMENT_TESTS

    python tools/segment_mesh_timing.py [--reps 5] [--out profiles/segment_mesh_timing.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(REPO / "tests"))

LANES = (1, 8, 64)


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 4, 5, 6, 7])
    ap.add_argument("--segments", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brute-max-tests", type=float, default=4e10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from recmv import metrics
    from test_nricp_cpu import icosphere
    dev = torch.device("cuda:0")
    rows = []
    for level in args.levels:
        v, f = icosphere(level)
        v, f = (0.5 * v).float().to(dev).contiguous(), f.to(dev).contiguous()
        for S in args.segments:
            g = torch.Generator().manual_seed(S + level)
            pq = (0.75 * (2 * torch.rand(2, S, 3, generator=g) - 1)).float().to(dev)
            p, q = pq[0].contiguous(), pq[1].contiguous()
            tests = S * f.shape[0]
            brute_on = tests <= args.brute_max_tests

            def grid(lanes, count):
                return metrics.MeshGrid(v, f).segment_hits(p, q, count=count, lanes=lanes)

            def brute(count):
                return metrics.segment_hits(p, q, v, f, count=count, method='brute')
            shapes = [(n, c) for n in LANES for c in (False, True)]
            want = brute(True) if brute_on else grid(1, True)
            same = True
            for n, c in shapes:                                                    # warm-up of every shape, and the comparison
                got = grid(n, c)
                same &= torch.equal(got['face'], want['face']) and torch.equal(got['t'].view(torch.int32), want['t'].view(torch.int32))
                same &= (not c) or torch.equal(got['count'], want['count'])
            t_grid = {s: [] for s in shapes}
            t_brute = {False: [], True: []}
            for _ in range(args.reps):                                             # alternated, repeat by repeat
                for n, c in shapes:
                    t_grid[(n, c)].append(_clock(lambda: grid(n, c))[0])
                if brute_on:
                    for c in (False, True):
                        t_brute[c].append(_clock(lambda: brute(c))[0])
            row = {"level": level, "faces": int(f.shape[0]), "segments": S, "tests": tests, "same_bits": bool(same),
                   "judge": "brute" if brute_on else "grid lanes 1",
                   "hitting": int((want['face'] >= 0).sum()), "grid": {}, "brute": {}}
            for (n, c), x in t_grid.items():
                row["grid"]["lanes%d_%s" % (n, "count" if c else "first")] = _stats(x)
            for c, x in t_brute.items():
                if x:
                    row["brute"]["count" if c else "first"] = _stats(x)
            rows.append(row)
            print(json.dumps(row), flush=True)
    total = {n: sum(r["grid"]["lanes%d_%s" % (n, m)]["median"] for r in rows for m in ("first", "count")) for n in LANES}
    best = min(total, key=total.get)

    def grid_always_faster(r):
        if not r["brute"]:
            return None
        return all(r["grid"]["lanes%d_%s" % (best, m)]["max"] < r["brute"][m]["min"] for m in ("first", "count"))
    ordered = sorted(rows, key=lambda r: r["tests"])
    auto = None
    for k in range(len(ordered) - 1, -1, -1):
        if grid_always_faster(ordered[k]) is False:
            break
        if grid_always_faster(ordered[k]):
            auto = ordered[k]["tests"]
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows, "summed_median_seconds": total,
           "best_lanes": best, "auto_min_tests": auto, "all_same_bits": all(r["same_bits"] for r in rows)}
    print(json.dumps({k: res[k] for k in ("best_lanes", "auto_min_tests", "all_same_bits", "summed_median_seconds")}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if res["all_same_bits"] else 1


if __name__ == "__main__":
    sys.exit(main())
