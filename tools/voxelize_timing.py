"""Time of recmv.voxelize.distance_field on one MI355X, against the composition the package offered before it: the level-4
irregular body (5 120 faces; tests/test_gpu_animation._irregular_body) on lattices of 65^3 and 129^3 nodes.
  field      distance_field, signed, at the default band of 3 steps: the band kernel, the inside test of the band nodes
             (metrics.points_inside, unchanged) and the column walk; and `unsigned`, the two kernels alone
  baseline   MeshGrid.closest_point on EVERY node plus metrics.points_inside on EVERY node (in slices of --slice nodes: its
             three segments per node are materialised) — what a caller had to do without the narrow band
Three repeats each after a warm-up, a host clock around work that ends in a synchronisation.  The two must agree: at the band
nodes the field's dist2 and face are the baseline's bits and its inside flags the baseline's; the mismatches are recorded.  No
test asserts a ratio; the file is the record.

Every lattice runs as a process of its own under `timeout`, and nothing is started after a step that failed; `--step N` runs
one lattice in this process.

    python tools/voxelize_timing.py [--reps 3] [--limit 300] [--out profiles/voxelize_timing.json]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "rec-mv_amd"), str(REPO), str(REPO / "tests")]
RESOLUTIONS = (65, 129)


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _timed(fn, reps):
    fn()                                                   # warm-up
    x = [_clock(fn)[0] for _ in range(reps)]
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def step(resolution, reps, slice_nodes):
    import torch
    from recmv import metrics, voxelize
    from test_gpu_animation import _irregular_body
    dev = torch.device("cuda:0")
    v, f = (x.to(dev).contiguous() for x in _irregular_body(level=4))
    lattice = voxelize.lattice_for(v, resolution=resolution)
    nodes = lattice.nodes(dev).reshape(-1, 3).contiguous()
    N = nodes.shape[0]

    def baseline():
        face, _, dist2 = metrics.MeshGrid(v, f).closest_point(nodes)
        inside = torch.cat([metrics.points_inside(nodes[s:s + slice_nodes], v, f) for s in range(0, N, slice_nodes)])
        return face, dist2, inside

    field = voxelize.distance_field(v, f, lattice)
    face, dist2, inside = baseline()
    b = torch.tensor(field['band'], dtype=torch.float32, device=dev)
    in_band = dist2 <= b * b
    got_d, got_f = field['dist2'].reshape(-1), field['face'].reshape(-1)
    res = {"faces": int(f.shape[0]), "lattice": lattice.json(), "nodes": N, "band": field['band'], "band_nodes": field['band_nodes'],
           "open_columns": field['open_columns'], "sign_conflicts": field['sign_conflicts'],
           "mismatches": {"band_membership": int((in_band != torch.isfinite(got_d)).sum()),
                          "dist2_bits": int((got_d[in_band].view(torch.int32) != dist2[in_band].view(torch.int32)).sum()),
                          "face": int((got_f[in_band] != face[in_band]).sum()),
                          "inside": int((field['inside'].reshape(-1) != inside).sum())},
           "field": _timed(lambda: voxelize.distance_field(v, f, lattice), reps),
           "unsigned": _timed(lambda: voxelize.distance_field(v, f, lattice, signed=False), reps),
           "baseline": _timed(baseline, reps)}
    res["baseline_over_field"] = res["baseline"]["median"] / res["field"]["median"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds every lattice may take")
    ap.add_argument("--slice", type=int, default=1 << 18, help="nodes per points_inside call of the baseline")
    ap.add_argument("--step", type=int, default=None, choices=RESOLUTIONS, help="run this one lattice in this process and print its JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.step:
        import torch
        res = step(args.step, args.reps, args.slice)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return 0
    res = {"reps": args.reps}
    for n in RESOLUTIONS:                                  # a fresh process per lattice, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--step", str(n),
                            "--reps", str(args.reps), "--slice", str(args.slice)], capture_output=True, text=True)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("lattice %d ended with status %d; nothing more is started\n%s" % (n, r.returncode, r.stderr[-4000:]), file=sys.stderr)
            return r.returncode or 1
        res["resolution_%d" % n] = json.loads(line[-1][len("RESULT "):])
        print("%d: done" % n, file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
