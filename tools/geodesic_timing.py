"""Times of recmv.geodesic on the GPU -> profiles/geodesic_timing.json: both routes across V for B = 1 and B = 32 (square grids
with alternating diagonals, a corner source per field — the farthest corner, so the most sweeps a grid can need), and the sweeps
route on a mesh of marching-cubes size (a 400 x 400 jittered grid, 160 000 vertices, once with its border as the sources and once
with a corner) with its sweep count.  Device events around whole solves (the convergence read-backs of the sweeps route included:
they are part of what a caller pays), after a warm-up; the median of `--reps` solves.

    python tools/geodesic_timing.py [--reps 5] [--out profiles/geodesic_timing.json]
"""
import argparse
import json
import os.path as osp
import sys

import numpy as np
import torch

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path[:0] = [osp.join(REPO, "rec-mv_amd")]


def grid(n, jitter=0., seed=0):
    rng = np.random.default_rng(seed)
    v = np.zeros((n, n, 3))
    v[..., 0], v[..., 1] = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    if jitter:
        v[1:-1, 1:-1, :2] += rng.uniform(-jitter, jitter, (n - 2, n - 2, 2))
        v[..., 2] = rng.uniform(-0.1, 0.1, (n, n))
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = (i * n + j).ravel(), ((i + 1) * n + j).ravel(), ((i + 1) * n + j + 1).ravel(), (i * n + j + 1).ravel()
    even = ((i + j) % 2 == 0).ravel()
    f = np.concatenate([np.where(even[:, None], np.stack([a, b, c], 1), np.stack([a, b, d], 1)),
                        np.where(even[:, None], np.stack([a, c, d], 1), np.stack([b, c, d], 1))])
    return torch.from_numpy(v.reshape(-1, 3).astype(np.float32)).cuda(), torch.from_numpy(f.astype(np.int64)).cuda()


def timed(call, reps):
    call()                                                 # warm-up (the library's load, the allocator, the code objects)
    call()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=osp.join(REPO, "profiles", "geodesic_timing.json"))
    args = ap.parse_args()
    from recmv import geodesic
    cap = geodesic.lds_max_vertices()
    res = {"device": torch.cuda.get_device_name(0), "unit": "microseconds per solve, median of %d" % args.reps,
           "lds_max_vertices": cap, "auto_max_vertices": geodesic.auto_max_vertices(),
           "check_every": geodesic.DEFAULT_CHECK_EVERY, "routes": []}
    for n in (8, 16, 23, 32, 45, 60):
        v, f = grid(n)
        V = n * n
        for B in (1, 32):
            src = [torch.tensor([(b * 37) % V if b else 0]) for b in range(B)]
            mesh = geodesic._Mesh(v, f)
            row = {"V": V, "B": B}
            for route in ("lds", "sweeps"):
                D, K = geodesic._distance(v, f, src, None, route, None, None, mesh)
                row["sweeps_max"] = int(K.max())
                row[route + "_us"] = timed(lambda: geodesic._distance(v, f, src, None, route, None, None, mesh), args.reps)
            print(row, flush=True)
            res["routes"].append(row)
    v, f = grid(400, jitter=0.4, seed=1)
    mesh = geodesic._Mesh(v, f)
    from recmv import connectivity
    border = connectivity.EdgeTable(f, 160000).boundary_vertex.nonzero().squeeze(1).cpu()
    large = []
    for name, src in (("border", [border]), ("corner", [torch.tensor([0])])):
        call = lambda: geodesic._distance(v, f, src, None, "sweeps", None, None, mesh)
        D, K = call()
        row = {"sources": name, "V": 160000, "F": int(f.shape[0]), "sweeps": int(K[0]), "finite": int(torch.isfinite(D).sum())}
        row["us"] = timed(call, max(args.reps // 2, 1))
        row["us_per_sweep"] = row["us"] / (int(K[0]) + 1)
        print(row, flush=True)
        large.append(row)
    res["marching_cubes_size"] = large
    with open(args.out, "w") as out:
        json.dump(res, out, indent=1)
        out.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
