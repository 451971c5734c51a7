"""Time of recmv.winding on one MI355X: the exact route against the pyramid route.
  body_88k      exact: 88 000 points against a body of 13 776 faces (a perturbed sphere of 84 x 83 segments), the size of a
                penetration report of a garment against the body
  lattice_129   exact and tree on every node of a lattice of 129 nodes along the longest axis around a mesh of 158 700 faces (a
  lattice_257   perturbed cube-sphere of 115 x 115 cells per side), and of 257: the sizes of a voxel remesh.  The tree's build
                (binning, sort, pyramid) is timed separately, its query with the queries sorted by cell and in lattice order;
                the largest |tree - exact| is recorded
Repeats after a warm-up, a host clock around work that ends in a synchronisation; the exact route at 257 runs once (it is the
long one).  No test asserts a ratio; the file is the record, and DESIGN.md §8 reads it.

Every step runs as a process of its own under `timeout`, and nothing is started after a step that failed; `--step NAME` runs one
step in this process.

    python tools/winding_timing.py [--reps 3] [--limit 300] [--out profiles/winding_timing.json]
"""
import argparse
import json
import math
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "rec-mv_amd"), str(REPO), str(REPO / "tests")]
STEPS = ("body_88k", "lattice_129", "lattice_257")


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _timed(fn, reps, warm=True):
    if warm:
        fn()
    x = [_clock(fn)[0] for _ in range(reps)]
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def _bumpy(p):
    """Points of the unit sphere pushed in and out by up to 9 %: a radius of 0.5 +- 9 %."""
    import torch
    r = 0.5 * (1. + 0.05 * torch.sin(7. * p[:, 0]) * torch.cos(5. * p[:, 1]) + 0.04 * torch.sin(9. * p[:, 2] + 1.))
    return (p * r[:, None]).float().contiguous()


def uv_sphere(n, m):
    """n segments around, m along: 2 n (m - 1) faces, outward."""
    import torch
    th = torch.arange(1, m, dtype=torch.float64) * (math.pi / m)
    ph = torch.arange(n, dtype=torch.float64) * (2. * math.pi / n)
    ring = torch.stack([torch.sin(th)[:, None] * torch.cos(ph)[None], torch.sin(th)[:, None] * torch.sin(ph)[None],
                        torch.cos(th)[:, None].expand(m - 1, n)], -1).reshape(-1, 3)
    v = torch.cat([torch.tensor([[0., 0., 1.]], dtype=torch.float64), ring, torch.tensor([[0., 0., -1.]], dtype=torch.float64)])
    idx = lambda i, j: 1 + i * n + (j % n)  # noqa: E731
    f = [[0, idx(0, j), idx(0, j + 1)] for j in range(n)]
    for i in range(m - 2):
        for j in range(n):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    last = 1 + (m - 1) * n
    f += [[last, idx(m - 2, j + 1), idx(m - 2, j)] for j in range(n)]
    return _bumpy(v), torch.tensor(f, dtype=torch.int64)


def cube_sphere(n):
    """The six sides of a cube, n x n cells each, pushed onto the sphere: 12 n^2 faces, outward (the sides are not welded)."""
    import torch
    t = torch.linspace(-1., 1., n + 1, dtype=torch.float64)
    a, b = torch.meshgrid(t, t, indexing='ij')
    one = torch.ones_like(a)
    sides = [torch.stack(s, -1) for s in ((one, a, b), (-one, b, a), (b, one, a), (a, -one, b), (a, b, one), (b, a, -one))]
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing='ij')
    q = (i * (n + 1) + j).reshape(-1)
    cell = torch.cat([torch.stack([q, q + n + 1, q + n + 2], 1), torch.stack([q, q + n + 2, q + 1], 1)])
    v = torch.cat([s.reshape(-1, 3) for s in sides])
    f = torch.cat([cell + k * (n + 1) ** 2 for k in range(6)])
    return _bumpy(v / v.norm(dim=1, keepdim=True)), f.contiguous()


def step(name, reps):
    import torch
    from recmv import voxelize, winding
    dev = torch.device("cuda:0")
    if name == "body_88k":
        v, f = (x.to(dev) for x in uv_sphere(84, 83))
        g = torch.Generator().manual_seed(0)
        pts = ((torch.rand(88000, 3, generator=g) - 0.5) * 1.3).to(dev)
        w = winding.winding_number(pts, v, f)
        inside = winding.inside_from_winding(w)
        return {"faces": int(f.shape[0]), "points": int(pts.shape[0]), "inside": int(inside.sum()),
                "closed_error": float((w - w.round()).abs().max()),
                "exact": _timed(lambda: winding.winding_number(pts, v, f), reps),
                "tree_build": _timed(lambda: winding.WindingTree(v, f), reps),
                "tree_query": _timed(lambda t=winding.WindingTree(v, f): t.query(pts), reps),
                "tree_levels": winding.WindingTree(v, f).levels}
    resolution = int(name.split("_")[1])
    v, f = (x.to(dev) for x in cube_sphere(115))
    lattice = voxelize.lattice_for(v, resolution=resolution)
    N = lattice.n_nodes

    def nodes(a, b):
        return lattice.points(torch.arange(a, b, device=dev))

    def sweep(fn, out=None):
        for a in range(0, N, voxelize.WINDING_SLICE):
            w = fn(nodes(a, min(a + voxelize.WINDING_SLICE, N)))
            if out is not None:
                out[a:a + voxelize.WINDING_SLICE] = w
        return out
    tree = winding.WindingTree(v, f)
    big = resolution > 200
    w_exact, w_tree = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev)
    res = {"faces": int(f.shape[0]), "lattice": lattice.json(), "nodes": N, "tree_levels": tree.levels, "beta": winding.DEFAULT_BETA,
           "occupied_finest_cells": int(((tree.cell_start[1:] - tree.cell_start[:-1]) > 0).sum()),
           "tree_build": _timed(lambda: winding.WindingTree(v, f), reps),
           "tree_query_sorted": _timed(lambda: sweep(lambda p: tree.query(p), w_tree), reps),
           "tree_query_lattice_order": _timed(lambda: sweep(lambda p: tree.query(p, sort=False)), reps),
           "exact": _timed(lambda: sweep(lambda p: winding.winding_number(p, v, f), w_exact), 1 if big else reps, warm=not big)}
    res["tree_max_error"] = float((w_tree - w_exact).abs().max())
    res["flags_differ"] = int((winding.inside_from_winding(w_tree) != winding.inside_from_winding(w_exact)).sum())
    res["inside"] = int(winding.inside_from_winding(w_exact).sum())
    res["exact_over_tree"] = res["exact"]["median"] / (res["tree_query_sorted"]["median"] + res["tree_build"]["median"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds every step may take")
    ap.add_argument("--step", default=None, choices=STEPS, help="run this one step in this process and print its JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.step:
        import torch
        res = step(args.step, args.reps)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return 0
    res = {"reps": args.reps}
    for n in STEPS:                                        # a fresh process per step, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--step", n,
                            "--reps", str(args.reps)], capture_output=True, text=True)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("step %s ended with status %d; nothing more is started\n%s" % (n, r.returncode, r.stderr[-4000:]), file=sys.stderr)
            return r.returncode or 1
        res[n] = json.loads(line[-1][len("RESULT "):])
        print("%s: done" % n, file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
