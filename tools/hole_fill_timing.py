"""Time of recmv.holes.triangulate_loops on one MI355X, per route, beside the numpy restatement (tests/hole_fill_reference.py,
on the host) and a plain-torch per-diagonal version on the same device (below): what a caller had without the kernel.
  cases     one noisy circle of 16, 64 (AUTO_MAX_EDGES: where 'auto' changes route), LDS_MAX_EDGES (the most the lds route
            holds) and 1024 vertices, and one call of 1 000 loops of 8-32 vertices
  kernel    every route the sizes allow ('lds' takes at most LDS_MAX_EDGES vertices), the wrapper's read-back of the offsets
            and its workspace allocation included
  torch     per loop and per diagonal one gather, one min: the restatement's arithmetic in float64 torch ops
A warm-up, then `--reps` windows of `--inner` calls each (so that a window is not a fraction of a millisecond), a host clock
around work that ends in a synchronisation; the routes of a case alternate window by window.  The kernel's faces and weights
must be the restatement's bits, and torch's too; the mismatches are recorded.  No test asserts a time; the file is the record.

    python tools/hole_fill_timing.py [--reps 5] [--out profiles/hole_fill_timing.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "rec-mv_amd"), str(REPO), str(REPO / "tests")]


def torch_triangulate(verts, loop_verts, offsets):
    """The restatement in torch float64 on the device: per loop, one diagonal at a time.  (faces, weight) like the kernel."""
    import hole_fill_reference as HR
    dev = verts.device
    faces, weight = [], []
    for l in range(len(offsets) - 1):
        ids = loop_verts[offsets[l]:offsets[l + 1]]
        P = verts[ids].double()
        n = P.shape[0]
        W = torch.zeros((n, n), dtype=torch.float64, device=dev)
        S = torch.zeros((n, n), dtype=torch.int64, device=dev)
        for d in range(2, n):
            I = torch.arange(n - d, device=dev)[:, None]
            K = I + 1 + torch.arange(d - 1, device=dev)[None]
            J = I + d
            u, v = P[K] - P[I], P[J] - P[I]
            cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
            cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
            cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
            c = (W[I, K] + W[K, J]) + 0.5 * torch.sqrt((cx * cx + cy * cy) + cz * cz)
            c = torch.where(torch.isnan(c), torch.full_like(c, float('inf')), c)
            best = c.min(1, keepdim=True)[0]
            m = (c == best).to(torch.int64).argmax(1)                        # the first minimum
            i = I[:, 0]
            W[i, i + d] = best[:, 0]
            S[i, i + d] = i + 1 + m
        faces.append(ids[torch.from_numpy(HR.tree_faces(S.cpu().numpy(), n)).to(dev)])
        weight.append(W[0, n - 1])
    return torch.cat(faces), torch.stack(weight)


def windows(fns, reps, inner):
    """{name: {...}} for alternating windows of `inner` calls of every fn."""
    for fn in fns.values():
        fn()                                                                 # warm-up
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner[k]):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) / inner[k])
    return {k: {"median": statistics.median(x), "min": min(x), "max": max(x), "windows": len(x), "calls_per_window": inner[k]}
            for k, x in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "hole_fill_timing.json"))
    args = ap.parse_args(argv)
    import hole_fill_cases as HC
    import hole_fill_reference as HR
    from recmv import holes
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    cases = {"n16": [HC.circle(16, .05, 16)], "n64": [HC.circle(64, .03, 64)],
             "n%d_lds_max" % holes.LDS_MAX_EDGES: [HC.circle(holes.LDS_MAX_EDGES, .02, 85)],
             "n1024": [HC.circle(1024, .002, 1024)],
             "1000_loops_8_to_32": [HC.circle(int(n), .1, int(n) + i) for i, n in enumerate(rng.integers(8, 33, 1000))]}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "lds_max_edges": holes.LDS_MAX_EDGES,
           "auto_max_edges": holes.AUTO_MAX_EDGES, "cases": {}}
    for name, sets in cases.items():
        verts, lv, lo = HC.pack(sets)
        t = time.perf_counter()
        want_f, want_w = HR.triangulate_loops(verts, lv, lo)
        numpy_s = time.perf_counter() - t
        v, l = torch.from_numpy(verts).to(dev), torch.from_numpy(lv).to(dev)
        o = torch.from_numpy(lo)
        nmax = int((lo[1:] - lo[:-1]).max())
        routes = ["auto", "global"] + (["lds"] if nmax <= holes.LDS_MAX_EDGES else [])
        fns = {r: (lambda r=r: holes.triangulate_loops(v, l, o, route=r)) for r in routes}
        big = nmax > 256 or len(sets) > 100
        inner = {r: 3 if big else 50 for r in routes}
        fns["torch"] = lambda: torch_triangulate(v, l, lo.tolist())
        inner["torch"] = 1
        entry = {"loops": len(sets), "largest": nmax, "candidates": int(sum(n * (n - 1) * (n - 2) // 6 for n in (lo[1:] - lo[:-1]).tolist())),
                 "numpy_seconds": numpy_s, "seconds": windows(fns, args.reps, inner), "mismatches": {}}
        for k, fn in fns.items():
            f, w = fn()
            entry["mismatches"][k] = {"faces": int((f.cpu().numpy() != want_f).any(1).sum()),
                                      "weights": int((w.cpu().numpy().view(np.uint64) != want_w.view(np.uint64)).sum())}
        res["cases"][name] = entry
        print(name, json.dumps(entry), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
    return res


if __name__ == "__main__":
    main()
