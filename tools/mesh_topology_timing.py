"""Time of recmv.topology at the size of an extraction: the irregular test body Loop-subdivided four times (327 680 faces) plus
2 000 floaters (small tetrahedra), on one MI355X.
  components         topology.components, 'vertex' and 'edge' (labels, dense ids, areas, boxes; its read-backs included)
  report             topology.report
  keep_components    topology.keep_components(min_area_frac=0.01)
  graph_components   the labels alone on the vertex rows (K = 3) and on the face-pair rows of the 'edge' mode (K = 2), for every
                     value of rounds-per-read-back in --per, with the rounds the fixpoint needed; the same rows once more with the
                     vertices numbered by a random permutation, and on a path over as many nodes numbered descending (one chain
                     through every node: the longest walk the compression can meet) and randomly (the most rounds)
  scipy              scipy.sparse.csgraph.connected_components on the host's CPU for the same rows (the matrix build included,
                     the copy of the rows to the host not)
Every sample is a host clock around work that ends in a synchronisation; the variants alternate repeat by repeat after a warm-up
of each.  The file also says whether the labels equal scipy's components.  No threshold hangs on these numbers;
recmv.topology.ROUNDS_PER_READBACK is to be set to the --per value with the lowest median.

    python tools/mesh_topology_timing.py [--levels 4] [--floaters 2000] [--reps 10] [--per 1 2 4 8 16]
        [--out profiles/mesh_topology_timing.json]
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


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def scene(levels, n_floaters, device):
    import numpy as np
    import torch
    import mesh_topology_cases as TC
    from recmv import iso_remesh
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)
    v, f = iso_remesh.loop_subdivide(v.to(device), f.to(device), levels=levels)
    g = np.random.default_rng(1)
    d = g.normal(size=(n_floaters, 3))
    d = (1.5 + g.random((n_floaters, 1))) * d / np.linalg.norm(d, axis=1, keepdims=True)
    fv, ff = TC.merge(*[TC.tetrahedron(0.002 * (1 + i / n_floaters), d[i]) for i in range(n_floaters)])   # no two of one size
    return (torch.cat([v, torch.from_numpy(fv).to(device)]).contiguous(),
            torch.cat([f, torch.from_numpy(ff + v.shape[0]).to(device)]).contiguous())


def scipy_components(n, rows):
    """(seconds, labels as the smallest member id) of scipy's connected components for rows [M,K] on the host."""
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = time.perf_counter()
    a = np.concatenate([rows[:, k] for k in range(rows.shape[1] - 1)])
    b = np.concatenate([rows[:, k + 1] for k in range(rows.shape[1] - 1)])
    _, lab = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
    dt = time.perf_counter() - t
    smallest = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    return dt, smallest[lab]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=4, help="Loop subdivisions of the 1 280-face body")
    ap.add_argument("--floaters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--per", type=int, nargs="+", default=[1, 2, 4, 8, 16], help="rounds between read-backs to try")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from recmv import connectivity, topology
    dev = torch.device("cuda:0")
    v, f = scene(args.levels, args.floaters, dev)
    V, F = v.shape[0], f.shape[0]
    edge, order = torch.sort(connectivity.edges_packed(f, V)[1].reshape(-1), stable=True)     # as topology.components does
    hface = order // 3
    same = edge[1:] == edge[:-1]
    pairs = torch.stack([hface[:-1][same], hface[1:][same]], 1).contiguous()
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(0)).to(dev)
    chain = torch.arange(V - 1, device=dev)
    graphs = {"vertex_rows": (V, f), "face_pair_rows": (F, pairs), "vertex_rows_shuffled": (V, perm[f].contiguous()),
              "path_descending": (V, torch.stack([chain + 1, chain], 1).contiguous()),
              "path_shuffled": (V, torch.stack([perm[chain + 1], perm[chain]], 1).contiguous())}
    res = {"device": torch.cuda.get_device_name(0), "vertices": V, "faces": F, "floaters": args.floaters, "reps": args.reps,
           "rounds_per_readback_in_use": topology.ROUNDS_PER_READBACK, "graph_components": {}}
    for name, (n, rows) in graphs.items():
        entry = {"nodes": n, "rows": int(rows.shape[0]), "K": int(rows.shape[1]), "per": {}}
        runs = {per: (lambda per=per: topology.graph_components(n, rows, return_info=True, rounds_per_readback=per)) for per in args.per}
        label, info = runs[args.per[0]]()
        for fn in runs.values():
            fn()                                           # warm-up of each
        times = {per: [] for per in args.per}
        for _ in range(args.reps):                         # alternated, repeat by repeat
            for per, fn in runs.items():
                times[per].append(_clock(fn)[0])
        entry["rounds"], entry["cap"], entry["invalid"] = info["rounds"], info["cap"], info["invalid"]
        entry["per"] = {str(per): _stats(t) for per, t in times.items()}
        entry["best_per"] = min(args.per, key=lambda per: statistics.median(times[per]))
        host_rows = rows.cpu().numpy()
        cpu = [scipy_components(n, host_rows) for _ in range(3)]
        entry["scipy_host_seconds"] = _stats([c[0] for c in cpu])
        entry["labels_equal_scipy"] = bool((label.cpu().numpy() == cpu[0][1]).all())
        res["graph_components"][name] = entry
    calls = {"components_vertex": lambda: topology.components(v, f, 'vertex'),
             "components_edge": lambda: topology.components(v, f, 'edge'),
             "report": lambda: topology.report(v, f),
             "keep_components": lambda: topology.keep_components(v, f, min_area_frac=0.01)}
    outs = {k: fn() for k, fn in calls.items()}            # warm-up of each
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            times[k].append(_clock(fn)[0])
    for k in calls:
        res[k] = _stats(times[k])
    res["components"] = {"vertex": outs["components_vertex"]["count"], "edge": outs["components_edge"]["count"],
                         "rounds_vertex": outs["components_vertex"]["rounds"], "rounds_edge": outs["components_edge"]["rounds"]}
    res["kept_faces"] = int(outs["keep_components"][1].shape[0])
    res["dropped_components"] = outs["keep_components"][2]["dropped_components"]
    rep = outs["report"]
    res["report_summary"] = {k: rep[k] for k in ("components_vertex", "components_edge", "boundary_loops", "euler_characteristic",
                                                 "watertight", "edges", "area")}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
