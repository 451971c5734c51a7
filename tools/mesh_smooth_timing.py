"""Time of recmv.smooth at a marching-cubes size, on one MI355X: the unit icosphere at level 7 (163 842 vertices, 327 680 faces)
with Gaussian noise of 0.2 x the mean edge length.
  kernels     recmv_cotan_weights, recmv_laplacian_step (uniform and weighted), recmv_face_normal_filter and
              recmv_vertex_from_normals, one launch each with the tables built beforehand (the launch and its synchronisation),
              and their plain-torch float64 restatements on the same card, alternated
  smooth      the whole call for taubin (uniform, cotangent) and bilateral with the defaults, kernel path and
              `use_kernels=False` on the same card, alternated; both include the tables and the info
Every sample is a host clock around work that ends in a synchronisation, after a warm-up of each.  No threshold hangs on these
numbers.
  --write-obj DIR     also writes the mesh as DIR/sphere7.obj (for `clean_fl.py --smooth` under a profiler)

    python tools/mesh_smooth_timing.py [--reps 10] [--call-reps 3] [--out profiles/mesh_smooth_timing.json] [--write-obj DIR]
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


def _alternate(calls, reps):
    for fn in calls.values():
        fn()                                               # warm-up of each
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            times[k].append(_clock(fn)[0])
    return {k: _stats(t) for k, t in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--call-reps", type=int, default=3)
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-obj", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import mesh_smooth_cases as MC
    from recmv import connectivity, smooth
    from recmv.utils import write_obj
    assert torch.cuda.is_available(), "the timing needs a GPU"
    dev = torch.device("cuda:0")
    v, f = MC.icosphere(args.level)
    v = (v + np.random.default_rng(7).standard_normal(v.shape) * (0.2 * MC.mean_edge_length(v, f))).astype(np.float32)
    if args.write_obj:
        Path(args.write_obj).mkdir(parents=True, exist_ok=True)
        write_obj(str(Path(args.write_obj) / ("sphere%d.obj" % args.level)), torch.from_numpy(v), torch.from_numpy(f))
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    V, F = tv.shape[0], tf.shape[0]
    table = connectivity.EdgeTable(tf, V)
    nbr, slots = connectivity.neighbours_csr(table.edges, V), connectivity.vertex_slots_csr(tf, V)
    ff = connectivity.face_neighbours_csr(table)
    unit, area, cen, _ = smooth.face_geometry(tv, tf)
    n32 = unit.float().contiguous()
    w = smooth.cotangent_weights(tv, tf, nbr, slots)
    sigma_c = 0.5 * MC.mean_edge_length(v, f)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "call_reps": args.call_reps, "vertices": V, "faces": F,
           "neighbour_entries": int(nbr[1].numel()), "face_neighbour_entries": int(ff[1].numel())}
    res["kernels"] = _alternate({
        "cotan_weights": lambda: smooth.cotangent_weights(tv, tf, nbr, slots),
        "torch_cotan_weights": lambda: smooth.cotangent_weights_torch(tv, tf, nbr, slots),
        "laplacian_step_uniform": lambda: smooth.laplacian_step(tv, nbr, 0.5),
        "torch_laplacian_step_uniform": lambda: smooth.laplacian_step_torch(tv, nbr, 0.5),
        "laplacian_step_weighted": lambda: smooth.laplacian_step(tv, nbr, 0.5, w),
        "torch_laplacian_step_weighted": lambda: smooth.laplacian_step_torch(tv, nbr, 0.5, w),
        "face_normal_filter": lambda: smooth.filter_face_normals(n32, area, cen, ff, sigma_c, 0.35),
        "torch_face_normal_filter": lambda: smooth.filter_face_normals_torch(n32, area, cen, ff, sigma_c, 0.35),
        "vertex_from_normals": lambda: smooth.update_vertices(tv, tf, n32, slots),
        "torch_vertex_from_normals": lambda: smooth.update_vertices_torch(tv, tf, n32, slots),
        "tables": lambda: (connectivity.EdgeTable(tf, V), connectivity.vertex_slots_csr(tf, V)),
        "face_neighbours_csr": lambda: connectivity.face_neighbours_csr(table),
    }, args.reps)
    print("kernels: done", file=sys.stderr, flush=True)
    res["smooth"] = {}
    for name, kw in (("taubin_uniform", dict(method="taubin")), ("taubin_cotangent", dict(method="taubin", weights="cotangent")),
                     ("bilateral", dict(method="bilateral"))):
        infos = {}

        def whole(use_kernels, kw=kw, infos=infos):
            x, infos[use_kernels] = smooth.smooth(tv, tf, use_kernels=use_kernels, **kw)
            return x
        entry = _alternate({"kernels": lambda: whole(True), "torch": lambda: whole(False)}, args.call_reps)
        entry["roughness"] = {k: [i["roughness_before"], i["roughness_after"]] for k, i in (("kernels", infos[True]), ("torch", infos[False]))}
        res["smooth"][name] = entry
        print("%s: done" % name, file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
