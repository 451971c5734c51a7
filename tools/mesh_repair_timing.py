"""Time of recmv.repair at the size of an extraction, on one MI355X: the bench scene's marching-cubes meshes (the frozen scene's
body and two garments after one re-mesh) as SOUP — every face given its own three vertices, about 1 M vertices — which is what
a scan exported with one vertex triple per face looks like.
  points_within      the whole call with eps = 0 (its two read-backs, the sort by cell and the tables included), and its three
                     launches alone on prebuilt tables (cells; count; fill), with the bytes each must move — the coordinates,
                     ids and cell table in, the counts or the offsets and the pair rows out, every array once — and the share
                     of the HBM peak (8.0 TB/s spec; about 6.3 TB/s is what a copy reaches) that makes
  weld, drop_degenerate, split_nonmanifold, orient, repair   every stage on the mesh the stage before it left, and the chain
Every sample is a host clock around work that ends in a synchronisation, medians of --reps repeats after a warm-up.  No
threshold hangs on these numbers.

The driver starts every step as a process of its own under `timeout`, so a step that hangs ends there and nothing is started
after a step that failed; `--step NAME` runs one step in this process.

    python tools/mesh_repair_timing.py [--reps 10] [--limit 240] [--out profiles/mesh_repair_timing.json]
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
STEPS = ("points_within", "stages")
HBM_PEAK = 8.0e12


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def _timed(fn, reps):
    fn()                                                   # warm-up
    return _stats([_clock(fn)[0] for _ in range(reps)])


def scene_soup(dev):
    """The frozen bench scene's marching-cubes meshes after one re-mesh, as one soup: (verts [3F,3] f32, faces [F,3] int64)."""
    import torch
    import bench
    from recmv.hocon import ConfigFactory
    from recmv.loop import HotLoop
    conf = ConfigFactory.parse_file(str(REPO / "configs" / "synthetic" / "people_snapshot_like.conf"))
    loop = HotLoop(conf, dev, stage="coarse", curves=True, **bench.HOTLOOP_KW)
    bench.load_scene(loop, bench.SCENE_FILE)
    loop.marching_cube_update({'sdfRatio': 1., 'deformerRatio': loop.opt_times / 2500. + 0.5, 'renderRatio': 1.})
    tri = torch.cat([v.detach().float()[f.long().reshape(-1)] for v, f in zip([loop.body_vs] + list(loop.garment_vs),
                                                                                [loop.body_fs] + list(loop.garment_fs))])
    faces = torch.arange(tri.shape[0], dtype=torch.int64, device=tri.device).reshape(-1, 3)
    return tri.contiguous(), faces.contiguous()


def step_points_within(reps):
    import torch
    from recmv import _lib as L
    from recmv import repair
    dev = torch.device("cuda:0")
    v, f = scene_soup(dev)
    V = v.shape[0]
    pairs, info = repair.points_within(v, 0., return_info=True)
    res = {"vertices": V, "faces": int(f.shape[0]), "eps": 0., "pairs": info["pairs"], "cell": info["cell"], "dims": list(info["dims"]),
           "call": _timed(lambda: repair.points_within(v, 0.), reps)}
    # the three launches alone, on the tables the call builds
    box = torch.stack([v.amin(0), v.amax(0)]).double().cpu().tolist()
    origin, cell, dims = repair.grid_layout(box[0], box[1], 0., V)
    grid = (origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2])
    cells = dims[0] * dims[1] * dims[2]
    lib, stream = L.lib(), L.stream_ptr(dev)
    cell_of = torch.empty(V, dtype=torch.int32, device=dev)

    def run_cells():
        L.check(lib.recmv_points_within_cells(L.ptr(v), V, *grid, L.ptr(cell_of), stream), "cells")
    run_cells()
    ids = (cell_of >= 0).nonzero().squeeze(1)
    key, perm = torch.sort(cell_of[ids].long(), stable=True)
    ids = ids[perm].contiguous()
    pts = v[ids].contiguous()
    n = int(ids.shape[0])
    cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = torch.cumsum(torch.bincount(key, minlength=cells), 0)
    counts = torch.empty(V, dtype=torch.int64, device=dev)

    def run_count():
        L.check(lib.recmv_points_within_count(L.ptr(pts), L.ptr(ids), n, V, 0., *grid, L.ptr(cell_start), L.ptr(counts), stream), "count")
    run_count()
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item())
    offsets = (ends - counts).contiguous()
    out = torch.empty((total, 2), dtype=torch.int64, device=dev)

    def run_fill():
        L.check(lib.recmv_points_within_fill(L.ptr(pts), L.ptr(ids), n, V, 0., *grid, L.ptr(cell_start), L.ptr(offsets), L.ptr(out), total,
                                             stream), "fill")
    run_fill()
    assert total == info["pairs"] and torch.equal(out, pairs)
    tables = n * 12 + n * 8 + (cells + 1) * 4
    nbytes = {"cells": V * 12 + V * 4, "count": tables + V * 8, "fill": tables + V * 8 + total * 16}
    res["cells_in_table"] = cells
    # the distance tests one launch makes: for every sorted vertex the vertices in the 27 cells round its own
    occ = (cell_start[1:] - cell_start[:-1]).reshape(dims[2], dims[1], dims[0]).float()
    box = torch.nn.functional.avg_pool3d(occ[None, None], 3, stride=1, padding=1, divisor_override=1)[0, 0]
    res["candidate_tests"] = int((box.double() * occ.double()).sum().item())
    res["kernels"] = {}
    for name, fn in (("cells", run_cells), ("count", run_count), ("fill", run_fill)):
        t = _timed(fn, reps)
        res["kernels"][name] = {**t, "bytes": nbytes[name], "hbm_share_of_8TBs": nbytes[name] / t["median"] / HBM_PEAK}
    both = res["kernels"]["count"]["median"] + res["kernels"]["fill"]["median"]
    res["search_bytes"] = nbytes["count"] + nbytes["fill"]
    res["search_seconds"] = both
    res["search_hbm_share_of_8TBs"] = res["search_bytes"] / both / HBM_PEAK
    res["candidate_tests_per_second"] = 2 * res["candidate_tests"] / both
    return res


def step_stages(reps):
    import torch
    from recmv import connectivity, repair, topology
    dev = torch.device("cuda:0")
    v, f = scene_soup(dev)
    res = {"vertices": int(v.shape[0]), "faces": int(f.shape[0])}
    wv, wf, wi = repair.weld(v, f, 0.)
    res["weld"] = {**_timed(lambda: repair.weld(v, f, 0.), reps), **repair.info_json(wi)}
    dv, df, di = repair.drop_degenerate(wv, wf)
    res["drop_degenerate"] = {**_timed(lambda: repair.drop_degenerate(wv, wf), reps), **repair.info_json(di)}
    sv, sf, si = repair.split_nonmanifold(dv, df)
    res["split_nonmanifold"] = {**_timed(lambda: repair.split_nonmanifold(dv, df), reps), **repair.info_json(si)}
    ov, of, oi = repair.orient(sv, sf)
    res["orient"] = {**_timed(lambda: repair.orient(sv, sf), reps), **repair.info_json(oi)}
    res["compact"] = _timed(lambda: connectivity.compact(ov, of), reps)
    rv, rf, ri = repair.repair(v, f, weld_eps=0.)
    res["repair"] = {**_timed(lambda: repair.repair(v, f, weld_eps=0.), reps), "vertices_after": int(rv.shape[0]),
                     "faces_after": int(rf.shape[0])}
    rep = topology.report(rv, rf)
    res["report_after"] = {k: rep[k] for k in ("vertices", "faces", "components_vertex", "boundary_edges", "nonmanifold_edges",
                                               "orientation_conflicts", "boundary_pinch_vertices", "zero_area_faces",
                                               "duplicate_faces", "watertight")}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds every step may take")
    ap.add_argument("--step", default=None, choices=STEPS, help="run this one step in this process and print its JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.step:
        import torch
        res = {"points_within": step_points_within, "stages": step_stages}[args.step](args.reps)
        res["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(res))
        return 0
    res = {"reps": args.reps, "hbm_peak_bytes_per_second": HBM_PEAK}
    for step in STEPS:                                     # a fresh process per step, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--step", step,
                            "--reps", str(args.reps)], capture_output=True, text=True)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("step %s ended with status %d; nothing more is started\n%s" % (step, r.returncode, r.stderr[-4000:]), file=sys.stderr)
            return r.returncode or 1
        res[step] = json.loads(line[-1][len("RESULT "):])
        print("%s: done" % step, file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
