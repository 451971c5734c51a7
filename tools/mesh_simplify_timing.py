"""Time of recmv.simplify at the bench scene's garment sizes, on one MI355X.  The frozen scene's two garments are marching-cubes
meshes of 88 k and 73 k vertices (176 k + 146 k faces).  The meshes here are the irregular test body Loop-subdivided four times
(327 680 faces: the two garments' faces together) and that mesh simplified to 176 000 and to 146 000 faces (irregular meshes of the
two garments' sizes).
  kernels     recmv_vertex_quadrics, recmv_edge_collapse_cost and recmv_collapse_flip_check on every edge of each mesh, with
              the tables built beforehand (the launch and its synchronisation), and their plain-torch float64 restatements on
              the same card
  simplify    the whole call to a quarter of the faces, kernel path and `use_kernels=False` on the same card, alternated, with
              the rounds and collapses it took; `rounds_kernels_upper` = quadrics + rounds x (cost + flip check on every edge of the
              input), an upper bound of the time the call spends in the three kernels (later rounds have fewer edges)
  quality     tests/mesh_simplify_cases.quality_figures (what tests/test_gpu_mesh_simplify.py asserts), written to --quality-out
Every sample is a host clock around work that ends in a synchronisation, after a warm-up of each.  No threshold hangs on these
numbers.

    python tools/mesh_simplify_timing.py [--reps 10] [--call-reps 3] [--out profiles/mesh_simplify_timing.json]
        [--quality-out profiles/mesh_simplify_quality.json]
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality-out", default=None)
    args = ap.parse_args(argv)
    import torch
    import mesh_simplify_cases as SC
    from recmv import connectivity, iso_remesh, simplify
    from recmv.iso_remesh import _Topo, _flip_ok
    from test_gpu_animation import _irregular_body
    dev = torch.device("cuda:0")
    v, f = _irregular_body(level=3)
    v, f = iso_remesh.loop_subdivide(v.to(dev), f.to(dev), levels=4)
    meshes = {"both_garments_327680": (v.contiguous(), f.contiguous())}
    for name, target in (("garment_176000", 176000), ("garment_146000", 146000)):
        gv, gf, _ = simplify.simplify(v, f, target_faces=target)
        meshes[name] = (gv, gf)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "call_reps": args.call_reps,
           "boundary_weight": simplify.BOUNDARY_WEIGHT, "reach": simplify.REACH, "round_share": simplify.ROUND_SHARE, "meshes": {}}
    for name, (mv, mf) in meshes.items():
        V, F = mv.shape[0], mf.shape[0]
        table = connectivity.EdgeTable(mf, V)
        topo = _Topo(mf, V)
        edges = table.edges.contiguous()
        code = torch.zeros(edges.shape[0], dtype=torch.uint8, device=dev)
        vf = (topo.vf[0], (topo.vf[1] // 3).contiguous())
        Q = simplify.vertex_quadrics(mv, mf, table)
        pos, _, _ = simplify.edge_collapse_cost(Q, mv, edges, code)
        entry = {"vertices": V, "faces": F, "edges": int(edges.shape[0])}
        entry["kernels"] = _alternate({
            "vertex_quadrics_with_tables": lambda: simplify.vertex_quadrics(mv, mf, table),
            "edge_collapse_cost": lambda: simplify.edge_collapse_cost(Q, mv, edges, code),
            "collapse_flip_check": lambda: simplify.collapse_flip_check(mv, mf, edges, pos, vf),
            "torch_vertex_quadrics": lambda: simplify.vertex_quadrics_torch(mv, mf, table),
            "torch_edge_collapse_cost": lambda: simplify.edge_collapse_cost_torch(Q, mv, edges, code),
            "torch_flip_check": lambda: _flip_ok(mv.double(), mf, topo, edges[:, 0], edges[:, 1], pos.double()),
            "tables_edge_table_and_topo": lambda: _Topo(mf, V),
        }, args.reps)
        # the quadric kernel alone: the wrapper above builds its two CSR tables on every call
        off, slots = connectivity.vertex_slots_csr(mf, V)
        border, boff, brows = connectivity.boundary_edges_csr(table)
        from recmv import _lib as L
        faces_of = (slots // 3).contiguous()
        out, counts = torch.empty(V, 11, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

        def quadrics_alone():
            L.check(L.lib().recmv_vertex_quadrics(L.ptr(mv), V, L.ptr(mf), F, L.ptr(off), L.ptr(faces_of), faces_of.numel(),
                                                  L.ptr(border), border.shape[0], L.ptr(boff), L.ptr(brows), brows.numel(),
                                                  simplify.BOUNDARY_WEIGHT, L.ptr(out), L.ptr(counts), L.stream_ptr(dev)), "quadrics")
        entry["kernels"].update(_alternate({"vertex_quadrics": quadrics_alone}, args.reps))
        info = {}

        def whole(use_kernels):
            nv, nf, i = simplify.simplify(mv, mf, ratio=0.25, use_kernels=use_kernels)
            info[use_kernels] = i
            return nv
        entry["simplify_to_a_quarter"] = _alternate({"kernels": lambda: whole(True), "torch": lambda: whole(False)}, args.call_reps)
        k = entry["kernels"]
        entry["rounds"] = {"kernels": info[True]["rounds"], "torch": info[False]["rounds"]}
        entry["collapses"] = {"kernels": info[True]["collapses"], "torch": info[False]["collapses"]}
        entry["faces_after"] = {"kernels": info[True]["faces_after"], "torch": info[False]["faces_after"]}
        entry["max_error"] = {"kernels": info[True]["max_error"], "torch": info[False]["max_error"]}
        entry["rounds_kernels_upper"] = k["vertex_quadrics"]["median"] + info[True]["rounds"] * (
            k["edge_collapse_cost"]["median"] + k["collapse_flip_check"]["median"])
        res["meshes"][name] = entry
        print("%s: done" % name, file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if args.quality_out:
        q = SC.quality_figures(dev)
        q["device"] = res["device"]
        print(json.dumps(q))
        with open(args.quality_out, "w") as fh:
            json.dump(q, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
