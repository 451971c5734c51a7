"""Wall time and CG iterations of the Laplacian alignment solve, kernel path against the dense torch path, on icospheres of
subdivision levels 4, 5 and 6 (2562 / 10242 / 40962 vertices before cutting) with four caps cut off and their rings displaced
along y as the curves.  Writes profiles/lap_align_timing.json (or --out).

    python tools/lap_align_timing.py [--levels 4 5 6] [--reps 3] [--out profiles/lap_align_timing.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(REPO / "tests"))


def _time(fn, reps):
    import torch
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 5, 6])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(REPO / "profiles" / "lap_align_timing.json"))
    args = ap.parse_args(argv)
    import torch
    from recmv import lap_align as LA
    from test_lap_align_cpu import CAPS, cut_sphere, ring
    dev = "cuda:0"
    rows = []
    for level in args.levels:
        v, f = cut_sphere(level)
        loops = LA.boundary_loops(f)
        curves = {n: ring(n, dy=0.15) for n in CAPS}
        fl = LA.assign_loops(loops, v, curves, list(CAPS), log=lambda s: None)
        t0 = time.perf_counter()
        idx, tgt, _ = LA.match(v, loops, fl, curves)
        cw, cwt = LA.constraint_weights(idx, tgt, v.shape[0], 1.)
        t_match = time.perf_counter() - t0
        topo = LA.Topology(f, v.shape[0], dev)
        vd = v.to(dev)
        t_solve, (u, iters, res) = _time(lambda: LA.solve(topo, vd, cw, cwt), args.reps)
        t_smooth, _ = _time(lambda: LA.smooth(topo, u), 20)
        row = dict(level=level, vertices=v.shape[0], faces=f.shape[0], pairs=int(idx.shape[0]), tol=LA.TOL,
                   cg_iterations=iters, residual=max(res), kernel_solve_s=t_solve, us_per_iteration=1e6 * t_solve / max(iters, 1),
                   kernel_smooth_s=t_smooth, match_cpu_s=t_match)
        if v.shape[0] <= LA.DENSE_MAX_V:
            t_dense, ut = _time(lambda: LA.solve_torch(topo, vd, cw, cwt), 1)
            row.update(torch_dense_solve_s=t_dense, max_abs_diff_vs_dense=float((u - ut).abs().max()))
        else:
            row.update(torch_dense_solve_s=None, note="over DENSE_MAX_V=%d: the torch path refuses" % LA.DENSE_MAX_V)
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0), rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
