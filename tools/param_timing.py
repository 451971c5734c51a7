"""Times of recmv.param on the GPU -> profiles/param_timing.json: the harmonic solve (cotangent weights, tol 1e-12, the circle
fixed, from 0) on square grids from 5 x 5 up to the lds route's capacity and on 65 x 65 and 129 x 129, on both routes where both
apply — device events around whole solves (the launch route's read-backs included: they are part of what a caller pays), two
warm-up solves, the median of `--reps`, per solve and per CG iteration — and the wall time of 20 ARAP iterations (tables built,
harmonic start excluded) on the cut shirt of tests/param_cases.py and on a 129 x 129 grid lifted to a sphere, per route.  The
largest size at which the lds route's median is below the launch route's is the crossover recmv_param_auto_max_vertices()
should hold.  Last, the CG iterations of the numpy restatement on the test cases (CPU).

    python tools/param_timing.py [--reps 7] [--out profiles/param_timing.json]
"""
import argparse
import json
import os.path as osp
import sys
import time

import numpy as np
import torch

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path[:0] = [osp.join(REPO, "rec-mv_amd"), osp.join(REPO, "tests")]


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


def wall(call, reps):
    call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=osp.join(REPO, "profiles", "param_timing.json"))
    args = ap.parse_args()
    import param_cases as PC
    from recmv import param
    cap = param.lds_max_vertices()
    res = {"device": torch.cuda.get_device_name(0), "unit": "microseconds per solve, median of %d" % args.reps,
           "lds_max_vertices": cap, "auto_max_vertices": param.auto_max_vertices(), "tol": 1e-12, "harmonic": []}
    crossover = 0
    for n in (5, 9, 17, 23, 33, 40, 47, 65, 129):
        v, f = (torch.from_numpy(x).cuda() for x in PC.cap(n))
        V = n * n
        mesh = param._Mesh(v, f)
        w = mesh.weights('cotangent')
        loop = param._disk_loop(mesh.faces, V)
        idx = torch.tensor(loop, device=v.device)
        fixed = torch.zeros(V, dtype=torch.uint8, device=v.device)
        fixed[idx] = 1
        u0 = torch.zeros(V, 2, dtype=torch.float64, device=v.device)
        u0[idx] = param.circle_boundary(v, loop)
        rhs = torch.zeros_like(u0)
        row = {"V": V}
        for route in ("lds", "launch"):
            if route == "lds" and V > cap:
                continue
            call = lambda: param.solve(mesh.nbr, w, fixed, rhs, u0, route=route, tol=1e-12)     # noqa: E731
            row["iterations"] = call()[1]["iterations"]
            row[route + "_us"] = timed(call, args.reps)
            row[route + "_us_per_iteration"] = row[route + "_us"] / max(row["iterations"], 1)
        if "lds_us" in row and row["lds_us"] < row["launch_us"]:
            crossover = V
        print(row, flush=True)
        res["harmonic"].append(row)
    res["largest_V_with_lds_faster"] = crossover
    arap = []
    shirt = param.cut_to_disk(*(torch.from_numpy(x).cuda() for x in PC.shirt()))[:2]
    for name, (v, f) in (("shirt", shirt), ("cap129", tuple(torch.from_numpy(x).cuda() for x in PC.cap(129)))):
        mesh = param._Mesh(v, f)
        mesh.frames()
        row = {"mesh": name, "V": int(v.shape[0]), "F": int(f.shape[0]), "iterations": 20}
        for route in ("lds", "launch"):
            if route == "lds" and v.shape[0] > cap:
                continue
            uv0 = param._harmonic(mesh, 'cotangent', route, 1e-12, None)[0]
            call = lambda: param._arap(mesh, uv0, 20, route, 1e-12)               # noqa: E731
            info = call()[1]
            row["cg_iterations"] = info["cg_iterations"]
            row["energy_first_last"] = [info["energies"][0], info["energies"][-1]]
            row[route + "_wall_ms"] = wall(call, 3)
        print(row, flush=True)
        arap.append(row)
    res["arap_20_iterations_wall_ms_median_of_3"] = arap
    # CG iterations to tol = 1e-12 of the numpy restatement on the CPU, (cotangent, uniform) per test case: the GPU runs the same
    # number by construction (tests/test_gpu_param.py)
    import param_reference as PR
    res["restatement_iterations"] = {name: [PR.solve(*PR.harmonic_system(*make(), wt), tol=1e-12)[1] for wt in ("cotangent", "uniform")]
                                     for name, (make, _) in sorted(PC.DISKS.items())}
    print(res["restatement_iterations"], flush=True)
    with open(args.out, "w") as out:
        json.dump(res, out, indent=1)
        out.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
