"""Times of recmv.bake on the GPU -> profiles/bake_timing.json: the UV rasteriser (clear, scatter, resolve), the gutter (4 passes)
and a whole bake() with a 160 k-face source, on 1024^2 and 2048^2 images, for a 5 k-face and a 160 k-face chart (square grids
lifted to a sphere, tests/param_cases.cap, with their planar uv fitted into the image), with 8 and with 64 lanes per face.
Device events around whole calls (the wrappers' allocations included: they are part of what a caller pays), two warm-up calls of
every shape, `--inner` calls per timed window, the median of `--reps` windows with their minimum and maximum; the whole bake is
a host clock around a call that ends in a synchronise (it reads its report back), the source's grid built inside it.  Both
lane counts are checked to give the same images before they are timed.  The default lanes rule of recmv.bake (by the mean area
of a face's texel box, LANES_SWITCH_AREA) is read off these rows.

    python tools/bake_timing.py [--reps 7] [--inner 10] [--out profiles/bake_timing.json]
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


def timed(call, reps, inner):
    call()                                                 # warm-up (the library's load, the allocator, the code objects)
    call()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / inner)
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def wall(call, reps):
    call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=osp.join(REPO, "profiles", "bake_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bake_timing.py needs a GPU")
    import param_cases as PC
    from recmv import bake, metrics
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner,
           "unit": "microseconds per call (raster, gutter), milliseconds per call (bake)", "lanes_switch_area": bake.LANES_SWITCH_AREA,
           "rows": []}
    sv, sf = (torch.from_numpy(x).cuda() for x in PC.cap(284))                      # the source: 160 178 faces
    grid_build = wall(lambda: metrics.MeshGrid(sv, sf), 3)
    res["source"] = {"faces": int(sf.shape[0]), "mesh_grid_build_ms": grid_build}
    for n in (51, 284):                                                             # 5 000 and 160 178 faces
        v, f = (torch.from_numpy(x).cuda() for x in PC.cap(n))
        flat = v[:, :2].double().contiguous()
        for size in (1024, 2048):
            uv = bake.fit_uv(flat, size, 4.)
            c = uv[f]
            ext = c.amax(1) - c.amin(1)
            row = {"faces": int(f.shape[0]), "size": size, "default_lanes": bake.default_lanes(uv, f, size),
                   "mean_box_texels": float(((ext[:, 0] * size + 1.) * (ext[:, 1] * size + 1.)).mean().item())}
            images = {lanes: bake.rasterize_uv(uv, f, size, lanes=lanes) for lanes in bake.LANES}
            assert all(torch.equal(a, b) for a, b in zip(images[8], images[64])), "the lane count changed a bit"
            face = images[8][0]
            row["covered_texels"] = int((face >= 0).sum().item())
            for lanes in bake.LANES:
                row["raster_us_lanes%d" % lanes] = timed(lambda: bake.rasterize_uv(uv, f, size, lanes=lanes), args.reps, args.inner)
            row["gutter4_us"] = timed(lambda: bake.gutter(face, 4), args.reps, args.inner)
            for lanes in bake.LANES:
                call = lambda: bake.bake(v, f, uv, size, source=(sv, sf), gutter=4, fit=False, lanes=lanes)     # noqa: E731
                row["bake_ms_lanes%d" % lanes] = wall(call, 3)
            print(row, flush=True)
            res["rows"].append(row)
    with open(args.out, "w") as out:
        json.dump(res, out, indent=1)
        out.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
