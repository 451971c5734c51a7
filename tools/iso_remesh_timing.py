"""Wall time of the iso-remesh kernels against their torch paths: closest point (every vertex of a 40962-vertex mesh onto
an 81920-face reference), tangential relaxation and one Loop level of that mesh, and a whole `isotropic_remesh` (3
iterations, kernel route) of a 40962-vertex icosphere stretched 3x along x.

    python tools/iso_remesh_timing.py [--reps 10]
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
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-torch-closest", action="store_true", help="skip the (slow) torch closest-point path")
    args = ap.parse_args(argv)
    import torch
    from recmv import iso_remesh as IR
    from recmv import nricp as K
    from test_nricp_cpu import icosphere
    dev = "cuda:0"
    torch.manual_seed(0)
    rv, rf = icosphere(6)                                          # reference: 40962 vertices, 81920 faces
    rv, rf = rv.to(dev), rf.to(dev)
    q = (rv * (1 + 0.05 * torch.randn(rv.shape[0], 1, device=dev))).contiguous()    # 40962 query points off the surface
    res = {"query_points": q.shape[0], "reference_faces": rf.shape[0]}
    res["closest_point_kernel_s"] = _time(lambda: IR.closest_point(q, rv, rf), args.reps)
    res["closest_point_tests_per_s"] = q.shape[0] * rf.shape[0] / res["closest_point_kernel_s"]
    if not args.skip_torch_closest:
        res["closest_point_torch_s"] = _time(lambda: IR.closest_point_torch(q, rv, rf), 1)
    edges, _ = K.edges_packed(rf, rv.shape[0])
    nbr = K.neighbours_csr(edges, rv.shape[0])
    n = K.verts_normals(q, rf)
    fixed = torch.rand(rv.shape[0], device=dev) < 0.1
    res["relax_kernel_s"] = _time(lambda: IR.iso_relax(q, n, fixed, nbr), args.reps)
    res["relax_torch_s"] = _time(lambda: IR.iso_relax_torch(q, n, fixed, nbr), args.reps)
    res["loop_kernel_s"] = _time(lambda: IR.loop_subdivide(q, rf, use_kernels=True), args.reps)
    res["loop_torch_s"] = _time(lambda: IR.loop_subdivide(q, rf, use_kernels=False), args.reps)
    sv = (rv * torch.tensor([3., 1., 1.], device=dev)).contiguous()
    for tag in ("warmup", "run"):
        torch.cuda.synchronize()
        t = time.perf_counter()
        v, f, stats = IR.isotropic_remesh(sv, rf, iterations=3, use_kernels=True)
        torch.cuda.synchronize()
        res["remesh_kernel_s"] = time.perf_counter() - t
    res["remesh_stats"] = stats
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
