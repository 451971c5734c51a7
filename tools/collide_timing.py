"""Time of one pass of the body-collision repair (nearest body triangle + push) per frame, kernel path against the same
search in plain torch, for the registered template size the NR-ICP numbers use (40 962 vertices) against a 6 890-vertex body.

The two paths alternate inside one process after a warm-up of each; every sample is a host clock around work that ends in
a device synchronise.  The operation count of the search is computed from the shapes: every (vertex, triangle) pair costs
POINT_TRIANGLE_FLOP float32 operations in Ericson's test as csrc/closest_tri.h writes it, and the share of the f32 vector
peak is that count over the median kernel time over PEAK_F32_VALU.

    python tools/collide_timing.py [--frames 1] [--reps 20] [--torch-reps 3] [--out profiles/collide_timing.json]
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

# closest_tri.h, counted by hand: ap, bp, cp (9 subtractions), d1..d6 (6 x 5), va, vb, vc (3 x 3), the residual (3 x 4) and its
# square (5), one division and the comparisons of the region tests (~12), the running minimum (2)
POINT_TRIANGLE_FLOP = 9 + 30 + 9 + 12 + 5 + 12 + 2
PEAK_F32_VALU = 157.3e12          # MI355X vector f32 peak (spec: packed FMA, 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz)


def _samples(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from recmv import collide, shading
    from test_nricp_cpu import icosphere
    assert torch.cuda.is_available(), "collide_timing.py measures on the GPU"
    dev = "cuda:0"
    torch.manual_seed(0)
    gv, _ = icosphere(6)                                           # garment: 40962 vertices
    bv, bf = icosphere(5)                                          # body: 10242 vertices, cut down to SMPL's size below
    # SMPL has 6890 vertices and 13776 faces: keep the body's first 13776 faces (the search is a brute force over faces;
    # which surface they form does not change its cost) and every vertex they use
    bf = bf[:13776]
    used, inv = torch.unique(bf.reshape(-1), return_inverse=True)
    bv, bf = bv[used].contiguous(), inv.view(-1, 3).contiguous()
    B = args.frames
    body = (0.5 * bv)[None].repeat(B, 1, 1).to(dev).contiguous()
    garment = (0.5 * gv * (1 + 0.01 * torch.sin(7 * gv[:, :1])))[None].repeat(B, 1, 1).to(dev).contiguous()
    bf = bf.to(dev)
    normals = shading.verts_normals(body, bf)
    N, V, F = garment.shape[1], body.shape[1], bf.shape[0]

    def kernel_nearest():
        return collide.point_mesh_nearest(garment, body, bf)

    face, d_k = kernel_nearest()

    def kernel_pass():
        f, _ = collide.point_mesh_nearest(garment, body, bf)
        collide.collision_push(garment, body, normals, bf, f)

    def torch_nearest():
        return collide.point_mesh_nearest_torch(garment, body, bf)

    # same results first (a faster path that computes something else is not faster)
    f_t, d_t = torch_nearest()
    same_face = float((f_t == face).float().mean())
    max_d = float((d_t - d_k).abs().max())
    for fn in (kernel_nearest, kernel_pass, torch_nearest):       # warm-up of every shape
        fn()
    k_near, k_pass, t_near = [], [], []
    for _ in range(args.torch_reps):                               # alternate the paths
        k_near += _samples(kernel_nearest, max(1, args.reps // args.torch_reps))
        t_near += _samples(torch_nearest, 1)
        k_pass += _samples(kernel_pass, max(1, args.reps // args.torch_reps))
    flop = float(B) * N * F * POINT_TRIANGLE_FLOP
    med = statistics.median
    res = {"frames": B, "garment_vertices": N, "body_vertices": V, "body_faces": F,
           "point_triangle_tests": B * N * F, "flop_per_test": POINT_TRIANGLE_FLOP, "flop": flop,
           "nearest_kernel_s": {"median": med(k_near), "min": min(k_near), "max": max(k_near), "n": len(k_near)},
           "nearest_plus_push_kernel_s": {"median": med(k_pass), "min": min(k_pass), "max": max(k_pass), "n": len(k_pass)},
           "nearest_torch_s": {"median": med(t_near), "min": min(t_near), "max": max(t_near), "n": len(t_near)},
           "torch_over_kernel": med(t_near) / med(k_near),
           "nearest_kernel_flops": flop / med(k_near), "peak_f32_valu_flops": PEAK_F32_VALU,
           "share_of_f32_valu_peak": flop / med(k_near) / PEAK_F32_VALU,
           "same_face_share_torch_vs_kernel": same_face, "max_abs_sqdist_difference_torch_vs_kernel": max_d}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    assert med(k_near) <= med(t_near), "the kernel path must not be slower than the torch baseline"
    return res


if __name__ == "__main__":
    main()
