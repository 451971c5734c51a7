"""Wall time of one NR-ICP registration step, kernel path against torch path: knn (one epoch's search), energy (one inner
iteration: forward + gradient; + the AdamW step) and a whole shortened fit, for a 5e4-vertex template and a 1.5e5-vertex target.

    python tools/nricp_timing.py [--epochs 3] [--reps 20]
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
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from recmv import nricp as K
    from recmv.engineer.optimizer import NRICP_Optimizer_AdamW, TriMesh
    from test_nricp_cpu import icosphere
    dev = "cuda:0"
    torch.manual_seed(0)
    tv, tf = icosphere(6)                                          # template: 40962 vertices
    tv, tf = tv.to(dev), tf.to(dev)
    gv, gf = K.densify(tv, tf, 150000)                             # target: 163842 vertices
    gv = gv * 1.05 + 0.01 * torch.stack([torch.sin(3 * gv[:, 1]), torch.cos(2 * gv[:, 0]), torch.sin(4 * gv[:, 2])], -1)
    N, M = tv.shape[0], gv.shape[0]
    res = {"template_vertices": N, "target_vertices": M}
    res["knn_kernel_s"] = _time(lambda: K.knn1(tv, gv), args.reps)
    res["knn_torch_s"] = _time(lambda: K.knn1_torch(tv, gv), max(1, args.reps // 10))
    # one inner iteration at maps near identity
    topo = K.EnergyTopology(tf, N, dev)
    A = (torch.eye(3, device=dev) + 0.01 * torch.randn(N, 3, 3, device=dev)).contiguous()
    b = (0.01 * torch.randn(N, 3, device=dev)).contiguous()
    idx, _ = K.knn1(tv, gv)
    gn = K.verts_normals(gv, gf)
    c, nc = gv[idx].contiguous(), gn[idx].contiguous()
    nx = K.verts_normals(tv, tf).contiguous()
    en = K.NricpEnergy(topo, dev)
    res["energy_kernel_s"] = _time(lambda: en(A, b, tv, c, nc, nx, 1., 50., 250., 0.3), args.reps)
    from recmv.engineer.optimizer.nricp_optimizer import Local_Affine
    la = Local_Affine(N, 1, topo.edges).to(dev)

    def torch_iter():
        v, st = la(tv[None], return_stiff=True)
        with torch.no_grad():
            wn, ok = la.forward_normal(nx[None])
            mask = ok & topo.interior[None] & (F.cosine_similarity(nc[None], wn, dim=2) > 0.3)
        loss = torch.sqrt(torch.sum(mask[..., None] * (v - c[None]) ** 2) + torch.sum(st) * 50.) + \
            K.laplacian_smoothing_torch(v[0], topo.edges) * 250.
        la.zero_grad()
        loss.backward()
    res["energy_torch_s"] = _time(torch_iter, args.reps)
    for path, use, epochs in (("kernel", True, 1), ("torch", False, 1), ("kernel", True, args.epochs),
                              ("torch", False, args.epochs)):          # the 1-epoch fits warm up both paths
        opt = NRICP_Optimizer_AdamW(epoch=epochs, dense_pcl=0, use_normal=True, stiffness_weight=[50, 20], mile_stone=[2],
                                    inner_iter=50, laplacian_weight=[250, 250], threshold=0.3, device=dev, use_kernels=use,
                                    log=None)
        torch.cuda.synchronize()
        t = time.perf_counter()
        opt(smpl_slice=TriMesh(tv, tf), cano_meshes=TriMesh(gv, gf), save_path=None, garment_name='g', static_pts_type=[],
            nricp_masks=None)
        torch.cuda.synchronize()
        res["fit_%s_s" % path] = time.perf_counter() - t
    t = time.perf_counter()
    K.EnergyTopology(tf, N, dev)
    torch.cuda.synchronize()
    res["topology_s"] = time.perf_counter() - t
    res["fit_inner_iterations"] = 100 + 50 * (args.epochs - 1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
