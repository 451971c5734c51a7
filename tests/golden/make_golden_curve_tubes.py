"""Golden vectors for the feature-curve tubes, from the REAL reference classes imported from /root/reference:

  curve_tubes.npz
    tube_*    engineer/utils/garment_structure.py `Intersect_Free_Curve.curve_to_mesh()` (:214-274) on seeded closed curves
              (L=4, S=24; non-trivial scale / nx_scale, some scales negative), num_joints 6 and 4.  `Meshes` is a plain
              holder (pytorch3d is absent).
    fl_*      engineer/networks/OptimGarmentNetwork.py `infer_garment_fl` (:2861-2935) on a stand-in self: reference
              deformer and skinner of common_setup, 2 frames, garment short_sleeve_upper; `trimesh.Trimesh` is a holder
              that keeps its arguments, `Tensor.cuda` the identity.
    fit_*     the fit branch of `curve_to_mesh` (:179-212) for K=200 of its 20000 iterations (the module gets its own
              `range`, which caps the single-argument call), S=40, M=64 target points per pair, 2 pairs.  pytorch3d's
              `chamfer_distance` — absent here — is a restatement of its documented default (mean over the points of each
              side, both sides added), so the chamfer arithmetic itself stays parity-unpinned, as in curves.npz.  Stored:
              the inputs, the curves after K steps, every pair's loss at steps 0 and K-1 (recomputed in float64 from the
              curves the reference handed to chamfer_distance in those steps), and the reference's spread against itself:
              the same run with the target points of every pair permuted, which changes only summation order, and the
              largest per-point distance between the two results (`fit_spread`).

    python tests/golden/make_golden_curve_tubes.py
"""
import contextlib
import io
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path[:0] = [str(REPO / "rec-mv_amd"), str(REPO)]
import ref_loader  # noqa: E402

ref_loader.install()
import common_setup as cs  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_curves import rings  # noqa: E402

K_FIT = 200
RATIO = {"sdfRatio": 0.8, "deformerRatio": 0.7, "renderRatio": 1.0}
NAMES = ['neck', 'left_cuff', 'right_cuff', 'upper_bottom']          # FL_EXTRACT['short_sleeve_upper']


class Meshes:
    """Stand-in for pytorch3d's Meshes([verts], [faces]): the three methods the reference calls on a curve mesh."""

    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces

    def verts_packed(self):
        return self.verts[0]

    def faces_packed(self):
        return self.faces[0]

    def clone(self):
        return Meshes([v.clone() for v in self.verts], [f.clone() for f in self.faces])


class Trimesh:
    def __init__(self, vertices, faces, process=True):
        self.vertices, self.faces = vertices, faces


def build_curve(G, curves, scale_seed):
    ref = object.__new__(G.Intersect_Free_Curve)
    torch.nn.Module.__init__(ref)
    ref.cano2canosmpl = lambda lst, nm: [0.9 * c for c in lst]
    ref.fl_names, ref.sample_num = list(NAMES), curves[0].shape[0]
    ref.initialize_parameters([c.clone() for c in curves])
    g = torch.Generator().manual_seed(scale_seed)
    with torch.no_grad():
        ref.scale.copy_(1.0 + 0.2 * torch.randn(ref.scale.shape, generator=g))
        ref.nx_scale.copy_(0.03 * torch.randn(ref.nx_scale.shape, generator=g))
    return ref


def chamfer_distance(x, y):
    """pytorch3d.loss.chamfer_distance(x, y) with its defaults, for one pair of clouds [1,n,3], [1,m,3]."""
    d = ((x[0, :, None, :] - y[0, None, :, :]) ** 2).sum(-1)
    return d.min(dim=1).values.mean() + d.min(dim=0).values.mean(), None


def fit_loss64(x, y):
    """The fit objective of one pair (garment_structure.py:198-208) in float64, on the curve x [S,3] and the polyline y."""
    import torch.nn.functional as F
    x, y = x.double(), y.double()
    cham = chamfer_distance(x[None], y[None])[0]
    diff_a = torch.cat([x[:-1] - x[1:], x[-1:] - x[0:1]], dim=0)
    diff_a = diff_a / (diff_a.norm(dim=-1, keepdim=True) + 1e-6)
    return 1000 * cham + 0.1 * (1 - F.cosine_similarity(diff_a[:-1], diff_a[1:], dim=-1)).sum()


def run_fit(G, curves, targets, curve_idx, target_idx, scale, nx_scale):
    """K_FIT iterations of the reference's fit: (curves after the fit [L,S,3], loss of every pair at step 0 and K-1)."""
    ref = build_curve(G, curves, 0)
    with torch.no_grad():
        ref.scale.copy_(scale)
        ref.nx_scale.copy_(nx_scale)
    seen = []

    def chamfer(x, y):
        seen.append((x[0].detach().clone(), y[0].detach().clone()))
        return chamfer_distance(x, y)

    real_range = range
    G.range = lambda *a: real_range(min(a[0], K_FIT)) if len(a) == 1 else real_range(*a)
    G.chamfer_distance = chamfer
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ref.curve_to_mesh(curve_verts=[t.numpy() for t in targets], curve_idx=curve_idx, target_idx=target_idx)
    finally:
        torch.Tensor.cuda = real_cuda
        del G.range
    P = len(curve_idx)
    assert len(seen) == K_FIT * P
    first = torch.stack([fit_loss64(*seen[p]) for p in range(P)])
    last = torch.stack([fit_loss64(*seen[(K_FIT - 1) * P + p]) for p in range(P)])
    return ref.inference().detach(), first, last


def main():
    torch.set_num_threads(1)
    ref_loader.ref_module("model.network")       # the reference's own entry order (its packages import each other)
    G = ref_loader.ref_module("engineer.utils.garment_structure")
    Dref = ref_loader.ref_module("model.Deformer")
    OGN = ref_loader.ref_module("engineer.networks.OptimGarmentNetwork")
    G.Meshes = Meshes
    out = {}
    # ---- curve_to_mesh
    curves = rings(21, n_lines=4, n=24)
    ref = build_curve(G, curves, 22)
    with torch.no_grad():
        ref.scale[1, 3:8] = -0.3                                      # the ReLU path
    out.update(tube_curves=torch.stack(curves), tube_scale=ref.scale, tube_nx_scale=ref.nx_scale, tube_nx=ref.cano_nx,
               tube_pts=ref.inference())
    for J in (6, 4):
        meshes = ref.curve_to_mesh(num_joints=J)
        out["tube_verts_j%d" % J] = torch.stack([m.verts_packed() for m in meshes])
        out["tube_faces_j%d" % J] = torch.stack([m.faces_packed() for m in meshes])
    # ---- infer_garment_fl
    OGN.trimesh = types.SimpleNamespace(Trimesh=Trimesh)
    fl_curves = [0.8 * c for c in rings(23, n_lines=4, n=24)]          # inside the skinning volume of common_setup
    fl_ref = build_curve(G, fl_curves, 24)
    tr = cs.build_translator(Dref.MLPTranslator)
    sk = cs.build_skinner(Dref.LBSkinner, Dref.batch_rodrigues)
    comp = Dref.CompositeDeformer([tr, sk])
    N = 2
    conds, _ = cs.conds_and_inds(8, nframes=N, condlen=128, seed=31)
    poses, trans = cs.poses_trans(N, seed=32)
    conds, poses, trans = conds.detach(), poses.detach(), trans.detach()
    fake = types.SimpleNamespace(inter_free_curve=fl_ref, fl_names=list(NAMES), garment_names=['short_sleeve_upper'],
                                 deformer=comp, get_grad_parameters=lambda fids, dev: ([None, conds], poses, trans, None))
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        mesh = OGN.OptimGarmentNetwork.infer_garment_fl(fake, [torch.zeros(1, 3)], [None], 64, 64, RATIO, torch.arange(N))
    finally:
        torch.Tensor.cuda = real_cuda
    out.update(fl_curves=torch.stack(fl_curves), fl_scale=fl_ref.scale, fl_nx_scale=fl_ref.nx_scale, fl_conds=conds,
               fl_poses=poses, fl_trans=trans, fl_verts=mesh.vertices, fl_faces=mesh.faces)
    # ---- the fit branch
    S, M = 40, 64
    fit_curves = rings(25, n_lines=4, n=S)
    curve_idx, target_idx = [0, 1], [3, 1]
    g = torch.Generator().manual_seed(26)
    scale = 1.0 + 0.1 * torch.randn(4, S, 1, generator=g)
    nx_scale = 0.01 * torch.randn(4, S, 1, generator=g)
    # the fit doubles init_scale and starts from the mean scale: polylines near 1.9 x the curve, with their own sampling
    targets = []
    for t_i in target_idx:
        c = fit_curves[t_i]
        centre = c.mean(0, keepdim=True)
        t = torch.linspace(0, 1, M + 1)[:-1] * S
        i0 = t.floor().long() % S
        w = (t - t.floor())[:, None]
        poly = (1 - w) * c[i0] + w * c[(i0 + 1) % S]
        targets.append((centre + 1.9 * (poly - centre) + 0.004 * torch.randn(M, 3, generator=g)).float())
    fitted, first, last = run_fit(G, fit_curves, targets, curve_idx, target_idx, scale, nx_scale)
    perm = [torch.randperm(M, generator=g) for _ in targets]
    fitted_p, first_p, last_p = run_fit(G, fit_curves, [t[p] for t, p in zip(targets, perm)], curve_idx, target_idx, scale,
                                        nx_scale)
    spread = (fitted - fitted_p).norm(dim=-1).max()
    print("fit: loss %s -> %s, spread against the permuted run %.3e" % (first.tolist(), last.tolist(), float(spread)))
    assert (last < first).all()
    out.update(fit_curves=torch.stack(fit_curves), fit_scale=scale, fit_nx_scale=nx_scale, fit_targets=torch.stack(targets),
               fit_curve_idx=np.array(curve_idx), fit_target_idx=np.array(target_idx), fit_iters=np.array(K_FIT),
               fit_result=fitted, fit_result_permuted=fitted_p, fit_first_loss=first, fit_last_loss=last,
               fit_spread=spread)
    save("curve_tubes", **out)


if __name__ == "__main__":
    main()
