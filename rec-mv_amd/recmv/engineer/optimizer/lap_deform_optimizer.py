"""Laplacian deformation of a garment template onto its feature curves (engineer/optimizer/lap_deform_optimizer.py:25-190 of
the reference): `Laplacian_Optimizer` with the reference's constructor arguments and `__call__(**inputs)` contract.

Every epoch, for each source mesh: match its boundary fields to the curves (recmv.lap_align.best_match), solve
argmin_u |L u - L v|^2 + w |C u - t|^2, replace every vertex by the mean of its neighbours (`smooth`), and write u back as
the mesh's vertices; the next epoch matches again from there.  Two paths compute the same minimiser:
  * kernels (default on the GPU): recmv_lap_align_solve (Jacobi-CG in f64) and recmv_lap_smooth;
  * torch (`use_kernels=False`, and always on the CPU): a dense f64 solve of the normal equations (up to
    recmv.lap_align.DENSE_MAX_V vertices).
The fields of a plain template are its boundary loops, assigned to the feature lines once, by centroid
(recmv.lap_align.assign_loops).  `dense_boundary` and the static points of the reference's SMPL-cut templates are not used.
"""
import torch

from ... import lap_align as LA
from ...utils.constant import GARMENT_FL_MATCH


def _points(t):
    t = getattr(t, 'verts', t)
    return torch.as_tensor(t).detach().reshape(-1, 3)


class Laplacian_Optimizer:
    """Laplacian alignment of garment templates to feature curves.  `__call__(source_fl_meshes=[mesh], target_meshes=[curve],
    source_type=[garment], target_fl_type=[fl_name], outlayer=True)` -> `inputs`, the meshes' `verts` replaced in place.
    Meshes are objects with `verts` [V,3] f32 and `faces` [F,3] (recmv.nricp.TriMesh); curves are [S,3] tensors (or objects
    with `verts`)."""

    def __init__(self, epoch=3, constrain_weight=1., optimizer_setting=None, smooth=True, use_kernels=True, log=print,
                 tol=LA.TOL, max_iter=LA.MAX_ITER):
        self.name = "Laplacian_Deform_Optimzier"
        self.optimizer_setting = optimizer_setting
        self.epoch = epoch
        self.constrain_weights = float(constrain_weight)
        self.smooth = smooth
        self.use_kernels = bool(use_kernels)
        self.log = log
        self.tol = tol
        self.max_iter = max_iter
        self.history = []        # per mesh and epoch: dict(garment, epoch, pairs, iters, residual, before, after)
        if not self.constrain_weights > 0.:
            raise ValueError("Laplacian_Optimizer: constrain_weight must be positive, got %r" % constrain_weight)

    def __call__(self, **inputs):
        return self.fitting(inputs)

    @torch.no_grad()
    def fitting(self, inputs):
        meshes = inputs['source_fl_meshes']
        types = inputs['source_type']
        curves = {name: _points(c) for c, name in zip(inputs['target_meshes'], inputs['target_fl_type'])}
        if len(types) != len(meshes):
            raise ValueError("Laplacian_Optimizer: one source_type per source mesh")
        self.history = []
        for mesh, garment in zip(meshes, types):
            self._fit_one(mesh, garment, curves)
        return inputs

    def _fit_one(self, mesh, garment, curves):
        verts = mesh.verts.detach().float().contiguous()
        V = verts.shape[0]
        kernels = self.use_kernels and verts.is_cuda
        topo = LA.Topology(mesh.faces, V, verts.device)
        loops = LA.boundary_loops(mesh.faces, V)
        fields = GARMENT_FL_MATCH[garment]
        field_loops = LA.assign_loops(loops, verts, curves, fields, log=self.log, garment=garment)
        if not field_loops:
            raise ValueError("Laplacian_Optimizer: nothing to constrain for %s (%d boundary loop(s), curves for %s)"
                             % (garment, len(loops), ", ".join(f for f in fields if f in curves) or "none of its fields"))
        for epoch in range(self.epoch):
            idx, tgt, counts = LA.match(verts, loops, field_loops, curves)
            if idx.numel() == 0:
                raise ValueError("Laplacian_Optimizer: no boundary vertex of %s passed the direction filter" % garment)
            cw, cwt = LA.constraint_weights(idx, tgt, V, self.constrain_weights)
            before = LA.boundary_distance(verts, loops, field_loops, curves)
            if kernels:
                u, iters, res = LA.solve(topo, verts, cw, cwt, tol=self.tol, max_iter=self.max_iter)
                u = LA.smooth(topo, u) if self.smooth else u
            else:
                u, iters, res = LA.solve_torch(topo, verts, cw, cwt), 0, None
                u = LA.smooth_torch(topo, u) if self.smooth else u
            if not torch.isfinite(u).all():
                raise FloatingPointError("Laplacian_Optimizer: non-finite vertices after the solve (%s)" % garment)
            verts = u.contiguous()
            after = LA.boundary_distance(verts, loops, field_loops, curves)
            self.history.append(dict(garment=garment, epoch=epoch, pairs=counts, iters=iters, residual=res,
                                     before=before, after=after))
            solve = ("CG %d iterations, residual %.2e" % (iters, max(res))) if res is not None else "dense f64 solve"
            self.log("Laplacian align %s epoch %d/%d: pairs %s; %s; boundary-to-curve %.5f -> %.5f"
                     % (garment, epoch + 1, self.epoch, " ".join("%s=%d" % kv for kv in counts.items()), solve, before,
                        after))
        mesh.verts = verts.to(mesh.verts.dtype)
