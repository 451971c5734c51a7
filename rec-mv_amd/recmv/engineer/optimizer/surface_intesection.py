"""engineer/optimizer/surface_intesection.py (reference): `Surface_Intesection`, the ray cast of a template's vertices along
their normals at a target mesh.  The reference builds a pyembree intersector, casts every template vertex along +normal and
-normal (`intersects_location`), concatenates the two result lists and stops at a breakpoint (`pdb.set_trace()`); the
optimisation loop below that breakpoint is unreachable and is NOT ported.  Here the ray cast is finished as a correspondence
query on the project's own segment kernels (recmv.metrics.segment_hits, csrc/segment_mesh.hip): per template vertex the nearer
of the two hits.  Rays are bounded (`max_dist`), where pyembree's are not: a segment query needs an end.
"""
import torch

from ... import metrics, shading
from ...nricp import TriMesh


def _mesh(m, faces=None):
    if faces is not None:
        return m, faces
    if hasattr(m, "verts") and hasattr(m, "faces"):
        return m.verts, m.faces
    verts, faces = m
    return verts, faces


class Surface_Intesection:
    """`__call__(smpl_slice=template, cano_meshes=target)` -> a dict per template vertex: `location` [V,3] f32 (NaN where
    not valid), `face` [V] int64 (-1), `distance` [V] f32 signed along the vertex normal (positive: hit along +normal; NaN)
    and `valid` [V] bool.  Template and target are `TriMesh`es or (verts [V,3] f32, faces [F,3] int64) pairs on one CUDA
    device.  Every vertex casts two segments of length `max_dist`, along +normal and -normal (`shading.verts_normals`, the
    reference's `verts_normals_packed`); the nearer hit wins, +normal on a tie.  `ray_dirs`, `optimizer_setting` and
    `use_normal` are the reference's constructor arguments: with `use_normal=False` every vertex casts along +-`ray_dirs`
    (normalised) instead."""

    def __init__(self, ray_dirs=(0., 0., -1.), optimizer_setting=None, use_normal=True, max_dist=0.1, method='auto'):
        self.name = 'Surface_Intesection'
        self.ray_dirs = tuple(float(x) for x in ray_dirs)
        self.optimizer_setting = optimizer_setting
        self.use_normal = bool(use_normal)
        self.max_dist = float(max_dist)
        self.method = method
        if not (self.max_dist > 0. and self.max_dist < float("inf")):
            raise ValueError("Surface_Intesection: max_dist must be positive and finite, got %r" % (max_dist,))
        if len(self.ray_dirs) != 3 or not any(self.ray_dirs):
            raise ValueError("Surface_Intesection: ray_dirs must be three numbers, not all zero")
        metrics.use_grid_for_segments(method, 0, 0)

    def __call__(self, **inputs):
        return self.fitting(inputs)

    @torch.no_grad()
    def fitting(self, inputs):
        sv, sf = _mesh(inputs['smpl_slice'])
        tv, tf = _mesh(inputs['cano_meshes'])
        sv, sf, tv, tf = sv.contiguous(), sf.contiguous(), tv.contiguous(), tf.contiguous()
        if self.use_normal:
            n = shading.verts_normals(sv, sf)
        else:
            d = torch.tensor(self.ray_dirs, dtype=torch.float32, device=sv.device)
            n = (d / d.norm()).expand_as(sv)
        V = sv.shape[0]
        p = torch.cat([sv, sv])
        q = torch.cat([sv + self.max_dist * n, sv - self.max_dist * n])
        hit = metrics.segment_hits(p, q, tv, tf, method=self.method)
        face, t = hit['face'].view(2, V), hit['t'].view(2, V)
        tt = torch.where(face >= 0, t, torch.full_like(t, float("inf")))
        back = tt[1] < tt[0]                                                      # the -normal hit is strictly nearer
        pick = back.long()[None]
        valid = (face >= 0).any(0)
        f = torch.gather(face, 0, pick)[0]
        tb = torch.gather(t, 0, pick)[0]
        location = torch.gather(hit['point'].view(2, V, 3), 0, pick[..., None].expand(1, V, 3))[0]
        sign = torch.where(back, -1., 1.).to(t.dtype)
        return {'location': location, 'face': f, 'distance': sign * tb * self.max_dist, 'valid': valid}
