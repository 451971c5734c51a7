"""Body-collision repair of posed garment meshes (csrc/mesh_collide.hip) — an ADDITION to the reference.

A garment animated on a pose the capture never saw is skinned with an offset field averaged over the capture, so some of
its vertices sink into the body.  The reference stops at a ray cast (engineer/optimizer/surface_intesection.py); here every
frame is repaired geometrically: for each garment vertex the exact nearest point q of the posed body mesh, the body normal
n interpolated there and the signed distance s = (p - q) . n, and a vertex with s < eps is pushed out to s = eps along n.

  point_mesh_nearest   recmv_point_mesh_nearest: nearest body triangle and squared distance of every vertex of every frame
  collision_push       recmv_collision_push: the push and the per-frame counts
  resolve              `iters` passes of the two (a push can change which face is nearest)
  intersection_report  what the repair leaves: per frame the garment FACES that still cut through the body, through the
                       garment itself and through another garment (recmv.metrics, csrc/mesh_intersect.hip), optionally the
                       garment VERTICES inside the body and their depth (csrc/segment_mesh.hip); detection only
  point_mesh_nearest_torch   the same search in plain torch (chunked point-triangle distances + argmin), the baseline of
                       tools/collide_timing.py

Opt-in (infer_fl_animation.py --fix-collisions); off by default, so the reference's output is what the command writes.
"""
import torch

from . import _lib as L
from . import shading

# User parameters in the capture's length unit (metres for SMPL captures), not measured quantities:
COLLISION_EPS = 2e-3           # the margin kept between cloth and body: the 2 mm collision threshold SNUG trains with
COLLISION_MAX_DEPTH = 3e-2     # a choice: a vertex deeper than 3 cm is nearer the far side of a thin limb than the side it
#                                entered through, and pushing it to the nearest surface would tear the cloth — it is left
#                                where it is and reported as unresolved
COLLISION_ITERS = 3


def _check(p, verts, faces):
    for t, name in ((p, "p"), (verts, "verts")):
        L.require_cuda(t, name)
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("%s must be float32 of shape [B,n,3]" % name)
    L.require_cuda(faces, "faces")
    if faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be int64 of shape [F,3]")
    if p.shape[0] != verts.shape[0]:
        raise ValueError("p and verts must have the same number of frames (got %d and %d)" % (p.shape[0], verts.shape[0]))
    if verts.shape[1] == 0 or faces.shape[0] == 0:
        raise ValueError("the body mesh is empty")
    if p.shape[0] > 65535:
        raise ValueError("at most 65535 frames per call")


def point_mesh_nearest(p, verts, faces):
    """Exact nearest triangle of frame b's mesh (verts [B,V,3] f32, one face table faces [F,3] int64, CUDA) to every point
    p [B,N,3] f32: (face [B,N] int64, squared distance [B,N] f32); ties go to the lowest face id."""
    _check(p, verts, faces)
    p, verts, faces = p.contiguous(), verts.contiguous(), faces.contiguous()
    B, N, dev = p.shape[0], p.shape[1], p.device
    face = L.scratch((B, N), torch.int64, dev)
    sqdist = L.scratch((B, N), torch.float32, dev)
    if B == 0 or N == 0:
        return face, sqdist
    ws = L.workspace(nbytes := int(L.lib().recmv_point_mesh_nearest_workspace_bytes(B, N)), dev, "point_mesh_nearest_workspace_bytes")
    L.launch("point_mesh_nearest", dev, L.ptr(p), L.ptr(verts), L.ptr(faces), B, N, verts.shape[1], faces.shape[0], L.ptr(face),
             L.ptr(sqdist), L.ptr(ws), nbytes)
    return face, sqdist


def collision_push(p, verts, vnormals, faces, face, eps=COLLISION_EPS, max_depth=COLLISION_MAX_DEPTH):
    """One push: (p_out [B,N,3], moved [B] int32, unresolved [B] int32) on the device.  With q the closest point of p on
    triangle `face` [B,N] (point_mesh_nearest), n the unit normal interpolated there from vnormals [B,V,3] and
    s = (p - q) . n: s >= eps copies the vertex bit for bit, -max_depth <= s < eps moves it to p + (eps - s) n,
    s < -max_depth copies it and counts it as unresolved."""
    _check(p, verts, faces)
    L.require_cuda(vnormals, "vnormals")
    L.require_cuda(face, "face")
    if vnormals.shape != verts.shape or vnormals.dtype != torch.float32:
        raise ValueError("vnormals must be float32 of the shape of verts")
    if face.dtype != torch.int64 or tuple(face.shape) != tuple(p.shape[:2]):
        raise ValueError("face must be int64 of shape [B,N]")
    if not (eps >= 0 and max_depth >= 0):
        raise ValueError("eps and max_depth must not be negative")
    p, verts, vnormals, faces, face = (t.contiguous() for t in (p, verts, vnormals, faces, face))
    B, N = p.shape[0], p.shape[1]
    out = L.scratch_like(p)
    moved = torch.zeros(B, dtype=torch.int32, device=p.device)
    unresolved = torch.zeros(B, dtype=torch.int32, device=p.device)
    if B == 0:
        return out, moved, unresolved
    L.launch("collision_push", p.device, L.ptr(p), L.ptr(verts), L.ptr(vnormals), L.ptr(faces), L.ptr(face), B, N, verts.shape[1],
             faces.shape[0], float(eps), float(max_depth), L.ptr(out), L.ptr(moved), L.ptr(unresolved))
    return out, moved, unresolved


@torch.no_grad()
def resolve(garment_vs, body_vs, body_fs, eps=COLLISION_EPS, max_depth=COLLISION_MAX_DEPTH, iters=COLLISION_ITERS):
    """Push the garment vertices garment_vs [B,N,3] out of the posed body (body_vs [B,V,3], body_fs [F,3] int64, any closed
    mesh): up to `iters` passes of nearest face + push, stopping after a pass that moves nothing.  Returns (vs [B,N,3],
    stats) with stats = {'moved': [B] vertices whose position changed, 'unresolved': [B] vertices deeper than `max_depth`
    in the last pass, 'passes': passes run, 'moved_per_pass': [[B], ...]} (python ints).  The input is not modified."""
    _check(garment_vs, body_vs, body_fs)
    if iters < 1:
        raise ValueError("resolve: iters must be at least 1")
    body_vs, body_fs = body_vs.contiguous(), body_fs.contiguous()
    B = garment_vs.shape[0]
    normals = shading.verts_normals(body_vs, body_fs) if B else body_vs
    vs = garment_vs.contiguous()
    per_pass, unresolved = [], [0] * B
    for _ in range(iters):
        face, _ = point_mesh_nearest(vs, body_vs, body_fs)
        vs, moved, unres = collision_push(vs, body_vs, normals, body_fs, face, eps, max_depth)
        per_pass.append(moved.cpu().tolist())                      # (one small copy per pass: the early stop needs it)
        unresolved = unres.cpu().tolist()
        if not any(per_pass[-1]):
            break
    changed = (vs != garment_vs).any(-1).sum(1).cpu().tolist() if B else []
    return vs, {'moved': changed, 'unresolved': unresolved, 'passes': len(per_pass), 'moved_per_pass': per_pass}


@torch.no_grad()
def intersection_report(garments, body_vs, body_fs, method='auto', penetration=False):
    """Crossing faces of posed garments, frame by frame.  `garments` maps a name to (vs [B,N,3] f32, faces [F,3] int64), the
    body is body_vs [B,V,3] f32 / body_fs [F,3] int64 (CUDA, one device, the same B).  Returns a list of B dicts:
    {name: {'body_faces': garment faces that cross a body face, 'self_faces': garment faces in a crossing pair of the
    garment with itself, 'faces': the garment's face count}, ..., 'between': {'<a>|<b>': {'faces_a', 'faces_b'}}} with one
    entry of 'between' per pair of garments (in the order given).  Crossing as in INTEGRATION.md §5 (strict: touching is
    none); a garment without faces reports zeros.  The vertex repair above judges vertices; this judges faces.
    `penetration`: every garment entry also gets 'inside_vertices', the garment vertices inside the (closed) body by
    metrics.points_inside — also those of a patch that lies wholly inside, where no face crosses — and 'max_depth', the
    largest distance of such a vertex to the body's surface (0. when there is none)."""
    from . import metrics
    names = list(garments)
    B = body_vs.shape[0]
    for name in names:
        vs, fs = garments[name]
        _check(vs, body_vs, body_fs)
    report = []
    for b in range(B):
        frame, between = {}, {}
        for name in names:
            vs, fs = garments[name]
            if fs.shape[0] == 0 or vs.shape[1] == 0:
                frame[name] = {'body_faces': 0, 'self_faces': 0, 'faces': int(fs.shape[0])}
                if penetration:
                    frame[name].update(_penetration_entry(vs[b], body_vs[b], body_fs, method))
                continue
            body = metrics.mesh_intersections(vs[b], fs, body_vs[b], body_fs, method=method)
            own = metrics.self_intersections(vs[b], fs, method=method)
            frame[name] = {'body_faces': int(body['faces_a'].shape[0]), 'self_faces': int(own['faces'].shape[0]),
                           'faces': int(fs.shape[0])}
            if penetration:
                frame[name].update(_penetration_entry(vs[b], body_vs[b], body_fs, method))
        for x, a in enumerate(names):
            for c in names[x + 1:]:
                (va, fa), (vc, fc) = garments[a], garments[c]
                if min(fa.shape[0], fc.shape[0], va.shape[1], vc.shape[1]) == 0:
                    between['%s|%s' % (a, c)] = {'faces_a': 0, 'faces_b': 0}
                    continue
                m = metrics.mesh_intersections(va[b], fa, vc[b], fc, method=method)
                between['%s|%s' % (a, c)] = {'faces_a': int(m['faces_a'].shape[0]), 'faces_b': int(m['faces_b'].shape[0])}
        frame['between'] = between
        report.append(frame)
    return report


def _penetration_entry(vs, body_v, body_fs, method):
    from . import metrics
    if vs.shape[0] == 0:
        return {'inside_vertices': 0, 'max_depth': 0.}
    m = metrics.penetration(vs.contiguous(), body_v, body_fs, method=method)
    return {'inside_vertices': m['count'], 'max_depth': m['max_depth']}


def point_mesh_nearest_torch(p, verts, faces, chunk_elems=1 << 22):
    """point_mesh_nearest in plain torch, frame by frame (iso_remesh.closest_point_torch: row chunks of a brute force, the
    first minimum kept)."""
    from .iso_remesh import closest_point_torch
    face, sqdist = [], []
    for b in range(p.shape[0]):
        f, _, d = closest_point_torch(p[b], verts[b], faces, chunk_elems)
        face.append(f)
        sqdist.append(d)
    if not face:
        return p.new_zeros(0, p.shape[1], dtype=torch.int64), p.new_zeros(0, p.shape[1])
    return torch.stack(face), torch.stack(sqdist)
