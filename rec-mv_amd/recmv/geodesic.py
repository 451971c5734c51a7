"""Geodesic distance fields on a triangle mesh (csrc/geodesic.hip) — an ADDITION to the reference: distance ALONG the surface,
where every other distance of the mesh toolkit is Euclidean or a hop count.

  distance           D [V] (or [B, V]) float64 from source vertices: the fixed point of the first-order Hopf-Lax update on the
                     triangles, reached by Jacobi sweeps from above.  route='sweeps' (a launch per sweep, any size), 'lds' (one
                     workgroup per field, up to lds_max_vertices() vertices) or 'auto'
  boundary_distance  the distance to the mesh's border, or one field per boundary loop
  nearest_source     the minimum over fields and which field attains it
  interpolate        a field at points that lie on given faces
  farthest_points    evenly spread landmarks by farthest-point sampling

The definition (the update, the order of its operations, unusable faces, the sweep count K) is that of include/recmv_hip.h and
INTEGRATION.md §5: both routes give the same bits and the same K, whatever the cadence of the convergence check.  First order:
on a flat grid the field errs by a few per cent next to the source.
"""
import torch

from . import _lib as L
from . import connectivity
from .mesh_args import check_mesh

ROUTES = ('auto', 'sweeps', 'lds')
DEFAULT_CHECK_EVERY = 32         # sweeps between two read-backs of last_changed on the sweeps route


def lds_max_vertices():
    """recmv_geodesic_lds_max_vertices(): the most vertices route='lds' takes."""
    return int(L.lib().recmv_geodesic_lds_max_vertices())


def auto_max_vertices():
    """recmv_geodesic_auto_max_vertices(): route='auto' takes the lds route up to this many vertices (measured)."""
    return int(L.lib().recmv_geodesic_auto_max_vertices())


class _Mesh:
    """The tables a solve reads, built once per mesh: contiguous verts and faces and the vertex -> corner-slot CSR of
    connectivity.vertex_slots_csr.  Corners outside [0, V) are filed under a row of their own, V, which no vertex reads."""

    def __init__(self, verts, faces):
        self.verts, self.faces = check_mesh(verts, faces)
        self.V, self.F, self.device = verts.shape[0], faces.shape[0], verts.device
        self.off, self.slots = connectivity.filed_slots_csr(self.faces, self.V)

    def args(self):
        return (L.ptr(self.verts), self.V, L.ptr(self.faces), self.F, L.ptr(self.off), L.ptr(self.slots))


def _host_sources(V, sources, values):
    """The sources of B fields as flat host tensors (index b * V + vertex, value), validated by the library on the host: the
    argument errors come before any device work."""
    lib = L.lib()
    B = len(sources)
    if values is None:
        values = [None] * B
    if not isinstance(values, (list, tuple)) or len(values) != B:
        raise ValueError("values must match sources: one tensor per field")
    idx, val = [torch.zeros(0, dtype=torch.int64)], [torch.zeros(0, dtype=torch.float64)]
    for b, (s, x) in enumerate(zip(sources, values)):
        s = torch.as_tensor(s)
        if s.dtype != torch.int64 or s.dim() != 1:
            raise ValueError("sources must be int64 of shape [S]")
        s = s.detach().cpu().contiguous()
        if x is None:
            x = torch.zeros(s.shape[0], dtype=torch.float64)
        else:
            x = torch.as_tensor(x)
            if not x.dtype.is_floating_point or x.shape != s.shape:
                raise ValueError("values must be floating point of the sources' shape")
            x = x.detach().cpu().to(torch.float64).contiguous()
        if lib.recmv_geodesic_check_sources(L.ptr(s), L.ptr(x), s.shape[0], V) != L.RECMV_OK:
            raise ValueError(lib.recmv_last_error().decode())
        idx.append(s + b * V)
        val.append(x)
    return torch.cat(idx), torch.cat(val)


def _initial(V, B, idx, val, device):
    """D^0 [B, V] float64: +inf except at the sources; of duplicate sources the least value holds."""
    D0 = torch.full((B, V), float("inf"), dtype=torch.float64, device=device)
    if idx.shape[0]:
        D0.view(-1).scatter_reduce_(0, idx.to(device), val.to(device), "amin")
    return D0


def _solve(mesh, D0, route, max_sweeps, check_every):
    """(D [B, V], sweeps [B] int64 on the host) of the initial fields D0 on one route."""
    B, V, dev = D0.shape[0], mesh.V, mesh.device
    if V == 0 or B == 0:
        return D0, torch.zeros(B, dtype=torch.int64)
    if route == 'lds':
        D = L.scratch((B, V), torch.float64, dev)
        sweeps = L.scratch((B,), torch.int32, dev)
        L.launch("geodesic_lds", dev, *mesh.args(), B, L.ptr(D0), L.ptr(D), L.ptr(sweeps), max_sweeps)
        sweeps = sweeps.cpu().to(torch.int64)
        if bool((sweeps < 0).any()):
            raise RuntimeError("geodesic distance: not converged within max_sweeps=%d sweeps" % max_sweeps)
        return D, sweeps
    ws = L.workspace(nbytes := int(L.lib().recmv_geodesic_workspace_bytes(V, mesh.F, B)), dev, "geodesic_workspace_bytes",
                     dtype=torch.float64)
    ws[:B * V].copy_(D0.view(-1))
    last = ws[nbytes // 8 - (4 * B + 7) // 8:].view(torch.int32)[:B]
    done = 0
    while True:
        n = min(check_every, max_sweeps + 1 - done)
        L.launch("geodesic_sweeps", dev, *mesh.args(), B, L.ptr(ws), nbytes, done, n)
        done += n
        sweeps = last.cpu().to(torch.int64)                # (the one read-back per interval)
        if int(sweeps.max()) < done:                       # the last sweep lowered nothing anywhere
            break
        if done > max_sweeps:                              # sweep max_sweeps + 1 still lowered a value
            raise RuntimeError("geodesic distance: not converged within max_sweeps=%d sweeps" % max_sweeps)
    return ws[(done & 1) * B * V:((done & 1) + 1) * B * V].view(B, V).clone(), sweeps


def _distance(verts, faces, sources, values, route, max_sweeps, check_every, mesh=None):
    """(D [B, V], sweeps [B]) of a list of source tensors.  Every argument error is raised before the device is touched."""
    if route not in ROUTES:
        raise ValueError("route must be one of %r (got %r)" % (ROUTES, route))
    check_mesh(verts, faces, cuda=False)
    V = verts.shape[0]
    max_sweeps = V + 1 if max_sweeps is None else int(max_sweeps)
    if not (0 <= max_sweeps <= 1 << 30):
        raise ValueError("max_sweeps must be 0 .. 2^30 (got %r)" % (max_sweeps,))
    check_every = DEFAULT_CHECK_EVERY if check_every is None else int(check_every)
    if check_every < 1:
        raise ValueError("check_every must be at least 1 (got %r)" % (check_every,))
    if route == 'lds' and V > lds_max_vertices():
        raise ValueError("route='lds' takes at most %d vertices (got %d)" % (lds_max_vertices(), V))
    idx, val = _host_sources(V, sources, values)
    mesh = mesh or _Mesh(verts, faces)
    if route == 'auto':
        route = 'lds' if V <= auto_max_vertices() else 'sweeps'
    return _solve(mesh, _initial(V, len(sources), idx, val, mesh.device), route, max_sweeps, check_every)


@torch.no_grad()
def distance(verts, faces, sources, values=None, route='auto', max_sweeps=None, check_every=None, return_sweeps=False):
    """The geodesic distance field of the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA tensors on one device) from the
    vertices `sources`: an int64 [S] tensor (any device) -> [V] float64, or a list of B such tensors -> [B, V].  `values` (same
    shapes, default 0) are the sources' distances; of duplicate sources the least value holds.  Unreachable vertices are +inf.
    A source outside [0, V) or a value that is not finite is a ValueError.  `max_sweeps` (V + 1): more sweeps than that is a
    RuntimeError, never a partial field.  `check_every` (32): sweeps between two convergence checks of route='sweeps'; it
    changes no result.  return_sweeps=True adds K, the number of sweeps (an int, or int64 [B] on the host)."""
    single = not isinstance(sources, (list, tuple))
    if single:
        sources, values = [sources], (None if values is None else [values])
    D, sweeps = _distance(verts, faces, list(sources), values, route, max_sweeps, check_every)
    if single:
        D, sweeps = D[0], int(sweeps[0])
    return (D, sweeps) if return_sweeps else D


@torch.no_grad()
def boundary_distance(verts, faces, per_loop=False, route='auto'):
    """The distance to the border of the mesh: [V] float64 with every boundary vertex a source (all +inf for a closed mesh).
    per_loop=True: (fields [n_loops, V], loops) — one field per loop of connectivity.boundary_loops, solved in one batched
    call; zero fields for a closed mesh.  Faces with an index outside [0, V) do not count towards the border."""
    if route not in ROUTES:
        raise ValueError("route must be one of %r (got %r)" % (ROUTES, route))
    mesh = _Mesh(verts, faces)
    V = mesh.V
    ok = ((mesh.faces >= 0) & (mesh.faces < V)).all(1)
    good = mesh.faces[ok]
    if per_loop:
        loops = connectivity.boundary_loops(good, V)
        srcs = [torch.tensor(l, dtype=torch.int64) for l in loops]
        return _distance(verts, faces, srcs, None, route, None, None, mesh)[0], loops
    border = connectivity.EdgeTable(good, V).boundary_vertex.nonzero().squeeze(1)
    return _distance(verts, faces, [border], None, route, None, None, mesh)[0][0]


def nearest_source(fields):
    """(the minimum over the fields [V], label [V] int64) of fields [B, V]: the label is the field that attains the minimum,
    the LOWEST index among equal values, and -1 where every field is +inf.  A later field replaces an earlier one only when
    it is strictly smaller."""
    if fields.dim() != 2:
        raise ValueError("fields must have shape [B,V]")
    B, V = fields.shape
    best = torch.full((V,), float("inf"), dtype=fields.dtype, device=fields.device)
    label = torch.full((V,), -1, dtype=torch.int64, device=fields.device)
    for b in range(B):
        take = fields[b] < best
        best = torch.where(take, fields[b], best)
        label = torch.where(take, torch.full_like(label, b), label)
    return best, label


def interpolate(field, verts, faces, face_ids, points):
    """The field [V] at points [P,3] that lie on the faces face_ids [P]: float64 barycentric weights of the point in its face
    (areas of the three sub-triangles over their sum), +inf when any corner of the face is +inf.  Plain torch."""
    if field.dim() != 1 or field.shape[0] != verts.shape[0]:
        raise ValueError("field must have shape [V]")
    if points.dim() != 2 or points.shape[1] != 3 or face_ids.dim() != 1 or face_ids.shape[0] != points.shape[0]:
        raise ValueError("points must have shape [P,3] and face_ids [P]")
    tri = faces[face_ids]
    p = verts.to(torch.float64)[tri]                                               # [P,3,3]
    q = points.to(torch.float64)
    d = field.to(torch.float64)[tri]                                               # [P,3]

    def area(a, b, c):
        return torch.linalg.cross(b - a, c - a, dim=1).norm(dim=1)
    w = torch.stack([area(q, p[:, 1], p[:, 2]), area(p[:, 0], q, p[:, 2]), area(p[:, 0], p[:, 1], q)], 1)
    w = w / w.sum(1, keepdim=True)
    fin = torch.isfinite(d).all(1)
    out = (w * torch.where(fin[:, None], d, torch.zeros_like(d))).sum(1)
    return torch.where(fin, out, torch.full_like(out, float("inf")))


@torch.no_grad()
def farthest_points(verts, faces, k, first=0, route='auto'):
    """Farthest-point sampling by geodesic distance: (ids, the running minimum field [V]).  ids[0] = first; each further id is
    the argmax of the running minimum over its finite entries, the lowest id among equal maxima.  Every field is solved
    afresh and folded in by an elementwise minimum.  Fewer than k ids come back when only +inf and 0 remain."""
    check_mesh(verts, faces, cuda=False)
    V, k, first = verts.shape[0], int(k), int(first)
    if route not in ROUTES:
        raise ValueError("route must be one of %r (got %r)" % (ROUTES, route))
    if k < 0:
        raise ValueError("k must not be negative (got %d)" % k)
    if k and not (0 <= first < V):
        raise ValueError("first=%d lies outside [0, %d)" % (first, V))
    mesh = _Mesh(verts, faces)
    ids, run = [], torch.full((V,), float("inf"), dtype=torch.float64, device=mesh.device)
    nxt = first
    while len(ids) < k:
        ids.append(nxt)
        run = torch.minimum(run, _distance(verts, faces, [torch.tensor([nxt])], None, route, None, None, mesh)[0][0])
        fin = torch.where(torch.isfinite(run), run, torch.full_like(run, -float("inf")))
        top = fin.max()
        if not bool(top > 0.):
            break
        nxt = int((fin == top).nonzero()[0, 0])            # the lowest id among equal maxima, written out
    return ids, run
