"""Mesh parameterisation (csrc/mesh_param.hip) — an ADDITION to the reference: the garment laid flat.

  cut_to_disk       seams along shortest paths between the boundary loops, so that a shirt (4 loops) or a skirt (2) becomes a disk
  circle_boundary   a loop's vertices on the unit circle, by arc length
  harmonic          the harmonic map of a disk onto the unit disk (cotangent or uniform weights; uniform never flips a face)
  arap              as-rigid-as-possible flattening by local/global iterations
  distortion        per-face singular values of the map and their area-weighted summaries
  flatten           cut, map, scale to the surface's area: the sewing pattern
  solve, face_frames, arap_rhs   the kernels' wrappers

The definitions (the system solved, the summation order, the ARAP step, unusable faces, the seam rule) are those of
include/recmv_hip.h and INTEGRATION.md §5.  The solver has two routes with the same bits and iteration count: 'launch' (any size)
and 'lds' (one workgroup, up to lds_max_vertices() vertices); 'auto' takes 'lds' up to auto_max_vertices().
"""
import heapq

import numpy as np
import torch

from . import _lib as L
from . import connectivity
from .mesh_args import check_csr, check_mesh

ROUTES = ('auto', 'launch', 'lds')
WEIGHTS = ('cotangent', 'uniform')
METHODS = ('arap', 'harmonic')
SLOT = 256                       # faces per energy partial: the kernels' workgroup


def lds_max_vertices():
    """recmv_param_lds_max_vertices(): the most vertices route='lds' takes."""
    return int(L.lib().recmv_param_lds_max_vertices())


def auto_max_vertices():
    """recmv_param_auto_max_vertices(): route='auto' takes the lds route up to this many vertices."""
    return int(L.lib().recmv_param_auto_max_vertices())


def _check_route(route):
    if route not in ROUTES:
        raise ValueError("route must be one of %r (got %r)" % (ROUTES, route))


def _check_solver(tol, max_iter):
    tol = float(tol)
    if not tol >= 0.:
        raise ValueError("tol must not be negative (got %r)" % (tol,))
    if max_iter is not None and int(max_iter) < 0:
        raise ValueError("max_iter must not be negative (got %r)" % (max_iter,))
    return tol, (None if max_iter is None else int(max_iter))


def _check_uv(uv, V, name="uv"):
    if not isinstance(uv, torch.Tensor) or uv.dtype != torch.float64 or uv.dim() != 2 or uv.shape != (V, 2):
        raise ValueError("%s must be float64 of shape [%d,2]" % (name, V))


# ------------------------------------------------------------------------------------------------------------- the cut
def _edge_length(p, a, b):
    d = p[a] - p[b]
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def cut_to_disk(verts, faces):
    """(verts', faces', origin [V'] int64, seams) of one connected, edge-manifold piece of genus 0 with n >= 1 boundary loops:
    n - 1 seams make it a disk.  Host logic on tensors of any device; the result is on the input's device and deterministic.
    From the longest loop (ties: the lowest vertex id) as the joined set: Dijkstra over the edges (float64 lengths; ties by the
    lowest vertex id) from every joined boundary and seam vertex to the nearest vertex of a loop not yet joined; the path is a
    seam and its loop joins.  Then every vertex's face corners are grouped into classes connected across unmarked edges; the
    class of the lowest face keeps the vertex, the others get copies V, V + 1, ... (by vertex, then class): verts'[k] ==
    verts[origin[k]].  seams: [{'vertices': original ids, 'length': float}].  ValueError names why a mesh is refused: closed,
    several pieces, genus > 0, non-manifold."""
    check_mesh(verts, faces, cuda=False)
    V, dev = verts.shape[0], verts.device
    f = faces.detach().cpu()
    if f.shape[0] == 0:
        raise ValueError("cut_to_disk: the mesh has no faces")
    if int(f.min()) < 0 or int(f.max()) >= V or bool(((f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])).any()):
        raise ValueError("cut_to_disk: a face is not valid (an index outside [0, V) or a repeated corner)")
    table = connectivity.EdgeTable(f, V)
    if bool(table.nonmanifold_edge.any()):
        raise ValueError("cut_to_disk: non-manifold: %d edges have more than two faces" % int(table.nonmanifold_edge.sum()))
    border_degree = torch.bincount(table.edges[table.boundary_edge].reshape(-1), minlength=V)
    if bool(((border_degree != 0) & (border_degree != 2)).any()):
        raise ValueError("cut_to_disk: non-manifold: boundary loops touch at a vertex")
    fl = f.tolist()
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in fl:
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    used = sorted(set(x for row in fl for x in row))
    if len(set(find(x) for x in used)) != 1:
        raise ValueError("cut_to_disk: several pieces: %d connected components" % len(set(find(x) for x in used)))
    loops = connectivity.boundary_loops(f, V)
    if not loops:
        raise ValueError("cut_to_disk: closed: the mesh has no boundary loop")
    twice_genus = 2 - (len(used) - table.E + len(fl)) - len(loops)
    if twice_genus != 0:
        raise ValueError("cut_to_disk: genus > 0: 2 - chi - loops = %d, a disk-like piece needs 0" % twice_genus)
    p = verts.detach().cpu().numpy().astype(np.float64)
    nbrs = [[] for _ in range(V)]
    for a, b in table.edges.tolist():
        w = _edge_length(p, a, b)
        nbrs[a].append((b, w))
        nbrs[b].append((a, w))
    lengths = [sum(_edge_length(p, l[k], l[(k + 1) % len(l)]) for k in range(len(l))) for l in loops]
    first = min(range(len(loops)), key=lambda k: (-lengths[k], min(loops[k])))
    loop_of = {}
    for k, l in enumerate(loops):
        for x in l:
            loop_of[x] = k
    joined, left = set(loops[first]), set(range(len(loops))) - {first}
    marked, seams = set(), []
    while left:
        dist, pred = {x: 0. for x in joined}, {x: -1 for x in joined}
        heap = [(0., x) for x in sorted(joined)]
        heapq.heapify(heap)
        settled, target = set(), None
        while heap:
            d, x = heapq.heappop(heap)
            if x in settled:
                continue
            settled.add(x)
            if x in loop_of and loop_of[x] in left:
                target = x
                break
            for y, w in nbrs[x]:
                nd = d + w
                if y not in dist or nd < dist[y] or (nd == dist[y] and y not in settled and x < pred[y]):
                    dist[y], pred[y] = nd, x
                    heapq.heappush(heap, (nd, y))
        if target is None:
            raise ValueError("cut_to_disk: several pieces: a boundary loop cannot be reached")
        path = [target]
        while pred[path[-1]] != -1:
            path.append(pred[path[-1]])
        path.reverse()
        length = 0.
        for a, b in zip(path[:-1], path[1:]):
            marked.add((min(a, b), max(a, b)))
            length += _edge_length(p, a, b)
        seams.append({'vertices': path, 'length': length})
        k = loop_of[target]
        joined |= set(loops[k]) | set(path)
        left.discard(k)
    # the cut: classes of a seam vertex's faces, connected across unmarked edges
    on_seam = sorted(set(x for e in marked for x in e))
    fan = {x: [] for x in on_seam}
    for t, row in enumerate(fl):
        for c in range(3):
            if row[c] in fan:
                fan[row[c]].append((t, c))
    origin = list(range(V))
    for x in on_seam:
        faces_x = [t for t, _ in fan[x]]
        cls = {t: t for t in faces_x}

        def root(t):
            while cls[t] != t:
                t = cls[t]
            return t
        by_edge = {}
        for t, c in fan[x]:
            for other in (fl[t][(c + 1) % 3], fl[t][(c + 2) % 3]):
                if (min(x, other), max(x, other)) not in marked:
                    by_edge.setdefault(other, []).append(t)
        for ts in by_edge.values():
            for t in ts[1:]:
                ra, rb = root(ts[0]), root(t)
                cls[max(ra, rb)] = min(ra, rb)
        roots = sorted(set(root(t) for t in faces_x))
        for r in roots[1:]:
            new = len(origin)
            origin.append(x)
            for t, c in fan[x]:
                if root(t) == r:
                    fl[t][c] = new
    origin = torch.tensor(origin, dtype=torch.int64, device=dev)
    return verts[origin], torch.tensor(fl, dtype=torch.int64, device=dev).reshape(-1, 3), origin, seams


def circle_boundary(verts, loop):
    """The vertices of `loop` (a list of ids along a closed walk) on the unit circle at angles proportional to the cumulative
    edge length: [len(loop), 2] float64 on verts' device.  Host arithmetic (numpy float64, sequential sums)."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("verts must have shape [V,3]")
    loop = [int(x) for x in loop]
    if not loop or min(loop) < 0 or max(loop) >= verts.shape[0]:
        raise ValueError("loop must list vertex ids in [0, %d)" % verts.shape[0])
    p = verts.detach()[torch.tensor(loop, device=verts.device)].cpu().numpy().astype(np.float32).astype(np.float64)
    d = np.roll(p, -1, 0) - p
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    total = length.sum()
    if not (np.isfinite(total) and total > 0):
        raise ValueError("circle_boundary: the loop has no length")
    cum = np.concatenate([[0.], np.cumsum(length)[:-1]])
    ang = 2. * np.pi * (cum / total)
    return torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], 1)).to(verts.device)


# ------------------------------------------------------------------------------------------------------------- kernels
class _Mesh:
    """The tables the kernels read, built once per mesh: the neighbour CSR, the vertex -> corner-slot CSR (corners outside
    [0, V) filed under a row of their own), and on demand the frames and the weights."""

    def __init__(self, verts, faces):
        self.verts, self.faces = check_mesh(verts, faces)
        self.V, self.F, self.device = verts.shape[0], faces.shape[0], verts.device
        V = self.V
        inside = ((self.faces >= 0) & (self.faces < V)).all(1)
        table = connectivity.EdgeTable(self.faces[inside], V)
        self.nbr = connectivity.neighbours_csr(table.edges, V)
        self.slots = connectivity.filed_slots_csr(self.faces, V)
        self._frames = None

    def frames(self):
        if self._frames is None:
            self._frames = face_frames(self.verts, self.faces)
        return self._frames

    def weights(self, kind):
        if kind == 'uniform':
            return torch.ones(self.nbr[1].shape[0], dtype=torch.float64, device=self.device)
        from . import smooth
        return smooth.cotangent_weights(self.verts, self.faces, self.nbr, self.slots)


@torch.no_grad()
def face_frames(verts, faces):
    """recmv_param_face_frames: (frames [F,4] = (x1, x2, y2, area), cots [F,3]) float64; zeros for unusable faces."""
    verts, faces = check_mesh(verts, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    frames, cots = L.scratch((F, 4), torch.float64, dev), L.scratch((F, 3), torch.float64, dev)
    L.launch("param_face_frames", dev, L.ptr(verts), V, L.ptr(faces), F, L.ptr(frames), L.ptr(cots))
    return frames, cots


@torch.no_grad()
def solve(nbr_csr, weights, fixed, rhs, u, route='auto', tol=1e-12, max_iter=None, batch=None):
    """The fixed-vertex solve of include/recmv_hip.h: sum_j w_ij (u_i - u_j) = rhs_i at the free vertices, two columns, Jacobi-
    preconditioned CG started from u.  nbr_csr: (offsets [V+1], neighbours) int32; weights [nnz] float64; fixed [V] uint8 or
    bool; rhs, u [V,2] float64 (CUDA).  -> (u' [V,2], {'iterations', 'residuals', 'zero_rows', 'route'}).  `batch`: iterations
    between two read-backs on the launch route; it changes no bit."""
    _check_route(route)
    tol, max_iter = _check_solver(tol, max_iter)
    V = max(nbr_csr[0].numel() - 1, 0)                     # (an empty offsets table fails the check: it wants V + 1 entries)
    off, nbr = check_csr(nbr_csr, V, torch.int32, "nbr_csr")
    nnz = nbr.numel()
    if weights.dtype != torch.float64 or weights.shape != (nnz,):
        raise ValueError("weights must be float64 of shape [%d]" % nnz)
    if fixed.dim() != 1 or fixed.shape[0] != V or fixed.dtype not in (torch.uint8, torch.bool):
        raise ValueError("fixed must be uint8 or bool of shape [%d]" % V)
    _check_uv(rhs, V, "rhs")
    _check_uv(u, V, "u")
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be at least 1 (got %r)" % (batch,))
    if route == 'lds' and V > lds_max_vertices():
        raise ValueError("route='lds' takes at most %d vertices (got %d)" % (lds_max_vertices(), V))
    for t, name in ((off, "nbr_csr"), (nbr, "nbr_csr"), (weights, "weights"), (fixed, "fixed"), (rhs, "rhs"), (u, "u")):
        L.require_cuda(t, name)
    if route == 'auto':
        route = 'lds' if V <= auto_max_vertices() else 'launch'
    max_iter = 10 * V + 100 if max_iter is None else max_iter
    dev = u.device
    weights, rhs = weights.contiguous(), rhs.contiguous()
    fixed = fixed.to(torch.uint8).contiguous()
    out = u.clone(memory_format=torch.contiguous_format)
    lib = L.lib()
    iters, zero = L.C.c_int32(0), L.C.c_int32(0)
    res = (L.C.c_double * 2)()
    head = (L.ptr(off), L.ptr(nbr), L.ptr(weights), V, nnz, L.ptr(fixed), L.ptr(rhs), L.ptr(out), tol, max_iter)
    with L.device_guard(dev):
        if route == 'lds':
            report = L.scratch((16,), torch.float64, dev)
            L.check(lib.recmv_param_solve_lds(*head, L.C.byref(iters), res, L.C.byref(zero), L.ptr(report), L.stream_ptr(dev)),
                    "param_solve_lds")
        else:
            ws = L.workspace(nbytes := int(lib.recmv_param_solve_workspace_bytes(V)), dev, "param_solve_workspace_bytes",
                             dtype=torch.float64, floor=nbytes + 256)      # 256 bytes more: room for the alignment skip
            skip = (-ws.data_ptr() % 256) // 8
            L.check(lib.recmv_param_solve(*head, 0 if batch is None else int(batch), L.C.byref(iters), res, L.C.byref(zero),
                                          L.ptr(ws[skip:]), nbytes, L.stream_ptr(dev)), "param_solve")
    return out, {'iterations': int(iters.value), 'residuals': [float(res[0]), float(res[1])], 'zero_rows': int(zero.value),
                 'route': route}


@torch.no_grad()
def arap_rhs(faces, frames, cots, uv, slots_csr):
    """recmv_param_arap_rhs: (rot [F,2], rhs [V,2], energy partials [(F + 255) // 256], energy [1]) float64 on the device."""
    F, V, dev = faces.shape[0], uv.shape[0], uv.device
    _check_uv(uv, V)
    if frames.shape != (F, 4) or cots.shape != (F, 3) or frames.dtype != torch.float64 or cots.dtype != torch.float64:
        raise ValueError("frames must be float64 [F,4] and cots float64 [F,3]")
    for t, name in ((faces, "faces"), (frames, "frames"), (cots, "cots"), (uv, "uv")):
        L.require_cuda(t, name)
    soff, slots = slots_csr
    rot, rhs = L.scratch((F, 2), torch.float64, dev), L.scratch((V, 2), torch.float64, dev)
    partials, energy = L.scratch(((F + SLOT - 1) // SLOT,), torch.float64, dev), L.scratch((1,), torch.float64, dev)
    L.launch("param_arap_rhs", dev, L.ptr(faces.contiguous()), F, L.ptr(frames.contiguous()), L.ptr(cots.contiguous()),
             L.ptr(uv.contiguous()), V, L.ptr(soff), L.ptr(slots), L.ptr(rot), L.ptr(rhs), L.ptr(partials), L.ptr(energy))
    return rot, rhs, partials, energy


# ------------------------------------------------------------------------------------------------------------- the maps
def _disk_loop(faces, V):
    loops = connectivity.boundary_loops(faces, V)
    if len(loops) != 1:
        raise ValueError("the mesh must be a disk: it has %d boundary loops (cut_to_disk makes one)" % len(loops))
    loop = loops[0]
    # walked along the faces' own half-edges, so that the circle keeps the faces' orientation (det > 0)
    f = faces.detach().cpu()
    ahead = set(zip(f.reshape(-1).tolist(), f[:, [1, 2, 0]].reshape(-1).tolist()))
    return loop if len(loop) < 2 or (loop[0], loop[1]) in ahead else [loop[0]] + loop[:0:-1]


def _harmonic(mesh, weights, route, tol, max_iter):
    V, dev = mesh.V, mesh.device
    loop = _disk_loop(mesh.faces, V)
    idx = torch.tensor(loop, dtype=torch.int64, device=dev)
    fixed = torch.zeros(V, dtype=torch.uint8, device=dev)
    fixed[idx] = 1
    u0 = torch.zeros(V, 2, dtype=torch.float64, device=dev)
    u0[idx] = circle_boundary(mesh.verts, loop)
    rhs = torch.zeros(V, 2, dtype=torch.float64, device=dev)
    return solve(mesh.nbr, mesh.weights(weights), fixed, rhs, u0, route, tol, max_iter)


@torch.no_grad()
def harmonic(verts, faces, weights='cotangent', route='auto', tol=1e-12, max_iter=None, return_info=False):
    """The harmonic map of the disk verts [V,3] f32 / faces [F,3] int64 (CUDA) onto the unit disk: uv [V,2] float64.  The
    boundary loop is fixed by circle_boundary, the free vertices start at 0.  weights='uniform' never flips a face (Tutte);
    'cotangent' follows the geometry.  return_info adds the solver's dict."""
    if weights not in WEIGHTS:
        raise ValueError("weights must be one of %r (got %r)" % (WEIGHTS, weights))
    _check_route(route)
    tol, max_iter = _check_solver(tol, max_iter)
    check_mesh(verts, faces, cuda=False)
    if route == 'lds' and verts.shape[0] > lds_max_vertices():
        raise ValueError("route='lds' takes at most %d vertices (got %d)" % (lds_max_vertices(), verts.shape[0]))
    uv, info = _harmonic(_Mesh(verts, faces), weights, route, tol, max_iter)
    return (uv, info) if return_info else uv


def _arap(mesh, uv, iterations, route, tol):
    frames, cots = mesh.frames()
    w = mesh.weights('cotangent')
    used = mesh.faces[frames[:, 3] > 0]
    fixed = torch.zeros(mesh.V, dtype=torch.uint8, device=mesh.device)
    if used.numel():
        fixed[used.min()] = 1                              # the lowest vertex of a usable face, at its current value
    energies, cg, taken = [], [], None
    for _ in range(iterations):
        _, rhs, _, energy = arap_rhs(mesh.faces, frames, cots, uv, mesh.slots)
        energies.append(float(energy.item()))
        uv, info = solve(mesh.nbr, w, fixed, rhs, uv, route, tol, None)
        cg.append(info['iterations'])
        taken = info['route']
    energies.append(float(arap_rhs(mesh.faces, frames, cots, uv, mesh.slots)[3].item()))
    return uv, {'energies': energies, 'cg_iterations': cg, 'route': taken}


@torch.no_grad()
def arap(verts, faces, uv0=None, iterations=20, route='auto', tol=1e-12, return_info=False):
    """As-rigid-as-possible flattening of the disk: `iterations` local/global steps from uv0 [V,2] float64 (default: harmonic).
    The local step fits a rotation per face in closed form; the global step solves the cotangent system for the rotated flat
    edges with only the lowest-id vertex of a usable face fixed at its current value, warm-started from the current uv.  info:
    'energies' (before every iteration and after the last), 'cg_iterations' per solve, 'route'."""
    _check_route(route)
    tol, _ = _check_solver(tol, None)
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative (got %r)" % (iterations,))
    check_mesh(verts, faces, cuda=False)
    if uv0 is not None:
        _check_uv(uv0, verts.shape[0], "uv0")
    if route == 'lds' and verts.shape[0] > lds_max_vertices():
        raise ValueError("route='lds' takes at most %d vertices (got %d)" % (lds_max_vertices(), verts.shape[0]))
    mesh = _Mesh(verts, faces)
    if uv0 is None:
        uv0 = _harmonic(mesh, 'cotangent', route, tol, None)[0]
    else:
        L.require_cuda(uv0, "uv0")
        _disk_loop(mesh.faces, mesh.V)
    uv, info = _arap(mesh, uv0, int(iterations), route, tol)
    return (uv, info) if return_info else uv


@torch.no_grad()
def distortion(verts, faces, uv):
    """How the map verts -> uv [V,2] float64 distorts each face (recmv_param_distortion) and in all.  A dict: 's1' >= 's2' [F]
    the singular values of the Jacobian (NaN for unusable faces), 'det' [F] its signed determinant (0), 'flipped' the usable
    faces with det <= 0, 'conformal' and 'area' the area-weighted means of s1 / s2 and s1 s2, 'isometric' and 'isometric_max' the
    area-weighted mean and the maximum of max(s1, 1 / s2), 'area_3d' and 'area_2d' the total areas (None where no face is
    usable)."""
    check_mesh(verts, faces, cuda=False)
    _check_uv(uv, verts.shape[0])
    check_mesh(verts, faces)
    L.require_cuda(uv, "uv")
    frames, _ = face_frames(verts, faces)
    return _distortion(faces.contiguous(), frames, uv.contiguous())


def _distortion(faces, frames, uv):
    F, V, dev = faces.shape[0], uv.shape[0], uv.device
    out = L.scratch((F, 3), torch.float64, dev)
    L.launch("param_distortion", dev, L.ptr(faces), F, L.ptr(frames), L.ptr(uv), V, L.ptr(out))
    s1, s2, det = out[:, 0], out[:, 1], out[:, 2]
    usable = ~torch.isnan(s1)
    a = frames[:, 3][usable]
    r = {'s1': s1, 's2': s2, 'det': det, 'flipped': int((usable & (det <= 0)).sum().item()), 'usable_faces': int(usable.sum().item())}
    total = float(a.sum().item()) if a.numel() else 0.
    if total > 0:
        t1, t2 = s1[usable], s2[usable]
        iso = torch.maximum(t1, 1. / t2)
        r.update(conformal=float((a * (t1 / t2)).sum().item()) / total, area=float((a * (t1 * t2)).sum().item()) / total,
                 isometric=float((a * iso).sum().item()) / total, isometric_max=float(iso.max().item()), area_3d=total,
                 area_2d=float((a * det[usable].abs()).sum().item()))
    else:
        r.update(conformal=None, area=None, isometric=None, isometric_max=None, area_3d=total, area_2d=0.)
    return r


def summary(dist):
    """The JSON-able part of distortion()'s dict."""
    return {k: v for k, v in dist.items() if k not in ('s1', 's2', 'det')}


@torch.no_grad()
def flatten(verts, faces, method='arap', normalise=True, weights='cotangent', iterations=20, route='auto', tol=1e-12):
    """cut_to_disk, then the map (`method`: 'arap' from the cotangent harmonic map, or 'harmonic' with `weights`).  normalise:
    one uniform scale so that the 2-D area equals the 3-D area, the scale of a sewing pattern.  A dict: 'verts', 'faces' (the
    cut mesh), 'uv' [V',2] float64, 'origin' [V'], 'seams', 'distortion' (summary), 'info' (solver iterations and route)."""
    if method not in METHODS:
        raise ValueError("method must be one of %r (got %r)" % (METHODS, method))
    if weights not in WEIGHTS:
        raise ValueError("weights must be one of %r (got %r)" % (WEIGHTS, weights))
    _check_route(route)
    tol, _ = _check_solver(tol, None)
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative (got %r)" % (iterations,))
    check_mesh(verts, faces)
    cv, cf, origin, seams = cut_to_disk(verts, faces)
    if route == 'lds' and cv.shape[0] > lds_max_vertices():
        raise ValueError("route='lds' takes at most %d vertices (the cut mesh has %d)" % (lds_max_vertices(), cv.shape[0]))
    mesh = _Mesh(cv, cf)
    if method == 'harmonic':
        uv, hinfo = _harmonic(mesh, weights, route, tol, None)
        info = {'method': method, 'route': hinfo['route'], 'cg_iterations': [hinfo['iterations']], 'zero_rows': hinfo['zero_rows']}
    else:
        uv0, hinfo = _harmonic(mesh, 'cotangent', route, tol, None)
        uv, ainfo = _arap(mesh, uv0, int(iterations), route, tol)
        info = {'method': method, 'route': hinfo['route'], 'cg_iterations': [hinfo['iterations']] + ainfo['cg_iterations'],
                'energies': ainfo['energies'], 'zero_rows': hinfo['zero_rows']}
    dist = _distortion(mesh.faces, mesh.frames()[0], uv)
    if normalise and dist['area_2d'] > 0:
        uv = uv * (dist['area_3d'] / dist['area_2d']) ** 0.5
        dist = _distortion(mesh.faces, mesh.frames()[0], uv)
    return {'verts': cv, 'faces': cf, 'uv': uv, 'origin': origin, 'seams': seams, 'distortion': summary(dist), 'info': info}
