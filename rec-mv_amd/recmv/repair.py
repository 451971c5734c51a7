"""Mesh repair (csrc/point_grid.hip) — an ADDITION to the reference, which never mends a mesh: the stage between reading a mesh
and every other mesh stage.  recmv.topology.report names the defects; simplify, iso_remesh and smooth refuse a mesh that is not
edge-manifold; this module gets it there.

  points_within     every pair of vertices no farther apart than eps (recmv_points_within_*): the fixed-radius neighbour search
                    over points, the fourth shared mesh primitive beside metrics.MeshGrid, topology.graph_components and
                    connectivity.EdgeTable
  weld              vertices within eps of each other, transitively, become one
  drop_degenerate   the mesh without its invalid, zero-area, non-finite and duplicate faces
  split_nonmanifold every edge with more than two faces and every pinch vertex taken apart by duplicating vertices
  orient            every orientable piece consistently oriented
  repair            those four in that order and connectivity.compact

Every function is CUDA-only and returns (verts', faces', info).  Vertex rows are only ever copied bit for bit; no position is
computed.

Definitions (INTEGRATION.md §5 repeats them; tests/mesh_repair_reference.py restates them in numpy):
  pair              (i, j), i < j, both vertices finite, d2 <= eps * eps with d2 = (dx * dx + dy * dy) + dz * dz in float64 from the
                    f32 coordinates, without contraction: membership is exact.  eps = 0 finds coincident vertices, +0.0 == -0.0.
                    A vertex with a NaN or inf coordinate is in no pair.
  weld              the clusters are the connected components of the pairs (topology.graph_components).  A cluster becomes its
                    lowest-numbered vertex, at that vertex's position; faces are re-indexed (an index outside [0, V) stays); no
                    vertex is dropped, the merged ones are left unreferenced.  cluster_radius_max is the largest distance from a
                    merged vertex to its representative (float64; sqrt is correctly rounded, so it is exact): above eps it shows
                    that a chain of pairs collapsed, which happens when eps comes near the edge length.
  drop_degenerate   in this order: INVALID faces (topology's definition), faces whose recmv_mesh_face_stats area is 0, faces
                    whose area is NaN (a corner that is not finite), and among what is left every face beyond the first (lowest
                    id) with one vertex set, whatever its winding.  Kept faces stay in order.
  split_nonmanifold valid faces only.  Nodes are the 3F corners.  For every undirected edge with exactly two faces, and for each
                    of its two end vertices, that vertex's corner in the one face is linked to its corner in the other; an edge
                    with one face or with more than two links nothing.  Every connected component of corners is one vertex of the
                    result: the component that holds an old vertex's lowest corner slot keeps the old id, the others are
                    appended from V on, ordered by (old id, lowest slot).  Vertices that no face uses stay.
                    Why one pass suffices: at a vertex, a corner has at most two links, through its face's two edges there, so
                    the components are paths or cycles of corners — fans.  A face on an edge with more than two faces lost the
                    link through that edge and is a path END there.  An edge of the result at a result vertex is an edge of that
                    vertex's one fan: between two linked corners it has their two faces, and at a path end it has the end's one
                    face; a path has two ends, so no edge of the result has more than two faces.  Every vertex of the result
                    has one fan, so there is no pinch vertex, and every boundary vertex (its fan is a path) has exactly two
                    boundary edges, one at either end of the fan.
  orient            the two-cover graph on 2F nodes (f, 0), (f, 1) (needs F < 2^30).  For an edge with exactly two faces f < g let
                    p = 1 when both traverse it in one direction (an orientation conflict), else 0: links (f, 0)-(g, p) and
                    (f, 1)-(g, 1 ^ p).  An edge-connected piece (joined through such edges only) is orientable exactly when
                    (f, 0) and (f, 1) carry different labels.  In an orientable piece the faces whose (f, 0) lies in the
                    component of the piece's lowest face's (f, 0) form one side; the smaller side by face count is flipped, on a
                    tie the side that does not hold the lowest face.  A flip swaps columns 1 and 2.  A piece that is not
                    orientable is left as it is and counted.  Invalid faces belong to no piece and stay.
  repair            weld (when weld_eps is given), drop_degenerate, split_nonmanifold, orient, connectivity.compact.  The chain
                    is idempotent: a second call with the same arguments changes nothing.

Deliberately out of scope: hole filling (garments are open by design, so which boundary loops are holes needs a rule of its
own: recmv.holes has it), outward orientation by signed volume, T-junctions, and the removal of self-intersections.
"""
import math

import torch

from . import _lib as L
from .connectivity import EdgeTable, compact
from .mesh_args import check_mesh, check_points, info_json  # noqa: F401  (info_json: the JSON-able part of an info dict)
from .topology import face_stats, graph_components, valid_faces

MAX_AXIS_CELLS = 1 << 20                                   # csrc/point_grid.hip checks both
MAX_CELLS = 1 << 24
CELLS_PER_VERTEX = 4                                       # the table is never larger than this many cells per vertex (or 64)
CELL_MARGIN = 1. + 2. ** -20                               # cell >= eps * this: the 27-cell search is complete under rounding


def grid_layout(lo, hi, eps, n):
    """The cell grid of points_within over the box lo .. hi (3 floats each) of n finite vertices: (origin (3 floats), cell,
    (nx, ny, nz)).  Cubic cells of edge cell >= eps * (1 + 2^-20); at most 2^20 along an axis and min(2^24, max(4 n, 64)) in
    all: where eps and the extent ask for more, the cells get COARSER (doubled until they fit), so the table never grows with
    the extent of the mesh.  Plain Python on the host."""
    eps = float(eps)
    ext = [max(float(h) - float(l), 0.) for l, h in zip(lo, hi)]
    cap = min(MAX_CELLS, max(CELLS_PER_VERTEX * int(n), 64))
    cell = max(eps * CELL_MARGIN, max(ext) / (MAX_AXIS_CELLS - 2))
    if not (cell > 0.):
        cell = 1.                                          # eps = 0 and every vertex in one place: one cell
    while True:
        dims = [min(int(e / cell) + 1, MAX_AXIS_CELLS) for e in ext]
        if dims[0] * dims[1] * dims[2] <= cap:
            return [float(x) for x in lo], cell, tuple(dims)
        cell *= 2.


def _check_eps(eps, name="eps"):
    eps = float(eps)
    if not (0. <= eps < math.inf):
        raise ValueError("%s must be finite and not negative (got %r)" % (name, eps))
    return eps


@torch.no_grad()
def points_within(verts, eps, max_pairs=None, return_info=False):
    """pairs [P,2] int64 (CUDA): every (i, j), i < j, of finite vertices of verts [V,3] f32 (CUDA) with d2 <= eps * eps (the
    module docstring has the exact expression), ordered by i; the same array on every run.  `max_pairs` (default 64 V): when
    there are more pairs a ValueError says that eps is too large for this mesh; nothing partial is returned.  `return_info`:
    also {'pairs', 'nonfinite_vertices', 'cell', 'dims'}.  Two host synchronisations: the bounding box and the pair count."""
    eps = _check_eps(eps)
    if max_pairs is not None and int(max_pairs) < 0:
        raise ValueError("max_pairs must not be negative")
    verts = check_points(verts, "verts", cuda=False, shape="[V,3]")
    if verts.shape[0] >= 1 << 31:
        raise ValueError("at most 2^31 - 1 vertices")
    L.require_cuda(verts, "verts")
    V, dev = verts.shape[0], verts.device
    max_pairs = 64 * V if max_pairs is None else int(max_pairs)
    empty = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    finite = torch.isfinite(verts).all(1)
    n_finite = int(finite.sum().item()) if V else 0
    info = {'pairs': 0, 'nonfinite_vertices': V - n_finite, 'cell': None, 'dims': None}
    if n_finite == 0:
        return (empty, info) if return_info else empty
    box = torch.stack([verts[finite].amin(0), verts[finite].amax(0)]).double().cpu().tolist()       # the read-back
    origin, cell, dims = grid_layout(box[0], box[1], eps, n_finite)
    info['cell'], info['dims'] = cell, dims
    grid = (origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2])
    cells = dims[0] * dims[1] * dims[2]
    cell_of = L.scratch((V,), torch.int32, dev)
    L.launch("points_within_cells", dev, L.ptr(verts), V, *grid, L.ptr(cell_of))
    ids = (cell_of >= 0).nonzero().squeeze(1)
    key, perm = torch.sort(cell_of[ids].long(), stable=True)                      # by cell, by id inside a cell
    ids = ids[perm].contiguous()
    pts = verts[ids].contiguous()
    n = int(ids.shape[0])
    cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = torch.cumsum(torch.bincount(key, minlength=cells), 0)
    counts = L.scratch((V,), torch.int64, dev)
    L.launch("points_within_count", dev, L.ptr(pts), L.ptr(ids), n, V, eps, *grid, L.ptr(cell_start), L.ptr(counts))
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item())                                                   # the read-back
    if total > max_pairs:
        raise ValueError("points_within: %d pairs among %d vertices, more than max_pairs=%d: eps=%g is too large for this mesh"
                         % (total, V, max_pairs, eps))
    info['pairs'] = total
    if total == 0:
        return (empty, info) if return_info else empty
    offsets = (ends - counts).contiguous()
    pairs = L.scratch((total, 2), torch.int64, dev)
    L.launch("points_within_fill", dev, L.ptr(pts), L.ptr(ids), n, V, eps, *grid, L.ptr(cell_start), L.ptr(offsets), L.ptr(pairs),
             total)
    return (pairs, info) if return_info else pairs


@torch.no_grad()
def weld(verts, faces, eps=0., max_pairs=None):
    """Vertices within eps of each other, transitively, become one — (verts, faces', info); the module docstring has the
    definition.  info: pairs, merged_vertices (vertices that are no longer their own representative), clusters (representatives
    of more than one vertex), vertex_map [V] int64 (old -> representative), nonfinite_vertices, cluster_radius_max."""
    eps = _check_eps(eps)
    verts, faces = check_mesh(verts, faces, cap31=True)
    V, dev = verts.shape[0], verts.device
    pairs, pinfo = points_within(verts, eps, max_pairs=max_pairs, return_info=True)
    label = graph_components(V, pairs)
    own = torch.arange(V, dtype=torch.int64, device=dev)
    merged = (label != own).nonzero().squeeze(1)
    n_merged = int(merged.shape[0])
    radius = 0.
    if n_merged:
        d = verts[merged].double() - verts[label[merged]].double()
        radius = float((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt().max().item())
    if V:
        inside = (faces >= 0) & (faces < V)
        new_faces = torch.where(inside, label[faces.clamp(0, V - 1)], faces)
    else:
        new_faces = faces.clone()
    info = {'pairs': pinfo['pairs'], 'merged_vertices': n_merged,
            'clusters': int(torch.unique(label[merged]).shape[0]) if n_merged else 0, 'vertex_map': label,
            'nonfinite_vertices': pinfo['nonfinite_vertices'], 'cluster_radius_max': radius}
    return verts.clone(), new_faces.contiguous(), info


@torch.no_grad()
def drop_degenerate(verts, faces):
    """The mesh without its invalid, zero-area, non-finite and duplicate faces — (verts, faces', info); the module docstring
    has the definition.  info: invalid_faces, zero_area_faces, nonfinite_faces, duplicate_faces, kept_faces [F'] int64."""
    verts, faces = check_mesh(verts, faces, cap31=True)
    V, F, dev = verts.shape[0], faces.shape[0], faces.device
    valid = valid_faces(faces, V)
    area = face_stats(verts, faces)[0]
    zero = valid & (area == 0)
    nonfinite = valid & torch.isnan(area)
    cand = (valid & ~zero & ~nonfinite).nonzero().squeeze(1)
    n_dup = 0
    if cand.shape[0]:
        _, group = torch.unique(torch.sort(faces[cand], dim=1)[0], dim=0, return_inverse=True)
        first = torch.full((int(group.max().item()) + 1,), F, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, group, cand, 'amin')
        keep = first[group] == cand
        n_dup = int((~keep).sum().item())
        cand = cand[keep]
    info = {'invalid_faces': F - int(valid.sum().item()), 'zero_area_faces': int(zero.sum().item()),
            'nonfinite_faces': int(nonfinite.sum().item()), 'duplicate_faces': n_dup, 'kept_faces': cand}
    return verts.clone(), faces[cand].contiguous(), info


def _require_valid(faces, V, what):
    if faces.shape[0] and not bool(valid_faces(faces, V).all().item()):
        raise ValueError("%s: the mesh has invalid faces (an index outside [0, V) or repeated): drop_degenerate removes them" % what)


def _two_face_edges(table):
    """The half-edge slots (3 f + k: the edge opposite corner k of face f) of the edges of an EdgeTable that have exactly two
    faces, as (first [M], second [M]): the two slots of every such edge, the lower face first, in edge order."""
    fe = table.face_to_edge.reshape(-1)
    slots = (table.count[fe] == 2).nonzero().squeeze(1)
    order = torch.sort(fe[slots], stable=True)[1]
    slots = slots[order]
    return slots[0::2], slots[1::2]


@torch.no_grad()
def split_nonmanifold(verts, faces):
    """Every edge with more than two faces and every pinch vertex taken apart by duplicating vertices — (verts', faces', info);
    the module docstring has the definition and the argument that one pass suffices.  Raises ValueError on invalid faces.
    info: split_vertices (old vertices that became several), added_vertices, nonmanifold_edges_before, origin [V'] int64 (the
    old id of every vertex)."""
    verts, faces = check_mesh(verts, faces, cap31=True)
    V, F, dev = verts.shape[0], faces.shape[0], faces.device
    _require_valid(faces, V, "split_nonmanifold")
    if 3 * F >= 1 << 31:
        raise ValueError("split_nonmanifold: at most (2^31 - 1) / 3 faces")
    own = torch.arange(V, dtype=torch.int64, device=dev)
    if F == 0:
        return verts.clone(), faces.clone(), {'split_vertices': 0, 'added_vertices': 0, 'nonmanifold_edges_before': 0, 'origin': own}
    table = EdgeTable(faces, V)
    h1, h2 = _two_face_edges(table)
    fv = faces.reshape(-1)
    f1, k1, f2, k2 = 3 * (h1 // 3), h1 % 3, 3 * (h2 // 3), h2 % 3
    a1, b1 = f1 + (k1 + 1) % 3, f1 + (k1 + 2) % 3                                  # the corners at the edge's two ends
    a2, b2 = f2 + (k2 + 1) % 3, f2 + (k2 + 2) % 3
    same = fv[a1] == fv[a2]
    links = torch.cat([torch.stack([a1, torch.where(same, a2, b2)], 1), torch.stack([b1, torch.where(same, b2, a2)], 1)], 0)
    label = graph_components(3 * F, links.contiguous())                            # the lowest corner slot of every fan
    slot = torch.arange(3 * F, dtype=torch.int64, device=dev)
    low = torch.full((V,), 3 * F, dtype=torch.int64, device=dev).scatter_reduce_(0, fv, slot, 'amin')
    roots = (label == slot).nonzero().squeeze(1)                                   # ascending
    extra = roots[low[fv[roots]] != roots]
    extra = extra[torch.sort(fv[extra], stable=True)[1]]                           # by (old id, lowest slot)
    A = int(extra.shape[0])
    new_id = fv.clone()
    new_id[extra] = V + torch.arange(A, dtype=torch.int64, device=dev)
    info = {'split_vertices': int(torch.unique(fv[extra]).shape[0]) if A else 0, 'added_vertices': A,
            'nonmanifold_edges_before': int(table.nonmanifold_edge.sum().item()), 'origin': torch.cat([own, fv[extra]])}
    return torch.cat([verts, verts[fv[extra]]]).contiguous(), new_id[label].reshape(F, 3).contiguous(), info


@torch.no_grad()
def orient(verts, faces):
    """Every orientable piece consistently oriented — (verts, faces', info); the module docstring has the definition.
    info: flipped_faces, conflicts_before (edges of exactly two faces that both traverse in one direction),
    non_orientable_pieces, flipped [F] bool."""
    verts, faces = check_mesh(verts, faces, cap31=True)
    V, F, dev = verts.shape[0], faces.shape[0], faces.device
    if F >= 1 << 30:
        raise ValueError("orient: at most 2^30 - 1 faces")
    flipped = torch.zeros(F, dtype=torch.bool, device=dev)
    info = {'flipped_faces': 0, 'conflicts_before': 0, 'non_orientable_pieces': 0, 'flipped': flipped}
    vf = valid_faces(faces, V).nonzero().squeeze(1)
    Fv = int(vf.shape[0])
    if Fv == 0:
        return verts.clone(), faces.clone(), info
    table = EdgeTable(faces[vf].contiguous(), V)
    h1, h2 = _two_face_edges(table)
    forward = table.forward.reshape(-1)
    p = (forward[h1] == forward[h2]).long()
    f, g = h1 // 3, h2 // 3
    links = torch.cat([torch.stack([2 * f, 2 * g + p], 1), torch.stack([2 * f + 1, 2 * g + (1 - p)], 1)], 0)
    label = graph_components(2 * Fv, links.contiguous()).reshape(Fv, 2)
    lowest = torch.minimum(label[:, 0], label[:, 1]) // 2                          # the lowest face of every face's piece
    orientable = label[:, 0] != label[:, 1]
    side_a = label[:, 0] == 2 * lowest                                             # with the lowest face as it stands
    n_a = torch.bincount(lowest[orientable & side_a], minlength=Fv)
    n_b = torch.bincount(lowest[orientable & ~side_a], minlength=Fv)
    flip_a = n_a < n_b                                                             # (a tie flips the other side)
    flip = orientable & torch.where(side_a, flip_a[lowest], ~flip_a[lowest])
    flipped[vf] = flip
    new_faces = torch.where(flipped[:, None], faces[:, [0, 2, 1]], faces)
    info.update({'flipped_faces': int(flip.sum().item()), 'conflicts_before': int(p.sum().item()),
                 'non_orientable_pieces': int(torch.unique(lowest[~orientable]).shape[0])})
    return verts.clone(), new_faces.contiguous(), info


@torch.no_grad()
def repair(verts, faces, weld_eps=None, degenerate=True, split=True, orientation=True, max_pairs=None):
    """weld (when weld_eps is not None), drop_degenerate, split_nonmanifold, orient and connectivity.compact, in that order —
    (verts', faces', info).  info holds each stage's info under 'weld', 'drop_degenerate', 'split_nonmanifold', 'orient', and
    for the whole chain vertex_map [V] int64 (old -> new; a welded vertex maps to its representative, a split one to the copy
    that kept its id; -1: dropped), kept_faces [F'] int64 (ids into faces) and origin [V'] int64 (the old vertex every vertex
    of the result is a copy of).  Idempotent: a second call with the same arguments changes nothing.  split_nonmanifold raises
    on invalid faces, so `degenerate=False` is for meshes that have none."""
    if weld_eps is not None:
        weld_eps = _check_eps(weld_eps, "weld_eps")
    v, f = check_mesh(verts, faces, cap31=True)
    V, F, dev = v.shape[0], f.shape[0], v.device
    info = {}
    vmap = torch.arange(V, dtype=torch.int64, device=dev)
    kept = torch.arange(F, dtype=torch.int64, device=dev)
    origin = vmap
    if weld_eps is not None:
        v, f, info['weld'] = weld(v, f, weld_eps, max_pairs=max_pairs)
        vmap = info['weld']['vertex_map']
    if degenerate:
        v, f, info['drop_degenerate'] = drop_degenerate(v, f)
        kept = kept[info['drop_degenerate']['kept_faces']]
    if split:
        v, f, info['split_nonmanifold'] = split_nonmanifold(v, f)
        origin = info['split_nonmanifold']['origin']
    if orientation:
        v, f, info['orient'] = orient(v, f)
    v, f, cmap = compact(v, f)
    info['vertex_map'] = cmap[vmap] if V else vmap
    info['kept_faces'] = kept
    info['origin'] = origin[cmap >= 0]
    return v.contiguous(), f.contiguous(), info
