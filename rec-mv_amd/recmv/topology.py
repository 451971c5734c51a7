"""What a triangle mesh is made of (csrc/mesh_topology.hip) — an ADDITION to the reference, which exports marching-cubes
extractions, registered garments and posed frames and never asks how many pieces they have, whether they are closed, or removes
the small detached pieces ("floaters") an SDF extraction leaves behind.

  graph_components  the connected components of a graph given as rows of 2 or 3 node ids (recmv_graph_components): for every
                    node the smallest node id of its component — the second shared mesh primitive beside metrics.MeshGrid
  components        the pieces of a mesh, joined through shared vertices or only across shared edges, with their face counts,
                    areas and bounding boxes (recmv_mesh_face_stats, recmv_segment_sums)
  report            a JSON-able description: counts, edge classes, pieces, boundary loops, Euler characteristic, watertightness,
                    triangle quality, and the largest pieces with their genus
  keep_components   the mesh without its floaters (and without invalid faces and unreferenced vertices)

Definitions (INTEGRATION.md §5 repeats them; tests/mesh_topology_reference.py restates them in numpy):
  valid face          its three indices lie in [0, V) and are distinct; every other face is INVALID: it belongs to no piece, has
                      no edges, area 0, and is always dropped
  'vertex' pieces     valid faces that share a vertex are one piece
  'edge' pieces       valid faces are one piece only when a chain of shared undirected edges joins them (what trimesh.split
                      does); an edge used by more than two faces joins all of them
  component ids       dense, 0 .. C - 1, ordered by the smallest member id (vertex id for 'vertex', face id for 'edge')
  edges               the distinct undirected edges of the valid faces: BOUNDARY when one face uses it, NON-MANIFOLD when more
                      than two do; an ORIENTATION CONFLICT is an edge of exactly two faces that both traverse in one direction
  boundary loops      the connected components of the graph of boundary edges; a PINCH vertex is a boundary vertex whose number
                      of boundary edges is not 2 (two loops touching there count as one loop)
  Euler characteristic  referenced vertices - edges + valid faces; genus = (2 - chi - loops) / 2 of a piece, given only when the
                      piece has no non-manifold edge, no orientation conflict and no pinch vertex
  watertight          at least one valid face and no boundary edge, non-manifold edge, orientation conflict, invalid face or face
                      of area 0
  area, angles        float64 from the float32 coordinates: 0.5 |(b - a) x (c - a)|, corner angles atan2(|u x w|, u . w)
Every integer is exact.  The float sums (areas, means) come from recmv_segment_sums and have the same bits on every run.
"""
import math

import torch

from . import _lib as L
from .connectivity import EdgeTable, compact, edges_packed
from .mesh_args import check_mesh

# Rounds of hook + compress launched between two read-backs of the device's "last round that hooked" counter.  A read-back
# costs a host synchronisation, a round past the fixpoint two launches that change nothing.  Measured on an MI355X
# (tools/mesh_topology_timing.py, profiles/mesh_topology_timing.json; DESIGN.md §8 "Topology"; 171 842 vertices, 335 680 faces,
# medians of 10 alternated repeats): the vertex rows (10 rounds) take 0.455 / 0.385 / 0.368 / 0.383 / 0.370 ms with 1 / 2 / 4 / 8 /
# 16 rounds per read-back, the face-pair rows of the 'edge' mode (7 rounds) 0.769 / 0.725 / 0.679 / 0.679 / 0.753 ms, a randomly
# numbered path over as many nodes (12 rounds) 0.864 / 0.781 / 0.734 / 0.741 / 0.722 ms: 4 and 8 are within 4 % of each other on
# every graph and ahead of 1 throughout.  It does not change any result, the reported round count included.
ROUNDS_PER_READBACK = 4
SMALL_ANGLE_DEG = 10.


def round_cap(n):
    """The rounds recmv_graph_components can need on n nodes, the round that finds nothing to hook included:
    2 ceil(log2 n) + 2 (csrc/mesh_topology.hip has the argument; at most 64 for int32 ids)."""
    return 2 * max(int(n) - 1, 0).bit_length() + 2


@torch.no_grad()
def graph_components(n, links, return_info=False, rounds_per_readback=None):
    """label [n] int64 (CUDA): the smallest node id of every node's connected component in the graph of `n` nodes whose rows
    links [M,2] or [M,3] int64 (CUDA) each join their nodes.  A row with an id outside [0, n) or a repeated id joins nothing; a
    node that no valid row touches is its own component.  `return_info`: also {'rounds', 'invalid', 'cap'} — the rounds the
    fixpoint needed (the one that found nothing to hook included; it depends on the graph alone), the rows that joined
    nothing, and round_cap(n).  The host launches ROUNDS_PER_READBACK rounds at a time until the device reports that the last one
    hooked nothing, and raises if round_cap(n) rounds did not get there."""
    L.require_cuda(links, "links")
    if links.dtype != torch.int64 or links.dim() != 2 or links.shape[1] not in (2, 3):
        raise ValueError("links must be int64 of shape [M,2] or [M,3]")
    n = int(n)
    if not (0 <= n < 1 << 31) or links.shape[0] >= 1 << 31:
        raise ValueError("graph_components: n=%d nodes, %d rows: at most 2^31 - 1 of each" % (n, links.shape[0]))
    per = ROUNDS_PER_READBACK if rounds_per_readback is None else int(rounds_per_readback)
    if per < 1:
        raise ValueError("rounds_per_readback must be at least 1")
    dev, M, K = links.device, links.shape[0], links.shape[1]
    cap = round_cap(n)
    if n == 0 or M == 0:
        label = torch.arange(n, dtype=torch.int64, device=dev)
        return (label, {'rounds': 1, 'invalid': 0, 'cap': cap}) if return_info else label
    links = links.contiguous()
    label = L.scratch((n,), torch.int32, dev)
    parent = L.scratch((n,), torch.int32, dev)
    state = L.scratch((4,), torch.int32, dev)
    done = 0
    while True:
        rounds = min(per, cap - done)
        L.launch("graph_components", dev, n, L.ptr(links), M, K, done, rounds, L.ptr(label), L.ptr(parent), L.ptr(state))
        done += rounds
        last_hooking, invalid = state[:2].cpu().tolist()                          # the read-back
        if last_hooking < done:
            break
        if done >= cap:                                    # cannot happen (the bound of csrc/mesh_topology.hip): never loop on
            raise RuntimeError("graph_components: no fixpoint after %d rounds on %d nodes (the cap)" % (done, n))
    label = label.long()
    return (label, {'rounds': last_hooking + 1, 'invalid': invalid, 'cap': cap}) if return_info else label


def valid_faces(faces, n_verts):
    """bool [F]: the three indices lie in [0, n_verts) and are distinct."""
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    return ((faces >= 0) & (faces < n_verts)).all(1) & (a != b) & (b != c) & (a != c)


def face_stats(verts, faces):
    """recmv_mesh_face_stats: (area [F], smallest angle [F] in radians, longest / shortest edge [F]) float64 and (invalid faces,
    valid faces with a corner that is not finite) as a device tensor [2] int32."""
    F, dev = faces.shape[0], faces.device
    area, angle, ratio = (L.scratch((F,), torch.float64, dev) for _ in range(3))
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    if F:
        L.launch("mesh_face_stats", dev, L.ptr(verts), verts.shape[0], L.ptr(faces), F, L.ptr(area), L.ptr(angle), L.ptr(ratio),
                 L.ptr(counts))
    return area, angle, ratio, counts


def segment_sums(values, offsets):
    """recmv_segment_sums: (sum, min, max) [S,C] float64 of the columns of values [N,C] float64 over the segments
    offsets[s] .. offsets[s + 1] of its rows (offsets [S + 1] int64, ascending); the same bits on every run."""
    L.require_cuda(values, "values")
    L.require_cuda(offsets, "offsets")
    if values.dtype != torch.float64 or values.dim() != 2 or not (1 <= values.shape[1] <= 8):
        raise ValueError("values must be float64 of shape [N,C] with C in 1 .. 8")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise ValueError("offsets must be int64 of shape [S + 1]")
    values, offsets = values.contiguous(), offsets.contiguous()
    (N, Cn), S, dev = values.shape, offsets.shape[0] - 1, values.device
    out = [L.scratch((S, Cn), torch.float64, dev) for _ in range(3)]
    if S == 0:
        return tuple(out)
    lib = L.lib()
    chunk = int(lib.recmv_segment_sums_chunk())
    chunks = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    chunks[1:] = torch.cumsum((offsets[1:] - offsets[:-1] + (chunk - 1)) // chunk, 0)
    ws = L.workspace(nbytes := int(lib.recmv_segment_sums_workspace_bytes(N, S, Cn)), dev, "segment_sums_workspace_bytes",
                     dtype=torch.float64)
    L.launch("segment_sums", dev, L.ptr(values), N, Cn, L.ptr(offsets), S, L.ptr(chunks), L.ptr(out[0]), L.ptr(out[1]),
             L.ptr(out[2]), L.ptr(ws), nbytes)
    return tuple(out)


def _total(values):
    """(sum, min, max) of a float64 vector as device scalars, through segment_sums (one segment)."""
    offsets = torch.tensor([0, values.shape[0]], dtype=torch.int64, device=values.device)
    s, lo, hi = segment_sums(values.reshape(-1, 1), offsets)
    return s[0, 0], lo[0, 0], hi[0, 0]


@torch.no_grad()
def components(verts, faces, connectivity='vertex'):
    """The pieces of the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA) — the module docstring has the definitions.  A dict:
      face_component [F] int64     dense ids 0 .. C - 1 ordered by the smallest member id; -1 for invalid faces
      vertex_component [V] int64   'vertex' only (None for 'edge'): -1 for vertices no valid face uses
      count C, faces_per_component [C] int64, area [C] float64, bbox_min / bbox_max [C,3] float32
      by_area [C] int64            component ids by decreasing area, ties to the lower id
      rounds, invalid_faces        the rounds recmv_graph_components needed; the faces that are not valid"""
    verts, faces = check_mesh(verts, faces)
    if connectivity not in ('vertex', 'edge'):
        raise ValueError("connectivity must be 'vertex' or 'edge' (got %r)" % (connectivity,))
    V, F, dev = verts.shape[0], faces.shape[0], faces.device
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError("components: at most 2^31 - 1 vertices and faces")
    valid = valid_faces(faces, V)
    vf = valid.nonzero().squeeze(1)
    vertex_component = None
    if connectivity == 'vertex':
        label, info = graph_components(V, faces, return_info=True)                # (an invalid face is a row that joins nothing)
        face_label = label[faces[vf, 0]]
    else:
        # the half-edges face by face, sorted by edge id; the sort is stable, so the faces of an edge are chained in face order
        edge, order = torch.sort(edges_packed(faces[vf], max(V, 1))[1].reshape(-1), stable=True)
        hface = vf[order // 3]
        same = edge[1:] == edge[:-1]
        label, info = graph_components(F, torch.stack([hface[:-1][same], hface[1:][same]], 1), return_info=True)
        face_label = label[vf]
    roots, dense = torch.unique(face_label, return_inverse=True)                  # sorted: the order of the smallest member
    count = int(roots.shape[0])
    face_component = torch.full((F,), -1, dtype=torch.int64, device=dev)
    face_component[vf] = dense
    if connectivity == 'vertex':
        used = torch.zeros(V, dtype=torch.bool, device=dev)
        used[faces[vf].reshape(-1)] = True
        vertex_component = torch.where(used, torch.searchsorted(roots, label).clamp_(max=max(count - 1, 0)),
                                       torch.full_like(label, -1)) if count else torch.full_like(label, -1)
    per = torch.bincount(dense, minlength=count)
    offsets = torch.zeros(count + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(per, 0)
    order = torch.sort(dense, stable=True)[1]              # the faces of a piece in face order: a fixed summation order
    area = face_stats(verts, faces)[0]
    tri = verts[faces[vf]]                                                         # [Fv,3,3]
    values = torch.cat([area[vf][:, None], tri.amin(1).double(), tri.amax(1).double()], 1)[order]
    s, lo, hi = segment_sums(values, offsets)
    comp_area = s[:, 0].contiguous()
    return {'face_component': face_component, 'vertex_component': vertex_component, 'count': count,
            'faces_per_component': per, 'area': comp_area, 'bbox_min': lo[:, 1:4].float(), 'bbox_max': hi[:, 4:7].float(),
            'by_area': torch.sort(comp_area, descending=True, stable=True)[1], 'rounds': info['rounds'],
            'invalid_faces': F - int(vf.shape[0])}


def _per(index, count):
    return torch.bincount(index, minlength=count).cpu().tolist()


@torch.no_grad()
def report(verts, faces, top=8):
    """A JSON-able description of the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA); the module docstring has the
    definitions.  Keys: vertices, faces, unreferenced_vertices, invalid_faces, zero_area_faces, nonfinite_faces (valid faces with a
    corner that is not finite), duplicate_faces (valid faces beyond the first with one vertex set), edges, boundary_edges,
    nonmanifold_edges, orientation_conflicts, components_vertex, components_edge, boundary_loops, boundary_pinch_vertices,
    euler_characteristic, watertight, area (valid faces with finite corners), min_angle_deg {min, mean, below_10_deg: the share
    of those faces whose smallest angle is below 10 degrees}, edge_length {min, mean, max} over the edges, and components: the
    `top` largest 'vertex' pieces by area, each {id, faces, area, area_share, bbox_min, bbox_max, boundary_loops,
    euler_characteristic, genus (None when not defined)}.  Quality figures of a mesh without faces to take them over are None."""
    comp = components(verts, faces, 'vertex')
    comp_edge = components(verts, faces, 'edge')
    verts, faces = verts.contiguous(), faces.contiguous()
    V, F, dev = verts.shape[0], faces.shape[0], faces.device
    Cn = comp['count']
    vc = comp['vertex_component']
    vf = (comp['face_component'] >= 0).nonzero().squeeze(1)
    n_valid = int(vf.shape[0])
    area, angle, _, counts = face_stats(verts, faces)
    nonfinite = int(counts[1].item())
    fine = vf[~torch.isnan(area[vf])]                                              # valid, every corner finite
    table = EdgeTable(faces[vf], V)
    E, ea, eb = table.E, table.edges[:, 0], table.edges[:, 1]
    ahead = torch.zeros(E, dtype=torch.int64, device=dev).index_add_(0, table.face_to_edge.reshape(-1),
                                                                     table.forward.reshape(-1).long())
    boundary, nonmanifold = table.boundary_edge, table.nonmanifold_edge
    conflict = (table.count == 2) & (ahead != 1)
    border = torch.stack([ea[boundary], eb[boundary]], 1)
    loop_label = graph_components(V, border)
    degree = torch.bincount(border.reshape(-1), minlength=V)
    loop_roots = torch.unique(loop_label[degree > 0])
    pinch = ((degree > 0) & (degree != 2)).nonzero().squeeze(1)
    referenced = int((vc >= 0).sum().item())
    duplicates = n_valid - int(torch.unique(torch.sort(faces[vf], dim=1)[0], dim=0).shape[0]) if n_valid else 0
    zero_area = int((area[vf] == 0).sum().item())
    out = {'vertices': V, 'faces': F, 'unreferenced_vertices': V - referenced, 'invalid_faces': F - n_valid,
           'zero_area_faces': zero_area, 'nonfinite_faces': nonfinite, 'duplicate_faces': duplicates, 'edges': E,
           'boundary_edges': int(boundary.sum().item()), 'nonmanifold_edges': int(nonmanifold.sum().item()),
           'orientation_conflicts': int(conflict.sum().item()), 'components_vertex': Cn,
           'components_edge': comp_edge['count'], 'boundary_loops': int(loop_roots.shape[0]),
           'boundary_pinch_vertices': int(pinch.shape[0]), 'euler_characteristic': referenced - E + n_valid}
    out['watertight'] = bool(n_valid > 0 and not (out['boundary_edges'] or out['nonmanifold_edges'] or out['orientation_conflicts']
                                                  or out['invalid_faces'] or out['zero_area_faces']))
    n_fine = int(fine.shape[0])
    total_area = float(_total(area[fine])[0].item()) if n_fine else 0.
    out['area'] = total_area
    if n_fine:
        a = angle[fine]
        s, lo, _ = _total(a)
        below = int((a < math.radians(SMALL_ANGLE_DEG)).sum().item())
        out['min_angle_deg'] = {'min': math.degrees(float(lo.item())), 'mean': math.degrees(float(s.item()) / n_fine),
                                'below_10_deg': below / n_fine}
    else:
        out['min_angle_deg'] = {'min': None, 'mean': None, 'below_10_deg': None}
    if E:
        d = verts[ea].double() - verts[eb].double()
        s, lo, hi = _total((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt())
        out['edge_length'] = {'min': float(lo.item()), 'mean': float(s.item()) / E, 'max': float(hi.item())}
    else:
        out['edge_length'] = {'min': None, 'mean': None, 'max': None}
    pieces = []
    if Cn:
        n_v, n_e = _per(vc[vc >= 0], Cn), _per(vc[ea], Cn)
        n_f, loops = comp['faces_per_component'].cpu().tolist(), _per(vc[loop_roots], Cn)
        flaws = [x + y + z for x, y, z in zip(_per(vc[ea[nonmanifold]], Cn), _per(vc[ea[conflict]], Cn), _per(vc[pinch], Cn))]
        areas, lo, hi = comp['area'].cpu().tolist(), comp['bbox_min'].cpu().tolist(), comp['bbox_max'].cpu().tolist()
        for c in comp['by_area'][:max(int(top), 0)].cpu().tolist():
            chi = n_v[c] - n_e[c] + n_f[c]
            twice = 2 - chi - loops[c]
            pieces.append({'id': c, 'faces': n_f[c], 'area': areas[c], 'area_share': areas[c] / total_area if total_area > 0 else None,
                           'bbox_min': lo[c], 'bbox_max': hi[c], 'boundary_loops': loops[c], 'euler_characteristic': chi,
                           'genus': twice // 2 if flaws[c] == 0 and twice >= 0 and twice % 2 == 0 else None})
    out['components'] = pieces
    return out


@torch.no_grad()
def keep_components(verts, faces, largest=None, min_area_frac=None, min_faces=None, connectivity='vertex'):
    """The mesh without the pieces that fail a rule — (verts', faces', info).  A piece (components(..., connectivity)) stays when
    it passes every rule given: `largest`: it is among the first `largest` entries of by_area; `min_area_frac`: its area is at
    least min_area_frac times the largest piece's area (float64, on the host); `min_faces`: it has at least that many faces.
    Invalid faces are always dropped, and so are the vertices no kept face uses; with no rule nothing else is.  Kept faces and
    vertices stay in their order and vertex rows are copied bit for bit.  info: kept_faces [F'] int64 (ids into faces),
    vertex_map [V] int64 (old -> new, -1: dropped), components, kept_components (ids), dropped_components, dropped_faces (valid
    faces of dropped pieces), dropped_area (their area), invalid_faces."""
    if largest is not None and int(largest) < 0:
        raise ValueError("largest must not be negative")
    if min_area_frac is not None and not (0. <= float(min_area_frac) <= 1.):
        raise ValueError("min_area_frac must be in [0, 1]")
    if min_faces is not None and int(min_faces) < 0:
        raise ValueError("min_faces must not be negative")
    comp = components(verts, faces, connectivity)
    Cn, dev = comp['count'], faces.device
    area = comp['area'].cpu().tolist()
    per = comp['faces_per_component'].cpu().tolist()
    keep = [True] * Cn
    if largest is not None:
        first = set(comp['by_area'][:int(largest)].cpu().tolist())
        keep = [k and c in first for c, k in enumerate(keep)]
    if min_area_frac is not None and Cn:
        bound = float(min_area_frac) * max(area)
        keep = [k and area[c] >= bound for c, k in enumerate(keep)]
    if min_faces is not None:
        keep = [k and per[c] >= int(min_faces) for c, k in enumerate(keep)]
    keep_t = torch.tensor(keep + [False], dtype=torch.bool, device=dev)            # (the last entry: component -1, invalid faces)
    kept_faces = keep_t[comp['face_component']].nonzero().squeeze(1)
    new_verts, new_faces, vertex_map = compact(verts, faces[kept_faces])
    dropped = [c for c in range(Cn) if not keep[c]]
    info = {'kept_faces': kept_faces, 'vertex_map': vertex_map, 'components': Cn,
            'kept_components': [c for c in range(Cn) if keep[c]], 'dropped_components': len(dropped),
            'dropped_faces': sum(per[c] for c in dropped), 'dropped_area': math.fsum(area[c] for c in dropped),
            'invalid_faces': comp['invalid_faces']}
    return new_verts.contiguous(), new_faces.contiguous(), info
