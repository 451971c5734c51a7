"""Quadric-error mesh simplification (csrc/mesh_simplify.hip) — an ADDITION to the reference, which thinned its meshes by hand in
MeshLab: make a mesh smaller while keeping its shape (Garland & Heckbert 1997, edge collapse in rounds of independent sets).

  vertex_quadrics       Q [V,11] float64 per vertex (recmv_vertex_quadrics)
  edge_collapse_cost    where a collapse puts the vertex, what it costs, the weight (recmv_edge_collapse_cost)
  collapse_flip_check   no surviving face turns over (recmv_collapse_flip_check)
  simplify              the driver: (verts', faces', info)
Each kernel has a plain-torch restatement in float64 (`*_torch`); `use_kernels=False` takes them and runs on CPU tensors too.

Definitions (INTEGRATION.md §5 and DESIGN.md §8 repeat them; tests/mesh_simplify_reference.py restates them in numpy):
  quadric      per vertex the sum over its faces of area * (n, d)(n, d)^T (unit normal, plane through the face's first corner) and,
               over its boundary edges, of boundary_weight * |e|^2 * (m, d)(m, d)^T, m the unit vector in the edge's face
               perpendicular to the edge; the weight is the sum of the areas.  Computed once from the input; a collapse adds the
               quadric of the vertex that goes to the one that stays.
  placement    code 1 / 2: the vertex stays at the edge's first / second end; 0: the cheapest of the solved optimum, the two
               ends and the midpoint, ties to the earlier.  The solved optimum takes part only when it is finite and within
               REACH edge lengths of the midpoint.  A boundary vertex joined to an interior one stays where it is; a boundary edge
               keeps its lower end, so that the border's vertices never leave the input's border; an interior edge between two
               boundary vertices is never collapsed.
  cost         x^T (Q[a] + Q[b]) x at the f32 point, float64: squared distances to the planes, weighted by area.  cost / weight is
               a mean squared distance; `max_error` (a length) refuses cost > max_error^2 * weight.
  refusals     the link condition, a boundary loop keeps at least 3 edges (both iso_remesh's), a surviving face would turn over, and
               a tetrahedron keeps its edges (two interior vertices of valence 3: the one case the counted link condition lets by).
  round        the valid candidates sorted by (cost, edge id); only the cheapest are considered: as many as bring the face count
               ROUND_SHARE of the way to the target (a boundary collapse takes 1 face, an interior one 2), at least one; of those an
               independent set (no two within two rings of each other, the lower rank wins) is collapsed at once.
Same input, same output bits on the kernel path: integer keys decide every choice, and every float64 sum has one order.
"""
import math

import torch

from . import _lib as L
from .connectivity import EdgeTable, boundary_edges_csr, compact, vertex_slots_csr
from .iso_remesh import _Topo, _boundary_loop_length, _flip_ok, _independent, _link_ok, _merge, _padded
from .mesh_args import check_mesh

BOUNDARY_WEIGHT = 10.       # a boundary edge's plane counts like 10 |e|^2 of face area
REACH = 2.                  # the solved optimum must lie within this many edge lengths of the edge's midpoint
ROUND_SHARE = 0.5           # the share of the remaining face budget whose cheapest candidates one round considers
MAX_ROUNDS = 1000
FREE, STAY_A, STAY_B = 0, 1, 2
_HINT = "run clean_fl.py or look at recmv.topology.report"


# ------------------------------------------------------------------------------------------------- kernels and restatements
def vertex_quadrics(verts, faces, table=None, boundary_weight=BOUNDARY_WEIGHT, return_counts=False):
    """recmv_vertex_quadrics: Q [V,11] float64 (xx xy xz xw yy yz yw zz zw ww, weight) of verts [V,3] f32 / faces [F,3] int64
    (CUDA); `table`: the mesh's EdgeTable, built when absent (the faces must then be valid).  `return_counts`: also the number
    of invalid faces."""
    verts, faces = check_mesh(verts, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    Q = L.scratch((V, 11), torch.float64, dev)
    counts = torch.zeros(1, dtype=torch.int32, device=dev)
    if V:
        table = EdgeTable(faces, V) if table is None else table
        off, slots = vertex_slots_csr(faces, V)
        vf = (slots // 3).contiguous()
        border, boff, brows = boundary_edges_csr(table)
        L.launch("vertex_quadrics", dev, L.ptr(verts), V, L.ptr(faces), F, L.ptr(off), L.ptr(vf), vf.numel(), L.ptr(border),
                 border.shape[0], L.ptr(boff), L.ptr(brows), brows.numel(), float(boundary_weight), L.ptr(Q), L.ptr(counts))
    return (Q, int(counts.item())) if return_counts else Q


def _plane_quadric(p, w):
    """w * p p^T as the 10 entries, [N,10] (the kernel's products: (w p_i) p_j)."""
    wp = w[:, None] * p
    return torch.stack([wp[:, 0] * p[:, 0], wp[:, 0] * p[:, 1], wp[:, 0] * p[:, 2], wp[:, 0] * p[:, 3], wp[:, 1] * p[:, 1],
                        wp[:, 1] * p[:, 2], wp[:, 1] * p[:, 3], wp[:, 2] * p[:, 2], wp[:, 2] * p[:, 3], wp[:, 3] * p[:, 3]], 1)


def _row_sums(values, off, idx, V):
    """sum of values[idx] over every CSR row, in row order: [V,C]."""
    out = torch.zeros(V, values.shape[1], dtype=values.dtype, device=values.device)
    if values.shape[0] == 0 or idx.numel() == 0:
        return out
    nbr, _ = _padded(off, idx, V)
    for j in range(nbr.shape[1]):                                              # a fixed summation order
        col = nbr[:, j]
        out = out + torch.where((col >= 0)[:, None], values[col.clamp(min=0)], torch.zeros_like(out))
    return out


def vertex_quadrics_torch(verts, faces, table=None, boundary_weight=BOUNDARY_WEIGHT):
    """vertex_quadrics in plain torch (float64, the same sums in the same order; valid faces)."""
    V, dev = verts.shape[0], verts.device
    table = EdgeTable(faces, V) if table is None else table
    x = verts.double()
    a = x[faces[:, 0]]
    n = torch.cross(x[faces[:, 1]] - a, x[faces[:, 2]] - a, dim=1)
    length = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]).sqrt()
    good = (length > 0) & torch.isfinite(length)
    unit = n / torch.where(good, length, torch.ones_like(length))[:, None]
    d = -(unit[:, 0] * a[:, 0] + unit[:, 1] * a[:, 1] + unit[:, 2] * a[:, 2])
    area = torch.where(good, 0.5 * length, torch.zeros_like(length))
    per_face = torch.cat([_plane_quadric(torch.cat([unit, d[:, None]], 1), area), area[:, None]], 1)
    per_face = torch.where(good[:, None], per_face, torch.zeros_like(per_face))
    off, slots = vertex_slots_csr(faces, V)
    Q = _row_sums(per_face, off, slots // 3, V)
    border, boff, brows = boundary_edges_csr(table)
    if border.shape[0]:
        pa = x[border[:, 0]]
        e = x[border[:, 1]] - pa
        m = torch.cross(n[border[:, 2]], e, dim=1)
        length = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2]).sqrt()
        good = (length > 0) & torch.isfinite(length)
        unit = m / torch.where(good, length, torch.ones_like(length))[:, None]
        d = -(unit[:, 0] * pa[:, 0] + unit[:, 1] * pa[:, 1] + unit[:, 2] * pa[:, 2])
        w = float(boundary_weight) * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        per_edge = _plane_quadric(torch.cat([unit, d[:, None]], 1), torch.where(good, w, torch.zeros_like(w)))
        per_edge = torch.where(good[:, None], per_edge, torch.zeros_like(per_edge))
        Q = Q + torch.cat([_row_sums(per_edge, boff, brows, V), torch.zeros(V, 1, dtype=Q.dtype, device=dev)], 1)
    return Q


def _check_edges(Q, verts, edges, code=None, pos=None):
    E = edges.shape[0]
    if edges.dtype != torch.int64 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be int64 of shape [E,2]")
    if Q is not None and (Q.dtype != torch.float64 or Q.dim() != 2 or Q.shape != (verts.shape[0], 11)):
        raise ValueError("Q must be float64 of shape [V,11]")
    if code is not None and (code.dtype != torch.uint8 or code.shape != (E,)):
        raise ValueError("code must be uint8 of shape [E]")
    if pos is not None and (pos.dtype != torch.float32 or pos.shape != (E, 3)):
        raise ValueError("pos must be float32 of shape [E,3]")


def edge_collapse_cost(Q, verts, edges, code, reach=REACH):
    """recmv_edge_collapse_cost: (pos [E,3] f32, cost [E] float64, weight [E] float64) of the candidate edges [E,2] int64 with
    placement codes [E] uint8 (FREE, STAY_A, STAY_B); all CUDA."""
    L.require_cuda(Q, "Q")
    L.require_cuda(verts, "verts")
    L.require_cuda(edges, "edges")
    L.require_cuda(code, "code")
    _check_edges(Q, verts, edges, code=code)
    if verts.dtype != torch.float32:
        raise ValueError("verts must be float32")
    Q, verts, edges, code = Q.contiguous(), verts.contiguous(), edges.contiguous(), code.contiguous()
    E, dev = edges.shape[0], edges.device
    pos = L.scratch((E, 3), torch.float32, dev)
    cost, weight = L.scratch((E,), torch.float64, dev), L.scratch((E,), torch.float64, dev)
    if E:
        counts = torch.zeros(1, dtype=torch.int32, device=dev)
        L.launch("edge_collapse_cost", dev, L.ptr(Q), L.ptr(verts), verts.shape[0], L.ptr(edges), E, L.ptr(code), float(reach),
                 L.ptr(pos), L.ptr(cost), L.ptr(weight), L.ptr(counts))
    return pos, cost, weight


def _cost_at(q, p):
    """x^T q x at the points p [N,3] float64, the kernel's ten terms in its order, clamped at 0."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = (q[:, 0] * x * x + 2. * q[:, 1] * x * y + 2. * q[:, 2] * x * z + 2. * q[:, 3] * x + q[:, 4] * y * y + 2. * q[:, 5] * y * z
         + 2. * q[:, 6] * y + q[:, 7] * z * z + 2. * q[:, 8] * z + q[:, 9])
    return torch.where(c > 0, c, torch.zeros_like(c))


def edge_collapse_cost_torch(Q, verts, edges, code, reach=REACH):
    """edge_collapse_cost in plain torch (float64; valid edges)."""
    a, b = edges[:, 0], edges[:, 1]
    q = Q[a] + Q[b]
    pa, pb = verts[a].float(), verts[b].float()
    da, db = pa.double(), pb.double()
    mid = 0.5 * (da + db)
    e = db - da
    len2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
    c00, c01, c02 = q[:, 4] * q[:, 7] - q[:, 5] * q[:, 5], q[:, 2] * q[:, 5] - q[:, 1] * q[:, 7], q[:, 1] * q[:, 5] - q[:, 2] * q[:, 4]
    c11, c12, c22 = q[:, 0] * q[:, 7] - q[:, 2] * q[:, 2], q[:, 1] * q[:, 2] - q[:, 0] * q[:, 5], q[:, 0] * q[:, 4] - q[:, 1] * q[:, 1]
    det = q[:, 0] * c00 + q[:, 1] * c01 + q[:, 2] * c02
    solvable = (det != 0) & torch.isfinite(det)
    den = torch.where(solvable, det, torch.ones_like(det))
    r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
    s = torch.stack([(c00 * r0 + c01 * r1 + c02 * r2) / den, (c01 * r0 + c11 * r1 + c12 * r2) / den,
                     (c02 * r0 + c12 * r1 + c22 * r2) / den], 1)
    solvable &= (s.abs() < 3.0e38).all(1)
    sf = torch.where(solvable[:, None], s, mid).float()
    ds = sf.double() - mid
    solvable &= (ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1] + ds[:, 2] * ds[:, 2]) <= (float(reach) * float(reach)) * len2
    free = (code != STAY_A) & (code != STAY_B)
    # the candidates in order; a later one wins only when it is strictly cheaper
    best, best_cost = pa, torch.full_like(det, float("inf"))
    for cand, allowed in ((sf, free & solvable), (pa, code != STAY_B), (pb, code != STAY_A), (mid.float(), free)):
        c = _cost_at(q, cand.double())
        take = allowed & (c < best_cost)
        best = torch.where(take[:, None], cand, best)
        best_cost = torch.where(take, c, best_cost)
    return best, best_cost, q[:, 10].clone()


def collapse_flip_check(verts, faces, edges, pos, vf=None):
    """recmv_collapse_flip_check: ok [E] bool of the collapses of edges [E,2] int64 to pos [E,3] f32 on verts [V,3] f32 /
    faces [F,3] int64 (CUDA); vf: (offsets, faces) int64 of the vertex -> face table, built when absent."""
    verts, faces = check_mesh(verts, faces)
    L.require_cuda(edges, "edges")
    L.require_cuda(pos, "pos")
    _check_edges(None, verts, edges, pos=pos)
    edges, pos = edges.contiguous(), pos.contiguous()
    V, F, E, dev = verts.shape[0], faces.shape[0], edges.shape[0], verts.device
    ok = L.scratch((E,), torch.uint8, dev)
    if E:
        if vf is None:
            off, slots = vertex_slots_csr(faces, V)
            vf = (off, slots // 3)
        off, idx = vf[0].contiguous(), vf[1].contiguous()
        L.launch("collapse_flip_check", dev, L.ptr(verts), V, L.ptr(faces), F, L.ptr(off), L.ptr(idx), idx.numel(), L.ptr(edges), E,
                 L.ptr(pos), L.ptr(ok))
    return ok.bool()


# ------------------------------------------------------------------------------------------------- the driver
@torch.no_grad()
def simplify(verts, faces, target_faces=None, ratio=None, max_error=None, boundary_weight=BOUNDARY_WEIGHT, use_kernels=True,
             log=None):
    """Quadric-error simplification of one triangle mesh (verts [V,3], faces [F,3] int64, one device): (verts' f32, faces',
    info).  Give `target_faces` or `ratio` (the target is round(ratio * F)), and / or `max_error`, the largest root of
    cost / weight a collapse may have (a length; alone it collapses until nothing cheaper is left).  The mesh must be
    edge-manifold with valid faces (ValueError otherwise); vertices no face uses are dropped.  The result never has fewer than
    the target's faces and ends with the target or one more unless info['stopped'] says why not: 'target', 'no_candidates',
    'max_error' (only the cap refused what was left) or 'max_rounds'.  info also has rounds, collapses, faces_before / _after,
    vertices_before / _after (before: after dropping unused vertices), target_faces, max_cost (the largest accepted cost) and
    max_error (the largest accepted root of cost / weight).  `use_kernels=False`: the same driver on the float64 restatements
    (CPU tensors too).  The module docstring has the definitions."""
    if target_faces is not None and ratio is not None:
        raise ValueError("simplify: give target_faces or ratio, not both")
    if target_faces is None and ratio is None and max_error is None:
        raise ValueError("simplify: give target_faces, ratio or max_error")
    if target_faces is not None and int(target_faces) < 0:
        raise ValueError("simplify: target_faces must not be negative")
    if ratio is not None and not (0. <= float(ratio) <= 1.):
        raise ValueError("simplify: ratio must be in [0, 1]")
    if max_error is not None and not (float(max_error) >= 0. and math.isfinite(float(max_error))):
        raise ValueError("simplify: max_error must be finite and not negative")
    if not (float(boundary_weight) >= 0. and math.isfinite(float(boundary_weight))):
        raise ValueError("simplify: boundary_weight must be finite and not negative")
    verts, faces = check_mesh(verts, faces, cuda=use_kernels, float_verts=True)
    verts = verts.float()
    V, dev = verts.shape[0], faces.device
    if faces.shape[0]:
        lo, hi = (int(x) for x in torch.aminmax(faces))
        distinct = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])
        if lo < 0 or hi >= V or not bool(distinct.all()):
            raise ValueError("simplify: the mesh has invalid faces (an index outside [0, %d) or repeated); %s" % (V, _HINT))
    verts, faces, _ = compact(verts, faces)
    table = EdgeTable(faces, verts.shape[0])
    if table.E and int(table.count.max()) > 2:
        raise ValueError("simplify: the mesh must be edge-manifold (%d edges have more than two faces); %s"
                         % (int(table.nonmanifold_edge.sum()), _HINT))
    F0, V0 = faces.shape[0], verts.shape[0]
    target = int(target_faces) if target_faces is not None else (int(float(ratio) * F0 + 0.5) if ratio is not None else 0)
    cap2 = None if max_error is None else float(max_error) ** 2
    if use_kernels:
        Q = vertex_quadrics(verts, faces, table, boundary_weight)
    else:
        Q = vertex_quadrics_torch(verts, faces, table, boundary_weight)
    rounds = collapses = 0
    max_cost = max_len2 = 0.
    stopped = None
    while stopped is None:
        budget = faces.shape[0] - target
        if budget <= 0 or faces.shape[0] == 0:
            stopped = 'target'
            break
        if rounds >= MAX_ROUNDS:
            stopped = 'max_rounds'
            break
        topo = _Topo(faces, verts.shape[0])
        a, b = topo.edges[:, 0], topo.edges[:, 1]
        ba, bb = topo.bvert[a], topo.bvert[b]
        cand = ~(~topo.bedge & ba & bb)                                        # never an interior edge between two boundary vertices
        if budget == 1:
            cand &= topo.bedge                                                 # only a boundary collapse takes one face
        ci = cand.nonzero().squeeze(1)
        if ci.numel() == 0:
            stopped = 'target' if budget == 1 else 'no_candidates'
            break
        ca, cb, bnd = a[ci], b[ci], topo.bedge[ci]
        code = torch.where(bnd | (ba[ci] & ~bb[ci]), STAY_A, torch.where(bb[ci] & ~ba[ci], STAY_B, FREE)).to(torch.uint8)
        edges = torch.stack([ca, cb], 1).contiguous()
        if use_kernels:
            pos, cost, weight = edge_collapse_cost(Q, verts, edges, code)
            flip_ok = collapse_flip_check(verts, faces, edges, pos, (topo.vf[0], topo.vf[1] // 3))
        else:
            pos, cost, weight = edge_collapse_cost_torch(Q, verts, edges, code)
            flip_ok = _flip_ok(verts.double(), faces, topo, ca, cb, pos.double())
        ok = _link_ok(topo, ca, cb, bnd) & flip_ok
        # the link condition's other half (the links share no edge) fails on a closed manifold only for a tetrahedron's edges: two
        # interior vertices of valence 3
        ok &= ba[ci] | bb[ci] | (topo.valence[ca] != 3) | (topo.valence[cb] != 3)
        ok &= ~bnd | (_boundary_loop_length(faces, topo)[ci] > 3)
        capped = ok & (cost > cap2 * weight) if cap2 is not None else torch.zeros_like(ok)
        n_ok = int(ok.sum())
        ok &= ~capped
        vi = ok.nonzero().squeeze(1)
        if vi.numel() == 0:
            stopped = 'target' if budget == 1 else ('max_error' if n_ok else 'no_candidates')
            break
        # the cheapest valid candidates, as many as ROUND_SHARE of the budget allows (at least one): sorted by (cost, edge id)
        order = vi[torch.sort(cost[vi], stable=True)[1]]
        takes = torch.where(bnd[order], 1, 2)
        allow = max(int(budget * ROUND_SHARE), int(takes[0]))                  # (never above the budget: budget 1 has boundary edges only)
        order = order[torch.cumsum(takes, 0) <= allow]
        rank = torch.arange(order.shape[0], device=dev)
        pick = order[_independent(topo, ca[order], cb[order], rank)]
        pa, pb = ca[pick], cb[pick]
        c, w = cost[pick], weight[pick]
        max_cost = max(max_cost, float(c.max()))
        max_len2 = max(max_len2, float(torch.where(w > 0, c / w, torch.zeros_like(c)).max()))
        Q = Q.clone()
        Q[pa] = Q[pa] + Q[pb]
        verts, faces = _merge(verts, faces, pa, pb, pos[pick])
        verts, faces, vmap = compact(verts, faces)
        Q = Q[vmap >= 0]
        rounds += 1
        collapses += int(pick.shape[0])
        if log is not None:
            log("simplify round %d: %d of %d candidates collapsed, %d faces left (target %d), largest cost %.3g"
                % (rounds, pick.shape[0], ci.shape[0], faces.shape[0], target, float(c.max())))
    info = {'stopped': stopped, 'rounds': rounds, 'collapses': collapses, 'faces_before': F0, 'faces_after': faces.shape[0],
            'vertices_before': V0, 'vertices_after': verts.shape[0], 'target_faces': target, 'max_cost': max_cost,
            'max_error': math.sqrt(max_len2)}
    return verts.contiguous(), faces.contiguous(), info
