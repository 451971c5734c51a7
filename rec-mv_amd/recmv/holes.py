"""Hole filling (csrc/hole_fill.hip) — an ADDITION to the reference, which never closes a mesh: the stage between
recmv.repair and every stage that needs a closed surface (voxelize.remesh, the volume of metrics).  Garments are open by
design, so which boundary loops are holes is a rule of the caller's: max_edges, max_perimeter, keep_largest.

  find_loops          the oriented boundary loops of an edge-manifold, consistently oriented mesh, and a table of them
  triangulate_loops   the minimum-area triangulation of many loops in one call (recmv_hole_triangulate)
  fill                find, select, triangulate, check, stitch; optionally refine and fair the patches
  info_json           the JSON-able part of fill's info

Definitions (INTEGRATION.md §5 repeats them; tests/hole_fill_reference.py restates them in numpy):
  input             verts [V,3] f32, faces [F,3] int64.  Invalid faces (topology's definition) take no part.  An edge with more
                    than two faces, or an edge whose two faces traverse it in one direction, is a ValueError that names
                    repair.repair.
  loops             every boundary half-edge a -> b, in the direction its one face traverses it, is an outgoing edge of a.  A
                    loop starts at the lowest vertex id that still has an unwalked outgoing edge, always takes the unwalked
                    outgoing edge to the lowest vertex id, and ends when it is back at its start: l_0 .. l_{n-1}.  Loops are
                    numbered in the order they are found, which is by starting vertex.  The walk runs on the host after ONE
                    read-back of the boundary half-edges (ends, face, float64 length).
  perimeter         the float64 sum, in loop order from 0., of the edge lengths sqrt((dx*dx + dy*dy) + dz*dz), d = p_b - p_a in
                    float64 from the f32 coordinates.
  status            'nonsimple': the loop passes a vertex with any number of boundary edges other than two (where loops
                    touch; after repair.split_nonmanifold there is none).  'duplicate': three vertices that already form a face
                    — the loop's three half-edges belong to one face, and the cap would be its mirror image.  Then, in this
                    order and each among the loops still open: 'max_edges' (more than max_edges vertices), 'max_perimeter'
                    (perimeter above max_perimeter), 'keep_largest' (the K loops of longest perimeter, on a tie the lower loop
                    number), 'too_large' (more than MAX_LOOP_EDGES vertices).  After the triangulation: 'nonfinite' (the total
                    is not finite: a point of the loop is not), 'chord_conflict' (a diagonal of the patch already is an edge
                    of the mesh: filling would make an edge with three faces).  Everything else is 'filled'.
  triangulation     points p_i = verts[l_i], float64 from the f32 coordinates, nothing contracted:
                      W[i][i+1] = 0;  W[i][j] = min over i < k < j of (W[i][k] + W[k][j]) + A(i,k,j)      (j - i >= 2)
                      u = p_k - p_i, v = p_j - p_i
                      cx = u.y * v.z - u.z * v.y;  cy = u.z * v.x - u.x * v.z;  cz = u.x * v.y - u.y * v.x
                      A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz)
                    A candidate wins only when it is smaller than the best so far, k ascending from +inf: ties go to the lowest
                    k, NaN never wins, an entry without a winner is +inf with k = i + 1.  patch_area is W[0][n-1].
  faces             n - 2 per loop in pre-order of the split tree — the triangle of (i, j), then everything of (i, k), then
                    everything of (k, j) — each (l_j, l_k, l_i): the reverse of the loop, so the patch agrees with the faces
                    around it.
  fill              verts' begins with verts bit for bit, faces' with faces; the patches follow loop by loop (face_start,
                    faces_added) and, with refine, so do the new vertices (verts_added).  With no loop filled the input comes
                    back.
  refine            per loop Lbar = perimeter / n.  A round splits every interior patch edge longer than 4/3 Lbar at its
                    midpoint (f32: (a + b) * 0.5), all of them at once with iso_remesh's one / two / three-split face
                    templates, then flips, in face- and vertex-disjoint sets, interior patch edges whose opposite angles sum
                    to more than pi (cot a + cot b < -1e-9 in float64) when the new edge is no edge yet and neither new face
                    folds over.  It stops when no interior edge is too long (refine_rounds) or after MAX_REFINE_ROUNDS
                    (refine_capped).  A split halves an edge, so 16 rounds reach edges 2^16 Lbar long.  Border edges of a
                    patch are never split or flipped.
  fair              smooth.smooth(method='laplacian', weights='uniform', boundary='fixed', fixed=every vertex that is not new).

MAX_LOOP_EDGES and the workspace: a loop of n vertices outside LDS costs n(n-1)/2 * 18 B (W and its transpose in float64, the
split table in u16) + 12 n B: 9.4 MB at n = 1024, 151 MB at the cap of 4096 (where the DP weighs n^3/6 = 1.1e10 candidates).
"""
import ctypes as C

import torch

from . import _lib as L
from .connectivity import EdgeTable
from .mesh_args import check_mesh, check_points, info_json  # noqa: F401  (info_json: the JSON-able part of fill's info)
from .topology import valid_faces

MAX_LOOP_EDGES = 4096                                      # csrc/hole_fill.hip: kHoleMaxN
LDS_MAX_EDGES = 85                                         # csrc/hole_fill.hip: kHoleLdsMaxN (64 KiB of LDS a loop)
AUTO_MAX_EDGES = 64                                        # csrc/hole_fill.hip: kHoleAutoMaxN (where 'auto' leaves LDS: measured)
MAX_REFINE_ROUNDS = 16
MAX_FLIP_PASSES = 8
REFINE_RATIO = 4. / 3.
ROUTES = {'auto': 0, 'lds': 1, 'global': 2}
STATUSES = ('filled', 'nonsimple', 'duplicate', 'max_edges', 'max_perimeter', 'keep_largest', 'too_large', 'nonfinite',
            'chord_conflict')


def _find(verts, faces):
    """(loops: lists of vertex ids on the host, table, edge keys V * lo + hi of the valid faces, sorted)."""
    V, dev = verts.shape[0], faces.device
    vf = faces[valid_faces(faces, V)].contiguous() if faces.shape[0] else faces
    table = EdgeTable(vf, V)
    keys = table.edges[:, 0] * max(V, 1) + table.edges[:, 1]
    if table.E and int(table.count.max()) > 2:
        raise ValueError("holes: the mesh is not edge-manifold (an edge has %d faces): repair.repair mends it"
                         % int(table.count.max()))
    fe = table.face_to_edge.reshape(-1)
    cnt = table.count[fe]
    two = (cnt == 2).nonzero().squeeze(1)
    if two.numel():
        forward = table.forward.reshape(-1)
        two = two[torch.sort(fe[two], stable=True)[1]]
        if bool((forward[two[0::2]] == forward[two[1::2]]).any()):
            raise ValueError("holes: the mesh is not consistently oriented (two faces traverse an edge in one direction): "
                             "repair.repair orients it")
    slots = (cnt == 1).nonzero().squeeze(1)
    loops, out = [], {'edges': [], 'perimeter': [], 'status': []}
    if slots.numel() == 0:
        return loops, out, keys
    fv = vf.reshape(-1)
    f, k = slots // 3, slots % 3
    a, b = fv[3 * f + (k + 1) % 3], fv[3 * f + (k + 2) % 3]
    d = verts[b].double() - verts[a].double()
    length = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()
    rows = torch.stack([a.double(), b.double(), f.double(), length], 1).cpu().tolist()               # the read-back
    succ, degree = {}, {}
    for x, y, face, ln in rows:
        x, y = int(x), int(y)
        succ.setdefault(x, []).append((y, int(face), ln))
        degree[x] = degree.get(x, 0) + 1
        degree[y] = degree.get(y, 0) + 1
    for x in succ:
        succ[x].sort()
    for start in sorted(succ):
        while succ[start]:
            loop, faces_of, per, cur = [start], [], 0., start
            while True:
                nxt, face, ln = succ[cur].pop(0)
                faces_of.append(face)
                per = per + ln
                if nxt == start:
                    break
                loop.append(nxt)
                cur = nxt
            status = 'open'
            if any(degree[v] != 2 for v in loop):
                status = 'nonsimple'
            elif len(loop) == 3 and faces_of[0] == faces_of[1] == faces_of[2]:
                status = 'duplicate'
            loops.append(loop)
            out['edges'].append(len(loop))
            out['perimeter'].append(per)
            out['status'].append(status)
    return loops, out, keys


def _flat(loops, dev):
    offsets = [0]
    for lp in loops:
        offsets.append(offsets[-1] + len(lp))
    lv = torch.tensor([v for lp in loops for v in lp], dtype=torch.int64).to(dev)
    return lv, torch.tensor(offsets, dtype=torch.int64)


@torch.no_grad()
def find_loops(verts, faces):
    """(loop_verts [total] int64, loop_offsets [L+1] int64, table) of verts [V,3] f32 / faces [F,3] int64: the oriented
    boundary loops, flat, on the mesh's device, and per loop table['edges'], table['perimeter'] (float64) and table['status']
    ('open' | 'nonsimple' | 'duplicate') before any selection; the module docstring has the definitions.  Plain torch and one
    read-back: it runs where the tensors live.  ValueError for a mesh that is not edge-manifold or not consistently oriented."""
    verts, faces = check_mesh(verts, faces, cuda=False, cap31=True)
    loops, table, _ = _find(verts, faces)
    lv, lo = _flat(loops, faces.device)
    return lv, lo.to(faces.device), table


@torch.no_grad()
def triangulate_loops(verts, loop_verts, loop_offsets, route='auto'):
    """recmv_hole_triangulate: (faces [total - 2 L, 3] int64, weight [L] float64), both CUDA, of the loops loop_verts [total]
    int64 (CUDA) / loop_offsets [L+1] int64 (CUDA or host; the sizes are needed on the host, so a CUDA tensor is read back)
    over verts [V,3] f32 (CUDA).  route 'auto' | 'lds' | 'global': the same bits; 'auto' keeps a loop of at most AUTO_MAX_EDGES
    vertices in LDS, 'lds' refuses a loop of more than LDS_MAX_EDGES."""
    if route not in ROUTES:
        raise ValueError("route must be one of %s" % (sorted(ROUTES),))
    verts = check_points(verts, "verts", shape="[V,3]")
    L.require_cuda(loop_verts, "loop_verts")
    if loop_verts.dtype != torch.int64 or loop_verts.dim() != 1 or loop_offsets.dtype != torch.int64 or loop_offsets.dim() != 1:
        raise ValueError("loop_verts and loop_offsets must be int64 vectors")
    if loop_offsets.shape[0] < 1:
        raise ValueError("loop_offsets must have L + 1 entries")
    dev = verts.device
    loop_verts = loop_verts.contiguous()
    host = loop_offsets.cpu().contiguous()
    n_loops = host.shape[0] - 1
    if int(host[0]) != 0 or int(host[-1]) != loop_verts.shape[0]:
        raise ValueError("loop_offsets must run from 0 to len(loop_verts)")
    faces = L.scratch((loop_verts.shape[0] - 2 * n_loops if n_loops else 0, 3), torch.int64, dev)
    weight = L.scratch((n_loops,), torch.float64, dev)
    if n_loops == 0:
        return faces, weight
    lib = L.lib()
    hp = C.c_void_p(host.data_ptr())
    ws_bytes = lib.recmv_hole_triangulate_workspace_bytes(hp, n_loops, ROUTES[route])
    if ws_bytes < 0:
        raise ValueError("triangulate_loops: " + lib.recmv_last_error().decode())
    ws = L.workspace(ws_bytes, dev, "hole_triangulate_workspace_bytes") if ws_bytes else None
    offsets_dev = host.to(dev) if not loop_offsets.is_cuda else loop_offsets.contiguous()
    L.launch("hole_triangulate", dev, L.ptr(verts), verts.shape[0], L.ptr(loop_verts), hp, L.ptr(offsets_dev), n_loops,
             L.ptr(faces), L.ptr(weight), L.ptr(ws), ws_bytes, ROUTES[route])
    return faces, weight


def select(table, max_edges=None, max_perimeter=None, keep_largest=0):
    """The status of every loop of a find_loops table after the selection, 'candidate' for the loops to triangulate; the module
    docstring has the order.  Plain Python."""
    status = ['candidate' if s == 'open' else s for s in table['status']]
    n, per = table['edges'], table['perimeter']
    idx = range(len(status))
    if max_edges is not None:
        for l in idx:
            if status[l] == 'candidate' and n[l] > max_edges:
                status[l] = 'max_edges'
    if max_perimeter is not None:
        for l in idx:
            if status[l] == 'candidate' and per[l] > max_perimeter:
                status[l] = 'max_perimeter'
    if keep_largest:
        for l in sorted((l for l in idx if status[l] == 'candidate'), key=lambda l: (-per[l], l))[:int(keep_largest)]:
            status[l] = 'keep_largest'
    for l in idx:
        if status[l] == 'candidate' and n[l] > MAX_LOOP_EDGES:
            status[l] = 'too_large'
    return status


# ------------------------------------------------------------------------------------------------- refinement
def _edge_len(verts, e):
    d = verts[e[:, 0]].double() - verts[e[:, 1]].double()
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()


def _edge_loop(table, face_loop):
    """The loop of every edge of a patch EdgeTable (a patch's faces all carry its loop)."""
    out = torch.zeros(table.E, dtype=torch.int64, device=face_loop.device)
    out[table.face_to_edge.reshape(-1)] = face_loop.repeat_interleave(3)
    return out


def _too_long(verts, table, face_loop, limit):
    interior = table.count == 2
    return interior & (_edge_len(verts, table.edges) > limit[_edge_loop(table, face_loop)])


def _split_long(verts, pf, pl, vloop, long_, table):
    """Split the flagged edges of the patch faces pf (loops pl) at their midpoints, all at once: iso_remesh._split's
    templates.  Returns (verts', pf', pl', vloop')."""
    dev, V = pf.device, verts.shape[0]
    e = table.edges
    n = int(long_.sum())
    new_id = torch.full((table.E,), -1, dtype=torch.int64, device=dev)
    new_id[long_] = V + torch.arange(n, device=dev)
    mid = (verts[e[long_, 0]] + verts[e[long_, 1]]) * 0.5
    verts = torch.cat([verts, mid], 0)
    vloop = torch.cat([vloop, _edge_loop(table, pl)[long_]])
    m = new_id[table.face_to_edge]                                            # midpoint opposite each corner, or -1
    ns = (m >= 0).sum(1)
    special = torch.where(ns == 2, (m < 0).to(torch.int64).argmax(1), (m >= 0).to(torch.int64).argmax(1))
    r = (special[:, None] + torch.arange(3, device=dev)[None]) % 3
    p, q = pf.gather(1, r), m.gather(1, r)
    p0, p1, p2, m0, m1, m2 = p[:, 0], p[:, 1], p[:, 2], q[:, 0], q[:, 1], q[:, 2]
    c0, c1, c2, c3 = ns == 0, ns == 1, ns == 2, ns == 3
    l1 = _edge_len(verts, torch.stack([m2.clamp(min=0), p2], 1))             # diagonal (m2, p2)
    l2 = _edge_len(verts, torch.stack([p1, m1.clamp(min=0)], 1))             # diagonal (p1, m1)
    use1 = (l1 < l2) | ((l1 == l2) & (torch.minimum(m2, p2) < torch.minimum(p1, m1)))
    d1, d2 = c2 & use1, c2 & ~use1
    parts = [(pf, c0), (torch.stack([p0, p1, m0], 1), c1), (torch.stack([p0, m0, p2], 1), c1),
             (torch.stack([p0, m2, m1], 1), c2), (torch.stack([m2, p1, p2], 1), d1), (torch.stack([m2, p2, m1], 1), d1),
             (torch.stack([p1, p2, m1], 1), d2), (torch.stack([p1, m1, m2], 1), d2),
             (torch.stack([p0, m2, m1], 1), c3), (torch.stack([p1, m0, m2], 1), c3), (torch.stack([p2, m1, m0], 1), c3),
             (torch.stack([m0, m1, m2], 1), c3)]
    return verts, torch.cat([x[k] for x, k in parts], 0), torch.cat([pl[k] for _, k in parts], 0), vloop


def _cot(verts, apex, u, w):
    """cot of the angle at apex between the edges to u and w, float64."""
    a, b = verts[u].double() - verts[apex].double(), verts[w].double() - verts[apex].double()
    return (a * b).sum(1) / torch.cross(a, b, dim=1).norm(dim=1).clamp(min=1e-300)


def _flip_pass(verts, pf, base_keys, V0):
    """One set of face- and vertex-disjoint Delaunay flips of interior patch edges; (pf', flips)."""
    dev, V = pf.device, verts.shape[0]
    table = EdgeTable(pf, V)
    ei = (table.count == 2).nonzero().squeeze(1)
    if ei.numel() == 0:
        return pf, 0
    F = pf.shape[0]
    fe = table.face_to_edge.reshape(-1)
    slots = torch.arange(3 * F, device=dev)
    order = torch.argsort(fe * (3 * F) + slots)
    start = torch.cumsum(table.count, 0) - table.count
    s0, s1 = order[start[ei]], order[start[ei] + 1]
    fv = pf.reshape(-1)
    f0, k0, f1 = s0 // 3, s0 % 3, s1 // 3
    a, b = fv[3 * f0 + (k0 + 1) % 3], fv[3 * f0 + (k0 + 2) % 3]               # f0 = (a, b, c), f1 = (b, a, d)
    c, d = fv[s0], fv[s1]
    ok = (_cot(verts, c, a, b) + _cot(verts, d, a, b)) < -1e-9
    nk = torch.minimum(c, d) * V + torch.maximum(c, d)
    pkeys = table.edges[:, 0] * V + table.edges[:, 1]
    old = torch.minimum(c, d) * V0 + torch.maximum(c, d)                      # the key among the mesh's own edges
    ok &= (c != d) & ~torch.isin(nk, pkeys) & ~(torch.isin(old, base_keys) & (c < V0) & (d < V0))
    x = verts.double()
    n0 = torch.cross(x[b] - x[a], x[c] - x[a], dim=1)
    n1 = torch.cross(x[a] - x[b], x[d] - x[b], dim=1)
    mean = n0 / n0.norm(dim=1, keepdim=True).clamp(min=1e-300) + n1 / n1.norm(dim=1, keepdim=True).clamp(min=1e-300)
    na = torch.cross(x[a] - x[c], x[d] - x[c], dim=1)
    nb = torch.cross(x[b] - x[d], x[c] - x[d], dim=1)
    ok &= ((na * mean).sum(1) > 0) & ((nb * mean).sum(1) > 0)
    oi = ok.nonzero().squeeze(1)
    if oi.numel() == 0:
        return pf, 0
    key, f0, f1, a, b, c, d, nk = ei[oi], f0[oi], f1[oi], a[oi], b[oi], c[oi], d[oi], nk[oi]
    vm = torch.full((V,), table.E, dtype=torch.int64, device=dev)
    vm = vm.scatter_reduce(0, torch.cat([a, b, c, d]), key.repeat(4), reduce="amin")
    pick = (vm[a] == key) & (vm[b] == key) & (vm[c] == key) & (vm[d] == key)
    if not bool(pick.any()):
        return pf, 0
    pf = pf.clone()
    pf[f0[pick]] = torch.stack([c, a, d], 1)[pick]
    pf[f1[pick]] = torch.stack([d, b, c], 1)[pick]
    return pf, int(pick.sum())


def _refine(verts, pf, pl, lbar, base_keys):
    """The refinement of the module docstring on the patch faces pf [T,3] with loops pl [T] over verts [V,3] f32; lbar [L]
    float64 per loop, base_keys the sorted edge keys of the mesh without the patches.  Plain torch on the tensors' device.
    (verts', pf', pl', loop of every new vertex, rounds, capped)."""
    V0, dev = verts.shape[0], pf.device
    limit = lbar * REFINE_RATIO
    vloop = torch.zeros(0, dtype=torch.int64, device=dev)
    rounds, capped = 0, False
    while True:
        table = EdgeTable(pf, verts.shape[0])
        long_ = _too_long(verts, table, pl, limit)
        if not bool(long_.any()):
            break
        if rounds == MAX_REFINE_ROUNDS:
            capped = True
            break
        rounds += 1
        verts, pf, pl, vloop = _split_long(verts, pf, pl, vloop, long_, table)
        for _ in range(MAX_FLIP_PASSES):
            pf, flips = _flip_pass(verts, pf, base_keys, V0)
            if flips == 0:
                break
    return verts, pf, pl, vloop, rounds, capped


# ------------------------------------------------------------------------------------------------- the stage
@torch.no_grad()
def fill(verts, faces, max_edges=None, max_perimeter=None, keep_largest=0, refine=False, fair_iterations=0, route='auto'):
    """Close the holes of verts [V,3] f32 / faces [F,3] int64 (CUDA) — (verts', faces', info); the module docstring has the
    definitions.  info: the counts 'loops', 'filled' and one per other status of STATUSES; per loop the lists 'edges',
    'perimeter', 'status', 'patch_area' (None unless filled), 'faces_added', 'verts_added', 'face_start' (-1 unless filled);
    'refine_rounds', 'refine_capped'.  RuntimeError for CPU tensors, ValueError for a mesh that is not edge-manifold or not
    consistently oriented, and for fair_iterations without refine (there is no new vertex to move)."""
    verts, faces = check_mesh(verts, faces, cap31=True)
    if route not in ROUTES:
        raise ValueError("route must be one of %s" % (sorted(ROUTES),))
    if max_edges is not None and int(max_edges) < 0 or int(keep_largest) < 0 or int(fair_iterations) < 0:
        raise ValueError("max_edges, keep_largest and fair_iterations must not be negative")
    if max_perimeter is not None and not float(max_perimeter) >= 0.:
        raise ValueError("max_perimeter must not be negative")
    if fair_iterations and not refine:
        raise ValueError("fair_iterations needs refine=True: without it a patch has no vertex of its own to move")
    V, F, dev = verts.shape[0], faces.shape[0], faces.device
    loops, table, base_keys = _find(verts, faces)
    status = select(table, max_edges, max_perimeter, keep_largest)
    n_loops = len(loops)
    info = {'loops': n_loops, 'edges': table['edges'], 'perimeter': table['perimeter'], 'status': status,
            'patch_area': [None] * n_loops, 'faces_added': [0] * n_loops, 'verts_added': [0] * n_loops,
            'face_start': [-1] * n_loops, 'refine_rounds': 0, 'refine_capped': False}
    cand = [l for l in range(n_loops) if status[l] == 'candidate']
    pf = torch.zeros((0, 3), dtype=torch.int64, device=dev)
    new_verts = verts[:0]
    if cand:
        lv, lo = _flat([loops[l] for l in cand], dev)
        tri, weight = triangulate_loops(verts, lv, lo, route=route)
        n = lo[1:] - lo[:-1]
        face_loop = torch.repeat_interleave(torch.arange(len(cand)), n - 2).to(dev)          # position in cand
        # a diagonal (an edge two patch faces share; the loops are vertex-disjoint) that already is an edge of the mesh
        ptab = EdgeTable(tri, V)
        diag = ptab.count == 2
        hit = diag & torch.isin(ptab.edges[:, 0] * max(V, 1) + ptab.edges[:, 1], base_keys)
        conflict = torch.zeros(len(cand), dtype=torch.bool, device=dev)
        conflict[_edge_loop(ptab, face_loop)[hit]] = True
        weight_h, conflict_h = weight.cpu().tolist(), conflict.cpu().tolist()                 # the read-back
        keep = []
        for c, l in enumerate(cand):
            if not (weight_h[c] - weight_h[c] == 0.):
                status[l] = 'nonfinite'
            elif conflict_h[c]:
                status[l] = 'chord_conflict'
            else:
                status[l] = 'filled'
                info['patch_area'][l] = weight_h[c]
                keep.append(c)
        keep_t = torch.zeros(len(cand), dtype=torch.bool)
        keep_t[keep] = True
        fk = keep_t.to(dev)[face_loop]
        pf, pl = tri[fk], torch.tensor(cand, dtype=torch.int64, device=dev)[face_loop[fk]]   # pl: loop numbers
        if refine and keep:
            lbar = torch.tensor([table['perimeter'][l] / table['edges'][l] for l in range(n_loops)], dtype=torch.float64,
                                device=dev)
            allv, pf, pl, vloop, info['refine_rounds'], info['refine_capped'] = _refine(verts, pf, pl, lbar, base_keys)
            # loop by loop: the faces by (loop, position), the new vertices by (loop, creation)
            order = torch.sort(pl, stable=True)[1]
            pf, pl = pf[order], pl[order]
            vorder = torch.sort(vloop, stable=True)[1]
            rank = torch.empty_like(vorder)
            rank[vorder] = torch.arange(vorder.shape[0], device=dev)
            remap = torch.cat([torch.arange(V, device=dev), V + rank])
            pf = remap[pf]
            new_verts = allv[V:][vorder]
            added = torch.bincount(vloop, minlength=n_loops).cpu().tolist()
            info['verts_added'] = [int(x) for x in added]
        counts = torch.bincount(pl, minlength=n_loops).cpu().tolist() if pf.shape[0] else [0] * n_loops
        at = F
        for l in range(n_loops):
            if status[l] == 'filled':
                info['faces_added'][l] = int(counts[l])
                info['face_start'][l] = at
                at += int(counts[l])
    for s in STATUSES:
        info[s] = sum(1 for x in status if x == s)
    if pf.shape[0] == 0:
        return verts, faces, info
    out_v = torch.cat([verts, new_verts]).contiguous() if new_verts.shape[0] else verts
    out_f = torch.cat([faces, pf]).contiguous()
    if fair_iterations and new_verts.shape[0]:
        from . import smooth
        fixed = torch.ones(out_v.shape[0], dtype=torch.bool, device=dev)
        fixed[V:] = False
        faired, _ = smooth.smooth(out_v, out_f, method='laplacian', iterations=int(fair_iterations), weights='uniform',
                                  boundary='fixed', fixed=fixed)
        out_v = torch.cat([verts, faired[V:].to(torch.float32)]).contiguous()
    return out_v, out_f, info
