"""Isotropic remeshing and Loop subdivision: the two MeshLab filters of the reference's `remesh_garment_mesh`
(engineer/utils/garment_structure.py:440-458, pymeshlab `meshing_isotropic_explicit_remeshing` then
`meshing_surface_subdivision_loop`), which `registration` runs between the coarse and the refine NR-ICP pass (:2477).

"iso-remesh" throughout, so that it is not mistaken for the marching-cubes re-extraction of the training loop.

isotropic_remesh   Botsch-Kobbelt (vcg::tri::IsotropicRemeshing): per iteration split long edges, collapse short ones,
                   flip towards the target valence, relax tangentially and project onto the frozen input surface.
loop_subdivide     Loop's original scheme with edge_subdivide's connectivity and face order.

The topology work is plain torch on the mesh's device with integer keys only (sort / unique / scatter_reduce / bincount),
so it does not depend on thread timing.  The geometry has a HIP kernel (csrc/iso_remesh.hip) and a plain-torch
restatement each; `use_kernels=False` (CPU tensors, register_fl.py --torch-path) takes the restatements.
"""
import math

import torch

from . import _lib as L
from . import nricp
from .connectivity import EdgeTable, compact, neighbours_csr, vertex_slots_csr
from .mesh_args import check_mesh, check_points

MAX_PASSES = 16                    # split passes, collapse rounds and flip rounds per iteration


# ------------------------------------------------------------------------------------------------- kernels
def closest_point(p, verts, faces):
    """Exact closest point on the mesh (verts [V,3] f32, faces [F,3] int64, CUDA) of every row of p [P,3] f32:
    (face [P] int64, point [P,3] f32, squared distance [P] f32); ties go to the lowest face id."""
    p = check_points(p, "p")
    verts, faces = check_mesh(verts, faces, allow_empty=False)
    P, dev = p.shape[0], p.device
    face = L.scratch((P,), torch.int64, dev)
    point = L.scratch((P, 3), torch.float32, dev)
    dist2 = L.scratch((P,), torch.float32, dev)
    if P == 0:
        return face, point, dist2
    ws = L.workspace(nbytes := int(L.lib().recmv_closest_point_workspace_bytes(P)), dev, "closest_point_workspace_bytes")
    L.launch("closest_point", dev, L.ptr(p), P, L.ptr(verts), verts.shape[0], L.ptr(faces), faces.shape[0], L.ptr(face),
             L.ptr(point), L.ptr(dist2), L.ptr(ws), nbytes)
    return face, point, dist2


def _closest_st(p, a, ab, ac):
    """Ericson's point-triangle test, broadcast over p [...,3] and a / ab / ac [...,3]: (s, t, squared distance) with
    the closest point a + s ab + t ac; the region is the first of Ericson's tests that holds."""
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    ap = p - a
    bp = ap - ab
    cp = ap - ac
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    den = va + vb + vc
    s, t = vb / den, vc / den                                                     # inside the face
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    regions = (((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), one - w, w),      # edge bc
               ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),      # edge ac
               ((d6 >= 0) & (d5 <= d6), zero, one),                            # vertex c
               ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),      # edge ab
               ((d3 >= 0) & (d4 <= d3), one, zero),                            # vertex b
               ((d1 <= 0) & (d2 <= 0), zero, zero))                            # vertex a
    for cond, cs, ct in regions:                                                  # the first test that holds wins
        s, t = torch.where(cond, cs, s), torch.where(cond, ct, t)
    d = ap - s[..., None] * ab - t[..., None] * ac
    return s, t, dot(d, d)


def closest_point_torch(p, verts, faces, chunk_elems=1 << 22):
    """closest_point in plain torch (row chunks of a brute force in p's dtype; the first minimum is kept)."""
    a = verts[faces[:, 0]]
    ab, ac = verts[faces[:, 1]] - a, verts[faces[:, 2]] - a
    rows = max(1, chunk_elems // max(faces.shape[0], 1))
    face, point, dist2 = [], [], []
    for s0 in range(0, p.shape[0], rows):
        q = p[s0:s0 + rows, None, :]
        s, t, d = _closest_st(q, a[None], ab[None], ac[None])
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        i = d.argmin(dim=1)
        r = torch.arange(i.shape[0], device=p.device)
        face.append(i)
        point.append(a[i] + s[r, i, None] * ab[i] + t[r, i, None] * ac[i])
        dist2.append(d[r, i])
    if not face:
        return (torch.zeros(0, dtype=torch.int64, device=p.device), p.new_zeros(0, 3), p.new_zeros(0))
    return torch.cat(face), torch.cat(point), torch.cat(dist2)


def _padded(off, idx, V):
    """Neighbour CSR as a padded table: (nbr [V, D] int64 with -1 padding, count [V])."""
    off = off.to(torch.int64)
    cnt = off[1:] - off[:-1]
    D = int(cnt.max()) if V > 0 else 0
    col = torch.arange(D, device=off.device)
    valid = col[None, :] < cnt[:, None]
    pos = (off[:-1, None] + col[None, :]).clamp(max=max(idx.shape[0] - 1, 0))
    nbr = torch.where(valid, idx.to(torch.int64)[pos] if idx.numel() else pos, torch.full_like(pos, -1))
    return nbr, cnt


def _gather_sum(x, nbr):
    """sum_j x[nbr[i, j]] over the valid (>= 0) entries, in column order."""
    g = x[nbr.clamp(min=0)] * (nbr >= 0)[..., None].to(x.dtype)
    s = torch.zeros_like(x)
    for j in range(nbr.shape[1]):                                                  # a fixed summation order
        s = s + g[:, j]
    return s


def iso_relax(verts, normals, fixed, nbr_csr):
    """recmv_iso_relax: p + (I - n n^T)(c - p) for the free vertices (verts / normals [V,3] f32 CUDA, fixed [V] bool)."""
    verts, normals = check_points(verts, "verts"), check_points(normals, "normals")
    V = verts.shape[0]
    off, idx = nbr_csr
    if normals.shape[0] != V or fixed.shape[0] != V or off.numel() != V + 1:
        raise ValueError("iso_relax: normals, fixed and the neighbour list must have %d rows" % V)
    fx = fixed.to(torch.uint8).contiguous()
    out = L.scratch_like(verts)
    L.launch("iso_relax", verts.device, L.ptr(off), L.ptr(idx), V, idx.numel(), L.ptr(verts), L.ptr(normals), L.ptr(fx), L.ptr(out))
    return out


def iso_relax_torch(verts, normals, fixed, nbr_csr):
    """iso_relax in plain torch, in f64 and rounded to verts' dtype."""
    V = verts.shape[0]
    nbr, cnt = _padded(nbr_csr[0], nbr_csr[1], V)
    x = verts.double()
    n = normals.double()
    c = _gather_sum(x, nbr) / cnt.clamp(min=1)[:, None].double()
    d = c - x
    moved = x + (d - (d * n).sum(1, keepdim=True) * n)
    keep = fixed.bool() | (cnt == 0)
    return torch.where(keep[:, None], x, moved).to(verts.dtype)


# ------------------------------------------------------------------------------------------------- topology
def _csr_rows(off, rows):
    """Expand CSR rows: (which query [K'] int64, position in the CSR's value list [K'] int64) for every entry of every
    row in `rows`, query by query and in CSR order."""
    off = off.to(torch.int64)
    start = off[rows]
    cnt = off[rows + 1] - start
    which = torch.repeat_interleave(torch.arange(rows.shape[0], device=rows.device), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    pos = start[which] + torch.arange(which.shape[0], device=rows.device) - first[which]
    return which, pos


class _Topo(EdgeTable):
    """The EdgeTable of one edge-manifold face table (f2e / bedge / bvert: its face_to_edge / boundary_edge / boundary_vertex)
    and what the remesher adds: per edge its first / second (face * 3 + corner) slot — the corner opposite the edge — in
    ascending slot order, the valence per vertex, the neighbour CSR and the vertex -> face CSR."""

    def __init__(self, faces, V):
        super().__init__(faces, V)
        dev, F, E = faces.device, self.F, self.E
        self.f2e, self.bedge, self.bvert = self.face_to_edge, self.boundary_edge, self.boundary_vertex
        if E and int(self.count.max()) > 2:
            raise ValueError("iso_remesh: the mesh must be edge-manifold (an edge has %d faces)" % int(self.count.max()))
        fe = self.f2e.reshape(-1)
        slots = torch.arange(3 * F, device=dev)
        order = torch.argsort(fe * (3 * F) + slots)
        start = torch.cumsum(self.count, 0) - self.count
        self.slot0 = order[start]
        self.slot1 = torch.where(self.count > 1, order[(start + 1).clamp(max=max(3 * F - 1, 0))],
                                 torch.full_like(start, -1))
        ones = torch.ones(2 * E, dtype=torch.int64, device=dev)
        self.valence = torch.zeros(V, dtype=torch.int64, device=dev).index_add(0, self.edges.reshape(-1), ones)
        self.nbr = neighbours_csr(self.edges, V)
        self.vf = vertex_slots_csr(faces, V)                                  # vertex -> face slots, ascending

    def edge_key(self, u, w):
        lo, hi = torch.minimum(u, w), torch.maximum(u, w)
        return lo * self.V + hi

    def has_edge(self, u, w):
        keys = self.edges[:, 0] * self.V + self.edges[:, 1]
        q = self.edge_key(u, w)
        i = torch.searchsorted(keys, q).clamp(max=max(self.E - 1, 0))
        return (keys[i] == q) if self.E else torch.zeros_like(q, dtype=torch.bool)


def _face_normals(verts, faces):
    a = verts[faces[:, 0]]
    return torch.cross(verts[faces[:, 1]] - a, verts[faces[:, 2]] - a, dim=1)


def _unit(n):
    return n / n.norm(dim=1, keepdim=True).clamp(min=1e-30)


def _fixed(verts, faces, topo, cos_feature):
    """(crease [E] bool, fixed [V] bool): interior edges whose dihedral angle exceeds the feature angle, and the boundary
    vertices plus the crease endpoints."""
    n = _unit(_face_normals(verts, faces))
    inner = topo.count == 2
    f0 = topo.slot0 // 3
    f1 = topo.slot1.clamp(min=0) // 3
    crease = inner & ((n[f0] * n[f1]).sum(1) < cos_feature)
    fixed = topo.bvert.clone()
    fixed[topo.edges[crease].reshape(-1)] = True
    return crease, fixed


def _boundary_loop_length(faces, topo):
    """Per boundary edge: the number of edges of its boundary loop (pointer doubling over the boundary successor)."""
    V, dev = topo.V, faces.device
    be = torch.nonzero(topo.bedge).flatten()
    if be.numel() == 0:
        return torch.zeros(topo.E, dtype=torch.int64, device=dev)
    s = topo.slot0[be]
    fv = faces.reshape(-1)
    f, k = s // 3, s % 3
    a = fv[3 * f + (k + 1) % 3]                                              # directed boundary edge a -> b of its face
    b = fv[3 * f + (k + 2) % 3]
    nxt = torch.arange(V, device=dev)
    nxt[a] = b
    label = torch.full((V,), V, dtype=torch.int64, device=dev)
    label[a] = a
    jump = nxt.clone()
    for _ in range(max(1, int(math.ceil(math.log2(max(be.numel(), 2)))) + 1)):
        label = torch.minimum(label, label[jump])
        jump = jump[jump]
    size = torch.bincount(label[a], minlength=V + 1)
    out = torch.zeros(topo.E, dtype=torch.int64, device=dev)
    out[be] = size[label[a]]
    return out


class _Surface:
    """The frozen reference surface: closest points by the kernel or by the restatement, and its boundary polyline."""

    def __init__(self, verts, faces, use_kernels):
        self.verts, self.faces, self.use_kernels = verts.clone(), faces.clone(), use_kernels
        topo = _Topo(faces, verts.shape[0])
        self.segments = topo.edges[topo.bedge]

    def closest(self, p):
        if p.shape[0] == 0:
            return p.clone(), p.new_zeros(0)
        if self.use_kernels:
            _, q, d2 = closest_point(p.float(), self.verts, self.faces)
        else:
            _, q, d2 = closest_point_torch(p, self.verts, self.faces)
        return q.to(p.dtype), d2.to(p.dtype)

    def on_boundary(self, p):
        """Closest points of p [K,3] on the boundary polyline (first minimum over the segments)."""
        if p.shape[0] == 0 or self.segments.shape[0] == 0:
            return p
        a, b = self.verts[self.segments[:, 0]].to(p.dtype), self.verts[self.segments[:, 1]].to(p.dtype)
        ab = b - a
        t = (((p[:, None] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1).clamp(min=1e-30)[None]).clamp(0., 1.)
        q = a[None] + t[..., None] * ab[None]
        i = ((q - p[:, None]) ** 2).sum(-1).argmin(1)
        return q[torch.arange(p.shape[0], device=p.device), i]


# ------------------------------------------------------------------------------------------------- the four steps
def _split(verts, faces, hi, surf):
    """Split every edge longer than `hi` at its midpoint, in passes until none is (at most MAX_PASSES)."""
    splits = 0
    for _ in range(MAX_PASSES):
        V = verts.shape[0]
        topo = _Topo(faces, V)
        e = topo.edges
        long_ = (verts[e[:, 0]] - verts[e[:, 1]]).norm(dim=1) > hi
        n = int(long_.sum())
        if n == 0:
            break
        splits += n
        new_id = torch.full((topo.E,), -1, dtype=torch.int64, device=faces.device)
        new_id[long_] = V + torch.arange(n, device=faces.device)
        mid = (verts[e[long_, 0]] + verts[e[long_, 1]]) * 0.5
        onb = topo.bedge[long_]
        mid[onb] = surf.on_boundary(mid[onb])
        verts = torch.cat([verts, mid], 0)
        m = new_id[topo.f2e]                                                  # midpoint opposite each corner, or -1
        ns = (m >= 0).sum(1)
        # roll every split face so that its special corner comes first: the split edge (1 split), the kept edge (2)
        special = torch.where(ns == 2, (m < 0).to(torch.int64).argmax(1), (m >= 0).to(torch.int64).argmax(1))
        r = (special[:, None] + torch.arange(3, device=faces.device)[None]) % 3
        p = faces.gather(1, r)
        q = m.gather(1, r)
        p0, p1, p2, m0, m1, m2 = p[:, 0], p[:, 1], p[:, 2], q[:, 0], q[:, 1], q[:, 2]
        out = [faces[ns == 0]]
        c1 = ns == 1
        out.append(torch.cat([torch.stack([p0, p1, m0], 1)[c1], torch.stack([p0, m0, p2], 1)[c1]], 0))
        c2 = ns == 2
        l1 = (verts[m2] - verts[p2]).norm(dim=1)                            # diagonal (m2, p2)
        l2 = (verts[p1] - verts[m1]).norm(dim=1)                            # diagonal (p1, m1)
        low1 = torch.minimum(m2, p2) < torch.minimum(p1, m1)
        use1 = (l1 < l2) | ((l1 == l2) & low1)
        d1 = c2 & use1
        d2 = c2 & ~use1
        out += [torch.stack([p0, m2, m1], 1)[c2],
                torch.stack([m2, p1, p2], 1)[d1], torch.stack([m2, p2, m1], 1)[d1],
                torch.stack([p1, p2, m1], 1)[d2], torch.stack([p1, m1, m2], 1)[d2]]
        c3 = ns == 3
        out += [torch.stack([p0, m2, m1], 1)[c3], torch.stack([p1, m0, m2], 1)[c3], torch.stack([p2, m1, m0], 1)[c3],
                torch.stack([m0, m1, m2], 1)[c3]]
        faces = torch.cat(out, 0)
    return verts, faces, splits


def _ring_min(key, nbr_off, nbr_idx):
    """min of key over the closed one-ring of every vertex."""
    V = key.shape[0]
    rows = torch.repeat_interleave(torch.arange(V, device=key.device), (nbr_off[1:] - nbr_off[:-1]).to(torch.int64))
    out = key.clone()
    if rows.numel():
        out = out.scatter_reduce(0, rows, key[nbr_idx.to(torch.int64)], reduce="amin")
    return out


def _link_ok(topo, ca, cb, bnd):
    """Link condition of the edges (ca, cb) (bnd: boundary edges): the common neighbours are exactly the opposite vertices."""
    off, idx = topo.nbr
    w_of, pos = _csr_rows(off, ca)
    w = idx[pos].to(torch.int64)
    common = torch.bincount(w_of[topo.has_edge(cb[w_of], w) & (w != cb[w_of])], minlength=ca.shape[0])
    return common == torch.where(bnd, 1, 2)


def _flip_ok(verts, faces, topo, ca, cb, p):
    """No face that survives the collapse of (ca, cb) to p flips or degenerates (in the dtype of verts and p)."""
    K = ca.shape[0]
    ok = torch.ones(K, dtype=torch.bool, device=faces.device)
    for ends in (ca, cb):
        s_of, pos = _csr_rows(topo.vf[0], ends)
        sl = topo.vf[1][pos]
        f = sl // 3
        tri = faces[f]
        gone = ((tri == ca[s_of, None]) | (tri == cb[s_of, None])).sum(1) == 2
        moved = tri == ends[s_of, None]
        tv = verts[tri]
        nv = torch.where(moved[..., None], p[s_of, None, :], tv)
        n_old = torch.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0], dim=1)
        n_new = torch.cross(nv[:, 1] - nv[:, 0], nv[:, 2] - nv[:, 0], dim=1)
        bad = ~gone & ((n_old * n_new).sum(1) <= 0)
        ok &= torch.bincount(s_of[bad], minlength=K) == 0
    return ok


def _independent(topo, ca, cb, key):
    """bool over the edges (ca, cb): an independent set by priority (key ascending, then position): no two chosen edges within
    two rings of each other."""
    dev = ca.device
    off, idx = topo.nbr
    order = torch.sort(key, stable=True)[1]
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.shape[0], device=dev)
    big = order.shape[0]
    m = torch.full((topo.V,), big, dtype=torch.int64, device=dev)
    m = m.scatter_reduce(0, torch.cat([ca, cb]), torch.cat([rank, rank]), reduce="amin")
    m = _ring_min(_ring_min(m, off, idx), off, idx)
    return (m[ca] == rank) & (m[cb] == rank)


def _merge(verts, faces, ca, cb, p):
    """Move the vertices ca to p, replace cb by ca in the faces and drop the faces that lose a corner."""
    verts = verts.clone()
    verts[ca] = p
    remap = torch.arange(verts.shape[0], device=faces.device)
    remap[cb] = ca
    faces = remap[faces]
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])]
    return verts, faces


def _collapse(verts, faces, lo, hi, cos_feature, max_dist, surf):
    """Collapse edges shorter than `lo` in rounds of independent sets (at most MAX_PASSES)."""
    collapses = 0
    dev = faces.device
    for _ in range(MAX_PASSES):
        V = verts.shape[0]
        topo = _Topo(faces, V)
        e = topo.edges
        a, b = e[:, 0], e[:, 1]
        elen = (verts[a] - verts[b]).norm(dim=1)
        _, fixed = _fixed(verts, faces, topo, cos_feature)
        cand = elen < lo
        cand &= ~(~topo.bedge & fixed[a] & fixed[b])                       # two fixed vertices through an interior edge
        ci = torch.nonzero(cand).flatten()
        if ci.numel() == 0:
            break
        ca, cb = a[ci], b[ci]
        fa, fb = fixed[ca], fixed[cb]
        bnd = topo.bedge[ci]
        p = (verts[ca] + verts[cb]) * 0.5
        p = torch.where((fa & ~fb)[:, None], verts[ca], p)
        p = torch.where((fb & ~fa)[:, None], verts[cb], p)
        p = torch.where(bnd[:, None], verts[ca], p)                          # boundary edge: the lower-index endpoint
        K = ci.shape[0]
        ok = torch.ones(K, dtype=torch.bool, device=dev)
        off, idx = topo.nbr
        ok &= _link_ok(topo, ca, cb, bnd)
        # a boundary loop keeps at least 3 edges
        ok &= ~bnd | (_boundary_loop_length(faces, topo)[ci] > 3)
        # no new edge longer than hi
        for ends in (ca, cb):
            w_of, pos = _csr_rows(off, ends)
            w = idx[pos].to(torch.int64)
            far = ((p[w_of] - verts[w]).norm(dim=1) > hi) & (w != ca[w_of]) & (w != cb[w_of])
            ok &= torch.bincount(w_of[far], minlength=K) == 0
        ok &= _flip_ok(verts, faces, topo, ca, cb, p)
        # no vertex farther than max_dist from the reference surface (only a midpoint is new)
        newp = ~bnd & (fa == fb)
        if bool(newp.any()):
            _, d2 = surf.closest(p[newp])
            far = torch.zeros(K, dtype=torch.bool, device=dev)
            far[newp] = d2 > max_dist * max_dist
            ok &= ~far
        ci, ca, cb, p, elen_c = ci[ok], ca[ok], cb[ok], p[ok], elen[ci[ok]]
        if ci.numel() == 0:
            break
        # independent set: priority by (length, edge id); no two chosen edges within two rings of each other
        pick = _independent(topo, ca, cb, elen_c)
        ca, cb, p = ca[pick], cb[pick], p[pick]
        collapses += int(ca.shape[0])
        verts, faces = _merge(verts, faces, ca, cb, p)
        verts, faces, _ = compact(verts, faces)
    return verts, faces, collapses


def _valence_dev(topo):
    target = torch.where(topo.bvert, 4, 6)
    return (topo.valence - target).abs()


def _flip(verts, faces, cos_feature):
    """Flip interior non-crease edges that lower the valence deviation, in rounds of face-disjoint sets."""
    flips = 0
    dev = faces.device
    for _ in range(MAX_PASSES):
        V = verts.shape[0]
        topo = _Topo(faces, V)
        crease, _ = _fixed(verts, faces, topo, cos_feature)
        ei = torch.nonzero((topo.count == 2) & ~crease).flatten()
        if ei.numel() == 0:
            break
        fv = faces.reshape(-1)
        s0, s1 = topo.slot0[ei], topo.slot1[ei]
        f0, k0, f1 = s0 // 3, s0 % 3, s1 // 3
        a = fv[3 * f0 + (k0 + 1) % 3]                                         # face f0 = (a, b, c), f1 = (b, a, d)
        b = fv[3 * f0 + (k0 + 2) % 3]
        c = fv[s0]
        d = fv[s1]
        target = torch.where(topo.bvert, 4, 6)
        val = topo.valence
        before = ((val[a] - target[a]).abs() + (val[b] - target[b]).abs() + (val[c] - target[c]).abs()
                  + (val[d] - target[d]).abs())
        after = ((val[a] - 1 - target[a]).abs() + (val[b] - 1 - target[b]).abs() + (val[c] + 1 - target[c]).abs()
                 + (val[d] + 1 - target[d]).abs())
        ok = (after < before) & (c != d) & ~topo.has_edge(c, d)
        n0 = _unit(_face_normals(verts, faces[f0]))
        n1 = _unit(_face_normals(verts, faces[f1]))
        mean = n0 + n1
        na = _face_normals(verts, torch.stack([c, a, d], 1))
        nb = _face_normals(verts, torch.stack([d, b, c], 1))
        ok &= ((na * mean).sum(1) > 0) & ((nb * mean).sum(1) > 0)
        E = topo.E
        key = (after - before + 8) * E + ei                                   # largest gain first, then edge id
        ok_i = torch.nonzero(ok).flatten()
        if ok_i.numel() == 0:
            break
        key, f0, f1, a, b, c, d = key[ok_i], f0[ok_i], f1[ok_i], a[ok_i], b[ok_i], c[ok_i], d[ok_i]
        # independent set: no two chosen flips share a face; they share no vertex either, so that the valence changes
        # a flip was chosen for are the ones that happen
        big = 16 * E + E
        vm = torch.full((V,), big, dtype=torch.int64, device=dev)
        vm = vm.scatter_reduce(0, torch.cat([a, b, c, d]), key.repeat(4), reduce="amin")
        pick = (vm[a] == key) & (vm[b] == key) & (vm[c] == key) & (vm[d] == key)
        # two flips of one round must not create the same edge
        nk = topo.edge_key(c, d)
        u, inv, cnt = torch.unique(nk[pick], return_inverse=True, return_counts=True)
        pk = torch.nonzero(pick).flatten()
        pick[pk[cnt[inv] > 1]] = False
        if not bool(pick.any()):
            break
        flips += int(pick.sum())
        faces = faces.clone()
        faces[f0[pick]] = torch.stack([c, a, d], 1)[pick]
        faces[f1[pick]] = torch.stack([d, b, c], 1)[pick]
    return faces, flips


def _keep_faces_unfolded(old, new, faces, keep=0.1):
    """Relax + project may push a vertex next to the boundary onto the boundary polyline or across a neighbour: a moved
    vertex of a face whose area along its old normal drops below `keep` x the old area goes back to its old position,
    in rounds until no such face is left."""
    n_old = _face_normals(old, faces)
    a_old = n_old.norm(dim=1)
    for _ in range(MAX_PASSES):
        moved = (new != old).any(1)
        proj = (_face_normals(new, faces) * n_old).sum(1)
        bad = (proj <= keep * a_old * a_old) & moved[faces].any(1)
        if not bool(bad.any()):
            break
        back = torch.zeros_like(moved)
        back[faces[bad].reshape(-1)] = True
        new = torch.where(back[:, None], old, new)
    return new


def _normals(verts, faces, use_kernels):
    if use_kernels:
        return nricp.verts_normals(verts, faces)
    return nricp.verts_normals(verts.cpu(), faces.cpu()).to(verts.device)


def _edge_stats(verts, topo, L_):
    el = (verts[topo.edges[:, 0]] - verts[topo.edges[:, 1]]).norm(dim=1) / L_
    return float(el.min()), float(el.mean()), float(el.max())


def isotropic_remesh(verts, faces, target_len=None, iterations=3, feature_deg=30., max_surf_dist=None, use_kernels=True,
                     log=None):
    """Botsch-Kobbelt isotropic remeshing of one triangle mesh (verts [V,3] float, faces [F,3] int64, one device):
    (verts, faces, stats), stats one dict per iteration.  `target_len` defaults to 0.01 x the bounding-box diagonal,
    `max_surf_dist` to target_len; `use_kernels` selects the HIP kernels (CUDA tensors) or their restatements."""
    faces = faces.to(torch.int64).contiguous()
    verts = verts.float().contiguous() if use_kernels else verts.contiguous()
    if use_kernels:
        L.require_cuda(verts, "verts")
    if faces.shape[0] == 0:
        raise ValueError("isotropic_remesh: the mesh has no faces")
    verts, faces, _ = compact(verts, faces)
    diag = float((verts.max(0)[0] - verts.min(0)[0]).norm())
    L_ = float(target_len) if target_len is not None else 0.01 * diag
    if not L_ > 0:
        raise ValueError("isotropic_remesh: the target edge length must be positive (got %r)" % L_)
    max_d = float(max_surf_dist) if max_surf_dist is not None else L_
    hi, lo = 4. / 3. * L_, 4. / 5. * L_
    cos_feature = math.cos(math.radians(feature_deg))
    surf = _Surface(verts, faces, use_kernels)
    stats = []
    for it in range(iterations):
        verts, faces, n_split = _split(verts, faces, hi, surf)
        verts, faces, n_coll = _collapse(verts, faces, lo, hi, cos_feature, max_d, surf)
        dev_pre = float(_valence_dev(_Topo(faces, verts.shape[0])).double().mean())
        faces, n_flip = _flip(verts, faces, cos_feature)
        topo = _Topo(faces, verts.shape[0])
        _, fixed = _fixed(verts, faces, topo, cos_feature)
        normals = _normals(verts, faces, use_kernels)
        if use_kernels:
            moved = iso_relax(verts, normals, fixed, topo.nbr)
        else:
            moved = iso_relax_torch(verts, normals, fixed, topo.nbr)
        free = torch.nonzero(~fixed).flatten()
        q, _ = surf.closest(moved[free])
        moved = moved.clone()
        moved[free] = q
        verts = _keep_faces_unfolded(verts, moved, faces)
        _, d2 = surf.closest(verts)
        emin, emean, emax = _edge_stats(verts, topo, L_)
        st = dict(iteration=it, V=verts.shape[0], F=faces.shape[0], splits=n_split, collapses=n_coll, flips=n_flip,
                  edge_min=emin, edge_mean=emean, edge_max=emax, max_dist=float(d2.max().clamp(min=0).sqrt()),
                  valence_dev_pre_flip=dev_pre, valence_dev=float(_valence_dev(topo).double().mean()))
        stats.append(st)
        if log is not None:
            log("iso-remesh %d/%d: V=%d F=%d splits=%d collapses=%d flips=%d edge/L min %.3f mean %.3f max %.3f "
                "max dist %.3g" % (it + 1, iterations, st['V'], st['F'], n_split, n_coll, n_flip, emin, emean, emax,
                                   st['max_dist']))
    return verts, faces, stats


# ------------------------------------------------------------------------------------------------- Loop subdivision
def _loop_tables(faces, V):
    """(edge table [E,4] int64 = (a, b, c, d), d = -1 on a boundary edge; boundary neighbours [V,2] int64, -1 when the
    vertex is interior; neighbour CSR) in edges_packed order."""
    topo = _Topo(faces, V)
    fv = faces.reshape(-1)
    c = fv[topo.slot0]
    d = torch.where(topo.slot1 >= 0, fv[topo.slot1.clamp(min=0)], torch.full_like(topo.slot1, -1))
    etab = torch.cat([topo.edges, c[:, None], d[:, None]], 1).contiguous()
    be = topo.edges[topo.bedge]
    rows = torch.cat([be[:, 0], be[:, 1]])
    cols = torch.cat([be[:, 1], be[:, 0]])
    o = torch.argsort(rows * max(V, 1) + cols)
    rows, cols = rows[o], cols[o]
    first = torch.ones_like(rows, dtype=torch.bool)
    first[1:] = rows[1:] != rows[:-1]
    bn = torch.full((V, 2), -1, dtype=torch.int64, device=faces.device)
    bn[rows[first], 0] = cols[first]
    second = torch.zeros_like(first)
    second[1:] = first[:-1] & ~first[1:]
    bn[rows[second], 1] = cols[second]
    return etab, bn.contiguous(), topo.nbr


def _loop_once_torch(verts, etab, bn, nbr_csr):
    V = verts.shape[0]
    x = verts.double()
    nbr, cnt = _padded(nbr_csr[0], nbr_csr[1], V)
    s = _gather_sum(x, nbr)
    n = cnt.double().clamp(min=1.)
    g = 0.375 + 0.25 * torch.cos(2. * math.pi / n)
    beta = (0.625 - g * g) / n
    even = (1. - n * beta)[:, None] * x + beta[:, None] * s
    even = torch.where((cnt == 0)[:, None], x, even)
    onb = (bn >= 0).any(1)
    bx = 0.75 * x + 0.125 * (x[bn[:, 0].clamp(min=0)] + x[bn[:, 1].clamp(min=0)])
    even = torch.where(onb[:, None], bx, even)
    a, b, c, d = etab[:, 0], etab[:, 1], etab[:, 2], etab[:, 3]
    ab = x[a] + x[b]
    odd = torch.where((d >= 0)[:, None], 0.375 * ab + 0.125 * (x[c] + x[d.clamp(min=0)]), 0.5 * ab)
    return torch.cat([even, odd], 0).to(verts.dtype)


def _loop_once_kernel(verts, etab, bn, nbr_csr):
    verts = check_points(verts, "verts")
    V, E = verts.shape[0], etab.shape[0]
    off, idx = nbr_csr
    out = L.scratch((V + E, 3), torch.float32, verts.device)
    L.launch("loop_subdivide", verts.device, L.ptr(off), L.ptr(idx), V, idx.numel(), L.ptr(verts), L.ptr(bn), L.ptr(etab), E,
             L.ptr(out))
    return out


def loop_subdivide(verts, faces, levels=1, use_kernels=True):
    """`levels` uniform Loop subdivisions (verts [V,3], faces [F,3] int64): the faces are edge_subdivide's (V + E
    vertices, 4F faces, corner faces then centre faces), the positions Loop's even and odd rules."""
    faces = faces.to(torch.int64).contiguous()
    if use_kernels:
        L.require_cuda(verts, "verts")
        verts = verts.float()
    for _ in range(levels):
        V = verts.shape[0]
        etab, bn, nbr = _loop_tables(faces, V)
        verts = (_loop_once_kernel if use_kernels else _loop_once_torch)(verts, etab, bn, nbr)
        _, faces = nricp.edge_subdivide(verts[:V], faces)
    return verts, faces
