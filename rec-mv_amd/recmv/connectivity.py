"""Which undirected edges a face table has and how many faces use each — the third shared mesh primitive beside
metrics.MeshGrid and topology.graph_components.  Plain torch on the faces' device (CPU or CUDA), integer tables only, no kernel.

  edges_packed        pytorch3d `Meshes.edges_packed` (unique undirected edges, sorted) and `faces_packed_to_edges_packed`
  incident_edges_csr / neighbours_csr   the per-vertex lists the NR-ICP and Laplacian kernels gather over
  EdgeTable           the one place that classifies edges: face count, border, non-manifold, border vertices, direction
  vertex_slots_csr / boundary_edges_csr   vertex -> its faces and vertex -> its border edges, what the quadric kernel gathers over
  face_neighbours_csr / boundary_neighbours   face -> the faces across its edges and vertex -> its two boundary neighbours, what the
                      smoothing kernels gather over
  boundary_loops      closed walks over the border edges (on the host)
  compact             drop the vertices no face uses and renumber
"""
import torch


def edges_packed(faces, V):
    """(edges [E,2] int64, v0 < v1, sorted by V * v0 + v1; face_to_edge [F,3]: the edges (v1,v2), (v2,v0), (v0,v1) of
    every face) — pytorch3d's `_compute_edges_packed`."""
    faces = faces.to(torch.int64)
    F = faces.shape[0]
    v0, v1, v2 = faces.chunk(3, dim=1)
    e = torch.cat([torch.cat([v1, v2], 1), torch.cat([v2, v0], 1), torch.cat([v0, v1], 1)], 0)
    e, _ = e.sort(dim=1)
    h = V * e[:, 0] + e[:, 1]
    u, inverse = torch.unique(h, return_inverse=True)
    edges = torch.stack([u // V, u % V], dim=1)
    face_to_edge = inverse[torch.arange(3 * F, device=faces.device).view(3, F).t()]
    return edges, face_to_edge


def _csr(rows, cols, V):
    """Rows sorted by (row, col): (offsets int32 [V+1], cols int32)."""
    order = torch.argsort(rows * max(int(cols.max()) + 1 if cols.numel() else 1, 1) + cols)
    counts = torch.bincount(rows, minlength=V)
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=rows.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32).contiguous(), cols[order].to(torch.int32).contiguous()


def incident_edges_csr(edges, V):
    """Vertex -> incident edge indices, ascending: (offsets int32 [V+1], edge ids int32 [2E])."""
    E = edges.shape[0]
    eid = torch.arange(E, device=edges.device, dtype=torch.int64)
    return _csr(torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([eid, eid]), V)


def neighbours_csr(edges, V):
    """Vertex -> neighbour vertices, ascending: (offsets int32 [V+1], neighbours int32 [2E]); degree = row length."""
    return _csr(torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]]), V)


class EdgeTable:
    """The undirected edges of faces [F,3] int64 with indices in [0, V) (checked here, once; F = 0 and V = 0 are fine):
      edges [E,2], face_to_edge [F,3]   edges_packed: column k of face_to_edge is the edge opposite corner k
      count [E]                         the faces that use the edge
      boundary_edge [E]                 count == 1
      nonmanifold_edge [E]              count > 2
      boundary_vertex [V]               an end of some boundary edge
      forward [F,3]                     half-edge k of a face runs faces[:, (k+1)%3] -> faces[:, (k+2)%3]: True when that is
                                        from the lower to the higher index"""

    def __init__(self, faces, V):
        if faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError("faces must be int64 of shape [F,3]")
        self.V, self.F, self.faces = int(V), faces.shape[0], faces
        if self.F:
            lo, hi = (int(x) for x in torch.aminmax(faces))
            if lo < 0 or hi >= self.V:
                raise ValueError("a face index lies outside [0, %d)" % self.V)
        self.edges, self.face_to_edge = edges_packed(faces, max(self.V, 1))
        self.E = self.edges.shape[0]
        self.count = torch.bincount(self.face_to_edge.reshape(-1), minlength=self.E)
        self.boundary_edge = self.count == 1
        self.boundary_vertex = torch.zeros(self.V, dtype=torch.bool, device=faces.device)
        self.boundary_vertex[self.edges[self.boundary_edge].reshape(-1)] = True

    @property
    def nonmanifold_edge(self):
        return self.count > 2

    @property
    def forward(self):
        return self.faces[:, [1, 2, 0]] < self.faces[:, [2, 0, 1]]


def vertex_slots_csr(faces, V):
    """Vertex -> the corner slots (face * 3 + corner) that hold it, ascending: (offsets int64 [V+1], slots int64 [3F]).  A valid
    face holds a vertex once, so slots // 3 are the vertex's faces, ascending."""
    F = faces.shape[0]
    fv = faces.reshape(-1)
    o = torch.argsort(fv * (3 * F) + torch.arange(3 * F, device=faces.device))
    cnt = torch.bincount(fv, minlength=V)
    off = torch.zeros(V + 1, dtype=torch.int64, device=faces.device)
    off[1:] = torch.cumsum(cnt, 0)
    return off, o


def filed_slots_csr(faces, V):
    """vertex_slots_csr of faces that may hold indices outside [0, V): such corners are filed under a row of their own, V,
    which no vertex reads — (offsets int64 [V+1], slots int64 [3F]), both contiguous."""
    if faces.shape[0] == 0:
        return (torch.zeros(V + 1, dtype=torch.int64, device=faces.device), torch.zeros(0, dtype=torch.int64, device=faces.device))
    off, slots = vertex_slots_csr(torch.where((faces >= 0) & (faces < V), faces, V), V + 1)
    return off[:V + 1].contiguous(), slots.contiguous()


def boundary_edges_csr(table):
    """The border of an EdgeTable as the quadric kernel reads it: (border [B,3] int64 = (v0, v1, the one face that uses the edge),
    in edge order; offsets int64 [V+1], rows int64 [2B]: vertex -> its rows of border, ascending)."""
    dev, V, F = table.faces.device, table.V, table.F
    be = table.boundary_edge.nonzero().squeeze(1)
    face_of = torch.zeros(table.E, dtype=torch.int64, device=dev)
    face_of.scatter_(0, table.face_to_edge.reshape(-1), torch.arange(3 * F, device=dev) // 3)   # one writer per border edge
    border = torch.cat([table.edges[be], face_of[be, None]], 1).contiguous()
    B = border.shape[0]
    rid = torch.arange(B, device=dev)
    rows, cols = torch.cat([border[:, 0], border[:, 1]]), torch.cat([rid, rid])
    order = torch.argsort(rows * max(B, 1) + cols)
    off = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(torch.bincount(rows, minlength=V), 0)
    return border, off, cols[order].contiguous()


def face_neighbours_csr(table):
    """Face -> the faces that share an edge with it, ascending and without the face itself, of an EdgeTable: (offsets int32
    [F+1], faces int32).  At a non-manifold edge those are all of the edge's other faces; a face met across two edges is
    listed once."""
    dev, F, E = table.faces.device, table.F, table.E
    fe = table.face_to_edge.reshape(-1)                                            # [3F], slot -> edge
    face = torch.arange(3 * F, device=dev) // 3
    order = torch.argsort(fe * max(F, 1) + face)                                   # slots by (edge, face)
    start = torch.zeros(E + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(table.count, 0)
    D = int(table.count.max()) if E else 0
    rows, cols = [], []
    for k in range(D):                                                             # the k-th face of every slot's edge
        has = table.count[fe] > k
        rows.append(face[has])
        cols.append(face[order[(start[fe[has]] + k)]])
    rows = torch.cat(rows) if rows else face[:0]
    cols = torch.cat(cols) if cols else face[:0]
    key = torch.unique((rows * max(F, 1) + cols)[rows != cols])                    # sorted by (row, col), repeats gone
    rows, cols = key // max(F, 1), key % max(F, 1)
    off = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(torch.bincount(rows, minlength=F), 0)
    return off.to(torch.int32).contiguous(), cols.to(torch.int32).contiguous()


def boundary_neighbours(table):
    """[V,2] int64 of an EdgeTable, the layout recmv_loop_subdivide and recmv_laplacian_step read: the two boundary neighbours
    of a vertex with exactly two boundary edges, ascending; (-1, -1) for an interior vertex; (lowest neighbour, -1) for a
    boundary vertex with any other number of boundary edges (where loops touch), which the readers then leave where it is."""
    dev, V = table.faces.device, table.V
    be = table.edges[table.boundary_edge]
    rows = torch.cat([be[:, 0], be[:, 1]])
    cols = torch.cat([be[:, 1], be[:, 0]])
    o = torch.argsort(rows * max(V, 1) + cols)
    rows, cols = rows[o], cols[o]
    degree = torch.bincount(rows, minlength=V)
    first = torch.ones_like(rows, dtype=torch.bool)
    first[1:] = rows[1:] != rows[:-1]
    bn = torch.full((V, 2), -1, dtype=torch.int64, device=dev)
    bn[rows[first], 0] = cols[first]
    second = torch.zeros_like(first)
    second[1:] = first[:-1] & ~first[1:]
    second &= degree[rows] == 2
    bn[rows[second], 1] = cols[second]
    return bn.contiguous()


def boundary_loops(faces, V=None):
    """Boundary loops of a triangle mesh: lists of vertex indices along closed walks over the edges used by one face.
    Each walk starts at the lowest vertex index with an unwalked boundary edge and always takes the lowest unwalked
    neighbour, so the result is deterministic (a vertex where two loops touch appears in both)."""
    f = torch.as_tensor(faces).detach().cpu().to(torch.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return []
    table = EdgeTable(f, int(f.max()) + 1 if V is None else V)
    nbrs = {}
    for a, b in table.edges[table.boundary_edge].tolist():
        nbrs.setdefault(a, []).append(b)
        nbrs.setdefault(b, []).append(a)
    for k in nbrs:
        nbrs[k].sort()
    used = set()

    def step(cur):
        for n in nbrs[cur]:
            if (min(cur, n), max(cur, n)) not in used:
                return n
        return None

    loops = []
    for start in sorted(nbrs):
        while step(start) is not None:
            loop, cur = [start], start
            while True:
                n = step(cur)
                if n is None:
                    break
                used.add((min(cur, n), max(cur, n)))
                if n == start:
                    break
                loop.append(n)
                cur = n
            loops.append(loop)
    return loops


def compact(verts, faces):
    """The mesh without the vertices no face uses: (verts', faces', vertex_map [V] int64: old -> new, -1: dropped).  Kept
    rows stay in their order and are copied bit for bit."""
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[faces.reshape(-1)] = True
    vertex_map = torch.where(used, torch.cumsum(used.long(), 0) - 1, -1)
    return verts[used], vertex_map[faces], vertex_map
