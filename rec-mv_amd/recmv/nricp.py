"""Non-rigid ICP building blocks: the HIP kernels of csrc/nricp.hip, their plain-torch restatements and the mesh helpers of a
fit.  The edge tables (edges_packed, the CSR lists, the boundary) are recmv.connectivity's; their names stay importable here.

  mesh_boundary       engineer/utils/mesh_utils.py:88 (vertices of edges used by one face)
  edge_subdivide      Garment_Mesh.__edge_dense_pcl (engineer/utils/garment_structure.py:989-1030) without colour labels
Kernels: knn1 (pytorch3d knn_points K=1 + knn_gather) and nricp_energy (one inner iteration of NRICP_Optimizer_AdamW,
forward and gradient).  `knn1_torch` and `laplacian_smoothing_torch` are the restatements the torch path and the tests use.
"""
import torch

from . import _lib as L
from .connectivity import EdgeTable, edges_packed, incident_edges_csr, neighbours_csr  # noqa: F401  (callers say K.edges_packed)
from .mesh_args import check_points


class TriMesh:
    """A triangle mesh: verts [V,3] float32, faces [F,3] int64 on one device."""

    def __init__(self, verts, faces):
        self.verts = verts
        self.faces = faces

    def to(self, device):
        return TriMesh(self.verts.to(device), self.faces.to(device))

    def verts_normals(self):
        return verts_normals(self.verts, self.faces)


# ------------------------------------------------------------------------------------------------- topology
def mesh_boundary(faces, V):
    """bool [V]: True on a vertex of an edge that only one face uses (engineer/utils/mesh_utils.py:88-116)."""
    return EdgeTable(faces, V).boundary_vertex


def edge_subdivide(verts, faces):
    """One edge subdivision (V + E vertices, 4F faces, orientation kept): a midpoint per edge, three corner faces and
    the centre face, in the reference's order."""
    V = verts.shape[0]
    edges, f2e = edges_packed(faces, V)
    mid = verts[edges].mean(1)
    fe = f2e + V
    f0 = torch.stack([fe[:, 0], faces[:, 2], fe[:, 1]], -1)
    f1 = torch.stack([fe[:, 1], faces[:, 0], fe[:, 2]], -1)
    f2 = torch.stack([fe[:, 2], faces[:, 1], fe[:, 0]], -1)
    return torch.cat([verts, mid], 0), torch.cat([f0, f1, f2, fe], 0)


def densify(verts, faces, dense_pcl):
    """Subdivide until there are at least `dense_pcl` vertices (nricp_optimizer.py:290-291)."""
    while verts.shape[0] < dense_pcl:
        verts, faces = edge_subdivide(verts, faces)
    return verts, faces


def laplacian_smoothing_torch(verts, edges):
    """pytorch3d `mesh_laplacian_smoothing(method="uniform")` of one mesh: mean_i |(1/deg_i) sum_{j in N(i)} v_j - v_i|
    (an isolated vertex's row is -v_i), differentiable in `verts`."""
    V = verts.shape[0]
    e0, e1 = edges[:, 0], edges[:, 1]
    ones = torch.ones(e0.shape[0], dtype=verts.dtype, device=verts.device)
    deg = torch.zeros(V, dtype=verts.dtype, device=verts.device).index_add(0, e0, ones).index_add(0, e1, ones)
    inv = torch.where(deg > 0, 1. / deg.clamp(min=1.), deg)
    s = torch.zeros_like(verts).index_add(0, e0, verts[e1] * inv[e0, None]).index_add(0, e1, verts[e0] * inv[e1, None])
    return (s - verts).norm(dim=1).mean()


def verts_normals(verts, faces):
    """pytorch3d vertex normals of one mesh [V,3]: the HIP kernel on the GPU, its restatement on the CPU."""
    if verts.is_cuda:
        from . import shading
        return shading.verts_normals(verts.contiguous(), faces.contiguous())
    n = torch.zeros_like(verts)
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = n.index_add(0, faces[:, 1], torch.cross(v2 - v1, v0 - v1, dim=1))
    n = n.index_add(0, faces[:, 2], torch.cross(v0 - v2, v1 - v2, dim=1))
    n = n.index_add(0, faces[:, 0], torch.cross(v1 - v0, v2 - v0, dim=1))
    return torch.nn.functional.normalize(n, eps=1e-6, dim=1)


# ------------------------------------------------------------------------------------------------- kernels
def knn1(p, q):
    """Exact 1-NN of every row of p [N,3] among q [M,3] (float32 CUDA): (idx [N] int64, squared distance [N] f32);
    ties go to the lowest index of q."""
    p, q = check_points(p, "p"), check_points(q, "q")
    if q.shape[0] == 0:
        raise ValueError("knn1: the target cloud is empty")
    N, dev = p.shape[0], p.device
    idx = L.scratch((N,), torch.int64, dev)
    dist = L.scratch((N,), torch.float32, dev)
    if N == 0:
        return idx, dist
    ws = L.workspace(nbytes := int(L.lib().recmv_knn1_workspace_bytes(N)), dev, "knn1_workspace_bytes")
    L.launch("knn1", dev, L.ptr(p), N, L.ptr(q), q.shape[0], L.ptr(idx), L.ptr(dist), L.ptr(ws), nbytes)
    return idx, dist


def knn1_torch(p, q, chunk_elems=1 << 24):
    """knn1 in plain torch (row chunks of a brute-force distance matrix; argmin keeps the first minimum)."""
    rows = max(1, chunk_elems // max(q.shape[0], 1))
    idx, dist = [], []
    for s in range(0, p.shape[0], rows):
        d = ((p[s:s + rows, None, :] - q[None, :, :]) ** 2).sum(-1)
        i = d.argmin(dim=1)
        m = d.gather(1, i[:, None])[:, 0]
        idx.append(i)
        dist.append(m)
    if not idx:
        return torch.zeros(0, dtype=torch.int64, device=p.device), torch.zeros(0, dtype=p.dtype, device=p.device)
    return torch.cat(idx), torch.cat(dist)


class EnergyTopology:
    """The per-fit lists recmv_nricp_energy reads: edges, incident-edge and neighbour CSR lists, interior mask."""

    def __init__(self, faces, V, device):
        table = EdgeTable(faces.to(device=device, dtype=torch.int64), V)
        self.V = V
        self.edges = table.edges.contiguous()
        self.interior = torch.logical_not(table.boundary_vertex)
        self.inc = incident_edges_csr(self.edges, V)
        self.nbr = neighbours_csr(self.edges, V)


class NricpEnergy:
    """recmv_nricp_energy with its buffers: `__call__(A, b, x, c, nc, nx, gamma, sw, lw, threshold)` writes the gradients
    into `self.dA` [N,3,3] / `self.db` [N,3] and returns (scalars [4] = loss, vert_sum, stiff_sum, lap on the device,
    weight mask [N] uint8), both buffers of this object that the next call overwrites."""

    def __init__(self, topo, device):
        self.topo = topo
        N = topo.V
        self.N = N
        self.ws = L.workspace(nbytes := int(L.lib().recmv_nricp_energy_workspace_bytes(N)), device, "nricp_energy_workspace_bytes",
                              floor=16)
        self.ws_bytes = nbytes
        self.scalars = L.scratch((4,), torch.float32, device)
        self.mask = L.scratch((N,), torch.uint8, device)
        self.dA = L.scratch((N, 3, 3), torch.float32, device)
        self.db = L.scratch((N, 3), torch.float32, device)
        self.interior = topo.interior.to(torch.uint8).contiguous()

    def __call__(self, A, b, x, c, nc, nx, gamma, stiffness_weight, laplacian_weight, threshold):
        N = self.N
        for t, name in ((A, "A"), (b, "b"), (x, "x"), (c, "c"), (nc, "nc"), (nx, "nx")):
            L.require_cuda(t, name)
            L.require_contiguous(t, name)
            if t.dtype != torch.float32 or t.numel() != (9 if name == "A" else 3) * N:
                raise ValueError("nricp_energy: %s must be float32 with %d rows" % (name, N))
        topo = self.topo
        E = topo.edges.shape[0]
        L.launch("nricp_energy", A.device, L.ptr(A), L.ptr(b), L.ptr(x), L.ptr(c), L.ptr(nc), L.ptr(nx), L.ptr(self.interior),
                 L.ptr(topo.edges), E, L.ptr(topo.inc[0]), L.ptr(topo.inc[1]), L.ptr(topo.nbr[0]), L.ptr(topo.nbr[1]), N,
                 float(gamma), float(stiffness_weight), float(laplacian_weight), float(threshold), L.ptr(self.scalars),
                 L.ptr(self.mask), L.ptr(self.dA), L.ptr(self.db), L.ptr(self.ws), self.ws_bytes)
        return self.scalars, self.mask
