"""NR-ICP registration without a GPU: mesh topology helpers, the plain-torch Laplacian term, a CPU fit, the argument checks of
the new C entry points and the command lines of register_fl.py / infer_fl.py --registry."""
import ctypes as C
import subprocess
import sys
import time
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))

from recmv import nricp as K  # noqa: E402


def icosphere(level):
    t = (1 + 5 ** .5) / 2
    v = torch.tensor([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                      [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=torch.float32)
    f = torch.tensor([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                      [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                      [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    v = v / v.norm(dim=1, keepdim=True)
    for _ in range(level):
        v, f = K.edge_subdivide(v, f)
        v = v / v.norm(dim=1, keepdim=True)
    return v, f


# two triangles sharing the edge (1,2)
SQUARE_V = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=torch.float32)
SQUARE_F = torch.tensor([[0, 1, 2], [1, 3, 2]])


def _normal(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return torch.cross(b - a, c - a, dim=1)


def test_edges_packed_are_unique_sorted_and_map_faces():
    edges, f2e = K.edges_packed(SQUARE_F, 4)
    assert edges.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    # column k of face_to_edge: the edge opposite corner k
    for f, fe in zip(SQUARE_F.tolist(), f2e.tolist()):
        for k in range(3):
            assert sorted(edges[fe[k]].tolist()) == sorted([f[(k + 1) % 3], f[(k + 2) % 3]])
    v, f = icosphere(1)
    e, _ = K.edges_packed(f, v.shape[0])
    assert e.shape[0] == 3 * f.shape[0] // 2 and (e[:, 0] < e[:, 1]).all()
    h = e[:, 0] * v.shape[0] + e[:, 1]
    assert (h[1:] > h[:-1]).all()


def test_mesh_boundary():
    assert K.mesh_boundary(SQUARE_F, 4).tolist() == [True] * 4
    v, f = icosphere(1)
    assert not K.mesh_boundary(f, v.shape[0]).any()
    # a 3x3 grid of vertices: only the centre is interior
    g = torch.tensor([[0, 1, 4], [0, 4, 3], [1, 2, 5], [1, 5, 4], [3, 4, 7], [3, 7, 6], [4, 5, 8], [4, 8, 7]])
    assert K.mesh_boundary(g, 9).tolist() == [True] * 4 + [False] + [True] * 4


def test_edge_subdivision_counts_and_orientation():
    v, f = icosphere(1)
    V, F = v.shape[0], f.shape[0]
    E = K.edges_packed(f, V)[0].shape[0]
    v2, f2 = K.edge_subdivide(v, f)
    assert v2.shape == (V + E, 3) and f2.shape == (4 * F, 3)
    assert torch.equal(v2[:V], v)
    # every child face points the way its parent does (the corner faces and the centre face)
    parent = _normal(v, f).repeat(4, 1)
    assert ((_normal(v2, f2) * parent).sum(1) > 0).all()
    # the midpoints
    e, _ = K.edges_packed(f, V)
    assert torch.allclose(v2[V:], (v[e[:, 0]] + v[e[:, 1]]) / 2)
    v3, f3 = K.densify(v, f, V + 1)
    assert v3.shape[0] == V + E
    v4, _ = K.densify(v, f, V)
    assert v4.shape[0] == V


def test_csr_lists():
    edges, _ = K.edges_packed(SQUARE_F, 5)                       # vertex 4 isolated
    off, inc = K.incident_edges_csr(edges, 5)
    assert off.tolist() == [0, 2, 5, 8, 10, 10] and off.dtype == torch.int32
    assert inc.tolist() == [0, 1, 0, 2, 3, 1, 2, 4, 3, 4]
    off, nbr = K.neighbours_csr(edges, 5)
    assert off.tolist() == [0, 2, 5, 8, 10, 10]
    assert nbr.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]


def test_laplacian_term_matches_dense_matrix_with_an_isolated_vertex():
    torch.manual_seed(0)
    v, f = icosphere(1)
    V = v.shape[0]
    verts = torch.cat([v + 0.05 * torch.randn_like(v), torch.tensor([[2., 0.5, -1.]])]).double()   # vertex V: isolated
    edges, _ = K.edges_packed(f, V + 1)
    A = torch.zeros(V + 1, V + 1, dtype=torch.float64)
    A[edges[:, 0], edges[:, 1]] = 1
    A[edges[:, 1], edges[:, 0]] = 1
    deg = A.sum(1)
    Lm = A / torch.where(deg > 0, deg, torch.ones_like(deg))[:, None] - torch.eye(V + 1, dtype=torch.float64)
    x = verts.clone().requires_grad_(True)
    got = K.laplacian_smoothing_torch(x, edges)
    want = (Lm @ verts).norm(dim=1).mean()
    assert torch.allclose(got, want, rtol=1e-12)
    got.backward()
    y = verts.clone().requires_grad_(True)
    (Lm @ y).norm(dim=1).mean().backward()
    assert torch.allclose(x.grad, y.grad, rtol=1e-10, atol=1e-12)
    # a zero row has a zero gradient
    flat = torch.zeros(V + 1, 3, dtype=torch.float64, requires_grad=True)
    K.laplacian_smoothing_torch(flat, edges).backward()
    assert torch.equal(flat.grad, torch.zeros_like(flat))


def test_cpu_fit_pulls_a_sphere_onto_a_wobbled_sphere():
    from recmv.engineer.optimizer import NRICP_Optimizer_AdamW, TriMesh
    tv, tf = icosphere(2)
    gv, gf = icosphere(4)
    gv = gv * 1.05 + 0.01 * torch.stack([torch.sin(3 * gv[:, 1]), torch.cos(2 * gv[:, 0]), torch.sin(4 * gv[:, 2])], -1)

    def mean_dist(v):
        return K.knn1_torch(v, gv)[1].sqrt().mean().item()

    t0 = time.time()
    lines = []
    opt = NRICP_Optimizer_AdamW(epoch=8, dense_pcl=0, use_normal=True, stiffness_weight=[5, 1], mile_stone=[4], inner_iter=50,
                                laplacian_weight=[1, 1], threshold=0.3, device='cpu', log=lines.append)
    assert opt.use_kernels is False                              # the CPU always takes the torch path
    loss, mesh = opt(smpl_slice=TriMesh(tv, tf), cano_meshes=TriMesh(gv, gf), save_path=None, garment_name='g',
                     static_pts_type=[], nricp_masks=None)
    assert time.time() - t0 < 60
    assert torch.isfinite(mesh.verts).all() and torch.isfinite(loss)
    assert mean_dist(mesh.verts) * 5 <= mean_dist(tv)
    assert len(lines) == 8 and lines[0].startswith("current 000 NRICP avg_update:") and "valid" in lines[0]
    assert torch.equal(mesh.faces, tf)
    with pytest.raises(NotImplementedError):
        opt(smpl_slice=TriMesh(tv, tf), cano_meshes=TriMesh(gv, gf), static_pts_type=['upper_bottom'], nricp_masks=None)


def test_new_abi_entry_points_reject_bad_arguments():
    from recmv import _lib as L
    lib = L.lib()
    assert lib.recmv_abi_version() == L.ABI_VERSION
    assert {"recmv_knn1", "recmv_knn1_workspace_bytes", "recmv_nricp_energy",
            "recmv_nricp_energy_workspace_bytes"} <= set(L.exported_symbols())
    n = C.c_void_p(0)
    assert lib.recmv_knn1(n, 4, n, 0, n, n, n, 0, n)== -1                # M = 0
    assert b"empty" in lib.recmv_last_error()
    assert lib.recmv_knn1(n, -1, n, 3, n, n, n, 0, n) == -1
    assert lib.recmv_knn1(n, 0, n, 3, n, n, n, 0, n) == 0                # N = 0: no-op
    assert lib.recmv_knn1(n, 4, n, 3, n, n, n, 0, n)== -1                # NULL pointers
    buf = (C.c_byte * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.recmv_knn1(p, 16, p, 3, p, p, p, 8, n)== -1                # workspace too small
    assert b"workspace" in lib.recmv_last_error()
    assert lib.recmv_knn1_workspace_bytes(10) == 80
    args = [p] * 8 + [5] + [p] * 4 + [10, 1.0, 1.0, 1.0, 0.5] + [p] * 4 + [p, 0, n]
    assert lib.recmv_nricp_energy(*args)== -1                              # workspace too small
    bad = list(args)
    bad[13] = 0
    assert lib.recmv_nricp_energy(*bad)== -1                               # N = 0
    bad = list(args)
    bad[0] = n
    assert lib.recmv_nricp_energy(*bad)== -1                               # NULL
    assert lib.recmv_nricp_energy_workspace_bytes(0) == 0 < lib.recmv_nricp_energy_workspace_bytes(10)


def test_knn1_wrapper_checks_inputs_without_a_gpu():
    with pytest.raises(RuntimeError):
        K.knn1(torch.zeros(3, 3), torch.zeros(2, 3))                     # CPU tensors are refused, no fallback


def test_register_fl_help_and_infer_fl_registry_flag_parse():
    out = subprocess.run([sys.executable, str(REPO / "rec-mv_amd" / "register_fl.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "--template" in out.stdout and "--rec-root" in out.stdout
    import importlib.util
    spec = importlib.util.spec_from_file_location("infer_fl", REPO / "rec-mv_amd" / "infer_fl.py")
    infer_fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(infer_fl)
    a = infer_fl.build_parser().parse_args(['--rec-root', 'x', '--registry'])
    assert a.registry is True
    assert infer_fl.build_parser().parse_args(['--rec-root', 'x']).registry is False
