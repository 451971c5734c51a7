"""Iso-remesh (isotropic remeshing) and Loop subdivision without a GPU: the torch route of recmv.iso_remesh against an
independently assembled Loop matrix and the mesh invariants of a remesh, argument checks of the new C entry points and
the register_fl.py flags."""
import ctypes as C
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from recmv import iso_remesh as IR  # noqa: E402
from recmv import lap_align as LA  # noqa: E402
from recmv import nricp as K  # noqa: E402
from test_lap_align_cpu import cut_sphere  # noqa: E402
from test_nricp_cpu import icosphere  # noqa: E402


def stretched_sphere(level):
    v, f = icosphere(level)
    return (v * torch.tensor([3., 1., 1.])).contiguous(), f


def loop_matrix(faces, V):
    """Loop's subdivision matrix S [V + E, V] (f64), assembled from python sets: new = S old."""
    faces = faces.tolist()
    opp = {}
    for a, b, c in faces:
        for u, w, o in ((a, b, c), (b, c, a), (c, a, b)):
            opp.setdefault((min(u, w), max(u, w)), []).append(o)
    edges = sorted(opp)
    nbrs = [set() for _ in range(V)]
    bnbrs = [set() for _ in range(V)]
    for (u, w), o in opp.items():
        nbrs[u].add(w)
        nbrs[w].add(u)
        if len(o) == 1:
            bnbrs[u].add(w)
            bnbrs[w].add(u)
    S = np.zeros((V + len(edges), V))
    for i in range(V):
        if bnbrs[i]:
            S[i, i] = 0.75
            for j in bnbrs[i]:
                S[i, j] += 0.125
        else:
            n = len(nbrs[i])
            beta = (5. / 8. - (3. / 8. + 0.25 * math.cos(2 * math.pi / n)) ** 2) / n
            S[i, i] = 1 - n * beta
            for j in nbrs[i]:
                S[i, j] += beta
    for k, (u, w) in enumerate(edges):
        o = opp[(u, w)]
        if len(o) == 2:
            S[V + k, u] += 3. / 8.
            S[V + k, w] += 3. / 8.
            S[V + k, o[0]] += 1. / 8.
            S[V + k, o[1]] += 1. / 8.
        else:
            S[V + k, u] += 0.5
            S[V + k, w] += 0.5
    return S


@pytest.mark.parametrize("mesh", ["icosphere", "cut_sphere"])
def test_loop_subdivide_matches_the_subdivision_matrix(mesh):
    v, f = icosphere(2) if mesh == "icosphere" else cut_sphere(3)
    v = v.double() + 0.01 * torch.randn(v.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    nv, nf = IR.loop_subdivide(v, f, levels=1, use_kernels=False)
    assert torch.equal(nf, K.edge_subdivide(v, f)[1])
    S = loop_matrix(f, v.shape[0])
    assert nv.dtype == torch.float64 and nv.shape[0] == S.shape[0]
    np.testing.assert_allclose(nv.numpy(), S @ v.numpy(), rtol=0, atol=1e-12)
    # two levels: the faces of two edge subdivisions
    nv2, nf2 = IR.loop_subdivide(v, f, levels=2, use_kernels=False)
    assert torch.equal(nf2, K.edge_subdivide(*K.edge_subdivide(v, f))[1])
    np.testing.assert_allclose(nv2.numpy(), loop_matrix(nf, S.shape[0]) @ (S @ v.numpy()), rtol=0, atol=1e-12)


def test_loop_subdivide_keeps_a_planar_patch_planar():
    v, f = cut_sphere(3)
    v = v.double()
    v[:, 2] = 0.25 * v[:, 0] - 0.5 * v[:, 1] + 0.1                        # a plane z = 0.25 x - 0.5 y + 0.1
    nv, _ = IR.loop_subdivide(v, f, levels=2, use_kernels=False)
    assert (nv[:, 2] - (0.25 * nv[:, 0] - 0.5 * nv[:, 1] + 0.1)).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------- iso-remesh
def seg_dist(p, a, b):
    """Distance of every row of p to the nearest of the segments (a, b) (f64)."""
    ab = b - a
    t = (((p[:, None] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1)[None]).clamp(0, 1)
    q = a[None] + t[..., None] * ab[None]
    return ((q - p[:, None]) ** 2).sum(-1).min(1)[0].sqrt()


def check_remesh(v0, f0, v, f, L, max_d):
    """The invariants of a remesh of (v0, f0) with target length L: see the assertions."""
    v0d, vd = v0.double().cpu(), v.double().cpu()
    f0, f = f0.cpu(), f.cpu()
    V = v.shape[0]
    diag = float((v0d.max(0)[0] - v0d.min(0)[0]).norm())
    # an oriented 2-manifold: every directed edge once, every undirected edge in one or two faces
    d = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert torch.unique(d[:, 0] * V + d[:, 1]).numel() == d.shape[0]
    u = torch.sort(d, 1)[0]
    _, cnt = torch.unique(u[:, 0] * V + u[:, 1], return_counts=True)
    assert cnt.max() <= 2
    assert torch.unique(f).numel() == V                                      # no unreferenced vertex
    # no (near-)degenerate face
    a = vd[f[:, 0]]
    area = 0.5 * torch.cross(vd[f[:, 1]] - a, vd[f[:, 2]] - a, dim=1).norm(dim=1)
    assert area.min() > 1e-12 * diag * diag
    # the topology is kept: Euler characteristic and boundary loops

    def euler(vv, ff):
        return vv.shape[0] - K.edges_packed(ff, vv.shape[0])[0].shape[0] + ff.shape[0]
    assert euler(vd, f) == euler(v0d, f0)
    loops0, loops = LA.boundary_loops(f0, v0.shape[0]), LA.boundary_loops(f, V)
    assert len(loops) == len(loops0)
    # boundary vertices lie on the input's boundary polyline
    if loops0:
        seg = np.array([[lp[i], lp[(i + 1) % len(lp)]] for lp in loops0 for i in range(len(lp))])
        bv = torch.tensor(sorted({i for lp in loops for i in lp}))
        assert seg_dist(vd[bv], v0d[seg[:, 0]], v0d[seg[:, 1]]).max() <= 1e-6 * diag
    # every vertex within max_d of the input surface
    _, _, d2 = IR.closest_point_torch(vd, v0d, f0)
    assert d2.max().sqrt() <= max_d
    # isotropic edges
    e = K.edges_packed(f, V)[0]
    el = (vd[e[:, 0]] - vd[e[:, 1]]).norm(dim=1) / L
    assert ((el >= 0.5) & (el <= 1.5)).double().mean() >= 0.95, el


def valence_dev(v, f):
    topo = IR._Topo(f, v.shape[0])
    return float(IR._valence_dev(topo).double().mean())


CASES = {"stretched": (lambda: stretched_sphere(2), 0.1), "cut_sphere": (lambda: cut_sphere(3), 0.06)}


@pytest.fixture(scope="module", params=sorted(CASES))
def remeshed(request):
    make, L = CASES[request.param]
    v0, f0 = make()
    v, f, stats = IR.isotropic_remesh(v0, f0, target_len=L, use_kernels=False)
    return request.param, v0, f0, v, f, stats, L


def test_isotropic_remesh_invariants(remeshed):
    name, v0, f0, v, f, stats, L = remeshed
    check_remesh(v0, f0, v, f, L, L)
    assert len(stats) == 3
    for st in stats:
        assert {"V", "F", "splits", "collapses", "flips", "edge_min", "edge_mean", "edge_max", "max_dist"} <= set(st)
        # the flip step lowers the mean |valence - target| of what split and collapse left
        assert st["valence_dev"] <= st["valence_dev_pre_flip"]
        assert st["flips"] == 0 or st["valence_dev"] < st["valence_dev_pre_flip"]
    assert stats[-1]["V"] == v.shape[0] and stats[-1]["F"] == f.shape[0]
    assert stats[0]["splits"] > 0 and stats[0]["collapses"] > 0 and stats[0]["flips"] > 0


def test_isotropic_remesh_lowers_the_valence_deviation_of_an_irregular_mesh():
    # an icosahedron: every vertex has valence 5, so the input deviates by 1 everywhere
    v0, f0 = stretched_sphere(0)
    v, f, _ = IR.isotropic_remesh(v0, f0, target_len=0.3, use_kernels=False)
    check_remesh(v0, f0, v, f, 0.3, 0.3)
    assert valence_dev(v, f) < valence_dev(v0, f0)


def test_isotropic_remesh_is_bit_identical_over_two_runs(remeshed):
    name, v0, f0, v, f, stats, L = remeshed
    v2, f2, stats2 = IR.isotropic_remesh(v0, f0, target_len=L, use_kernels=False)
    assert torch.equal(v, v2) and torch.equal(f, f2) and stats == stats2


def cube(level):
    """A closed cube [-1,1]^3 of 12 triangles, edge-subdivided `level` times (all vertices on the surface)."""
    v = torch.tensor([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [[a, b, c], [a, c, d]]
    f = torch.tensor(f)
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    f = torch.where(((n * v[f].mean(1)).sum(1) < 0)[:, None], f[:, [0, 2, 1]], f)      # outward
    for _ in range(level):
        v, f = K.edge_subdivide(v, f)
    return v, f


def test_isotropic_remesh_keeps_the_creases_of_a_cube():
    v0, f0 = cube(2)
    L = 0.25
    v, f, _ = IR.isotropic_remesh(v0, f0, target_len=L, feature_deg=30., use_kernels=False)
    check_remesh(v0, f0, v, f, L, L)
    assert (v.abs().max(1)[0] - 1).abs().max() < 1e-5                      # on the cube's surface
    corners = torch.tensor([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)])
    assert torch.cdist(corners, v).min(1)[0].max() == 0                      # the corners stay vertices
    # the crease edges: every dihedral angle above 30 degrees lies on a cube edge, and they cover all 12 edges
    topo = IR._Topo(f, v.shape[0])
    crease, _ = IR._fixed(v, f, topo, math.cos(math.radians(30.)))
    ce = topo.edges[crease]
    on_edge = ((v[ce].abs() > 1 - 1e-6).sum(-1) >= 2).all(1)
    assert on_edge.all()
    length = (v[ce[:, 0]] - v[ce[:, 1]]).norm(dim=1).sum()
    assert abs(float(length) - 12 * 2.) < 1e-4


def test_new_abi_entry_points_reject_bad_arguments():
    from recmv import _lib as L
    lib = L.lib()
    assert lib.recmv_abi_version() == L.ABI_VERSION == 11
    assert {"recmv_closest_point", "recmv_closest_point_workspace_bytes", "recmv_iso_relax",
            "recmv_loop_subdivide"} <= set(L.exported_symbols())
    n = C.c_void_p(0)
    buf = (C.c_byte * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.recmv_closest_point(n, 4, n, 3, n, 0, n, n, n, n, 0, n) == -1          # F = 0
    assert b"empty" in lib.recmv_last_error()
    assert lib.recmv_closest_point(n, -1, n, 3, n, 1, n, n, n, n, 0, n) == -1
    assert lib.recmv_closest_point(n, 0, n, 3, n, 1, n, n, n, n, 0, n) == 0           # P = 0: no-op
    assert lib.recmv_closest_point(n, 4, n, 3, n, 1, n, n, n, n, 0, n) == -1          # NULL pointers
    assert lib.recmv_closest_point(p, 16, p, 3, p, 1, p, p, p, p, 8, n) == -1         # workspace too small
    assert b"workspace" in lib.recmv_last_error()
    assert lib.recmv_closest_point_workspace_bytes(10) == 80
    assert lib.recmv_closest_point_workspace_bytes(0) == 0
    assert lib.recmv_iso_relax(p, p, -1, 0, p, p, p, p, n) == -1                       # V < 0
    assert lib.recmv_iso_relax(n, n, 0, 0, n, n, n, n, n) == 0                         # V = 0: no-op
    assert lib.recmv_iso_relax(p, n, 4, 6, p, p, p, p, n) == -1                        # NULL neighbour list
    assert lib.recmv_iso_relax(p, p, 4, 6, p, p, p, p, n) == -1                        # out aliases verts
    assert b"alias" in lib.recmv_last_error()
    q = C.cast(C.byref(buf, 32), C.c_void_p)
    assert lib.recmv_loop_subdivide(p, p, 4, 6, p, p, n, 3, q, n) == -1               # NULL edge table
    assert lib.recmv_loop_subdivide(p, p, 4, 6, p, p, p, -1, q, n) == -1              # E < 0
    assert lib.recmv_loop_subdivide(p, p, 4, 6, p, p, p, 3, p, n) == -1               # out aliases verts
    assert lib.recmv_loop_subdivide(n, n, 0, 0, n, n, n, 0, n, n) == 0                 # empty: no-op


def test_kernel_wrappers_refuse_cpu_tensors():
    v, f = icosphere(1)
    with pytest.raises(RuntimeError):
        IR.closest_point(v, v, f)
    with pytest.raises(RuntimeError):
        IR.isotropic_remesh(v, f, use_kernels=True)
    with pytest.raises(RuntimeError):
        IR.loop_subdivide(v, f, use_kernels=True)


def test_register_fl_iso_remesh_flags():
    script = str(REPO / "rec-mv_amd" / "register_fl.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--iso-remesh", "--iso-remesh-iters", "--iso-remesh-len", "--iso-remesh-subdiv"):
        assert flag in out.stdout
    out = subprocess.run([sys.executable, script, "--gpu-ids", "0", "--rec-root", "/nonexistent", "--iso-remesh-iters",
                          "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--iso-remesh-iters needs --iso-remesh" in out.stderr
