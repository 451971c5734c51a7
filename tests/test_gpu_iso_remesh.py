"""Iso-remesh on the GPU: recmv_closest_point against an f64 brute force (random points, points on vertices and on edges of
a 40962-vertex icosphere), recmv_iso_relax and recmv_loop_subdivide against their torch restatements, the kernel route of
isotropic_remesh against the mesh invariants and the torch route, and register_fl.py --iso-remesh end to end."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from recmv import iso_remesh as IR  # noqa: E402
from recmv import nricp as K  # noqa: E402
from test_iso_remesh_cpu import check_remesh, stretched_sphere  # noqa: E402
from test_lap_align_cpu import cut_sphere  # noqa: E402
from test_nricp_cpu import icosphere  # noqa: E402

DEV = "cuda:0"


def brute_force_top2(p, v, f, rows=32):
    """f64 closest-point distances: (best d^2, its lowest face id, second-best d^2 over the other faces)."""
    a = v[f[:, 0]]
    ab, ac = v[f[:, 1]] - a, v[f[:, 2]] - a
    best, idx, second = [], [], []
    for s in range(0, p.shape[0], rows):
        _, _, d = IR._closest_st(p[s:s + rows, None], a[None], ab[None], ac[None])
        i = d.argmin(1)                                                    # the first minimum: the lowest face id
        b = d.gather(1, i[:, None])[:, 0]
        d2 = d.scatter(1, i[:, None], float("inf"))
        best.append(b)
        idx.append(i)
        second.append(d2.min(1)[0])
    return torch.cat(best), torch.cat(idx), torch.cat(second)


def test_closest_point_matches_an_f64_brute_force():
    v, f = icosphere(6)                                                    # 40962 vertices, 81920 faces
    v, f = v.to(DEV), f.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    n = 1500
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=1)
    r = 0.7 + 0.28 * torch.rand(n, 1, device=DEV, generator=g)
    r = torch.where(torch.rand(n, 1, device=DEV, generator=g) < 0.5, r, 2.0 - r)   # 0.7..0.98 and 1.02..1.3
    on_v = v[torch.randint(0, v.shape[0], (400,), device=DEV, generator=g)]
    e, _ = K.edges_packed(f, v.shape[0])
    e = e[torch.randint(0, e.shape[0], (400,), device=DEV, generator=g)]
    on_e = (v[e[:, 0]] + v[e[:, 1]]) * 0.5
    p = torch.cat([dirs * r, on_v, on_e]).contiguous()
    face, point, d2 = IR.closest_point(p, v, f)
    face2, point2, d22 = IR.closest_point(p, v, f)
    assert torch.equal(face, face2) and torch.equal(point, point2) and torch.equal(d2, d22)
    best, idx, second = brute_force_top2(p.double(), v.double(), f)
    tol = 1e-6 * best + 1e-12
    assert ((d2.double() - best).abs() <= tol).all(), (d2.double() - best).abs().max()
    unique = second > best + 2 * tol
    assert unique[:n].float().mean() > 0.5                                 # many project onto an edge or vertex
    assert torch.equal(face[unique], idx[unique])
    exact = on_v.shape[0]
    assert (best[n:n + exact] == 0).all() and (d2[n:n + exact] == 0).all()
    assert torch.equal(face[n:n + exact], idx[n:n + exact])               # exact ties: the lowest face id
    # the returned point is on the returned face, at the returned distance
    assert ((point - p).pow(2).sum(1).double() - d2.double()).abs().max() < 1e-6
    # the reference restatement agrees on a smaller set in f32
    fi, pt, dd = IR.closest_point_torch(p[:200], v, f)
    assert ((dd.double() - best[:200]).abs() <= 1e-5 * best[:200] + 1e-10).all()


def _mesh_case():
    v, f = cut_sphere(5)
    g = torch.Generator().manual_seed(1)
    v = (v + 0.003 * torch.randn(v.shape, generator=g)).to(DEV)
    return v.contiguous(), f.to(DEV)


def test_iso_relax_matches_its_restatement():
    v, f = _mesh_case()
    diag = float((v.max(0)[0] - v.min(0)[0]).norm())
    edges, _ = K.edges_packed(f, v.shape[0])
    nbr = K.neighbours_csr(edges, v.shape[0])
    n = K.verts_normals(v, f)
    fixed = K.mesh_boundary(f, v.shape[0]) | (torch.arange(v.shape[0], device=DEV) % 7 == 0)
    out = IR.iso_relax(v, n, fixed, nbr)
    assert torch.equal(out, IR.iso_relax(v, n, fixed, nbr))
    ref = IR.iso_relax_torch(v.double(), n.double(), fixed, nbr)
    assert (out.double() - ref).abs().max() <= 1e-6 * diag
    assert torch.equal(out[fixed], v[fixed]) and not torch.equal(out[~fixed], v[~fixed])


def test_loop_subdivide_kernel_matches_its_restatement():
    v, f = _mesh_case()
    diag = float((v.max(0)[0] - v.min(0)[0]).norm())
    nv, nf = IR.loop_subdivide(v, f, levels=2, use_kernels=True)
    nv2, nf2 = IR.loop_subdivide(v, f, levels=2, use_kernels=True)
    assert torch.equal(nv, nv2) and torch.equal(nf, nf2)
    rv, rf = IR.loop_subdivide(v.double(), f, levels=2, use_kernels=False)
    assert torch.equal(nf, rf) and torch.equal(nf.cpu(), K.edge_subdivide(*K.edge_subdivide(v.cpu(), f.cpu()))[1])
    assert nv.dtype == torch.float32 and (nv.double() - rv).abs().max() <= 1e-6 * diag


@pytest.mark.parametrize("case", ["stretched", "cut_sphere"])
def test_isotropic_remesh_kernel_route(case):
    v0, f0 = stretched_sphere(3) if case == "stretched" else cut_sphere(4)
    L = 0.06 if case == "stretched" else 0.04
    v0, f0 = v0.to(DEV), f0.to(DEV)
    logs = []
    v, f, stats = IR.isotropic_remesh(v0, f0, target_len=L, use_kernels=True, log=logs.append)
    assert len(logs) == 3 and all(s.startswith("iso-remesh ") for s in logs)
    check_remesh(v0, f0, v, f, L, L)
    v2, f2, stats2 = IR.isotropic_remesh(v0, f0, target_len=L, use_kernels=True)
    assert torch.equal(v, v2) and torch.equal(f, f2) and stats == stats2
    vt, ft, _ = IR.isotropic_remesh(v0, f0, target_len=L, use_kernels=False)
    assert abs(vt.shape[0] - v.shape[0]) <= 0.01 * vt.shape[0]
    assert abs(ft.shape[0] - f.shape[0]) <= 0.01 * ft.shape[0]


def test_register_fl_iso_remesh_end_to_end(tmp_path):
    from recmv import utils
    env = dict(os.environ)
    subprocess.run([sys.executable, str(REPO / "tools" / "make_infer_run.py"), str(tmp_path / "iso"), "--size", "128"],
                   check=True, timeout=600, env=env)
    shutil.copytree(tmp_path / "iso", tmp_path / "plain")
    runs = {tag: str(tmp_path / tag / "capture" / "result") for tag in ("plain", "iso")}
    tv, tf = icosphere(2)
    tv = tv * 0.3
    tpl = str(tmp_path / "template.obj")
    utils.write_obj(tpl, tv, tf)
    import capture_fixture as cf
    from recmv.utils.constant import TEMPLATE_GARMENT
    names = TEMPLATE_GARMENT[cf.GARMENT_TYPE]

    def cmd(run):
        c = [sys.executable, str(REPO / "rec-mv_amd" / "register_fl.py"), "--gpu-ids", "0", "--rec-root", run,
             "--data-type", "scene", "--fit-epochs", "3", "--refine-epochs", "2", "--inner-iter", "10", "--dense-pcl", "600"]
        for n in names:
            c += ["--template", "%s=%s" % (n, tpl)]
        return c
    out = subprocess.run(cmd(runs["plain"]), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "iso-remesh" not in out.stdout
    out = subprocess.run(cmd(runs["iso"]) + ["--iso-remesh", "--iso-remesh-iters", "2", "--iso-remesh-len", "0.03"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("iso-remesh 2/2:") == len(names) and "NRICP avg_update" in out.stdout
    for n in names:
        v, f = utils.read_obj(os.path.join(runs["iso"], "registry_%s.obj" % n))
        vp, fp = utils.read_obj(os.path.join(runs["plain"], "registry_%s.obj" % n))
        assert torch.isfinite(v).all() and v.shape[0] != vp.shape[0]
        f = f.long()
        V = v.shape[0]
        d = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert torch.unique(d[:, 0] * V + d[:, 1]).numel() == d.shape[0]
        u = torch.sort(d, 1)[0]
        assert torch.unique(u[:, 0] * V + u[:, 1], return_counts=True)[1].max() <= 2
        assert V - K.edges_packed(f, V)[0].shape[0] + f.shape[0] == 2          # still a sphere
    out3 = subprocess.run([sys.executable, str(REPO / "rec-mv_amd" / "infer_fl.py"), "--gpu-ids", "0", "--rec-root",
                           runs["iso"], "--data-type", "scene", "--frames", "2", "--registry", "--nColor"],
                          capture_output=True, text=True, timeout=600, env=env)
    assert out3.returncode == 0, out3.stdout[-3000:] + out3.stderr[-3000:]
    for fid in (0, 1, 2):
        for n in names:
            v, f = utils.read_obj(os.path.join(runs["iso"], "meshs/%s_%06d.obj" % (n, fid)))
            reg_v, reg_f = utils.read_obj(os.path.join(runs["iso"], "registry_%s.obj" % n))
            assert v.shape[0] == reg_v.shape[0] and torch.equal(f, reg_f)
        assert os.path.getsize(os.path.join(runs["iso"], "render/%06d.png" % fid)) > 0
